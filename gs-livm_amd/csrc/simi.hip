// simi.hip -- the LiDAR similarity loss of GS-LIVM's optimiser (optimize_vis step 3), fused:
//
//   r = mean(scales[sel])                      one scalar over the 3n selected (activated) scale elements
//   L = lambda / m * sum_i max(min_j |p_i - x_sel[j]| - r, 0)
//
// Reference: GaussianModel::compute_min_distance (src/gs/gaussian.cu:87-114) called from calcSimiLoss (:201-239) at
// src/liw/lioOptimization.cpp:1675 with lambda_depth_simi (config/basic_common.yaml:64).  The reference expands
// m x n x 3 floats several times over, forward and backward; since r is ONE scalar, clamp and min commute and the term
// is a nearest-neighbour search followed by one clamp per point:
//   k_simi_nearest   lane = point, workgroup = 64 points x one chunk of the gathered centres (staged through LDS 256 at
//                    a time, each of the four waves scans a quarter of a tile): per (point, chunk) the smallest squared
//                    distance and its position in `sel`; the workgroups of the first point block also sum their chunk's
//                    scales (f64, fixed order)
//   k_simi_points    thread = point: fixed-order minimum over the chunks, r from the chunk sums, the clamp, and the
//                    point's gradient record (position of its nearest centre or -1, and -lambda/m (p - x)/d);
//                    per-workgroup partial sums of the clamped distances (f64) and counts of points outside r
//   k_simi_grads     thread = selected row: walks the m records in ascending point order and sums those that name it
//                    (several points may share a nearest Gaussian: a deterministic many-to-one accumulation without
//                    atomics); every selected scale element receives dL/dr / (3n); workgroup 0 writes
//                    {loss, mean clamped distance, r}
// No float atomics, every reduction in a fixed order (bitwise reproducible), no host synchronisation, three launches
// on the caller's stream.  Ties (two centres at bit-equal squared distance) go to the lower position in `sel`; a point
// at exactly d == r contributes nothing (the reference leaves both undefined).  m and n are bounded by int only: the
// 500-point cap of the reference (MAX_SIMI, include/gs/gp3d/gp_types.h:15) is the host's policy.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

constexpr int SM_PTS_ = 64;        // points per workgroup of k_simi_nearest (one per lane)
constexpr int SM_TILE_ = 256;      // centres staged per LDS tile (one per thread)
constexpr int SM_TARGET_WGS_ = 1024;  // k_simi_nearest's grid aims at four workgroups on each of the 256 CUs, once
constexpr int SM_REC_TILE_ = 1024;  // records staged per LDS tile of k_simi_grads

struct SimiPlan {
  int pblocks, ntiles, tiles_per_chunk, nchunks, nblocks2;
};

static SimiPlan simi_plan(int m, int n) {
  SimiPlan p;
  p.pblocks = (m + SM_PTS_ - 1) / SM_PTS_;
  p.ntiles = (n + SM_TILE_ - 1) / SM_TILE_;
  // the work is latency-bound at the sizes of the loop (4-16 M distances): as many chunks as fill the device once, no
  // more (every chunk costs each point one partial record)
  int want = SM_TARGET_WGS_ / (p.pblocks > 0 ? p.pblocks : 1);
  if (want < 1) want = 1;
  if (want > p.ntiles) want = p.ntiles;
  if (want < 1) want = 1;
  p.tiles_per_chunk = (p.ntiles + want - 1) / want;
  if (p.tiles_per_chunk < 1) p.tiles_per_chunk = 1;
  p.nchunks = (p.ntiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk;  // (no empty chunk)
  p.nblocks2 = (m + 255) / 256;
  return p;
}

struct SimiWorkspace {
  float* part_d2;    // [nchunks][m] smallest squared distance of the point inside the chunk
  int* part_k;       // [nchunks][m] its position in sel
  double* scale_part;  // [nchunks]
  int* rec_k;        // [m] position in sel of the nearest centre, -1: the point lies inside r
  float* rec_g;      // [m][3] the point's contribution to dL/dxyz of that row
  double* hinge_part;  // [nblocks2]
  int* count_part;   // [nblocks2]
  float* r;          // [1]
  size_t bytes;
  static SimiWorkspace carve(char* base, int m, int n) {
    const SimiPlan p = simi_plan(m, n);
    Carver cv(base);
    SimiWorkspace w;
    w.part_d2 = cv.take<float>((size_t)p.nchunks * m);
    w.part_k = cv.take<int>((size_t)p.nchunks * m);
    w.scale_part = cv.take<double>((size_t)p.nchunks);
    w.rec_k = cv.take<int>((size_t)m);
    w.rec_g = cv.take<float>((size_t)m * 3);
    w.hinge_part = cv.take<double>((size_t)p.nblocks2);
    w.count_part = cv.take<int>((size_t)p.nblocks2);
    w.r = cv.take<float>(1);
    w.bytes = align_up(cv.off) + ALIGN;
    return w;
  }
};

// A row index of `sel` as the kernels use it for READS: clamped into [0, P), so that a selection that breaks its
// contract (each < P) reads a wrong row instead of foreign memory; writes test the unclamped index and are skipped.
__device__ __forceinline__ int clamp_row(int row, int P) { return min(max(row, 0), P - 1); }

__global__ __launch_bounds__(256) void k_simi_nearest(const int P, const int m, const int n, const int tiles_per_chunk,
                                                      const int ntiles, const float* __restrict__ points,
                                                      const int* __restrict__ sel, const float* __restrict__ xyz,
                                                      const float* __restrict__ scaling,
                                                      float* __restrict__ part_d2, int* __restrict__ part_k,
                                                      double* __restrict__ scale_part) {
  __shared__ float4 cs[SM_TILE_];   // one broadcast ds_read_b128 per centre
  __shared__ float wd2[4][SM_PTS_];
  __shared__ int wk[4][SM_PTS_];
  __shared__ double shsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * SM_PTS_ + lane;
  const int ic = min(i, m - 1);
  const float px = points[3 * (size_t)ic], py = points[3 * (size_t)ic + 1], pz = points[3 * (size_t)ic + 2];
  const int t0 = blockIdx.y * tiles_per_chunk, t1 = min(t0 + tiles_per_chunk, ntiles);
  const bool sums = blockIdx.x == 0;  // (uniform over the workgroup)
  float best = __builtin_inff();
  int bestk = -1;
  double ssum = 0.0;
  for (int t = t0; t < t1; t++) {
    const int k = t * SM_TILE_ + (int)threadIdx.x;
    // a slot past the end holds a centre no finite point is near: its squared distance overflows to +inf, which never
    // passes the strict comparison
    float4 c = make_float4(3e38f, 3e38f, 3e38f, 0.f);
    if (k < n) {
      const size_t row = (size_t)clamp_row(sel[k], P);
      c.x = xyz[3 * row]; c.y = xyz[3 * row + 1]; c.z = xyz[3 * row + 2];
      if (sums) ssum += ((double)scaling[3 * row] + (double)scaling[3 * row + 1]) + (double)scaling[3 * row + 2];
    }
    __syncthreads();  // (the previous tile has been scanned)
    cs[threadIdx.x] = c;
    __syncthreads();
    const int j0 = wave * 64;
#pragma unroll 8
    for (int j = 0; j < 64; j++) {
      const float4 q = cs[j0 + j];
      const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
      const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
      if (d2 < best) { best = d2; bestk = t * SM_TILE_ + j0 + j; }  // ascending positions, strict: the lowest wins a tie
    }
  }
  wd2[wave][lane] = best;
  wk[wave][lane] = bestk;
  __syncthreads();
  if (wave == 0 && i < m) {
    float b = wd2[0][lane];
    int bk = wk[0][lane];
#pragma unroll
    for (int w = 1; w < 4; w++) {
      const float d = wd2[w][lane];
      const int kk = wk[w][lane];
      // within a tile the waves scan ascending quarters, but over several tiles wave 0 may hold a LATER position than
      // wave 1: equal distances are settled by the position itself
      if (d < b || (d == b && kk >= 0 && (bk < 0 || kk < bk))) { b = d; bk = kk; }
    }
    const size_t o = (size_t)blockIdx.y * m + i;
    part_d2[o] = b;
    part_k[o] = bk;
  }
  if (sums) {
    const double s = block_sum(ssum, shsum);
    if (threadIdx.x == 0) scale_part[blockIdx.y] = s;
  }
}

__global__ __launch_bounds__(256) void k_simi_points(const int P, const int m, const int n, const int nchunks,
                                                     const float* __restrict__ points, const int* __restrict__ sel,
                                                     const float* __restrict__ xyz,
                                                     const float* __restrict__ part_d2, const int* __restrict__ part_k,
                                                     const double* __restrict__ scale_part, const float lam_over_m,
                                                     int* __restrict__ rec_k, float* __restrict__ rec_g,
                                                     double* __restrict__ hinge_part, int* __restrict__ count_part,
                                                     float* __restrict__ r_out) {
  __shared__ double shsum[4];
  __shared__ int shcnt[4];
  // r: every workgroup sums the chunk sums in the same fixed order (thread-strided, then the workgroup tree)
  const double s = partials_sum(scale_part, nchunks, shsum);
  const float r = (float)(s / (3.0 * (double)n));
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  float hinge = 0.f;
  int active = 0;
  if (i < m) {
    float best = __builtin_inff();
    int bk = -1;
    for (int c = 0; c < nchunks; c++) {  // ascending chunks hold ascending positions: strict, the lowest wins a tie
      const float d = part_d2[(size_t)c * m + i];
      const int kk = part_k[(size_t)c * m + i];
      if (d < best) { best = d; bk = kk; }
    }
    int rk = -1;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (bk >= 0) {
      const size_t row = (size_t)clamp_row(sel[bk], P);
      const float dx = points[3 * (size_t)i] - xyz[3 * row], dy = points[3 * (size_t)i + 1] - xyz[3 * row + 1],
                  dz = points[3 * (size_t)i + 2] - xyz[3 * row + 2];
      const float d = sqrtf(best);
      const float t = d - r;
      if (t > 0.f) {  // max(t, 0): the clamp passes the gradient on where t > 0 only
        hinge = t;
        active = 1;
        rk = bk;
        const float w = d > 0.f ? -lam_over_m / d : 0.f;  // d|p - x|/dx = -(p - x)/d  (0 at d = 0, as Torch's norm)
        gx = w * dx; gy = w * dy; gz = w * dz;
      }
    } else {
      hinge = best;  // no centre compared below +inf (non-finite input): the loss says so, nothing is written
    }
    rec_k[i] = rk;
    rec_g[3 * (size_t)i] = gx; rec_g[3 * (size_t)i + 1] = gy; rec_g[3 * (size_t)i + 2] = gz;
  }
  double hs = (double)hinge;
  block_sum_pair(hs, active, shsum, shcnt);
  if (threadIdx.x == 0) {
    hinge_part[blockIdx.x] = hs;
    count_part[blockIdx.x] = active;
    if (blockIdx.x == 0) *r_out = r;
  }
}

__global__ __launch_bounds__(256) void k_simi_grads(const int P, const int m, const int n, const int nblocks2,
                                                    const int* __restrict__ sel, const int* __restrict__ rec_k,
                                                    const float* __restrict__ rec_g,
                                                    const double* __restrict__ hinge_part,
                                                    const int* __restrict__ count_part, const float* __restrict__ r_in,
                                                    const float lambda, const int accumulate,
                                                    float* __restrict__ out3, float* __restrict__ grad_xyz,
                                                    float* __restrict__ grad_scaling) {
  __shared__ __attribute__((aligned(16))) int sk[SM_REC_TILE_];
  __shared__ double shsum[4];
  // number of points outside r (integers: exact in any order) and, for workgroup 0, the loss
  double hs, cnt;
  partial_pairs_sum(hinge_part, count_part, nblocks2, shsum, hs, cnt);
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) {
      const float mean_min = (float)(hs / (double)m);
      out3[0] = lambda * mean_min;
      out3[1] = mean_min;
      out3[2] = *r_in;
    }
  }
  if (!grad_xyz && !grad_scaling) return;  // (uniform)
  const int k = blockIdx.x * 256 + (int)threadIdx.x;
  const int kq = k < n ? k : -2;  // (-2 matches no record; the thread still helps to stage)
  float ax = 0.f, ay = 0.f, az = 0.f;
  if (grad_xyz) {
    for (int base = 0; base < m; base += SM_REC_TILE_) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < SM_REC_TILE_ / 256; q++) {
        const int i = base + q * 256 + (int)threadIdx.x;
        sk[q * 256 + threadIdx.x] = i < m ? rec_k[i] : -1;
      }
      __syncthreads();
      const int cntv = min(SM_REC_TILE_, m - base);
      for (int q = 0; q < cntv; q += 4) {  // ascending point order: the sum of a shared row has ONE order
        const int4 v = *reinterpret_cast<const int4*>(&sk[q]);
        if (v.x == kq || v.y == kq || v.z == kq || v.w == kq) {
          const int e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int u = 0; u < 4; u++)
            if (e[u] == kq) {
              const size_t i = (size_t)(base + q + u);
              ax += rec_g[3 * i]; ay += rec_g[3 * i + 1]; az += rec_g[3 * i + 2];
            }
        }
      }
    }
  }
  if (k >= n) return;
  const int row = sel[k];
  if (row < 0 || row >= P) return;  // (a selection that breaks its contract writes nothing)
  if (grad_xyz) {
    float* g = grad_xyz + 3 * (size_t)row;
    if (accumulate) { g[0] += ax; g[1] += ay; g[2] += az; }
    else { g[0] = ax; g[1] = ay; g[2] = az; }
  }
  if (grad_scaling) {
    // dL/dr = -lambda/m * (points outside r), spread evenly over the 3n elements r averages
    const float gs = (float)(-((double)lambda / (double)m) * cnt / (3.0 * (double)n));
    float* g = grad_scaling + 3 * (size_t)row;
    if (accumulate) { g[0] += gs; g[1] += gs; g[2] += gs; }
    else { g[0] = gs; g[1] = gs; g[2] = gs; }
  }
}

__global__ void k_simi_zero3(float* __restrict__ out3) {
  if (threadIdx.x < 3) out3[threadIdx.x] = 0.f;
}

static size_t simi_workspace_bytes(int m, int n) { return SimiWorkspace::carve(nullptr, m, n).bytes; }

static hipError_t launch_similarity_loss(int P, int m, int n, const float* points, const int* sel, const float* xyz,
                                         const float* scaling, float lambda, float* out3, float* grad_xyz,
                                         float* grad_scaling, int accumulate, char* workspace, hipStream_t s) {
  if (m == 0 || n == 0) {  // no term: {0, 0, 0}, no gradient
    ProfScope ps(K_SIMI_GRADS, s);
    hipLaunchKernelGGL(k_simi_zero3, dim3(1), dim3(64), 0, s, out3);
    return hipGetLastError();
  }
  const SimiPlan p = simi_plan(m, n);
  const SimiWorkspace w = SimiWorkspace::carve(workspace, m, n);
  {
    ProfScope ps(K_SIMI_NEAREST, s);
    hipLaunchKernelGGL(k_simi_nearest, dim3(p.pblocks, p.nchunks), dim3(256), 0, s, P, m, n, p.tiles_per_chunk,
                       p.ntiles, points, sel, xyz, scaling, w.part_d2, w.part_k, w.scale_part);
  }
  {
    ProfScope ps(K_SIMI_POINTS, s);
    hipLaunchKernelGGL(k_simi_points, dim3(p.nblocks2), dim3(256), 0, s, P, m, n, p.nchunks, points, sel, xyz,
                       w.part_d2, w.part_k, w.scale_part, lambda / (float)m, w.rec_k, w.rec_g, w.hinge_part,
                       w.count_part, w.r);
  }
  {
    ProfScope ps(K_SIMI_GRADS, s);
    const int grid = (grad_xyz || grad_scaling) ? (n + 255) / 256 : 1;
    hipLaunchKernelGGL(k_simi_grads, dim3(grid), dim3(256), 0, s, P, m, n, p.nblocks2, sel, w.rec_k, w.rec_g,
                       w.hinge_part, w.count_part, w.r, lambda, accumulate, out3, grad_xyz, grad_scaling);
  }
  return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_similarity_loss_workspace(int m, int n) {
  if (m <= 0 || n <= 0 || n > 0x7fffffff - 1024) return 0;
  return simi_workspace_bytes(m, n);
}

int gsr_similarity_loss(int P, int m, int n, const float* points, const int* sel, const float* xyz,
                        const float* scaling, float lambda, float* out3, float* grad_xyz, float* grad_scaling,
                        int accumulate, char* workspace, size_t workspace_bytes, void* stream_) {
  clear_error();
  if (P < 0 || m < 0 || n < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P/m/n");
  if (n > P) return fail(GSR_ERR_INVALID_ARGUMENT, "n = %d selected rows of P = %d (the selection is unique)", n, P);
  if (n > 0x7fffffff - 1024) return fail(GSR_ERR_INVALID_ARGUMENT, "n too large");
  if (!out3) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (m > 0 && n > 0) {
    if (!points || !sel || !xyz || !scaling || !workspace) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
    if (int e = check_workspace(workspace_bytes, simi_workspace_bytes(m, n))) return e;
  }
  HIP_TRY(launch_similarity_loss(P, m, n, points, sel, xyz, scaling, lambda, out3, grad_xyz, grad_scaling,
                                 accumulate ? 1 : 0, workspace, (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
