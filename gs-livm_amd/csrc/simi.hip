// simi.hip -- the LiDAR similarity loss of GS-LIVM's optimiser (optimize_vis step 3), fused:
//
//   r = mean(scales[sel])                      one scalar over the 3n selected (activated) scale elements
//   L = lambda / m * sum_i max(min_j |p_i - x_sel[j]| - r, 0)
//
// Reference: GaussianModel::compute_min_distance (src/gs/gaussian.cu:87-114) called from calcSimiLoss (:201-239) at
// src/liw/lioOptimization.cpp:1675 with lambda_depth_simi (config/basic_common.yaml:64).  The reference expands
// m x n x 3 floats several times over, forward and backward; since r is ONE scalar, clamp and min commute and the term
// is a nearest-neighbour search followed by one clamp per point.  The search, its tie rule, the launch plan and the
// walk of the records are gsr_nearest.hpp's (its header has the shape of the three launches); what is this term's:
//   k_simi_nearest   side job of the search: the workgroups of the first point block sum their chunk's scales (f64,
//                    fixed order)
//   k_simi_points    r from the chunk sums, the clamp, and the point's gradient record (position of its nearest centre
//                    or -1, and -lambda/m (p - x)/d); per-workgroup partial sums of the clamped distances (f64) and
//                    counts of points outside r
//   k_simi_grads     the summed records ARE the row of dL/dxyz; every selected scale element receives dL/dr / (3n);
//                    workgroup 0 writes {loss, mean clamped distance, r}
// No float atomics, every reduction in a fixed order (bitwise reproducible), no host synchronisation, three launches
// on the caller's stream.  A point at exactly d == r contributes nothing (the reference leaves that undefined, as it
// does a tie between two centres).  m and n are bounded by int only: the 500-point cap of the reference (MAX_SIMI,
// include/gs/gp3d/gp_types.h:15) is the host's policy.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_nearest.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

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
    const NearestPlan p = nearest_plan(m, n);
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
    w.bytes = cv.bytes();
    return w;
  }
};

__global__ __launch_bounds__(256) void k_simi_nearest(const int P, const int m, const int n, const int tiles_per_chunk,
                                                      const int ntiles, const float* __restrict__ points,
                                                      const int* __restrict__ sel, const float* __restrict__ xyz,
                                                      const float* __restrict__ scaling,
                                                      float* __restrict__ part_d2, int* __restrict__ part_k,
                                                      double* __restrict__ scale_part) {
  __shared__ double shsum[4];
  double ssum = 0.0;
  nearest_chunk_scan(P, m, n, tiles_per_chunk, ntiles, points, sel, xyz, part_d2, part_k, [&](int, size_t row3) {
    ssum += ((double)scaling[row3] + (double)scaling[row3 + 1]) + (double)scaling[row3 + 2];
  });
  if (blockIdx.x == 0) {  // (uniform over the workgroup: the workgroups whose threads ran the side job)
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
    const NearestHit hit = nearest_over_chunks(part_d2, part_k, m, nchunks, i);
    const float best = hit.d2;
    const int bk = hit.k;
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
  float a[3] = {0.f, 0.f, 0.f};
  if (grad_xyz) sum_records(m, rec_k, rec_g, kq, a);
  if (k >= n) return;
  const int row = sel[k];
  if (row < 0 || row >= P) return;  // (a selection that breaks its contract writes nothing)
  if (grad_xyz) store_row(grad_xyz + 3 * (size_t)row, a, accumulate);
  if (grad_scaling) {
    // dL/dr = -lambda/m * (points outside r), spread evenly over the 3n elements r averages
    const float gs = (float)(-((double)lambda / (double)m) * cnt / (3.0 * (double)n));
    const float v[3] = {gs, gs, gs};
    store_row(grad_scaling + 3 * (size_t)row, v, accumulate);
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
  const NearestPlan p = nearest_plan(m, n);
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
  if (m <= 0 || n <= 0 || n > NEAREST_MAX_N) return 0;
  return simi_workspace_bytes(m, n);
}

int gsr_similarity_loss(int P, int m, int n, const float* points, const int* sel, const float* xyz,
                        const float* scaling, float lambda, float* out3, float* grad_xyz, float* grad_scaling,
                        int accumulate, char* workspace, size_t workspace_bytes, void* stream_) {
  clear_error();
  if (int e = check_selection_sizes(P, m, n)) return e;
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
