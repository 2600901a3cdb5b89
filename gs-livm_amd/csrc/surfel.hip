// surfel.hip -- the point-to-plane LiDAR loss on oriented surfels (an extension: the reference has no such term), fused:
//
//   k*_j = index of the smallest activated scale of selected row j (strict < from index 0: the lowest index wins a tie)
//   n_j  = column k*_j of R(q_j), q = (w, x, y, z) as given (NOT renormalised, as the rasterizer uses it),
//          R = [[1-2(y^2+z^2), 2(xy-wz), 2(xz+wy)], [2(xy+wz), 1-2(x^2+z^2), 2(yz-wx)], [2(xz-wy), 2(yz+wx), 1-2(x^2+y^2)]]
//          (column k is the axis of scaling[.][k]: Sigma = R S^2 R^T, cov3d_from_scale_rot in preprocess.hip)
//   j(i) = the nearest selected centre of point i, ties to the lower position in `sel` (gsr_nearest.hpp)
//   v_i = p_i - x_j,  d_i = |v_i|,  g_i = [d_i <= max_dist],  e_i = n_j . v_i
//   rho(e) = |e| (huber = 0);  e^2 / (2 huber) for |e| <= huber, |e| - huber / 2 beyond it (huber > 0)
//   L = lambda / m * sum_i g_i rho(e_i)  +  lambda_flat / n * sum_j scaling[j][k*_j]
//
// The search, the launch plan and the row stores are gsr_nearest.hpp's (its header has the shape of the three
// launches).  The walk of the 16-byte records stays written out in k_surfel_grads: taken from the header's
// sum_records<4> the same walk measured 4 % on the whole call (0.126 against 0.121 ms at 3 000 x 50 000), written in
// place it costs nothing; order and comparisons are sum_records'.  What is this term's:
//   k_surfel_nearest  side job of the search: the workgroups of the first point block write k* per selected row and sum
//                     their chunk's smallest scales (f64, fixed order)
//   k_surfel_points   the winner's centre, quaternion and k*, the normal, gate, residual, rho and rho'; the point's
//                     20-byte record (position in sel or -1, rho', rho' v); per-workgroup partial sums of rho (f64) and
//                     counts of gated-in points
//   k_surfel_grads    from the summed records (A = sum rho', B = sum rho' v) dL/dxyz = -(lambda/m) A n,
//                     dL/drotation = (dn/dq)^T (lambda/m) B (the 3x4 Jacobian of the column, w included, no
//                     normalisation term: the activation's backward owns that) and dL/dscaling[k*] = lambda_flat / n;
//                     workgroup 0 writes out4
// No float atomics, every reduction in a fixed order (bitwise reproducible), no host synchronisation, no allocation,
// the caller's stream only.  The profiler's id word is full: the three launches are timed under K_SIMI_NEAREST /
// K_SIMI_POINTS / K_SIMI_GRADS, the ids of the family's three launches (gsr_kernel_count() stays 64).
// Built with -ffp-contract=off (build.py): accumulate = 1 adds the very bits accumulate = 0 writes, so no product may
// fuse into the add behind it; the multiply-add of the residual is written out.
// Every global access is a 4-byte one (the doubles live in the workspace, which is carved from the next multiple of
// 256): the caller's arrays need 4-byte alignment only.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_nearest.hpp"
#include "gsr_surfel_axis.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

struct SurfelWorkspace {
  float* part_d2;     // [nchunks][m] smallest squared distance of the point inside the chunk
  int* part_k;        // [nchunks][m] its position in sel
  int* kstar;         // [n] index of the smallest scale of the selected row
  double* flat_part;  // [nchunks] sum of the chunk's smallest scales
  int* rec_k;         // [m] position in sel of the nearest centre, -1: gated out (or no centre)
  float* rec_g;       // [m][4] rho', rho' v
  double* rho_part;   // [nblocks2]
  int* gate_part;     // [nblocks2]
  size_t bytes;
  static SurfelWorkspace carve(char* base, int m, int n) {
    const NearestPlan p = nearest_plan(m, n);
    Carver cv = Carver::aligned(base);
    SurfelWorkspace w;
    w.part_d2 = cv.take<float>((size_t)p.nchunks * m);
    w.part_k = cv.take<int>((size_t)p.nchunks * m);
    w.kstar = cv.take<int>((size_t)n);
    w.flat_part = cv.take<double>((size_t)p.nchunks);
    w.rec_k = cv.take<int>((size_t)m);
    w.rec_g = cv.take<float>((size_t)m * 4);
    w.rho_part = cv.take<double>((size_t)p.nblocks2);
    w.gate_part = cv.take<int>((size_t)p.nblocks2);
    w.bytes = cv.bytes();
    return w;
  }
};

__global__ __launch_bounds__(256) void k_surfel_nearest(const int P, const int m, const int n,
                                                        const int tiles_per_chunk, const int ntiles,
                                                        const float* __restrict__ points, const int* __restrict__ sel,
                                                        const float* __restrict__ xyz,
                                                        const float* __restrict__ scaling,
                                                        float* __restrict__ part_d2, int* __restrict__ part_k,
                                                        int* __restrict__ kstar, double* __restrict__ flat_part) {
  __shared__ double shsum[4];
  double ssum = 0.0;
  nearest_chunk_scan(P, m, n, tiles_per_chunk, ntiles, points, sel, xyz, part_d2, part_k, [&](int k, size_t row3) {
    float smin;  // (k* and the column: gsr_surfel_axis.hpp, shared with normal.hip)
    kstar[k] = surfel_thin_index(scaling[row3], scaling[row3 + 1], scaling[row3 + 2], smin);
    ssum += (double)smin;
  });
  if (blockIdx.x == 0) {  // (uniform over the workgroup: the workgroups whose threads ran the side job)
    const double s = block_sum(ssum, shsum);
    if (threadIdx.x == 0) flat_part[blockIdx.y] = s;
  }
}

__global__ __launch_bounds__(256) void k_surfel_points(const int P, const int m, const int n, const int nchunks,
                                                       const float* __restrict__ points, const int* __restrict__ sel,
                                                       const float* __restrict__ xyz,
                                                       const float* __restrict__ rotation,
                                                       const float* __restrict__ part_d2,
                                                       const int* __restrict__ part_k, const int* __restrict__ kstar,
                                                       const float huber, const float max_dist,
                                                       int* __restrict__ rec_k, float* __restrict__ rec_g,
                                                       double* __restrict__ rho_part, int* __restrict__ gate_part) {
  __shared__ double shsum[4];
  __shared__ int shcnt[4];
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  float rho = 0.f;
  int gated = 0;
  if (i < m) {
    const NearestHit hit = nearest_over_chunks(part_d2, part_k, m, nchunks, i);
    const float best = hit.d2;
    const int bk = hit.k;
    int rk = -1;
    float dr = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
    // (bk < 0: no centre compared below +inf -- a non-finite point or centre: nothing is added, nothing is written;
    // bk >= n: a padding slot of the last tile, which only a point beyond 1e38 can be near: no centre either)
    if (bk >= 0 && bk < n && sqrtf(best) <= max_dist) {
      const size_t row = (size_t)clamp_row(sel[bk], P);
      const float vx = points[3 * (size_t)i] - xyz[3 * row], vy = points[3 * (size_t)i + 1] - xyz[3 * row + 1],
                  vz = points[3 * (size_t)i + 2] - xyz[3 * row + 2];
      float n0, n1, n2;
      surfel_axis(kstar[bk], rotation[4 * row], rotation[4 * row + 1], rotation[4 * row + 2], rotation[4 * row + 3],
                  n0, n1, n2);
      const float e = __builtin_fmaf(n2, vz, __builtin_fmaf(n1, vy, n0 * vx));
      const float ae = fabsf(e);
      if (huber > 0.f && ae <= huber) {
        rho = e * e / (2.f * huber);
        dr = e / huber;
      } else {
        rho = ae - 0.5f * huber;
        dr = e > 0.f ? 1.f : (e < 0.f ? -1.f : e);  // sign(0) = 0 (a NaN residual stays a NaN)
      }
      gated = 1;
      rk = bk;
      bx = dr * vx; by = dr * vy; bz = dr * vz;
    }
    rec_k[i] = rk;
    float* g = rec_g + 4 * (size_t)i;
    g[0] = dr; g[1] = bx; g[2] = by; g[3] = bz;
  }
  double rs = (double)rho;
  block_sum_pair(rs, gated, shsum, shcnt);
  if (threadIdx.x == 0) {
    rho_part[blockIdx.x] = rs;
    gate_part[blockIdx.x] = gated;
  }
}

__global__ __launch_bounds__(256) void k_surfel_grads(const int P, const int m, const int n, const int nchunks,
                                                      const int nblocks2, const int* __restrict__ sel,
                                                      const float* __restrict__ rotation,
                                                      const int* __restrict__ kstar, const int* __restrict__ rec_k,
                                                      const float* __restrict__ rec_g,
                                                      const double* __restrict__ flat_part,
                                                      const double* __restrict__ rho_part,
                                                      const int* __restrict__ gate_part, const float lambda,
                                                      const float lambda_flat, const int accumulate,
                                                      float* __restrict__ out4, float* __restrict__ grad_xyz,
                                                      float* __restrict__ grad_scaling,
                                                      float* __restrict__ grad_rotation) {
  __shared__ __attribute__((aligned(16))) int sk[NEAREST_REC_TILE];
  __shared__ double shsum[4];
  if (blockIdx.x == 0) {  // (uniform over the workgroup)
    double rs, cnt;
    partial_pairs_sum(rho_part, gate_part, nblocks2, shsum, rs, cnt);
    const double fs = partials_sum(flat_part, nchunks, shsum);
    if (threadIdx.x == 0) {
      const float mean_rho = (float)(rs / (double)m), mean_flat = (float)(fs / (double)n);
      out4[0] = lambda * mean_rho + lambda_flat * mean_flat;
      out4[1] = mean_rho;
      out4[2] = mean_flat;
      out4[3] = (float)(cnt / (double)m);
    }
  }
  if (!grad_xyz && !grad_scaling && !grad_rotation) return;  // (uniform)
  const int k = blockIdx.x * 256 + (int)threadIdx.x;
  const int kq = k < n ? k : -2;  // (-2 matches no record; the thread still helps to stage)
  float a = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
  if (grad_xyz || grad_rotation) {
    for (int base = 0; base < m; base += NEAREST_REC_TILE) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < NEAREST_REC_TILE / 256; q++) {
        const int i = base + q * 256 + (int)threadIdx.x;
        sk[q * 256 + threadIdx.x] = i < m ? rec_k[i] : -1;
      }
      __syncthreads();
      const int cntv = min(NEAREST_REC_TILE, m - base);
      for (int q = 0; q < cntv; q += 4) {  // ascending point order: the sum of a shared row has ONE order
        const int4 v = *reinterpret_cast<const int4*>(&sk[q]);  // (the same address in every lane: a broadcast read)
        if (v.x == kq || v.y == kq || v.z == kq || v.w == kq) {
          const int e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int u = 0; u < 4; u++)
            if (e[u] == kq) {
              const float* g = rec_g + 4 * (size_t)(base + q + u);
              a += g[0]; bx += g[1]; by += g[2]; bz += g[3];
            }
        }
      }
    }
  }
  if (k >= n) return;
  const int row = sel[k];
  if (row < 0 || row >= P) return;  // (a selection that breaks its contract writes nothing)
  const int ks = kstar[k];
  const float c = lambda / (float)m;
  const float qw = rotation[4 * (size_t)row], qx = rotation[4 * (size_t)row + 1], qy = rotation[4 * (size_t)row + 2],
              qz = rotation[4 * (size_t)row + 3];
  if (grad_xyz) {
    float n0, n1, n2;
    surfel_axis(ks, qw, qx, qy, qz, n0, n1, n2);
    const float ca = -(c * a);
    const float v[3] = {ca * n0, ca * n1, ca * n2};
    store_row(grad_xyz + 3 * (size_t)row, v, accumulate);
  }
  if (grad_rotation) {
    // (dn/dq)^T b for the column ks of R, b = (lambda/m) B: the derivative of the polynomial, all four components
    const float b0 = c * bx, b1 = c * by, b2 = c * bz;
    float gw, gx, gy, gz;
    if (ks == 0) {
      gw = 2.f * (qz * b1 - qy * b2);
      gx = 2.f * (qy * b1 + qz * b2);
      gy = 2.f * (qx * b1 - qw * b2) - 4.f * qy * b0;
      gz = 2.f * (qw * b1 + qx * b2) - 4.f * qz * b0;
    } else if (ks == 1) {
      gw = 2.f * (qx * b2 - qz * b0);
      gx = 2.f * (qy * b0 + qw * b2) - 4.f * qx * b1;
      gy = 2.f * (qx * b0 + qz * b2);
      gz = 2.f * (qy * b2 - qw * b0) - 4.f * qz * b1;
    } else {
      gw = 2.f * (qy * b0 - qx * b1);
      gx = 2.f * (qz * b0 - qw * b1) - 4.f * qx * b2;
      gy = 2.f * (qw * b0 + qz * b1) - 4.f * qy * b2;
      gz = 2.f * (qx * b0 + qy * b1);
    }
    const float v[4] = {gw, gx, gy, gz};
    store_row(grad_rotation + 4 * (size_t)row, v, accumulate);
  }
  if (grad_scaling) {
    // the flatness prior reaches the thin axis only; the choice of k* carries no gradient
    const float gs = lambda_flat / (float)n;
    float* g = grad_scaling + 3 * (size_t)row;
    if (accumulate) {
      g[ks] += gs;
    } else {
      g[0] = ks == 0 ? gs : 0.f; g[1] = ks == 1 ? gs : 0.f; g[2] = ks == 2 ? gs : 0.f;
    }
  }
}

__global__ void k_surfel_zero4(float* __restrict__ out4) {
  if (threadIdx.x < 4) out4[threadIdx.x] = 0.f;
}

static size_t surfel_workspace_bytes(int m, int n) { return SurfelWorkspace::carve(nullptr, m, n).bytes; }

static hipError_t launch_surfel_plane_loss(int P, int m, int n, const float* points, const int* sel, const float* xyz,
                                           const float* scaling, const float* rotation, float lambda, float huber,
                                           float max_dist, float lambda_flat, float* out4, float* grad_xyz,
                                           float* grad_scaling, float* grad_rotation, int accumulate, char* workspace,
                                           hipStream_t s) {
  if (m == 0 || n == 0) {  // no term: {0, 0, 0, 0}, no gradient
    ProfScope ps(K_SIMI_GRADS, s);
    hipLaunchKernelGGL(k_surfel_zero4, dim3(1), dim3(64), 0, s, out4);
    return hipGetLastError();
  }
  const NearestPlan p = nearest_plan(m, n);
  const SurfelWorkspace w = SurfelWorkspace::carve(workspace, m, n);
  {
    ProfScope ps(K_SIMI_NEAREST, s);
    hipLaunchKernelGGL(k_surfel_nearest, dim3(p.pblocks, p.nchunks), dim3(256), 0, s, P, m, n, p.tiles_per_chunk,
                       p.ntiles, points, sel, xyz, scaling, w.part_d2, w.part_k, w.kstar, w.flat_part);
  }
  {
    ProfScope ps(K_SIMI_POINTS, s);
    hipLaunchKernelGGL(k_surfel_points, dim3(p.nblocks2), dim3(256), 0, s, P, m, n, p.nchunks, points, sel, xyz,
                       rotation, w.part_d2, w.part_k, w.kstar, huber, max_dist, w.rec_k, w.rec_g, w.rho_part,
                       w.gate_part);
  }
  {
    ProfScope ps(K_SIMI_GRADS, s);
    const int grid = (grad_xyz || grad_scaling || grad_rotation) ? (n + 255) / 256 : 1;
    hipLaunchKernelGGL(k_surfel_grads, dim3(grid), dim3(256), 0, s, P, m, n, p.nchunks, p.nblocks2, sel, rotation,
                       w.kstar, w.rec_k, w.rec_g, w.flat_part, w.rho_part, w.gate_part, lambda, lambda_flat,
                       accumulate, out4, grad_xyz, grad_scaling, grad_rotation);
  }
  return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_surfel_plane_loss_workspace(int m, int n) {
  if (m <= 0 || n <= 0 || n > NEAREST_MAX_N) return 0;
  return surfel_workspace_bytes(m, n);
}

int gsr_surfel_plane_loss(int P, int m, int n, const float* points, const int* sel, const float* xyz,
                          const float* scaling, const float* rotation, float lambda, float huber, float max_dist,
                          float lambda_flat, float* out4, float* grad_xyz, float* grad_scaling, float* grad_rotation,
                          int accumulate, char* workspace, size_t workspace_bytes, void* stream_) {
  clear_error();
  if (int e = check_selection_sizes(P, m, n)) return e;
  if (!(lambda >= 0.f && lambda < __builtin_inff())) return fail(GSR_ERR_INVALID_ARGUMENT, "bad lambda");
  if (!(huber >= 0.f && huber < __builtin_inff())) return fail(GSR_ERR_INVALID_ARGUMENT, "bad huber");
  if (!(lambda_flat >= 0.f && lambda_flat < __builtin_inff())) return fail(GSR_ERR_INVALID_ARGUMENT, "bad lambda_flat");
  if (!(max_dist > 0.f)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad max_dist");
  if (!out4) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (m > 0 && n > 0) {
    if (!points || !sel || !xyz || !scaling || !rotation || !workspace)
      return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
    if (int e = check_workspace(workspace_bytes, surfel_workspace_bytes(m, n))) return e;
  }
  if (int e = check_aligned4((uintptr_t)points | (uintptr_t)sel | (uintptr_t)xyz | (uintptr_t)scaling |
                             (uintptr_t)rotation | (uintptr_t)out4 | (uintptr_t)grad_xyz | (uintptr_t)grad_scaling |
                             (uintptr_t)grad_rotation))
    return e;
  HIP_TRY(launch_surfel_plane_loss(P, m, n, points, sel, xyz, scaling, rotation, lambda, huber, max_dist, lambda_flat,
                                   out4, grad_xyz, grad_scaling, grad_rotation, accumulate ? 1 : 0, workspace,
                                   (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
