// delta.hip -- the delta-depth loss between a history keyframe and its successor (optimize_vis step 5), fused, with
// the gradients towards both rendered depth images.
//
// Reference: the loop at src/liw/lioOptimization.cpp:1780-1801 around GaussianModel::calcDeltaSimi
// (src/gs/gaussian.cu:116-199), inv_depth (include/gs/gs/loss_utils.cuh:15-21), lambda_delta_depth_simi
// (config/basic_common.yaml:65).  Per pair (src, ref) of H x W images, for every SOURCE pixel (u, v), d = depth_src[v,u]:
//   cam = inv_K_src (u d, v d, d)                                   gaussian.cu:133-135
//   p'  = R_rel cam + t_rel,  [R_rel | t_rel] = T_ref T_src^-1      :154-163
//   Z'[v,u] = p'.z,  (X, Y) = (K_ref p').xy / (K_ref p').z          :165-171
//   out[v,u] = bilinear sample of Z' at (X, Y), zero padding, align_corners = true          :173-194
//   a = inv_depth(out), b = inv_depth(depth_ref), inv_depth(x) = x <= 0.01 ? 0 : 1 / x      lioOptimization.cpp:1783-1784
//   mask = !(acc_src < 0.5) !(acc_ref < 0.5)                                                :1786-1795
//   L = lambda mean_{all H W pixels} |a mask - b mask|                                      :1797-1799
// Z' is an image indexed by SOURCE pixels and it is sampled at the REFERENCE-view coordinates of those same pixels:
// the reference resamples the transformed depth in the source frame's own grid (gaussian.cu:171-194; its division by
// W-1, H-1 and grid_sample's un-normalisation cancel).  That is arguably not the warp its author meant -- a forward
// splat or a sample of depth_ref would be -- and it is what a drop-in has to reproduce, so it is reproduced.
// A masked pixel contributes exactly 0 (the reference multiplies, which differs for non-finite values only).
//
// The composition is done once on the host in double (launch_delta_depth_loss): A = R_rel inv_K_src, M = K_ref A,
// n = K_ref t_rel, so that per pixel  Z' = d (A_2 . (u,v,1)) + t_z  and  N = d (M (u,v,1)) + n,  (X, Y) = N.xy / N.z.
//
// Gradient (the derivative of the forward above; the reference's own backward never reaches a Gaussian):
//   g_i  = mask_i sign(a_i - b_i)                    sign(0) = 0, as loss.hip
//   dL/ddepth_ref[i] = c g_i b_i^2                   c = lambda / (H W); 0 where depth_ref <= 0.01
//   u_i  = -g_i a_i^2                                the unit upstream of out_i; 0 where out_i <= 0.01
//   dL/ddepth_src[j] = c ( r_z(j) sum_{i, k: tap k of i is j} u_i w_ik               Z'_j is linear in d_j, slope r_z(j)
//                          + u_j (dout_j/dX dX_j/dd + dout_j/dY dY_j/dd) )           the sample coordinates of j itself
//   dout/dX = (1-fy)(Z10 - Z00) + fy (Z11 - Z01) with taps outside the image read as 0, dX/dd = (m_x - X m_z) / N_z;
//   at an integer coordinate the cell floor() selects gives the slope.  acc gets no gradient (comparisons).
//
// The tap route is a many-to-one scatter (every hole of depth 0 lands in one cell).  It is summed in 64-bit integer
// fixed point: |u_i| <= 1e4 by the clamp at 0.01 and w <= 1, the per-call maximum Mx = max_i |u_i| is found with an
// integer atomic maximum on the float's bits, Mx < 2^e, and with nb = ceil(log2(4 H W)) every contribution is scaled by
// 2^s, s = 62 - nb - e, so that 4 H W contributions of magnitude < 2^(e+s) stay below 2^62.  The product u w is exact in
// double (24 + 24 bits), is rounded ONCE to an integer and added with a 64-bit integer vector atomic whose result is not
// used; integer addition commutes, so the sum does not depend on the order and is converted back once.
// Quantisation: each contribution is off by at most half a grid step 2^-(s+1); a destination j that receives N_j
// contributions is off by at most  N_j 2^-(s+1) |r_z(j)| c  in dL/ddepth_src[j], and 2^-s <= 4 (4 H W) Mx 2^-62
// (tests/test_gpu_delta.py adds this term to its bar).  Contributions with u_i == 0 (masked pixels: the holes) are
// skipped.  No float atomics; the scalar sums are f64 partials added in a fixed order: bitwise reproducible.
//
// Bounds: a sample coordinate that is not finite or lies beyond +-2^30 is "outside" (value 0, no gradient) and is never
// converted to an integer; every tap index is tested against the image before any read or atomic.  Non-finite depths
// are outside the contract; they stay in bounds and terminate (a non-finite u is not scattered).
//
// Four launches on the caller's stream (three without dL_ddepth_src), no host synchronisation, no allocation:
//   k_delta_project  thread = source pixel: Z', (X, Y); zeroes the pixel's accumulator and the maximum word
//   k_delta_sample   thread = pixel: out, warped, a, b, mask, gap; dL/ddepth_ref; u_i and the coordinate-route term into
//                    the workspace; per-workgroup f64 gap sums and mask counts; the maximum of |u|
//   k_delta_scatter  thread = pixel: the four fixed-point contributions; workgroup 0 sums the partials and writes out3
//   k_delta_convert  thread = destination pixel: accumulator back to float, times r_z, plus the coordinate term, times c
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

struct DeltaCam {   // composed on the host in double, rounded once
  float a2[3];      // third row of A = R_rel inv_K_src: r_z(u, v) = a2 . (u, v, 1) = dZ'/dd
  float tz;
  float m[9];       // M = K_ref A, row-major
  float n[3];       // K_ref t_rel
};

struct DeltaWorkspace {
  float* zp;                 // [HW] Z'
  float2* xy;                // [HW] (X, Y)
  float* up;                 // [HW] u_i
  float* coord;              // [HW] u_j (dout/dX dX/dd + dout/dY dY/dd)
  unsigned long long* acc;   // [HW] fixed-point sums of u_i w_ik per destination
  double* gap_part;          // [nblocks]
  int* cnt_part;             // [nblocks]
  unsigned int* maxbits;     // [1] bits of max |u|
  size_t bytes;
  static DeltaWorkspace carve(char* base, int H, int W) {
    const size_t N = (size_t)H * W, nblocks = (N + 255) / 256;
    Carver cv = Carver::aligned(base);
    DeltaWorkspace w;
    w.zp = cv.take<float>(N);
    w.xy = cv.take<float2>(N);
    w.up = cv.take<float>(N);
    w.coord = cv.take<float>(N);
    w.acc = cv.take<unsigned long long>(N);
    w.gap_part = cv.take<double>(nblocks);
    w.cnt_part = cv.take<int>(nblocks);
    w.maxbits = cv.take<unsigned int>(1);
    w.bytes = cv.bytes();
    return w;
  }
};

constexpr float DELTA_MIN_DEPTH_ = 0.01f;         // inv_depth's clamp (loss_utils.cuh:15-21)

// The cell of a sample coordinate: false = outside (no tap can lie in the image); else the integer corner (ix, iy) in
// [-1, W) x [-1, H) and the fractions.  The comparison is false for NaN, so nothing non-finite reaches the conversion.
__device__ __forceinline__ bool delta_cell(float X, float Y, int W, int H, int& ix, int& iy, float& fx, float& fy) {
  if (!(fabsf(X) <= COORD_MAX_) || !(fabsf(Y) <= COORD_MAX_)) return false;
  const float x0 = floorf(X), y0 = floorf(Y);
  ix = (int)x0; iy = (int)y0;
  fx = X - x0; fy = Y - y0;
  return ix >= -1 && ix < W && iy >= -1 && iy < H;
}

__global__ __launch_bounds__(256) void k_delta_project(const int N, const int W, const DeltaCam cam,
                                                       const float* __restrict__ depth_src, float* __restrict__ zp,
                                                       float2* __restrict__ xy, unsigned long long* __restrict__ acc,
                                                       unsigned int* __restrict__ maxbits) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i == 0) *maxbits = 0u;
  if (i >= N) return;
  const float u = (float)(i % W), v = (float)(i / W);
  const float d = depth_src[i];
  const float rz = __builtin_fmaf(cam.a2[0], u, __builtin_fmaf(cam.a2[1], v, cam.a2[2]));
  const float mx = __builtin_fmaf(cam.m[0], u, __builtin_fmaf(cam.m[1], v, cam.m[2]));
  const float my = __builtin_fmaf(cam.m[3], u, __builtin_fmaf(cam.m[4], v, cam.m[5]));
  const float mz = __builtin_fmaf(cam.m[6], u, __builtin_fmaf(cam.m[7], v, cam.m[8]));
  const float nz = __builtin_fmaf(d, mz, cam.n[2]);
  zp[i] = __builtin_fmaf(d, rz, cam.tz);
  xy[i] = make_float2(__builtin_fmaf(d, mx, cam.n[0]) / nz, __builtin_fmaf(d, my, cam.n[1]) / nz);
  if (acc) acc[i] = 0ull;
}

__global__ __launch_bounds__(256) void k_delta_sample(const int N, const int W, const int H, const DeltaCam cam,
                                                      const float c, const float* __restrict__ depth_src,
                                                      const float* __restrict__ acc_src,
                                                      const float* __restrict__ depth_ref,
                                                      const float* __restrict__ acc_ref, const float* __restrict__ zp,
                                                      const float2* __restrict__ xy, float* __restrict__ warped,
                                                      float* __restrict__ dL_ddepth_ref, float* __restrict__ up,
                                                      float* __restrict__ coord, double* __restrict__ gap_part,
                                                      int* __restrict__ cnt_part, unsigned int* __restrict__ maxbits) {
  __shared__ double shsum[4];
  __shared__ int shcnt[4];
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  float gap = 0.f, absu = 0.f;
  int on = 0;
  if (i < N) {
    const float2 p = xy[i];
    int ix, iy;
    float fx, fy;
    float out = 0.f, sx = 0.f, sy = 0.f;
    const bool inside = delta_cell(p.x, p.y, W, H, ix, iy, fx, fy);
    if (inside) {
      const bool x0 = ix >= 0, x1 = ix + 1 < W, y0 = iy >= 0, y1 = iy + 1 < H;  // (ix < W and iy < H by delta_cell)
      const size_t o = (size_t)(iy < 0 ? 0 : iy) * W + (size_t)(ix < 0 ? 0 : ix);  // in bounds; used where x0 && y0
      const float z00 = (x0 && y0) ? zp[o] : 0.f;
      const float z10 = (x1 && y0) ? zp[(size_t)iy * W + ix + 1] : 0.f;
      const float z01 = (x0 && y1) ? zp[(size_t)(iy + 1) * W + ix] : 0.f;
      const float z11 = (x1 && y1) ? zp[(size_t)(iy + 1) * W + ix + 1] : 0.f;
      const float gx = 1.f - fx, gy = 1.f - fy;
      out = __builtin_fmaf(fx * fy, z11, __builtin_fmaf(gx * fy, z01, __builtin_fmaf(fx * gy, z10, (gx * gy) * z00)));
      sx = __builtin_fmaf(fy, z11 - z01, gy * (z10 - z00));
      sy = __builtin_fmaf(fx, z11 - z10, gx * (z01 - z00));
    }
    if (warped) warped[i] = out;
    const float dr = depth_ref[i];
    const float a = out <= DELTA_MIN_DEPTH_ ? 0.f : 1.f / out;
    const float b = dr <= DELTA_MIN_DEPTH_ ? 0.f : 1.f / dr;
    on = (!(acc_src[i] < 0.5f) && !(acc_ref[i] < 0.5f)) ? 1 : 0;
    const float df = a - b;
    const float g = on ? (float)((df > 0.f) - (df < 0.f)) : 0.f;
    gap = on ? fabsf(df) : 0.f;
    if (dL_ddepth_ref) dL_ddepth_ref[i] = (g != 0.f && dr > DELTA_MIN_DEPTH_) ? c * (g * (b * b)) : 0.f;
    if (up) {
      float ui = (g != 0.f && out > DELTA_MIN_DEPTH_) ? -g * (a * a) : 0.f;
      if (!(fabsf(ui) <= 1.0e4f * 1.0001f)) ui = 0.f;  // (non-finite input only: nothing non-finite is scattered)
      float cr = 0.f;
      if (ui != 0.f) {
        const float u = (float)(i % W), v = (float)(i / W);
        const float mx = __builtin_fmaf(cam.m[0], u, __builtin_fmaf(cam.m[1], v, cam.m[2]));
        const float my = __builtin_fmaf(cam.m[3], u, __builtin_fmaf(cam.m[4], v, cam.m[5]));
        const float mz = __builtin_fmaf(cam.m[6], u, __builtin_fmaf(cam.m[7], v, cam.m[8]));
        const float nz = __builtin_fmaf(depth_src[i], mz, cam.n[2]);
        const float dX = __builtin_fmaf(-p.x, mz, mx) / nz, dY = __builtin_fmaf(-p.y, mz, my) / nz;
        cr = ui * __builtin_fmaf(sy, dY, sx * dX);
      }
      up[i] = ui;
      coord[i] = cr;
      absu = fabsf(ui);
    }
  }
  double gs = (double)gap;
  block_sum_pair(gs, on, shsum, shcnt);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) absu = fmaxf(absu, __shfl_xor(absu, o, 64));
  // non-negative floats order like their bits; a maximum does not depend on the order it is taken in
  if ((threadIdx.x & 63) == 0 && absu > 0.f) atomicMax(maxbits, __float_as_uint(absu));
  if (threadIdx.x == 0) {
    gap_part[blockIdx.x] = gs;
    cnt_part[blockIdx.x] = on;
  }
}

// s of the header: Mx < 2^e from the float's exponent field (a denormal maximum counts as the smallest normal)
__device__ __forceinline__ int delta_scale(unsigned int maxbits, int nb) {
  if (maxbits == 0u) return 0;
  const int e = (int)(maxbits >> 23) - 126;  // bits of a positive finite float: 2^(e-1) <= Mx < 2^e
  return 62 - nb - e;
}

__global__ __launch_bounds__(256) void k_delta_scatter(const int N, const int W, const int H, const int nb,
                                                       const int nblocks, const float lambda,
                                                       const float2* __restrict__ xy, const float* __restrict__ up,
                                                       unsigned long long* __restrict__ acc,
                                                       const double* __restrict__ gap_part,
                                                       const int* __restrict__ cnt_part,
                                                       const unsigned int* __restrict__ maxbits,
                                                       float* __restrict__ out3) {
  __shared__ double shsum[4];
  if (blockIdx.x == 0) {  // the scalars: thread-strided over the partials, then the workgroup tree -- one fixed order
    double gs, cs;
    partial_pairs_sum(gap_part, cnt_part, nblocks, shsum, gs, cs);
    if (threadIdx.x == 0) {
      const float mean_gap = (float)(gs / (double)N);
      out3[0] = lambda * mean_gap;
      out3[1] = mean_gap;
      out3[2] = (float)(cs / (double)N);
    }
  }
  if (!up) return;  // (uniform: no dL_ddepth_src wanted)
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= N) return;
  const float ui = up[i];
  if (ui == 0.f) return;
  const float2 p = xy[i];
  int ix, iy;
  float fx, fy;
  if (!delta_cell(p.x, p.y, W, H, ix, iy, fx, fy)) return;
  const int s = delta_scale(*maxbits, nb);
  const float gx = 1.f - fx, gy = 1.f - fy;
  const float w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int x = ix + (k & 1), y = iy + (k >> 1);
    if (x < 0 || x >= W || y < 0 || y >= H || w[k] == 0.f) continue;
    // |ui w| < 2^e, so |q| < 2^(62 - nb): exact product, one rounding
    const long long q = __double2ll_rn(ldexp((double)ui * (double)w[k], s));
    atomicAdd(&acc[(size_t)y * W + x], (unsigned long long)q);
  }
}

__global__ __launch_bounds__(256) void k_delta_convert(const int N, const int W, const int nb, const DeltaCam cam,
                                                       const float c, const unsigned long long* __restrict__ acc,
                                                       const float* __restrict__ coord,
                                                       const unsigned int* __restrict__ maxbits,
                                                       float* __restrict__ dL_ddepth_src) {
  const int j = blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= N) return;
  const int s = delta_scale(*maxbits, nb);
  const float taps = (float)ldexp((double)(long long)acc[j], -s);
  const float u = (float)(j % W), v = (float)(j / W);
  const float rz = __builtin_fmaf(cam.a2[0], u, __builtin_fmaf(cam.a2[1], v, cam.a2[2]));
  dL_ddepth_src[j] = c * __builtin_fmaf(rz, taps, coord[j]);
}

static size_t delta_workspace_bytes(int H, int W) { return DeltaWorkspace::carve(nullptr, H, W).bytes; }

static hipError_t launch_delta_depth_loss(int H, int W, const float* depth_src, const float* acc_src,
                                          const float* depth_ref, const float* acc_ref, const float* inv_K_src9,
                                          const float* K_ref9, const float* T_rel12, float lambda, float* out3,
                                          float* warped, float* dL_ddepth_src, float* dL_ddepth_ref, char* workspace,
                                          hipStream_t s) {
  const int N = H * W, nblocks = (N + 255) / 256;
  DeltaCam cam;
  {
    double A[9], M[9];
    for (int r = 0; r < 3; r++)
      for (int q = 0; q < 3; q++) {
        double v = 0.0;
        for (int k = 0; k < 3; k++) v += (double)T_rel12[4 * r + k] * (double)inv_K_src9[3 * k + q];
        A[3 * r + q] = v;
      }
    for (int r = 0; r < 3; r++) {
      for (int q = 0; q < 3; q++) {
        double v = 0.0;
        for (int k = 0; k < 3; k++) v += (double)K_ref9[3 * r + k] * A[3 * k + q];
        M[3 * r + q] = v;
      }
      double v = 0.0;
      for (int k = 0; k < 3; k++) v += (double)K_ref9[3 * r + k] * (double)T_rel12[4 * k + 3];
      cam.n[r] = (float)v;
    }
    for (int q = 0; q < 3; q++) cam.a2[q] = (float)A[6 + q];
    for (int q = 0; q < 9; q++) cam.m[q] = (float)M[q];
    cam.tz = T_rel12[11];
  }
  int nb = 0;  // ceil(log2(4 N))
  while ((1ull << nb) < 4ull * (unsigned long long)N) nb++;
  const float c = lambda / (float)N;
  const DeltaWorkspace w = DeltaWorkspace::carve(workspace, H, W);
  const bool gsrc = dL_ddepth_src != nullptr;
  {
    ProfScope ps(K_DELTA_PROJECT, s);
    hipLaunchKernelGGL(k_delta_project, dim3(nblocks), dim3(256), 0, s, N, W, cam, depth_src, w.zp, w.xy,
                       gsrc ? w.acc : nullptr, w.maxbits);
  }
  {
    ProfScope ps(K_DELTA_SAMPLE, s);
    hipLaunchKernelGGL(k_delta_sample, dim3(nblocks), dim3(256), 0, s, N, W, H, cam, c, depth_src, acc_src, depth_ref,
                       acc_ref, w.zp, w.xy, warped, dL_ddepth_ref, gsrc ? w.up : nullptr, w.coord, w.gap_part,
                       w.cnt_part, w.maxbits);
  }
  {
    ProfScope ps(K_DELTA_SCATTER, s);
    hipLaunchKernelGGL(k_delta_scatter, dim3(gsrc ? nblocks : 1), dim3(256), 0, s, N, W, H, nb, nblocks, lambda, w.xy,
                       gsrc ? w.up : nullptr, w.acc, w.gap_part, w.cnt_part, w.maxbits, out3);
  }
  if (gsrc) {
    ProfScope ps(K_DELTA_CONVERT, s);
    hipLaunchKernelGGL(k_delta_convert, dim3(nblocks), dim3(256), 0, s, N, W, nb, cam, c, w.acc, w.coord, w.maxbits,
                       dL_ddepth_src);
  }
  return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_delta_depth_loss_workspace(int height, int width) {
  if (height < 2 || width < 2 || !plane_fits(height, width, 0x80000000ull)) return 0;
  return delta_workspace_bytes(height, width);
}

int gsr_delta_depth_loss(int height, int width, const float* depth_src, const float* acc_src, const float* depth_ref,
                         const float* acc_ref, const float* inv_K_src9, const float* K_ref9, const float* T_rel12,
                         float lambda, float* out3, float* warped, float* dL_ddepth_src, float* dL_ddepth_ref,
                         char* workspace, size_t workspace_bytes, void* stream_) {
  clear_error();
  if (height < 2 || width < 2)  // (the reference divides by W - 1 and H - 1)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape: at least 2 x 2");
  if (int e = check_plane(height, width, 0x80000000ull)) return e;  // (32-bit pixel indices)
  if (!depth_src || !acc_src || !depth_ref || !acc_ref || !inv_K_src9 || !K_ref9 || !T_rel12 || !out3 || !workspace)
    return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_workspace(workspace_bytes, delta_workspace_bytes(height, width))) return e;
  HIP_TRY(launch_delta_depth_loss(height, width, depth_src, acc_src, depth_ref, acc_ref, inv_K_src9, K_ref9, T_rel12,
                                  lambda, out3, warped, dL_ddepth_src, dL_ddepth_ref, workspace,
                                  (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
