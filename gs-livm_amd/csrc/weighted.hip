// weighted.hip -- the weighted photometric loss (an extension: the reference has no such term): exposure.hip's loss
// with a weight per pixel, a silhouette gate and the exposure each optional, normalised by the weight sum.
//
//   x'(p) = fma(g_c, x(p), b_c) with an exposure, x(p) without one (no FMA is issued)
//   w(p)  = weights(p) * [acc(p) >= acc_min]        a NaN acc fails the comparison: weight 0; [H][W], shared by the channels
//   S     = sum_p w(p)                              over the H W pixels
//   l1    = sum_c sum_p w |x' - y| / (C S)          ssim = sum_c sum_q w(q) SSIM_c(q) / (C S), the windows over the FULL x', y
//   L     = (1 - lambda) l1 + lambda (1 - ssim)     mse_c = sum_p w (x' - y)^2 / S,  psnr = metrics.hip's rule on mse_c
//   G(p)  = dL/dx'(p) = (1 - lambda) / (C S) w(p) sign(x' - y) - lambda / (C S) sum_q k(p, q) w(q) [A + 2 x'(p) B + y(p) C](q)
//   dL/dx = g_c G,   dL/dg_c = sum_p G x (the ORIGINAL x),   dL/db_c = sum_p G
//
// The weights and acc are data: no gradient reaches them, and the gate is a step.  Weights are the caller's contract:
// finite and >= 0.  A ZERO WEIGHT DOES NOT PROTECT AGAINST A NON-FINITE PIXEL: the SSIM windows of the weighted
// neighbours within 5 pixels read it.  S = 0: L = l1 = ssim = mse = 0, psnr = +inf and every gradient element is zero.
//   k_weighted_loss_forward   k_exposure_loss_forward's arithmetic in its order; stores w A, w B, w C; four partials per
//                             work unit: sum w |d|, sum w SSIM, sum w d^2, sum w (channel 0's define S)
//   k_weighted_loss_backward  k_exposure_loss_backward's arithmetic with w(p) on the L1 term; every workgroup forms
//                             (float)(1 / (C S)) itself from channel 0's partials of sum w, in one fixed order; the
//                             float64 pair sums only with an exposure
//   k_weighted_loss_finish    one workgroup: out6 = {L, l1, ssim, S, mean_c mse_c, psnr} and dL_dexposure; S in the
//                             backward's order: the same bits
// Three launches with a gradient, two without, as the exposure loss; no host wait.
// With weights of one (given or absent) every term equals exposure.hip's bit for bit: a weight enters as one factor of
// a fused multiply-add whose other operands are exactly those of the unweighted statement as the compiler contracts it
// (DESIGN.md section 4), so a factor of 1 changes no rounding; a power of two scales every sum exactly.
// Deterministic: no atomics, fixed-order reductions.  Built with loss.hip's flags (build.py).
#include <math.h>

#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_window.hpp"

namespace gsr {

constexpr int WPART_ = 4;  // partials per work unit: sum w |d|, sum w SSIM, sum w d^2, sum w

// w(p) at N plane offsets.  Both pointers are uniform over the launch: an absent operand costs no load, and the N loads
// of a present one are in flight together.
template <int N>
__device__ __forceinline__ void pixel_weights(const float* __restrict__ weights, const float* __restrict__ acc,
                                              const float acc_min, const int (&off)[N], float (&w)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) w[i] = 1.f;
  if (weights) {
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = weights[off[i]];
  }
  if (acc) {
    float a[N];
#pragma unroll
    for (int i = 0; i < N; i++) a[i] = acc[off[i]];
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = a[i] >= acc_min ? w[i] : 0.f;  // (NaN >= x is false)
  }
}

template <bool HAS_E>
__global__ __launch_bounds__(256) void k_weighted_loss_forward(const int C, const int H, const int W,
                                                               const float* __restrict__ img,
                                                               const float* __restrict__ gt,
                                                               const float* __restrict__ weights,
                                                               const float* __restrict__ acc, const float acc_min,
                                                               const float* __restrict__ exposure, const Window win,
                                                               float* __restrict__ mapA, float* __restrict__ mapB,
                                                               float* __restrict__ mapC, float* __restrict__ partials) {
  __shared__ WindowLds hv[4];  // vertically filtered moments
  __shared__ float red[WPART_][4];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * WIN_TX, y0 = blockIdx.y * WIN_TY;
  const size_t plane = (size_t)c * H * W;
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  float sums[WPART_] = {0.f, 0.f, 0.f, 0.f};
  {
    const float* const planes[2] = {img + plane, gt + plane};
    float v[2][WIN_IN];
    float wv[WIN_SEG];  // the weights of this thread's own eight output pixels (clamped addresses, used in the image only)
    {
      const int gxc = min(max(x0 - WIN_HALO + lane, 0), W - 1);
      int off[WIN_SEG];
#pragma unroll
      for (int o = 0; o < WIN_SEG; o++) off[o] = min(y0 + WIN_SEG * seg + o, H - 1) * W + gxc;
      pixel_weights(weights, acc, acc_min, off, wv);
    }
    const bool col_in = window_load_columns(planes, H, W, x0, y0, v);
    if (HAS_E) {  // x' inside the image; the padding stays 0 (fma(g, 0, b) would make it b)
      const float gain = exposure[2 * c], bias = exposure[2 * c + 1];
#pragma unroll
      for (int i = 0; i < WIN_IN; i++) {
        const int gy = y0 + WIN_SEG * seg - WIN_HALO + i;
        v[0][i] = col_in && gy >= 0 && gy < H ? __builtin_fmaf(gain, v[0][i], bias) : 0.f;
      }
    }
    window_vertical<4, false>(win, hv, [&](int i, float(&m)[4]) {
      const float x = v[0][i], y = v[1][i];
      m[0] = x; m[1] = y; m[2] = __builtin_fmaf(y, y, x * x); m[3] = x * y;
    });
    if (lane >= WIN_HALO && lane < WIN_HALO + WIN_TX && col_in) {  // the per-pixel terms of this thread's own eight output pixels
#pragma unroll
      for (int o = 0; o < WIN_SEG; o++)
        if (y0 + WIN_SEG * seg + o < H) {
          const float d = v[0][o + WIN_HALO] - v[1][o + WIN_HALO];
          sums[0] = __builtin_fmaf(wv[o], fabsf(d), sums[0]);
          sums[2] = __builtin_fmaf(wv[o] * d, d, sums[2]);
          sums[3] += wv[o];
        }
    }
  }
  __syncthreads();
  {
    const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * WIN_HO;
    const int gy = y0 + r;
    float wh[WIN_HO];  // the weights of this thread's seven outputs of the horizontal pass, requested before it
    {
      int off[WIN_HO];
#pragma unroll
      for (int o = 0; o < WIN_HO; o++) off[o] = min(gy, H - 1) * W + min(x0 + c0 + o, W - 1);
      pixel_weights(weights, acc, acc_min, off, wh);
    }
    float m[4][WIN_HO];
    window_horizontal<4, false>(win, hv, m);
    float oa[WIN_HO], ob[WIN_HO], oc[WIN_HO];
#pragma unroll
    for (int o = 0; o < WIN_HO; o++) {
      const int gx = x0 + c0 + o;
      oa[o] = ob[o] = oc[o] = 0.f;
      if (c0 + o < WIN_TX && gx < W && gy < H) {  // (k_loss_forward's SSIM and its three derivative maps, term for term)
        const float mu1 = m[0][o], mu2 = m[1][o], e_sum = m[2][o], e12 = m[3][o];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s12 = e12 - mu12;
        const float n1 = 2.f * mu12 + SSIM_C1, n2 = 2.f * s12 + SSIM_C2;
        const float d1 = mu1_sq + mu2_sq + SSIM_C1, d2 = (e_sum - mu1_sq - mu2_sq) + SSIM_C2;
        const float r1 = __builtin_amdgcn_rcpf(d1), r2 = __builtin_amdgcn_rcpf(d2);
        const float inv = r1 * r2;
        const float n12 = n1 * n2;
        const float sv = n12 * inv;
        const float ds_dmu1 = 2.f * n2 * (mu2 * d1 - mu1 * n1) * inv * r1;
        const float ds_ds1 = -sv * r2;
        const float ds_ds12 = 2.f * n1 * inv;
        const float a = ds_dmu1 - 2.f * mu1 * ds_ds1 - mu2 * ds_ds12;
        oa[o] = wh[o] * a;
        ob[o] = wh[o] * ds_ds1;
        oc[o] = wh[o] * ds_ds12;
        // the unweighted statement `sum += n1 * n2 * inv` is contracted to fma(n1 n2, inv, sum): w rides on n1 n2
        sums[1] = __builtin_fmaf(wh[o] * n12, inv, sums[1]);
      }
    }
    __syncthreads();  // (everyone has read hv)
#pragma unroll
    for (int o = 0; o < WIN_HO; o++) { hv[0][r][c0 + o] = oa[o]; hv[1][r][c0 + o] = ob[o]; hv[2][r][c0 + o] = oc[o]; }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < WIN_FLAT; it++) {  // the maps leave in the flattened order of the tile
    const int e = it * 256 + (int)threadIdx.x;
    const int row = e / WIN_TX, col = e - row * WIN_TX;
    const int gx = x0 + col, gy = y0 + row;
    if (e < WIN_TX * WIN_TY && gx < W && gy < H) {
      const size_t oidx = plane + (size_t)gy * W + gx;
      mapA[oidx] = hv[0][row][col];
      mapB[oidx] = hv[1][row][col];
      mapC[oidx] = hv[2][row][col];
    }
  }
  window_store_partials(sums, red, partials);  // four partials per workgroup
}

// S = the sum of channel 0's nper float32 partials of sum w, in float64 and in ONE order wherever it is formed: the first
// 256 threads of the workgroup add the partials thread-strided (weight_thread_sum: four loads in flight, added in
// index order; an absent one adds +0), each wave adds its lanes (wave_sum), and the first four wave sums are added as
// (s0 + s1) + (s2 + s3) (weight_total).  The backward's workgroups (256 threads) and the finish (1024) both do exactly
// this, so the S of out6[3] and the S behind every gradient element are the same bits, with no launch in between.
__device__ __forceinline__ double weight_thread_sum(const float* __restrict__ partials, const int nper) {
  double s = 0.0;
  if (threadIdx.x < 256) {
    for (int base = threadIdx.x; base < nper; base += 1024) {
      float a[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int i = base + 256 * k;
        const float v = partials[WPART_ * (size_t)min(i, nper - 1) + 3];
        a[k] = i < nper ? v : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) s += (double)a[k];
    }
  }
  return s;
}

// after every wave's lane 0 of the first four waves has stored wave_sum(weight_thread_sum) in sh[wave], and a barrier
__device__ __forceinline__ double weight_total(const double* sh) { return (sh[0] + sh[1]) + (sh[2] + sh[3]); }

// (float)(1 / (C S)); 0 for S = 0, which makes every gradient element zero
__device__ __forceinline__ float inv_weight(const int C, const double S) {
  return S > 0.0 ? (float)(1.0 / ((double)C * S)) : 0.f;
}

// G(p) as k_exposure_loss_backward forms it (in the compiler's contraction of that kernel, written out), the L1 term
// carrying w(p); the maps already carry w(q).  1 / (C S): every workgroup adds channel 0's partials of sum w itself, the
// loads requested with the weights' and the wave sums handed over at a barrier the kernel has anyway.  pairs as in
// exposure.hip, written only with an exposure.
template <bool HAS_E>
__global__ __launch_bounds__(256) void k_weighted_loss_backward(const int C, const int H, const int W,
                                                                const float* __restrict__ img,
                                                                const float* __restrict__ gt,
                                                                const float* __restrict__ weights,
                                                                const float* __restrict__ acc, const float acc_min,
                                                                const float* __restrict__ exposure, const Window win,
                                                                const float* __restrict__ mapA,
                                                                const float* __restrict__ mapB,
                                                                const float* __restrict__ mapC,
                                                                const float* __restrict__ partials, const int nper,
                                                                const float lambda, float* __restrict__ dL_dimg,
                                                                double* __restrict__ pairs) {
  __shared__ WindowLds hv[3];
  __shared__ double sh[WG_WAVES];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * WIN_TX, y0 = blockIdx.y * WIN_TY;
  const size_t plane = (size_t)c * H * W;
  const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * WIN_HO;
  const float gain = HAS_E ? exposure[2 * c] : 1.f, bias = HAS_E ? exposure[2 * c + 1] : 0.f;
  double s_w;
  float px[WIN_FLAT], py[WIN_FLAT], pw[WIN_FLAT];  // img / gt / w at this thread's output pixels (flattened order)
  {
    const float* const planes[3] = {mapA + plane, mapB + plane, mapC + plane};
    float v[3][WIN_IN];
    window_load_columns(planes, H, W, x0, y0, v);
#pragma unroll
    for (int it = 0; it < WIN_FLAT; it++) {  // (pixels outside the image or the tile are never used: any valid address)
      const int e = it * 256 + (int)threadIdx.x;
      const int row = e / WIN_TX, col = e - row * WIN_TX;
      const int off = min(y0 + row, H - 1) * W + min(x0 + col, W - 1);
      px[it] = img[plane + off];
      py[it] = gt[plane + off];
    }
    window_vertical<3, true>(win, hv, [&](int i, float(&m)[3]) { m[0] = v[0][i]; m[1] = v[1][i]; m[2] = v[2][i]; });
  }
  __syncthreads();
  {  // the weights are requested here, behind the vertical pass's registers, and arrive during the horizontal pass
    int off[WIN_FLAT];
#pragma unroll
    for (int it = 0; it < WIN_FLAT; it++) {
      const int e = it * 256 + (int)threadIdx.x;
      const int row = e / WIN_TX, col = e - row * WIN_TX;
      off[it] = min(y0 + row, H - 1) * W + min(x0 + col, W - 1);
    }
    pixel_weights(weights, acc, acc_min, off, pw);
    s_w = weight_thread_sum(partials, nper);
  }
  float t[3][WIN_HO];
  window_horizontal<3, true>(win, hv, t);
  __syncthreads();  // (everyone has read hv)
#pragma unroll
  for (int o = 0; o < WIN_HO; o++) { hv[0][r][c0 + o] = t[0][o]; hv[1][r][c0 + o] = t[1][o]; hv[2][r][c0 + o] = t[2][o]; }
  s_w = wave_sum(s_w);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s_w;
  __syncthreads();
  const float inv_n = inv_weight(C, weight_total(sh));
  const float k_l1 = (1.f - lambda) * inv_n, k_ssim = lambda * inv_n;
  double sum_gx = 0.0, sum_g = 0.0;
#pragma unroll
  for (int it = 0; it < WIN_FLAT; it++) {
    const int e = it * 256 + (int)threadIdx.x;
    const int row = e / WIN_TX, col = e - row * WIN_TX;
    const int gx = x0 + col, gy = y0 + row;
    if (e < WIN_TX * WIN_TY && gx < W && gy < H) {
      const float x = HAS_E ? __builtin_fmaf(gain, px[it], bias) : px[it], y = py[it];
      const float d = x - y;
      // w sign(d), exact; torch: abs'(0) = 0.  +0 at w = 0 whatever d is: an unweighted pixel's data reaches no output bit
      const float wsgn = d > 0.f ? pw[it] : (d < 0.f && pw[it] > 0.f ? -pw[it] : 0.f);
      const float inner = __builtin_fmaf(y, hv[2][row][col], __builtin_fmaf(x + x, hv[1][row][col], hv[0][row][col]));
      const float G = __builtin_fmaf(k_l1, wsgn, -(k_ssim * inner));
      dL_dimg[plane + (size_t)gy * W + gx] = HAS_E ? gain * G : G;
      if (HAS_E) {
        sum_gx += (double)G * (double)px[it];
        sum_g += (double)G;
      }
    }
  }
  if (!HAS_E) return;
  sum_gx = block_sum(sum_gx, sh);
  sum_g = block_sum(sum_g, sh);
  if (threadIdx.x == 0) {
    const size_t u = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    pairs[2 * u] = sum_gx;
    pairs[2 * u + 1] = sum_g;
  }
}

// One workgroup, launched last.  {l1, ssim} as k_exposure_loss_finish narrows them, L in its contraction; the squared
// error per channel as k_metrics_finalize sums it, over S instead of H W; dL_dexposure as k_exposure_loss_finish sums it
// (the same thread-strided float64 sums and tree, the three of a channel side by side in one pass of the tree).
__global__ __launch_bounds__(1024) void k_weighted_loss_finish(const float* __restrict__ partials, const int nper,
                                                               const int C, const float lambda,
                                                               float* __restrict__ out6,
                                                               const double* __restrict__ pairs,
                                                               float* __restrict__ dL_dexposure) {
  __shared__ double r[3][1024];
  __shared__ double sh[WG_WAVES];
  {
    const double s_w = wave_sum(weight_thread_sum(partials, nper));
    if (threadIdx.x < 256 && (threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s_w;
  }
  __syncthreads();
  const double S = weight_total(sh);
  double t[2] = {0.0, 0.0};
  const int nblocks = nper * C;
  for (int i = threadIdx.x; i < nblocks; i += 1024) {
    t[0] += partials[WPART_ * i]; t[1] += partials[WPART_ * i + 1];
  }
  tree_sum_1024(t, r);
  double psnr_sum = 0.0, mse_sum = 0.0;  // (thread 0's)
  for (int c = 0; c < C; c++) {           // per channel ONE tree: the squared error and, with a gradient, the pair
    const float* p = partials + (size_t)c * nper * WPART_;
    const double* pp = pairs + (size_t)c * nper * 2;
    double q[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nper; i += 1024) {
      q[0] += p[WPART_ * i + 2];
      if (dL_dexposure) { q[1] += pp[2 * i]; q[2] += pp[2 * i + 1]; }
    }
    tree_sum_1024(q, r);
    if (threadIdx.x == 0) {
      if (S > 0.0) {  // metrics.hip's rule in float64; mse_c == 0 -> 1 / 0 = +inf, as there
        const double mse_c = q[0] / S;
        psnr_sum += 20.0 * log10(1.0 / sqrt(mse_c));
        mse_sum += mse_c;
      }
      if (dL_dexposure) {
        dL_dexposure[2 * c] = (float)q[1];
        dL_dexposure[2 * c + 1] = (float)q[2];
      }
    }
  }
  if (threadIdx.x == 0) {
    if (S > 0.0) {
      const float inv_n = inv_weight(C, S);
      const float l1 = (float)(t[0] * inv_n), ssim = (float)(t[1] * inv_n);
      out6[0] = __builtin_fmaf(1.f - lambda, l1, lambda * (1.f - ssim));
      out6[1] = l1;
      out6[2] = ssim;
      out6[3] = (float)S;
      out6[4] = (float)(mse_sum / (double)C);
      out6[5] = (float)(psnr_sum / (double)C);
    } else {  // nothing is supervised
      out6[0] = out6[1] = out6[2] = out6[3] = out6[4] = 0.f;
      out6[5] = INFINITY;
    }
  }
}

// three maps, four floats per unit, and behind them (16-byte aligned inside a workspace of any address) one float64
// pair per unit
struct WeightedCarve {
  float* maps[3];
  float* partials;
  size_t tail_off;
  WeightedCarve(char* ws, int C, int H, int W) {
    Carver cv(ws);
    const size_t n = (size_t)C * H * W;
    for (int k = 0; k < 3; k++) maps[k] = cv.take<float>(n);
    partials = cv.take<float>(WindowGrid(C, H, W).units * WPART_);
    tail_off = align_up(cv.off);
  }
};

static size_t weighted_loss_workspace_bytes(int C, int H, int W) {
  return WeightedCarve(nullptr, C, H, W).tail_off + WindowGrid(C, H, W).units * 2 * sizeof(double) + 16;
}

static hipError_t launch_weighted_loss(int C, int H, int W, const float* img, const float* gt, const float* weights,
                                       const float* acc, float acc_min, const float* exposure, const float* window11,
                                       float lambda, float* out6, float* dL_dimg, float* dL_dexposure, char* workspace,
                                       hipStream_t s) {
  const WeightedCarve cv(workspace, C, H, W);
  const WindowGrid wg(C, H, W);
  double* pairs = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace + cv.tail_off) + 15u) & ~(uintptr_t)15u);
  const int nper = (int)(wg.grid.x * wg.grid.y);
  const Window win(window11);
  {
    ProfScope ps(K_EXPOSURE_LOSS_FWD, s);
    hipLaunchKernelGGL(exposure ? k_weighted_loss_forward<true> : k_weighted_loss_forward<false>, wg.grid, dim3(256), 0,
                       s, C, H, W, img, gt, weights, acc, acc_min, exposure, win, cv.maps[0], cv.maps[1], cv.maps[2],
                       cv.partials);
  }
  if (dL_dimg) {
    ProfScope ps(K_EXPOSURE_LOSS_BWD, s);
    hipLaunchKernelGGL(exposure ? k_weighted_loss_backward<true> : k_weighted_loss_backward<false>, wg.grid, dim3(256),
                       0, s, C, H, W, img, gt, weights, acc, acc_min, exposure, win, cv.maps[0], cv.maps[1], cv.maps[2],
                       cv.partials, nper, lambda, dL_dimg, pairs);
  }
  {
    ProfScope ps(K_EXPOSURE_LOSS_FINISH, s);
    hipLaunchKernelGGL(k_weighted_loss_finish, dim3(1), dim3(1024), 0, s, cv.partials, nper, C, lambda, out6, pairs,
                       dL_dexposure);
  }
  return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_weighted_loss_workspace(int channels, int height, int width) {
  if (channels <= 0 || height <= 0 || width <= 0 || !plane_fits(height, width, 0x7fffffffull)) return 0;
  return weighted_loss_workspace_bytes(channels, height, width);
}

int gsr_weighted_loss(int channels, int height, int width, const float* img, const float* gt, const float* weights,
                      const float* acc, float acc_min, const float* exposure, const float* window11_host,
                      float lambda_dssim, float* out6, float* dL_dimg, float* dL_dexposure, char* workspace,
                      size_t workspace_bytes, void* stream_) {
  clear_error();
  if (channels <= 0 || height <= 0 || width <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x7fffffffull)) return e;  // (32-bit offsets inside a plane)
  if (!img || !gt || !window11_host || !out6 || !workspace) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (dL_dexposure && !exposure) return fail(GSR_ERR_INVALID_ARGUMENT, "dL_dexposure without an exposure");
  if (exposure && !dL_dimg != !dL_dexposure)
    return fail(GSR_ERR_INVALID_ARGUMENT, "dL_dimg and dL_dexposure: both or neither");
  if (acc && !(fabsf(acc_min) <= 3.402823466e38f)) return fail(GSR_ERR_INVALID_ARGUMENT, "acc_min must be finite");
  if (int e = check_workspace(workspace_bytes, weighted_loss_workspace_bytes(channels, height, width))) return e;
  HIP_TRY(launch_weighted_loss(channels, height, width, img, gt, weights, acc, acc_min, exposure, window11_host,
                               lambda_dssim, out6, dL_dimg, dL_dexposure, workspace, (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
