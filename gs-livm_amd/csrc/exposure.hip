// exposure.hip -- per-keyframe exposure compensation, fused into the photometric loss (an extension: the reference has
// no such term).  A keyframe of an auto-exposure camera is the scene's radiance up to an affine map per channel,
//
//   x'(p) = fma(g_c, x(p), b_c)            exposure[c] = (g_c, b_c), identity (1, 0)
//   L     = (1 - lambda) * mean|x' - gt| + lambda * (1 - mean(SSIM(x', gt)))             (loss.hip's L, taken on x')
//
// and with G(p) = dL/dx'(p):   dL/dx(p) = g_c G(p),   dL/dg_c = sum_p G(p) x(p)  (the ORIGINAL x),   dL/db_c = sum_p G(p).
// The gain enters linearly (no transcendental on the device): a host restates x' exactly, and a log-gain is exp() on C
// numbers in the host's autograd.
//   k_exposure_loss_forward   k_loss_forward's arithmetic in its order, x' formed on load for in-image pixels only: the
//                             padding is conv2d's on the compensated image -- zero, not b_c
//   k_exposure_loss_backward  k_loss_backward's arithmetic on x' -> G; stores g_c G; G and G x widened to float64 and
//                             added per thread, wave and workgroup in block_sum's order: one float64 pair per work unit
//   k_exposure_loss_finish    one workgroup: {L, l1, ssim} as k_loss_finalize writes them, and dL_dexposure[c] from the
//                             channel's contiguous range of float64 pairs, narrowed once
//   k_apply_exposure          out = fma(g_c, x, b_c) over [C][H][W] (evaluation and export), 16-byte accesses where the
//                             addresses allow
// Deterministic: no atomics, fixed-order reductions.  The window passes are gsr_window.hpp's, the float64 sums
// gsr_workgroup.hpp's; built with loss.hip's flags (build.py).
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_window.hpp"

namespace gsr {

__global__ __launch_bounds__(256) void k_exposure_loss_forward(const int C, const int H, const int W,
                                                               const float* __restrict__ img,
                                                               const float* __restrict__ gt,
                                                               const float* __restrict__ exposure, const Window win,
                                                               float* __restrict__ mapA, float* __restrict__ mapB,
                                                               float* __restrict__ mapC, float* __restrict__ partials) {
  __shared__ WindowLds hv[4];  // vertically filtered moments
  __shared__ float red[2][4];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * WIN_TX, y0 = blockIdx.y * WIN_TY;
  const size_t plane = (size_t)c * H * W;
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const float gain = exposure[2 * c], bias = exposure[2 * c + 1];
  float sums[2] = {0.f, 0.f};  // |x' - y|, SSIM
  {
    const float* const planes[2] = {img + plane, gt + plane};
    float v[2][WIN_IN];
    const bool col_in = window_load_columns(planes, H, W, x0, y0, v);
#pragma unroll
    for (int i = 0; i < WIN_IN; i++) {  // x' inside the image; the padding stays 0 (fma(g, 0, b) would make it b)
      const int gy = y0 + WIN_SEG * seg - WIN_HALO + i;
      v[0][i] = col_in && gy >= 0 && gy < H ? __builtin_fmaf(gain, v[0][i], bias) : 0.f;
    }
    window_vertical<4, false>(win, hv, [&](int i, float(&m)[4]) {
      const float x = v[0][i], y = v[1][i];
      m[0] = x; m[1] = y; m[2] = __builtin_fmaf(y, y, x * x); m[3] = x * y;
    });
    if (lane >= WIN_HALO && lane < WIN_HALO + WIN_TX && col_in) {  // the L1 term of this thread's own eight output pixels
#pragma unroll
      for (int o = 0; o < WIN_SEG; o++)
        if (y0 + WIN_SEG * seg + o < H) sums[0] += fabsf(v[0][o + WIN_HALO] - v[1][o + WIN_HALO]);
    }
  }
  __syncthreads();
  {
    const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * WIN_HO;
    float m[4][WIN_HO];
    window_horizontal<4, false>(win, hv, m);
    const int gy = y0 + r;
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
        const float sv = n1 * n2 * inv;
        const float ds_dmu1 = 2.f * n2 * (mu2 * d1 - mu1 * n1) * inv * r1;
        const float ds_ds1 = -sv * r2;
        const float ds_ds12 = 2.f * n1 * inv;
        oa[o] = ds_dmu1 - 2.f * mu1 * ds_ds1 - mu2 * ds_ds12;
        ob[o] = ds_ds1;
        oc[o] = ds_ds12;
        sums[1] += sv;
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
  window_store_partials(sums, red, partials);  // one partial pair per workgroup
}

// G(p) = dL/dx'(p) is k_loss_backward's expression at x' = fma(g, x, b); the image gradient is g G.  The two exposure
// sums run over values the thread already holds: G and the ORIGINAL x, widened to float64 (their product is exact).
// pairs[2 u] = sum G x, pairs[2 u + 1] = sum G of work unit u, units ordered by channel (blockIdx.z major).
__global__ __launch_bounds__(256) void k_exposure_loss_backward(const int C, const int H, const int W,
                                                                const float* __restrict__ img,
                                                                const float* __restrict__ gt,
                                                                const float* __restrict__ exposure, const Window win,
                                                                const float* __restrict__ mapA,
                                                                const float* __restrict__ mapB,
                                                                const float* __restrict__ mapC, const float inv_n,
                                                                const float lambda, float* __restrict__ dL_dimg,
                                                                double* __restrict__ pairs) {
  __shared__ WindowLds hv[3];
  __shared__ double sh[WG_WAVES];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * WIN_TX, y0 = blockIdx.y * WIN_TY;
  const size_t plane = (size_t)c * H * W;
  const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * WIN_HO;
  const float gain = exposure[2 * c], bias = exposure[2 * c + 1];
  float px[WIN_FLAT], py[WIN_FLAT];  // img / gt at this thread's output pixels (flattened order), requested with the maps
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
  float t[3][WIN_HO];
  window_horizontal<3, true>(win, hv, t);
  __syncthreads();  // (everyone has read hv)
#pragma unroll
  for (int o = 0; o < WIN_HO; o++) { hv[0][r][c0 + o] = t[0][o]; hv[1][r][c0 + o] = t[1][o]; hv[2][r][c0 + o] = t[2][o]; }
  __syncthreads();
  double sum_gx = 0.0, sum_g = 0.0;
#pragma unroll
  for (int it = 0; it < WIN_FLAT; it++) {
    const int e = it * 256 + (int)threadIdx.x;
    const int row = e / WIN_TX, col = e - row * WIN_TX;
    const int gx = x0 + col, gy = y0 + row;
    if (e < WIN_TX * WIN_TY && gx < W && gy < H) {
      const float x = __builtin_fmaf(gain, px[it], bias), y = py[it];
      const float d = x - y;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);  // torch: abs'(0) = 0
      const float G = (1.f - lambda) * inv_n * sgn -
                      lambda * inv_n * (hv[0][row][col] + 2.f * x * hv[1][row][col] + y * hv[2][row][col]);
      dL_dimg[plane + (size_t)gy * W + gx] = gain * G;
      sum_gx += (double)G * (double)px[it];
      sum_g += (double)G;
    }
  }
  sum_gx = block_sum(sum_gx, sh);
  sum_g = block_sum(sum_g, sh);
  if (threadIdx.x == 0) {
    const size_t u = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    pairs[2 * u] = sum_gx;
    pairs[2 * u + 1] = sum_g;
  }
}

// One workgroup, launched last.  The three scalars are k_loss_finalize's, sum for sum; then, with a gradient, channel c's
// nper pairs (thread-strided float64 sums, then the tree) -> dL_dexposure[c] = (dL/dg_c, dL/db_c).
__global__ __launch_bounds__(1024) void k_exposure_loss_finish(const float* __restrict__ partials, const int nper,
                                                               const int C, const float inv_n, const float lambda,
                                                               float* __restrict__ out3,
                                                               const double* __restrict__ pairs,
                                                               float* __restrict__ dL_dexposure) {
  __shared__ double r[2][1024];
  double t[2] = {0.0, 0.0};
  const int nblocks = nper * C;
  for (int i = threadIdx.x; i < nblocks; i += 1024) {
    const float2 v = reinterpret_cast<const float2*>(partials)[i];
    t[0] += v.x; t[1] += v.y;
  }
  tree_sum_1024(t, r);
  if (threadIdx.x == 0) {
    const float l1 = (float)(t[0] * inv_n), ssim = (float)(t[1] * inv_n);
    out3[0] = (1.f - lambda) * l1 + lambda * (1.f - ssim);
    out3[1] = l1;
    out3[2] = ssim;
  }
  if (!dL_dexposure) return;
  for (int c = 0; c < C; c++) {
    const double* p = pairs + (size_t)c * nper * 2;
    double q[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nper; i += 1024) { q[0] += p[2 * i]; q[1] += p[2 * i + 1]; }
    tree_sum_1024(q, r);
    if (threadIdx.x == 0) {
      dL_dexposure[2 * c] = (float)q[0];
      dL_dexposure[2 * c + 1] = (float)q[1];
    }
  }
}

// Channel blockIdx.y's plane of n floats: `head` scalars up to the first 16-byte boundary of img (out sits at the same
// phase), nvec float4s, the rest scalars; with head == n (the phases differ, or the plane is short) everything is scalar.
// A thread reads what it writes and nothing else, so out == img is allowed; hence no __restrict__ on the two.
__global__ __launch_bounds__(256) void k_apply_exposure(const int n, const float* img, const float* __restrict__ exposure,
                                                        float* out, const int vec) {
  const int c = blockIdx.y;
  const float gain = exposure[2 * c], bias = exposure[2 * c + 1];
  const float* src = img + (size_t)c * n;
  float* dst = out + (size_t)c * n;
  const int head = vec ? min(n, (int)((16u - ((uint32_t)reinterpret_cast<uintptr_t>(src) & 15u)) & 15u) >> 2) : n;
  const int nvec = (n - head) >> 2;
  const int t = (int)min(blockIdx.x * 256u + threadIdx.x, 0x7fffffffu);  // (n < 2^31 - 1: such a thread has no element)
  if (t < nvec) {
    const float4 v = *reinterpret_cast<const float4*>(src + head + 4 * (size_t)t);
    float4 o;
    o.x = __builtin_fmaf(gain, v.x, bias); o.y = __builtin_fmaf(gain, v.y, bias);
    o.z = __builtin_fmaf(gain, v.z, bias); o.w = __builtin_fmaf(gain, v.w, bias);
    *reinterpret_cast<float4*>(dst + head + 4 * (size_t)t) = o;
    return;
  }
  const long long s = t - nvec;  // the scalars: the head, then the tail behind the float4s
  const long long i = s < head ? s : s + 4ll * nvec;
  if (i < n) dst[i] = __builtin_fmaf(gain, src[i], bias);
}

// the plain loss's carve (three maps, one float pair per unit) and one float64 pair per unit behind it, with the slack
// to align the doubles inside a workspace of any address
static inline size_t exposure_carve(Carver& cv, int C, int H, int W, float** maps3, float** partials) {
  const size_t n = (size_t)C * H * W;
  for (int k = 0; k < 3; k++) maps3[k] = cv.take<float>(n);
  *partials = cv.take<float>(WindowGrid(C, H, W).units * 2);
  return align_up(cv.off);
}

static size_t exposure_loss_workspace_bytes(int C, int H, int W) {
  Carver cv(nullptr);
  float *maps[3], *partials;
  return exposure_carve(cv, C, H, W, maps, &partials) + WindowGrid(C, H, W).units * 2 * sizeof(double) + 16;
}

static hipError_t launch_exposure_loss(int C, int H, int W, const float* img, const float* gt, const float* exposure,
                                       const float* window11, float lambda, float* loss_out3, float* dL_dimg,
                                       float* dL_dexposure, char* workspace, hipStream_t s) {
  Carver cv(workspace);
  float *maps[3], *partials;
  const size_t pairs_off = exposure_carve(cv, C, H, W, maps, &partials);
  double* pairs = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace + pairs_off) + 15u) & ~(uintptr_t)15u);
  const WindowGrid wg(C, H, W);
  const int nper = (int)(wg.grid.x * wg.grid.y);
  const Window win(window11);
  const float inv_n = (float)(1.0 / (double)((size_t)C * H * W));
  {
    ProfScope ps(K_EXPOSURE_LOSS_FWD, s);
    hipLaunchKernelGGL(k_exposure_loss_forward, wg.grid, dim3(256), 0, s, C, H, W, img, gt, exposure, win, maps[0],
                       maps[1], maps[2], partials);
  }
  if (dL_dimg) {  // (first: the render backward waits for this one, nobody on the stream for the finish)
    ProfScope ps(K_EXPOSURE_LOSS_BWD, s);
    hipLaunchKernelGGL(k_exposure_loss_backward, wg.grid, dim3(256), 0, s, C, H, W, img, gt, exposure, win, maps[0],
                       maps[1], maps[2], inv_n, lambda, dL_dimg, pairs);
  }
  {
    ProfScope ps(K_EXPOSURE_LOSS_FINISH, s);
    hipLaunchKernelGGL(k_exposure_loss_finish, dim3(1), dim3(1024), 0, s, partials, nper, C, inv_n, lambda, loss_out3,
                       pairs, dL_dimg ? dL_dexposure : nullptr);
  }
  return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_exposure_loss_workspace(int channels, int height, int width) {
  if (channels <= 0 || height <= 0 || width <= 0 || !plane_fits(height, width, 0x7fffffffull)) return 0;
  return exposure_loss_workspace_bytes(channels, height, width);
}

int gsr_exposure_loss(int channels, int height, int width, const float* img, const float* gt, const float* exposure,
                      const float* window11_host, float lambda_dssim, float* loss_out3, float* dL_dimg,
                      float* dL_dexposure, char* workspace, size_t workspace_bytes, void* stream_) {
  clear_error();
  if (channels <= 0 || height <= 0 || width <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x7fffffffull)) return e;  // (32-bit offsets inside a plane)
  if (!img || !gt || !exposure || !window11_host || !loss_out3 || !workspace)
    return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (!dL_dimg != !dL_dexposure)
    return fail(GSR_ERR_INVALID_ARGUMENT, "dL_dimg and dL_dexposure: both or neither");
  if (int e = check_workspace(workspace_bytes, exposure_loss_workspace_bytes(channels, height, width))) return e;
  HIP_TRY(launch_exposure_loss(channels, height, width, img, gt, exposure, window11_host, lambda_dssim, loss_out3,
                               dL_dimg, dL_dexposure, workspace, (hipStream_t)stream_));
  return GSR_OK;
}

int gsr_apply_exposure(int channels, int height, int width, const float* img, const float* exposure, float* out,
                       void* stream_) {
  clear_error();
  if (channels <= 0 || height <= 0 || width <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x7fffffffull)) return e;
  if (!img || !exposure || !out) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_aligned4(reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(exposure) |
                             reinterpret_cast<uintptr_t>(out)))
    return e;
  hipStream_t s = (hipStream_t)stream_;
  const int n = height * width;  // (H W < 2^31)
  // 16-byte accesses need img and out at the same phase; then every plane has at most 3 + 3 scalars
  const int vec = ((reinterpret_cast<uintptr_t>(img) ^ reinterpret_cast<uintptr_t>(out)) & 15u) == 0 && n >= 8;
  const unsigned threads = vec ? (unsigned)(n / 4 + 6) : (unsigned)n;
  ProfScope ps(K_APPLY_EXPOSURE, s);
  hipLaunchKernelGGL(k_apply_exposure, dim3((threads + 255u) / 256u, channels), dim3(256), 0, s, n, img, exposure, out,
                     vec);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
