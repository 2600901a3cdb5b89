// metrics.hip -- the evaluation pass that follows a forward-only render, fused: what GS-LIVM runs on the device around
// the rasterizer when it measures its own result (saveRender, src/liw/lioOptimization.cpp:2182-2245, and the status line
// of optimize_vis, :1739-1776):
//
//   psnr = mean_c 20 log10(1 / sqrt(mse_c)),  mse_c = mean over H W of (img - gt)^2 in channel c
//          (gaussian_splatting::psnr, include/gs/gs/loss_utils.cuh:89-93: the mean of the per-channel PSNRs)
//   ssim = mean(SSIM(img, gt))                (::ssim, loss_utils.cuh:43-70)
//   8-bit images for cv::imwrite              (tensor2CvMat3X :2113-2136, tensor2CvMat2X :2150-2164)
//
//   k_metrics_forward   the forward of loss.hip without its outputs per pixel: the same 54 x 32 work unit and separable
//                       11-tap window, no derivative maps, one trip through LDS; per workgroup three partial sums:
//                       |x - y|, SSIM, (x - y)^2
//   k_metrics_finalize  fixed-order float64 sums of the partials (the squared error per channel) -> {psnr, ssim, l1, mse}
//                       and, optionally, their accumulation into four device doubles (a keyframe sweep's running sums)
//   k_pack_image_u8     [3][H][W] f32 -> interleaved 8-bit [H][W][3] (RGB or BGR) with a row pitch
//   k_pack_depth_u8     [H][W] f32 -> 8-bit [H][W] with a row pitch, round-half-even of d * (255 / max_depth)
// Deterministic: no atomics, fixed-order reductions.
#include <math.h>

#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_window.hpp"

namespace gsr {

constexpr int MPART_ = 3;  // partials per workgroup: sum|x - y|, sum SSIM, sum (x - y)^2

// k_loss_forward's passes and order of operations (the window unit of gsr_window.hpp: vertical pass in registers from
// coalesced loads, one trip through LDS, horizontal pass seven outputs to a thread); nothing is stored per pixel.
__global__ __launch_bounds__(256) void k_metrics_forward(const int C, const int H, const int W,
                                                         const float* __restrict__ img, const float* __restrict__ gt,
                                                         const Window win, float* __restrict__ partials) {
  __shared__ WindowLds hv[4];  // vertically filtered moments
  __shared__ float red[MPART_][4];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * WIN_TX, y0 = blockIdx.y * WIN_TY;
  const size_t plane = (size_t)c * H * W;
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  float sums[MPART_] = {0.f, 0.f, 0.f};
  {
    const float* const planes[2] = {img + plane, gt + plane};
    float v[2][WIN_IN];
    const bool col_in = window_load_columns(planes, H, W, x0, y0, v);
    window_vertical<4, false>(win, hv, [&](int i, float(&m)[4]) {
      const float x = v[0][i], y = v[1][i];
      m[0] = x; m[1] = y; m[2] = __builtin_fmaf(y, y, x * x); m[3] = x * y;
    });
    if (lane >= WIN_HALO && lane < WIN_HALO + WIN_TX && col_in) {  // the L1 and squared-error terms of this thread's own eight pixels
#pragma unroll
      for (int o = 0; o < WIN_SEG; o++)
        if (y0 + WIN_SEG * seg + o < H) {
          const float d = v[0][o + WIN_HALO] - v[1][o + WIN_HALO];
          sums[0] += fabsf(d);
          sums[2] = __builtin_fmaf(d, d, sums[2]);
        }
    }
  }
  __syncthreads();
  {
    const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * WIN_HO;
    float m[4][WIN_HO];
    window_horizontal<4, false>(win, hv, m);
    const int gy = y0 + r;
#pragma unroll
    for (int o = 0; o < WIN_HO; o++) {
      const int gx = x0 + c0 + o;
      if (c0 + o < WIN_TX && gx < W && gy < H) {
        const float mu1 = m[0][o], mu2 = m[1][o], e_sum = m[2][o], e12 = m[3][o];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s12 = e12 - mu12;
        const float n1 = 2.f * mu12 + SSIM_C1, n2 = 2.f * s12 + SSIM_C2;
        const float d1 = mu1_sq + mu2_sq + SSIM_C1, d2 = (e_sum - mu1_sq - mu2_sq) + SSIM_C2;
        const float r1 = __builtin_amdgcn_rcpf(d1), r2 = __builtin_amdgcn_rcpf(d2);  // (1 ulp, as in k_loss_forward)
        sums[1] += n1 * n2 * (r1 * r2);
      }
    }
  }
  window_store_partials(sums, red, partials);  // three partials per workgroup, in the block order of k_loss_forward's
}

// One workgroup, fixed association order (thread-strided sums in f64, then a tree): deterministic.  The squared error
// is summed per channel; |x - y| and SSIM run through all channels.  partials: [C][nper][3] floats, element-aligned.
__global__ __launch_bounds__(1024) void k_metrics_finalize(const float* __restrict__ partials, const int nper, const int C,
                                                           const float inv_n, const double plane_px,
                                                           float* __restrict__ out4, double* __restrict__ totals) {
  __shared__ double r12[2][1024], r3[1][1024];
  double ab[2] = {0.0, 0.0};
  for (size_t i = threadIdx.x; i < (size_t)nper * C; i += 1024) {  // (the order of k_loss_finalize)
    ab[0] += partials[MPART_ * i]; ab[1] += partials[MPART_ * i + 1];
  }
  double psnr_sum = 0.0, mse_sum = 0.0;  // (thread 0's)
  for (int c = 0; c < C; c++) {
    const float* p = partials + (size_t)c * nper * MPART_;
    double q[1] = {0.0};
    for (int i = threadIdx.x; i < nper; i += 1024) q[0] += p[MPART_ * i + 2];
    tree_sum_1024(q, r3);
    if (threadIdx.x == 0) {  // loss_utils.cuh:89-93 in float64; mse_c == 0 -> 1 / 0 = +inf, as there
      const double mse_c = q[0] / plane_px;
      psnr_sum += 20.0 * log10(1.0 / sqrt(mse_c));
      mse_sum += mse_c;
    }
  }
  tree_sum_1024(ab, r12);
  if (threadIdx.x == 0) {
    const float psnr = (float)(psnr_sum / (double)C);
    const float ssim = (float)(ab[1] * inv_n), l1 = (float)(ab[0] * inv_n);  // (as k_loss_finalize narrows them)
    const float mse = (float)(mse_sum / (double)C);
    out4[0] = psnr; out4[1] = ssim; out4[2] = l1; out4[3] = mse;
    if (totals) {  // the values as stored, widened: the running sums are the float64 sum of the per-frame outputs
      totals[0] += (double)psnr; totals[1] += (double)ssim; totals[2] += (double)l1; totals[3] += 1.0;
    }
  }
}

// tensor2CvMat3X's arithmetic: x * 255 (one f32 multiply), clamp to [0, 255], truncate; NaN -> 0 (fmaxf drops it)
__device__ __forceinline__ uint32_t unit_to_u8(float x) { return (uint32_t)(int)fminf(fmaxf(x * 255.f, 0.f), 255.f); }

// A thread owns four consecutive pixels of a row: 12 output bytes, three 4-byte stores where the row's first byte is
// 4-byte aligned (12 q keeps that), byte stores for the last, partial group of a row and for misaligned rows.
// vec_in: the three planes can be read 16 bytes at a time (base 16-byte aligned, W a multiple of 4).
__global__ __launch_bounds__(256) void k_pack_image_u8(const int H, const int W, const float* __restrict__ img,
                                                       const int bgr, unsigned char* __restrict__ out,
                                                       const size_t pitch, const int groups_per_row,
                                                       const uint32_t ngroups, const int vec_in) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= ngroups) return;
  const int y = (int)(g / (uint32_t)groups_per_row);
  const int px = 4 * (int)(g - (uint32_t)y * (uint32_t)groups_per_row);
  const int n = min(4, W - px);  // 1 .. 4 pixels
  const size_t hw = (size_t)H * W;
  const size_t in0 = (size_t)y * W + px;
  float v[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const float* p = img + ch * hw + in0;
    if (vec_in) {
      const float4 t = *reinterpret_cast<const float4*>(p);
      v[ch][0] = t.x; v[ch][1] = t.y; v[ch][2] = t.z; v[ch][3] = t.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) v[ch][k] = p[min(k, n - 1)];  // (clamped: never read behind the row)
    }
  }
  uint32_t b[12];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t c0 = unit_to_u8(v[0][k]), c1 = unit_to_u8(v[1][k]), c2 = unit_to_u8(v[2][k]);
    b[3 * k] = bgr ? c2 : c0; b[3 * k + 1] = c1; b[3 * k + 2] = bgr ? c0 : c2;
  }
  unsigned char* row = out + (size_t)y * pitch;
  unsigned char* dst = row + 3 * (size_t)px;
  if (n == 4 && (reinterpret_cast<uintptr_t>(row) & 3) == 0) {
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int j = 0; j < 3; j++) d32[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 12; k++)
      if (k < 3 * n) dst[k] = (unsigned char)b[k];
  }
}

// cv::Mat::convertTo(CV_8U) of depth * (255 / max_depth) as OpenCV documents it: round half to even, saturate; NaN -> 0.
// A thread owns four consecutive pixels of a row: one 4-byte store where the row's first byte is 4-byte aligned.
__global__ __launch_bounds__(256) void k_pack_depth_u8(const int H, const int W, const float* __restrict__ depth,
                                                       const float scale, unsigned char* __restrict__ out,
                                                       const size_t pitch, const int groups_per_row,
                                                       const uint32_t ngroups, const int vec_in) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= ngroups) return;
  const int y = (int)(g / (uint32_t)groups_per_row);
  const int px = 4 * (int)(g - (uint32_t)y * (uint32_t)groups_per_row);
  const int n = min(4, W - px);
  const float* p = depth + (size_t)y * W + px;
  float v[4];
  if (vec_in) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = p[min(k, n - 1)];
  }
  uint32_t b[4];
#pragma unroll
  for (int k = 0; k < 4; k++) b[k] = (uint32_t)(int)fminf(fmaxf(rintf(v[k] * scale), 0.f), 255.f);
  unsigned char* row = out + (size_t)y * pitch;
  unsigned char* dst = row + px;
  if (n == 4 && (reinterpret_cast<uintptr_t>(row) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(dst) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < n) dst[k] = (unsigned char)b[k];
  }
}

// the partials only: three floats per work unit, element alignment
static size_t metrics_workspace_bytes(int C, int H, int W) {
  return WindowGrid(C, H, W).units * MPART_ * sizeof(float);
}

static hipError_t launch_image_metrics(int C, int H, int W, const float* img, const float* gt, const float* window11,
                                       float* out4, double* totals, char* workspace, hipStream_t s) {
  float* partials = reinterpret_cast<float*>(workspace);
  const dim3 grid = WindowGrid(C, H, W).grid;
  const Window win(window11);
  const float inv_n = (float)(1.0 / (double)((size_t)C * H * W));
  {
    ProfScope ps(K_METRICS_FWD, s);
    hipLaunchKernelGGL(k_metrics_forward, grid, dim3(256), 0, s, C, H, W, img, gt, win, partials);
  }
  {
    ProfScope ps(K_METRICS_FINALIZE, s);
    hipLaunchKernelGGL(k_metrics_finalize, dim3(1), dim3(1024), 0, s, partials, (int)(grid.x * grid.y), C, inv_n,
                       (double)H * (double)W, out4, totals);
  }
  return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_image_metrics_workspace(int channels, int height, int width) {
  if (channels <= 0 || height <= 0 || width <= 0 || !plane_fits(height, width, 0x7fffffffull)) return 0;
  return metrics_workspace_bytes(channels, height, width);
}

int gsr_image_metrics(int channels, int height, int width, const float* img, const float* gt,
                      const float* window11_host, float* out4, double* totals, char* workspace, size_t workspace_bytes,
                      void* stream_) {
  clear_error();
  if (channels <= 0 || height <= 0 || width <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x7fffffffull)) return e;  // (32-bit offsets inside a plane)
  if (!img || !gt || !window11_host || !out4 || !workspace) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_workspace(workspace_bytes, metrics_workspace_bytes(channels, height, width))) return e;
  HIP_TRY(launch_image_metrics(channels, height, width, img, gt, window11_host, out4, totals, workspace,
                               (hipStream_t)stream_));
  return GSR_OK;
}

int gsr_pack_image_u8(int height, int width, const float* img3, int bgr, unsigned char* out, size_t pitch_bytes,
                      void* stream_) {
  clear_error();
  if (height <= 0 || width <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x7fffffffull)) return e;
  if (!img3 || !out) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (pitch_bytes < 3 * (size_t)width)
    return fail(GSR_ERR_INVALID_ARGUMENT, "pitch too small: a row has %zu bytes", 3 * (size_t)width);
  hipStream_t s = (hipStream_t)stream_;
  const int gpr = (width + 3) / 4;
  const uint32_t ngroups = (uint32_t)((size_t)gpr * height);  // (H W < 2^31)
  const int vec_in = (reinterpret_cast<uintptr_t>(img3) & 15) == 0 && (width & 3) == 0;
  ProfScope ps(K_PACK_IMAGE_U8, s);
  hipLaunchKernelGGL(k_pack_image_u8, dim3((ngroups + 255) / 256), dim3(256), 0, s, height, width, img3, bgr ? 1 : 0,
                     out, pitch_bytes, gpr, ngroups, vec_in);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

int gsr_pack_depth_u8(int height, int width, const float* depth, float max_depth, unsigned char* out,
                      size_t pitch_bytes, void* stream_) {
  clear_error();
  if (height <= 0 || width <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x7fffffffull)) return e;
  if (!depth || !out) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (pitch_bytes < (size_t)width)
    return fail(GSR_ERR_INVALID_ARGUMENT, "pitch too small: a row has %zu bytes", (size_t)width);
  if (!(max_depth > 0.f) || !(max_depth <= 3.402823466e38f))
    return fail(GSR_ERR_INVALID_ARGUMENT, "max_depth must be positive and finite");
  hipStream_t s = (hipStream_t)stream_;
  const int gpr = (width + 3) / 4;
  const uint32_t ngroups = (uint32_t)((size_t)gpr * height);
  const int vec_in = (reinterpret_cast<uintptr_t>(depth) & 15) == 0 && (width & 3) == 0;
  const float scale = 255.0f / max_depth;  // formed in float32, as `depthMap * (255.0f / maxDepth)` (:2155)
  ProfScope ps(K_PACK_DEPTH_U8, s);
  hipLaunchKernelGGL(k_pack_depth_u8, dim3((ngroups + 255) / 256), dim3(256), 0, s, height, width, depth, scale, out,
                     pitch_bytes, gpr, ngroups, vec_in);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
