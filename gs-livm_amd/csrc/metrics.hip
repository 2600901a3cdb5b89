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

#include "gsr_internal.hpp"

namespace gsr {

// The work unit of loss.hip (its LW_ .. LSTRIDE_, restated: that file and its code object stay as they are).
constexpr int MW_ = 11;                    // window taps
constexpr int MR_ = MW_ / 2;               // halo
constexpr int MTX_ = 54, MTY_ = 32;        // outputs of one 256-thread workgroup
constexpr int MSEG_ = 8;                   // output rows per wave
constexpr int MIN_ = MSEG_ + 2 * MR_;      // 18 input rows per wave
constexpr int MHO_ = 7;                    // horizontal pass: outputs per thread
constexpr int MSTRIDE_ = 72;               // LDS row stride (conflict-free over a wave's 8 x 8, see loss.hip)
constexpr float M_SSIM_C1 = 0.01f * 0.01f, M_SSIM_C2 = 0.03f * 0.03f;  // loss_utils.cuh:8-9
constexpr int MPART_ = 3;                  // partials per workgroup: sum|x - y|, sum SSIM, sum (x - y)^2

struct MetricsWindow { float w[MW_]; };

// Same passes and the same order of operations as k_loss_forward (vertical pass in registers from coalesced loads, one
// trip through LDS, horizontal pass seven outputs to a thread); nothing is stored per pixel.
__global__ __launch_bounds__(256) void k_metrics_forward(const int C, const int H, const int W,
                                                         const float* __restrict__ img, const float* __restrict__ gt,
                                                         const MetricsWindow win, float* __restrict__ partials) {
  __shared__ float hv[4][MTY_][MSTRIDE_];  // vertically filtered moments
  __shared__ float red[MPART_][4];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * MTX_, y0 = blockIdx.y * MTY_;
  const size_t plane = (size_t)c * H * W;
  const float* X = img + plane;
  const float* Y = gt + plane;
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  float l1 = 0.f, ss = 0.f, sq = 0.f;
  {
    const int gx = x0 - MR_ + lane;
    const bool col_in = gx >= 0 && gx < W;
    const int gxc = min(max(gx, 0), W - 1);
    float vx[MIN_], vy[MIN_];
#pragma unroll
    for (int i = 0; i < MIN_; i++) {  // (clamped addresses, unconditional loads, zero padding by select)
      const int gy = y0 + MSEG_ * seg - MR_ + i;
      const int off = min(max(gy, 0), H - 1) * W + gxc;
      const float a = X[off], b = Y[off];
      const bool in = col_in && gy >= 0 && gy < H;
      vx[i] = in ? a : 0.f;
      vy[i] = in ? b : 0.f;
    }
    float acc[MSEG_][4];
#pragma unroll
    for (int o = 0; o < MSEG_; o++) acc[o][0] = acc[o][1] = acc[o][2] = acc[o][3] = 0.f;
#pragma unroll
    for (int i = 0; i < MIN_; i++) {
      const float x = vx[i], y = vy[i];
      const float p2 = __builtin_fmaf(y, y, x * x), p3 = x * y;
#pragma unroll
      for (int o = 0; o < MSEG_; o++) {
        const int k = i - o;
        if (k >= 0 && k < MW_) {
          const float wk = win.w[k];
          acc[o][0] += wk * x; acc[o][1] += wk * y; acc[o][2] += wk * p2; acc[o][3] += wk * p3;
        }
      }
    }
#pragma unroll
    for (int o = 0; o < MSEG_; o++) {
#pragma unroll
      for (int q = 0; q < 4; q++) hv[q][MSEG_ * seg + o][lane] = acc[o][q];
    }
    if (lane >= MR_ && lane < MR_ + MTX_ && col_in) {  // the L1 and squared-error terms of this thread's own eight pixels
#pragma unroll
      for (int o = 0; o < MSEG_; o++)
        if (y0 + MSEG_ * seg + o < H) {
          const float d = vx[o + MR_] - vy[o + MR_];
          l1 += fabsf(d);
          sq = __builtin_fmaf(d, d, sq);
        }
    }
  }
  __syncthreads();
  {
    const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * MHO_;
    float m[4][MHO_];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float v[MHO_ + MW_ - 1];
#pragma unroll
      for (int k = 0; k < MHO_ + MW_ - 1; k++) v[k] = hv[q][r][c0 + k];  // (the last group reads into the row padding)
#pragma unroll
      for (int o = 0; o < MHO_; o++) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < MW_; k++) a += win.w[k] * v[o + k];
        m[q][o] = a;
      }
    }
    const int gy = y0 + r;
#pragma unroll
    for (int o = 0; o < MHO_; o++) {
      const int gx = x0 + c0 + o;
      if (c0 + o < MTX_ && gx < W && gy < H) {
        const float mu1 = m[0][o], mu2 = m[1][o], e_sum = m[2][o], e12 = m[3][o];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s12 = e12 - mu12;
        const float n1 = 2.f * mu12 + M_SSIM_C1, n2 = 2.f * s12 + M_SSIM_C2;
        const float d1 = mu1_sq + mu2_sq + M_SSIM_C1, d2 = (e_sum - mu1_sq - mu2_sq) + M_SSIM_C2;
        const float r1 = __builtin_amdgcn_rcpf(d1), r2 = __builtin_amdgcn_rcpf(d2);  // (1 ulp, as in k_loss_forward)
        ss += n1 * n2 * (r1 * r2);
      }
    }
  }
  // fixed-order workgroup reduction -> three partials per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    l1 += __shfl_xor(l1, o, 64);
    ss += __shfl_xor(ss, o, 64);
    sq += __shfl_xor(sq, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = l1; red[1][threadIdx.x >> 6] = ss; red[2][threadIdx.x >> 6] = sq;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // ordered by channel (blockIdx.z major), as the partials of k_loss_forward
    const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#pragma unroll
    for (int q = 0; q < MPART_; q++)
      partials[MPART_ * b + q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  }
}

// One workgroup, fixed association order (thread-strided sums in f64, then a tree): deterministic.  The squared error
// is summed per channel; |x - y| and SSIM run through all channels.  partials: [C][nper][3] floats, element-aligned.
__global__ __launch_bounds__(1024) void k_metrics_finalize(const float* __restrict__ partials, const int nper, const int C,
                                                           const float inv_n, const double plane_px,
                                                           float* __restrict__ out4, double* __restrict__ totals) {
  __shared__ double r1[1024], r2[1024], r3[1024];
  double a = 0.0, b = 0.0;
  for (size_t i = threadIdx.x; i < (size_t)nper * C; i += 1024) {  // (the order of k_loss_finalize)
    a += partials[MPART_ * i]; b += partials[MPART_ * i + 1];
  }
  double psnr_sum = 0.0, mse_sum = 0.0;  // (thread 0's)
  for (int c = 0; c < C; c++) {
    const float* p = partials + (size_t)c * nper * MPART_;
    double q = 0.0;
    for (int i = threadIdx.x; i < nper; i += 1024) q += p[MPART_ * i + 2];
    r3[threadIdx.x] = q;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) r3[threadIdx.x] += r3[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) {  // loss_utils.cuh:89-93 in float64; mse_c == 0 -> 1 / 0 = +inf, as there
      const double mse_c = r3[0] / plane_px;
      psnr_sum += 20.0 * log10(1.0 / sqrt(mse_c));
      mse_sum += mse_c;
    }
    __syncthreads();  // (r3 is refilled by the next channel)
  }
  r1[threadIdx.x] = a; r2[threadIdx.x] = b;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float psnr = (float)(psnr_sum / (double)C);
    const float ssim = (float)(r2[0] * inv_n), l1 = (float)(r1[0] * inv_n);  // (as k_loss_finalize narrows them)
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

static size_t metrics_units(int C, int H, int W) {
  return (size_t)((W + MTX_ - 1) / MTX_) * ((H + MTY_ - 1) / MTY_) * C;
}

// the partials only: three floats per work unit, element alignment
size_t metrics_workspace_bytes(int C, int H, int W) { return metrics_units(C, H, W) * MPART_ * sizeof(float); }

hipError_t launch_image_metrics(int C, int H, int W, const float* img, const float* gt, const float* window11,
                                float* out4, double* totals, char* workspace, hipStream_t s) {
  float* partials = reinterpret_cast<float*>(workspace);
  const dim3 grid((W + MTX_ - 1) / MTX_, (H + MTY_ - 1) / MTY_, C);
  MetricsWindow win;
  for (int k = 0; k < MW_; k++) win.w[k] = window11[k];
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

hipError_t launch_pack_image_u8(int H, int W, const float* img3, int bgr, unsigned char* out, size_t pitch,
                                hipStream_t s) {
  const int gpr = (W + 3) / 4;
  const uint32_t ngroups = (uint32_t)((size_t)gpr * H);  // (H W < 2^31)
  const int vec_in = (reinterpret_cast<uintptr_t>(img3) & 15) == 0 && (W & 3) == 0;
  ProfScope ps(K_PACK_IMAGE_U8, s);
  hipLaunchKernelGGL(k_pack_image_u8, dim3((ngroups + 255) / 256), dim3(256), 0, s, H, W, img3, bgr ? 1 : 0, out, pitch,
                     gpr, ngroups, vec_in);
  return hipGetLastError();
}

hipError_t launch_pack_depth_u8(int H, int W, const float* depth, float max_depth, unsigned char* out, size_t pitch,
                                hipStream_t s) {
  const int gpr = (W + 3) / 4;
  const uint32_t ngroups = (uint32_t)((size_t)gpr * H);
  const int vec_in = (reinterpret_cast<uintptr_t>(depth) & 15) == 0 && (W & 3) == 0;
  const float scale = 255.0f / max_depth;  // formed in float32, as `depthMap * (255.0f / maxDepth)` (:2155)
  ProfScope ps(K_PACK_DEPTH_U8, s);
  hipLaunchKernelGGL(k_pack_depth_u8, dim3((ngroups + 255) / 256), dim3(256), 0, s, H, W, depth, scale, out, pitch, gpr,
                     ngroups, vec_in);
  return hipGetLastError();
}

}  // namespace gsr
