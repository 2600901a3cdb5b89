// loss.hip -- the photometric loss that follows every render in GS-LIVM's optimiser, fused
// ("next" row 2):
//
//   L = (1 - lambda) * mean|img - gt|  +  lambda * (1 - mean(SSIM(img, gt)))
//
// Reference: gaussian_splatting::l1_loss and ::ssim (include/gs/gs/loss_utils.cuh:11-13, 43-70), combined at
// src/liw/lioOptimization.cpp:1705-1710 with lambda = lambda_dssim (config/basic_common.yaml:63).  The
// reference runs five grouped 11x11 conv2d + ~15 elementwise kernels forward and their autograd backward per
// view; here:
//   k_loss_forward   one pass: separable 11-tap window over (x, y, x^2 + y^2, xy) -- vertical pass in registers
//                    straight from coalesced loads, horizontal pass through LDS --, SSIM map, the three per-pixel
//                    derivative maps the backward needs, per-workgroup partial sums of |x-y| and SSIM
//   k_loss_finalize  fixed-order sum of the partials -> {loss, l1, ssim}   (deterministic: no float atomics)
//   k_loss_backward  dL/dimg = (1-lambda)/N * sign(x-y) - lambda/N * [convT(A) + 2x convT(B) + y convT(C)]
// The window is whatever 1-D kernel the caller passes (the 2-D window of the reference is its outer product,
// loss_utils.cuh:33-37) -- including the reference's own, which is NOT symmetric (gaussian() floors
// (x - window_size)/2, loss_utils.cuh:24-31), so correlation (forward) and its transpose (backward) are kept
// apart.  Zero padding of window/2, as conv2d(padding = window_size / 2).
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_window.hpp"

namespace gsr {

// mu(q) = sum_k w[k] * f(q + k - 5)   (cross-correlation, zero padded): what conv2d computes.  SSIM needs the two
// variances only through their sum (d2 = sigma1^2 + sigma2^2 + C2), so four windowed moments are carried, not five:
// E[x], E[y], E[x^2 + y^2], E[xy].
__global__ __launch_bounds__(256) void k_loss_forward(const int C, const int H, const int W,
                                                      const float* __restrict__ img, const float* __restrict__ gt,
                                                      const Window win, float* __restrict__ mapA,
                                                      float* __restrict__ mapB, float* __restrict__ mapC,
                                                      float* __restrict__ partials) {
  __shared__ WindowLds hv[4];  // vertically filtered moments
  __shared__ float red[2][4];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * WIN_TX, y0 = blockIdx.y * WIN_TY;
  const size_t plane = (size_t)c * H * W;
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  float sums[2] = {0.f, 0.f};  // |x - y|, SSIM
  {
    const float* const planes[2] = {img + plane, gt + plane};
    float v[2][WIN_IN];
    const bool col_in = window_load_columns(planes, H, W, x0, y0, v);
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
      if (c0 + o < WIN_TX && gx < W && gy < H) {
        const float mu1 = m[0][o], mu2 = m[1][o], e_sum = m[2][o], e12 = m[3][o];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s12 = e12 - mu12;
        const float n1 = 2.f * mu12 + SSIM_C1, n2 = 2.f * s12 + SSIM_C2;
        const float d1 = mu1_sq + mu2_sq + SSIM_C1, d2 = (e_sum - mu1_sq - mu2_sq) + SSIM_C2;
        const float r1 = __builtin_amdgcn_rcpf(d1), r2 = __builtin_amdgcn_rcpf(d2);  // (1 ulp; d1, d2 >= C1, C2 > 0 up to rounding)
        const float inv = r1 * r2;
        const float sv = n1 * n2 * inv;
        // partials of s w.r.t. (mu1, sigma1_sq, sigma12) at fixed img2
        const float ds_dmu1 = 2.f * n2 * (mu2 * d1 - mu1 * n1) * inv * r1;  // d/dmu1 of n1/d1 times n2/d2
        const float ds_ds1 = -sv * r2;
        const float ds_ds12 = 2.f * n1 * inv;
        // total derivative through sigma1_sq = E[x^2] - mu1^2 and sigma12 = E[xy] - mu1*mu2:
        oa[o] = ds_dmu1 - 2.f * mu1 * ds_ds1 - mu2 * ds_ds12;
        ob[o] = ds_ds1;
        oc[o] = ds_ds12;
        sums[1] += sv;
      }
    }
    // A thread's seven outputs are adjacent in a row: stored from here, a wave's store would be 64 separate 4-byte
    // accesses (measured: the kernel was bound by them, not by its arithmetic).  The maps change hands through LDS
    // and leave in the flattened order of the tile, 54-float row segments to consecutive lanes.
    __syncthreads();  // (everyone has read hv)
#pragma unroll
    for (int o = 0; o < WIN_HO; o++) { hv[0][r][c0 + o] = oa[o]; hv[1][r][c0 + o] = ob[o]; hv[2][r][c0 + o] = oc[o]; }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < WIN_FLAT; it++) {
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

__global__ __launch_bounds__(1024) void k_loss_finalize(const float* __restrict__ partials, const int nblocks,
                                                        const float inv_n, const float lambda,
                                                        float* __restrict__ out3) {
  // one workgroup, fixed association order (thread-strided partial sums in f64, then a tree): deterministic
  __shared__ double r[2][1024];
  double t[2] = {0.0, 0.0};
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
}

// dL/dx(p) = (1-lambda)/N sign(x-y) - lambda/N * sum_q w(p - q + 5) * [A(q) + 2 x(p) B(q) + y(p) C(q)]
// i.e. the transposed correlation: taps are read flipped.  Same work unit and passes as the forward, over the three
// derivative maps.
__global__ __launch_bounds__(256) void k_loss_backward(const int C, const int H, const int W,
                                                       const float* __restrict__ img, const float* __restrict__ gt,
                                                       const Window win, const float* __restrict__ mapA,
                                                       const float* __restrict__ mapB, const float* __restrict__ mapC,
                                                       const float inv_n, const float lambda,
                                                       float* __restrict__ dL_dimg) {
  __shared__ WindowLds hv[3];
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * WIN_TX, y0 = blockIdx.y * WIN_TY;
  const size_t plane = (size_t)c * H * W;
  const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * WIN_HO;
  float px[WIN_FLAT], py[WIN_FLAT];  // img / gt at this thread's output pixels (flattened order), requested with the maps
  {
    const float* const planes[3] = {mapA + plane, mapB + plane, mapC + plane};
    float v[3][WIN_IN];
    window_load_columns(planes, H, W, x0, y0, v);
#pragma unroll
    for (int it = 0; it < WIN_FLAT; it++) {  // (pixels outside the image or the tile are never stored: any valid address)
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
  // the filtered maps change hands through LDS (as the forward's outputs do): the image is read and the gradient
  // written in the flattened order of the tile, 54-float row segments to consecutive lanes
  __syncthreads();  // (everyone has read hv)
#pragma unroll
  for (int o = 0; o < WIN_HO; o++) { hv[0][r][c0 + o] = t[0][o]; hv[1][r][c0 + o] = t[1][o]; hv[2][r][c0 + o] = t[2][o]; }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < WIN_FLAT; it++) {
    const int e = it * 256 + (int)threadIdx.x;
    const int row = e / WIN_TX, col = e - row * WIN_TX;
    const int gx = x0 + col, gy = y0 + row;
    if (e < WIN_TX * WIN_TY && gx < W && gy < H) {
      const float x = px[it], y = py[it];
      const float d = x - y;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);  // torch: abs'(0) = 0
      dL_dimg[plane + (size_t)gy * W + gx] =
          (1.f - lambda) * inv_n * sgn -
          lambda * inv_n * (hv[0][row][col] + 2.f * x * hv[1][row][col] + y * hv[2][row][col]);
    }
  }
}

static size_t loss_workspace_bytes(int C, int H, int W) {
  const size_t maps = 3 * align_up((size_t)C * H * W * sizeof(float));
  return maps + align_up(WindowGrid(C, H, W).units * 2 * sizeof(float)) + ALIGN;
}

static hipError_t launch_photometric_loss(int C, int H, int W, const float* img, const float* gt,
                                          const float* window11, float lambda, float* loss_out3, float* dL_dimg,
                                          char* workspace, hipStream_t s) {
  Carver cv(workspace);
  const size_t n = (size_t)C * H * W;
  float* mapA = cv.take<float>(n);
  float* mapB = cv.take<float>(n);
  float* mapC = cv.take<float>(n);
  const WindowGrid wg(C, H, W);
  const dim3 grid = wg.grid;
  const int nblocks = (int)wg.units;
  float* partials = cv.take<float>((size_t)nblocks * 2);
  const Window win(window11);
  const float inv_n = (float)(1.0 / (double)n);
  {
    ProfScope ps(K_LOSS_FWD, s);
    hipLaunchKernelGGL(k_loss_forward, grid, dim3(256), 0, s, C, H, W, img, gt, win, mapA, mapB, mapC, partials);
  }
  if (dL_dimg) {  // (first: the render backward waits for this one, nobody on the stream for the three scalars)
    ProfScope ps(K_LOSS_BWD, s);
    hipLaunchKernelGGL(k_loss_backward, grid, dim3(256), 0, s, C, H, W, img, gt, win, mapA, mapB, mapC, inv_n, lambda,
                       dL_dimg);
  }
  {
    ProfScope ps(K_LOSS_FINALIZE, s);
    hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(1024), 0, s, partials, nblocks, inv_n, lambda, loss_out3);
  }
  return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_photometric_loss_workspace(int channels, int height, int width) {
  if (channels <= 0 || height <= 0 || width <= 0) return 0;
  return loss_workspace_bytes(channels, height, width);
}

int gsr_photometric_loss(int channels, int height, int width, const float* img, const float* gt,
                         const float* window11_host, float lambda_dssim, float* loss_out3, float* dL_dimg,
                         char* workspace, size_t workspace_bytes, void* stream_) {
  clear_error();
  if (channels <= 0 || height <= 0 || width <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x7fffffffull)) return e;  // (32-bit offsets inside a plane)
  if (!img || !gt || !window11_host || !loss_out3 || !workspace) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_workspace(workspace_bytes, loss_workspace_bytes(channels, height, width))) return e;
  HIP_TRY(launch_photometric_loss(channels, height, width, img, gt, window11_host, lambda_dssim, loss_out3, dL_dimg,
                                  workspace, (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
