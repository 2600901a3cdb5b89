// lidar.hip -- LiDAR depth supervision: a sweep's z-buffer in a keyframe's view (once per keyframe) and the masked
// depth L1 of a render against it, fused, with the gradients towards the rasterizer's depth and silhouette outputs
// (per view per optimiser iteration).  An extension: the reference has no such term (its rasterizer's backward drops
// dL/ddepth); it is the first consumer named for gsr_backward_depth.
//
// 1. gsr_lidar_depth_image.  Per point x (world):
//   p = R x + t, z = p.z                              [R | t] = T_cw, x_c = R x_w + t
//   (X, Y) = (K p).xy / (K p).z                       N = M (x, 1) with M = K [R | t] composed on the host in double and
//                                                     rounded once (lidar_compose, gsr_lidar_project.hpp), as delta.hip's matrices
//   (ix, iy) = (floor(X + 0.5), floor(Y + 0.5))       pixel u covers [u - 0.5, u + 0.5): the rasterizer's ndc2Pix
//   dropped: a coordinate of x, z, X or Y not finite; z <= min_depth; z > max_depth; |X| or |Y| beyond 2^30 (tested
//   before any conversion to an integer, as delta_cell); the pixel outside the image
//   lidar_depth[iy][ix] = the SMALLEST z of the points of the pixel, 0 where there is none
// A kept z is a positive finite float, and the bits of positive floats order like the floats: the minimum is taken with
// a 32-bit unsigned integer vector atomic on the image itself (no workspace), which commutes -- the image does not
// depend on the order of the points or of the waves, bit for bit.  No float atomics.  The two counts are integer atomic
// adds (one per wave), which commute too.
// Three launches on the caller's stream (one when n == 0):
//   k_lidar_clear    thread = pixel: the "empty" word (all ones: above the bits of every float); zeroes counts2
//   k_lidar_splat    thread = point: the atomic minimum; counts the points kept
//   k_lidar_convert  thread = pixel: empty -> 0.0f (every other word already IS the float); counts the pixels hit
//
// 2. gsr_lidar_depth_loss.  D = sum z alpha T and A = sum alpha T are the rasterizer's second and third outputs.
//   supervised: lidar_depth > 0 and A >= acc_min      (false for NaN)
//   e = D / A - z_L,  L = lambda sum|e| / max(n_sup, 1)
//   dL/dD = c sign(e) / A,  dL/dA = -c sign(e) D / A^2,  c = lambda / n_sup,  sign(0) = 0 as loss.hip; 0 elsewhere
// The normaliser is the supervised count, known on the device only, so the gradients are a launch of their own behind
// the finish.  The sums are per-workgroup f64 partials added in one fixed order (block_sum's tree, gsr_workgroup.hpp)
// and narrowed once: bitwise reproducible.  Three launches (two without gradients), no host synchronisation, no allocation:
//   k_lidar_loss_forward  thread = pixel: |e| and the mask; per-workgroup f64 sums and counts into the workspace
//   k_lidar_loss_finish   one workgroup: the partials in a fixed order; out3; c into the workspace
//   k_lidar_loss_grads    thread = pixel: both gradients, every element written
// Bounds: every thread tests its index against the count; a pixel index comes from coordinates that were tested
// against +-2^30 and then against the image before the atomic.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_lidar_project.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

struct LidarWorkspace {
  double* abs_part;   // [nblocks]
  int* cnt_part;      // [nblocks]
  float* scale;       // [1] c = lambda / n_sup (0 when nothing is supervised)
  size_t bytes;
  static LidarWorkspace carve(char* base, int H, int W) {
    const size_t N = (size_t)H * W, nblocks = (N + 255) / 256;
    // (the caller's workspace need not be aligned: as DeltaWorkspace)
    char* b = base ? reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(base))) : nullptr;
    Carver cv(b);
    LidarWorkspace w;
    w.abs_part = cv.take<double>(nblocks);
    w.cnt_part = cv.take<int>(nblocks);
    w.scale = cv.take<float>(1);
    w.bytes = align_up(cv.off) + ALIGN;
    return w;
  }
};

constexpr unsigned int LIDAR_EMPTY_ = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void k_lidar_clear(const int N, const unsigned int word,
                                                     unsigned int* __restrict__ image, int* __restrict__ counts2) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i < 2 && counts2) counts2[i] = 0;
  if (i < N) image[i] = word;
}

__global__ __launch_bounds__(256) void k_lidar_splat(const int n, const int W, const int H, const LidarCam cam,
                                                     const float min_depth, const float max_depth,
                                                     const float* __restrict__ points,
                                                     unsigned int* __restrict__ image, int* __restrict__ counts2) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  int kept = 0;
  if (i < n) {
    const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], w = points[3 * (size_t)i + 2];
    LidarHit h;   // (the projection and the drop rule: gsr_lidar_project.hpp, shared with seed.hip)
    if (lidar_project(cam, x, y, w, min_depth, max_depth, W, H, h)) {
      kept = 1;
      // z > min_depth >= 0: a positive float, whose bits order like the float (result unused: no return)
      atomicMin(&image[(size_t)h.iy * W + h.ix], __float_as_uint(h.z));
    }
  }
  if (counts2) {
    kept = wave_sum(kept);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&counts2[0], kept);
  }
}

__global__ __launch_bounds__(256) void k_lidar_convert(const int N, unsigned int* __restrict__ image,
                                                       int* __restrict__ counts2) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  int hit = 0;
  if (i < N) {
    if (image[i] == LIDAR_EMPTY_) image[i] = 0u;  // 0.0f
    else hit = 1;
  }
  if (counts2) {
    hit = wave_sum(hit);
    if ((threadIdx.x & 63) == 0 && hit) atomicAdd(&counts2[1], hit);
  }
}

__global__ __launch_bounds__(256) void k_lidar_loss_forward(const int N, const float acc_min,
                                                            const float* __restrict__ depth,
                                                            const float* __restrict__ acc,
                                                            const float* __restrict__ lidar,
                                                            double* __restrict__ abs_part, int* __restrict__ cnt_part) {
  __shared__ double shsum[4];
  __shared__ int shcnt[4];
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  float ae = 0.f;
  int on = 0;
  if (i < N) {
    const float zl = lidar[i], a = acc[i];
    on = (zl > 0.f && a >= acc_min) ? 1 : 0;
    if (on) ae = fabsf(depth[i] / a - zl);
  }
  double s = (double)ae;
  block_sum_pair(s, on, shsum, shcnt);
  if (threadIdx.x == 0) {
    abs_part[blockIdx.x] = s;
    cnt_part[blockIdx.x] = on;
  }
}

__global__ __launch_bounds__(256) void k_lidar_loss_finish(const int N, const int nblocks, const float lambda,
                                                           const double* __restrict__ abs_part,
                                                           const int* __restrict__ cnt_part, float* __restrict__ out3,
                                                           float* __restrict__ scale) {
  __shared__ double shsum[4];
  // thread-strided over the partials, then the workgroup tree -- one fixed order (the counts are exact in double)
  double as, cs;
  partial_pairs_sum(abs_part, cnt_part, nblocks, shsum, as, cs);
  if (threadIdx.x == 0) {
    const float mean_abs = cs > 0.0 ? (float)(as / cs) : 0.f;
    out3[0] = cs > 0.0 ? lambda * mean_abs : 0.f;
    out3[1] = mean_abs;
    out3[2] = (float)(cs / (double)N);
    *scale = cs > 0.0 ? (float)((double)lambda / cs) : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_lidar_loss_grads(const int N, const float acc_min,
                                                          const float* __restrict__ depth,
                                                          const float* __restrict__ acc,
                                                          const float* __restrict__ lidar,
                                                          const float* __restrict__ scale,
                                                          float* __restrict__ dL_ddepth, float* __restrict__ dL_dacc) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= N) return;
  const float c = *scale;
  const float zl = lidar[i], a = acc[i];
  float gd = 0.f, ga = 0.f;
  if (zl > 0.f && a >= acc_min) {
    const float q = depth[i] / a;
    const float e = q - zl;
    const float g = (float)((e > 0.f) - (e < 0.f));
    if (g != 0.f) {
      gd = (c * g) / a;
      ga = -gd * q;
    }
  }
  if (dL_ddepth) dL_ddepth[i] = gd;
  if (dL_dacc) dL_dacc[i] = ga;
}

static hipError_t launch_lidar_depth_image(int n, const float* points_world, const float* T_cw12, const float* K9,
                                           int H, int W, float min_depth, float max_depth, float* lidar_depth,
                                           int* counts2, hipStream_t s) {
  const int N = H * W, nblocks = (int)(((long long)N + 255) / 256);
  unsigned int* image = reinterpret_cast<unsigned int*>(lidar_depth);
  {
    ProfScope ps(K_LIDAR_CLEAR, s);
    hipLaunchKernelGGL(k_lidar_clear, dim3(nblocks), dim3(256), 0, s, N, n ? LIDAR_EMPTY_ : 0u, image, counts2);
  }
  if (n == 0) return hipGetLastError();
  const LidarCam cam = lidar_compose(T_cw12, K9);
  {
    ProfScope ps(K_LIDAR_SPLAT, s);
    hipLaunchKernelGGL(k_lidar_splat, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, s, n, W, H, cam, min_depth, max_depth,
                       points_world, image, counts2);
  }
  {
    ProfScope ps(K_LIDAR_CONVERT, s);
    hipLaunchKernelGGL(k_lidar_convert, dim3(nblocks), dim3(256), 0, s, N, image, counts2);
  }
  return hipGetLastError();
}

static size_t lidar_loss_workspace_bytes(int H, int W) { return LidarWorkspace::carve(nullptr, H, W).bytes; }

static hipError_t launch_lidar_depth_loss(int H, int W, const float* depth, const float* acc,
                                          const float* lidar_depth, float acc_min, float lambda, float* out3,
                                          float* dL_ddepth, float* dL_dacc, char* workspace, hipStream_t s) {
  const int N = H * W, nblocks = (int)(((long long)N + 255) / 256);
  const LidarWorkspace w = LidarWorkspace::carve(workspace, H, W);
  {
    ProfScope ps(K_LIDAR_LOSS_FWD, s);
    hipLaunchKernelGGL(k_lidar_loss_forward, dim3(nblocks), dim3(256), 0, s, N, acc_min, depth, acc, lidar_depth,
                       w.abs_part, w.cnt_part);
  }
  {
    ProfScope ps(K_LIDAR_LOSS_FINISH, s);
    hipLaunchKernelGGL(k_lidar_loss_finish, dim3(1), dim3(256), 0, s, N, nblocks, lambda, w.abs_part, w.cnt_part,
                       out3, w.scale);
  }
  if (dL_ddepth || dL_dacc) {
    ProfScope ps(K_LIDAR_LOSS_GRADS, s);
    hipLaunchKernelGGL(k_lidar_loss_grads, dim3(nblocks), dim3(256), 0, s, N, acc_min, depth, acc, lidar_depth,
                       w.scale, dL_ddepth, dL_dacc);
  }
  return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_lidar_depth_image(int n, const float* points_world, const float* T_cw12, const float* K9, int height, int width,
                          float min_depth, float max_depth, float* lidar_depth, int* counts2, void* stream_) {
  clear_error();
  if (n < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad n");
  if (height < 1 || width < 1) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x80000000ull)) return e;  // (32-bit pixel indices)
  if ((n > 0 && !points_world) || !T_cw12 || !K9 || !lidar_depth) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (!(min_depth >= 0.f && min_depth <= 3.402823466e38f))  // (false for NaN and +inf)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad min_depth: finite and >= 0");
  if (!(max_depth > min_depth)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad max_depth: greater than min_depth");
  HIP_TRY(launch_lidar_depth_image(n, points_world, T_cw12, K9, height, width, min_depth, max_depth, lidar_depth,
                                   counts2, (hipStream_t)stream_));
  return GSR_OK;
}

size_t gsr_lidar_depth_loss_workspace(int height, int width) {
  if (height < 1 || width < 1 || !plane_fits(height, width, 0x80000000ull)) return 0;
  return lidar_loss_workspace_bytes(height, width);
}

int gsr_lidar_depth_loss(int height, int width, const float* depth, const float* acc, const float* lidar_depth,
                         float acc_min, float lambda, float* out3, float* dL_ddepth, float* dL_dacc, char* workspace,
                         size_t workspace_bytes, void* stream_) {
  clear_error();
  if (height < 1 || width < 1) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x80000000ull)) return e;  // (32-bit pixel indices)
  if (!depth || !acc || !lidar_depth || !out3 || !workspace) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (!(acc_min > 0.f && acc_min <= 3.402823466e38f))  // (false for NaN and +inf)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad acc_min: finite and > 0");
  if (int e = check_workspace(workspace_bytes, lidar_loss_workspace_bytes(height, width))) return e;
  HIP_TRY(launch_lidar_depth_loss(height, width, depth, acc, lidar_depth, acc_min, lambda, out3, dL_ddepth, dL_dacc,
                                  workspace, (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
