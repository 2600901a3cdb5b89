// normal.hip -- rendered normal maps and the depth-normal consistency loss (an extension: the reference has neither;
// 2DGS and PGSR hold the normals of the rendered depth to a normal map blended from the primitives' orientations).
//
// 1. gsr_blend_attributes.  The entry point of the attribute walk: out[c][pixel] = sum attr[splat][c] alpha T over the
//    splats the pixel took.  The kernel, k_attribute_tile, lives in render.hip beside k_contribution_tile, whose walk it
//    repeats with render.hip's device functions and compiler flags.
//
// 2. gsr_surfel_normals.  One launch, thread = row:
//   k*  = index of the smallest activated scale, n_w = column k* of R(q) (gsr_surfel_axis.hpp, shared with surfel.hip)
//   n_c = R_cw n_w,  p_c = R_cw x + t,  flipped when n_c . p_c > 0 (exactly 0: not flipped): the normal faces the camera
//   Every row is written, whatever the forward made of it.  [R | t] = T_cw travels by value.
//
// 3. gsr_normal_consistency_loss.  D = sum z alpha T and A = sum alpha T are the rasterizer's second and third outputs,
//    N = sum n_c alpha T the blended normal image (un-normalised).  At pixel (u, v):
//   z = D / A,  X = ((u - cx) z / fx, (v - cy) z / fy, z);  valid: A >= acc_min (false for NaN)
//   supervised: 1 <= u <= W-2, 1 <= v <= H-2; the pixel and its four neighbours valid; |z(nb) - z| <= jump_rel z for the
//   four (jump_rel = +inf: the gate is off, no comparison is made); |N| >= normal_min A; |c| > 0
//   a = X(u+1, v) - X(u-1, v),  b = X(u, v+1) - X(u, v-1),  c = b x a (towards the camera for a surface facing it)
//   rho = 1 - (N / |N|) . (c / |c|),  L = lambda sum rho / max(S, 1),  S = supervised pixels
//   Gradients towards D and A only (N is data, the gates are steps): with g_c = -(n_r - (n_r . n_d) n_d) / |c|,
//   drho/da = g_c x b and drho/db = a x g_c; z of pixel q enters the a of its W and E neighbours and the b of its N and
//   S neighbours with dX/dz = r_q = ((u - cx) / fx, (v - cy) / fy, 1):
//   g_z(q) = (lambda / S) r_q . (ga(u-1, v) - ga(u+1, v) + gb(u, v-1) - gb(u, v+1)),  dL/dD = g_z / A,  dL/dA = -g_z D / A^2
// Three launches (two without gradients), lidar.hip's shape, timed under its three ids (the profiler's id word is full):
//   k_normal_loss_forward  thread = pixel: the gates and rho; per-workgroup f64 sums and counts; with gradients asked
//                          for, the pixel's drho/da and drho/db are parked in the workspace (six planes of H W floats,
//                          zeros where the pixel is not supervised: 24 B written per pixel)
//   k_normal_loss_finish   one workgroup: the partials in a fixed order; out3; lambda / S into the workspace
//   k_normal_loss_grads    thread = pixel: a gather of the four neighbours' parked vectors in the fixed order W, E, N, S
//                          (48 B read per pixel); every element written, zeros where nothing flows.  No atomics.
// Bitwise reproducible; no host synchronisation, no allocation, the caller's stream only.  Every global access of a
// caller's array is a 4-byte one.  Bounds: every thread tests its index against the pixel count, and a neighbour is
// read only after the pixel's coordinates were tested against the image.
// Built with -ffp-contract=off (build.py): the column of R(q) has surfel.hip's bits, and every multiply-add of the
// normals kernel is an explicit __builtin_fmaf, as in gsr_lidar_project.hpp.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_surfel_axis.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

struct Tcw12 {  // [R | t], row-major 3 x 4, x_c = R x_w + t
  float m[12];
};

__global__ __launch_bounds__(WG_THREADS) void k_surfel_normals(const int P, const float* __restrict__ xyz,
                                                               const float* __restrict__ scaling,
                                                               const float* __restrict__ rotation, const Tcw12 T,
                                                               float* __restrict__ normals) {
  const int i = blockIdx.x * WG_THREADS + (int)threadIdx.x;
  if (i >= P) return;
  const size_t r3 = 3 * (size_t)i, r4 = 4 * (size_t)i;
  float smin;
  const int ks = surfel_thin_index(scaling[r3], scaling[r3 + 1], scaling[r3 + 2], smin);
  float n0, n1, n2;
  surfel_axis(ks, rotation[r4], rotation[r4 + 1], rotation[r4 + 2], rotation[r4 + 3], n0, n1, n2);
  const float x = xyz[r3], y = xyz[r3 + 1], z = xyz[r3 + 2];
  float nc[3], pc[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    nc[r] = __builtin_fmaf(T.m[4 * r], n0, __builtin_fmaf(T.m[4 * r + 1], n1, T.m[4 * r + 2] * n2));
    pc[r] = __builtin_fmaf(T.m[4 * r], x, __builtin_fmaf(T.m[4 * r + 1], y, __builtin_fmaf(T.m[4 * r + 2], z, T.m[4 * r + 3])));
  }
  const float d = __builtin_fmaf(nc[0], pc[0], __builtin_fmaf(nc[1], pc[1], nc[2] * pc[2]));
  const bool flip = d > 0.f;  // (the normal of the CAMERA-space axis: a test on n_w would ignore the view)
  normals[r3] = flip ? -nc[0] : nc[0];
  normals[r3 + 1] = flip ? -nc[1] : nc[1];
  normals[r3 + 2] = flip ? -nc[2] : nc[2];
}

struct NormalWorkspace {
  double* rho_part;  // [nblocks]
  int* cnt_part;     // [nblocks]
  float* scale;      // [1] lambda / S (0 when nothing is supervised)
  float* park;       // [6][H W] drho/da (planes 0..2) and drho/db (planes 3..5) of every pixel
  size_t bytes;
  static NormalWorkspace carve(char* base, int H, int W) {
    const size_t N = (size_t)H * W, nblocks = (N + 255) / 256;
    Carver cv = Carver::aligned(base);
    NormalWorkspace w;
    w.rho_part = cv.take<double>(nblocks);
    w.cnt_part = cv.take<int>(nblocks);
    w.scale = cv.take<float>(1);
    w.park = cv.take<float>(6 * N);
    w.bytes = cv.bytes();
    return w;
  }
};

struct NormalCam {
  float fx, fy, cx, cy;
};

__global__ __launch_bounds__(256) void k_normal_loss_forward(const int W, const int H, const NormalCam cam,
                                                             const float acc_min, const float normal_min,
                                                             const float jump_rel, const float* __restrict__ depth,
                                                             const float* __restrict__ acc,
                                                             const float* __restrict__ normals,
                                                             double* __restrict__ rho_part,
                                                             int* __restrict__ cnt_part, float* __restrict__ park) {
  __shared__ double shsum[4];
  __shared__ int shcnt[4];
  const int N = W * H;
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  float rho = 0.f;
  int on = 0;
  float ga[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f};
  if (i < N) {
    const int v = i / W, u = i - v * W;
    if (u >= 1 && u <= W - 2 && v >= 1 && v <= H - 2) {  // (the four neighbours are inside the image)
      const float Ac = acc[i], Ae = acc[i + 1], Aw = acc[i - 1], As = acc[i + W], An = acc[i - W];
      if (Ac >= acc_min && Ae >= acc_min && Aw >= acc_min && As >= acc_min && An >= acc_min) {
        const float zc = depth[i] / Ac, ze = depth[i + 1] / Ae, zw = depth[i - 1] / Aw, zs = depth[i + W] / As,
                    zn = depth[i - W] / An;
        const float lim = jump_rel * zc;
        const bool smooth = jump_rel == INFINITY || (fabsf(ze - zc) <= lim && fabsf(zw - zc) <= lim &&
                                                     fabsf(zs - zc) <= lim && fabsf(zn - zc) <= lim);
        const float N0 = normals[i], N1 = normals[(size_t)N + i], N2 = normals[2 * (size_t)N + i];
        const float nlen = sqrtf(N0 * N0 + N1 * N1 + N2 * N2);
        if (smooth && nlen >= normal_min * Ac) {  // (S is counted behind the |N| gate and the |c| gate)
          const float xu = (float)u - cam.cx, xe = (float)(u + 1) - cam.cx, xw = (float)(u - 1) - cam.cx;
          const float yv = (float)v - cam.cy, ys = (float)(v + 1) - cam.cy, yn = (float)(v - 1) - cam.cy;
          const float a0 = xe * ze / cam.fx - xw * zw / cam.fx, a1 = yv * ze / cam.fy - yv * zw / cam.fy, a2 = ze - zw;
          const float b0 = xu * zs / cam.fx - xu * zn / cam.fx, b1 = ys * zs / cam.fy - yn * zn / cam.fy, b2 = zs - zn;
          const float c0 = b1 * a2 - b2 * a1, c1 = b2 * a0 - b0 * a2, c2 = b0 * a1 - b1 * a0;  // c = b x a
          const float clen = sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
          if (clen > 0.f) {
            on = 1;
            const float d0 = c0 / clen, d1 = c1 / clen, d2 = c2 / clen;
            const float r0 = N0 / nlen, r1 = N1 / nlen, r2 = N2 / nlen;
            const float dot = r0 * d0 + r1 * d1 + r2 * d2;
            rho = 1.f - dot;
            // g_c = drho/dc = -(n_r - (n_r . n_d) n_d) / |c|;  drho/da = g_c x b,  drho/db = a x g_c
            const float g0 = -(r0 - dot * d0) / clen, g1 = -(r1 - dot * d1) / clen, g2 = -(r2 - dot * d2) / clen;
            ga[0] = g1 * b2 - g2 * b1; ga[1] = g2 * b0 - g0 * b2; ga[2] = g0 * b1 - g1 * b0;
            gb[0] = a1 * g2 - a2 * g1; gb[1] = a2 * g0 - a0 * g2; gb[2] = a0 * g1 - a1 * g0;
          }
        }
      }
    }
    if (park) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        park[(size_t)k * N + i] = ga[k];
        park[(size_t)(3 + k) * N + i] = gb[k];
      }
    }
  }
  double s = (double)rho;
  block_sum_pair(s, on, shsum, shcnt);
  if (threadIdx.x == 0) {
    rho_part[blockIdx.x] = s;
    cnt_part[blockIdx.x] = on;
  }
}

__global__ __launch_bounds__(256) void k_normal_loss_finish(const int N, const int nblocks, const float lambda,
                                                            const double* __restrict__ rho_part,
                                                            const int* __restrict__ cnt_part, float* __restrict__ out3,
                                                            float* __restrict__ scale) {
  __shared__ double shsum[4];
  double rs, cs;
  partial_pairs_sum(rho_part, cnt_part, nblocks, shsum, rs, cs);
  if (threadIdx.x == 0) {
    const float mean_rho = cs > 0.0 ? (float)(rs / cs) : 0.f;
    out3[0] = cs > 0.0 ? lambda * mean_rho : 0.f;
    out3[1] = mean_rho;
    out3[2] = (float)(cs / (double)N);
    *scale = cs > 0.0 ? (float)((double)lambda / cs) : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_normal_loss_grads(const int W, const int H, const NormalCam cam,
                                                           const float* __restrict__ depth,
                                                           const float* __restrict__ acc,
                                                           const float* __restrict__ park,
                                                           const float* __restrict__ scale,
                                                           float* __restrict__ dL_ddepth, float* __restrict__ dL_dacc) {
  const int N = W * H;
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= N) return;
  const int v = i / W, u = i - v * W;
  // z of this pixel is the E end of its W neighbour's a (+), the W end of its E neighbour's a (-), the S end of its N
  // neighbour's b (+) and the N end of its S neighbour's b (-): four additions in this order
  float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float* const pa = park + (size_t)k * N;
    const float* const pb = park + (size_t)(3 + k) * N;
    if (u >= 1) s[k] += pa[i - 1];
    if (u <= W - 2) s[k] -= pa[i + 1];
    if (v >= 1) s[k] += pb[i - W];
    if (v <= H - 2) s[k] -= pb[i + W];
  }
  const float rx = ((float)u - cam.cx) / cam.fx, ry = ((float)v - cam.cy) / cam.fy;
  const float gz = *scale * (rx * s[0] + ry * s[1] + s[2]);
  float gd = 0.f, gacc = 0.f;
  if (gz != 0.f) {  // (nothing flows: zeros, whatever D and A hold -- a NaN in A stays inside its own gate)
    const float a = acc[i];
    gd = gz / a;
    gacc = -gd * (depth[i] / a);
  }
  if (dL_ddepth) dL_ddepth[i] = gd;
  if (dL_dacc) dL_dacc[i] = gacc;
}

static size_t normal_workspace_bytes(int H, int W) { return NormalWorkspace::carve(nullptr, H, W).bytes; }

static hipError_t launch_normal_loss(int H, int W, const float* depth, const float* acc, const float* normals,
                                     const NormalCam cam, float acc_min, float normal_min, float jump_rel, float lambda,
                                     float* out3, float* dL_ddepth, float* dL_dacc, char* workspace, hipStream_t s) {
  const int N = H * W, nblocks = (int)(((long long)N + 255) / 256);
  const NormalWorkspace w = NormalWorkspace::carve(workspace, H, W);
  const bool grads = dL_ddepth || dL_dacc;
  {
    ProfScope ps(K_LIDAR_LOSS_FWD, s);
    hipLaunchKernelGGL(k_normal_loss_forward, dim3(nblocks), dim3(256), 0, s, W, H, cam, acc_min, normal_min, jump_rel,
                       depth, acc, normals, w.rho_part, w.cnt_part, grads ? w.park : nullptr);
  }
  {
    ProfScope ps(K_LIDAR_LOSS_FINISH, s);
    hipLaunchKernelGGL(k_normal_loss_finish, dim3(1), dim3(256), 0, s, N, nblocks, lambda, w.rho_part, w.cnt_part,
                       out3, w.scale);
  }
  if (grads) {
    ProfScope ps(K_LIDAR_LOSS_GRADS, s);
    hipLaunchKernelGGL(k_normal_loss_grads, dim3(nblocks), dim3(256), 0, s, W, H, cam, depth, acc, w.park, w.scale,
                       dL_ddepth, dL_dacc);
  }
  return hipGetLastError();
}

static const char* const kMisalignedWorkspace = "misaligned pointer: the workspace needs 8-byte alignment";

}  // namespace gsr

using namespace gsr;

// ---- the entry points.  The order of the checks is part of the contract (include/gsraster.h): shape and parameter
// range, then null pointers, then alignment (then the workspace's size).
extern "C" {

int gsr_blend_attributes(int P, int R, int width, int height, int channels, const float* attributes,
                         const char* geom_buffer, const char* binning_buffer, const char* image_buffer, float* out,
                         void* stream_) {
  clear_error();
  if (channels < 1 || channels > 4) return fail(GSR_ERR_INVALID_ARGUMENT, "bad channels: 1..4");
  if (P < 0 || R < 0 || width <= 0 || height <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P/R/width/height");
  if (int e = check_plane(height, width, 0x80000000ull)) return e;
  const bool walk = P > 0 && R > 0;
  if (!out || (walk && !attributes)) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (walk && (!geom_buffer || !binning_buffer || !image_buffer))
    return fail(GSR_ERR_INVALID_ARGUMENT, "null state blob");
  if (int e = check_aligned4((uintptr_t)out | (walk ? (uintptr_t)attributes : 0))) return e;
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_VISIBILITY, s);
  if (!walk) {  // nothing was blended: zeros, written by a fill; the blobs are not read
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)channels * (size_t)width * (size_t)height * sizeof(float), s));
    return GSR_OK;
  }
  FrameParams fp{};
  fp.P = P;
  fp.W = width;
  fp.H = height;
  fp.gx = (width + TILE - 1) / TILE;
  fp.gy = (height + TILE - 1) / TILE;
  const GeomState g = GeomState::carve(const_cast<char*>(geom_buffer), (size_t)P);
  const BinningState b = BinningState::carve(const_cast<char*>(binning_buffer), (size_t)R);
  const ImageState im = ImageState::carve(const_cast<char*>(image_buffer), width, height);
  HIP_TRY(launch_attributes(fp, g, b, im, channels, attributes, out, s));
  return GSR_OK;
}

int gsr_surfel_normals(int P, const float* xyz, const float* scaling, const float* rotation, const float* T_cw12,
                       float* normals, void* stream_) {
  clear_error();
  if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
  if (P == 0) return GSR_OK;
  if (!xyz || !scaling || !rotation || !T_cw12 || !normals) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_aligned4((uintptr_t)xyz | (uintptr_t)scaling | (uintptr_t)rotation | (uintptr_t)normals)) return e;
  Tcw12 T;
  for (int k = 0; k < 12; k++) T.m[k] = T_cw12[k];
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_VISIBILITY, s);
  hipLaunchKernelGGL(k_surfel_normals, dim3((unsigned)(((long long)P + WG_THREADS - 1) / WG_THREADS)), dim3(WG_THREADS),
                     0, s, P, xyz, scaling, rotation, T, normals);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

size_t gsr_normal_consistency_workspace(int height, int width) {
  if (height < 1 || width < 1 || !plane_fits(height, width, 0x80000000ull)) return 0;
  return normal_workspace_bytes(height, width);
}

int gsr_normal_consistency_loss(int height, int width, const float* depth, const float* acc, const float* normals,
                                float fx, float fy, float cx, float cy, float acc_min, float normal_min,
                                float jump_rel, float lambda, float* out3, float* dL_ddepth, float* dL_dacc,
                                char* workspace, size_t workspace_bytes, void* stream_) {
  clear_error();
  if (height < 1 || width < 1) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x80000000ull)) return e;  // (32-bit pixel indices)
  if (!(acc_min >= 0.f)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad acc_min: >= 0");  // (false for NaN)
  if (!(normal_min >= 0.f)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad normal_min: >= 0");
  if (!(lambda >= 0.f)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad lambda: >= 0");
  if (!(jump_rel >= 0.f)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad jump_rel: >= 0 (+inf: no gate)");
  auto finite_pos = [](float v) { return v > 0.f && v <= 3.402823466e38f; };  // (false for NaN and +inf)
  if (!finite_pos(fx) || !finite_pos(fy)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad fx / fy: finite and > 0");
  if (!depth || !acc || !normals || !out3 || !workspace) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_aligned4((uintptr_t)depth | (uintptr_t)acc | (uintptr_t)normals | (uintptr_t)out3 |
                             (uintptr_t)dL_ddepth | (uintptr_t)dL_dacc))
    return e;
  if ((uintptr_t)workspace & 7u) return fail(GSR_ERR_INVALID_ARGUMENT, "%s", kMisalignedWorkspace);
  if (int e = check_workspace(workspace_bytes, normal_workspace_bytes(height, width))) return e;
  const NormalCam cam{fx, fy, cx, cy};
  HIP_TRY(launch_normal_loss(height, width, depth, acc, normals, cam, acc_min, normal_min, jump_rel, lambda, out3,
                             dL_ddepth, dL_dacc, workspace, (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
