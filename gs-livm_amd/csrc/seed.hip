// seed.hip -- sweep admission: which points of a LiDAR sweep does the map, as a keyframe renders it, not explain yet,
// what colour is each of them in the keyframe's image, and how large is its pixel footprint.  The producer-side step in
// front of GrowableGaussians.add_new_pointcloud.  An extension: the reference seeds a voxel once whatever the map holds
// (src/gp3d/map.cpp:68-110) and colours the points on the host from the nearest pixel (src/liw/lioOptimization.cpp:66-70).
//
// Per point x (world), ONE reason code, decided in this order:
//   1 OUT         the drop rule of gsr_lidar_depth_image, bit for bit (lidar_project, gsr_lidar_project.hpp)
//   2 OCCLUDED    lidar_depth given: zmin = the smallest positive lidar_depth over |dx|, |dy| <= occlusion_radius around
//                 (ix, iy), clamped to the image; z - zmin > occlusion_tol z
//   3 EXPLAINED   depth = D and acc = A given, A >= acc_min (false for NaN: the silhouette is missing, the point goes on);
//   4 BEHIND      r = D / A;  r - z > depth_tol z: the measurement lies in front of the render, the point goes on;
//                 z - r > depth_tol z: 4;  anything else, a NaN r included: 3
//   5 DUPLICATE   one_per_pixel: among the points that got this far a pixel keeps the smallest (bits(z) << 32) | index --
//                 the nearest point, the lowest index among equal z; the others are 5
//   0 ADMITTED    everything else
// The admitted points are compacted stably (input order) into xyz / covs / rgb / index / pixel / z; rows at and behind
// the admitted count are not written.
//   covs    covs_in's row bit for bit, or sigma^2 I with sigma = ((footprint z) 2) / (fx + fy), off-diagonals exact zeros
//   rgb     bilinear at (X, Y), pixel centres at the integers, the four taps clamped to the image (border replication);
//           two horizontal lerps and one vertical, each a + t (b - a); the keyframe's exposure inverted, (v - b) / g;
//           then times 255.  No clamp.
//
// Launches on the caller's stream: FIVE with one_per_pixel, FOUR without, ONE when n == 0 (the scan, which zeroes the
// counts).  All are timed under k_visibility (the profiler's mask is full).
//   k_seed_clear     thread = pixel: the per-pixel plane to all ones (above every key)            [one_per_pixel only]
//   k_seed_classify  thread = point: codes 0..4 into the workspace; a survivor's key into its pixel (64-bit unsigned
//                    integer vector atomic minimum, result unused)
//   k_seed_resolve   thread = point: code 5 where the pixel holds another key; reasons[]; per-workgroup totals of
//                    every code (ballots)
//   k_seed_scan      ONE workgroup: exclusive scan of the admitted totals (scan_totals), counts6
//   k_seed_emit      thread = point: row = workgroup base + rank_in_block; the outputs of an admitted point
// Integer atomics only, and the minimum commutes: the same bits on every run whatever the order of the waves.  No
// workgroup waits for another.  The projection is recomputed in k_seed_emit rather than stored: same code, same bits.
// Bounds: every thread tests its index against the count; a pixel index comes from coordinates lidar_project tested
// against +-2^30 and then against the image; the occlusion window and the four colour taps are clamped to the image;
// an output row is workgroup base + rank < admitted <= n.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_lidar_project.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

constexpr int SEED_CODES = 6;   // admitted, out, occluded, explained, behind, duplicate
constexpr unsigned long long SEED_EMPTY_ = ~0ull;

struct SeedWorkspace {
  unsigned long long* plane;   // [H W] the smallest key of the pixel (one_per_pixel)
  int* totals;                 // [6][nblocks] per-workgroup count of each code; [0] -> its exclusive scan
  unsigned char* codes;        // [n]
  size_t bytes;
  static SeedWorkspace carve(char* base, int n, int H, int W) {
    const size_t N = (size_t)H * W, nblocks = ((size_t)n + WG_THREADS - 1) / WG_THREADS;
    Carver cv = Carver::aligned(base);
    SeedWorkspace w;
    w.plane = cv.take<unsigned long long>(N);
    w.totals = cv.take<int>(SEED_CODES * nblocks);
    w.codes = cv.take<unsigned char>((size_t)n);
    w.bytes = cv.bytes();
    return w;
  }
};

struct SeedArgs {
  int n, W, H;
  LidarCam cam;
  float min_depth, max_depth;
  float acc_min, depth_tol, occlusion_tol, footprint;
  float fsum;                  // fx + fy, each rounded to float once
  int radius, one_per_pixel;
  const float* points;         // [n][3]
  const float* covs_in;        // [n][9] or null
  const float* depth;          // [H][W] or null (with acc)
  const float* acc;
  const float* lidar;          // [H][W] or null
  const float* image;          // [3][H][W] or null
  const float* exposure;       // [3][2] or null
};

__device__ __forceinline__ unsigned long long seed_key(const float z, const int i) {
  return ((unsigned long long)__float_as_uint(z) << 32) | (unsigned int)i;
}

__global__ __launch_bounds__(256) void k_seed_clear(const int N, unsigned long long* __restrict__ plane) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i < N) plane[i] = SEED_EMPTY_;
}

__global__ __launch_bounds__(WG_THREADS) void k_seed_classify(const SeedArgs a, unsigned char* __restrict__ codes,
                                                              unsigned long long* __restrict__ plane) {
  const int i = blockIdx.x * WG_THREADS + (int)threadIdx.x;
  if (i >= a.n) return;
  const float x = a.points[3 * (size_t)i], y = a.points[3 * (size_t)i + 1], w = a.points[3 * (size_t)i + 2];
  LidarHit h;
  unsigned code = 0;
  if (!lidar_project(a.cam, x, y, w, a.min_depth, a.max_depth, a.W, a.H, h)) {
    codes[i] = 1;
    return;
  }
  const float z = h.z;
  const size_t pix = (size_t)h.iy * a.W + h.ix;
  if (a.lidar) {
    const int x0 = max(h.ix - a.radius, 0), x1 = min(h.ix + a.radius, a.W - 1);
    const int y0 = max(h.iy - a.radius, 0), y1 = min(h.iy + a.radius, a.H - 1);
    float zmin = INFINITY;
    for (int v = y0; v <= y1; v++)
      for (int u = x0; u <= x1; u++) {
        const float q = a.lidar[(size_t)v * a.W + u];
        if (q > 0.f && q < zmin) zmin = q;
      }
    if (zmin < INFINITY && z - zmin > a.occlusion_tol * z) code = 2;
  }
  if (code == 0 && a.depth) {
    const float A = a.acc[pix];
    if (A >= a.acc_min) {
      const float r = a.depth[pix] / A;
      const float band = a.depth_tol * z;
      if (r - z > band) code = 0;        // the measurement lies in front of the render
      else if (z - r > band) code = 4;
      else code = 3;
    }
  }
  codes[i] = (unsigned char)code;
  // z > min_depth >= 0: a positive float, whose bits order like the float (result unused: no return)
  if (code == 0 && a.one_per_pixel) atomicMin(&plane[pix], seed_key(z, i));
}

__global__ __launch_bounds__(WG_THREADS) void k_seed_resolve(const SeedArgs a, unsigned char* __restrict__ codes,
                                                             const unsigned long long* __restrict__ plane,
                                                             unsigned char* __restrict__ reasons,
                                                             int* __restrict__ totals, const int nblocks) {
  __shared__ int sh[WG_WAVES][SEED_CODES];
  const int i = blockIdx.x * WG_THREADS + (int)threadIdx.x;
  const bool in = i < a.n;
  unsigned code = 0;
  if (in) {
    code = codes[i];
    if (code == 0 && a.one_per_pixel) {
      const float x = a.points[3 * (size_t)i], y = a.points[3 * (size_t)i + 1], w = a.points[3 * (size_t)i + 2];
      LidarHit h;
      if (lidar_project(a.cam, x, y, w, a.min_depth, a.max_depth, a.W, a.H, h)) {  // (true: the code is 0)
        if (plane[(size_t)h.iy * a.W + h.ix] != seed_key(h.z, i)) {
          code = 5;
          codes[i] = 5;
        }
      }
    }
    if (reasons) reasons[i] = (unsigned char)code;
  }
  int cnt[SEED_CODES];
#pragma unroll
  for (int k = 0; k < SEED_CODES; k++) cnt[k] = __popcll(__ballot(in && code == (unsigned)k));
  store_block_totals(cnt, sh, totals, nblocks);
}

// ONE workgroup.  totals[0][.] -> exclusive scan in place; the six totals -> counts6.  nblocks == 0 writes zeros.
__global__ __launch_bounds__(WG_THREADS) void k_seed_scan(int* __restrict__ totals, const int nblocks,
                                                          int* __restrict__ counts6) {
  __shared__ int sh[WG_WAVES];
  const int admitted = scan_totals(totals, nblocks, sh);
  int c[SEED_CODES];
  c[0] = admitted;
#pragma unroll
  for (int k = 1; k < SEED_CODES; k++) {
    int t = 0;
    for (int j = threadIdx.x; j < nblocks; j += WG_THREADS) t += totals[(size_t)k * nblocks + j];
    c[k] = block_sum(t, sh);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < SEED_CODES; k++) counts6[k] = c[k];
  }
}

// one colour plane at (X, Y): border replication, two horizontal lerps and one vertical
__device__ __forceinline__ float seed_sample(const float* __restrict__ p, const int W, const int xa, const int xb,
                                             const int ya, const int yb, const float tx, const float ty) {
  const float v00 = p[(size_t)ya * W + xa], v01 = p[(size_t)ya * W + xb];
  const float v10 = p[(size_t)yb * W + xa], v11 = p[(size_t)yb * W + xb];
  const float top = v00 + tx * (v01 - v00);
  const float bot = v10 + tx * (v11 - v10);
  return top + ty * (bot - top);
}

__global__ __launch_bounds__(WG_THREADS) void k_seed_emit(const SeedArgs a, const unsigned char* __restrict__ codes,
                                                          const int* __restrict__ bases, float* __restrict__ xyz_out,
                                                          float* __restrict__ covs_out, float* __restrict__ rgb_out,
                                                          int* __restrict__ index_out, int* __restrict__ pixel_out,
                                                          float* __restrict__ z_out) {
  __shared__ int sh[WG_WAVES];
  const int i = blockIdx.x * WG_THREADS + (int)threadIdx.x;
  const bool mine = i < a.n && codes[i] == 0;
  const int rank = rank_in_block(mine, sh);
  if (!mine) return;
  const size_t j = (size_t)(bases[blockIdx.x] + rank);
  const float x = a.points[3 * (size_t)i], y = a.points[3 * (size_t)i + 1], w = a.points[3 * (size_t)i + 2];
  LidarHit h;
  if (!lidar_project(a.cam, x, y, w, a.min_depth, a.max_depth, a.W, a.H, h)) return;  // (never: the code is 0)
  index_out[j] = i;
  xyz_out[3 * j] = x;
  xyz_out[3 * j + 1] = y;
  xyz_out[3 * j + 2] = w;
  if (pixel_out) pixel_out[j] = h.iy * a.W + h.ix;
  if (z_out) z_out[j] = h.z;
  if (a.covs_in) {
#pragma unroll
    for (int k = 0; k < 9; k++) covs_out[9 * j + k] = a.covs_in[9 * (size_t)i + k];
  } else {
    const float sigma = ((a.footprint * h.z) * 2.f) / a.fsum;
    const float var = sigma * sigma;
#pragma unroll
    for (int k = 0; k < 9; k++) covs_out[9 * j + k] = (k == 0 || k == 4 || k == 8) ? var : 0.f;
  }
  if (a.image && rgb_out) {
    const float fx0 = floorf(h.X), fy0 = floorf(h.Y);   // X in [-0.5, W - 0.5): x0 in [-1, W - 1]
    const float tx = h.X - fx0, ty = h.Y - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int xa = min(max(x0, 0), a.W - 1), xb = min(max(x0 + 1, 0), a.W - 1);
    const int ya = min(max(y0, 0), a.H - 1), yb = min(max(y0 + 1, 0), a.H - 1);
    const size_t N = (size_t)a.H * a.W;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float v = seed_sample(a.image + c * N, a.W, xa, xb, ya, yb, tx, ty);
      if (a.exposure) v = (v - a.exposure[2 * c + 1]) / a.exposure[2 * c];
      rgb_out[3 * j + c] = v * 255.f;
    }
  }
}

static size_t seed_workspace_bytes(int n, int H, int W) { return n > 0 ? SeedWorkspace::carve(nullptr, n, H, W).bytes : 0; }

static hipError_t launch_sweep_admit(const SeedArgs& a, float* xyz_out, float* covs_out, float* rgb_out, int* index_out,
                                     int* pixel_out, float* z_out, unsigned char* reasons, int* counts6,
                                     char* workspace, hipStream_t s) {
  ProfScope ps(K_VISIBILITY, s);
  const int nblocks = (int)(((long long)a.n + WG_THREADS - 1) / WG_THREADS);
  if (a.n == 0) {
    hipLaunchKernelGGL(k_seed_scan, dim3(1), dim3(WG_THREADS), 0, s, (int*)nullptr, 0, counts6);
    return hipGetLastError();
  }
  const SeedWorkspace w = SeedWorkspace::carve(workspace, a.n, a.H, a.W);
  if (a.one_per_pixel) {
    const int N = a.H * a.W;
    hipLaunchKernelGGL(k_seed_clear, dim3((unsigned)(((long long)N + 255) / 256)), dim3(256), 0, s, N, w.plane);
  }
  hipLaunchKernelGGL(k_seed_classify, dim3(nblocks), dim3(WG_THREADS), 0, s, a, w.codes, w.plane);
  hipLaunchKernelGGL(k_seed_resolve, dim3(nblocks), dim3(WG_THREADS), 0, s, a, w.codes, w.plane, reasons, w.totals,
                     nblocks);
  hipLaunchKernelGGL(k_seed_scan, dim3(1), dim3(WG_THREADS), 0, s, w.totals, nblocks, counts6);
  hipLaunchKernelGGL(k_seed_emit, dim3(nblocks), dim3(WG_THREADS), 0, s, a, w.codes, w.totals, xyz_out, covs_out,
                     rgb_out, index_out, pixel_out, z_out);
  return hipGetLastError();
}

static bool seed_tol_ok(float v) { return v >= 0.f && v <= 3.402823466e38f; }  // (false for NaN and +inf)

}  // namespace gsr

using namespace gsr;

// ---- the entry points.  The order of the checks is part of the contract (include/gsraster.h).
extern "C" {

size_t gsr_sweep_admit_workspace(int n, int height, int width) {
  if (n < 0 || height < 1 || width < 1 || !plane_fits(height, width, 0x80000000ull)) return 0;
  return seed_workspace_bytes(n, height, width);
}

int gsr_sweep_admit(int n, const float* points_world, const float* covs_in, const float* T_cw12, const float* K9,
                    int height, int width, float min_depth, float max_depth, const float* depth, const float* acc,
                    float acc_min, float depth_tol, const float* lidar_depth, int occlusion_radius,
                    float occlusion_tol, const float* image, const float* exposure, float footprint,
                    int one_per_pixel, float* xyz_out, float* covs_out, float* rgb_out, int* index_out, int* pixel_out,
                    float* z_out, unsigned char* reasons, int* counts6, char* workspace, size_t workspace_bytes,
                    void* stream_) {
  clear_error();
  if (n < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad n");
  if (height < 1 || width < 1) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x80000000ull)) return e;  // (32-bit pixel indices)
  if ((n > 0 && !points_world) || !T_cw12 || !K9 || !xyz_out || !covs_out || !index_out || !counts6)
    return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if ((depth == nullptr) != (acc == nullptr))
    return fail(GSR_ERR_INVALID_ARGUMENT, "depth and acc are given together or not at all");
  if (!(acc_min > 0.f && acc_min <= 3.402823466e38f))  // (false for NaN and +inf)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad acc_min: finite and > 0");
  if (!seed_tol_ok(depth_tol)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad depth_tol: finite and >= 0");
  if (!seed_tol_ok(occlusion_tol)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad occlusion_tol: finite and >= 0");
  if (!seed_tol_ok(footprint)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad footprint: finite and >= 0");
  if (occlusion_radius < 0 || occlusion_radius > 3) return fail(GSR_ERR_INVALID_ARGUMENT, "bad occlusion_radius: 0 to 3");
  if (!(min_depth >= 0.f && min_depth <= 3.402823466e38f))  // (false for NaN and +inf)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad min_depth: finite and >= 0");
  if (!(max_depth > min_depth)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad max_depth: greater than min_depth");
  if (int e = check_workspace(workspace_bytes, seed_workspace_bytes(n, height, width))) return e;
  if (n > 0 && !workspace) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_aligned4((uintptr_t)points_world | (uintptr_t)covs_in | (uintptr_t)depth | (uintptr_t)acc |
                             (uintptr_t)lidar_depth | (uintptr_t)image | (uintptr_t)exposure | (uintptr_t)xyz_out |
                             (uintptr_t)covs_out | (uintptr_t)rgb_out | (uintptr_t)index_out | (uintptr_t)pixel_out |
                             (uintptr_t)z_out | (uintptr_t)counts6))
    return e;
  SeedArgs a;
  a.n = n; a.W = width; a.H = height;
  a.cam = lidar_compose(T_cw12, K9);
  a.min_depth = min_depth; a.max_depth = max_depth;
  a.acc_min = acc_min; a.depth_tol = depth_tol; a.occlusion_tol = occlusion_tol; a.footprint = footprint;
  a.fsum = K9[0] + K9[4];
  a.radius = occlusion_radius; a.one_per_pixel = one_per_pixel ? 1 : 0;
  a.points = points_world; a.covs_in = covs_in; a.depth = depth; a.acc = acc; a.lidar = lidar_depth;
  a.image = image; a.exposure = exposure;
  HIP_TRY(launch_sweep_admit(a, xyz_out, covs_out, rgb_out, index_out, pixel_out, z_out, reasons, counts6, workspace,
                             (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
