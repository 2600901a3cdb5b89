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
//
// 3. gsr_lidar_occlusion_filter and 4. gsr_lidar_depth_loss_robust sit beside the two above and leave them as they are:
// the occlusion rule of sweep admission (seed.hip, code 2) applied to the supervision image itself, and the depth loss
// with a Huber residual and a clip.  Each is described in front of its kernels.
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
    Carver cv = Carver::aligned(base);
    LidarWorkspace w;
    w.abs_part = cv.take<double>(nblocks);
    w.cnt_part = cv.take<int>(nblocks);
    w.scale = cv.take<float>(1);
    w.bytes = cv.bytes();
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

// ---- 3. gsr_lidar_occlusion_filter ---------------------------------------------------------------------------------
// One launch of at most FILTER_MAX_GROUPS workgroups; a workgroup walks tiles of FILTER_TW x FILTER_TH pixels (64 x 16:
// rows of 256 bytes, four pixels of one column per thread) and adds its two counts once at its end -- one integer
// atomic per count per WORKGROUP, not per wave: at 1920 x 1080 one pair per wave is 16 200 adds to one cache line,
// which were measured to cost five times the filter itself.  The tile plus a halo of R pixels is staged in LDS with every value that is not > 0 (0, negatives,
// NaN) and every position outside the image mapped to +inf, so that the minimum needs no mask; the window minimum is
// separable and exact (min is associative and commutative on non-NaN floats): row minima of the staged rows into a
// second LDS plane, then column minima of those -- 2 (2R + 1) taps instead of (2R + 1)^2.  The removal test is
// k_seed_classify's expression restated (seed.hip is built without contraction; the subtraction and the product are
// explicit here): one subtraction, one product, one compare.  Scalar 4-byte accesses only: a row of an arbitrary-width
// image at a 4-byte-aligned base has no wider alignment.  Every index is tested against the image.
constexpr int FILTER_TW = 64, FILTER_TH = 16, FILTER_RMAX = 3;
constexpr int FILTER_MAX_GROUPS = 1024;  // workgroups of the one launch: four per CU, each walks its tiles

template <int R>
__global__ __launch_bounds__(WG_THREADS) void k_lidar_occlusion_filter(const int H, const int W, const int tiles_x,
                                                                       const int tiles, const float tol,
                                                                       const float* __restrict__ lidar,
                                                                       float* __restrict__ filtered,
                                                                       int* __restrict__ counts2) {
  constexpr int SW = FILTER_TW + 2 * R, SH = FILTER_TH + 2 * R;
  __shared__ float stage[SH][SW];            // the tile and its halo, invalid -> +inf
  __shared__ float rowmin[SH][FILTER_TW];    // min over |dx| <= R of stage
  __shared__ int shkept[WG_WAVES], shremoved[WG_WAVES];
  const int lx = threadIdx.x & (FILTER_TW - 1), ly0 = (int)(threadIdx.x >> 6) * (FILTER_TH / WG_WAVES);
  int kept = 0, removed = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform over the workgroup: it holds barriers)
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int x0 = tile_x * FILTER_TW, y0 = tile_y * FILTER_TH;
    for (int k = threadIdx.x; k < SH * SW; k += WG_THREADS) {
      const int sy = k / SW, sx = k - sy * SW;
      const int y = y0 + sy - R, x = x0 + sx - R;
      float q = INFINITY;
      if (x >= 0 && x < W && y >= 0 && y < H) {
        const float v = lidar[(size_t)y * W + x];
        if (v > 0.f) q = v;
      }
      stage[sy][sx] = q;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < SH * FILTER_TW; k += WG_THREADS) {
      const int sy = k / FILTER_TW, sx = k - sy * FILTER_TW;
      float m = stage[sy][sx];
#pragma unroll
      for (int d = 1; d <= 2 * R; d++) m = fminf(m, stage[sy][sx + d]);
      rowmin[sy][sx] = m;
    }
    __syncthreads();
    const int x = x0 + lx;
#pragma unroll
    for (int j = 0; j < FILTER_TH / WG_WAVES; j++) {
      const int ly = ly0 + j, y = y0 + ly;
      if (x < W && y < H) {
        float zmin = rowmin[ly][lx];
#pragma unroll
        for (int d = 1; d <= 2 * R; d++) zmin = fminf(zmin, rowmin[ly + d][lx]);
        const size_t p = (size_t)y * W + x;
        const float z = lidar[p];
        float out = 0.f;
        if (z > 0.f) {
          if (zmin < INFINITY && __fsub_rn(z, zmin) > __fmul_rn(tol, z)) removed++;
          else { out = z; kept++; }
        }
        filtered[p] = out;
      }
    }
    __syncthreads();  // the next tile overwrites both planes
  }
  if (counts2) {  // the workgroup's tiles together: one integer atomic add per count
    kept = wave_sum(kept);
    removed = wave_sum(removed);
    if ((threadIdx.x & 63) == 0) { shkept[threadIdx.x >> 6] = kept; shremoved[threadIdx.x >> 6] = removed; }
    __syncthreads();
    if (threadIdx.x == 0) {
      kept = (shkept[0] + shkept[1]) + (shkept[2] + shkept[3]);
      removed = (shremoved[0] + shremoved[1]) + (shremoved[2] + shremoved[3]);
      if (kept) atomicAdd(&counts2[0], kept);
      if (removed) atomicAdd(&counts2[1], removed);
    }
  }
}

// ---- 4. gsr_lidar_depth_loss_robust --------------------------------------------------------------------------------
// gsr_lidar_depth_loss with a Huber residual and a clip, the same three launches over the same candidates
// (lidar_depth > 0 and A >= acc_min):
//   q = D / A, e = q - z_L, a = |e|, tau = huber_abs + huber_rel z_L, clip = clip_abs + clip_rel z_L
//   a > clip: clipped -- not supervised, counted in n_clip, both gradients 0 (false for a NaN a: it stays supervised)
//   a < tau:  rho = 0.5 a (a / tau), psi = e / tau;  otherwise rho = a - 0.5 tau, psi = sign(e), sign(0) = 0
//   L = lambda sum rho / max(n_sup, 1);  dL/dD = (c psi) / A, dL/dA = -(dL/dD) q, c = lambda / n_sup narrowed once
// With huber_abs = huber_rel = clip_rel = 0 and clip_abs = +inf, tau is 0 and clip is +inf: `a < 0` and `a > inf` are
// never true, rho = a - 0.5f * 0 is a and psi is sign(e) -- the sums, in block_sum's order, and both gradients are
// those of gsr_lidar_depth_loss bit for bit.
struct LidarRobustWorkspace {
  double* rho_part;   // [nblocks]
  double* abs_part;   // [nblocks]
  int* sup_part;      // [nblocks]
  int* clip_part;     // [nblocks]
  float* scale;       // [1] c = lambda / n_sup (0 when nothing is supervised)
  size_t bytes;
  static LidarRobustWorkspace carve(char* base, int H, int W) {
    const size_t N = (size_t)H * W, nblocks = (N + 255) / 256;
    Carver cv = Carver::aligned(base);
    LidarRobustWorkspace w;
    w.rho_part = cv.take<double>(nblocks);
    w.abs_part = cv.take<double>(nblocks);
    w.sup_part = cv.take<int>(nblocks);
    w.clip_part = cv.take<int>(nblocks);
    w.scale = cv.take<float>(1);
    w.bytes = cv.bytes();
    return w;
  }
};

struct LidarRobust {
  float huber_abs, huber_rel, clip_abs, clip_rel;
};

// One candidate pixel, shared by the forward and the gradients: false when it is clipped.
__device__ __forceinline__ bool lidar_robust_term(const LidarRobust r, const float e, const float zl, float& a,
                                                  float& rho, float& psi) {
  a = fabsf(e);
  const float tau = r.huber_abs + r.huber_rel * zl;
  const float clip = r.clip_abs + r.clip_rel * zl;
  rho = 0.f;
  psi = 0.f;
  if (a > clip) return false;
  if (a < tau) {
    rho = 0.5f * a * (a / tau);
    psi = e / tau;
  } else {
    rho = a - 0.5f * tau;
    psi = (float)((e > 0.f) - (e < 0.f));
  }
  return true;
}

__global__ __launch_bounds__(256) void k_lidar_robust_forward(const int N, const float acc_min, const LidarRobust r,
                                                              const float* __restrict__ depth,
                                                              const float* __restrict__ acc,
                                                              const float* __restrict__ lidar,
                                                              double* __restrict__ rho_part,
                                                              double* __restrict__ abs_part,
                                                              int* __restrict__ sup_part, int* __restrict__ clip_part) {
  __shared__ double shrho[4], shabs[4];
  __shared__ int shsup[4], shclip[4];
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  float ae = 0.f, rho = 0.f;
  int on = 0, clipped = 0;
  if (i < N) {
    const float zl = lidar[i], a = acc[i];
    if (zl > 0.f && a >= acc_min) {
      float av, rv, psi;
      if (lidar_robust_term(r, depth[i] / a - zl, zl, av, rv, psi)) {
        on = 1;
        ae = av;
        rho = rv;
      } else {
        clipped = 1;
      }
    }
  }
  // block_sum_pair's order for each of the four sums, behind ONE pair of barriers
  // (the wave butterflies are what this kernel costs beyond its loads, DESIGN.md section 5: the two counts, at most 64
  // each, share one -- supervised in the low half, clipped in the high half)
  const double s = wave_sum((double)rho), t = wave_sum((double)ae);
  const int both = wave_sum(on | (clipped << 16));
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    shrho[w] = s;
    shabs[w] = t;
    shsup[w] = both & 0xFFFF;
    shclip[w] = both >> 16;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    rho_part[blockIdx.x] = (shrho[0] + shrho[1]) + (shrho[2] + shrho[3]);
    abs_part[blockIdx.x] = (shabs[0] + shabs[1]) + (shabs[2] + shabs[3]);
    sup_part[blockIdx.x] = (shsup[0] + shsup[1]) + (shsup[2] + shsup[3]);
    clip_part[blockIdx.x] = (shclip[0] + shclip[1]) + (shclip[2] + shclip[3]);
  }
}

__global__ __launch_bounds__(256) void k_lidar_robust_finish(const int N, const int nblocks, const float lambda,
                                                             const double* __restrict__ rho_part,
                                                             const double* __restrict__ abs_part,
                                                             const int* __restrict__ sup_part,
                                                             const int* __restrict__ clip_part,
                                                             float* __restrict__ out4, float* __restrict__ scale) {
  __shared__ double shsum[4][4];
  // thread-strided over the partials, then the workgroup tree: partial_pairs_sum's order for each of the four sums,
  // in ONE walk -- the finish is a single workgroup waiting on memory, and a second walk doubles it
  double rs = 0.0, cs = 0.0, as = 0.0, ks = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += WG_THREADS) {
    rs += rho_part[b];
    as += abs_part[b];
    cs += (double)sup_part[b];
    ks += (double)clip_part[b];
  }
  rs = wave_sum(rs);
  cs = wave_sum(cs);
  as = wave_sum(as);
  ks = wave_sum(ks);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    shsum[0][w] = rs;
    shsum[1][w] = cs;
    shsum[2][w] = as;
    shsum[3][w] = ks;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    rs = (shsum[0][0] + shsum[0][1]) + (shsum[0][2] + shsum[0][3]);
    cs = (shsum[1][0] + shsum[1][1]) + (shsum[1][2] + shsum[1][3]);
    as = (shsum[2][0] + shsum[2][1]) + (shsum[2][2] + shsum[2][3]);
    ks = (shsum[3][0] + shsum[3][1]) + (shsum[3][2] + shsum[3][3]);
    const float mean_rho = cs > 0.0 ? (float)(rs / cs) : 0.f;
    out4[0] = cs > 0.0 ? lambda * mean_rho : 0.f;
    out4[1] = cs > 0.0 ? (float)(as / cs) : 0.f;
    out4[2] = (float)(cs / (double)N);
    out4[3] = (float)(ks / (double)N);
    *scale = cs > 0.0 ? (float)((double)lambda / cs) : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_lidar_robust_grads(const int N, const float acc_min, const LidarRobust r,
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
    float av, rv, psi;
    if (lidar_robust_term(r, q - zl, zl, av, rv, psi) && psi != 0.f) {
      gd = (c * psi) / a;
      ga = -gd * q;
    }
  }
  if (dL_ddepth) dL_ddepth[i] = gd;
  if (dL_dacc) dL_dacc[i] = ga;
}

template <int R>
static void launch_filter_r(int H, int W, int tiles_x, int tiles, float tol, const float* lidar, float* filtered,
                            int* counts2, hipStream_t s) {
  const int groups = tiles < FILTER_MAX_GROUPS ? tiles : FILTER_MAX_GROUPS;
  hipLaunchKernelGGL(k_lidar_occlusion_filter<R>, dim3(groups), dim3(WG_THREADS), 0, s, H, W, tiles_x, tiles, tol, lidar,
                     filtered, counts2);
}

static hipError_t launch_lidar_occlusion_filter(int H, int W, const float* lidar, int radius, float tol,
                                                float* filtered, int* counts2, hipStream_t s) {
  // (H W < 2^31: the tile count is below 2^28, a one-dimensional grid)
  const long long tx = ((long long)W + FILTER_TW - 1) / FILTER_TW, ty = ((long long)H + FILTER_TH - 1) / FILTER_TH;
  const int tiles = (int)(tx * ty);
  // the two counts start at zero: eight bytes cleared on the stream in front of the one launch
  if (counts2) {
    const hipError_t e = hipMemsetAsync(counts2, 0, 2 * sizeof(int), s);
    if (e != hipSuccess) return e;
  }
  ProfScope ps(K_LIDAR_CONVERT, s);
  switch (radius) {
    case 0: launch_filter_r<0>(H, W, (int)tx, tiles, tol, lidar, filtered, counts2, s); break;
    case 1: launch_filter_r<1>(H, W, (int)tx, tiles, tol, lidar, filtered, counts2, s); break;
    case 2: launch_filter_r<2>(H, W, (int)tx, tiles, tol, lidar, filtered, counts2, s); break;
    default: launch_filter_r<3>(H, W, (int)tx, tiles, tol, lidar, filtered, counts2, s); break;
  }
  return hipGetLastError();
}

static size_t lidar_robust_workspace_bytes(int H, int W) { return LidarRobustWorkspace::carve(nullptr, H, W).bytes; }

static hipError_t launch_lidar_depth_loss_robust(int H, int W, const float* depth, const float* acc,
                                                 const float* lidar_depth, float acc_min, float lambda,
                                                 const LidarRobust r, float* out4, float* dL_ddepth, float* dL_dacc,
                                                 char* workspace, hipStream_t s) {
  const int N = H * W, nblocks = (int)(((long long)N + 255) / 256);
  const LidarRobustWorkspace w = LidarRobustWorkspace::carve(workspace, H, W);
  {
    ProfScope ps(K_LIDAR_LOSS_FWD, s);
    hipLaunchKernelGGL(k_lidar_robust_forward, dim3(nblocks), dim3(256), 0, s, N, acc_min, r, depth, acc, lidar_depth,
                       w.rho_part, w.abs_part, w.sup_part, w.clip_part);
  }
  {
    ProfScope ps(K_LIDAR_LOSS_FINISH, s);
    hipLaunchKernelGGL(k_lidar_robust_finish, dim3(1), dim3(256), 0, s, N, nblocks, lambda, w.rho_part, w.abs_part,
                       w.sup_part, w.clip_part, out4, w.scale);
  }
  if (dL_ddepth || dL_dacc) {
    ProfScope ps(K_LIDAR_LOSS_GRADS, s);
    hipLaunchKernelGGL(k_lidar_robust_grads, dim3(nblocks), dim3(256), 0, s, N, acc_min, r, depth, acc, lidar_depth,
                       w.scale, dL_ddepth, dL_dacc);
  }
  return hipGetLastError();
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

int gsr_lidar_occlusion_filter(int height, int width, const float* lidar_depth, int radius, float tol, float* filtered,
                               int* counts2, void* stream_) {
  clear_error();
  if (height < 1 || width < 1) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x80000000ull)) return e;  // (32-bit pixel indices)
  if (!lidar_depth || !filtered) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (radius < 0 || radius > FILTER_RMAX) return fail(GSR_ERR_INVALID_ARGUMENT, "bad radius: 0..3");
  if (!(tol >= 0.f && tol <= 3.402823466e38f))  // (false for NaN and +inf)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad tol: finite and >= 0");
  {
    // the window reads neighbours: the filter is out of place
    const uintptr_t bytes = (uintptr_t)height * (uintptr_t)width * sizeof(float);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(lidar_depth), d0 = reinterpret_cast<uintptr_t>(filtered);
    if (s0 < d0 + bytes && d0 < s0 + bytes)
      return fail(GSR_ERR_INVALID_ARGUMENT, "lidar_depth and filtered overlap: the filter is out of place");
  }
  HIP_TRY(launch_lidar_occlusion_filter(height, width, lidar_depth, radius, tol, filtered, counts2,
                                        (hipStream_t)stream_));
  return GSR_OK;
}

size_t gsr_lidar_depth_loss_robust_workspace(int height, int width) {
  if (height < 1 || width < 1 || !plane_fits(height, width, 0x80000000ull)) return 0;
  return lidar_robust_workspace_bytes(height, width);
}

int gsr_lidar_depth_loss_robust(int height, int width, const float* depth, const float* acc, const float* lidar_depth,
                                float acc_min, float lambda, float huber_abs, float huber_rel, float clip_abs,
                                float clip_rel, float* out4, float* dL_ddepth, float* dL_dacc, char* workspace,
                                size_t workspace_bytes, void* stream_) {
  clear_error();
  if (height < 1 || width < 1) return fail(GSR_ERR_INVALID_ARGUMENT, "bad image shape");
  if (int e = check_plane(height, width, 0x80000000ull)) return e;  // (32-bit pixel indices)
  if (!depth || !acc || !lidar_depth || !out4 || !workspace) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (!(acc_min > 0.f && acc_min <= 3.402823466e38f))  // (false for NaN and +inf)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad acc_min: finite and > 0");
  auto finite_nonneg = [](float v) { return v >= 0.f && v <= 3.402823466e38f; };  // (false for NaN and +inf)
  if (!finite_nonneg(huber_abs)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad huber_abs: finite and >= 0");
  if (!finite_nonneg(huber_rel)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad huber_rel: finite and >= 0");
  if (!(clip_abs >= 0.f)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad clip_abs: >= 0 (+inf: no clip)");
  if (!finite_nonneg(clip_rel)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad clip_rel: finite and >= 0");
  if (int e = check_workspace(workspace_bytes, lidar_robust_workspace_bytes(height, width))) return e;
  const LidarRobust r{huber_abs, huber_rel, clip_abs, clip_rel};
  HIP_TRY(launch_lidar_depth_loss_robust(height, width, depth, acc, lidar_depth, acc_min, lambda, r, out4, dL_ddepth,
                                         dL_dacc, workspace, (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
