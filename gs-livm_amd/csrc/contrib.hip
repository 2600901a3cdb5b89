// contrib.hip -- per-Gaussian blend contribution of a completed forward (an extension: the reference's rasterizer has no
// such output; MonoGS' hands back n_touched): the entry points, the zero fill of the frame rows and the finish kernel.
// The walk itself, k_contribution_tile, lives in render.hip beside the blend kernels whose alpha it recomputes with
// their own device functions and compiler flags.
//
//   k_contribution_finish  one thread per row: the integer frame row {u64 wsum_fx, u32 pixels, u32 wmax_bits} becomes
//                          n_touched, weight_sum = (float)((double)wsum_fx 2^-32), weight_max, the mask
//                          (n_touched >= min_pixels && weight_max >= min_weight) and / or is folded into the sweep
//                          statistics {weight_sum_total, views, weight_max}; every requested element is written.
// Plain vector loads and stores only.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

__global__ __launch_bounds__(WG_THREADS) void k_contribution_finish(const int P, const uint2* __restrict__ rows,
                                                                   const int min_pixels, const float min_weight,
                                                                   int* __restrict__ n_touched,
                                                                   float* __restrict__ weight_sum,
                                                                   float* __restrict__ weight_max,
                                                                   unsigned char* __restrict__ mask,
                                                                   float* __restrict__ stats) {
  const int i = blockIdx.x * WG_THREADS + threadIdx.x;
  if (i >= P) return;
  // two 8-byte loads: the rows are only 8-byte aligned.  (wsum_fx low, wsum_fx high | pixels, wmax_bits)
  const uint2 lo = rows[2 * (size_t)i], r = rows[2 * (size_t)i + 1];
  const unsigned long long fx = ((unsigned long long)lo.y << 32) | lo.x;
  const int n = (int)r.x;  // < 2^31: the entry point refuses larger planes
  const float ws = (float)((double)fx * (1.0 / 4294967296.0));
  const float wm = __uint_as_float(r.y);
  if (n_touched) n_touched[i] = n;
  if (weight_sum) weight_sum[i] = ws;
  if (weight_max) weight_max[i] = wm;
  if (mask) mask[i] = (n >= min_pixels && wm >= min_weight) ? 1 : 0;
  if (stats) {
    float* const s = stats + 3 * (size_t)i;
    s[0] += ws;
    s[1] += n > 0 ? 1.0f : 0.0f;
    s[2] = fmaxf(s[2], wm);
  }
}

static const char* const kMisalignedRows = "misaligned pointer: frame rows need 8-byte alignment";

}  // namespace gsr

using namespace gsr;

// ---- the entry points.  The order of the checks is part of the contract (include/gsraster.h): shape, then "nothing
// asked for", then null pointers, then alignment.
extern "C" {

size_t gsr_contribution_workspace(int P) { return P > 0 ? 16 * (size_t)P : 0; }

int gsr_contribution(int P, int R, int width, int height, const char* geom_buffer, const char* binning_buffer,
                     const char* image_buffer, char* frame_rows, void* stream_) {
  clear_error();
  if (P < 0 || R < 0 || width <= 0 || height <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P/R/width/height");
  if (int e = check_plane(height, width, 0x80000000ull)) return e;
  if (P == 0) return GSR_OK;
  if (!frame_rows) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (R > 0 && (!geom_buffer || !binning_buffer || !image_buffer))
    return fail(GSR_ERR_INVALID_ARGUMENT, "null state blob");
  if ((uintptr_t)frame_rows & 7u) return fail(GSR_ERR_INVALID_ARGUMENT, "%s", kMisalignedRows);
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_VISIBILITY, s);
  HIP_TRY(hipMemsetAsync(frame_rows, 0, 16 * (size_t)P, s));
  if (R == 0) return GSR_OK;
  FrameParams fp{};
  fp.P = P;
  fp.W = width;
  fp.H = height;
  fp.gx = (width + TILE - 1) / TILE;
  fp.gy = (height + TILE - 1) / TILE;
  const GeomState g = GeomState::carve(const_cast<char*>(geom_buffer), (size_t)P);
  const BinningState b = BinningState::carve(const_cast<char*>(binning_buffer), (size_t)R);
  const ImageState im = ImageState::carve(const_cast<char*>(image_buffer), width, height);
  HIP_TRY(launch_contribution(fp, g, b, im, frame_rows, s));
  return GSR_OK;
}

int gsr_contribution_finish(int P, const char* frame_rows, int min_pixels, float min_weight, int* n_touched,
                            float* weight_sum, float* weight_max, unsigned char* mask, float* stats, void* stream_) {
  clear_error();
  if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
  if (min_pixels < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad min_pixels");
  if (!(min_weight >= 0.0f)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad min_weight");
  if (!n_touched && !weight_sum && !weight_max && !mask && !stats)
    return fail(GSR_ERR_INVALID_ARGUMENT, "no output is asked for");
  if (P == 0) return GSR_OK;
  if (!frame_rows) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if ((uintptr_t)frame_rows & 7u) return fail(GSR_ERR_INVALID_ARGUMENT, "%s", kMisalignedRows);
  if (int e = check_aligned4((uintptr_t)n_touched | (uintptr_t)weight_sum | (uintptr_t)weight_max | (uintptr_t)stats))
    return e;
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_VISIBILITY, s);
  hipLaunchKernelGGL(k_contribution_finish, dim3((unsigned)(((long long)P + WG_THREADS - 1) / WG_THREADS)), dim3(WG_THREADS), 0, s,
                     P, reinterpret_cast<const uint2*>(frame_rows), min_pixels, min_weight, n_touched, weight_sum,
                     weight_max, mask, stats);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
