// prune.hip -- in-place pruning of the model: rows that are dead to the rasterizer for good are marked, the surviving
// rows get their new row numbers, and the leaves and their Adam moments are compacted (the shrinking half of the
// optimiser-state surgery: GaussianModel::prune_optimizer, reference src/gs/gaussian.cu:430-449 -- an index_select of a
// leaf and of both of its moments, per group; the reference never calls it, so this is an extension).
//
// Removal is a STABLE stream compaction: survivors keep their relative order, so a voxel's row range stays a range
// (VoxelIndex) and the rasterizer's depth ties, which are broken by ascending row number, fall as before.
//
// Launches of one prune of a whole model, whatever P: FOUR.
//   k_prune_mark     one thread per row: the drop rule -> reasons[P]; per-workgroup totals of "kept" and of each reason
//   k_prune_scan     ONE workgroup: exclusive scan of the per-workgroup kept totals (in place), the reason totals,
//                    counts[5] and row_map[P] = P'
//   k_prune_rank     one thread per row: row_map[i] = workgroup base + rank inside the workgroup (ballot / popcount)
//   k_prune_compact  one thread per SOURCE float of the virtual concatenation of up to 18 tensors:
//                    dst[row_map[i]] = src[i] where reasons[i] == 0
// No workgroup waits for another (no look-back chain, no spin), and no atomics: row_map and the counts are the same
// whatever the order the workgroups run in.  Plain vector loads and stores only.
//
// The compaction is out of place on purpose: an in-place stable compaction races between workgroups (one writes the
// rows another has yet to read).  Rows [P', ...) of a destination are not written.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

constexpr int PRUNE_BLOCK = WG_THREADS;  // rows per workgroup of k_prune_mark / k_prune_rank (4 waves)
constexpr int COMPACT_ITEMS = 4;      // floats per thread of k_prune_compact, 256 apart: 1024 consecutive floats per workgroup
constexpr int COMPACT_TILE = 256 * COMPACT_ITEMS;
constexpr int PRUNE_MAX_TENSORS = 18;  // tensors one compaction launch moves (CompactArgs)

// reasons[i]: 0 = keep
constexpr unsigned R_OPACITY = 1u, R_SCALE = 2u, R_NONFINITE = 4u, R_MASK = 8u;

inline size_t prune_blocks(int P) { return ((size_t)P + PRUNE_BLOCK - 1) / PRUNE_BLOCK; }
// [5][nblocks] int32: [0] kept rows per workgroup -> their exclusive scan; [1..4] rows per workgroup with reason bit 0..3
static size_t prune_workspace_bytes(int P) { return P > 0 ? 5 * prune_blocks(P) * sizeof(int) : 0; }

// The activated values are those of k_activate / k_model_step bit for bit (same expf, same sigmoidf_), so "dropped for
// scale" is exactly "k_preprocess' scale cull fires at scale_modifier 1", and the comparisons are the rasterizer's:
// a value ON a threshold is kept (the culls are strict), a NaN compares false in both tests (hence the third bit).
__global__ __launch_bounds__(PRUNE_BLOCK) void k_prune_mark(const int P, const float* __restrict__ xyz,
                                                            const float* __restrict__ scaling_raw,
                                                            const float* __restrict__ rotation_raw,
                                                            const float* __restrict__ opacity_raw,
                                                            const unsigned char* __restrict__ drop,
                                                            const float min_opacity, const float max_scale,
                                                            const int drop_nonfinite, unsigned char* __restrict__ reasons,
                                                            int* __restrict__ totals, const int nblocks) {
  __shared__ int sh[WG_WAVES][5];
  const int i = blockIdx.x * PRUNE_BLOCK + threadIdx.x;
  const bool in = i < P;
  unsigned r = 0;
  if (in) {
    const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
    const float o = opacity_raw[i];
    const float s0 = scaling_raw[i3], s1 = scaling_raw[i3 + 1], s2 = scaling_raw[i3 + 2];
    if (sigmoidf_(o) < min_opacity) r |= R_OPACITY;
    if (expf(s0) > max_scale || expf(s1) > max_scale || expf(s2) > max_scale) r |= R_SCALE;
    if (drop_nonfinite) {
      bool bad = nonfinite_(o) || nonfinite_(s0) || nonfinite_(s1) || nonfinite_(s2);
#pragma unroll
      for (int k = 0; k < 3; k++) bad = bad || nonfinite_(xyz[i3 + k]);
#pragma unroll
      for (int k = 0; k < 4; k++) bad = bad || nonfinite_(rotation_raw[i4 + k]);
      if (bad) r |= R_NONFINITE;
    }
    if (drop && drop[i]) r |= R_MASK;
    reasons[i] = (unsigned char)r;
  }
  int n[5];  // kept, then the four reasons
  n[0] = __popcll(__ballot(in && r == 0));
#pragma unroll
  for (int k = 0; k < 4; k++) n[1 + k] = __popcll(__ballot((r >> k) & 1u));
  store_block_totals(n, sh, totals, nblocks);
}

// ONE workgroup.  totals[0][.] -> exclusive scan in place (scan_totals); then the four reason totals, counts5 and
// row_map[P].  nblocks == 0 (P == 0) writes zeros.
__global__ __launch_bounds__(PRUNE_BLOCK) void k_prune_scan(int* __restrict__ totals, const int nblocks,
                                                            int* __restrict__ counts5, int* __restrict__ row_map_end) {
  __shared__ int sh[WG_WAVES];
  const int carry = scan_totals(totals, nblocks, sh);
  int n_r[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int t = 0;
    for (int j = threadIdx.x; j < nblocks; j += PRUNE_BLOCK) t += totals[(size_t)(1 + k) * nblocks + j];
    n_r[k] = block_sum(t, sh);
  }
  if (threadIdx.x == 0) {
    counts5[0] = carry;
#pragma unroll
    for (int k = 0; k < 4; k++) counts5[1 + k] = n_r[k];
    *row_map_end = carry;
  }
}

__global__ __launch_bounds__(PRUNE_BLOCK) void k_prune_rank(const int P, const unsigned char* __restrict__ reasons,
                                                            const int* __restrict__ bases, int* __restrict__ row_map) {
  __shared__ int sh[WG_WAVES];
  const int i = blockIdx.x * PRUNE_BLOCK + threadIdx.x;
  const int rank = rank_in_block(i < P && reasons[i] == 0, sh);
  if (i < P) row_map[i] = bases[blockIdx.x] + rank;
}

struct CompactArgs {
  const float* src[PRUNE_MAX_TENSORS];
  float* dst[PRUNE_MAX_TENSORS];
  unsigned long long numel[PRUNE_MAX_TENSORS];  // P * width
  unsigned end[PRUNE_MAX_TENSORS];              // cumulative count of workgroups (COMPACT_TILE floats each)
  unsigned width[PRUNE_MAX_TENSORS];            // floats per row (> 0: empty tensors are left out on the host)
  int n;
  const unsigned char* reasons;
  const int* row_map;
};

// Thread per source float: a wave instruction reads 64 consecutive floats and writes them, as far as they are kept,
// to consecutive addresses again (a kept run of rows stays a run; the write only shifts down).  A workgroup takes 1024
// consecutive floats of ONE tensor (the tensor is looked up once, on the scalar unit); its first float's row and column
// take one division, the 1024 floats behind it 32-bit arithmetic on small numbers.  The four loads of a thread are
// issued before the first store depends on them.
__global__ __launch_bounds__(256) void k_prune_compact(const CompactArgs a) {
  int t = 0;
  unsigned start = 0;
#pragma unroll
  for (int k = 0; k < PRUNE_MAX_TENSORS; k++) {
    if (k < a.n && blockIdx.x >= a.end[k]) { t = k + 1; start = a.end[k]; }
  }
  if (t >= a.n) return;
  const unsigned long long numel = a.numel[t];
  const unsigned w = a.width[t];
  const float* __restrict__ src = a.src[t];
  float* __restrict__ dst = a.dst[t];
  const unsigned long long e0 = (unsigned long long)(blockIdx.x - start) * COMPACT_TILE;
  unsigned long long row0;
  unsigned c0;
  if (numel <= 0xFFFFFFFFull) { const uint32_t q = (uint32_t)e0 / w; row0 = q; c0 = (uint32_t)e0 - q * w; }
  else { row0 = e0 / w; c0 = (unsigned)(e0 - row0 * w); }
  float v[COMPACT_ITEMS];
  unsigned long long out[COMPACT_ITEMS];
  bool keep[COMPACT_ITEMS];
#pragma unroll
  for (int k = 0; k < COMPACT_ITEMS; k++) {
    const unsigned local = (unsigned)k * 256u + threadIdx.x;
    const unsigned long long e = e0 + local;
    keep[k] = false;
    v[k] = 0.f;
    out[k] = 0;
    if (e < numel) {
      const unsigned l = c0 + local;  // < width + COMPACT_TILE
      const unsigned dr = l / w, c = l - dr * w;
      const unsigned long long i = row0 + dr;  // < P
      v[k] = src[e];
      keep[k] = a.reasons[i] == 0;
      out[k] = (unsigned long long)(unsigned)a.row_map[i] * w + c;
    }
  }
#pragma unroll
  for (int k = 0; k < COMPACT_ITEMS; k++)
    if (keep[k]) dst[out[k]] = v[k];
}

// workgroups of the one compaction launch (the entry point refuses a model that needs more than a grid holds)
static unsigned long long prune_compact_blocks(int P, int n, const int* widths) {
  unsigned long long blocks = 0;
  for (int k = 0; k < n; k++)
    if (widths[k] > 0) blocks += ((unsigned long long)P * (unsigned long long)widths[k] + COMPACT_TILE - 1) / COMPACT_TILE;
  return blocks;
}

static hipError_t launch_prune_compact(int P, int n, const float* const* src, float* const* dst, const int* widths,
                                       const unsigned char* reasons, const int* row_map, hipStream_t s) {
  CompactArgs a;
  a.n = 0;
  a.reasons = reasons;
  a.row_map = row_map;
  unsigned long long cum = 0;
  for (int k = 0; k < PRUNE_MAX_TENSORS; k++) {
    a.src[k] = nullptr; a.dst[k] = nullptr; a.numel[k] = 0; a.width[k] = 1; a.end[k] = 0;
  }
  for (int k = 0; k < n; k++) {
    if (widths[k] <= 0) continue;  // e.g. _features_rest at M = 1: nothing to move
    const int j = a.n++;
    a.src[j] = src[k]; a.dst[j] = dst[k];
    a.width[j] = (unsigned)widths[k];
    a.numel[j] = (unsigned long long)P * (unsigned long long)widths[k];
    cum += (a.numel[j] + COMPACT_TILE - 1) / COMPACT_TILE;
    a.end[j] = (unsigned)cum;
  }
  for (int k = a.n; k < PRUNE_MAX_TENSORS; k++) a.end[k] = (unsigned)cum;
  if (cum == 0) return hipSuccess;
  ProfScope ps(K_PRUNE_COMPACT, s);
  hipLaunchKernelGGL(k_prune_compact, dim3((unsigned)cum), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_prune_workspace(int P) {
  if (P <= 0 || P > GSR_PRUNE_MAX_ROWS) return 0;
  return prune_workspace_bytes(P);
}

int gsr_prune_mark(int P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                   const float* opacity_raw, const unsigned char* drop, float min_opacity, float max_scale,
                   int drop_nonfinite, unsigned char* reasons, int* row_map, int* counts5, char* workspace,
                   size_t workspace_bytes, void* stream_) {
  clear_error();
  if (P < 0 || P > GSR_PRUNE_MAX_ROWS) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
  if (!row_map || !counts5) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (P > 0 && (!xyz || !scaling_raw || !rotation_raw || !opacity_raw || !reasons || !workspace))
    return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_aligned4((uintptr_t)xyz | (uintptr_t)scaling_raw | (uintptr_t)rotation_raw | (uintptr_t)opacity_raw |
                             (uintptr_t)row_map | (uintptr_t)counts5 | (uintptr_t)workspace))
    return e;
  if (int e = check_workspace(workspace_bytes, prune_workspace_bytes(P))) return e;
  hipStream_t s = (hipStream_t)stream_;
  const int nblocks = (int)prune_blocks(P);
  int* totals = reinterpret_cast<int*>(workspace);
  if (nblocks) {
    ProfScope ps(K_PRUNE_MARK, s);
    hipLaunchKernelGGL(k_prune_mark, dim3(nblocks), dim3(PRUNE_BLOCK), 0, s, P, xyz, scaling_raw, rotation_raw,
                       opacity_raw, drop, min_opacity, max_scale, drop_nonfinite ? 1 : 0, reasons, totals, nblocks);
  }
  {
    ProfScope ps(K_PRUNE_SCAN, s);
    hipLaunchKernelGGL(k_prune_scan, dim3(1), dim3(PRUNE_BLOCK), 0, s, totals, nblocks, counts5, row_map + P);
  }
  if (nblocks) {
    ProfScope ps(K_PRUNE_RANK, s);
    hipLaunchKernelGGL(k_prune_rank, dim3(nblocks), dim3(PRUNE_BLOCK), 0, s, P, reasons, totals, row_map);
  }
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

int gsr_prune_compact(int P, int n_tensors, const float* const* src, float* const* dst, const int* widths,
                      const unsigned char* reasons, const int* row_map, void* stream_) {
  clear_error();
  if (P < 0 || P > GSR_PRUNE_MAX_ROWS) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
  if (n_tensors < 0 || n_tensors > PRUNE_MAX_TENSORS)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad tensor count: at most %d", PRUNE_MAX_TENSORS);
  if (n_tensors > 0 && !widths) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  for (int k = 0; k < n_tensors; k++)
    if (widths[k] < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad row width (tensor %d)", k);
  if (n_tensors > 0 && prune_compact_blocks(P, n_tensors, widths) > 0x7fffffffull)
    return fail(GSR_ERR_INVALID_ARGUMENT, "model too large for one compaction launch");
  if (P == 0 || n_tensors == 0) return GSR_OK;
  if (!src || !dst || !reasons || !row_map) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  for (int k = 0; k < n_tensors; k++)
    if (widths[k] > 0 && (!src[k] || !dst[k])) return fail(GSR_ERR_INVALID_ARGUMENT, "null tensor pointer (tensor %d)", k);
  if (int e = check_aligned4((uintptr_t)row_map)) return e;
  for (int k = 0; k < n_tensors; k++)
    if (widths[k] > 0 && (((uintptr_t)src[k] | (uintptr_t)dst[k]) & 3u))
      return fail(GSR_ERR_INVALID_ARGUMENT, "%s (tensor %d)", kMisaligned, k);
  HIP_TRY(launch_prune_compact(P, n_tensors, src, dst, widths, reasons, row_map, (hipStream_t)stream_));
  return GSR_OK;
}

}  // extern "C"
