// densify.hip -- adaptive density control: the view-space gradient statistics, the clone / split rule and the in-place
// clone and split of rows together with their Adam moments (the growing counterpart of prune.hip).  The reference
// carries the remains of it -- densification_postfix (src/gs/gaussian.cu:521-540), the commented _xyz_gradient_accum /
// _max_radii2D (:362, :398, :535-537), cat_tensors_to_optimizer (:451-472) -- and never runs the loop, so this is an
// extension; the rule is upstream 3D-Gaussian-splatting's densify_and_clone / densify_and_split with N = 2.
//
// Launches: ONE per view for the statistics, THREE for the marks, ONE for the surgery, whatever P.
//   k_density_accumulate  one thread per row: stats[i] = {grad_sum + |dL_dmean2D.xy|, views + 1, max(max_radius, radius)}
//                         for a visible row with a finite norm; any other row is not touched
//   k_densify_mark        one thread per row: the rule -> kinds[P] (0 none, 1 clone, 2 split), still uncapped; per-workgroup
//                         totals of candidates and of splits
//   k_densify_scan        ONE workgroup: exclusive scan of the candidate totals (in place), the accepted splits under the
//                         cap (whole workgroups from their totals, the one workgroup the cap cuts through from its 256
//                         kinds), counts3 and offsets[P]
//   k_densify_rank        one thread per row: offsets[i] = min(workgroup base + rank, cap); a candidate at or beyond the cap
//                         loses its mark
//   k_densify_apply       one thread per SOURCE row: a marked row writes row P + offsets[i] (and, for a split, itself)
// No workgroup waits for another, no atomics: every output is the same whatever the order the workgroups run in.  Plain
// vector loads and stores only.  This file is built with -ffp-contract=off, so the accumulated norm and the marks can be
// restated bit for bit in float32 on a host (sqrtf and the division are correctly rounded).
//
// The surgery is in place and race free: a thread reads only its own row i < P, and writes only row i and row
// P + offsets[i] >= P, which no other thread reads or writes.  The parent of a split becomes its first child in place,
// so every existing row keeps its number (VoxelIndex needs no remap) and nothing is compacted.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

constexpr int DENSIFY_BLOCK = WG_THREADS;  // rows per workgroup (4 waves)
constexpr float LN_1_6 = 0.47000363f;  // log(0.8 * 2): a child's scale is the parent's / 1.6

inline size_t densify_blocks(int P) { return ((size_t)P + DENSIFY_BLOCK - 1) / DENSIFY_BLOCK; }
// [2][nblocks] int32: [0] candidates per workgroup -> their exclusive scan; [1] splits per workgroup
static size_t densify_workspace_bytes(int P) { return P > 0 ? 2 * densify_blocks(P) * sizeof(int) : 0; }

__global__ __launch_bounds__(DENSIFY_BLOCK) void k_density_accumulate(const int P, const int* __restrict__ radii,
                                                                      const float* __restrict__ dL_dmean2D,
                                                                      float* __restrict__ stats) {
  const int i = blockIdx.x * DENSIFY_BLOCK + threadIdx.x;
  if (i >= P) return;
  const int r = radii[i];
  if (r <= 0) return;
  const size_t i3 = 3 * (size_t)i;
  const float gx = dL_dmean2D[i3], gy = dL_dmean2D[i3 + 1];
  const float n = sqrtf(gx * gx + gy * gy);
  if (nonfinite_(n)) return;
  stats[i3] += n;
  stats[i3 + 1] += 1.0f;
  stats[i3 + 2] = fmaxf(stats[i3 + 2], (float)r);
}

// The activated scale is k_activate's bit for bit (same expf); the size comparison is strict, as the prune rule's.
__global__ __launch_bounds__(DENSIFY_BLOCK) void k_densify_mark(const int P, const float* __restrict__ stats,
                                                                const float* __restrict__ scaling_raw,
                                                                const float grad_threshold, const float size_threshold,
                                                                unsigned char* __restrict__ kinds,
                                                                int* __restrict__ totals, const int nblocks) {
  __shared__ int sh[WG_WAVES][2];
  const int i = blockIdx.x * DENSIFY_BLOCK + threadIdx.x;
  unsigned kind = 0;
  if (i < P) {
    const size_t i3 = 3 * (size_t)i;
    const float grad_sum = stats[i3], views = stats[i3 + 1];
    const float avg = views > 0.f ? grad_sum / views : 0.f;
    const float s0 = scaling_raw[i3], s1 = scaling_raw[i3 + 1], s2 = scaling_raw[i3 + 2];
    if (avg >= grad_threshold && !(nonfinite_(s0) || nonfinite_(s1) || nonfinite_(s2)))
      kind = (expf(s0) > size_threshold || expf(s1) > size_threshold || expf(s2) > size_threshold) ? 2u : 1u;
    kinds[i] = (unsigned char)kind;
  }
  const int n[2] = {(int)__popcll(__ballot(kind != 0)), (int)__popcll(__ballot(kind == 2))};  // candidates, splits
  store_block_totals(n, sh, totals, nblocks);
}

// ONE workgroup.  totals[0][.] -> exclusive scan in place (scan_totals).  cap: max_new, or INT_MAX for "unlimited".
// A workgroup that ends at or below the cap contributes its split total; at most one workgroup starts below the cap
// and ends beyond it, and its accepted splits are counted from its kinds.  nblocks == 0 (P == 0) writes zeros.
__global__ __launch_bounds__(DENSIFY_BLOCK) void k_densify_scan(const int P, const unsigned char* __restrict__ kinds,
                                                                int* __restrict__ totals, const int nblocks,
                                                                const int cap, int* __restrict__ counts3,
                                                                int* __restrict__ offsets_end) {
  __shared__ int sh[WG_WAVES];
  __shared__ int sh_cut[2];  // the workgroup the cap cuts through and its first offset
  if (threadIdx.x == 0) sh_cut[0] = -1;  // (visible to the items: they run behind the barriers of their pass)
  int splits = 0;
  const int carry = scan_totals(totals, nblocks, sh, [&](int j, int base, int total) {
    if (base + total <= cap) splits += totals[(size_t)nblocks + j];
    else if (base < cap) { sh_cut[0] = j; sh_cut[1] = base; }
  });
  __syncthreads();
  const int cut = sh_cut[0];
  if (cut >= 0) {  // (uniform)
    const long long i = (long long)cut * DENSIFY_BLOCK + threadIdx.x;
    const unsigned kind = i < P ? kinds[i] : 0u;
    const int rank = rank_in_block(kind != 0, sh);
    if (kind == 2 && sh_cut[1] + rank < cap) splits++;
  }
  const int n_split = block_sum(splits, sh);
  if (threadIdx.x == 0) {
    const int n_new = carry < cap ? carry : cap;
    counts3[0] = n_new;
    counts3[1] = n_new - n_split;
    counts3[2] = n_split;
    *offsets_end = n_new;
  }
}

__global__ __launch_bounds__(DENSIFY_BLOCK) void k_densify_rank(const int P, unsigned char* __restrict__ kinds,
                                                                const int* __restrict__ bases, const int cap,
                                                                int* __restrict__ offsets) {
  __shared__ int sh[WG_WAVES];
  const int i = blockIdx.x * DENSIFY_BLOCK + threadIdx.x;
  const bool cand = i < P && kinds[i] != 0;
  const int at = bases[blockIdx.x] + rank_in_block(cand, sh);
  if (i < P) {
    offsets[i] = at < cap ? at : cap;
    if (cand && at >= cap) kinds[i] = 0;
  }
}

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key k[2]
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// z ~ N(0, I3) of child c of row i (include/gsraster.h): depends on (seed, i, c) only
__device__ __forceinline__ void split_normal(uint32_t k0, uint32_t k1, uint32_t i, uint32_t c, float z[3]) {
  uint32_t o[4] = {i, c, 0u, 0u};
  philox4x32_10(o, k0, k1);
  float u[4];
#pragma unroll
  for (int k = 0; k < 4; k++) u[k] = ((float)(o[k] >> 9) + 0.5f) * 1.1920928955078125e-7f;  // exact: 2n + 1 < 2^24
  const float r1 = sqrtf(-2.0f * logf(u[0])), t1 = 6.2831855f * u[1];
  const float r2 = sqrtf(-2.0f * logf(u[2])), t2 = 6.2831855f * u[3];
  z[0] = r1 * cosf(t1); z[1] = r1 * sinf(t1); z[2] = r2 * cosf(t2);
}

struct DensifyArgs {
  float* p[6];  // xyz, features_dc, features_rest, scaling, rotation, opacity
  float* m[6];  // exp_avg    (all null: no moments)
  float* v[6];  // exp_avg_sq
  float* stats;
  const unsigned char* kinds;
  const int* offsets;
  int P, M;
  uint32_t k0, k1;
};

__device__ __forceinline__ void zero_row(float* __restrict__ t, size_t row, int w) {
  if (!t) return;
  for (int e = 0; e < w; e++) t[row * w + e] = 0.f;
}

__global__ __launch_bounds__(DENSIFY_BLOCK) void k_densify_apply(const DensifyArgs a) {
  const int i = blockIdx.x * DENSIFY_BLOCK + threadIdx.x;
  if (i >= a.P) return;
  const unsigned kind = a.kinds[i];
  if (kind == 0) return;
  const size_t src = (size_t)i, dst = (size_t)a.P + (size_t)a.offsets[i];
  const int width[6] = {3, 3, 3 * (a.M - 1), 3, 4, 1};
  const bool split = kind == 2;
  float c0[3], c1[3], s[3];
  if (split) {
    float x[3], q[4], sg[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { x[k] = a.p[0][3 * src + k]; s[k] = a.p[3][3 * src + k]; sg[k] = expf(s[k]); }
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = a.p[4][4 * src + k];
    // torch::nn::functional::normalize, as k_activate: x / max(||x||_2, 1e-12); component order w, x, y, z
    const float inv = 1.0f / fmaxf(sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]), 1e-12f);
    const float w = q[0] * inv, qx = q[1] * inv, qy = q[2] * inv, qz = q[3] * inv;
    const float R[3][3] = {{1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - w * qz), 2.f * (qx * qz + w * qy)},
                           {2.f * (qx * qy + w * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - w * qx)},
                           {2.f * (qx * qz - w * qy), 2.f * (qy * qz + w * qx), 1.f - 2.f * (qx * qx + qy * qy)}};
    float z0[3], z1[3];
    split_normal(a.k0, a.k1, (uint32_t)i, 0u, z0);
    split_normal(a.k0, a.k1, (uint32_t)i, 1u, z1);
#pragma unroll
    for (int k = 0; k < 3; k++) { z0[k] *= sg[k]; z1[k] *= sg[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      c0[k] = x[k] + ((R[k][0] * z0[0] + R[k][1] * z0[1]) + R[k][2] * z0[2]);
      c1[k] = x[k] + ((R[k][0] * z1[0] + R[k][1] * z1[1]) + R[k][2] * z1[2]);
      s[k] -= LN_1_6;
    }
  }
#pragma unroll
  for (int t = 0; t < 6; t++) {
    const int w = width[t];  // 0: _features_rest at M = 1, whose pointers are not looked at
    if (w == 0) continue;
    if (!(split && (t == 0 || t == 3)))
      for (int e = 0; e < w; e++) a.p[t][dst * w + e] = a.p[t][src * w + e];
    zero_row(a.m[t], dst, w);
    zero_row(a.v[t], dst, w);
    if (split) { zero_row(a.m[t], src, w); zero_row(a.v[t], src, w); }
  }
  if (split) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      a.p[0][3 * src + k] = c0[k]; a.p[0][3 * dst + k] = c1[k];
      a.p[3][3 * src + k] = s[k]; a.p[3][3 * dst + k] = s[k];
    }
    zero_row(a.stats, src, 3);
  }
  zero_row(a.stats, dst, 3);
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_density_accumulate(int P, const int* radii, const float* dL_dmean2D, float* stats, void* stream_) {
  clear_error();
  if (P < 0 || P > GSR_PRUNE_MAX_ROWS) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
  if (P == 0) return GSR_OK;
  if (!radii || !dL_dmean2D || !stats) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_aligned4((uintptr_t)radii | (uintptr_t)dL_dmean2D | (uintptr_t)stats)) return e;
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_DENSITY_ACCUMULATE, s);
  hipLaunchKernelGGL(k_density_accumulate, dim3((unsigned)densify_blocks(P)), dim3(DENSIFY_BLOCK), 0, s, P, radii,
                     dL_dmean2D, stats);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

size_t gsr_densify_workspace(int P) {
  if (P <= 0 || P > GSR_PRUNE_MAX_ROWS) return 0;
  return densify_workspace_bytes(P);
}

int gsr_densify_mark(int P, const float* stats, const float* scaling_raw, float grad_threshold, float size_threshold,
                     int max_new, unsigned char* kinds, int* offsets, int* counts3, char* workspace,
                     size_t workspace_bytes, void* stream_) {
  clear_error();
  if (P < 0 || P > GSR_PRUNE_MAX_ROWS) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
  if (!offsets || !counts3) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (P > 0 && (!stats || !scaling_raw || !kinds || !workspace)) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_aligned4((uintptr_t)stats | (uintptr_t)scaling_raw | (uintptr_t)offsets | (uintptr_t)counts3 |
                             (uintptr_t)workspace))
    return e;
  if (int e = check_workspace(workspace_bytes, densify_workspace_bytes(P))) return e;
  hipStream_t s = (hipStream_t)stream_;
  const int nblocks = (int)densify_blocks(P);
  const int cap = max_new < 0 ? 0x7fffffff : max_new;
  int* totals = reinterpret_cast<int*>(workspace);
  if (nblocks) {
    ProfScope ps(K_DENSIFY_MARK, s);
    hipLaunchKernelGGL(k_densify_mark, dim3(nblocks), dim3(DENSIFY_BLOCK), 0, s, P, stats, scaling_raw, grad_threshold,
                       size_threshold, kinds, totals, nblocks);
  }
  {
    ProfScope ps(K_DENSIFY_SCAN, s);
    hipLaunchKernelGGL(k_densify_scan, dim3(1), dim3(DENSIFY_BLOCK), 0, s, P, kinds, totals, nblocks, cap, counts3,
                       offsets + P);
  }
  if (nblocks) {
    ProfScope ps(K_DENSIFY_RANK, s);
    hipLaunchKernelGGL(k_densify_rank, dim3(nblocks), dim3(DENSIFY_BLOCK), 0, s, P, kinds, totals, cap, offsets);
  }
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

int gsr_densify_apply(int P, int M, int n_new, const unsigned char* kinds, const int* offsets, unsigned long long seed,
                      float* xyz, float* features_dc, float* features_rest, float* scaling_raw, float* rotation_raw,
                      float* opacity_raw, float* const* exp_avg6, float* const* exp_avg_sq6, float* stats,
                      void* stream_) {
  clear_error();
  if (P < 0 || n_new < 0 || (long long)P + (long long)n_new > (long long)GSR_PRUNE_MAX_ROWS)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad P/n_new");
  if (M < 1 || M > 16) return fail(GSR_ERR_INVALID_ARGUMENT, "bad M");
  if (P == 0 || n_new == 0) return GSR_OK;
  float* const params6[6] = {xyz, features_dc, M > 1 ? features_rest : nullptr, scaling_raw, rotation_raw, opacity_raw};
  if (!kinds || !offsets) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  for (int k = 0; k < 6; k++) {
    if (k == 2 && M == 1) continue;  // _features_rest at M = 1: its pointers are not looked at
    if (!params6[k] || (exp_avg6 && !exp_avg6[k]) || (exp_avg_sq6 && !exp_avg_sq6[k]))
      return fail(GSR_ERR_INVALID_ARGUMENT, "null tensor pointer (group %d)", k);
  }
  uintptr_t bits = (uintptr_t)offsets | (uintptr_t)stats;
  for (int k = 0; k < 6; k++) {
    if (k == 2 && M == 1) continue;
    bits |= (uintptr_t)params6[k] | (uintptr_t)(exp_avg6 ? exp_avg6[k] : nullptr) |
            (uintptr_t)(exp_avg_sq6 ? exp_avg_sq6[k] : nullptr);
  }
  if (int e = check_aligned4(bits)) return e;
  hipStream_t s = (hipStream_t)stream_;
  DensifyArgs a;
  for (int t = 0; t < 6; t++) {
    const bool has = t != 2 || M > 1;
    a.p[t] = has ? params6[t] : nullptr;
    a.m[t] = has && exp_avg6 ? exp_avg6[t] : nullptr;
    a.v[t] = has && exp_avg_sq6 ? exp_avg_sq6[t] : nullptr;
  }
  a.stats = stats; a.kinds = kinds; a.offsets = offsets; a.P = P; a.M = M;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  ProfScope ps(K_DENSIFY_APPLY, s);
  hipLaunchKernelGGL(k_densify_apply, dim3((unsigned)densify_blocks(P)), dim3(DENSIFY_BLOCK), 0, s, a);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
