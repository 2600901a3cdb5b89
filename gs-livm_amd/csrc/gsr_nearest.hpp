// gsr_nearest.hpp -- what the LiDAR terms on a selection of Gaussians share (simi.hip, surfel.hip), each written once:
// the launch plan, the nearest-selected-centre search with its tie rule, and the walk that hands every selected row the
// records of the points that chose it.  A term has three launches in this shape:
//   nearest   lane = point, workgroup = 64 points x one chunk of the gathered centres (staged through LDS 256 at a
//             time, each of the four waves scans a quarter of a tile): per (point, chunk) the smallest squared distance
//             and its position in `sel` (nearest_chunk_scan); the workgroups of the first point block also see every
//             selected row once (the term's per-row side job)
//   points    thread = point: the fixed-order minimum over the chunks (nearest_over_chunks), then the term's own
//             arithmetic and the point's record: the position of its centre in `sel` or -1, and N floats
//   grads     thread = selected row: sums the records that name it, in ascending point order (sum_records: a
//             deterministic many-to-one accumulation without atomics), then the term's own gradients (store_row)
// THE TIE RULE: of two centres at bit-equal squared distance the one at the LOWER position in `sel` wins -- inside a
// wave's quarter (ascending positions, strict <), between the four waves (the position itself settles it), between the
// chunks (ascending, strict <).  Every comparison here keeps its strictness and every sum its order: both are part of
// the behaviour (tests/test_gpu_simi.py, tests/test_gpu_plane.py hold the terms to it bit for bit).
// Inlined into the including unit, whose build flags it inherits (build.py) -- and it must give the same bits with and
// without -ffp-contract=off: the one multiply-add chain is written out with __builtin_fmaf, nothing else here multiplies
// into an add.  The workgroup functions are for 256 threads and are called by ALL threads of the workgroup (barriers).
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_api.hpp"

namespace gsr {

constexpr int NEAREST_PTS = 64;           // points per workgroup of the search (one per lane)
constexpr int NEAREST_TILE = 256;         // centres staged per LDS tile (one per thread; 4 KiB: occupancy is not LDS-bound)
constexpr int NEAREST_TARGET_WGS = 1024;  // the search's grid aims at four workgroups on each of the 256 CUs, once
constexpr int NEAREST_REC_TILE = 1024;    // records staged per LDS tile of sum_records
constexpr int NEAREST_MAX_N = 0x7fffffff - 1024;  // (positions in `sel`, padded to a tile, stay ints)

struct NearestPlan {
  int pblocks, ntiles, tiles_per_chunk, nchunks, nblocks2;
};

inline NearestPlan nearest_plan(int m, int n) {
  NearestPlan p;
  p.pblocks = (m + NEAREST_PTS - 1) / NEAREST_PTS;
  p.ntiles = (n + NEAREST_TILE - 1) / NEAREST_TILE;
  // the work is latency-bound at the sizes of the loop (4-16 M distances): as many chunks as fill the device once, no
  // more (every chunk costs each point one partial record)
  int want = NEAREST_TARGET_WGS / (p.pblocks > 0 ? p.pblocks : 1);
  if (want < 1) want = 1;
  if (want > p.ntiles) want = p.ntiles;
  if (want < 1) want = 1;
  p.tiles_per_chunk = (p.ntiles + want - 1) / want;
  if (p.tiles_per_chunk < 1) p.tiles_per_chunk = 1;
  p.nchunks = (p.ntiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk;  // (no empty chunk)
  p.nblocks2 = (m + 255) / 256;
  return p;
}

// The refusals every entry point of the family starts with: GSR_OK, or the error as fail() left it.
inline int check_selection_sizes(int P, int m, int n) {
  if (P < 0 || m < 0 || n < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P/m/n");
  if (n > P) return fail(GSR_ERR_INVALID_ARGUMENT, "n = %d selected rows of P = %d (the selection is unique)", n, P);
  if (n > NEAREST_MAX_N) return fail(GSR_ERR_INVALID_ARGUMENT, "n too large");
  return GSR_OK;
}

// A row index of `sel` as the kernels use it for READS: clamped into [0, P), so that a selection that breaks its
// contract (each < P) reads a wrong row instead of foreign memory; writes test the unclamped index and are skipped.
__device__ __forceinline__ int clamp_row(int row, int P) { return min(max(row, 0), P - 1); }

// The search of one workgroup (blockIdx.x: block of 64 points, blockIdx.y: chunk of tiles_per_chunk tiles): writes
// part_d2 / part_k [blockIdx.y][i] for its points.  side(k, row3) runs once for every position k < n of the chunk, in
// the workgroups of the first point block only, on the thread that stages the centre; row3 = 3 * the (clamped) row,
// the offset of the row's first element in an [P][3] array.
template <class Side>
__device__ __forceinline__ void nearest_chunk_scan(const int P, const int m, const int n, const int tiles_per_chunk,
                                                   const int ntiles, const float* points,
                                                   const int* sel, const float* xyz,
                                                   float* part_d2, int* part_k, Side side) {
  __shared__ float4 cs[NEAREST_TILE];   // one broadcast ds_read_b128 per centre
  __shared__ float wd2[4][NEAREST_PTS];
  __shared__ int wk[4][NEAREST_PTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * NEAREST_PTS + lane;
  const int ic = min(i, m - 1);
  const float px = points[3 * (size_t)ic], py = points[3 * (size_t)ic + 1], pz = points[3 * (size_t)ic + 2];
  const int t0 = blockIdx.y * tiles_per_chunk, t1 = min(t0 + tiles_per_chunk, ntiles);
  const bool first = blockIdx.x == 0;  // (uniform over the workgroup)
  float best = __builtin_inff();
  int bestk = -1;
  for (int t = t0; t < t1; t++) {
    const int k = t * NEAREST_TILE + (int)threadIdx.x;
    // a slot past the end holds a centre no finite point is near: its squared distance overflows to +inf, which never
    // passes the strict comparison
    float4 c = make_float4(3e38f, 3e38f, 3e38f, 0.f);
    if (k < n) {
      const size_t row3 = 3 * (size_t)clamp_row(sel[k], P);  // (formed once, for the centre and for the side job)
      c.x = xyz[row3]; c.y = xyz[row3 + 1]; c.z = xyz[row3 + 2];
      if (first) side(k, row3);
    }
    __syncthreads();  // (the previous tile has been scanned)
    cs[threadIdx.x] = c;
    __syncthreads();
    const int j0 = wave * 64;
#pragma unroll 8
    for (int j = 0; j < 64; j++) {
      const float4 q = cs[j0 + j];
      const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
      const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
      if (d2 < best) { best = d2; bestk = t * NEAREST_TILE + j0 + j; }  // ascending positions, strict: the lowest wins a tie
    }
  }
  wd2[wave][lane] = best;
  wk[wave][lane] = bestk;
  __syncthreads();
  if (wave == 0 && i < m) {
    float b = wd2[0][lane];
    int bk = wk[0][lane];
#pragma unroll
    for (int w = 1; w < 4; w++) {
      const float d = wd2[w][lane];
      const int kk = wk[w][lane];
      // within a tile the waves scan ascending quarters, but over several tiles wave 0 may hold a LATER position than
      // wave 1: equal distances are settled by the position itself
      if (d < b || (d == b && kk >= 0 && (bk < 0 || kk < bk))) { b = d; bk = kk; }
    }
    const size_t o = (size_t)blockIdx.y * m + i;
    part_d2[o] = b;
    part_k[o] = bk;
  }
}

// Point i's nearest centre over all chunks: its squared distance and its position in `sel` (-1: no centre compared
// below +inf).
struct NearestHit {
  float d2;
  int k;
};
__device__ __forceinline__ NearestHit nearest_over_chunks(const float* part_d2, const int* part_k, const int m,
                                                          const int nchunks, const int i) {
  float best = __builtin_inff();
  int bk = -1;
  for (int c = 0; c < nchunks; c++) {  // ascending chunks hold ascending positions: strict, the lowest wins a tie
    const float d = part_d2[(size_t)c * m + i];
    const int kk = part_k[(size_t)c * m + i];
    if (d < best) { best = d; bk = kk; }
  }
  return {best, bk};
}

// acc[0 .. N) += the rows rec_g[i][0 .. N) of the records with rec_k[i] == kq, i ascending over the m points: the sum
// of a row that many points share has ONE order.  rec_k is staged through LDS 1024 at a time; kq = -2 matches no record
// (a thread without a row still helps to stage).
template <int N>
__device__ __forceinline__ void sum_records(const int m, const int* rec_k, const float* rec_g,
                                            const int kq, float (&acc)[N]) {
  __shared__ __attribute__((aligned(16))) int sk[NEAREST_REC_TILE];
  for (int base = 0; base < m; base += NEAREST_REC_TILE) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NEAREST_REC_TILE / 256; q++) {
      const int i = base + q * 256 + (int)threadIdx.x;
      sk[q * 256 + threadIdx.x] = i < m ? rec_k[i] : -1;
    }
    __syncthreads();
    const int cntv = min(NEAREST_REC_TILE, m - base);
    for (int q = 0; q < cntv; q += 4) {
      const int4 v = *reinterpret_cast<const int4*>(&sk[q]);  // (the same address in every lane: a broadcast read)
      if (v.x == kq || v.y == kq || v.z == kq || v.w == kq) {
        const int e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; u++)
          if (e[u] == kq) {
            const float* g = rec_g + N * (size_t)(base + q + u);
#pragma unroll
            for (int c = 0; c < N; c++) acc[c] += g[c];
          }
      }
    }
  }
}

// One row of a gradient: written, or added to what the caller's buffer holds.
template <int N>
__device__ __forceinline__ void store_row(float* g, const float (&v)[N], const int accumulate) {
  if (accumulate) {
#pragma unroll
    for (int c = 0; c < N; c++) g[c] += v[c];
  } else {
#pragma unroll
    for (int c = 0; c < N; c++) g[c] = v[c];
  }
}

}  // namespace gsr
