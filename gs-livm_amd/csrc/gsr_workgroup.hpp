// gsr_workgroup.hpp -- the device idioms the kernels around the rasterizer share, each written once: wave and workgroup
// sums, the rank of a marked row, per-workgroup ballot totals and their one-workgroup scan.  Every workgroup function
// here is for 256 threads = four waves of 64 and is called by ALL threads of the workgroup (they hold barriers).
// The order of every floating-point sum is part of the behaviour (bit equality from run to run and from route to route
// is asserted in tests/): butterfly inside a wave, then the four wave sums as (s0 + s1) + (s2 + s3).
// Inlined into the including unit: the code inherits that unit's build flags (build.py).
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

constexpr int WG_THREADS = 256;          // threads per workgroup of every function below
constexpr int WG_WAVES = WG_THREADS / 64;
constexpr int TOTALS_SCAN_ITEMS = 4;     // consecutive workgroup totals per thread of scan_totals: 1024 per pass
constexpr float COORD_MAX_ = 1073741824.f;  // 2^30: beyond it (or not finite) a coordinate is never converted to an integer

__device__ __forceinline__ bool nonfinite_(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }

// Sum over the 64 lanes of a wave (int, float or double), xor-butterfly: every lane receives the result, in one fixed
// order.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum of one value per thread (double or int) over the workgroup, in a fixed order: xor-butterfly inside each wave,
// then the four wave sums as (s0 + s1) + (s2 + s3).  Every thread receives the result.  `sh` holds 4 values; two
// barriers, the first of which makes back-to-back calls on one `sh` safe (sh may still be read from an earlier call).
template <class T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// "One f64 partial plus one int count per workgroup", the producing side: both sums of block_sum behind the same two
// barriers.  `shv`: 4 doubles, `shc`: 4 ints.
__device__ __forceinline__ void block_sum_pair(double& v, int& c, double* shv, int* shc) {
  v = wave_sum(v);
  c = wave_sum(c);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shc[threadIdx.x >> 6] = c; }
  __syncthreads();
  v = (shv[0] + shv[1]) + (shv[2] + shv[3]);
  c = (shc[0] + shc[1]) + (shc[2] + shc[3]);
}

// Sum of n per-workgroup f64 partials in ONE fixed order: thread-strided over the partials, then the workgroup tree.
// Every thread receives the result.
__device__ __forceinline__ double partials_sum(const double* __restrict__ part, const int n, double* sh) {
  double s = 0.0;
  for (int b = threadIdx.x; b < n; b += WG_THREADS) s += part[b];
  return block_sum(s, sh);
}

// The finishing side of the pair: the f64 partials and the counts (exact in double) of n workgroups, both loads of a
// pass in flight together, each sum in the order of partials_sum.
__device__ __forceinline__ void partial_pairs_sum(const double* __restrict__ part, const int* __restrict__ cnt,
                                                  const int n, double* sh, double& s, double& c) {
  s = 0.0;
  c = 0.0;
  for (int b = threadIdx.x; b < n; b += WG_THREADS) {
    s += part[b];
    c += (double)cnt[b];
  }
  s = block_sum(s, sh);
  c = block_sum(c, sh);
}

// Rank of a marked row among the marked rows of its workgroup: ballot, popcount below the lane, the waves before.
// `sh`: 4 ints; one barrier.
__device__ __forceinline__ int rank_in_block(bool marked, int* sh) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long b = __ballot(marked);
  if (lane == 0) sh[wave] = __popcll(b);
  __syncthreads();
  int before = __popcll(b & ((1ull << lane) - 1ull));
#pragma unroll
  for (int w = 0; w < WG_WAVES; w++)
    if (w < wave) before += sh[w];
  return before;
}

// K per-wave ballot counts (n[k] = __popcll(__ballot(..)), uniform over the wave) -> per-workgroup totals, written as
// totals[k * nblocks + blockIdx.x].  `sh`: [4][K] ints; one barrier.
template <int K>
__device__ __forceinline__ void store_block_totals(const int (&n)[K], int (*sh)[K], int* __restrict__ totals,
                                                   const int nblocks) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) sh[wave][k] = n[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < WG_WAVES; w++) t += sh[w][threadIdx.x];
    totals[(size_t)threadIdx.x * nblocks + blockIdx.x] = t;
  }
}

struct ScanNoItem {
  __device__ __forceinline__ void operator()(int, int, int) const {}
};

// ONE workgroup.  totals[0 .. nblocks) -> their exclusive scan in place, 1024 workgroup totals per pass of the loop with
// the running sum carried in a register; returns the sum of all of them to every thread.  Each thread owns
// TOTALS_SCAN_ITEMS consecutive totals; the threads' sums are scanned inside the wave with __shfl_up and the waves
// before are added from `sh` (4 ints).  item(j, base, total) runs for every j < nblocks with its scanned base and its
// total before the scan, on the thread that owns j, after the pass's barriers.  nblocks == 0 returns 0.
template <class F = ScanNoItem>
__device__ __forceinline__ int scan_totals(int* __restrict__ totals, const int nblocks, int* sh, F item = F()) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int carry = 0;
  for (int base = 0; base < nblocks; base += WG_THREADS * TOTALS_SCAN_ITEMS) {  // (uniform trip count)
    const int j0 = base + (int)threadIdx.x * TOTALS_SCAN_ITEMS;
    int v[TOTALS_SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int k = 0; k < TOTALS_SCAN_ITEMS; k++) {
      v[k] = j0 + k < nblocks ? totals[j0 + k] : 0;
      mine += v[k];
    }
    int incl = mine;  // inclusive scan of the threads' sums inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    __syncthreads();  // the previous pass has read sh
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    int before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < WG_WAVES; w++) {
      if (w < wave) before += sh[w];
      all += sh[w];
    }
    int run = before + incl - mine;
#pragma unroll
    for (int k = 0; k < TOTALS_SCAN_ITEMS; k++) {
      if (j0 + k < nblocks) {
        totals[j0 + k] = run;
        item(j0 + k, run, v[k]);
      }
      run += v[k];
    }
    carry += all;
  }
  return carry;
}

}  // namespace gsr
