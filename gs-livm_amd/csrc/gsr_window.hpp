// gsr_window.hpp -- the work unit of the 11-tap separable window that loss.hip (forward and backward) and metrics.hip
// share: its constants, the column load, the vertical pass in registers, the hand-over through LDS, the horizontal
// pass, the per-workgroup partial sums, the one-workgroup float64 tree that adds them and the grid on the host.
// Inlined into the including unit: the code inherits that unit's build flags (-fno-slp-vectorize, build.py).
#pragma once
#include "gsr_workgroup.hpp"

namespace gsr {

constexpr int WIN_TAPS = 11;            // window taps
constexpr int WIN_HALO = WIN_TAPS / 2;  // halo
// Work unit of one 256-thread workgroup: 54 x 32 outputs.  Wave w owns the 8 output rows 8w .. 8w+7, lane l the input
// column x0 - 5 + l (64 columns = 54 outputs + the halo), so every global load of the vertical pass is one coalesced
// 256-byte row segment and the pass runs in registers straight from those loads (18 rows -> 8 outputs per moment, taps
// in the order of a plain 11-tap sum); its results cross the workgroup's ONE barrier through LDS and the horizontal pass
// is register-blocked seven outputs to a thread (17 staged values per moment).
constexpr int WIN_TX = 54, WIN_TY = 32;
constexpr int WIN_SEG = 8;                      // output rows per wave
constexpr int WIN_IN = WIN_SEG + 2 * WIN_HALO;  // 18 input rows per wave
constexpr int WIN_HO = 7;                       // horizontal pass: outputs per thread (8 threads x 7 >= 54)
constexpr int WIN_FLAT = (WIN_TX * WIN_TY + 255) / 256;  // 7 elements per thread in the tile's flattened order
constexpr int WIN_STRIDE = 72;  // LDS row stride: (8 r + 7 g + k) mod 64 is conflict-free over a wave's 8 x 8
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;  // loss_utils.cuh:8-9

// The 1-D window, by value in the kernel arguments.  Whatever the caller passes, the reference's own included, which
// is NOT symmetric: correlation (FLIP = false) and its transpose (FLIP = true, taps read flipped) are kept apart.
struct Window {
  float w[WIN_TAPS];
  explicit Window(const float* window11) {
    for (int k = 0; k < WIN_TAPS; k++) w[k] = window11[k];
  }
};

using WindowLds = float[WIN_TY][WIN_STRIDE];  // one vertically filtered moment of the unit

// Grid of the unit over C planes of H x W, and its number of workgroups.
struct WindowGrid {
  dim3 grid;
  size_t units;
  WindowGrid(int C, int H, int W) : grid((W + WIN_TX - 1) / WIN_TX, (H + WIN_TY - 1) / WIN_TY, C),
                                    units((size_t)grid.x * grid.y * grid.z) {}
};

// This lane's column of N planes (pointers to the unit's channel), the 18 rows its wave needs: all N x 18 loads are in
// flight before the first is consumed -- clamped addresses, unconditional loads, zero padding by select (no branch per
// load).  Returns whether the column lies in the image.
template <int N>
__device__ __forceinline__ bool window_load_columns(const float* const (&planes)[N], const int H, const int W,
                                                    const int x0, const int y0, float (&v)[N][WIN_IN]) {
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int gx = x0 - WIN_HALO + lane;
  const bool col_in = gx >= 0 && gx < W;
  const int gxc = min(max(gx, 0), W - 1);
#pragma unroll
  for (int i = 0; i < WIN_IN; i++) {
    const int gy = y0 + WIN_SEG * seg - WIN_HALO + i;
    const int off = min(max(gy, 0), H - 1) * W + gxc;
    float t[N];
#pragma unroll
    for (int p = 0; p < N; p++) t[p] = planes[p][off];
    const bool in = col_in && gy >= 0 && gy < H;
#pragma unroll
    for (int p = 0; p < N; p++) v[p][i] = in ? t[p] : 0.f;
  }
  return col_in;
}

// Vertical pass: Q moments of the 8 output rows of this lane's column into hv, taps in ascending k from 0.f.
// moments(i, m) turns loaded row i into its Q moments.
template <int Q, bool FLIP, class F>
__device__ __forceinline__ void window_vertical(const Window& win, WindowLds* hv, F moments) {
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  float acc[WIN_SEG][Q];
#pragma unroll
  for (int o = 0; o < WIN_SEG; o++) {
#pragma unroll
    for (int q = 0; q < Q; q++) acc[o][q] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < WIN_IN; i++) {
    float m[Q];
    moments(i, m);
#pragma unroll
    for (int o = 0; o < WIN_SEG; o++) {
      const int k = i - o;
      if (k >= 0 && k < WIN_TAPS) {
        const float wk = win.w[FLIP ? WIN_TAPS - 1 - k : k];
#pragma unroll
        for (int q = 0; q < Q; q++) acc[o][q] += wk * m[q];
      }
    }
  }
#pragma unroll
  for (int o = 0; o < WIN_SEG; o++) {
#pragma unroll
    for (int q = 0; q < Q; q++) hv[q][WIN_SEG * seg + o][lane] = acc[o][q];
  }
}

// Horizontal pass, after the barrier: thread t filters row t / 8, its seven outputs from column 7 (t % 8) on (the last
// group reads into the row padding), taps in ascending k from 0.f.
template <int Q, bool FLIP>
__device__ __forceinline__ void window_horizontal(const Window& win, const WindowLds* hv, float (&m)[Q][WIN_HO]) {
  const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * WIN_HO;
#pragma unroll
  for (int q = 0; q < Q; q++) {
    float v[WIN_HO + WIN_TAPS - 1];
#pragma unroll
    for (int k = 0; k < WIN_HO + WIN_TAPS - 1; k++) v[k] = hv[q][r][c0 + k];
#pragma unroll
    for (int o = 0; o < WIN_HO; o++) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < WIN_TAPS; k++) a += win.w[FLIP ? WIN_TAPS - 1 - k : k] * v[o + k];
      m[q][o] = a;
    }
  }
}

// Fixed-order workgroup reduction of N per-thread sums -> N partials of this workgroup, ordered by channel
// (blockIdx.z major): partials[N * b + q].  `red`: [N][4] floats; one barrier.
template <int N>
__device__ __forceinline__ void window_store_partials(float (&v)[N], float (*red)[4], float* __restrict__ partials) {
#pragma unroll
  for (int q = 0; q < N; q++) v[q] = wave_sum(v[q]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < N; q++) red[q][threadIdx.x >> 6] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#pragma unroll
    for (int q = 0; q < N; q++) partials[N * b + q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  }
}

// Sum of N values per thread over ONE 1024-thread workgroup in a fixed association order (the callers' thread-strided
// f64 sums, then this tree): deterministic.  THREAD 0 receives the sums in v, nobody else.  `r`: [N][1024] doubles.
// Calls may follow each other on one `r`: behind the last barrier only thread 0 reads, and only its own slot.
template <int N>
__device__ __forceinline__ void tree_sum_1024(double (&v)[N], double (*r)[1024]) {
#pragma unroll
  for (int q = 0; q < N; q++) r[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int q = 0; q < N; q++) r[q][threadIdx.x] += r[q][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < N; q++) v[q] = r[q][0];
  }
}

}  // namespace gsr
