// covis.hip -- keyframe covisibility: one bit per (keyframe, Gaussian), kept on the device (an extension: the reference
// draws its training views blindly, lioOptimization.cpp:1573-1641; MonoGS and SplaTAM keep what is kept here).
//
// A visibility row is `words` little-endian 64-bit words: bit i % 64 of word i / 64 belongs to model row i.  The rows of
// several keyframes lie in one slab with a row pitch counted in words.  All four kernels are integer arithmetic: every
// result is exact, independent of the order the workgroups run in, and the same on every run.
//
//   k_visibility_pack     one __ballot = one word: bit = radii[i] > 0 (or mask[i] != 0).  A wave makes eight consecutive
//                         words (its eight loads per lane are in flight together) and stores them with one
//                         instruction, lane j word j.  Every word of the row is written, bits at and beyond P are zero.
//   k_visibility_overlap  workgroup = 8 query rows x 256 word columns: the eight query words of a thread's column stay in
//                         registers, the keyframe rows stream past them (one coalesced 8-byte load per thread and
//                         keyframe, used eight times).  The eight popcounts of a keyframe are summed over the wave in
//                         TEN shuffles (a halving exchange: 8 values -> 4 -> 2 -> 1, then three butterfly steps), and
//                         the partial counts of the four waves meet in LDS; the workgroup adds them to inter[q][k] with
//                         32-bit integer atomics, one per (query row, keyframe).
//   k_visibility_count    wave = one word column, lane l = bit l: the load of keyframe k's word is uniform over the wave;
//                         count[i] and / or drop[i] = (i >= first_row && count[i] < min_count) in the same pass.
//   k_visibility_remap    a GATHER, wave = one DESTINATION word: lane l finds the source row of destination row
//                         64 w + l -- the last row whose row_map entry is that number (the dropped rows in front of a
//                         survivor carry the survivor's entry) -- by a binary search over row_map, once; then one
//                         __ballot per keyframe makes the word.  Every destination word is stored exactly once, zeros
//                         beyond P' included: no atomics, no zero fill, nothing out of a row's dst_words words.
// Plain vector loads and stores only.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

constexpr int VIS_BLOCK = WG_THREADS;      // four waves: four words (pack, count, remap), 256 word columns (overlap)
constexpr int PACK_WORDS = 8;              // words a wave of k_visibility_pack makes: eight loads per lane in flight
constexpr int OVERLAP_QTILE = 8;          // query rows held in registers per workgroup
constexpr int OVERLAP_KT = 64;             // keyframes whose partial counts a workgroup gathers in LDS before it adds them

__global__ __launch_bounds__(VIS_BLOCK) void k_visibility_pack(const int P, const int* __restrict__ radii,
                                                               const unsigned char* __restrict__ mask,
                                                               unsigned long long* __restrict__ bits, const int words) {
  // a wave makes PACK_WORDS consecutive words: its loads are all issued before the first ballot needs one
  const long long w0 = ((long long)blockIdx.x * WG_WAVES + (threadIdx.x >> 6)) * PACK_WORDS;  // uniform over the wave
  if (w0 >= words) return;
  const int lane = threadIdx.x & 63;
  bool seen[PACK_WORDS];
#pragma unroll
  for (int j = 0; j < PACK_WORDS; j++) {
    const long long i = (w0 + j) * 64 + lane;  // < P: an int (the entry point keeps words * 64 <= INT_MAX)
    seen[j] = false;
    if (i < P) seen[j] = radii ? radii[i] > 0 : mask[i] != 0;
  }
  unsigned long long mine = 0;  // lane j keeps word w0 + j
#pragma unroll
  for (int j = 0; j < PACK_WORDS; j++) {
    const unsigned long long b = __ballot(seen[j]);
    if (lane == j) mine = b;
  }
  if (lane < PACK_WORDS && w0 + lane < words) bits[w0 + lane] = mine;  // one store of up to 64 consecutive bytes
}

// Sum of eight ints per lane over the 64 lanes of a wave in ten shuffles.  Three halving exchanges: a lane keeps half of
// its values and hands the other half to its partner 32 (16, 8) lanes away, so that after them lane l holds ONE value:
// the sum of value l >> 3 over the eight lanes that differ from l in bits 5, 4, 3.  Three butterfly steps over bits
// 2, 1, 0 finish it: lane l holds the wave's total of value l >> 3.
__device__ __forceinline__ int wave_sum8(int (&v)[8]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const bool up = lane & 32;
    const int got = __shfl_xor(up ? v[j] : v[j + 4], 32, 64);
    v[j] = (up ? v[j + 4] : v[j]) + got;
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const bool up = lane & 16;
    const int got = __shfl_xor(up ? v[j] : v[j + 2], 16, 64);
    v[j] = (up ? v[j + 2] : v[j]) + got;
  }
  {
    const bool up = lane & 8;
    const int got = __shfl_xor(up ? v[0] : v[1], 8, 64);
    v[0] = (up ? v[1] : v[0]) + got;
  }
  int s = v[0];
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// blockIdx.x = tile * chunks + chunk: tile = eight query rows, chunk = 256 word columns.  The outputs are zero when the
// kernel starts (the launch function fills them on the stream).  The partial counts of the four waves meet in LDS (integer
// ds_add), 64 keyframes at a time, and leave the workgroup as ONE global atomic per (query row, keyframe), issued as
// wave instructions over consecutive ints of a row of `inter`.  Zero partial counts add nothing and are skipped.
__global__ __launch_bounds__(VIS_BLOCK) void k_visibility_overlap(
    const int Q, const unsigned long long* __restrict__ q_bits, const long long q_pitch, const int K,
    const unsigned long long* __restrict__ k_bits, const long long k_pitch, const int words, const unsigned chunks,
    int* __restrict__ inter, int* __restrict__ q_count, int* __restrict__ k_count) {
  __shared__ int acc[OVERLAP_QTILE + 1][OVERLAP_KT];  // [8][.]: the keyframe rows' own counts
  __shared__ int acc_q[OVERLAP_QTILE];
  const unsigned tile = blockIdx.x / chunks, chunk = blockIdx.x - tile * chunks;
  const int lane = threadIdx.x & 63;
  const int w = (int)(chunk * (unsigned)VIS_BLOCK + threadIdx.x);
  const bool in = w < words;
  const int q0 = (int)tile * OVERLAP_QTILE;  // < Q
  unsigned long long q[OVERLAP_QTILE];
#pragma unroll
  for (int j = 0; j < OVERLAP_QTILE; j++)
    q[j] = (in && q0 + j < Q) ? q_bits[(long long)(q0 + j) * q_pitch + w] : 0ull;
  const int j_mine = lane >> 3;  // the value whose wave total this lane holds after wave_sum8
  const bool adder = (lane & 7) == 0;
  constexpr int ACC = (OVERLAP_QTILE + 1) * OVERLAP_KT;
  for (int t = threadIdx.x; t < ACC; t += VIS_BLOCK) (&acc[0][0])[t] = 0;
  if (threadIdx.x < OVERLAP_QTILE) acc_q[threadIdx.x] = 0;
  __syncthreads();
  if (q_count) {
    int c[OVERLAP_QTILE];
#pragma unroll
    for (int j = 0; j < OVERLAP_QTILE; j++) c[j] = __popcll(q[j]);
    const int s = wave_sum8(c);
    if (adder && s != 0) atomicAdd(&acc_q[j_mine], s);
  }
  const bool own = k_count && tile == 0;  // the keyframe rows' own counts: once, by the first tile
  for (int kb = 0; kb < K; kb += OVERLAP_KT) {  // (uniform trip counts: every thread meets every barrier)
    const int kn = K - kb < OVERLAP_KT ? K - kb : OVERLAP_KT;
    for (int kk = 0; kk < kn; kk++) {
      const unsigned long long kw = in ? k_bits[(long long)(kb + kk) * k_pitch + w] : 0ull;
      int c[OVERLAP_QTILE];
#pragma unroll
      for (int j = 0; j < OVERLAP_QTILE; j++) c[j] = __popcll(q[j] & kw);
      const int s = wave_sum8(c);
      if (adder && s != 0) atomicAdd(&acc[j_mine][kk], s);
      if (own) {
        const int n = wave_sum(__popcll(kw));
        if (lane == 0 && n != 0) atomicAdd(&acc[OVERLAP_QTILE][kk], n);
      }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ACC; t += VIS_BLOCK) {  // a thread flushes and clears the entries it owns
      const int j = t / OVERLAP_KT, kk = t - j * OVERLAP_KT;
      const int v = acc[j][kk];
      acc[j][kk] = 0;
      if (v != 0 && kk < kn) {
        if (j == OVERLAP_QTILE) atomicAdd(&k_count[kb + kk], v);
        else if (q0 + j < Q) atomicAdd(&inter[(size_t)(q0 + j) * (size_t)K + (size_t)(kb + kk)], v);
      }
    }
    __syncthreads();
  }
  // (K > 0: the loop's barriers are behind the adds to acc_q)
  if (q_count && threadIdx.x < OVERLAP_QTILE && q0 + (int)threadIdx.x < Q && acc_q[threadIdx.x] != 0)
    atomicAdd(&q_count[q0 + threadIdx.x], acc_q[threadIdx.x]);
}

__global__ __launch_bounds__(VIS_BLOCK) void k_visibility_count(const int K, const unsigned long long* __restrict__ bits,
                                                                const long long pitch, const int P, const int words,
                                                                const int first_row, const int min_count,
                                                                int* __restrict__ count, unsigned char* __restrict__ drop) {
  const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * WG_WAVES + (threadIdx.x >> 6));
  if (w >= words) return;  // words = ceil(P / 64)
  const int lane = threadIdx.x & 63;
  const unsigned long long* __restrict__ col = bits + w;
  int c = 0;
#pragma unroll 8
  for (int k = 0; k < K; k++) c += (int)((col[(long long)k * pitch] >> lane) & 1ull);
  const int i = w * 64 + lane;
  if (i < P) {
    if (count) count[i] = c;
    if (drop) drop[i] = (i >= first_row && c < min_count) ? 1 : 0;
  }
}

__global__ __launch_bounds__(VIS_BLOCK) void k_visibility_remap(const int K, const unsigned long long* __restrict__ src,
                                                                const long long src_pitch, const int P,
                                                                const unsigned char* __restrict__ reasons,
                                                                const int* __restrict__ row_map,
                                                                unsigned long long* __restrict__ dst,
                                                                const long long dst_pitch, const int dst_words) {
  const int w = blockIdx.x * WG_WAVES + (threadIdx.x >> 6);  // uniform over the wave
  if (w >= dst_words) return;
  const int lane = threadIdx.x & 63;
  const int d = w * 64 + lane;  // dst_words * 64 <= INT_MAX (the entry point)
  const int P_new = row_map[P];
  // the first row whose entry is beyond d, minus one: row_map[0 .. P) is non-decreasing, and of the rows that share an
  // entry only the last is kept
  int lo = 0, hi = P;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (row_map[mid] <= d) lo = mid + 1; else hi = mid;
  }
  const int i = lo - 1;
  const bool live = d < P_new && i >= 0 && reasons[i] == 0 && row_map[i] == d;
  const unsigned long long* __restrict__ from = src + (live ? (i >> 6) : 0);
  const int bit = i & 63;
  unsigned long long* __restrict__ to = dst + w;
  for (int k = 0; k < K; k++) {
    const bool set = live && ((from[(long long)k * src_pitch] >> bit) & 1ull);
    const unsigned long long b = __ballot(set);
    if (lane == 0) to[(long long)k * dst_pitch] = b;
  }
}

// workgroups of the one overlap launch (the entry point refuses a problem that needs more than a grid holds)
static unsigned long long visibility_overlap_blocks(int Q, int words) {
  const unsigned long long tiles = ((unsigned long long)Q + OVERLAP_QTILE - 1) / OVERLAP_QTILE;
  const unsigned long long chunks = ((unsigned long long)words + VIS_BLOCK - 1) / VIS_BLOCK;
  return tiles * chunks;
}

static long long vis_need(int P) { return ((long long)P + 63) / 64; }
static const long long kVisMaxWords = 0x7fffffffLL / 64;  // words * 64 stays an int32
static const char* const kMisaligned8 = "misaligned pointer: visibility words need 8-byte alignment";

}  // namespace gsr

using namespace gsr;

// ---- the entry points.  The order of the checks is part of the contract (include/gsraster.h): shape, then the choice of
// sources / outputs, then null pointers, then alignment, then (remap) overlapping slabs.
extern "C" {

size_t gsr_visibility_words(int P) { return P > 0 ? (size_t)vis_need(P) : 0; }

int gsr_visibility_pack(int P, const int* radii, const unsigned char* mask, unsigned long long* bits, int words,
                        void* stream_) {
  clear_error();
  if (P <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
  if (words < vis_need(P)) return fail(GSR_ERR_INVALID_ARGUMENT, "words too small: need %lld", vis_need(P));
  if (words > kVisMaxWords) return fail(GSR_ERR_INVALID_ARGUMENT, "words * 64 beyond int32");
  if ((radii != nullptr) == (mask != nullptr))
    return fail(GSR_ERR_INVALID_ARGUMENT, "exactly one of radii and mask is given");
  if (!bits) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if ((uintptr_t)bits & 7u) return fail(GSR_ERR_INVALID_ARGUMENT, "%s", kMisaligned8);
  if (int e = check_aligned4((uintptr_t)radii)) return e;
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_VISIBILITY, s);
  constexpr int per_block = WG_WAVES * PACK_WORDS;
  hipLaunchKernelGGL(k_visibility_pack, dim3((unsigned)((words + per_block - 1) / per_block)), dim3(VIS_BLOCK), 0, s, P,
                     radii, mask, bits, words);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

int gsr_covisibility(int Q, const unsigned long long* q_bits, long long q_pitch, int K,
                     const unsigned long long* k_bits, long long k_pitch, int words, int* inter, int* q_count,
                     int* k_count, void* stream_) {
  clear_error();
  if (Q <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad Q");
  if (K <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad K");
  if (words <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad words");
  if (q_pitch < words || k_pitch < words) return fail(GSR_ERR_INVALID_ARGUMENT, "pitch too small: need %d", words);
  if (words > kVisMaxWords) return fail(GSR_ERR_INVALID_ARGUMENT, "words * 64 beyond int32");
  if ((long long)Q * (long long)K > 0x7fffffffLL) return fail(GSR_ERR_INVALID_ARGUMENT, "Q * K beyond int32");
  if (visibility_overlap_blocks(Q, words) > 0x7fffffffull)
    return fail(GSR_ERR_INVALID_ARGUMENT, "problem too large for one overlap launch");
  if (!q_bits || !k_bits || !inter) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (((uintptr_t)q_bits | (uintptr_t)k_bits) & 7u) return fail(GSR_ERR_INVALID_ARGUMENT, "%s", kMisaligned8);
  if (int e = check_aligned4((uintptr_t)inter | (uintptr_t)q_count | (uintptr_t)k_count)) return e;
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_VISIBILITY, s);
  HIP_TRY(hipMemsetAsync(inter, 0, (size_t)Q * (size_t)K * sizeof(int), s));
  if (q_count) HIP_TRY(hipMemsetAsync(q_count, 0, (size_t)Q * sizeof(int), s));
  if (k_count) HIP_TRY(hipMemsetAsync(k_count, 0, (size_t)K * sizeof(int), s));
  const unsigned chunks = (unsigned)(((unsigned long long)words + VIS_BLOCK - 1) / VIS_BLOCK);
  hipLaunchKernelGGL(k_visibility_overlap, dim3((unsigned)visibility_overlap_blocks(Q, words)), dim3(VIS_BLOCK), 0, s, Q,
                     q_bits, q_pitch, K, k_bits, k_pitch, words, chunks, inter, q_count, k_count);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

int gsr_observation_count(int K, const unsigned long long* bits, long long pitch, int P, int first_row, int min_count,
                          int* count, unsigned char* drop, void* stream_) {
  clear_error();
  if (K <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad K");
  if (P <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
  if (pitch < vis_need(P)) return fail(GSR_ERR_INVALID_ARGUMENT, "pitch too small: need %lld", vis_need(P));
  if (vis_need(P) > kVisMaxWords) return fail(GSR_ERR_INVALID_ARGUMENT, "words * 64 beyond int32");
  if (first_row < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad first_row");
  if (min_count < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad min_count");
  if (!count && !drop) return fail(GSR_ERR_INVALID_ARGUMENT, "neither count nor drop is asked for");
  if (!bits) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if ((uintptr_t)bits & 7u) return fail(GSR_ERR_INVALID_ARGUMENT, "%s", kMisaligned8);
  if (int e = check_aligned4((uintptr_t)count)) return e;
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_VISIBILITY, s);
  const int words = (int)vis_need(P);
  hipLaunchKernelGGL(k_visibility_count, dim3((unsigned)((words + WG_WAVES - 1) / WG_WAVES)), dim3(VIS_BLOCK), 0, s, K,
                     bits, pitch, P, words, first_row, min_count, count, drop);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

int gsr_visibility_remap(int K, const unsigned long long* src, long long src_pitch, int P, const unsigned char* reasons,
                         const int* row_map, unsigned long long* dst, long long dst_pitch, int dst_words,
                         void* stream_) {
  clear_error();
  if (K <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad K");
  if (P <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad P");
  if (dst_words <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "bad dst_words");
  if (src_pitch < vis_need(P)) return fail(GSR_ERR_INVALID_ARGUMENT, "pitch too small: need %lld", vis_need(P));
  if (dst_pitch < dst_words) return fail(GSR_ERR_INVALID_ARGUMENT, "pitch too small: need %d", dst_words);
  if (vis_need(P) > kVisMaxWords || dst_words > kVisMaxWords)
    return fail(GSR_ERR_INVALID_ARGUMENT, "words * 64 beyond int32");
  if (!src || !reasons || !row_map || !dst) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (((uintptr_t)src | (uintptr_t)dst) & 7u) return fail(GSR_ERR_INVALID_ARGUMENT, "%s", kMisaligned8);
  if (int e = check_aligned4((uintptr_t)row_map)) return e;
  {  // the slabs from their first word to the last word of their last row
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + 8u * (uintptr_t)((long long)(K - 1) * src_pitch + vis_need(P));
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + 8u * (uintptr_t)((long long)(K - 1) * dst_pitch + dst_words);
    if (s0 < d1 && d0 < s1) return fail(GSR_ERR_INVALID_ARGUMENT, "src and dst overlap: the remap is out of place");
  }
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_VISIBILITY, s);
  hipLaunchKernelGGL(k_visibility_remap, dim3((unsigned)((dst_words + WG_WAVES - 1) / WG_WAVES)), dim3(VIS_BLOCK), 0, s,
                     K, src, src_pitch, P, reasons, row_map, dst, dst_pitch, dst_words);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
