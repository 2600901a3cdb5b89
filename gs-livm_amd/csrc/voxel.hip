// voxel.hip -- the sweep voxel map: a persistent open-addressing table on the device that voxelises LiDAR sweeps with
// exact, order-independent per-voxel moments, and one oriented Gaussian (a surfel seed) per voxel that matures.  The
// producer-side step between sweep admission (seed.hip) and GrowableGaussians.add_new_pointcloud; it stands where the
// reference walks an unordered_map on the host (GpMap::splitPointsIntoCell / dividePointsIntoCellInitMap,
// src/gp3d/map.cpp).  An extension: one Gaussian per voxel from the moments, no Gaussian-process regression.
//
// The contract (include/gsraster.h, restated in float64 by tests/voxel_ref.py), with g = (double)grid, Q = 2^20:
//   t_k = (double)p_k / g, c_k = floor(t_k); OUT when a t_k is not finite or |c_k| >= Q
//   key = ((c_x + Q) << 42) | ((c_y + Q) << 21) | (c_z + Q)               (every field in 1 .. 2Q - 1: never 0)
//   q_k = min(Q - 1, (int64)floor((t_k - c_k) Q))
//   per voxel, unsigned 64-bit INTEGER atomic adds only: count, S1[3] = sum q_k, S2[6] = sum q_i q_j (xx xy xz yy yz zz),
//   SC[3] = sum clamp(llrint(colour 256), 0, 65535)
// Integer addition commutes: the same bits for every order of the threads and every permutation of the sweep.
//
// One slot = 16 words of 64 bits = 128 bytes:
//   0 key (0 = empty)  1 closed  2 count  3-5 S1  6-11 S2  12-14 SC  15 the call's first point: ~index (0 = untouched)
//
// Launches of gsr_voxel_sweep on the caller's stream, FOUR (ONE when n == 0), all timed under k_visibility (the
// profiler's mask is full):
//   k_voxel_insert  thread = point: key, probe (64-bit compare-and-swap on word 0, at most `capacity` steps), status by
//                   the closed word AS THE PREVIOUS CALL LEFT IT (nothing here writes it), the 13 adds, and a 32-bit
//                   atomic maximum of ~index on word 15 (the minimum of the index)
//   k_voxel_flag    thread = point: the point whose index word 15 holds owns its voxel for this call; it matures when
//                   count >= min_points; per-workgroup totals of the statuses, the matured and the new keys (ballots)
//   k_voxel_scan    ONE workgroup: exclusive scan of the matured totals (scan_totals), counts6
//   k_voxel_emit    thread = point: an owner clears word 15; a matured one writes seed row = workgroup base +
//                   rank_in_block -- the order of first appearance in the call -- and closes the voxel
// No float atomic, no sort, no workgroup waits for another.  Bounds: a point index is tested against n; a slot number
// is hash & (capacity - 1) with capacity a power of two; a seed row is base + rank < matured <= n.
#include "gsr_api.hpp"
#include "gsr_internal.hpp"
#include "gsr_workgroup.hpp"

namespace gsr {

typedef unsigned long long u64;

constexpr int VOX_WORDS = 16;
constexpr long long VOX_Q = 1ll << 20;
constexpr int VOX_MAX_N = 1 << 22, VOX_MAX_MIN_POINTS = 1 << 20;
constexpr long long VOX_MAX_CAPACITY = 1ll << 26;   // 8 GiB of table; the live count stays an int
constexpr int VOX_JACOBI_SWEEPS = 12;               // fixed: the same bits on every run
enum { VOX_ACCUMULATED = 0, VOX_SEEDED = 1, VOX_OUT = 2, VOX_FULL = 3 };
enum { W_KEY = 0, W_CLOSED = 1, W_COUNT = 2, W_S1 = 3, W_S2 = 6, W_SC = 12, W_FIRST = 15 };
constexpr int VOX_TOTALS = 6;   // matured, accumulated, seeded, out, full, new keys

struct VoxelWorkspace {
  int* slots;              // [n] the slot of an ACCUMULATED point
  int* totals;             // [6][nblocks]; [0] -> its exclusive scan
  unsigned char* codes;    // [n] bit 0: owner, bit 1: matured, bit 2: inserted the key
  size_t bytes;
  static VoxelWorkspace carve(char* base, int n) {
    const size_t nblocks = ((size_t)n + WG_THREADS - 1) / WG_THREADS;
    Carver cv = Carver::aligned(base);
    VoxelWorkspace w;
    w.slots = cv.take<int>((size_t)n);
    w.totals = cv.take<int>(VOX_TOTALS * nblocks);
    w.codes = cv.take<unsigned char>((size_t)n);
    w.bytes = cv.bytes();
    return w;
  }
};

struct VoxelArgs {
  int n, min_points;
  double g;                // (double)grid
  double min_var;          // (double)min_sigma squared
  double scale_factor;
  const float* points;     // [n][3]
  const float* colors;     // [n][3] or null
  u64* table;
  long long capacity;
};

__host__ __device__ __forceinline__ u64 voxel_hash(u64 k) {   // (splitmix64's finisher)
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27; k *= 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

// cell and offset of one coordinate; false = OUT
__device__ __forceinline__ bool voxel_cell(const float p, const double g, long long& c, u64& q) {
  const double t = (double)p / g;
  if (!(fabs(t) <= 1.79769313486231570815e308)) return false;   // (NaN and the infinities)
  const double f = floor(t);
  if (!(fabs(f) < (double)VOX_Q)) return false;
  c = (long long)f;
  long long o = (long long)floor((t - f) * (double)VOX_Q);
  q = (u64)(o < VOX_Q - 1 ? o : VOX_Q - 1);
  return true;
}

__device__ __forceinline__ u64 voxel_colour(const float v) {
  const double s = (double)v * 256.0;
  if (!(s > 0.0)) return 0;   // (NaN, zero and the negatives)
  if (s >= 65535.0) return 65535;
  return (u64)llrint(s);
}

__global__ __launch_bounds__(WG_THREADS) void k_voxel_insert(const VoxelArgs a, unsigned char* __restrict__ status,
                                                             long long* __restrict__ point_keys,
                                                             int* __restrict__ slots, unsigned char* __restrict__ codes) {
  const int i = blockIdx.x * WG_THREADS + (int)threadIdx.x;
  if (i >= a.n) return;
  long long c[3];
  u64 q[3];
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; k++) in = voxel_cell(a.points[3 * (size_t)i + k], a.g, c[k], q[k]) && in;
  codes[i] = 0;
  slots[i] = 0;
  if (!in) {
    status[i] = VOX_OUT;
    point_keys[i] = -1;
    return;
  }
  const u64 key = ((u64)(c[0] + VOX_Q) << 42) | ((u64)(c[1] + VOX_Q) << 21) | (u64)(c[2] + VOX_Q);
  point_keys[i] = (long long)key;
  const u64 mask = (u64)a.capacity - 1;
  u64 s = voxel_hash(key) & mask;
  bool found = false, inserted = false;
  for (long long step = 0; step < a.capacity; step++) {   // (bounded by the capacity: the loop always ends)
    u64* slot = a.table + s * VOX_WORDS;
    u64 seen = __hip_atomic_load(&slot[W_KEY], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == 0) {
      seen = atomicCAS(&slot[W_KEY], 0ull, key);
      if (seen == 0) { found = true; inserted = true; break; }
    }
    if (seen == key) { found = true; break; }
    s = (s + 1) & mask;
  }
  if (!found) {
    status[i] = VOX_FULL;
    return;
  }
  u64* slot = a.table + s * VOX_WORDS;
  // written by k_voxel_emit of an earlier call only; a slot claimed in this launch holds the zero it was created with
  if (slot[W_CLOSED] != 0) {
    status[i] = VOX_SEEDED;
    return;
  }
  status[i] = VOX_ACCUMULATED;
  slots[i] = (int)s;
  if (inserted) codes[i] = 4;
  atomicAdd(&slot[W_COUNT], 1ull);
#pragma unroll
  for (int k = 0; k < 3; k++) atomicAdd(&slot[W_S1 + k], q[k]);
  atomicAdd(&slot[W_S2 + 0], q[0] * q[0]);
  atomicAdd(&slot[W_S2 + 1], q[0] * q[1]);
  atomicAdd(&slot[W_S2 + 2], q[0] * q[2]);
  atomicAdd(&slot[W_S2 + 3], q[1] * q[1]);
  atomicAdd(&slot[W_S2 + 4], q[1] * q[2]);
  atomicAdd(&slot[W_S2 + 5], q[2] * q[2]);
  if (a.colors) {
#pragma unroll
    for (int k = 0; k < 3; k++) atomicAdd(&slot[W_SC + k], voxel_colour(a.colors[3 * (size_t)i + k]));
  }
  // the smallest index of the call: the largest ~index in the low half of word 15 (little endian; n <= 2^22: never 0)
  atomicMax(reinterpret_cast<unsigned int*>(&slot[W_FIRST]), ~(unsigned int)i);
}

__global__ __launch_bounds__(WG_THREADS) void k_voxel_flag(const VoxelArgs a, const unsigned char* __restrict__ status,
                                                           const int* __restrict__ slots,
                                                           unsigned char* __restrict__ codes, int* __restrict__ totals,
                                                           const int nblocks) {
  __shared__ int sh[WG_WAVES][VOX_TOTALS];
  const int i = blockIdx.x * WG_THREADS + (int)threadIdx.x;
  const bool in = i < a.n;
  unsigned st = 255, code = 0;
  if (in) {
    st = status[i];
    code = codes[i];
    if (st == VOX_ACCUMULATED) {
      const u64* slot = a.table + (size_t)slots[i] * VOX_WORDS;
      if ((unsigned int)slot[W_FIRST] == ~(unsigned int)i) {
        code |= 1;
        if (slot[W_COUNT] >= (u64)a.min_points) code |= 2;
        codes[i] = (unsigned char)code;
      }
    }
  }
  int cnt[VOX_TOTALS];
  cnt[0] = __popcll(__ballot((code & 2) != 0));
#pragma unroll
  for (int k = 0; k < 4; k++) cnt[1 + k] = __popcll(__ballot(st == (unsigned)k));
  cnt[5] = __popcll(__ballot((code & 4) != 0));
  store_block_totals(cnt, sh, totals, nblocks);
}

// ONE workgroup.  totals[0][.] -> exclusive scan in place; counts6 = {accumulated, seeded, out, full, matured,
// live_before + new keys}.  nblocks == 0 writes {0, 0, 0, 0, 0, live_before}.
__global__ __launch_bounds__(WG_THREADS) void k_voxel_scan(int* __restrict__ totals, const int nblocks,
                                                           const int live_before, int* __restrict__ counts6) {
  __shared__ int sh[WG_WAVES];
  const int matured = scan_totals(totals, nblocks, sh);
  int c[VOX_TOTALS];
  c[0] = matured;
#pragma unroll
  for (int k = 1; k < VOX_TOTALS; k++) {
    int t = 0;
    for (int j = threadIdx.x; j < nblocks; j += WG_THREADS) t += totals[(size_t)k * nblocks + j];
    c[k] = block_sum(t, sh);
  }
  if (threadIdx.x == 0) {
    counts6[0] = c[1]; counts6[1] = c[2]; counts6[2] = c[3]; counts6[3] = c[4];
    counts6[4] = c[0];
    counts6[5] = live_before + c[5];
  }
}

// One rotation of the cyclic Jacobi method on the symmetric A (full storage), accumulating the axes in the columns of V.
__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&V)[3][3], const int p, const int q) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const int r = 3 - p - q;
  const double app = A[p][p], aqq = A[q][q], arp = A[r][p], arq = A[r][q];
  A[p][p] = app - t * apq;
  A[q][q] = aqq + t * apq;
  A[p][q] = A[q][p] = 0.0;
  A[r][p] = A[p][r] = c * arp - s * arq;
  A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double vp = V[k][p], vq = V[k][q];
    V[k][p] = c * vp - s * vq;
    V[k][q] = s * vp + c * vq;
  }
}

struct VoxelOut {
  float* xyz; float* covs; float* rgb; long long* keys; int* points; float* scaling; float* rotation; float* normal;
};

__global__ __launch_bounds__(WG_THREADS) void k_voxel_emit(const VoxelArgs a, const int* __restrict__ slots,
                                                           const unsigned char* __restrict__ codes,
                                                           const int* __restrict__ bases, const VoxelOut o) {
  __shared__ int sh[WG_WAVES];
  const int i = blockIdx.x * WG_THREADS + (int)threadIdx.x;
  const unsigned code = i < a.n ? codes[i] : 0u;
  const int rank = rank_in_block((code & 2) != 0, sh);
  if (!(code & 1)) return;
  u64* slot = a.table + (size_t)slots[i] * VOX_WORDS;
  slot[W_FIRST] = 0;   // this thread owns the slot for the rest of the call
  if (!(code & 2)) return;
  const size_t j = (size_t)(bases[blockIdx.x] + rank);
  const u64 key = slot[W_KEY], cnt = slot[W_COUNT];
  const double n = (double)cnt, Q = (double)VOX_Q;
  double m[3], mean[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double cell = (double)((long long)((key >> (42 - 21 * k)) & 0x1fffffull) - VOX_Q);
    m[k] = (double)slot[W_S1 + k] / n;
    mean[k] = (cell + (m[k] + 0.5) / Q) * a.g;
    o.xyz[3 * j + k] = (float)mean[k];
  }
  const double unit = a.g / Q, unit2 = unit * unit;
  double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  {
    int w = 0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = r; c < 3; c++, w++) A[r][c] = A[c][r] = ((double)slot[W_S2 + w] / n - m[r] * m[c]) * unit2;
  }
  for (int sweep = 0; sweep < VOX_JACOBI_SWEEPS; sweep++) {
    jacobi_rotate(A, V, 0, 1);
    jacobi_rotate(A, V, 0, 2);
    jacobi_rotate(A, V, 1, 2);
  }
  // descending eigenvalues (a three-element sorting network on the columns), then the clamp
  double lam[3] = {A[0][0], A[1][1], A[2][2]};
  auto order = [&](const int x, const int y) {
    if (lam[x] < lam[y]) {
      const double t = lam[x]; lam[x] = lam[y]; lam[y] = t;
#pragma unroll
      for (int k = 0; k < 3; k++) { const double u = V[k][x]; V[k][x] = V[k][y]; V[k][y] = u; }
    }
  };
  order(0, 1); order(1, 2); order(0, 1);
#pragma unroll
  for (int k = 0; k < 3; k++) lam[k] = lam[k] > a.min_var ? lam[k] : a.min_var;   // (a NaN becomes min_var)
  // right-handed axes: the third column follows the first two
  const double det = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                     V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
  if (det < 0.0) {
#pragma unroll
    for (int k = 0; k < 3; k++) V[k][2] = -V[k][2];
  }
  // Sigma = V diag(lam) V^T, symmetric by construction
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = r; c < 3; c++) {
      const float v = (float)((V[r][0] * lam[0]) * V[c][0] + (V[r][1] * lam[1]) * V[c][1] + (V[r][2] * lam[2]) * V[c][2]);
      o.covs[9 * j + 3 * r + c] = v;
      o.covs[9 * j + 3 * c + r] = v;
    }
  // the quaternion (w, x, y, z) of the rotation whose COLUMNS are the axes: Sigma = R S^2 R^T in the rasterizer's
  // convention (its matrix from a quaternion is this rotation's transpose, and it forms M^T M with M = S R^T)
  double qw, qx, qy, qz;
  const double tr = V[0][0] + V[1][1] + V[2][2];
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(tr + 1.0);
    qw = 0.25 * s; qx = (V[2][1] - V[1][2]) / s; qy = (V[0][2] - V[2][0]) / s; qz = (V[1][0] - V[0][1]) / s;
  } else if (V[0][0] > V[1][1] && V[0][0] > V[2][2]) {
    const double s = 2.0 * sqrt(1.0 + V[0][0] - V[1][1] - V[2][2]);
    qw = (V[2][1] - V[1][2]) / s; qx = 0.25 * s; qy = (V[0][1] + V[1][0]) / s; qz = (V[0][2] + V[2][0]) / s;
  } else if (V[1][1] > V[2][2]) {
    const double s = 2.0 * sqrt(1.0 + V[1][1] - V[0][0] - V[2][2]);
    qw = (V[0][2] - V[2][0]) / s; qx = (V[0][1] + V[1][0]) / s; qy = 0.25 * s; qz = (V[1][2] + V[2][1]) / s;
  } else {
    const double s = 2.0 * sqrt(1.0 + V[2][2] - V[0][0] - V[1][1]);
    qw = (V[1][0] - V[0][1]) / s; qx = (V[0][2] + V[2][0]) / s; qy = (V[1][2] + V[2][1]) / s; qz = 0.25 * s;
  }
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz), sg = qw < 0.0 ? -1.0 : 1.0;
  o.rotation[4 * j + 0] = (float)(sg * qw / qn);
  o.rotation[4 * j + 1] = (float)(sg * qx / qn);
  o.rotation[4 * j + 2] = (float)(sg * qy / qn);
  o.rotation[4 * j + 3] = (float)(sg * qz / qn);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    o.scaling[3 * j + k] = (float)log(sqrt(lam[k] * a.scale_factor));
    o.normal[3 * j + k] = (float)V[k][2];
  }
  if (o.rgb) {
#pragma unroll
    for (int k = 0; k < 3; k++) o.rgb[3 * j + k] = (float)((double)slot[W_SC + k] / (256.0 * n));
  }
  o.keys[j] = (long long)key;
  o.points[j] = (int)cnt;
  slot[W_CLOSED] = 1;
}

// thread = source slot: the whole record to the first free slot of its probe sequence in dst
__global__ __launch_bounds__(256) void k_voxel_rehash(const u64* __restrict__ src, const long long cap_src,
                                                      u64* __restrict__ dst, const long long cap_dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap_src) return;
  const u64* from = src + (size_t)i * VOX_WORDS;
  const u64 key = from[W_KEY];
  if (key == 0) return;
  const u64 mask = (u64)cap_dst - 1;
  u64 s = voxel_hash(key) & mask;
  for (long long step = 0; step < cap_dst; step++) {   // (bounded; the keys of one table are distinct)
    u64* to = dst + s * VOX_WORDS;
    if (atomicCAS(&to[W_KEY], 0ull, key) == 0) {
#pragma unroll
      for (int k = 1; k < VOX_WORDS; k++) to[k] = from[k];
      return;
    }
    s = (s + 1) & mask;
  }
}

static size_t voxel_workspace_bytes(int n) { return n > 0 ? VoxelWorkspace::carve(nullptr, n).bytes : 0; }

static bool voxel_capacity_ok(long long c) { return c >= 1 && c <= VOX_MAX_CAPACITY && (c & (c - 1)) == 0; }

static hipError_t launch_voxel_sweep(const VoxelArgs& a, unsigned char* status, long long* point_keys,
                                     const VoxelOut& o, int live_before, int* counts6, char* workspace, hipStream_t s) {
  ProfScope ps(K_VISIBILITY, s);
  if (a.n == 0) {
    hipLaunchKernelGGL(k_voxel_scan, dim3(1), dim3(WG_THREADS), 0, s, (int*)nullptr, 0, live_before, counts6);
    return hipGetLastError();
  }
  const int nblocks = (a.n + WG_THREADS - 1) / WG_THREADS;
  const VoxelWorkspace w = VoxelWorkspace::carve(workspace, a.n);
  hipLaunchKernelGGL(k_voxel_insert, dim3(nblocks), dim3(WG_THREADS), 0, s, a, status, point_keys, w.slots, w.codes);
  hipLaunchKernelGGL(k_voxel_flag, dim3(nblocks), dim3(WG_THREADS), 0, s, a, status, w.slots, w.codes, w.totals, nblocks);
  hipLaunchKernelGGL(k_voxel_scan, dim3(1), dim3(WG_THREADS), 0, s, w.totals, nblocks, live_before, counts6);
  hipLaunchKernelGGL(k_voxel_emit, dim3(nblocks), dim3(WG_THREADS), 0, s, a, w.slots, w.codes, w.totals, o);
  return hipGetLastError();
}

static bool positive_finite(float v) { return v > 0.f && v <= 3.402823466e38f; }   // (false for NaN and +inf)

}  // namespace gsr

using namespace gsr;

// ---- the entry points.  The order of the checks is part of the contract (include/gsraster.h).
extern "C" {

size_t gsr_voxel_table_bytes(long long capacity) {
  return voxel_capacity_ok(capacity) ? (size_t)capacity * VOX_WORDS * sizeof(u64) : 0;
}

size_t gsr_voxel_sweep_workspace(int n) { return n < 0 || n > VOX_MAX_N ? 0 : voxel_workspace_bytes(n); }

int gsr_voxel_sweep(int n, const float* points, const float* colors, float grid, int min_points, float min_sigma,
                    float scale_factor, long long* table, long long capacity, int live_before, unsigned char* status,
                    long long* point_keys, float* xyz_out, float* covs_out, float* rgb_out, long long* keys_out,
                    int* points_out, float* scaling_out, float* rotation_out, float* normal_out, int* counts6,
                    char* workspace, size_t workspace_bytes, void* stream_) {
  clear_error();
  if (n < 0 || n > VOX_MAX_N) return fail(GSR_ERR_INVALID_ARGUMENT, "bad n: 0 to 2^22 points per call");
  if (min_points < 1 || min_points > VOX_MAX_MIN_POINTS)
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad min_points: 1 to 2^20");
  if (!positive_finite(grid)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad grid: finite and > 0");
  if (!positive_finite(min_sigma)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad min_sigma: finite and > 0");
  if (!positive_finite(scale_factor)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad scale_factor: finite and > 0");
  if (!voxel_capacity_ok(capacity)) return fail(GSR_ERR_INVALID_ARGUMENT, "bad capacity: a power of two up to 2^26");
  if (live_before < 0 || live_before > capacity) return fail(GSR_ERR_INVALID_ARGUMENT, "bad live_before: 0 to capacity");
  if (!table || !counts6 ||
      (n > 0 && (!points || !status || !point_keys || !xyz_out || !covs_out || !keys_out || !points_out ||
                 !scaling_out || !rotation_out || !normal_out || (colors && !rgb_out))))
    return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_workspace(workspace_bytes, voxel_workspace_bytes(n))) return e;
  if (n > 0 && !workspace) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (int e = check_aligned4((uintptr_t)points | (uintptr_t)colors | (uintptr_t)xyz_out | (uintptr_t)covs_out |
                             (uintptr_t)rgb_out | (uintptr_t)points_out | (uintptr_t)scaling_out |
                             (uintptr_t)rotation_out | (uintptr_t)normal_out | (uintptr_t)counts6))
    return e;
  if (((uintptr_t)table | (uintptr_t)point_keys | (uintptr_t)keys_out) & 7u)
    return fail(GSR_ERR_INVALID_ARGUMENT, "misaligned pointer: the table and the key arrays need 8-byte alignment");
  VoxelArgs a;
  a.n = n; a.min_points = min_points;
  a.g = (double)grid;
  a.min_var = (double)min_sigma * (double)min_sigma;
  a.scale_factor = (double)scale_factor;
  a.points = points; a.colors = colors;
  a.table = reinterpret_cast<u64*>(table); a.capacity = capacity;
  VoxelOut o;
  o.xyz = xyz_out; o.covs = covs_out; o.rgb = colors ? rgb_out : nullptr; o.keys = keys_out; o.points = points_out;
  o.scaling = scaling_out; o.rotation = rotation_out; o.normal = normal_out;
  HIP_TRY(launch_voxel_sweep(a, status, point_keys, o, live_before, counts6, workspace, (hipStream_t)stream_));
  return GSR_OK;
}

int gsr_voxel_rehash(const long long* src, long long capacity_src, long long* dst, long long capacity_dst,
                     void* stream_) {
  clear_error();
  if (!voxel_capacity_ok(capacity_src) || !voxel_capacity_ok(capacity_dst))
    return fail(GSR_ERR_INVALID_ARGUMENT, "bad capacity: a power of two up to 2^26");
  if (capacity_dst < capacity_src) return fail(GSR_ERR_INVALID_ARGUMENT, "bad capacity: the destination is smaller");
  if (!src || !dst) return fail(GSR_ERR_INVALID_ARGUMENT, "null pointer");
  if (((uintptr_t)src | (uintptr_t)dst) & 7u)
    return fail(GSR_ERR_INVALID_ARGUMENT, "misaligned pointer: the table and the key arrays need 8-byte alignment");
  if (src == dst) return fail(GSR_ERR_INVALID_ARGUMENT, "source and destination are one table");
  hipStream_t s = (hipStream_t)stream_;
  ProfScope ps(K_VISIBILITY, s);
  hipLaunchKernelGGL(k_voxel_rehash, dim3((unsigned)((capacity_src + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const u64*>(src), capacity_src, reinterpret_cast<u64*>(dst), capacity_dst);
  HIP_TRY(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
