// Order statistics of SQL window frames for gfx950: for every row i (rows in window order) and each of m ranks
// k_t[i], the POSITION of the k_t[i]-th smallest counted row of its frame x[a[i] .. b[i]] in the total order (key,
// position) — or -1 when k_t[i] is negative or not below the frame's count of counted rows.  A row's key is one
// 64-bit order-key word that compares unsigned (ops/sort.column_order_key); a row is counted when its validity
// byte is non-zero.  The window evaluator (engine/windowfn.py) gathers the values at those positions and finishes
// percentile / median / percentile_approx; returning positions keeps these kernels free of value types, and ties
// are deterministic: the earlier row wins.
//
// Two entry points, both one thread per row with a grid-stride loop, each ONE launch for all rows and ranks:
//   * dxa_frame_select_direct — short frames.  For every counted candidate j of the frame, count the frame's
//     counted rows that precede it in (key, position) order; a candidate whose count equals k_t is answer t, so one
//     sweep answers all m ranks.  O(len^2) loads, which neighbouring rows serve from cache.
//   * dxa_frame_select_tree — any frame length: a range k-th query on a wavelet matrix over the rows' global ranks.
//     r[i] is row i's position in one stable sort by (not counted, key); level l (most significant of L =
//     bit_length(n - 1) bits first) stores Z_l[0 .. n], the inclusive prefix count of zero bits in the level's
//     ordering (Z_l[0] = 0, Z_l[n] = z_l, the level's zero total), and each level orders the rows by a stable
//     partition on its bit, zeros first.  The query for [lo, hi1) and rank k runs per level: with c0 = Z[hi1] -
//     Z[lo], k < c0 goes left (lo = Z[lo], hi1 = Z[hi1], bit 0), else right (k -= c0, lo = z + lo - Z[lo], hi1 = z +
//     hi1 - Z[hi1], bit 1).  The L bits are a global rank, and the sort permutation turns it into a row position.
//     Rows that are not counted hold the largest global ranks, so a rank below the frame's count never reaches one;
//     the count itself comes from a prefix count of the validity bytes.  Frames never cross a partition, so the
//     global structure needs no partition case.
//   dxa_wavelet_level is the build step of that matrix: the stable scatter of one level into the next level's
//   ordering, fused with the next level's zero-bit flags (the prefix count between two levels is the caller's).
//
// Every index is clamped or checked before its load: frames are clipped to [0, n), a > b writes -1, the tree walk's
// bounds are clamped to [0, n] and its final rank to n - 1, scatter destinations outside [0, n) are dropped.  No
// atomics, no LDS, no inter-workgroup traffic: a thread writes its own row's words only (the scatter: its own
// element's destination, a permutation when Z is a prefix count).
#include "dxa_common.h"

namespace {

constexpr int kMaxRanks = 16;

// The frame of row i clipped to [0, n): first row and one past the last (lo == hi1: empty).
__device__ __forceinline__ void frame_of(const int64_t* a, const int64_t* b, int64_t n, int64_t i, int64_t& lo,
                                         int64_t& hi1) {
  int64_t l = a[i], h = b[i];
  lo = 0;
  hi1 = 0;
  if (l > h) return;
  if (l < 0) l = 0;
  if (h > n - 1) h = n - 1;
  if (l > h) return;
  lo = l;
  hi1 = h + 1;
}

// A rank as an int32 that matches no count when it is out of range (n < 2^31, so every count fits).
__device__ __forceinline__ int32_t rank_of(const int64_t* ranks, int64_t n, int t, int64_t i) {
  const int64_t k = ranks[(int64_t)t * n + i];
  return (k < 0 || k > 0x7fffffff) ? -1 : (int32_t)k;
}

__global__ __launch_bounds__(256) void select_direct_kernel(const uint64_t* __restrict__ key,
                                                            const uint8_t* __restrict__ valid,
                                                            const int64_t* __restrict__ a,
                                                            const int64_t* __restrict__ b, int64_t n,
                                                            const int64_t* __restrict__ ranks, int m,
                                                            int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo, hi1;
    frame_of(a, b, n, i, lo, hi1);
    // constant indices after unrolling: both arrays stay in registers
    int32_t want[kMaxRanks];
    int32_t found[kMaxRanks];                           // positions fit: n < 2^31
#pragma unroll
    for (int t = 0; t < kMaxRanks; ++t) {
      want[t] = t < m ? rank_of(ranks, n, t, i) : -1;
      found[t] = -1;
    }
    for (int64_t j = lo; j < hi1; ++j) {
      if (valid != nullptr && valid[j] == 0) continue;
      const uint64_t kj = key[j];
      int32_t before = 0;
      for (int64_t q = lo; q < hi1; ++q) {
        const uint64_t kq = key[q];
        const bool counted = valid == nullptr || valid[q] != 0;
        before += (counted && (kq < kj || (kq == kj && q < j))) ? 1 : 0;
      }
#pragma unroll
      for (int t = 0; t < kMaxRanks; ++t)
        if (want[t] == before) found[t] = (int32_t)j;
    }
#pragma unroll
    for (int t = 0; t < kMaxRanks; ++t)
      if (t < m) out[(int64_t)t * n + i] = (int64_t)found[t];
  }
}

__device__ __forceinline__ int64_t clamp_index(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void select_tree_kernel(const int32_t* __restrict__ Z,
                                                          const int64_t* __restrict__ perm,
                                                          const int64_t* __restrict__ vcum,
                                                          const int64_t* __restrict__ a,
                                                          const int64_t* __restrict__ b, int64_t n, int levels,
                                                          const int64_t* __restrict__ ranks, int m,
                                                          int64_t* __restrict__ out) {
  const int64_t stride = n + 1;                         // one level of Z
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo, hi1;
    frame_of(a, b, n, i, lo, hi1);
    const int64_t count = vcum[hi1] - vcum[lo];         // 0 <= lo <= hi1 <= n; vcum has n + 1 entries
    for (int t = 0; t < m; ++t) {
      int64_t k = ranks[(int64_t)t * n + i];
      int64_t pos = -1;
      if (k >= 0 && k < count) {
        int64_t l = lo, h = hi1, rank = 0;
        for (int lev = 0; lev < levels; ++lev) {
          const int32_t* z = Z + (int64_t)lev * stride;
          const int64_t zl = z[l], zh = z[h], zt = z[n];
          const int64_t c0 = zh - zl;
          if (k < c0) {
            l = zl;
            h = zh;
            rank <<= 1;
          } else {
            k -= c0;
            l = zt + l - zl;
            h = zt + h - zh;
            rank = (rank << 1) | 1;
          }
          l = clamp_index(l, n);
          h = clamp_index(h, n);
        }
        pos = perm[clamp_index(rank, n - 1)];
      }
      out[(int64_t)t * n + i] = pos;
    }
  }
}

// cur: the global ranks in this level's ordering; Zl: this level's inclusive prefix count of zero bits (n + 1
// entries).  Element i goes to Zl[i] when its bit is 0, to z + i - Zl[i] when it is 1 (a stable partition), and the
// zero flag of its next lower bit is written beside it for the next level's prefix count.
__global__ __launch_bounds__(256) void wavelet_level_kernel(const int32_t* __restrict__ cur,
                                                            const int32_t* __restrict__ Zl, int64_t n, int bit,
                                                            int32_t* __restrict__ nxt,
                                                            int32_t* __restrict__ next_flags) {
  const int64_t zt = Zl[n];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = cur[i];
    const int64_t zi = Zl[i];
    const int64_t dst = ((v >> bit) & 1) ? zt + i - zi : zi;
    if (dst < 0 || dst >= n) continue;                  // not a prefix count: drop, never write outside
    nxt[dst] = v;
    next_flags[dst] = ((v >> (bit - 1)) & 1) ^ 1;
  }
}

inline int levels_of(int64_t n) {                       // bit_length(n - 1)
  int levels = 0;
  while (levels < 31 && ((int64_t)1 << levels) < n) ++levels;
  return levels;
}

}  // namespace

// key, a, b: n entries; valid: n bytes or null (every row counted); ranks, out: m * n int64, rank t of row i at
// [t * n + i].
DXA_API int dxa_frame_select_direct(const uint64_t* key, const uint8_t* valid, const int64_t* a, const int64_t* b,
                                    int64_t n, const int64_t* ranks, int32_t m, int64_t* out, void* st) {
  if (n < 0 || n >= ((int64_t)1 << 31) || m < 1 || m > kMaxRanks) return (int)hipErrorInvalidValue;
  if (key == nullptr || a == nullptr || b == nullptr || ranks == nullptr || out == nullptr)
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(select_direct_kernel, dim3(dxa_blocks(n, 256)), dim3(256), 0, (hipStream_t)st, key, valid, a, b,
                     n, ranks, (int)m, out);
  return (int)hipGetLastError();
}

// Z: levels * (n + 1) int32 (unused when levels == 0, i.e. n == 1); perm: the sort permutation, n entries; vcum:
// n + 1 int64, vcum[j] = counted rows among the first j; levels must be bit_length(n - 1).
DXA_API int dxa_frame_select_tree(const int32_t* Z, const int64_t* perm, const int64_t* vcum, const int64_t* a,
                                  const int64_t* b, int64_t n, int32_t levels, const int64_t* ranks, int32_t m,
                                  int64_t* out, void* st) {
  if (n < 0 || n >= ((int64_t)1 << 31) || m < 1 || m > kMaxRanks) return (int)hipErrorInvalidValue;
  if (perm == nullptr || vcum == nullptr || a == nullptr || b == nullptr || ranks == nullptr || out == nullptr)
    return (int)hipErrorInvalidValue;
  if (n == 0) return levels == 0 ? 0 : (int)hipErrorInvalidValue;
  if (levels != levels_of(n) || (levels > 0 && Z == nullptr)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(select_tree_kernel, dim3(dxa_blocks(n, 256)), dim3(256), 0, (hipStream_t)st, Z, perm, vcum, a,
                     b, n, (int)levels, ranks, (int)m, out);
  return (int)hipGetLastError();
}

// One build step: bit is the level's bit (1 <= bit < 31; the last level, bit 0, has no next ordering).
DXA_API int dxa_wavelet_level(const int32_t* cur, const int32_t* Zl, int64_t n, int32_t bit, int32_t* nxt,
                              int32_t* next_flags, void* st) {
  if (n < 0 || n >= ((int64_t)1 << 31) || bit < 1 || bit > 30) return (int)hipErrorInvalidValue;
  if (cur == nullptr || Zl == nullptr || nxt == nullptr || next_flags == nullptr) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(wavelet_level_kernel, dim3(dxa_blocks(n, 256)), dim3(256), 0, (hipStream_t)st, cur, Zl, n,
                     (int)bit, nxt, next_flags);
  return (int)hipGetLastError();
}
