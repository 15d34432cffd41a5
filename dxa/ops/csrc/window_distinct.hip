// Distinct counts of SQL window frames for gfx950: for every row i (rows in window order), the number of different
// counted values in its frame x[a[i] .. b[i]].  The window evaluator (engine/windowfn.py) reduces the question to one
// int array p over the rows: p[j] is the position of the previous counted row with the same value, -1 for a value's
// first counted occurrence, and a sentinel >= n for a row that is not counted.  A value of the frame [lo, hi1) is
// then counted once — at its first row inside the frame, the one row of the value whose previous occurrence lies
// before lo — so the answer is #{ j in [lo, hi1) : p[j] < lo }.  Frames never cross a partition, and a previous
// occurrence in another partition lies before lo, so there is no partition case; value types never reach these
// kernels.
//
// Two entry points, both one thread per row with a grid-stride loop, each ONE launch for all rows:
//   * dxa_frame_distinct_direct — short frames.  Scan p[lo .. hi1) and count the entries below lo: O(len) loads per
//     row, which neighbouring rows (whose frames overlap) serve from cache.
//   * dxa_frame_distinct_tree — any frame length: a range count-below-threshold query on the wavelet matrix of
//     window_select.hip (same Z layout, built by dxa_wavelet_level) over the rows' global ranks in (not counted, p,
//     position) order.  With T[i] the number of counted rows of the whole array with p < lo[i], the rows with
//     p < lo are exactly the global ranks below T[i], so the answer is the number of the frame's rows with rank <
//     T[i].  The walk for [l, h) runs per level (most significant of L = bit_length(n - 1) bits first) with c0 =
//     Z[h] - Z[l] zeros in the range: where T's bit is 1 every zero-bit rank of the range is below T — add c0 and go
//     right (l = z + l - Z[l], h = z + h - Z[h]); where it is 0 go left (l = Z[l], h = Z[h]).  T can be 2^L (n a
//     power of two, every row a counted first occurrence): no rank reaches it, the answer is hi1 - lo and no level is
//     read.
//
// Every index is clamped or checked before its load: frames are clipped to [0, n) as in window_select.hip, a > b
// writes 0, the walk's bounds are clamped to [0, n], a negative T counts nothing.  No atomics, no LDS, no
// inter-workgroup traffic: a thread writes its own row's word only.
#include "dxa_common.h"

namespace {

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

__global__ __launch_bounds__(256) void distinct_direct_kernel(const int32_t* __restrict__ p,
                                                              const int64_t* __restrict__ a,
                                                              const int64_t* __restrict__ b, int64_t n,
                                                              int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo, hi1;
    frame_of(a, b, n, i, lo, hi1);
    const int32_t first = (int32_t)lo;                  // lo < n < 2^31
    int32_t count = 0;
    for (int64_t j = lo; j < hi1; ++j) count += p[j] < first ? 1 : 0;
    out[i] = (int64_t)count;
  }
}

__device__ __forceinline__ int64_t clamp_index(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void distinct_tree_kernel(const int32_t* __restrict__ Z,
                                                            const int64_t* __restrict__ T,
                                                            const int64_t* __restrict__ a,
                                                            const int64_t* __restrict__ b, int64_t n, int levels,
                                                            int64_t* __restrict__ out) {
  const int64_t stride = n + 1;                         // one level of Z
  const int64_t top = (int64_t)1 << levels;             // no rank reaches it
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo, hi1;
    frame_of(a, b, n, i, lo, hi1);
    const int64_t t = T[i];
    int64_t count = 0;
    if (t >= top) {
      count = hi1 - lo;
    } else if (t > 0 && lo < hi1) {
      int64_t l = lo, h = hi1;
      for (int lev = 0; lev < levels; ++lev) {
        const int32_t* z = Z + (int64_t)lev * stride;
        const int64_t zl = z[l], zh = z[h];
        if ((t >> (levels - 1 - lev)) & 1) {
          const int64_t zt = z[n];
          count += zh - zl;
          l = zt + l - zl;
          h = zt + h - zh;
        } else {
          l = zl;
          h = zh;
        }
        l = clamp_index(l, n);
        h = clamp_index(h, n);
      }
    }
    out[i] = count;
  }
}

inline int levels_of(int64_t n) {                       // bit_length(n - 1)
  int levels = 0;
  while (levels < 31 && ((int64_t)1 << levels) < n) ++levels;
  return levels;
}

}  // namespace

// p: n int32 (previous occurrence, -1, or a sentinel >= n); a, b, out: n int64.
DXA_API int dxa_frame_distinct_direct(const int32_t* p, const int64_t* a, const int64_t* b, int64_t n, int64_t* out,
                                      void* st) {
  if (n < 0 || n >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  if (p == nullptr || a == nullptr || b == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(distinct_direct_kernel, dim3(dxa_blocks(n, 256)), dim3(256), 0, (hipStream_t)st, p, a, b, n,
                     out);
  return (int)hipGetLastError();
}

// Z: levels * (n + 1) int32 (unused when levels == 0, i.e. n == 1); T: n int64, the global count of counted rows
// with p < lo[i]; a, b, out: n int64; levels must be bit_length(n - 1).
DXA_API int dxa_frame_distinct_tree(const int32_t* Z, const int64_t* T, const int64_t* a, const int64_t* b,
                                    int64_t n, int32_t levels, int64_t* out, void* st) {
  if (n < 0 || n >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  if (T == nullptr || a == nullptr || b == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (levels != levels_of(n) || (levels > 0 && Z == nullptr)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(distinct_tree_kernel, dim3(dxa_blocks(n, 256)), dim3(256), 0, (hipStream_t)st, Z, T, a, b, n,
                     (int)levels, out);
  return (int)hipGetLastError();
}
