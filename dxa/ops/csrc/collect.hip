// collect_list / collect_set for gfx950: the slot matrices of an array column, for GROUP BY and for SQL window frames.
//
// An array column (engine/column.py ArrayColumn) keeps K element slots per row, slot-major: slot k of every row is
// one contiguous run, so a [K, rows] matrix is K element columns without a copy.  Both entry points fill such
// matrices in ONE launch each; neither moves a string byte (a string slot is its starts / lens words over the
// argument's own arena) and neither knows a value type: GROUP BY's equality has already been applied by the caller.
//
//   * dxa_collect_scatter (GROUP BY).  The caller has the counted rows in (group id, input position) order — one
//     stable radix argsort — and every group's start and count among them.  One thread per slot (k, g), consecutive
//     lanes on consecutive groups of one slot: where k < count[g] it reads the row number rows[start[g] + k] once and
//     moves that row's word of every leaf (up to kMaxLeaves: data, decimal lanes, string starts / lens; 1, 2, 4 or 8
//     bytes) to out_leaf[k * ngroups + g]; elsewhere it writes 0.  The same thread writes valid[k * ngroups + g] and,
//     reading its index the other way round (g' = t / K, k' = t % K), present[g' * K + k'], so every store of the
//     launch is coalesced and no matrix needs a memset or an int64 index temporary.
//   * dxa_frame_collect (window frames).  out[s * n + i] is the sorted-order position of the s-th kept row of row
//     i's frame [a[i], b[i]], -1 from the frame's kept count on: row j is kept when counted[j] and, for the set
//     (p != NULL, windowfn._prev_occurrence), when p[j] < a[i] — the value's first occurrence inside the frame.
//     One thread per row, so consecutive lanes write consecutive columns of one slot row.  A wave-per-row shape
//     (lanes on 64 consecutive j, a ballot as the keep mask, the popcount of the lanes below as the slot) was
//     measured beside it and left out: its stores go to 64 different rows of the matrix, and it took about three
//     times as long at frames of 8, 64 and 256 rows (profiles/collect/README.md).
//
// Every index is clamped or checked before its load or store: frames are clipped to [0, n) as in
// window_distinct.hip, a slot at or past K is never written (K is the caller's maximum, so none occurs), a row number
// outside [0, nrows) moves zero.  No atomics, no LDS, no inter-workgroup traffic.
#include "dxa_common.h"

namespace {

constexpr int kMaxLeaves = 8;

struct CollectLeaf {
  const void* src;       // nrows words
  void* dst;             // K * ngroups words, slot-major
  int32_t elem;          // 1, 2, 4 or 8 bytes
  int32_t pad;
};

struct CollectArgs {
  CollectLeaf leaf[kMaxLeaves];
  int32_t nleaves;
  uint32_t K;
  uint32_t ngroups;
  int64_t nrows;                // rows of every leaf
  int64_t m;                    // counted rows
  const int64_t* rows;          // m: the counted rows in (group, input position) order
  const int64_t* start;         // ngroups: a group's first entry of rows
  const int64_t* count;         // ngroups: its number of entries
  uint8_t* valid;               // K * ngroups, slot-major (may be NULL)
  uint8_t* present;             // ngroups * K, row-major (may be NULL)
};

template <typename T>
__device__ __forceinline__ void move_word(const CollectLeaf& c, uint32_t t, int64_t r, bool ok) {
  reinterpret_cast<T*>(c.dst)[t] = ok ? reinterpret_cast<const T*>(c.src)[r] : T(0);
}

__global__ __launch_bounds__(256) void collect_scatter_kernel(const CollectArgs a) {
  const uint32_t total = a.K * a.ngroups;                // < 2^31, checked by the entry point
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const uint32_t k = t / a.ngroups, g = t - k * a.ngroups;
    bool ok = (int64_t)k < a.count[g];
    int64_t r = 0;
    if (ok) {
      const int64_t at = a.start[g] + (int64_t)k;
      ok = at >= 0 && at < a.m;
      if (ok) {
        r = a.rows[at];
        ok = r >= 0 && r < a.nrows;
        if (!ok) r = 0;
      }
    }
    for (int c = 0; c < a.nleaves; ++c) {
      const CollectLeaf& leaf = a.leaf[c];
      switch (leaf.elem) {
        case 8: move_word<uint64_t>(leaf, t, r, ok); break;
        case 4: move_word<uint32_t>(leaf, t, r, ok); break;
        case 2: move_word<uint16_t>(leaf, t, r, ok); break;
        default: move_word<uint8_t>(leaf, t, r, ok); break;
      }
    }
    if (a.valid != nullptr) a.valid[t] = ok ? 1 : 0;
    if (a.present != nullptr) {
      const uint32_t g2 = t / a.K, k2 = t - g2 * a.K;    // the same index space read group-major
      a.present[t] = (int64_t)k2 < a.count[g2] ? 1 : 0;
    }
  }
}

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

__device__ __forceinline__ bool kept(const uint8_t* counted, const int32_t* p, int64_t j, int32_t first) {
  return counted[j] != 0 && (p == nullptr || p[j] < first);
}

__global__ __launch_bounds__(256) void frame_collect_kernel(const int64_t* __restrict__ a,
                                                            const int64_t* __restrict__ b,
                                                            const uint8_t* __restrict__ counted,
                                                            const int32_t* __restrict__ p, int64_t n, int64_t K,
                                                            int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo, hi1;
    frame_of(a, b, n, i, lo, hi1);
    const int32_t first = (int32_t)lo;                  // lo < n < 2^31
    int64_t s = 0;
    for (int64_t j = lo; j < hi1 && s < K; ++j) {
      if (kept(counted, p, j, first)) {
        out[s * n + i] = j;
        ++s;
      }
    }
    for (; s < K; ++s) out[s * n + i] = -1;
  }
}

}  // namespace

// rows: m int64 row numbers in (group, input position) order; start, count: ngroups int64; srcs / dsts / elems:
// nleaves entries, every src nrows words of elems[c] bytes, every dst K * ngroups such words; valid: K * ngroups
// bytes or NULL; present: ngroups * K bytes or NULL.
DXA_API int dxa_collect_scatter(const int64_t* rows, int64_t m, const int64_t* start, const int64_t* count,
                                int64_t ngroups, int64_t K, const void* const* srcs, void* const* dsts,
                                const int32_t* elems, int32_t nleaves, int64_t nrows, uint8_t* valid,
                                uint8_t* present, void* st) {
  if (ngroups < 0 || K < 0 || m < 0 || nrows < 0 || nleaves < 0 || nleaves > kMaxLeaves)
    return (int)hipErrorInvalidValue;
  if (ngroups == 0 || K == 0) return 0;
  if (K >= ((int64_t)1 << 31) || ngroups >= ((int64_t)1 << 31) || K * ngroups >= ((int64_t)1 << 31))
    return (int)hipErrorInvalidValue;
  if (start == nullptr || count == nullptr || (m > 0 && rows == nullptr)) return (int)hipErrorInvalidValue;
  CollectArgs a{};
  for (int c = 0; c < nleaves; ++c) {
    if (elems[c] != 1 && elems[c] != 2 && elems[c] != 4 && elems[c] != 8) return (int)hipErrorInvalidValue;
    if (srcs[c] == nullptr || dsts[c] == nullptr) return (int)hipErrorInvalidValue;
    a.leaf[c] = CollectLeaf{srcs[c], dsts[c], elems[c], 0};
  }
  a.nleaves = nleaves;
  a.K = (uint32_t)K;
  a.ngroups = (uint32_t)ngroups;
  a.nrows = nrows;
  a.m = m;
  a.rows = rows;
  a.start = start;
  a.count = count;
  a.valid = valid;
  a.present = present;
  hipLaunchKernelGGL(collect_scatter_kernel, dim3(dxa_blocks(K * ngroups, 256)), dim3(256), 0, (hipStream_t)st, a);
  return (int)hipGetLastError();
}

// a, b: n int64 frame bounds; counted: n bytes; p: n int32 (previous occurrence, -1, or a sentinel >= n) or NULL for
// the list; out: K * n int64, slot-major.
DXA_API int dxa_frame_collect(const int64_t* a, const int64_t* b, const uint8_t* counted, const int32_t* p,
                              int64_t n, int64_t K, int64_t* out, void* st) {
  if (n < 0 || n >= ((int64_t)1 << 31) || K < 0) return (int)hipErrorInvalidValue;
  if (n == 0 || K == 0) return 0;
  if (a == nullptr || b == nullptr || counted == nullptr || out == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(frame_collect_kernel, dim3(dxa_blocks(n, 256)), dim3(256), 0, (hipStream_t)st, a, b,
                     counted, p, n, K, out);
  return (int)hipGetLastError();
}
