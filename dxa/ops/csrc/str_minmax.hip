// MIN / MAX over a string column per group, for gfx950: the index of a row holding each group's extreme string.
//
// Order: unsigned byte order of the UTF-8 bytes, a proper prefix before the longer string (ops/sort.string_ranks'
// order, and Python's on valid UTF-8).  NULL rows, rows a keep mask drops and rows whose id is outside [0, ngroups)
// are skipped; a group without a row keeps -1.  Among equal strings the smallest row index wins, so the candidates
// of a group are totally ordered — by (string, then the smaller index) — and the result does not depend on the
// order the rows arrive in.
//
// One pass, compare-and-CAS on a per-group "best row" word, chosen over rounds of 8-byte prefix words refined by a
// 64-bit max (the way win_dec_kernel refines a two-word key): the rounds form needs one sweep over the rows per 8
// bytes of the longest string — unbounded here, strings may have any length — and a rule for what to do past the
// bound, while this form reads a row's bytes only as far as its first difference from the current best and has no
// bound at all.  A lane loads the group's best row index, compares its own string with that row's 8 bytes per step
// (dxa::load_le, byte-swapped so that an integer compare is the byte order) and, when it is better, installs its
// index with a 64-bit compare-and-swap; a lost CAS hands back the new best and the lane compares again.  The best
// only ever improves in the total order above, so a lane stops as soon as it no longer beats it, every failed CAS
// is another lane's success (lock-free: no lane waits on a flag or on another lane), and the word ends at the
// order's maximum whatever the interleaving.
//
// A statement with a handful of groups would put every row of a workgroup on a handful of global words, so ids below
// kLdsGroups go through an LDS best-row array (64-bit LDS CAS) that each workgroup flushes with the same
// compare-and-CAS, one global attempt per touched group; ids at or above the bound go straight to global memory,
// which such a grouping spreads over many words.  The worst case for the chain is one group whose rows arrive in
// ascending order under MAX: every row of a wave beats the best it read, one CAS wins and the others compare again.
#include "dxa_common.h"

namespace {

constexpr int kLdsGroups = dxa::kLdsGroupIds;    // the bound of window_ring.hip's second passes too

struct StrRows {
  const uint8_t* arena;
  const int64_t* starts;
  const int32_t* lens;
};

// byte order of row a's string against row b's: < 0, 0, > 0
__device__ __forceinline__ int str_compare(const StrRows& c, int64_t a, int64_t b) {
  int32_t la = c.lens[a], lb = c.lens[b];
  la = la < 0 ? 0 : la;
  lb = lb < 0 ? 0 : lb;
  const int32_t m = la < lb ? la : lb;
  const uint8_t* x = c.arena + c.starts[a];
  const uint8_t* y = c.arena + c.starts[b];
  for (int32_t q = 0; q < m; q += 8) {
    const int nb = m - q < 8 ? m - q : 8;
    const uint64_t xw = dxa::load_le(x + q, nb), yw = dxa::load_le(y + q, nb);
    if (xw != yw) return __builtin_bswap64(xw) < __builtin_bswap64(yw) ? -1 : 1;
  }
  return la < lb ? -1 : la > lb ? 1 : 0;
}

// row a replaces row b as the group's best: a greater (MAX) or smaller (MIN) string, or the same at a smaller index
__device__ __forceinline__ bool str_beats(const StrRows& c, int64_t a, int64_t b, bool mx) {
  const int cmp = str_compare(c, a, b);
  if (cmp == 0) return a < b;
  return mx ? cmp > 0 : cmp < 0;
}

// install row i in ``slot`` (an LDS or a global word; -1: no row yet) unless the row it holds is at least as good
__device__ __forceinline__ void str_install(unsigned long long* slot, int64_t i, const StrRows& c, bool mx) {
  long long cur = (long long)*(volatile unsigned long long*)slot;
  while (cur < 0 || str_beats(c, i, cur, mx)) {
    const long long prev = (long long)atomicCAS(slot, (unsigned long long)cur, (unsigned long long)i);
    if (prev == cur) break;
    cur = prev;
  }
}

__global__ __launch_bounds__(256) void str_argext_kernel(const int32_t* __restrict__ gid, int64_t n, int32_t ngroups,
                                                         const StrRows c, const uint8_t* __restrict__ valid,
                                                         const uint8_t* __restrict__ keep, int32_t mx,
                                                         unsigned long long* __restrict__ best) {
  __shared__ unsigned long long part[kLdsGroups];
  const int32_t lds_groups = ngroups < kLdsGroups ? ngroups : kLdsGroups;
  for (int g = threadIdx.x; g < kLdsGroups; g += blockDim.x) part[g] = ~0ull;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if ((keep && !keep[i]) || (valid && !valid[i])) continue;
    const int32_t g = gid[i];
    if (g < 0 || g >= ngroups) continue;
    str_install(g < kLdsGroups ? &part[g] : best + g, i, c, mx != 0);
  }
  __syncthreads();
  for (int g = threadIdx.x; g < lds_groups; g += blockDim.x) {
    const long long i = (long long)part[g];
    if (i >= 0) str_install(best + g, i, c, mx != 0);
  }
}

}  // namespace

// best[g] = a row of group g holding its greatest (dir 1) or smallest (dir 0) non-NULL string, the smallest index
// among equals, or -1; ``valid`` and ``keep`` may be null.  ``best`` [ngroups] is initialised here.
DXA_API int dxa_str_argext(const int32_t* gid, int64_t n, int32_t ngroups, const uint8_t* arena, const int64_t* starts,
                           const int32_t* lens, const uint8_t* valid, const uint8_t* keep, int32_t dir, int64_t* best,
                           void* st) {
  hipStream_t s = (hipStream_t)st;
  if (ngroups < 0 || (dir != 0 && dir != 1) || !best) return (int)hipErrorInvalidValue;
  if (ngroups == 0) return 0;
  hipMemsetAsync(best, 0xFF, (size_t)ngroups * 8, s);
  if (n <= 0) return (int)hipGetLastError();
  if (!gid || !starts || !lens) return (int)hipErrorInvalidValue;
  const StrRows c{arena, starts, lens};
  // 8 rows per lane amortise a workgroup's LDS clear and flush, as the ring's second-pass kernels do
  hipLaunchKernelGGL(str_argext_kernel, dim3(dxa_blocks((n + 7) / 8, 256, 512)), dim3(256), 0, s, gid, n, ngroups, c,
                     valid, keep, dir, (unsigned long long*)best);
  return (int)hipGetLastError();
}
