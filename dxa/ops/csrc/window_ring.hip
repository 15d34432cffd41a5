// Dense sliding-window aggregation for gfx950: a persistent group dictionary + a ring of per-pane accumulator rows,
// resident in HBM across micro-batches (SURVEY §2.F K16 "window ring buffer + slicing kernels", the reference's
// past-RDD union + GROUP BY at CommonProcessorFactory.scala:156-236).
//
// A GROUP BY over a 5-minute / 1-second sliding window is answered per batch by
//   1. win_insert  — the entering pane's rows hash their key and look it up in the PERSISTENT open-addressed
//                    dictionary (the table, the slot → group-id map and the group counter survive from batch to
//                    batch); a new key draws the next dense group id and its claiming lane copies the key values into
//                    fixed-width dictionary columns (strings up to kKeyWidth bytes) before publishing the id, so
//                    output keys never point into a pane that will be evicted; every other row compares its key with
//                    the entry (64-bit hash collisions and over-long strings are reported, never merged: the host then
//                    answers the batch the generic way); filtered rows (WHERE) go to the dump row ``gcap``;
//   2. the fused multi-aggregate (hash_groupby.hip agg_multi) accumulates the pane into its ring slot's
//      [group][stride] rows (complete blocks of panes are pre-combined into block slots once);
//   3. win_combine — the window's ring / block slots are combined per (group, word) in one pass (sum / f64 sum / max
//                    — the accumulator kinds of agg_multi), only for the groups the dictionary holds;
//   4. win_keep + win_compact — groups with rows in the window are flagged, counted into the batch's one host read
//                    and listed in group order;
//   5. win_emit    — every kept group's key columns and finished aggregates are written by output position, so the
//                    host only slices the outputs after its read.
// When the dictionary fills (the group counter passes the capacity) it is rebuilt instead of abandoned: win_live
// finds the groups that still have rows in the panes the ring holds, win_remap_dict / win_remap_slot renumber them
// densely in the key columns and in every held pane slot, win_rehash refills the cleared table (dxa_win_live …
// dxa_win_rehash below; the policy is the host's, dxa/engine/window_dense.py DenseWindow.rebuild).
// COUNT(DISTINCT x) rides on the same ring: a pair dictionary keyed by (group id, x) and one presence byte per ring
// slot and pair (win_pair_mark), ORed over the window and added into the combined rows between steps 3 and 4
// (win_distinct_fold) — see the section before the entry points.  The rest of the DISTINCT family is answered from the
// same state: the pair dictionary holds every live pair's x, so SUM / AVG(DISTINCT x) are one more instantiation of
// the fold, which also adds the live pairs' values into sum words of the combined row (reduced in the wave, one atomic
// per parent, word and wave); count(DISTINCT a, b, …) is the count fold over a dictionary keyed by (group id, a, b, …)
// — the same insert kernel with more key columns; approx_count_distinct is the exact distinct count.
// The variance family (M2) and skewness / kurtosis / corr / covar (M3, M4, Cxy) keep centred sums per pane and group:
// second passes over the pane fill them (win_m2_kernel, win_mom_kernel) and win_combine merges slots by the multi-way
// form of Chan's update.
// Decimal arguments stay exact: SUM / AVG keep three 32-bit limb sums per pane and group as ordinary MA_ADD_U64 words
// (win_dec_kernel fills them from the decimal column in place, win_emit_kernel reassembles the 128-bit total and, for
// AVG, divides it exactly with HALF_UP rounding); MIN / MAX of a two-lane decimal keep a two-word order key, the hi
// word an ordinary MA_MAX word and the lo word in a line of the combine op MA_LOKEY (described by ``lodesc``).
// Every layout goes through the same two host entry points, dxa_win_answer (steps 3-5) and dxa_win_combine_block; the
// descriptors a layout passes (none, m2desc, m2desc + momdesc; with or without lodesc; with or without pickdesc; with
// or without strdesc) pick
// the win_combine_kernel instantiation.
// first / last / max_by / min_by keep a row pick per pane and group (a rank word, the picked row's value and its
// validity; win_pick_kernel and win_pick_gather_kernel fill them) and slots combine by their place in the window.
// MIN / MAX over a string argument keep the winning value's order key — a whole line of 8 words — per pane and group
// (dxa_win_strkey: str_minmax.hip's arg-extreme kernel, then win_strkey_gather_kernel) and slots combine by the
// greatest key tuple (``strdesc``).
// So a batch costs one pane's aggregation plus a (groups × window panes) combine of L2/HBM-resident rows, instead of
// re-grouping ~40 partial tables (the previous paned path), and one synchronising read instead of three.
#include "dxa_common.h"

namespace {

constexpr int kMaxKeyCols = 16;
constexpr int kKeyWidth = 48;            // bytes of a string key kept in the dictionary
enum : int32_t { KC_I64 = 0, KC_F64 = 1, KC_STR = 2 };
enum : int32_t { MA_ADD_U64 = 0, MA_ADD_F64 = 1, MA_MAX_I64 = 2 };
// A combine op of this file only: the word is a group's centred sum of squares M2 = Σ (x − mean)² about the mean of
// the slot's own rows.  agg_multi sees such a line as MA_ADD_F64 with unused slots (every pane starts it at 0.0),
// win_m2_kernel fills it, and slots are combined with Chan et al.'s update (win_combine_kernel).
enum : int32_t { MA_M2 = 3 };
// The other centred words of this file: a group's third and fourth central sums M3 = Σ (x − mean)³, M4 = Σ (x − mean)⁴
// and the co-moment Cxy = Σ (x − mean_x)(y − mean_y) of a pair, each about the means of the slot's own rows.  All
// three sit in lines of one combine op; ``momdesc`` says per word which it is and which words of the row it reads
// (kind << 24 | four 6-bit word indices).  agg_multi sees such a line as unused f64 words, win_mom_kernel fills it.
enum : int32_t { MA_MOM = 4 };
enum : int32_t { MOM_M3 = 1, MOM_M4 = 2, MOM_CXY = 3 };
// The low word of a two-word order key (MIN / MAX of a decimal held as two int64 lanes): the key's high word is an
// ordinary MA_MAX word of the same row (the hi lane, complemented for MIN), this word holds the lo lane's unsigned
// order mapped to signed (lo ^ 2^63, complemented for MIN) of the rows whose high key equals the row's high word.
// ``lodesc`` names per word its high word (index | 1 << 16; 0: padding).  agg_multi sees such a line as MA_MAX with
// unused slots (every pane starts it at INT64_MIN), win_dec_kernel fills it after the high word is finished.
enum : int32_t { MA_LOKEY = 5 };
// Row picks (first / last / max_by / min_by): per pane and group the state is "which row wins" and that row's value.
//   MA_PICK_RANK lines hold rank words R: identity INT64_MIN ("no row"), else a monotone map of the winning row's index
//                in its pane — INT64_MAX − i where the smallest index wins (first, max_by, min_by: ties on the key keep
//                the first row), i where the largest wins (last).  win_pick_kernel fills them by a 64-bit max.
//   MA_PICK_VAL  lines hold, per payload argument x, a word P = the 64 bits of x of the winning row and a word V =
//                1.0 / 0.0 (x non-NULL / NULL there), both 0 without a row; win_pick_gather_kernel fills them.
// max_by / min_by also have a key word K, an ordinary MA_MAX word agg_multi fills from y (complemented for min_by).
// ``pickdesc`` [stride] names per word of these lines its R word (bits 0-7), its K word + 1 (bits 8-15; 0: not
// keyed), "last among equals" (bit 16) and "in use" (bit 17; 0: padding).  Ranks of different panes do not compare:
// slots are combined by their place in the ``slots`` array (the window's row order), see win_combine_kernel.
// agg_multi sees both kinds of line as unused words (INT64_MIN and 0).
enum : int32_t { MA_PICK_RANK = 6, MA_PICK_VAL = 7 };
// MIN / MAX over a string argument of up to kKeyWidth bytes: a whole line is one order key.  Words 0-5 hold the
// string's bytes big-endian and zero-padded, each mapped to the signed order (^ 2^63); word 6 holds its length
// (signed); word 7 is spare.  For MIN every used word is complemented, so that "greatest tuple" is the smallest
// string.  The identity of every word is INT64_MIN: the empty string's byte words equal it under MAX, and its length
// word 0 > INT64_MIN still beats "no row"; zero padding makes "ab" and "ab\0" equal in the byte words and the
// length word puts the prefix first.  ``strdesc`` [stride] names per word of such a line its place in the tuple + 1
// (0: the spare word, or a line not in use).  agg_multi sees the line as MA_MAX with unused slots (every pane starts
// it at INT64_MIN); dxa_win_strkey fills it after the multi-aggregate.
enum : int32_t { MA_STRKEY = 8 };

// same layout as hash_groupby.hip's KeyCols (built by dxa/ops/hashing.py key_cols)
struct KeyCol {
  const void* data;
  const int64_t* starts;
  const int32_t* lens;
  const uint8_t* valid;
  int32_t kind;
  int32_t pad;
};
struct KeyCols {
  KeyCol c[kMaxKeyCols];
  int32_t ncols;
  int64_t n;
};

// dictionary key storage, one entry per key column: int64 values (doubles as normalised bit patterns) or
// kKeyWidth-byte string slots + lengths; validity per group
struct DictCol {
  void* vals;          // int64 [gcap + 1]  or  uint8 [(gcap + 1) * kKeyWidth]
  int32_t* lens;       // strings only
  uint8_t* valid;
  int32_t kind;
  int32_t pad;
};
struct DictCols {
  DictCol c[kMaxKeyCols];
  int32_t ncols;
  int32_t gcap;
};

__device__ __forceinline__ uint64_t norm_f64_bits(double d) {
  if (d == 0.0) d = 0.0;                                   // -0.0 groups with 0.0
  uint64_t b = (uint64_t)__double_as_longlong(d);
  return d != d ? 0x7ff8000000000000ull : b;               // one NaN
}

__device__ __forceinline__ uint64_t key_word(const KeyCol& k, int64_t i) {
  return k.kind == KC_F64 ? norm_f64_bits(((const double*)k.data)[i]) : (uint64_t)((const int64_t*)k.data)[i];
}

// 5. combine the window's ring slots: out[g][w] = ⊕ over slots s of ring[s][g][w], for g < groups in the dictionary.
// With ``fixed_rows`` (a block combine) every one of those rows is written, but the member slots are read only for
// the groups the dictionary holds: the rows above them are the identity in every member (no row has been
// accumulated there), so they are written as the identity without a read and the cost follows the groups in use,
// not the capacity.  (A template parameter, so the per-batch combine keeps its wave-uniform slot loop.)
// ``kM2``: the layout has MA_M2 lines and ``m2desc`` [stride] names, for each M2 word, the row's count word (low 16
// bits) and sum word (high 16 bits) of the same argument.  An M2 word combines as
//   M2 = Σ_s [ M2_s + n_s (sum_s / n_s − mean)² ],  mean = Σ sum_s / Σ n_s,  over the slots with n_s > 0
// (the multi-way form of Chan's update: exact algebra, every term centred), so a block slot holds a valid
// (n, sum, M2) triple about the block's mean and blocks and loose panes combine by the same formula.  Without kM2
// the branch is compiled out (dxa_win_live runs that form over any layout: it reads the count word only).
// ``kMom``: the layout has MA_MOM lines and ``momdesc`` [stride] describes each of their words: kind << 24 and the
// row's words a | b << 6 | c << 12 | d << 18 — a the count, b the sum (of x), then for M3 c = M2; for M4 c = M2,
// d = M3; for Cxy c = the sum of y.  With δ_s = sum_s / n_s − mean (ε_s the same for y) over the slots with n_s > 0:
//   M3  = Σ_s [ M3_s + 3 δ_s M2_s + n_s δ_s³ ]
//   M4  = Σ_s [ M4_s + 4 δ_s M3_s + 6 δ_s² M2_s + n_s δ_s⁴ ]
//   Cxy = Σ_s [ Cxy_s + n_s δ_s ε_s ]
// Every right-hand side reads the slots' words only, never a combined word, so each output word is computed on its
// own like M2.  A padding word of such a line (kind 0) is written as 0.0.  Without kMom the branch is compiled out.
// ``kKey``: the layout has MA_LOKEY lines and ``lodesc`` [stride] names each of their words' high word.  Such a word
// combines as the max of the slots' words over the slots whose high word equals the max of the high words, so the
// (high, low) pair is the lexicographic max; slots that are all the identity (INT64_MIN twice) give the identity.
// Without kKey the branch is compiled out.
// ``kPick``: the layout has MA_PICK_RANK / MA_PICK_VAL lines and ``pickdesc`` [stride] names each of their words' R
// word and K word.  Such a word is taken from one slot: among the slots, in the order of ``slots``, whose R word is not
// the identity — and, for a keyed pick, whose K word equals the max of the K words — the first one, or the last one
// for ``last``.  R, P and V of one pick choose the same slot, so a block slot holds a consistent (K, R, P, V) again
// (its R only says "has a row": nothing decodes a combined rank).  No such slot gives the line's identity.  Without
// kPick the branch is compiled out.
// ``kStr``: the layout has MA_STRKEY lines and ``strdesc`` [stride] names each of their words' place in the line's
// 7-word tuple.  Such a word is taken from the slot whose tuple is lexicographically greatest (the first such slot;
// equal tuples hold equal words), so the line stays one string's key; slots that are all the identity give the
// identity.  A maximum over a total order: associative, so block slots and scratch slots combine like panes.
// Without kStr the branch is compiled out.
template <bool kBlock, bool kM2, bool kMom, bool kKey, bool kPick, bool kStr>
__global__ __launch_bounds__(256) void win_combine_kernel(const unsigned long long* __restrict__ ring,
                                                          int64_t slot_words, const int32_t* __restrict__ slots,
                                                          int32_t nslots_in, int32_t stride,
                                                          const int32_t* __restrict__ line_op,
                                                          const int32_t* __restrict__ scal, int32_t gcap,
                                                          int32_t fixed_rows, unsigned long long* __restrict__ out,
                                                          const int32_t* __restrict__ m2desc,
                                                          const int32_t* __restrict__ momdesc,
                                                          const int32_t* __restrict__ lodesc,
                                                          const int32_t* __restrict__ pickdesc,
                                                          const int32_t* __restrict__ strdesc) {
  int32_t ng = scal[0];
  if (ng > gcap) ng = gcap;
  const int64_t held = (int64_t)ng * stride;
  const int64_t total = kBlock ? (int64_t)fixed_rows * stride : held;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int w = (int)(idx % stride);
    const int op = line_op[w >> 3];
    const int nslots = (!kBlock || idx < held) ? nslots_in : 0;   // no member reads above the groups in use
    if (op == MA_ADD_F64) {
      double acc = 0.0;
      for (int s = 0; s < nslots; ++s) acc += __longlong_as_double((long long)ring[(int64_t)slots[s] * slot_words + idx]);
      out[idx] = (unsigned long long)__double_as_longlong(acc);
    } else if (op == MA_ADD_U64) {
      unsigned long long acc = 0;
      for (int s = 0; s < nslots; ++s) acc += ring[(int64_t)slots[s] * slot_words + idx];
      out[idx] = acc;
    } else if (kM2 && op == MA_M2) {
      const int32_t dsc = m2desc[w];
      const int64_t ci = idx - w + (dsc & 0xffff), si = idx - w + (dsc >> 16);
      double n = 0.0, sum = 0.0;
      for (int s = 0; s < nslots; ++s) {
        const int64_t base = (int64_t)slots[s] * slot_words;
        n += __longlong_as_double((long long)ring[base + ci]);
        sum += __longlong_as_double((long long)ring[base + si]);
      }
      const double mean = sum / (n > 0.0 ? n : 1.0);
      double acc = 0.0;
      for (int s = 0; s < nslots; ++s) {
        const int64_t base = (int64_t)slots[s] * slot_words;
        const double ns = __longlong_as_double((long long)ring[base + ci]);
        if (ns == 0.0) continue;
        const double d = __longlong_as_double((long long)ring[base + si]) / ns - mean;
        acc += __longlong_as_double((long long)ring[base + idx]) + ns * d * d;
      }
      out[idx] = (unsigned long long)__double_as_longlong(acc);
    } else if (kMom && op == MA_MOM) {
      const int32_t dsc = momdesc[w];
      const int kind = dsc >> 24;
      const int64_t r0 = idx - w;
      const int64_t ci = r0 + (dsc & 63), si = r0 + ((dsc >> 6) & 63), ti = r0 + ((dsc >> 12) & 63),
                    ui = r0 + ((dsc >> 18) & 63);
      const int ns_in = kind ? nslots : 0;
      double n = 0.0, sum = 0.0, sumy = 0.0;
      for (int s = 0; s < ns_in; ++s) {
        const int64_t base = (int64_t)slots[s] * slot_words;
        n += __longlong_as_double((long long)ring[base + ci]);
        sum += __longlong_as_double((long long)ring[base + si]);
        if (kind == MOM_CXY) sumy += __longlong_as_double((long long)ring[base + ti]);
      }
      const double den = n > 0.0 ? n : 1.0;
      const double mean = sum / den, meany = sumy / den;
      double acc = 0.0;
      for (int s = 0; s < ns_in; ++s) {
        const int64_t base = (int64_t)slots[s] * slot_words;
        const double ns = __longlong_as_double((long long)ring[base + ci]);
        if (ns == 0.0) continue;
        const double d = __longlong_as_double((long long)ring[base + si]) / ns - mean;
        const double own = __longlong_as_double((long long)ring[base + idx]);
        const double t = __longlong_as_double((long long)ring[base + ti]);     // M2_s, or the slot's sum of y
        if (kind == MOM_CXY) {
          acc += own + ns * d * (t / ns - meany);
        } else if (kind == MOM_M3) {
          acc += own + 3.0 * d * t + ns * d * d * d;
        } else {
          const double m3 = __longlong_as_double((long long)ring[base + ui]);
          acc += own + 4.0 * d * m3 + 6.0 * d * d * t + ns * d * d * d * d;
        }
      }
      out[idx] = (unsigned long long)__double_as_longlong(acc);
    } else if (kKey && op == MA_LOKEY) {
      const int32_t dsc = lodesc[w];
      const int64_t hi_at = idx - w + (dsc & 0xffff);
      const int ns_in = dsc ? nslots : 0;
      long long top = (long long)0x8000000000000000ull;
      for (int s = 0; s < ns_in; ++s) {
        const long long h = (long long)ring[(int64_t)slots[s] * slot_words + hi_at];
        top = h > top ? h : top;
      }
      long long acc = (long long)0x8000000000000000ull;
      for (int s = 0; s < ns_in; ++s) {
        const int64_t base = (int64_t)slots[s] * slot_words;
        if ((long long)ring[base + hi_at] != top) continue;
        const long long v = (long long)ring[base + idx];
        acc = v > acc ? v : acc;
      }
      out[idx] = (unsigned long long)acc;
    } else if (kPick && (op == MA_PICK_RANK || op == MA_PICK_VAL)) {
      const int32_t dsc = pickdesc[w];
      const int ns_in = dsc ? nslots : 0;
      const int64_t r_at = idx - w + (dsc & 0xff);
      const int kw = (dsc >> 8) & 0xff;
      const int64_t k_at = idx - w + kw - 1;
      const bool last = (dsc >> 16) & 1;
      const long long none = (long long)0x8000000000000000ull;
      long long top = none;
      for (int s = 0; kw && s < ns_in; ++s) {
        const long long k = (long long)ring[(int64_t)slots[s] * slot_words + k_at];
        top = k > top ? k : top;
      }
      unsigned long long acc = op == MA_PICK_RANK ? 0x8000000000000000ull : 0ull;
      for (int s = 0; s < ns_in; ++s) {
        const int64_t base = (int64_t)slots[s] * slot_words;
        if ((long long)ring[base + r_at] == none || (kw && (long long)ring[base + k_at] != top)) continue;
        acc = ring[base + idx];
        if (!last) break;
      }
      out[idx] = acc;
    } else if (kStr && op == MA_STRKEY) {
      const int32_t dsc = strdesc[w];
      const int ns_in = dsc ? nslots : 0;
      const int64_t t_at = idx - (w & 7);
      const long long none = (long long)0x8000000000000000ull;
      long long top[7] = {none, none, none, none, none, none, none};
      for (int s = 0; s < ns_in; ++s) {
        const unsigned long long* t = ring + (int64_t)slots[s] * slot_words + t_at;
        bool greater = false;
#pragma unroll
        for (int q = 0; q < 7; ++q) {
          const long long v = (long long)t[q];
          if (v != top[q]) {
            greater = v > top[q];
            break;
          }
        }
        if (!greater) continue;
#pragma unroll
        for (int q = 0; q < 7; ++q) top[q] = (long long)t[q];
      }
      long long acc = none;
#pragma unroll
      for (int q = 0; q < 7; ++q) acc = dsc == q + 1 ? top[q] : acc;
      out[idx] = (unsigned long long)acc;
    } else {
      long long acc = (long long)0x8000000000000000ull;
      for (int s = 0; s < nslots; ++s) {
        const long long v = (long long)ring[(int64_t)slots[s] * slot_words + idx];
        acc = v > acc ? v : acc;
      }
      out[idx] = (unsigned long long)acc;
    }
  }
}

// 6. groups with rows in the window: keep[g] = count word > 0 (count words are f64 sums), counted into scal[2]
__global__ void win_keep_kernel(const unsigned long long* __restrict__ acc, int32_t stride, int32_t count_word,
                                const int32_t* __restrict__ scal_in, int32_t gcap, uint8_t* __restrict__ keep,
                                int32_t* __restrict__ scal) {
  int32_t ng = scal_in[0];
  if (ng > gcap) ng = gcap;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < gcap; g += (int64_t)gridDim.x * blockDim.x) {
    bool k = false;
    if (g < ng) k = __longlong_as_double((long long)acc[g * stride + count_word]) > 0.0;
    keep[g] = k ? 1 : 0;
    if (k) atomicAdd(&scal[2], 1);
  }
}

// exclusive positions of the kept groups (one block-sequential scan is enough for ≤ 2^20 groups: the keep flags
// are scanned by a single workgroup in 256-wide chunks) → out_idx[pos] = g
__global__ __launch_bounds__(256) void win_compact_kernel(const uint8_t* __restrict__ keep, int32_t gcap,
                                                          const int32_t* __restrict__ scal,
                                                          int64_t* __restrict__ out_idx) {
  __shared__ int32_t part[256];
  int32_t base = 0;
  int32_t ng = scal[0];
  if (ng > gcap) ng = gcap;
  for (int32_t c0 = 0; c0 < ng; c0 += 256 * 16) {
    // each thread counts 16 consecutive flags
    const int32_t lo = c0 + threadIdx.x * 16;
    int32_t cnt = 0;
    for (int q = 0; q < 16; ++q) cnt += (lo + q < ng && keep[lo + q]) ? 1 : 0;
    part[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {              // inclusive scan of the 256 counts
      const int32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
      __syncthreads();
      part[threadIdx.x] += v;
      __syncthreads();
    }
    int32_t pos = base + part[threadIdx.x] - cnt;
    for (int q = 0; q < 16; ++q) {
      const int32_t g = lo + q;
      if (g < ng && keep[g]) out_idx[pos++] = g;
    }
    base += part[255];
    __syncthreads();
  }
}

// 2b. the second pass of a pane's accumulation, for the variance family: agg_multi has finished the slot's count and
// sum words, so every row's group mean is known and each row with a valid argument adds (x − sum_g / n_g)² into the
// group's M2 word — the centred form; Σx² − (Σx)²/n would cancel catastrophically at offset values.  Rows of the dump
// row (WHERE-filtered or dictionary-full, gid == gcap) are skipped: nobody reads its M2 and they would all hit one
// address.  A window with a handful of groups puts every row of a pane on a handful of words, and every adder on one
// row runs an order of magnitude below the float-atomic rate, so groups with ids below kM2LdsGroups are summed in
// LDS (f64 LDS adds) and flushed with one global add per touched group and workgroup; ids at or above the bound go
// straight to global adds, which such a dictionary spreads over many rows.  The choice is made per row here — the
// host's group count is a batch stale — so both halves are always correct.  One launch covers all of a statement's
// variance arguments, one after the other through the same LDS array.
constexpr int kMaxM2Args = 8;
constexpr int kM2LdsGroups = dxa::kLdsGroupIds;      // (str_minmax.hip's arg-extreme kernel uses the same bound)
struct M2Arg {
  const double* x;
  const uint8_t* valid;
  int32_t cnt;             // words of the slot row: the argument's count, sum and M2
  int32_t sum;
  int32_t m2;
  int32_t pad;
};
struct M2Args {
  M2Arg a[kMaxM2Args];
  const int32_t* gid;
  double* row;             // the ring slot: [gcap + 1][stride]
  int64_t n;
  int32_t gcap;
  int32_t stride;
  int32_t nargs;
  int32_t pad;
};

__global__ __launch_bounds__(256) void win_m2_kernel(const M2Args m) {
  __shared__ double part[kM2LdsGroups];
  const int32_t lds_groups = m.gcap < kM2LdsGroups ? m.gcap : kM2LdsGroups;
  for (int k = 0; k < m.nargs; ++k) {
    const M2Arg a = m.a[k];
    for (int g = threadIdx.x; g < kM2LdsGroups; g += blockDim.x) part[g] = 0.0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m.n; i += (int64_t)gridDim.x * blockDim.x) {
      const int32_t g = m.gid[i];
      if (g < 0 || g >= m.gcap || (a.valid && !a.valid[i])) continue;
      double* r = m.row + (int64_t)g * m.stride;
      const double d = a.x[i] - r[a.sum] / r[a.cnt];      // the row itself was counted: n_g ≥ 1
      if (g < kM2LdsGroups) atomicAdd(&part[g], d * d);
      else atomicAdd(r + a.m2, d * d);
    }
    __syncthreads();
    for (int g = threadIdx.x; g < lds_groups; g += blockDim.x) {
      const double v = part[g];
      if (v != 0.0) atomicAdd(m.row + (int64_t)g * m.stride + a.m2, v);
    }
    __syncthreads();
  }
}

// 2c. the same second pass for the MA_MOM words (skewness / kurtosis: M3 and M4 of an argument; corr / covar: Cxy
// of a pair of arguments whose validity is already "both non-null"): d = x − sum_g / n_g as above, and d³, d⁴ or
// d_x · d_y go into the group's words.  One sweep per argument (or pair) adds all of its words — the row's group id,
// value and the dependent read of the group's sum and count are fetched once for M3 and M4 — through two LDS arrays
// (16 KB: the occupancy stays bounded by the 512-workgroup grid, not by LDS).  Ids below kM2LdsGroups are summed in
// LDS and flushed with one global add per touched group, word and workgroup; the others add straight to the row.
constexpr int kMaxMomArgs = 8;
struct MomArg {
  const double* x;
  const double* y;         // null: M3 (w0) and, with w1 >= 0, M4 (w1) of x; else Cxy (w0) of (x, y)
  const uint8_t* valid;
  int32_t cnt;             // words of the slot row: the count, the sum of x, the sum of y, the output words
  int32_t sum;
  int32_t sumy;
  int32_t w0;
  int32_t w1;
  int32_t pad;
};
struct MomArgs {
  MomArg a[kMaxMomArgs];
  const int32_t* gid;
  double* row;             // the ring slot: [gcap + 1][stride]
  int64_t n;
  int32_t gcap;
  int32_t stride;
  int32_t nargs;
  int32_t pad;
};

__global__ __launch_bounds__(256) void win_mom_kernel(const MomArgs m) {
  __shared__ double part[2][kM2LdsGroups];
  const int32_t lds_groups = m.gcap < kM2LdsGroups ? m.gcap : kM2LdsGroups;
  for (int k = 0; k < m.nargs; ++k) {
    const MomArg a = m.a[k];
    const bool two = a.w1 >= 0;
    for (int g = threadIdx.x; g < kM2LdsGroups; g += blockDim.x) {
      part[0][g] = 0.0;
      part[1][g] = 0.0;
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m.n; i += (int64_t)gridDim.x * blockDim.x) {
      const int32_t g = m.gid[i];
      if (g < 0 || g >= m.gcap || (a.valid && !a.valid[i])) continue;
      double* r = m.row + (int64_t)g * m.stride;
      const double nn = r[a.cnt];                          // the row itself was counted: n_g ≥ 1
      const double d = a.x[i] - r[a.sum] / nn;
      double v0, v1 = 0.0;
      if (a.y) {
        v0 = d * (a.y[i] - r[a.sumy] / nn);
      } else {
        v0 = d * d * d;
        v1 = v0 * d;
      }
      if (g < kM2LdsGroups) {
        atomicAdd(&part[0][g], v0);
        if (two) atomicAdd(&part[1][g], v1);
      } else {
        atomicAdd(r + a.w0, v0);
        if (two) atomicAdd(r + a.w1, v1);
      }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < lds_groups; g += blockDim.x) {
      const double v = part[0][g];
      if (v != 0.0) atomicAdd(m.row + (int64_t)g * m.stride + a.w0, v);
      if (two) {
        const double u = part[1][g];
        if (u != 0.0) atomicAdd(m.row + (int64_t)g * m.stride + a.w1, u);
      }
    }
    __syncthreads();
  }
}

// 2d. the same second pass for decimal arguments, read in place: ``x`` is the column's int64 storage, one lane per
// row (a value below 10^18, hi = its sign) or two (lo at 2i, hi at 2i + 1).
//   DEC_SUM: the row adds lo & 0xffffffff, lo >> 32 (unsigned) and hi (signed) into three MA_ADD_U64 words of its
//            group.  Each word is exact while a group has fewer than 2^31 rows in the window, the words combine with
//            the ordinary u64 add, and integer adds make the result independent of the arrival order.
//   DEC_KEY_MAX / DEC_KEY_MIN: agg_multi has finished the group's high key word (w1); a row whose high key (hi, ~hi
//            for MIN) equals it puts its low key (lo ^ 2^63, complemented for MIN) into the MA_LOKEY word w0 by max.
// Ids below kM2LdsGroups go through LDS u64 arrays and are flushed with one global atomic per touched group, word
// and workgroup; the others go straight to the row with non-returning 64-bit atomics.  Rows of the dump row and
// rows with a NULL argument are skipped.  One launch covers all decimal jobs of a statement.
constexpr int kMaxDecJobs = 8;
enum : int32_t { DEC_SUM = 0, DEC_KEY_MAX = 1, DEC_KEY_MIN = 2 };
struct DecJob {
  const long long* x;
  const uint8_t* valid;
  int32_t lanes;           // 1 or 2
  int32_t kind;
  int32_t w0;              // words of the slot row: DEC_SUM: the three limb sums; keys: the low word, the high word
  int32_t w1;
  int32_t w2;
  int32_t pad;
};
struct DecArgs {
  DecJob a[kMaxDecJobs];
  const int32_t* gid;
  unsigned long long* row; // the ring slot: [gcap + 1][stride]
  int64_t n;
  int32_t gcap;
  int32_t stride;
  int32_t nargs;
  int32_t pad;
};

__global__ __launch_bounds__(256) void win_dec_kernel(const DecArgs m) {
  __shared__ unsigned long long part[3][kM2LdsGroups];
  constexpr unsigned long long kLowest = 0x8000000000000000ull;
  const int32_t lds_groups = m.gcap < kM2LdsGroups ? m.gcap : kM2LdsGroups;
  for (int k = 0; k < m.nargs; ++k) {
    const DecJob a = m.a[k];
    const bool sum = a.kind == DEC_SUM;
    for (int g = threadIdx.x; g < kM2LdsGroups; g += blockDim.x) {
      part[0][g] = sum ? 0ull : kLowest;
      part[1][g] = 0ull;
      part[2][g] = 0ull;
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m.n; i += (int64_t)gridDim.x * blockDim.x) {
      const int32_t g = m.gid[i];
      if (g < 0 || g >= m.gcap || (a.valid && !a.valid[i])) continue;
      const long long lo = a.x[i * a.lanes];
      const long long hi = a.lanes == 2 ? a.x[i * 2 + 1] : (lo >> 63);
      unsigned long long* r = m.row + (int64_t)g * m.stride;
      if (sum) {
        const unsigned long long l0 = (unsigned long long)lo & 0xffffffffull, l1 = (unsigned long long)lo >> 32;
        if (g < kM2LdsGroups) {
          atomicAdd(&part[0][g], l0);
          atomicAdd(&part[1][g], l1);
          if (hi) atomicAdd(&part[2][g], (unsigned long long)hi);
        } else {
          atomicAdd(r + a.w0, l0);
          atomicAdd(r + a.w1, l1);
          if (hi) atomicAdd(r + a.w2, (unsigned long long)hi);
        }
      } else {
        const bool mn = a.kind == DEC_KEY_MIN;
        if ((mn ? ~hi : hi) != (long long)r[a.w1]) continue;
        long long key = lo ^ (long long)kLowest;
        if (mn) key = ~key;
        if (g < kM2LdsGroups) atomicMax((long long*)&part[0][g], key);
        else atomicMax((long long*)(r + a.w0), key);
      }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < lds_groups; g += blockDim.x) {
      unsigned long long* r = m.row + (int64_t)g * m.stride;
      if (sum) {
        const unsigned long long v0 = part[0][g], v1 = part[1][g], v2 = part[2][g];
        if (v0) atomicAdd(r + a.w0, v0);
        if (v1) atomicAdd(r + a.w1, v1);
        if (v2) atomicAdd(r + a.w2, v2);
      } else if (part[0][g] != kLowest) {
        atomicMax((long long*)(r + a.w0), (long long)part[0][g]);
      }
    }
    __syncthreads();
  }
}

// 2e. the same second pass for row picks, in two launches.
// win_pick_kernel: every rank job of the statement, one after the other through one LDS u64 array (8 KB).  A row that
// counts puts its rank (INT64_MAX − i: the smallest index wins; i for ``last``) into its group's R word by a 64-bit
// max.  Rows of the dump row (WHERE-filtered or dictionary-full) and ids outside [0, gcap) never count.  For a keyed
// job (max_by / min_by) agg_multi has finished the group's K word from the same ``y`` array, so a row counts when its
// y is non-NULL and its key — y itself, or hash_groupby.hip's f64_ordered(y) for a double (MV_F64_ORD), complemented
// for min_by — equals K: the rows that tie on the extreme y, of which the smallest index wins.
//   Order of a double y: query._arg_extreme sorts by ops/sort.py's order key, where NaN is the largest value, every
//   NaN is the same value and -0.0 == 0.0.  f64_ordered agrees on NaN (one canonical NaN, the greatest) but puts
//   -0.0 below 0.0, so the host hands both kernels a copy of y with -0.0 replaced by 0.0 (window_dense.py
//   ``accumulate``): the zeros tie and the first row wins, as in _arg_extreme.
// Ids below kM2LdsGroups go through LDS and are flushed with one global atomic per touched group and workgroup, the
// others go straight to the row with non-returning 64-bit atomics.
// win_pick_gather_kernel: a second launch, because R must be complete.  Threads stride over the groups in use (the
// device's group counter, clamped to gcap: no host read); per payload job the row index is decoded from R and checked
// against [0, n) before any load — the identity or a stale R never becomes an index — and x[row]'s 64 bits go into P,
// 1.0 / 0.0 from x's validity into V.  A group without a row keeps the identities (R = INT64_MIN, P = V = 0).
constexpr int kMaxPickJobs = 8;
struct PickRank {
  const long long* y;      // null: first / last (every row of the group counts)
  const uint8_t* yvalid;
  int32_t kind;            // keyed: the K slot's agg_multi value kind, MV_I64 (1) or MV_F64_ORD (3), | MV_NOT (4)
  int32_t k;               // words of the slot row: K (keyed jobs) and R
  int32_t r;
  int32_t last;
};
struct PickVal {
  const long long* x;      // the payload argument as 64-bit words
  const uint8_t* xvalid;
  int32_t r;               // words of the slot row: the rank word read, the payload and validity words written
  int32_t p;
  int32_t v;
  int32_t last;            // how R maps to a row index
};
struct PickArgs {
  PickRank rank[kMaxPickJobs];
  PickVal val[kMaxPickJobs];
  const int32_t* gid;
  unsigned long long* row; // the ring slot: [gcap + 1][stride]
  const int32_t* scal;     // the dictionary's status: scal[0] = groups in use
  int64_t n;
  int32_t gcap;
  int32_t stride;
  int32_t nrank;
  int32_t nval;
};

// hash_groupby.hip's f64_ordered: the total order of doubles as signed integers, NaN canonical and greatest
__device__ __forceinline__ long long pick_f64_ordered(double d) {
  long long b = __double_as_longlong(d);
  if (d != d) b = 0x7ff8000000000000ll;
  return b >= 0 ? b : (b ^ 0x7fffffffffffffffll);
}

__global__ __launch_bounds__(256) void win_pick_kernel(const PickArgs m) {
  __shared__ long long part[kM2LdsGroups];
  constexpr long long kNone = (long long)0x8000000000000000ull;
  const int32_t lds_groups = m.gcap < kM2LdsGroups ? m.gcap : kM2LdsGroups;
  for (int k = 0; k < m.nrank; ++k) {
    const PickRank a = m.rank[k];
    for (int g = threadIdx.x; g < kM2LdsGroups; g += blockDim.x) part[g] = kNone;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m.n; i += (int64_t)gridDim.x * blockDim.x) {
      const int32_t g = m.gid[i];
      if (g < 0 || g >= m.gcap) continue;
      unsigned long long* r = m.row + (int64_t)g * m.stride;
      if (a.y) {
        if (a.yvalid && !a.yvalid[i]) continue;
        long long key = (a.kind & 3) == 3 ? pick_f64_ordered(__longlong_as_double(a.y[i])) : a.y[i];
        if (a.kind & 4) key = ~key;
        if (key != (long long)r[a.k]) continue;
      }
      const long long rank = a.last ? (long long)i : 0x7fffffffffffffffll - (long long)i;
      if (g < kM2LdsGroups) atomicMax(&part[g], rank);
      else atomicMax((long long*)(r + a.r), rank);
    }
    __syncthreads();
    for (int g = threadIdx.x; g < lds_groups; g += blockDim.x)
      if (part[g] != kNone) atomicMax((long long*)(m.row + (int64_t)g * m.stride + a.r), part[g]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void win_pick_gather_kernel(const PickArgs m) {
  constexpr long long kNone = (long long)0x8000000000000000ull;
  int32_t ng = m.scal[0];
  if (ng > m.gcap) ng = m.gcap;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long* r = m.row + g * m.stride;
    for (int k = 0; k < m.nval; ++k) {
      const PickVal a = m.val[k];
      const long long rank = (long long)r[a.r];
      if (rank == kNone) continue;
      // (unsigned: a stale word may hold anything, and the subtraction must not overflow)
      const long long i = a.last ? rank : (long long)(0x7fffffffffffffffull - (unsigned long long)rank);
      if (i < 0 || i >= m.n) continue;
      r[a.p] = (unsigned long long)a.x[i];
      r[a.v] = (unsigned long long)__double_as_longlong(a.xvalid && !a.xvalid[i] ? 0.0 : 1.0);
    }
  }
}

// 2f. the same second pass for MIN / MAX over strings.  Per job str_minmax.hip's arg-extreme kernel (dxa_str_argext,
// over the pane's rows with the pane's ids and WHERE mask; the dump row's id gcap is outside its [0, gcap)) leaves in
// ``best`` [job][gcap] the pane's winning row per group, then win_strkey_gather_kernel — threads stride over the
// groups in use, as win_pick_gather_kernel's do — checks each index against [0, n) before any load and writes the
// winner's packed words into the job's MA_STRKEY line.  A winner longer than kKeyWidth bytes has no key: status bit 8
// is set (never cleared; the host sends the statement to the paned path) and the line keeps the identity.  A later
// job that could reuse the line for a row pick's string payload only needs another source of the row index.
constexpr int kMaxStrJobs = 8;
struct StrJob {
  const uint8_t* arena;
  const int64_t* starts;
  const int32_t* lens;
  const uint8_t* valid;
  int32_t line;            // the first word of the job's line in the slot row (a multiple of 8)
  int32_t min;             // 1: MIN (every used word complemented)
};
struct StrKeyArgs {
  StrJob a[kMaxStrJobs];
  const int32_t* gid;
  const uint8_t* keep;     // the pane's WHERE mask or null
  unsigned long long* row; // the ring slot: [gcap + 1][stride]
  int32_t* scal;           // the dictionary's status: scal[0] = groups in use, scal[1] |= 8: a winner too long
  int64_t* best;           // [njobs][gcap] scratch
  int64_t n;
  int32_t gcap;
  int32_t stride;
  int32_t njobs;
  int32_t pad;
};

__global__ __launch_bounds__(256) void win_strkey_gather_kernel(const StrKeyArgs m) {
  int32_t ng = m.scal[0];
  if (ng > m.gcap) ng = m.gcap;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long* r = m.row + g * m.stride;
    for (int k = 0; k < m.njobs; ++k) {
      const StrJob a = m.a[k];
      const long long i = m.best[(int64_t)k * m.gcap + g];
      if (i < 0 || i >= m.n) continue;
      const int32_t l = a.lens[i];
      if (l < 0 || l > kKeyWidth) {
        atomicOr(&m.scal[1], 8);
        continue;
      }
      const uint8_t* p = a.arena + a.starts[i];
#pragma unroll
      for (int q = 0; q < kKeyWidth / 8; ++q) {
        const int32_t left = l - 8 * q;
        const uint64_t w = left <= 0 ? 0ull : __builtin_bswap64(dxa::load_le(p + 8 * q, left < 8 ? left : 8));
        const long long key = (long long)(w ^ 0x8000000000000000ull);
        r[a.line + q] = (unsigned long long)(a.min ? ~key : key);
      }
      r[a.line + kKeyWidth / 8] = (unsigned long long)(a.min ? ~(long long)l : (long long)l);
    }
  }
}

__device__ __forceinline__ uint64_t row_hash(const KeyCols& a, int64_t i) {
  uint64_t h = 0;
  for (int j = 0; j < a.ncols; ++j) {
    const KeyCol& k = a.c[j];
    uint64_t x;
    if (k.valid && !k.valid[i]) x = dxa::kNullHash;
    else if (k.kind == KC_STR) x = dxa::hash_bytes((const uint8_t*)k.data + k.starts[i], k.lens[i]);
    else x = dxa::hash_i64(key_word(k, i));
    h = j ? dxa::hash_combine(h, x) : x;
  }
  return h;
}

// store row i's key as group g's dictionary entry (the claiming lane, before it publishes g)
__device__ __forceinline__ void store_key(const KeyCols& a, const DictCols& d, int64_t i, int32_t g,
                                          int32_t* __restrict__ scal) {
  for (int j = 0; j < a.ncols; ++j) {
    const KeyCol& k = a.c[j];
    const DictCol& e = d.c[j];
    const bool ok = k.valid ? k.valid[i] != 0 : true;
    e.valid[g] = ok ? 1 : 0;
    if (!ok) continue;
    if (k.kind == KC_STR) {
      const int32_t l = k.lens[i];
      if (l > kKeyWidth) {
        atomicOr(&scal[1], 4);
        e.lens[g] = 0;
        continue;
      }
      const uint8_t* src = (const uint8_t*)k.data + k.starts[i];
      uint8_t* dst = (uint8_t*)e.vals + (int64_t)g * kKeyWidth;
      for (int32_t q = 0; q < l; ++q) dst[q] = src[q];
      e.lens[g] = l;
    } else {
      ((int64_t*)e.vals)[g] = (int64_t)key_word(k, i);
    }
  }
}

__device__ __forceinline__ bool key_differs(const KeyCols& a, const DictCols& d, int64_t i, int32_t g) {
  for (int j = 0; j < a.ncols; ++j) {
    const KeyCol& k = a.c[j];
    const DictCol& e = d.c[j];
    const bool vi = k.valid ? k.valid[i] != 0 : true;
    if (vi != (e.valid[g] != 0)) return true;
    if (!vi) continue;
    if (k.kind == KC_STR) {
      const int32_t l = k.lens[i];
      if (l != e.lens[g] || l > kKeyWidth) return true;
      // 8 bytes per step (dxa::load_le): the slot is 8-byte aligned, the row's bytes are not
      const uint8_t* x = (const uint8_t*)k.data + k.starts[i];
      const uint64_t* y = (const uint64_t*)((const uint8_t*)e.vals + (int64_t)g * kKeyWidth);
      for (int32_t q = 0; q < l; q += 8) {
        const int32_t nb = l - q < 8 ? l - q : 8;
        const uint64_t yw = nb < 8 ? y[q >> 3] & ((1ull << (8 * nb)) - 1ull) : y[q >> 3];
        if (dxa::load_le(x + q, nb) != yw) return true;
      }
    } else if ((int64_t)key_word(k, i) != ((const int64_t*)e.vals)[g]) {
      return true;
    }
  }
  return false;
}

// steps 1-3 in ONE pass: hash the row's key, look it up in the persistent dictionary; the lane whose CAS claims a
// new entry draws the group id, writes the key into the dictionary and only then publishes the id (release), so a
// lane that finds the entry (acquire) compares its key with a complete dictionary entry — a 64-bit collision or a
// key too long for a slot is flagged, never merged.  Claims and publications precede every wait in straight-line
// code (as hash_groupby.hip group_build_kernel): a waiting lane only waits on another wave.
__global__ void win_insert_kernel(const KeyCols a, DictCols d, const uint8_t* __restrict__ keep,
                                  uint64_t* __restrict__ keys, int64_t cap_mask,
                                  int32_t* __restrict__ gid_of_slot, int32_t* __restrict__ scal,
                                  int32_t* __restrict__ gid) {
  const int32_t gcap = d.gcap;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    if (keep && !keep[i]) {
      gid[i] = gcap;
      continue;
    }
    const uint64_t k = dxa::fix_key(row_hash(a, i));
    int64_t s = (int64_t)(dxa::fmix64(k) & (uint64_t)cap_mask);
    bool claimed = false;
    int64_t probes = 0;
    while (true) {
      const uint64_t cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == k) break;
      if (cur == dxa::kEmpty) {
        const uint64_t prev = atomicCAS((unsigned long long*)&keys[s], (unsigned long long)dxa::kEmpty,
                                        (unsigned long long)k);
        if (prev == dxa::kEmpty) { claimed = true; break; }
        if (prev == k) break;
      }
      s = (s + 1) & cap_mask;
      if (++probes > cap_mask) { s = -1; break; }
    }
    if (s < 0) {
      atomicOr(&scal[1], 2);
      gid[i] = gcap;
      continue;
    }
    int32_t g = -1;
    if (claimed) {
      g = atomicAdd(&scal[0], 1);
      if (g >= gcap) {
        atomicOr(&scal[1], 2);
        g = gcap;
      } else {
        store_key(a, d, i, g, scal);
      }
      __hip_atomic_store(&gid_of_slot[s], g, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!claimed) {
      do {
        g = __hip_atomic_load(&gid_of_slot[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      } while (g < 0);
      if (g < gcap && key_differs(a, d, i, g)) atomicOr(&scal[1], 1);
    }
    gid[i] = g;
  }
}

// The window's output rows, written once by position (no gather launches afterwards): position p < kept holds
// group out_idx[p]: its key columns (int64 words / the string's dictionary slot) and every requested aggregate
// finished from the combined accumulator row (the kinds of hash_groupby.hip agg_finish_kernel).  Outputs are
// [gcap]-strided; the host slices the first ``kept`` entries after its one read.
constexpr int kMaxEmit = 64;
enum : int { F_COUNT = 0, F_I64 = 1, F_F64 = 2, F_AVG = 3, F_F64_ORD = 4, F_VAR_SAMP = 5, F_VAR_POP = 6, F_NOT = 8,
             F_SQRT = 16 };
// The kinds with more operands live in bits 5-7 (their low three bits are 0): pos = Cxy / M3 / M4, cnt = n and
//   F_COVAR_POP  Cxy / n                       F_COVAR_SAMP  Cxy / (n − 1), NaN for n = 1
//   F_CORR       Cxy / sqrt(M2x · M2y), op2 = M2x, op3 = M2y; NaN unless M2x · M2y > 0
//   F_SKEW       sqrt(n) · M3 / M2^1.5, op2 = M2;  F_KURT  n · M4 / M2² − 3, op2 = M2; NaN unless M2 > 0
// (Spark 2.4's Covariance / Corr / CentralMomentAgg; n = 0 is NULL by the validity rule, as everywhere).
enum : int { F_COVAR_POP = 32, F_COVAR_SAMP = 64, F_CORR = 96, F_SKEW = 128, F_KURT = 160, F_KIND_MASK = 7 | 224 };
// Decimal results are 128-bit integers and take two output rows each, the same recipe once without and once with
// F_HI (the bit F_SQRT has in the variance kinds): the low 64 bits, then the signed high word.
//   F_DEC_SUM  pos, op2, op3 = the limb sums Σ (lo & 0xffffffff), Σ (lo >> 32), Σ hi: their carry-propagated total
//   F_DEC_AVG  the same words, cnt = n: total · 10^4 / n rounded HALF_UP (away from zero at a tie), exactly
//   F_DEC_MM   pos = the high key word (F_NOT: MIN, complemented), op2 = the low key word: the key mapping undone
enum : int { F_DEC_MM = 7, F_DEC_SUM = 192, F_DEC_AVG = 224, F_HI = 16 };
// A byte word of a string MIN / MAX key (MA_STRKEY): MIN's complement (F_NOT), then the order mapping, undone — the
// eight bytes big-endian again.  Its length word is finished as F_I64 (| F_NOT).  The kinds 0-7 and every multiple of
// 32 up to 224 are taken, so this one is the exception to the rule above: bits 5-7 AND a low bit set, with no further
// operand (emit_ok's range tests on the multi-operand kinds do not reach it, and F_KIND_MASK keeps it whole).
enum : int { F_STRW = 33 };
struct EmitArgs {
  const long long* acc;
  int32_t stride;
  int32_t nreq;
  int32_t kind[kMaxEmit];
  int32_t pos[kMaxEmit];
  int32_t cnt[kMaxEmit];
  int32_t op2[kMaxEmit];         // further words of the kinds above F_SQRT (unused: -1)
  int32_t op3[kMaxEmit];
  long long* dst;                // [nreq][gcap]
  uint8_t* dvalid;               // [nreq][gcap]
  int64_t* okey[kMaxKeyCols];    // [gcap] int64 key words, or the strings' starts in the dictionary arena
  int32_t* olen[kMaxKeyCols];    // strings: [gcap] lengths
  uint8_t* ovalid[kMaxKeyCols];  // [gcap]
  const int64_t* out_idx;
  const int32_t* scal;
  int32_t gcap;
};

// the 128-bit total w0 + w1 · 2^32 + w2 · 2^64 (mod 2^128) of a decimal argument's limb sums
__device__ __forceinline__ void dec_total(unsigned long long w0, unsigned long long w1, unsigned long long w2,
                                          unsigned long long& lo, long long& hi) {
  lo = w0 + (w1 << 32);
  hi = (long long)(w2 + (w1 >> 32) + (lo < w0 ? 1ull : 0ull));
}

// (hi, lo) · 10^4 / n rounded HALF_UP on the magnitude, for 0 < n < 2^31: q, r = |v| divmod n by schoolbook division
// over 32-bit limbs (the running remainder is below n, so every step fits 64 bits), then
// q · 10^4 + ⌊(2 · r · 10^4 + n) / 2n⌋ — the second term is the rounded quotient of the remainder, at most 10^4 —
// and the sign goes back on.  No 128-bit division: only 64-bit ones, which the compiler expands inline.
__device__ __forceinline__ void dec_avg(unsigned long long& lo, long long& hi, unsigned long long n) {
  const bool neg = hi < 0;
  unsigned long long ml = lo, mh = (unsigned long long)hi;
  if (neg) {
    ml = 0ull - lo;
    mh = ~mh + (lo == 0ull ? 1ull : 0ull);
  }
  const unsigned long long x[4] = {ml & 0xffffffffull, ml >> 32, mh & 0xffffffffull, mh >> 32};
  unsigned long long q[4], rem = 0;
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    const unsigned long long cur = (rem << 32) | x[i];
    q[i] = cur / n;
    rem = cur - q[i] * n;
  }
  unsigned long long carry = (2ull * rem * 10000ull + n) / (2ull * n);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned long long t = q[i] * 10000ull + carry;      // q[i] < 2^32: below 2^46
    q[i] = t & 0xffffffffull;
    carry = t >> 32;
  }
  ml = q[0] | (q[1] << 32);
  mh = q[2] | (q[3] << 32);
  if (neg) {
    mh = ~mh + (ml == 0ull ? 1ull : 0ull);
    ml = 0ull - ml;
  }
  lo = ml;
  hi = (long long)mh;
}

__global__ __launch_bounds__(256) void win_emit_kernel(const EmitArgs e, DictCols d) {
  const int32_t kept = e.scal[2];
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < kept; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = e.out_idx[p];
    for (int j = 0; j < d.ncols; ++j) {
      const DictCol& c = d.c[j];
      e.ovalid[j][p] = c.valid[g];
      if (c.kind == KC_STR) {
        e.okey[j][p] = g * kKeyWidth;
        e.olen[j][p] = c.lens[g];
      } else {
        e.okey[j][p] = ((const int64_t*)c.vals)[g];
      }
    }
    const long long* row = e.acc + g * e.stride;
    for (int r = 0; r < e.nreq; ++r) {
      const int k = e.kind[r];
      long long v = row[e.pos[r]];
      if (k & F_NOT) v = ~v;
      const double c = e.cnt[r] >= 0 ? __longlong_as_double(row[e.cnt[r]]) : 1.0;
      long long o;
      switch (k & F_KIND_MASK) {
        case F_COUNT: o = (long long)__longlong_as_double(v); break;
        case F_AVG: o = __double_as_longlong(__longlong_as_double(v) / (c > 1.0 ? c : 1.0)); break;
        case F_F64_ORD: o = v < 0 ? (v ^ 0x7fffffffffffffffll) : v; break;
        case F_VAR_SAMP:
        case F_VAR_POP: {
          // pos = the M2 word, cnt = the count word n: M2 / (n − 1) or M2 / n; Spark 2.4's sample statistic of
          // one row is NaN (n = 0 is NULL by the validity rule below)
          const bool samp = (k & F_KIND_MASK) == F_VAR_SAMP;
          const double den = samp ? c - 1.0 : c;
          double r = __longlong_as_double(v) / (den > 0.0 ? den : 1.0);
          if (samp && c == 1.0) r = __longlong_as_double(0x7ff8000000000000ll);
          if (k & F_SQRT) r = sqrt(r);
          o = __double_as_longlong(r);
          break;
        }
        case F_COVAR_POP: o = __double_as_longlong(__longlong_as_double(v) / (c > 1.0 ? c : 1.0)); break;
        case F_COVAR_SAMP: {
          double r = __longlong_as_double(v) / (c > 1.0 ? c - 1.0 : 1.0);
          if (!(c > 1.0)) r = __longlong_as_double(0x7ff8000000000000ll);
          o = __double_as_longlong(r);
          break;
        }
        case F_CORR: {
          const double p = __longlong_as_double(row[e.op2[r]]) * __longlong_as_double(row[e.op3[r]]);
          o = p > 0.0 ? __double_as_longlong(__longlong_as_double(v) / sqrt(p)) : 0x7ff8000000000000ll;
          break;
        }
        case F_SKEW: {
          const double m2 = __longlong_as_double(row[e.op2[r]]);
          o = m2 > 0.0 ? __double_as_longlong(sqrt(c) * __longlong_as_double(v) / (m2 * sqrt(m2)))
                       : 0x7ff8000000000000ll;
          break;
        }
        case F_KURT: {
          const double m2 = __longlong_as_double(row[e.op2[r]]);
          o = m2 > 0.0 ? __double_as_longlong(c * __longlong_as_double(v) / (m2 * m2) - 3.0) : 0x7ff8000000000000ll;
          break;
        }
        case F_DEC_SUM:
        case F_DEC_AVG: {
          unsigned long long lo;
          long long hi;
          dec_total((unsigned long long)row[e.pos[r]], (unsigned long long)row[e.op2[r]],
                    (unsigned long long)row[e.op3[r]], lo, hi);
          if ((k & F_KIND_MASK) == F_DEC_AVG) dec_avg(lo, hi, c > 1.0 ? (unsigned long long)c : 1ull);
          o = (k & F_HI) ? hi : (long long)lo;
          break;
        }
        case F_DEC_MM: {
          // v is the high word with MIN's complement undone; the low key: the complement, then the order mapping
          long long l = row[e.op2[r]];
          if (k & F_NOT) l = ~l;
          o = (k & F_HI) ? v : (l ^ (long long)0x8000000000000000ull);
          break;
        }
        case F_STRW: o = v ^ (long long)0x8000000000000000ull; break;
        default: o = v; break;
      }
      e.dst[(int64_t)r * e.gcap + p] = o;
      e.dvalid[(int64_t)r * e.gcap + p] = c > 0.0 ? 1 : 0;
    }
  }
}

// ---- dictionary rebuild (see dxa_win_live below): old group out_idx[p] becomes group p, p < live -----------------

// key columns: one thread per live group copies its entry of every column (a string slot is kKeyWidth / 8 words)
__global__ __launch_bounds__(256) void win_remap_dict_kernel(const DictCols src, const DictCols dst,
                                                             const int64_t* __restrict__ out_idx, int32_t live) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < live; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = out_idx[p];
    for (int j = 0; j < src.ncols; ++j) {
      const DictCol& a = src.c[j];
      const DictCol& b = dst.c[j];
      b.valid[p] = a.valid[g];
      if (a.kind == KC_STR) {
        const uint64_t* x = (const uint64_t*)((const uint8_t*)a.vals + g * kKeyWidth);
        uint64_t* y = (uint64_t*)((uint8_t*)b.vals + p * kKeyWidth);
        for (int q = 0; q < kKeyWidth / 8; ++q) y[q] = x[q];
        b.lens[p] = a.lens[g];
      } else {
        ((int64_t*)b.vals)[p] = ((const int64_t*)a.vals)[g];
      }
    }
  }
}

// one ring slot: dst row p = src row out_idx[p] for p < live, the accumulator identity (agg_multi_init_kernel's)
// for every other row up to and including the dump row — a group that draws one of those ids later has no rows in
// this pane.  ``src`` and ``dst`` are different slots; consecutive lanes move consecutive words of a row.
__global__ __launch_bounds__(256) void win_remap_slot_kernel(const unsigned long long* __restrict__ src,
                                                             unsigned long long* __restrict__ dst,
                                                             const int64_t* __restrict__ out_idx, int32_t live,
                                                             int32_t rows, int32_t stride,
                                                             const int32_t* __restrict__ line_op) {
  const int64_t total = (int64_t)rows * stride;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = idx / stride;
    const int w = (int)(idx - p * stride);
    const int op = line_op[w >> 3];
    // (MA_PICK_VAL words start at 0)
    const bool lowest = op == MA_MAX_I64 || op == MA_LOKEY || op == MA_PICK_RANK || op == MA_STRKEY;
    unsigned long long v = lowest ? 0x8000000000000000ull : 0ull;
    if (p < live) v = src[out_idx[p] * stride + w];
    dst[idx] = v;
  }
}

// a dictionary entry's key hash: equal to row_hash of the row that claimed it (the entry holds the row's key words
// — doubles already normalised — or its string bytes).  Recomputed here rather than kept per group at insert: the
// insert kernel is the hot one, and a [gcap + 1] hash array written by every claiming lane would cost it a store
// per new key and the ring 8 bytes per group for a value a rare rebuild can derive.
__device__ __forceinline__ uint64_t dict_hash(const DictCols& d, int64_t g) {
  uint64_t h = 0;
  for (int j = 0; j < d.ncols; ++j) {
    const DictCol& c = d.c[j];
    uint64_t x;
    if (!c.valid[g]) x = dxa::kNullHash;
    else if (c.kind == KC_STR) x = dxa::hash_bytes((const uint8_t*)c.vals + g * kKeyWidth, c.lens[g]);
    else x = dxa::hash_i64((uint64_t)((const int64_t*)c.vals)[g]);
    h = j ? dxa::hash_combine(h, x) : x;
  }
  return h;
}

// the table of the renumbered dictionary (cleared before): one thread per live group claims the first empty slot
// along its probe sequence and stores the id.  Live keys have distinct hashes (a duplicate raised the collision
// flag at insert), so nobody looks an entry up here and nothing waits: a lost CAS moves on to the next slot.
// Thread 0 publishes the new group count and clears the "dictionary full" flag (atomically: another lane may be
// raising the collision flag, which is never cleared).
__global__ __launch_bounds__(256) void win_rehash_kernel(const DictCols d, uint64_t* __restrict__ keys,
                                                         int64_t cap_mask, int32_t* __restrict__ gid_of_slot,
                                                         int32_t live, int32_t* __restrict__ scal) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    scal[0] = live;
    atomicAnd(&scal[1], ~2);
  }
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < live; g += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = dxa::fix_key(dict_hash(d, g));
    int64_t s = (int64_t)(dxa::fmix64(k) & (uint64_t)cap_mask);
    bool placed = false;
    for (int64_t probes = 0; probes <= cap_mask && !placed; ++probes) {
      const uint64_t prev = atomicCAS((unsigned long long*)&keys[s], (unsigned long long)dxa::kEmpty,
                                      (unsigned long long)k);
      if (prev == dxa::kEmpty) {
        gid_of_slot[s] = (int32_t)g;
        placed = true;
      } else if (prev == k) {
        break;                                             // two live groups with one hash: reported below
      }
      s = (s + 1) & cap_mask;
    }
    if (!placed) atomicOr(&scal[1], 1);
  }
}

// ---- COUNT(DISTINCT x) over the window: a distinct count is a count of live (group, x) pairs, and "live" is an OR
// over the window's panes.  Each distinct argument has a second persistent dictionary keyed by (parent group id, x)
// — filled by win_insert_kernel itself, with the outer insert's ids widened to int64 as key column 0 — and a
// presence ring of one byte per (ring slot, pair).  Bytes, not accumulator lines: at 2^20 pairs and ~320 slots the
// presence ring is ~335 MB where 64-byte lines would be over 20 GB.  count(DISTINCT a, b, …) has the key (parent
// group id, a, b, …); SUM / AVG(DISTINCT x) read x back from key column 1 of x's dictionary (PairFold::vals).

constexpr int kMaxPairStates = 4;
struct PairFold {
  const uint8_t* pres;     // [ring slots][pitch], pitch a multiple of 16
  int64_t pitch;
  const int64_t* parent;   // the pair dictionary's key column 0: each pair's group id
  const int32_t* pscal;    // the pair dictionary's counter and flags
  int32_t pcap;
  int32_t word;            // the count word of the combined row this distinct count is added into
  // SUM / AVG(DISTINCT x): the pair dictionary's key column 1 — every pair's x, int64 or the normalised bits of a
  // double (``vkind`` KC_I64 / KC_F64) — and the words of the combined row the live pairs' values are added into: an
  // MA_ADD_U64 word (the wrapping int64 sum) and an MA_ADD_F64 word (the sum as doubles); -1: absent.  Both absent
  // (a distinct count alone): ``vals`` is not read
  const int64_t* vals;
  int32_t vkind;
  int32_t isum;
  int32_t fsum;
  int32_t pad;
};
struct PairFolds {
  PairFold p[kMaxPairStates];
  int32_t n;
  int32_t pad;
};

// the pair insert's inputs from the outer insert's ids: column 0 (int64) and the row mask — rows the outer insert
// sent to the dump row (filtered by WHERE, or drawn past the capacity) and rows whose x is NULL create no pair
__global__ void win_pair_prep_kernel(const int32_t* __restrict__ gid, int64_t n, int32_t gcap,
                                     const uint8_t* __restrict__ xvalid, int64_t* __restrict__ gid64,
                                     uint8_t* __restrict__ keep) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t g = gid[i];
    gid64[i] = g;
    keep[i] = (g >= 0 && g < gcap && (!xvalid || xvalid[i])) ? 1 : 0;
  }
}

// a pane's pairs into its (zeroed) presence row: plain idempotent stores, no atomics
__global__ void win_pair_mark_kernel(const int32_t* __restrict__ pid, int64_t n, int32_t pcap,
                                     uint8_t* __restrict__ row) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t p = pid[i];
    if (p >= 0 && p < pcap) row[p] = 1;
  }
}

// a complete block's presence rows ORed into a block slot, 16 pairs per lane; the whole pitch is written, so pairs
// the dictionary gains later read 0 there
__global__ __launch_bounds__(256) void win_pair_or_kernel(const uint8_t* __restrict__ pres, int64_t pitch,
                                                          const int32_t* __restrict__ slots, int32_t nslots,
                                                          uint8_t* __restrict__ dst) {
  const int64_t chunks = pitch >> 4;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * blockDim.x) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    for (int s = 0; s < nslots; ++s) {
      const uint4 w = *(const uint4*)(pres + (int64_t)slots[s] * pitch + (c << 4));
      v.x |= w.x; v.y |= w.y; v.z |= w.z; v.w |= w.w;
    }
    *(uint4*)(dst + (c << 4)) = v;
  }
}

// the window's distinct counts into the combined rows (after win_combine, before win_keep / win_emit): a pair is
// live when any of the window's slots has its byte set; every live pair adds 1.0 to its parent's reserved count
// word, which win_emit's F_COUNT then finishes like any other count.  A lane owns 16 consecutive pairs (one 16-byte
// load per slot).  The adds are aggregated in the wave first — one atomic of the popcount per distinct parent per
// wave and pair position: the global form has every pair under one parent, and every adder on one row runs an order
// of magnitude below the float-atomic rate.  Counts are integers in f64, so the sums are exact in any order.
// kSums (SUM / AVG(DISTINCT x); a layout without them runs the other instantiation, which is the kernel as it was):
// a live pair's lane also loads the pair's x from the dictionary's value column — never for a pair that is not live —
// and, in the same leader loop, the values of the parent's members are reduced over the wave (the other lanes
// contribute 0 to a full-wave xor tree), so the leader issues one atomic per word beside the count's: an unsigned
// 64-bit add into the integer word (wrapping, order-free) and an f64 add into the double word (the sum's last bits
// depend on the arrival order, as every f64 atomic sum's do).  Values come from the dictionary: -0.0 is stored as
// 0.0 and every NaN as the canonical one.
template <bool kSums>
__global__ __launch_bounds__(256) void win_distinct_fold_kernel(const PairFold f, const int32_t* __restrict__ slots,
                                                                int32_t nslots, const int32_t* __restrict__ scal,
                                                                int32_t gcap, double* __restrict__ acc,
                                                                int32_t stride) {
  int32_t ng = scal[0];
  if (ng > gcap) ng = gcap;
  int32_t np = f.pscal[0];
  if (np > f.pcap) np = f.pcap;
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  // c0: the wave's first chunk, so the loop (and the ballots in it) is wave-uniform
  for (int64_t c0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; c0 * 16 < np; c0 += step) {
    const int64_t p0 = (c0 + lane) * 16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (p0 < np) {
      for (int s = 0; s < nslots; ++s) {
        const uint4 v = *(const uint4*)(f.pres + (int64_t)slots[s] * f.pitch + p0);
        w[0] |= v.x; w[1] |= v.y; w[2] |= v.z; w[3] |= v.w;
      }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const bool on = p0 + q < np && ((w[q >> 2] >> (8 * (q & 3))) & 0xffu) != 0u;
      const int64_t par = on ? f.parent[p0 + q] : -1;
      const bool active = on && par >= 0 && par < ng;
      const int32_t mine = active ? (int32_t)par : -1;
      unsigned long long xi = 0ull;
      double xd = 0.0;
      if (kSums && active) {
        const int64_t b = f.vals[p0 + q];
        xi = (unsigned long long)b;
        xd = f.vkind == KC_F64 ? __longlong_as_double(b) : (double)b;
      }
      unsigned long long todo = __ballot(active);
      while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int32_t first = __shfl(mine, lead);
        const bool member = active && mine == first;
        const unsigned long long same = __ballot(member);
        double* row = acc + (int64_t)first * stride;
        if (lane == lead) atomicAdd(row + f.word, (double)__popcll(same));
        if (kSums) {
          // (a parent with one member in this ballot — the usual case with many groups — needs no tree: ``same`` is
          // wave-uniform, so is the branch)
          const bool alone = (same & (same - 1)) == 0ull;
          if (f.isum >= 0) {
            unsigned long long si = member ? xi : 0ull;
            if (!alone)
              for (int o = 32; o; o >>= 1) si += __shfl_xor(si, o);
            if (lane == lead) atomicAdd((unsigned long long*)row + f.isum, si);
          }
          if (f.fsum >= 0) {
            double sd = member ? xd : 0.0;
            if (!alone)
              for (int o = 32; o; o >>= 1) sd += __shfl_xor(sd, o);
            if (lane == lead) atomicAdd(row + f.fsum, sd);
          }
        }
        todo &= ~same;
      }
    }
  }
}

}  // namespace

DXA_API int dxa_win_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(KeyCols);
  out[1] = (int32_t)sizeof(DictCols);
  out[2] = kKeyWidth;
  return 0;
}

// table init (once per dictionary): keys = empty, gid_of_slot = -1
DXA_API int dxa_win_init(uint64_t* keys, int32_t* gid_of_slot, int64_t cap, void* st) {
  hipStream_t s = (hipStream_t)st;
  hipMemsetAsync(keys, 0xFF, (size_t)cap * 8, s);
  hipMemsetAsync(gid_of_slot, 0xFF, (size_t)cap * 4, s);
  return (int)hipGetLastError();
}

// ---- the combine and the window's answer: one entry point each, for every layout ---------------------------------
// A layout with MA_M2 lines passes ``m2desc`` [stride] on the device (win_combine_kernel) and ``m2desc_host``, the same
// words for the bounds check here; one with MA_MOM lines also ``momdesc`` / ``momdesc_host``, and then ``m2desc`` is
// required too (all zero without M2 lines).  A layout without such lines passes null for both pairs.  A layout with
// MA_LOKEY lines passes ``lodesc`` / ``lodesc_host`` the same way, independently of the other two, and one with
// MA_PICK_RANK / MA_PICK_VAL lines ``pickdesc`` / ``pickdesc_host``, independently again.

static bool m2desc_ok(const int32_t* host_desc, int32_t stride) {
  for (int w = 0; w < stride; ++w) {
    const int32_t d = host_desc[w];
    if (d < 0 || (d & 0xffff) >= stride || (d >> 16) >= stride) return false;
  }
  return true;
}

// (the word indices are 6-bit fields: no layout of more than 64 words can have MA_MOM lines)
static bool momdesc_ok(const int32_t* host_desc, int32_t stride) {
  if (stride > 64) return false;
  for (int w = 0; w < stride; ++w) {
    const int32_t d = host_desc[w];
    if (d < 0 || (d >> 24) > MOM_CXY) return false;
    if (!d) continue;
    for (int q = 0; q < 24; q += 6)
      if (((d >> q) & 63) >= stride) return false;
  }
  return true;
}

static bool lodesc_ok(const int32_t* host_desc, int32_t stride) {
  for (int w = 0; w < stride; ++w) {
    const int32_t d = host_desc[w];
    if (d && ((d >> 16) != 1 || (d & 0xffff) >= stride)) return false;
  }
  return true;
}

// (the word indices are 8-bit fields: R, then K + 1 or 0; bit 16 "last", bit 17 "in use")
static bool pickdesc_ok(const int32_t* host_desc, int32_t stride) {
  if (stride > 255) return false;
  for (int w = 0; w < stride; ++w) {
    const int32_t d = host_desc[w];
    if (d && ((d >> 17) != 1 || (d & 0xff) >= stride || ((d >> 8) & 0xff) > stride)) return false;
  }
  return true;
}

// (per word its place in the line's tuple + 1, so word w of a line holds (w & 7) + 1; 0: spare or unused)
static bool strdesc_ok(const int32_t* host_desc, int32_t stride) {
  for (int w = 0; w < stride; ++w) {
    const int32_t d = host_desc[w];
    if (d && (d != (w & 7) + 1 || d > 7)) return false;
  }
  return true;
}

static bool descs_ok(const int32_t* m2desc, const int32_t* m2desc_host, const int32_t* momdesc,
                     const int32_t* momdesc_host, const int32_t* lodesc, const int32_t* lodesc_host,
                     const int32_t* pickdesc, const int32_t* pickdesc_host, const int32_t* strdesc,
                     const int32_t* strdesc_host, int32_t stride) {
  if (!m2desc != !m2desc_host || !momdesc != !momdesc_host || (momdesc && !m2desc) || !lodesc != !lodesc_host ||
      !pickdesc != !pickdesc_host || !strdesc != !strdesc_host)
    return false;
  return (!m2desc || m2desc_ok(m2desc_host, stride)) && (!momdesc || momdesc_ok(momdesc_host, stride)) &&
         (!lodesc || lodesc_ok(lodesc_host, stride)) && (!pickdesc || pickdesc_ok(pickdesc_host, stride)) &&
         (!strdesc || strdesc_ok(strdesc_host, stride));
}

static bool folds_ok(const PairFolds* pf, int32_t stride) {
  if (!pf) return true;
  if (pf->n < 0 || pf->n > kMaxPairStates) return false;
  for (int k = 0; k < pf->n; ++k) {
    const PairFold& f = pf->p[k];
    if (f.word < 0 || f.word >= stride || (f.pitch & 15) || f.pitch < (int64_t)f.pcap + 1) return false;
    if (f.isum < -1 || f.isum >= stride || f.fsum < -1 || f.fsum >= stride) return false;
    if ((f.isum >= 0 || f.fsum >= 0) && (!f.vals || (f.vkind != KC_I64 && f.vkind != KC_F64))) return false;
  }
  return true;
}

// the further operand words of the kinds above F_SQRT and of F_DEC_MM (no other kind reads op2 / op3)
static bool emit_ok(const EmitArgs& ea, int32_t stride) {
  for (int r = 0; r < ea.nreq && r < kMaxEmit; ++r) {
    const int k = ea.kind[r] & F_KIND_MASK;
    if (k >= F_CORR && (ea.op2[r] < 0 || ea.op2[r] >= stride)) return false;
    if ((k == F_CORR || k >= F_DEC_SUM) && (ea.op3[r] < 0 || ea.op3[r] >= stride)) return false;
    if (k == F_DEC_MM && (ea.op2[r] < 0 || ea.op2[r] >= stride)) return false;
  }
  return true;
}

// The combine of ``slots`` into ``out`` with the instantiation the (checked) descriptors call for: the per-batch form
// over the groups in use, or (kBlock) the block form that writes all gcap + 1 rows.
template <bool kBlock, bool kKey, bool kPick, bool kStr>
static void launch_combine_as(const unsigned long long* ring, int32_t gcap, int32_t stride, const int32_t* slots,
                              int32_t nslots, const int32_t* line_op, const int32_t* scal, unsigned long long* out,
                              const int32_t* m2desc, const int32_t* momdesc, const int32_t* lodesc,
                              const int32_t* pickdesc, const int32_t* strdesc, hipStream_t s) {
  const int32_t rows = kBlock ? gcap + 1 : gcap;
  auto kernel = momdesc  ? win_combine_kernel<kBlock, true, true, kKey, kPick, kStr>
                : m2desc ? win_combine_kernel<kBlock, true, false, kKey, kPick, kStr>
                         : win_combine_kernel<kBlock, false, false, kKey, kPick, kStr>;
  hipLaunchKernelGGL(kernel, dim3(dxa_blocks((int64_t)rows * stride, 256, 256 * 64)), dim3(256), 0, s, ring,
                     (int64_t)(gcap + 1) * stride, slots, nslots, stride, line_op, scal, gcap, kBlock ? rows : 0, out,
                     m2desc, momdesc, lodesc, pickdesc, strdesc);
}

// one instantiation per combination of descriptors present: a layout without a family runs the combine without
// that family's branch
template <bool kBlock>
static void launch_combine(const unsigned long long* ring, int32_t gcap, int32_t stride, const int32_t* slots,
                           int32_t nslots, const int32_t* line_op, const int32_t* scal, unsigned long long* out,
                           const int32_t* m2desc, const int32_t* momdesc, const int32_t* lodesc,
                           const int32_t* pickdesc, const int32_t* strdesc, hipStream_t s) {
  auto plain = launch_combine_as<kBlock, false, false, false>, keyed = launch_combine_as<kBlock, true, false, false>,
       pick_plain = launch_combine_as<kBlock, false, true, false>,
       pick_keyed = launch_combine_as<kBlock, true, true, false>,
       str_plain = launch_combine_as<kBlock, false, false, true>,
       str_keyed = launch_combine_as<kBlock, true, false, true>,
       str_pick_plain = launch_combine_as<kBlock, false, true, true>,
       str_pick_keyed = launch_combine_as<kBlock, true, true, true>;
  auto launch = strdesc ? (pickdesc ? (lodesc ? str_pick_keyed : str_pick_plain) : (lodesc ? str_keyed : str_plain))
                        : (pickdesc ? (lodesc ? pick_keyed : pick_plain) : (lodesc ? keyed : plain));
  launch(ring, gcap, stride, slots, nslots, line_op, scal, out, m2desc, momdesc, lodesc, pickdesc, strdesc, s);
}

// a block of ring slots pre-combined into another ring slot (every row is written, so groups the dictionary gains
// later read the identity there; the members are read only for the scal[0] groups in use): out = ring slot ``dst``
DXA_API int dxa_win_combine_block(void* ring, int32_t gcap, int32_t stride, const int32_t* slots, int32_t nslots,
                                  const int32_t* line_op, int32_t dst, const int32_t* scal, const int32_t* m2desc,
                                  const int32_t* m2desc_host, const int32_t* momdesc, const int32_t* momdesc_host,
                                  const int32_t* lodesc, const int32_t* lodesc_host, const int32_t* pickdesc,
                                  const int32_t* pickdesc_host, const int32_t* strdesc, const int32_t* strdesc_host,
                                  void* st) {
  if (!descs_ok(m2desc, m2desc_host, momdesc, momdesc_host, lodesc, lodesc_host, pickdesc, pickdesc_host, strdesc,
                strdesc_host, stride))
    return (int)hipErrorInvalidValue;
  unsigned long long* r = (unsigned long long*)ring;
  launch_combine<true>(r, gcap, stride, slots, nslots, line_op, scal, r + (int64_t)dst * (gcap + 1) * stride, m2desc,
                       momdesc, lodesc, pickdesc, strdesc, (hipStream_t)st);
  return (int)hipGetLastError();
}

// The window's answer: ring [R][(gcap+1)*stride] u64, slots [nslots] (device) → acc [(gcap+1)*stride] the combined
// rows, keep [gcap] scratch, out_idx [gcap] (the first scal[2] entries are the kept groups, in group order).
// Steps 5-6: the combine, one distinct fold per pair state of ``folds`` (may be null) into the combined rows, keep,
// compaction, and — unless ``emit`` is null — the output rows by position (win_emit_kernel).
DXA_API int dxa_win_answer(const void* ring, int32_t gcap, int32_t stride, const int32_t* slots, int32_t nslots,
                           const int32_t* line_op, int32_t count_word, int32_t* scal, void* acc, uint8_t* keep,
                           int64_t* out_idx, const void* emit, const void* dictcols, const void* folds,
                           const int32_t* m2desc, const int32_t* m2desc_host, const int32_t* momdesc,
                           const int32_t* momdesc_host, const int32_t* lodesc, const int32_t* lodesc_host,
                           const int32_t* pickdesc, const int32_t* pickdesc_host, const int32_t* strdesc,
                           const int32_t* strdesc_host, void* st) {
  hipStream_t s = (hipStream_t)st;
  const EmitArgs* ea = (const EmitArgs*)emit;
  const PairFolds* pf = (const PairFolds*)folds;
  if (!descs_ok(m2desc, m2desc_host, momdesc, momdesc_host, lodesc, lodesc_host, pickdesc, pickdesc_host, strdesc,
                strdesc_host, stride) ||
      !folds_ok(pf, stride) || (ea && (!dictcols || !emit_ok(*ea, stride))))
    return (int)hipErrorInvalidValue;
  hipMemsetAsync(scal + 2, 0, 4, s);
  launch_combine<false>((const unsigned long long*)ring, gcap, stride, slots, nslots, line_op, scal,
                        (unsigned long long*)acc, m2desc, momdesc, lodesc, pickdesc, strdesc, s);
  for (int k = 0; pf && k < pf->n; ++k) {
    auto fold = pf->p[k].isum >= 0 || pf->p[k].fsum >= 0 ? win_distinct_fold_kernel<true>
                                                         : win_distinct_fold_kernel<false>;
    hipLaunchKernelGGL(fold, dim3(dxa_blocks(((int64_t)pf->p[k].pcap + 15) >> 4, 256, 256 * 8)), dim3(256), 0, s,
                       pf->p[k], slots, nslots, scal, gcap, (double*)acc, stride);
  }
  hipLaunchKernelGGL(win_keep_kernel, dim3(dxa_blocks(gcap, 256)), dim3(256), 0, s,
                     (const unsigned long long*)acc, stride, count_word, scal, gcap, keep, scal);
  hipLaunchKernelGGL(win_compact_kernel, dim3(1), dim3(256), 0, s, keep, gcap, scal, out_idx);
  if (ea) hipLaunchKernelGGL(win_emit_kernel, dim3(dxa_blocks(gcap, 256)), dim3(256), 0, s, *ea,
                             *(const DictCols*)dictcols);
  return (int)hipGetLastError();
}

// ---- dictionary rebuild: when the group counter passes the capacity the host drops the panes accumulated since the
// last clean status, finds the groups that still have rows in the panes it holds (dxa_win_live), and renumbers them
// densely: old id out_idx[p] becomes p, p < live.  Off the hot path (once per ~capacity / 2 new keys at the least).

// The live groups of the given pane slots: the answer's combine, keep and compact passes over those slots, without
// descriptors whatever the layout (only the combined count word is read afterwards) and without output rows →
// out_idx[0 .. scal[2]) = the old ids with COUNT(*) > 0 there, increasing.
DXA_API int dxa_win_live(const void* ring, int32_t gcap, int32_t stride, const int32_t* slots, int32_t nslots,
                         const int32_t* line_op, int32_t count_word, int32_t* scal, void* acc, uint8_t* keep,
                         int64_t* out_idx, void* st) {
  return dxa_win_answer(ring, gcap, stride, slots, nslots, line_op, count_word, scal, acc, keep, out_idx, nullptr,
                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, st);
}

// The dictionary's key columns into fresh ones (``dst`` is zero-filled; earlier batches' output strings are views of
// the old arena and may still be rendering, so nothing moves in place).
DXA_API int dxa_win_remap_dict(const void* src, const void* dst, const int64_t* out_idx, int32_t live, void* st) {
  const DictCols& a = *(const DictCols*)src;
  const DictCols& b = *(const DictCols*)dst;
  if (live < 0 || live > a.gcap || live > b.gcap || a.ncols != b.ncols) return (int)hipErrorInvalidValue;
  if (live == 0) return 0;
  hipLaunchKernelGGL(win_remap_dict_kernel, dim3(dxa_blocks(live, 256)), dim3(256), 0, (hipStream_t)st, a, b, out_idx,
                     live);
  return (int)hipGetLastError();
}

// The pane slots ``slots`` (a HOST array) of ``src`` [.][(gcap_src + 1) * stride] into the same slots of ``dst``
// [.][(gcap_dst + 1) * stride].  A grown ring is a new allocation and each slot is gathered straight into it.  With
// src == dst (capacity unchanged) each slot is gathered into ``tmp_slot`` — a slot of the ring whose contents are
// dead during a rebuild (the host passes a scratch slot: those are refilled every batch) — and copied back, so the
// in-place form needs no extra memory and has no cross-thread hazard.
DXA_API int dxa_win_remap_ring(const void* src, void* dst, int32_t gcap_src, int32_t gcap_dst, int32_t stride,
                               const int32_t* slots, int32_t nslots, int32_t tmp_slot, const int32_t* line_op,
                               const int64_t* out_idx, int32_t live, void* st) {
  hipStream_t s = (hipStream_t)st;
  const bool in_place = src == dst;
  if (live < 0 || live > gcap_src || live > gcap_dst || (in_place && gcap_src != gcap_dst))
    return (int)hipErrorInvalidValue;
  const int64_t src_words = (int64_t)(gcap_src + 1) * stride, dst_words = (int64_t)(gcap_dst + 1) * stride;
  const unsigned long long* from = (const unsigned long long*)src;
  unsigned long long* to = (unsigned long long*)dst;
  for (int32_t k = 0; k < nslots; ++k) {
    if (in_place && slots[k] == tmp_slot) return (int)hipErrorInvalidValue;
    unsigned long long* out = to + (int64_t)(in_place ? tmp_slot : slots[k]) * dst_words;
    hipLaunchKernelGGL(win_remap_slot_kernel, dim3(dxa_blocks(dst_words, 256, 256 * 64)), dim3(256), 0, s,
                       from + (int64_t)slots[k] * src_words, out, out_idx, live, gcap_dst + 1, stride, line_op);
    if (in_place) hipMemcpyAsync(to + (int64_t)slots[k] * dst_words, out, (size_t)dst_words * 8,
                                 hipMemcpyDeviceToDevice, s);
  }
  return (int)hipGetLastError();
}

// The hash table of the renumbered dictionary: cleared as dxa_win_init clears it, then every live group's hash goes
// back in; the same launch sets the group counter to ``live`` and clears the "dictionary full" flag.
DXA_API int dxa_win_rehash(const void* dictcols, uint64_t* keys, int32_t* gid_of_slot, int64_t cap, int32_t live,
                           int32_t* scal, void* st) {
  const DictCols& d = *(const DictCols*)dictcols;
  if (live < 0 || live > d.gcap || cap < 2 * (int64_t)d.gcap || (cap & (cap - 1))) return (int)hipErrorInvalidValue;
  const int rc = dxa_win_init(keys, gid_of_slot, cap, st);
  if (rc) return rc;
  hipLaunchKernelGGL(win_rehash_kernel, dim3(dxa_blocks(live, 256)), dim3(256), 0, (hipStream_t)st, d, keys, cap - 1,
                     gid_of_slot, live, scal);
  return (int)hipGetLastError();
}

DXA_API int dxa_win_emit_size() { return (int)sizeof(EmitArgs); }

// one pane into the dictionary (fused hash + lookup / claim + key store + verify)
DXA_API int dxa_win_insert_fused(const void* keycols, const void* dictcols, const uint8_t* keep, uint64_t* keys,
                                 int64_t cap, int32_t* gid_of_slot, int32_t* scal, int32_t* gid, void* st) {
  const KeyCols& a = *(const KeyCols*)keycols;
  if (a.n <= 0) return 0;
  hipLaunchKernelGGL(win_insert_kernel, dim3(dxa_blocks(a.n, 256)), dim3(256), 0, (hipStream_t)st, a,
                     *(const DictCols*)dictcols, keep, keys, cap - 1, gid_of_slot, scal, gid);
  return (int)hipGetLastError();
}

// ---- COUNT(DISTINCT x): entry points (the folds themselves are launched by dxa_win_answer) ------------------------

DXA_API int dxa_win_pairfold_size() { return (int)sizeof(PairFolds); }

// column 0 and the row mask of a pane's pair insert (win_pair_prep_kernel)
DXA_API int dxa_win_pair_prep(const int32_t* gid, int64_t n, int32_t gcap, const uint8_t* xvalid, int64_t* gid64,
                              uint8_t* keep, void* st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(win_pair_prep_kernel, dim3(dxa_blocks(n, 256)), dim3(256), 0, (hipStream_t)st, gid, n, gcap,
                     xvalid, gid64, keep);
  return (int)hipGetLastError();
}

// a pane entering ring slot ``slot``: the slot's presence row is zeroed, then every row's pair id is marked
DXA_API int dxa_win_pair_mark(const int32_t* pid, int64_t n, int32_t pcap, uint8_t* pres, int64_t pitch, int32_t slot,
                              void* st) {
  hipStream_t s = (hipStream_t)st;
  if (pitch < (int64_t)pcap + 1 || (pitch & 15) || slot < 0) return (int)hipErrorInvalidValue;
  uint8_t* row = pres + (int64_t)slot * pitch;
  hipMemsetAsync(row, 0, (size_t)pitch, s);
  if (n > 0)
    hipLaunchKernelGGL(win_pair_mark_kernel, dim3(dxa_blocks(n, 256)), dim3(256), 0, s, pid, n, pcap, row);
  return (int)hipGetLastError();
}

// a block of presence rows ORed into slot ``dst`` (not a member), as dxa_win_combine_block does for accumulators
DXA_API int dxa_win_pair_or_block(uint8_t* pres, int64_t pitch, const int32_t* slots, int32_t nslots, int32_t dst,
                                  void* st) {
  if ((pitch & 15) || dst < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(win_pair_or_kernel, dim3(dxa_blocks(pitch >> 4, 256, 256 * 64)), dim3(256), 0, (hipStream_t)st,
                     (const uint8_t*)pres, pitch, slots, nslots, pres + (int64_t)dst * pitch);
  return (int)hipGetLastError();
}

// ---- STDDEV / VARIANCE: the pane's second pass (the combine is dxa_win_answer's and dxa_win_combine_block's) -------

DXA_API int dxa_win_m2_size() { return (int)sizeof(M2Args); }

// ids below this go through LDS in win_m2_kernel and the other second passes (dxa::kLdsGroupIds: str_minmax.hip's
// bound too), the others straight to global memory
DXA_API int dxa_win_m2_lds_groups() { return kM2LdsGroups; }

// a pane's M2 words, on the same stream right after dxa_aggregate_multi filled the slot (win_m2_kernel)
DXA_API int dxa_win_m2(const void* args, void* st) {
  const M2Args& m = *(const M2Args*)args;
  if (m.nargs < 0 || m.nargs > kMaxM2Args || m.gcap < 0 || m.stride <= 0) return (int)hipErrorInvalidValue;
  for (int k = 0; k < m.nargs; ++k) {
    const M2Arg& a = m.a[k];
    if (a.cnt < 0 || a.cnt >= m.stride || a.sum < 0 || a.sum >= m.stride || a.m2 < 0 || a.m2 >= m.stride || !a.x)
      return (int)hipErrorInvalidValue;
  }
  if (m.n <= 0 || m.nargs == 0) return 0;
  // 8 rows per lane amortise a workgroup's LDS clear and flush; at most two workgroups per CU's worth of adders
  hipLaunchKernelGGL(win_m2_kernel, dim3(dxa_blocks((m.n + 7) / 8, 256, 512)), dim3(256), 0, (hipStream_t)st, m);
  return (int)hipGetLastError();
}

// ---- CORR / COVAR / SKEWNESS / KURTOSIS: the pane's moment pass -----------------------------------------------------

DXA_API int dxa_win_mom_size() { return (int)sizeof(MomArgs); }

// a pane's M3 / M4 / Cxy words, on the same stream after dxa_aggregate_multi filled the slot (win_mom_kernel)
DXA_API int dxa_win_mom(const void* args, void* st) {
  const MomArgs& m = *(const MomArgs*)args;
  if (m.nargs < 0 || m.nargs > kMaxMomArgs || m.gcap < 0 || m.stride <= 0) return (int)hipErrorInvalidValue;
  for (int k = 0; k < m.nargs; ++k) {
    const MomArg& a = m.a[k];
    if (a.cnt < 0 || a.cnt >= m.stride || a.sum < 0 || a.sum >= m.stride || a.w0 < 0 || a.w0 >= m.stride ||
        a.w1 >= m.stride || !a.x || (a.y && (a.sumy < 0 || a.sumy >= m.stride || a.w1 >= 0)))
      return (int)hipErrorInvalidValue;
  }
  if (m.n <= 0 || m.nargs == 0) return 0;
  hipLaunchKernelGGL(win_mom_kernel, dim3(dxa_blocks((m.n + 7) / 8, 256, 512)), dim3(256), 0, (hipStream_t)st, m);
  return (int)hipGetLastError();
}

// ---- decimal SUM / AVG / two-lane MIN / MAX: the pane's decimal pass -------------------------------------------------

DXA_API int dxa_win_dec_size() { return (int)sizeof(DecArgs); }

// a pane's limb sums and low key words, on the same stream after dxa_aggregate_multi filled the slot (win_dec_kernel)
DXA_API int dxa_win_dec(const void* args, void* st) {
  const DecArgs& m = *(const DecArgs*)args;
  if (m.nargs < 0 || m.nargs > kMaxDecJobs || m.gcap < 0 || m.stride <= 0) return (int)hipErrorInvalidValue;
  for (int k = 0; k < m.nargs; ++k) {
    const DecJob& a = m.a[k];
    if (!a.x || (a.lanes != 1 && a.lanes != 2) || a.kind < DEC_SUM || a.kind > DEC_KEY_MIN || a.w0 < 0 ||
        a.w0 >= m.stride || a.w1 < 0 || a.w1 >= m.stride)
      return (int)hipErrorInvalidValue;
    if (a.kind == DEC_SUM ? (a.w2 < 0 || a.w2 >= m.stride) : a.lanes != 2) return (int)hipErrorInvalidValue;
  }
  if (m.n <= 0 || m.nargs == 0) return 0;
  hipLaunchKernelGGL(win_dec_kernel, dim3(dxa_blocks((m.n + 7) / 8, 256, 512)), dim3(256), 0, (hipStream_t)st, m);
  return (int)hipGetLastError();
}

// ---- MIN / MAX over strings: the pane's string pass ---------------------------------------------------------------

extern "C" int dxa_str_argext(const int32_t* gid, int64_t n, int32_t ngroups, const uint8_t* arena,
                              const int64_t* starts, const int32_t* lens, const uint8_t* valid, const uint8_t* keep,
                              int32_t dir, int64_t* best, void* st);       // str_minmax.hip

DXA_API int dxa_win_strkey_size() { return (int)sizeof(StrKeyArgs); }

// a pane's string order keys, on the same stream after dxa_aggregate_multi initialised the slot: per job the winning
// row per group (str_minmax.hip), then every job's packed words in one gather launch (win_strkey_gather_kernel)
DXA_API int dxa_win_strkey(const void* args, void* st) {
  const StrKeyArgs& m = *(const StrKeyArgs*)args;
  if (m.njobs < 1 || m.njobs > kMaxStrJobs || m.gcap < 0 || m.stride <= 0 || !m.gid || !m.row || !m.scal || !m.best)
    return (int)hipErrorInvalidValue;
  for (int k = 0; k < m.njobs; ++k) {
    const StrJob& a = m.a[k];
    if (!a.starts || !a.lens || a.line < 0 || (a.line & 7) || a.line + 8 > m.stride || (a.min != 0 && a.min != 1))
      return (int)hipErrorInvalidValue;
  }
  if (m.n <= 0) return 0;
  for (int k = 0; k < m.njobs; ++k) {
    const StrJob& a = m.a[k];
    const int rc = dxa_str_argext(m.gid, m.n, m.gcap, a.arena, a.starts, a.lens, a.valid, m.keep, a.min ? 0 : 1,
                                  m.best + (int64_t)k * m.gcap, st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(win_strkey_gather_kernel, dim3(dxa_blocks(m.gcap, 256, 1024)), dim3(256), 0, (hipStream_t)st, m);
  return (int)hipGetLastError();
}

// ---- first / last / max_by / min_by: the pane's pick pass -----------------------------------------------------------

DXA_API int dxa_win_pick_size() { return (int)sizeof(PickArgs); }

// a pane's rank words, then its payload and validity words, on the same stream after dxa_aggregate_multi filled the
// slot's key words (win_pick_kernel, win_pick_gather_kernel)
DXA_API int dxa_win_pick(const void* args, void* st) {
  const PickArgs& m = *(const PickArgs*)args;
  if (m.nrank < 1 || m.nrank > kMaxPickJobs || m.nval < 1 || m.nval > kMaxPickJobs || m.gcap < 0 || m.stride <= 0 ||
      !m.gid || !m.row || !m.scal)
    return (int)hipErrorInvalidValue;
  for (int k = 0; k < m.nrank; ++k) {
    const PickRank& a = m.rank[k];
    if (a.r < 0 || a.r >= m.stride || (a.last != 0 && a.last != 1)) return (int)hipErrorInvalidValue;
    if (a.y && (a.k < 0 || a.k >= m.stride || a.k == a.r || ((a.kind & 3) != 1 && (a.kind & 3) != 3) || (a.kind & ~7)))
      return (int)hipErrorInvalidValue;
  }
  for (int k = 0; k < m.nval; ++k) {
    const PickVal& a = m.val[k];
    if (!a.x || a.r < 0 || a.r >= m.stride || a.p < 0 || a.p >= m.stride || a.v < 0 || a.v >= m.stride ||
        a.p == a.v || a.p == a.r || a.v == a.r || (a.last != 0 && a.last != 1))
      return (int)hipErrorInvalidValue;
  }
  if (m.n <= 0) return 0;
  hipStream_t s = (hipStream_t)st;
  hipLaunchKernelGGL(win_pick_kernel, dim3(dxa_blocks((m.n + 7) / 8, 256, 512)), dim3(256), 0, s, m);
  hipLaunchKernelGGL(win_pick_gather_kernel, dim3(dxa_blocks(m.gcap, 256, 1024)), dim3(256), 0, s, m);
  return (int)hipGetLastError();
}
