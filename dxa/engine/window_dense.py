"""Dense sliding-window GROUP BY: a persistent device group dictionary + a ring of per-pane accumulator rows
(``dxa/ops/csrc/window_ring.hip``).

The reference answers a windowed statement by unioning the retained batches and running the GROUP BY over the union
every batch (DataProcessing/datax-host/src/main/scala/datax/processor/CommonProcessorFactory.scala:156-236).  The
paned path (``query._paned_aggregate``) already avoids re-reading the rows by caching per-pane partial tables, but
it still concatenates ~40 partial tables and re-groups them every batch — host-side work that kept the 300-pane
window flow host-bound.  Here the state a window needs lives in HBM in the shape the merge wants:

* a **group dictionary** (open-addressed table of key hashes → dense group id, plus each group's key values in
  fixed-width columns) that persists from batch to batch — a key seen once keeps its id for the life of the stream;
* a **ring** of accumulator rows ``[ring slot][group][stride]`` (the fused multi-aggregate's layout), one slot per
  retained pane; a pane is aggregated into its slot once, when it first enters a window;
* per batch, one kernel combines the window's slots per (group, word), flags the groups with rows in the window and
  compacts them; the host reads one 12-byte status (groups, collisions, output rows) — the statement's only
  synchronisation — and builds the output columns as views of the dictionary and the finished aggregates.

Eligible: GROUP BY statements whose aggregates are COUNT / SUM / MIN / MAX / AVG over numeric (decimals
included, below), boolean or timestamp arguments (and COUNT / SUM / AVG(DISTINCT x), count(DISTINCT a, b, …) and
approx_count_distinct, the variance family and corr / covar_pop /
covar_samp / skewness / kurtosis, below; count_if; bool_and / every, bool_or / any / some; first / last / max_by /
min_by, below), with plain key columns,
deterministic, on a GPU.  With N ranks each rank's window
comes out of its ring as a partial table of ``distagg.local_partials``' layout and goes through the same key
exchange and merge as the paned path (``dense_partials``).  Anything else — and any batch whose dictionary
reports a hash collision or an over-long string key — is answered by the paned path, which stays the reference
implementation (tests compare both).

**A full dictionary is rebuilt, not abandoned** (``DenseWindow.rebuild``).  The dictionary starts at ``DENSE_GROUPS``
ids.  When the group counter passes the capacity, the panes accumulated since the last clean status are dropped from
the ring (some of their rows went to the dump row), the groups that still have rows in the panes the ring holds are
found on the device, renumbered densely — key columns into fresh tensors, every held pane slot, the hash table — and
the dropped panes are accumulated again; when more than half the capacity is still live the capacity doubles, up to
``DENSE_GROUPS_MAX``.  So a stream whose keys come and go stays on this path; only a window that really holds more
than ``DENSE_GROUPS_MAX`` groups at once (or whose grown ring would not fit in memory) falls back for good.  A stream
whose live set sits just under ``DENSE_GROUPS_MAX`` rebuilds as often as a few new keys arrive: accepted, and counted
in ``DenseWindow.rebuilds``.  A rebuild is local to a rank and issues no collective: with N ranks a rank that
rebuilds (or falls back) still hands ``dense_partials``' caller a partial table or None, and the caller's exchange is
the same either way, so the ranks stay in step.

**COUNT(DISTINCT x)** (one argument, any key-column type the dictionary holds; up to ``MAX_DISTINCT`` different
arguments per statement) is a count of live (group, x) pairs, and "live" is an OR over the window's panes — the
shape the ring already keeps for groups.  Each distinct argument has a ``PairState``: a second persistent dictionary
keyed by (group id, x) — filled by the same insert kernel, with the ids the group insert just drew as key column 0;
rows sent to the dump row and rows whose x is NULL are masked out — and a presence ring ``uint8 [ring slot][pair]``:
a pane entering a slot zeroes the slot's row and stores 1 for each of its pairs; complete blocks are ORed into the
block slot the accumulators use.  Per batch ``win_distinct_fold_kernel`` runs between the combine and the keep
pass: it ORs the window's slots per pair and adds the live pairs into a count word of their group's combined row
that no pane accumulates into, so the emit kernel finishes it like any count.  The pair statuses (counter, flags)
travel in the same tensor as the group status: still one read per batch.  When either kind of dictionary is full
the dirty panes are dropped from both rings; a full group dictionary is renumbered as above and every pair state
after it (its column 0 mapped old id → new id; a live pair has rows in a held pane, so its group is live too), a
full pair dictionary alone is rebuilt over the pairs with a byte set in a held pane slot and grows by the same
policy between ``DENSE_PAIRS`` and ``DENSE_PAIRS_MAX`` ("pair dictionary full" beyond that).  A statement without
GROUP BY that has such a distinct count runs as one group under a constant key that is not emitted; when nothing in
the window passes its WHERE the one output row (counts 0, the rest NULL) is built once the status says no group was
kept.  A distinct count has no mergeable partial: with N ranks it is answered here only over a replicated view, and
a statement the ring declines goes to the generic path (the materialised window), never to the pane partials.

**SUM / AVG(DISTINCT x), count(DISTINCT a, b, …), approx_count_distinct** are answered from the same pair states
(``_requests(…, distinct_sums=True)``; routed like the distinct count: the ring or the generic path).  The pair
dictionary of x holds every live pair's value in key column 1, so SUM(DISTINCT x) is the sum of that column over a
group's live pairs: COUNT, SUM and AVG(DISTINCT x) of one x share one ``PairState`` and one fold launch,
``win_distinct_fold_kernel<true>``, which also loads each live pair's value and adds it — reduced in the wave per
distinct parent, then one atomic per word — into sum words of the combined row that no pane accumulates into (value
kind -1, 0 in every pane and block slot, like the ``dcount`` word): an ``MA_ADD_U64`` word for SUM(DISTINCT integral),
the exact wrapping ``long``, and an ``MA_ADD_F64`` word for SUM(DISTINCT float / double) and every AVG(DISTINCT x)
(accumulated as doubles, as the plain AVG slot is).  A distinct sum or average always has x's ``dcount`` word as its
count word, so ``win_emit_kernel``'s existing kinds finish it and a group without a non-NULL x gives NULL; a
non-numeric x is "sum type" / "avg type", a decimal x "argument type".  The values come from the dictionary, which
stores -0.0 as 0.0 and every NaN as the canonical one, where ``query._distinct_agg`` sums the bits of each value's
first row: a zero sum may differ in sign from the generic path's (equal under ==).  An f64 sum's last bits depend on
the order the atomics arrive in.  A layout without distinct sums runs the fold instantiation it always ran.
count(DISTINCT a, b, …) of two to ``MAX_DISTINCT_COLS`` arguments ("too many distinct columns" beyond) is one pair
state keyed by (group id, a, b, …) — the same insert kernel with more key columns; a row with a NULL in any argument
creates no pair (the validities are ANDed once per pane) — and the count fold.  approx_count_distinct(x[, rsd]) is in
this engine the exact distinct count (``query._eval_agg``): the ``dcount`` of x, sharing the state and the word of
COUNT(DISTINCT x); rsd must be a constant and is ignored.  Each different argument or tuple is one of the
``MAX_DISTINCT`` pair states.

**STDDEV / VARIANCE** (``_VARIANCE``; up to ``MAX_VARIANCE`` different arguments per statement) keep, per pane and
group, the triple (n, Σx, M2) with M2 = Σ (x − mean)² about the pane's own mean: n and Σx are the count and sum words
AVG of the same argument uses, M2 is one more word in a line whose combine op (``MA_M2``) only window_ring.hip knows.
A pane is accumulated in two passes: the fused multi-aggregate, which sees that line as unused f64 words and leaves
them 0.0, then ``win_m2_kernel``, which reads each row's group mean from the finished slot and adds the squared
distance.  The combine merges slots with the multi-way form of Chan's update (``distagg._chan_merge``'s formula), so
a block slot is again a valid triple and nothing is ever computed as Σx² − (Σx)²/n.  A layout without a variance
argument has no such line, passes no ``m2desc`` and so runs the combine without the M2 branch (below).  With N ranks
the partial states are ("s", "m2", "cnt"), the table ``distagg._partials`` builds.

**CORR / COVAR_POP / COVAR_SAMP / SKEWNESS / KURTOSIS** (``_MOMENTS``; up to ``MAX_MOMENTS`` different arguments
and pairs per statement, fallback reason "too many moment arguments") close the moment family.  skewness(x) /
kurtosis(x) reuse x's count, sum and M2 words and add M3 = Σ (x − mean)³ (kurtosis also M4, whose combine reads M3).
A pair (x, y) is keyed by both argument keys (``pair_keys``) and shared by corr, covar_pop and covar_samp of it: a
count and two sums over the rows where both are non-null — the argument columns keep their data under the validity
``x.valid & y.valid``, built once per pane in ``accumulate`` — a word Cxy = Σ (x − mean_x)(y − mean_y), and for corr
two ordinary M2 words over the masked columns (the variance machinery, unchanged; they count towards
``MAX_VARIANCE``).  M3, M4 and Cxy sit in lines of one more combine op (``MA_MOM`` = 4) that agg_multi sees as
unused; ``momdesc`` names per word its kind and the words it reads (count, sum, M2 / sum of y, M3; 6 bits each).
``win_mom_kernel`` fills them after the multi-aggregate (one sweep per argument or pair, all of its words at once),
the combine merges slots with the multi-way shift formulas (window_ring.hip), and ``win_emit_kernel`` finishes them
by Spark 2.4's rules (``fin`` entries of these kinds carry two more operand words).  A layout without one of these
aggregates has no op-4 line and no ``momdesc``.  The NaN rules test M2 > 0 on a
rounded M2: equal values that are not exactly summable can give a huge number where Spark gives NaN
(``query._moments`` has the same property).  With N ranks the partial states are those of ``distagg._partials``:
("s", "m2", "m3"[, "m4"], "cnt") and ("sx", "sy"[, "m2x", "m2y"], "cxy", "cnt").

**Exact decimals** (an unsuffixed fractional literal is a decimal and a JSON integer a long, so ``AVG(temp * 1.8 +
32)`` has a decimal argument).  SUM(x) and AVG(x) of ``decimal(p, s)``, p ≤ ``SUM_PRECISION`` = 28, one int64 lane
per row or two, keep three words per pane and group: w0 = Σ (lo & 0xffffffff), w1 = Σ (lo >> 32) (unsigned) and
w2 = Σ hi (signed; ``x >> 63`` of a one-lane value), shared by SUM and AVG of one argument with its count word.
Each word is exact below 2^31 rows per group in the window, and then the total is below 10^28 · 2^31 < 10^38: it
cannot overflow the p + 10 digits of SUM's type, so no ``fits`` test is needed (p > 28, where Spark caps the sum
type at 38 digits, overflow-to-NULL matters and a 128-bit total can wrap, stays on the paned path: "decimal
precision").  The words sit in ordinary ``MA_ADD_U64`` lines: the combine, block slots, rebuild and remap treat them
as plain u64 sums; agg_multi sees them as unused (value kind -1) and leaves them 0, and ``win_dec_kernel`` — one
launch per accumulated pane for all decimal jobs of the statement, after the multi-aggregate — reads the decimal
column in place (a pointer and a lane stride of 1 or 2) and adds the limbs, ids below the LDS bound in LDS u64
arrays, the others with 64-bit global atomics.  Integer adds: the result does not depend on the arrival order.
``win_emit_kernel`` reassembles (lo, hi) with carries and, for AVG, divides the 128-bit magnitude exactly by the
count (32-bit schoolbook division, HALF_UP on the magnitude, the sign afterwards — ``decimal.avg_from_sum``'s
result without its host loop); a decimal result takes two output rows, packed per result type by ``decimal.pack``.
MIN / MAX of a one-lane decimal is the int64 slot with a decimal dtype.  Of a two-lane decimal it is a two-word
order key: the hi lane in an ``MA_MAX`` slot (``MV_NOT`` for MIN) filled by agg_multi from a contiguous copy of the
lane, and the lo lane's key (unsigned order mapped to signed, complemented for MIN) in a line of one more combine
op (``MA_LOKEY`` = 5) that agg_multi sees as an unused ``MA_MAX`` line (INT64_MIN); a second job kind of
``win_dec_kernel`` takes the max of the lo keys of the rows whose hi key equals the slot's finished hi word, and the
combine the max of the lo words over the slots whose hi word equals the max hi (``lodesc`` names each lo word's hi
word), so all-identity rows stay the identity.  COUNT and count_if over a decimal read its validity or the
predicate; the variance and moment families take ``decimal.to_double`` of it (as ``distagg._as_double`` does).  The
results have the paned path's types — SUM ``decimal(p + 10, s)``, AVG ``decimal(p + 4, s + 4)``, MIN / MAX the
argument's — and the partial states are ``distagg._partials``': SUM ("v" of the sum type, "cnt"), AVG
("davg_{p}_{s}" — the sum —, "cnt"), MIN / MAX ("v", "cnt").  Decimal group keys and COUNT(DISTINCT decimal)
remain ineligible ("key type", "argument type").

**Row picks: first / last / max_by / min_by** (``_PICKS``; ``first_value`` / ``last_value`` are first / last; up to
``MAX_PICK`` different rank jobs and as many payload jobs per statement, fallback reason "too many pick arguments").
All four are one state per pane and group: which row wins, and that row's value.  The window's row order is that of
the materialised view: the panes in the order of ``PanedTable.pieces()`` — the view's pane list, never the order of
the pane keys —, a pane's rows in table order, a clipped pane's in-range rows in table order.  ``first(x)`` /
``last(x)`` give x of the group's first / last row that passes WHERE, NULL if that x is NULL (NULLs are not skipped);
``max_by(x, y)`` / ``min_by(x, y)`` x of the row with the largest / smallest non-NULL y, the first such row among
equals, NULL without one or if that x is NULL.  The words: a rank word R in a line of the combine op ``MA_PICK_RANK``
(identity INT64_MIN; INT64_MAX − row index where the smallest index wins, the row index for ``last``), and per payload
argument a word P (the 64 bits of x) and a word V (1.0 / 0.0: x non-NULL / NULL) in lines of ``MA_PICK_VAL`` (identity
0); agg_multi sees both kinds of line as unused.  max_by / min_by also have a key word K, the ordinary ``MA_MAX`` slot
of y (``MV_NOT`` for min_by) that MAX(y) / MIN(y) of the same statement share.  first(a) and first(b) share R,
max_by(a, y) and max_by(b, y) share K and R; each payload argument has its own P and V.  After the multi-aggregate
``dxa_win_pick`` issues two launches per accumulated pane: ``win_pick_kernel`` puts the rank of every row that counts —
for a keyed job: y non-NULL and its key equal to the slot's finished K — into R by a 64-bit max (ids below the LDS
bound through an LDS array), then ``win_pick_gather_kernel`` decodes R per group in use (the device's counter, no host
read), checks the index against the pane's rows and copies x's bits and validity.  ``pickdesc`` names per word of the
two ops its R word, its K word and the direction; the combine (one more ``win_combine_kernel`` flag, instantiated only
with a ``pickdesc``) takes such a word from one slot: among the slots — in the order of the ``slots`` array — whose
R is not the identity and, for a keyed pick, whose K is the max K, the first, or the last for ``last``.  So for a
layout with picks ``_enqueue`` passes the slots in the window's row order (``_ordered_slots``): scratch slots at their
panes' places, a complete block as its pre-combined slot only where its members stand together (combined in that
order).  Layouts without picks keep their slot order, so their f64 sums add in the order they always did.
``win_emit_kernel`` needs no new kind: P is finished by the default kind with V as its count word, and "count > 0 →
valid" makes a NULL x or a group without a row NULL.  The result has x's type: boolean is read back as ``!= 0``, float
and double from the stored double's bits, a narrow decimal keeps its ``DecimalType``.  Eligible x and y fit one 64-bit
word: byte … long, boolean, timestamp / date, float / double, decimal(p ≤ 18); anything else is "argument type".  A
double y orders as ``query._arg_extreme`` orders it — NaN the largest, -0.0 equal to 0.0 —: ``MV_F64_ORD`` has NaN
right but puts -0.0 below 0.0, so such a pick's K slot reads a copy of y with -0.0 replaced by 0.0 (``pick_y_key``) and
is not shared with MAX(y), which keeps -0.0.  first / last have the partial state "v" (``distagg._partials``), its
validity taken from V, so N ranks merge them like the paned path; max_by / min_by have no mergeable partial: like a
distinct count they are tried here and nowhere else (``query._paned_aggregate``), and take the generic path when the
ring declines, when the statement is not cacheable, or over a partitioned view at N ranks.

**String arguments: COUNT / MIN / MAX** (a plain ``StrColumn``; up to ``MAX_STRING`` MIN / MAX jobs — argument and
direction — per statement, "too many string arguments" beyond).  COUNT(x) reads the column's validity into the ordinary
count slot.  The order of MIN / MAX is unsigned byte order of the UTF-8 bytes, a proper prefix first
(``ops/sort.string_ranks``' and Python's).  A job is one whole line of the combine op ``MA_STRKEY`` = 8, for values of
up to ``STR_WIDTH`` = 48 bytes: six words of the zero-padded bytes big-endian, each mapped to the signed order (^ 2^63),
a length word and a spare; MIN complements every word; the identity of every word is INT64_MIN, below every value — ""
included, whose length word is 0 (``pack_str_words`` / ``unpack_str_words`` are the host forms).  agg_multi sees the
line as unused MAX words.  After the multi-aggregate ``dxa_win_strkey`` — one call per accumulated pane for all jobs —
runs str_minmax.hip's arg-extreme kernel over the pane's rows (the pane's ids and WHERE mask) and a gather over the
groups in use that checks the winning row index against [0, n) and writes its packed words.  The combine (one more
``win_combine_kernel`` flag, instantiated only with a ``strdesc``) takes each word of the line from the slot whose
7-word tuple is lexicographically greatest: a maximum over a total order, so block slots, scratch slots and rebuilds
stay valid.  ``win_emit_kernel``'s kind ``F_STRW`` undoes a byte word's mapping and ``str_column_of`` builds the
result column with tensor operations; the count word (shared with COUNT(x)) gives the validity.  A winning value of
more than 48 bytes has no key: the gather sets status flag 8, which travels in the one status read, and the statement
goes to the paned path for good ("argument too long"), where ``groupby.aggregate`` runs the same kernel per pane.  The
partial states are ``distagg._partials``': "v" (a string column) and "cnt".  Everything else over a string, string
payloads of row picks included, stays "argument type"; a pick's payload could reuse the line with its rank word as the
source of the row index.

**One answer, one plan entry per aggregate.**  Every layout is answered by the same call, ``dxa_win_answer``
(combine, one distinct fold per pair state, keep, compaction, output rows), and its complete blocks are combined by
``dxa_win_combine_block``; the families differ only in what they hand over — the pair states' folds, ``m2desc``,
``momdesc``, ``lodesc``, ``pickdesc``, ``strdesc``, each 0 when the layout has none — and the absent descriptors pick
the ``win_combine_kernel`` instantiation without that branch, so a layout without X issues the launches it would issue
if X did not exist (tests/test_window_dense_comoments.py pins the sequences).  ``plan_layout`` describes an aggregate
once, where its slots are chosen: its ``plan`` entry, its finishing recipe and its partial states, all in slot terms;
one pass after packing turns slots into words.  Adding an aggregate means one arm there (and, for a new kind of word,
its kernels).
"""
from __future__ import annotations

import ctypes
import heapq
from typing import Dict, List, Optional

import torch

from ..ops import native as N
from ..ops.groupby import (_DEC_KEY_MAX, _DEC_KEY_MIN, _DEC_SUM, _F_AVG, _F_CORR, _F_COUNT, _F_COVAR_POP, _F_COVAR_SAMP,
                           _F_DEC_AVG, _F_DEC_MM, _F_DEC_SUM, _F_F64, _F_F64_ORD, _F_HI, _F_I64, _F_KURT, _F_NOT,
                           _F_SKEW, _F_SQRT, _F_STRW, _F_VAR_POP, _F_VAR_SAMP, _MA_ADD_F64, _MA_ADD_U64, _MA_LOKEY,
                           _MA_M2, _MA_MAX, _MA_MOM, _MA_PICK_RANK, _MA_PICK_VAL, _MA_STRKEY, _MOM_CXY, _MOM_M3,
                           _MOM_M4, _MV_COUNT, _MV_F64, _MV_F64_ORD, _MV_I64, _MV_NOT, _PICK_LAST, _PICK_USED)
from ..ops.hashing import MAX_KEY_COLS, _KeyCols, key_cols
from . import decimal as Dec
from .column import ConstColumn, PrimColumn, StrColumn, materialize
from .decimal import is_decimal
from ..sql.ast import Literal

DENSE_GROUPS = 1 << 16            # initial dictionary capacity per statement (groups with ids at one time)
DENSE_GROUPS_MAX = 1 << 20        # the capacity grows to this at most (win_compact_kernel's single-workgroup scan)
SCRATCH_SLOTS = 4                 # ring slots for panes only partly inside a window (re-aggregated every batch)
BLOCK = 16                        # consecutive in-window panes pre-combined into one block slot, once
DENSE_PAIRS = 1 << 16             # initial capacity of a COUNT(DISTINCT x) pair dictionary ((group, x) pairs with ids)
DENSE_PAIRS_MAX = 1 << 20         # it grows to this at most (its presence ring is one byte per ring slot and pair)
MAX_DISTINCT = 4                  # different distinct arguments per statement (window_ring.hip kMaxPairStates)
MAX_DISTINCT_COLS = 4             # arguments of one count(DISTINCT a, b, …): value columns of its pair dictionary
MAX_VARIANCE = 8                  # different STDDEV / VARIANCE arguments per statement (window_ring.hip kMaxM2Args)
MAX_MOMENTS = 8                   # skewness / kurtosis arguments plus corr / covar pairs (window_ring.hip kMaxMomArgs)
MAX_DECIMAL = 8                   # decimal sum arguments plus two-lane decimal MIN / MAX (window_ring.hip kMaxDecJobs)
SUM_PRECISION = 28                # SUM / AVG of decimal(p, s) is answered here for p up to this (``plan_layout``)
MAX_PICK = 8                      # different rank jobs, and different payload jobs, of first / last / max_by / min_by
                                  # per statement (window_ring.hip kMaxPickJobs)
MAX_STRING = 8                    # string MIN / MAX jobs (argument and direction) per statement (kMaxStrJobs)
STR_WIDTH = 48                    # bytes of a string MIN / MAX value the ring holds (window_ring.hip kKeyWidth)
_ANSWER = [N.c_p, N.c_i32, N.c_i32, N.c_p, N.c_i32, N.c_p, N.c_i32, N.c_p, N.c_p, N.c_p, N.c_p]    # ring … out_idx
# m2desc, its host copy, momdesc, its host copy, lodesc, its host copy, pickdesc, its host copy, strdesc, its host copy
# (0: the layout has none)
_DESCS = [N.c_p, N.c_p, N.c_p, N.c_p, N.c_p, N.c_p, N.c_p, N.c_p, N.c_p, N.c_p]
N.register_sigs({
    "dxa_win_sizes": [N.c_p],
    "dxa_win_emit_size": [],
    "dxa_win_pairfold_size": [],
    "dxa_win_m2_size": [],
    "dxa_win_m2_lds_groups": [],
    "dxa_win_mom_size": [],
    "dxa_win_dec_size": [],
    "dxa_win_dec": [N.c_p, N.c_p],
    "dxa_win_pick_size": [],
    "dxa_win_pick": [N.c_p, N.c_p],
    "dxa_win_strkey_size": [],
    "dxa_win_strkey": [N.c_p, N.c_p],
    "dxa_win_init": [N.c_p, N.c_p, N.c_i64, N.c_p],
    "dxa_win_insert_fused": [N.c_p, N.c_p, N.c_p, N.c_p, N.c_i64, N.c_p, N.c_p, N.c_p, N.c_p],
    "dxa_win_m2": [N.c_p, N.c_p],
    "dxa_win_mom": [N.c_p, N.c_p],
    "dxa_win_pair_prep": [N.c_p, N.c_i64, N.c_i32, N.c_p, N.c_p, N.c_p, N.c_p],
    "dxa_win_pair_mark": [N.c_p, N.c_i64, N.c_i32, N.c_p, N.c_i64, N.c_i32, N.c_p],
    "dxa_win_pair_or_block": [N.c_p, N.c_i64, N.c_p, N.c_i32, N.c_i32, N.c_p],
    "dxa_win_combine_block": [N.c_p, N.c_i32, N.c_i32, N.c_p, N.c_i32, N.c_p, N.c_i32, N.c_p, *_DESCS, N.c_p],
    "dxa_win_answer": [*_ANSWER, N.c_p, N.c_p, N.c_p, *_DESCS, N.c_p],       # … emit, dictcols, folds, …, stream
    "dxa_win_live": [*_ANSWER, N.c_p],
    "dxa_win_remap_dict": [N.c_p, N.c_p, N.c_p, N.c_i32, N.c_p],
    "dxa_win_remap_ring": [N.c_p, N.c_p, N.c_i32, N.c_i32, N.c_i32, N.c_p, N.c_i32, N.c_i32, N.c_p, N.c_p, N.c_i32,
                           N.c_p],
    "dxa_win_rehash": [N.c_p, N.c_p, N.c_p, N.c_i64, N.c_i32, N.c_p, N.c_p],
})
# the variance family → the finishing kind of its M2 word (window_ring.hip win_emit_kernel)
_VARIANCE = {"stddev": _F_VAR_SAMP | _F_SQRT, "std": _F_VAR_SAMP | _F_SQRT, "stddev_samp": _F_VAR_SAMP | _F_SQRT,
             "stddev_pop": _F_VAR_POP | _F_SQRT, "variance": _F_VAR_SAMP, "var_samp": _F_VAR_SAMP,
             "var_pop": _F_VAR_POP}
_BOOL = {"bool_and": "min", "every": "min", "bool_or": "max", "any": "max", "some": "max"}
# the other central-moment aggregates → the finishing kind of their M3 / M4 / Cxy word; the last three take a pair
_MOMENTS = {"skewness": _F_SKEW, "kurtosis": _F_KURT, "covar_pop": _F_COVAR_POP, "covar_samp": _F_COVAR_SAMP,
            "corr": _F_CORR}
_PAIRED = ("covar_pop", "covar_samp", "corr")
_NUMERIC = ("byte", "short", "int", "long", "double", "float")
# row picks: x of one row of the group — the first or last in the window's row order, or the one with the extreme y
_PICKS = ("first", "last", "max_by", "min_by")
_PICKABLE = (*_NUMERIC, "boolean", "timestamp", "date")      # (and decimal(p, s), p ≤ 18): one 64-bit word per value
_PICK_ALIAS = {"first_value": "first", "last_value": "last"}
_SUPPORTED = {"count", "sum", "min", "max", "avg", "mean", "count_if", *_VARIANCE, *_BOOL, *_MOMENTS}
# The row picks are eligible only for a caller that passes the combine its slots in the window's row order, and says so
# (``_requests(aggs, picks=True)``; ``dense_answer`` does): the first two have a mergeable partial state, the keyed
# ones have none and only the ring answers them (as it does COUNT(DISTINCT x))
_RING_ONLY = ("max_by", "min_by")
# The pair-state aggregates beyond COUNT(DISTINCT x) — SUM / AVG(DISTINCT x), count(DISTINCT a, b, …) and
# approx_count_distinct(x[, rsd]) — are eligible only under ``_requests(aggs, distinct_sums=True)`` (``dense_answer``
# passes it): their funcs are "dsum", "davg" and "dcount" (the last with a tuple of arguments for several columns)
_DISTINCT = ("dcount", "dsum", "davg")


def distinct_key(arg):
    """The key of a pair state: the argument's key, or for count(DISTINCT a, b, …) — ``arg`` a tuple — the tuple of
    its arguments' keys under a tag no expression key starts with."""
    return ("dtuple", *(a.key() for a in arg)) if isinstance(arg, tuple) else arg.key()


def pick_y_key(y):
    """The argument key of a double order key y of max_by / min_by with -0.0 replaced by 0.0 (``DenseWindow.accumulate``
    builds the column): the K slot of such a pick reads it, so its zeros tie as they do in ``query._arg_extreme``."""
    return ("pick_y", y.key())


def pair_keys(x, y):
    """The argument keys of the columns x and y of a pair (x, y) restricted to the rows where both are non-null:
    their data is the arguments', their validity ``x.valid & y.valid`` (``DenseWindow.accumulate``)."""
    return ("pair_x", x.key(), y.key()), ("pair_y", x.key(), y.key())


class _DictCol(ctypes.Structure):
    _fields_ = [("vals", ctypes.c_void_p), ("lens", ctypes.c_void_p), ("valid", ctypes.c_void_p),
                ("kind", ctypes.c_int32), ("pad", ctypes.c_int32)]


class _DictCols(ctypes.Structure):
    _fields_ = [("c", _DictCol * MAX_KEY_COLS), ("ncols", ctypes.c_int32), ("gcap", ctypes.c_int32)]


class _EmitArgs(ctypes.Structure):
    _fields_ = [("acc", ctypes.c_void_p), ("stride", ctypes.c_int32), ("nreq", ctypes.c_int32),
                ("kind", ctypes.c_int32 * 64), ("pos", ctypes.c_int32 * 64), ("cnt", ctypes.c_int32 * 64),
                ("op2", ctypes.c_int32 * 64), ("op3", ctypes.c_int32 * 64), ("dst", ctypes.c_void_p),
                ("dvalid", ctypes.c_void_p), ("okey", ctypes.c_void_p * MAX_KEY_COLS),
                ("olen", ctypes.c_void_p * MAX_KEY_COLS), ("ovalid", ctypes.c_void_p * MAX_KEY_COLS),
                ("out_idx", ctypes.c_void_p), ("scal", ctypes.c_void_p), ("gcap", ctypes.c_int32)]


class _PairFold(ctypes.Structure):
    _fields_ = [("pres", ctypes.c_void_p), ("pitch", ctypes.c_int64), ("parent", ctypes.c_void_p),
                ("pscal", ctypes.c_void_p), ("pcap", ctypes.c_int32), ("word", ctypes.c_int32),
                ("vals", ctypes.c_void_p), ("vkind", ctypes.c_int32), ("isum", ctypes.c_int32),
                ("fsum", ctypes.c_int32), ("pad", ctypes.c_int32)]


class _PairFolds(ctypes.Structure):
    _fields_ = [("p", _PairFold * MAX_DISTINCT), ("n", ctypes.c_int32), ("pad", ctypes.c_int32)]


class _M2Arg(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("cnt", ctypes.c_int32), ("sum", ctypes.c_int32),
                ("m2", ctypes.c_int32), ("pad", ctypes.c_int32)]


class _M2Args(ctypes.Structure):
    _fields_ = [("a", _M2Arg * MAX_VARIANCE), ("gid", ctypes.c_void_p), ("row", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("gcap", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("nargs", ctypes.c_int32), ("pad", ctypes.c_int32)]


class _MomArg(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("cnt", ctypes.c_int32),
                ("sum", ctypes.c_int32), ("sumy", ctypes.c_int32), ("w0", ctypes.c_int32), ("w1", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


class _MomArgs(ctypes.Structure):
    _fields_ = [("a", _MomArg * MAX_MOMENTS), ("gid", ctypes.c_void_p), ("row", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("gcap", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("nargs", ctypes.c_int32), ("pad", ctypes.c_int32)]


class _DecJob(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("lanes", ctypes.c_int32),
                ("kind", ctypes.c_int32), ("w0", ctypes.c_int32), ("w1", ctypes.c_int32), ("w2", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


class _DecArgs(ctypes.Structure):
    _fields_ = [("a", _DecJob * MAX_DECIMAL), ("gid", ctypes.c_void_p), ("row", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("gcap", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("nargs", ctypes.c_int32), ("pad", ctypes.c_int32)]


class _PickRank(ctypes.Structure):
    _fields_ = [("y", ctypes.c_void_p), ("yvalid", ctypes.c_void_p), ("kind", ctypes.c_int32), ("k", ctypes.c_int32),
                ("r", ctypes.c_int32), ("last", ctypes.c_int32)]


class _PickVal(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("xvalid", ctypes.c_void_p), ("r", ctypes.c_int32), ("p", ctypes.c_int32),
                ("v", ctypes.c_int32), ("last", ctypes.c_int32)]


class _PickArgs(ctypes.Structure):
    _fields_ = [("rank", _PickRank * MAX_PICK), ("val", _PickVal * MAX_PICK), ("gid", ctypes.c_void_p),
                ("row", ctypes.c_void_p), ("scal", ctypes.c_void_p), ("n", ctypes.c_int64), ("gcap", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("nrank", ctypes.c_int32), ("nval", ctypes.c_int32)]


class _StrJob(ctypes.Structure):
    _fields_ = [("arena", ctypes.c_void_p), ("starts", ctypes.c_void_p), ("lens", ctypes.c_void_p),
                ("valid", ctypes.c_void_p), ("line", ctypes.c_int32), ("min", ctypes.c_int32)]


class _StrKeyArgs(ctypes.Structure):
    _fields_ = [("a", _StrJob * MAX_STRING), ("gid", ctypes.c_void_p), ("keep", ctypes.c_void_p),
                ("row", ctypes.c_void_p), ("scal", ctypes.c_void_p), ("best", ctypes.c_void_p), ("n", ctypes.c_int64),
                ("gcap", ctypes.c_int32), ("stride", ctypes.c_int32), ("njobs", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


_SIZES: Optional[List[int]] = None


def _sizes() -> List[int]:
    global _SIZES
    if _SIZES is None:
        out = (ctypes.c_int32 * 3)()
        N.lib().dxa_win_sizes(out)
        _SIZES = list(out)
        if _SIZES[0] != ctypes.sizeof(_KeyCols) or _SIZES[1] != ctypes.sizeof(_DictCols) or \
                N.lib().dxa_win_emit_size() != ctypes.sizeof(_EmitArgs) or \
                N.lib().dxa_win_pairfold_size() != ctypes.sizeof(_PairFolds) or \
                N.lib().dxa_win_m2_size() != ctypes.sizeof(_M2Args) or \
                N.lib().dxa_win_mom_size() != ctypes.sizeof(_MomArgs) or \
                N.lib().dxa_win_dec_size() != ctypes.sizeof(_DecArgs) or \
                N.lib().dxa_win_pick_size() != ctypes.sizeof(_PickArgs) or \
                N.lib().dxa_win_strkey_size() != ctypes.sizeof(_StrKeyArgs) or _SIZES[2] != STR_WIDTH:
            raise N.NativeError("window_ring.hip struct layout differs from window_dense.py")
    return _SIZES


class Ineligible(Exception):
    """The statement (or this batch) is answered by the paned path."""


_I64_MIN = -(1 << 63)


def _signed(u: int) -> int:
    return u - (1 << 64) if u >> 63 else u


def pack_str_words(b: bytes, is_min: bool = False) -> tuple:
    """The 7 order-key words (signed 64-bit integers) of a string MIN / MAX value of up to ``STR_WIDTH`` bytes, as
    win_strkey_gather_kernel writes them: six words of the zero-padded bytes big-endian, each mapped to the signed
    order (^ 2^63), and the length; every word complemented for MIN.  The tuple order of two values' words is the byte
    order of the values (reversed for MIN), and every tuple is above the identity (INT64_MIN seven times)."""
    assert len(b) <= STR_WIDTH
    padded = b.ljust(STR_WIDTH, b"\0")
    words = [_signed(int.from_bytes(padded[q:q + 8], "big") ^ 1 << 63) for q in range(0, STR_WIDTH, 8)] + [len(b)]
    return tuple(~w for w in words) if is_min else tuple(words)


def unpack_str_words(words, is_min: bool = False) -> Optional[bytes]:
    """``pack_str_words`` undone; the identity ("no row") gives None."""
    if all(w == _I64_MIN for w in words):
        return None
    words = [~w for w in words] if is_min else list(words)
    raw = b"".join(((w ^ _I64_MIN) & (1 << 64) - 1).to_bytes(8, "big") for w in words[:6])
    return raw[:words[6]]


def str_column_of(words: List[torch.Tensor], lens: torch.Tensor, ok: torch.Tensor) -> StrColumn:
    """The finished words of a string MIN / MAX (win_emit_kernel has undone the mapping: six rows of big-endian byte
    words and a row of lengths, [groups] each) as a string column over a fresh arena of ``STR_WIDTH`` bytes per group.
    Tensor operations only."""
    n = int(lens.shape[0])
    arena = torch.stack(words, dim=1).contiguous().view(torch.uint8).view(n, len(words), 8).flip(2).reshape(-1)
    starts = torch.arange(n, dtype=torch.int64, device=lens.device) * STR_WIDTH
    c = StrColumn(arena, starts, torch.where(ok, lens, torch.zeros_like(lens)).to(torch.int32), ok)
    c.max_len = STR_WIDTH
    return c


def _requests(aggs: Dict, picks: bool = False, distinct_sums: bool = False):
    """[(agg key, func, arg expr or None)] or Ineligible.  ``COUNT(DISTINCT x)`` with one argument is the func
    "dcount"; every other DISTINCT aggregate is ineligible, and so are more than ``MAX_DISTINCT`` different
    distinct arguments.  The variance family keeps its name (``_VARIANCE``), ``bool_and`` / ``every`` are "min" and
    ``bool_or`` / ``any`` / ``some`` "max" of a boolean result ("bmin" / "bmax"); more than ``MAX_VARIANCE``
    different variance arguments are ineligible.  ``skewness`` / ``kurtosis`` (one argument) and ``corr`` /
    ``covar_pop`` / ``covar_samp`` (two: the arg entry is the tuple (x, y)) keep their names too; each different
    argument or pair is one job of the pane's moment pass, and more than ``MAX_MOMENTS`` of them are ineligible.  The
    M2 words they need (skewness / kurtosis: of the argument; corr: of both masked columns of the pair) count as
    variance arguments.  ``first`` / ``last`` (one argument; ``first_value`` / ``last_value`` are the
    same funcs, and the two-argument ``first(x, true)`` stays ineligible under its own name) and ``max_by`` /
    ``min_by`` (two: the arg entry is the tuple (x, y)) keep their names — all four only with ``picks``, which promises
    that the combine gets its slots in the window's row order, as ``_enqueue`` passes them; more than ``MAX_PICK``
    different rank jobs (first, last, and one per direction and y) or payload jobs (rank job and x) are ineligible.
    With ``distinct_sums`` (the caller hands ``plan_layout`` the distinct arguments' types too, and its pair states
    take several value columns): ``SUM(DISTINCT x)`` / ``AVG(DISTINCT x)`` are "dsum" / "davg" of x,
    ``count(DISTINCT a, b, …)`` of two to ``MAX_DISTINCT_COLS`` arguments is "dcount" of the tuple (more: "too many
    distinct columns"), ``approx_count_distinct(x)`` / ``approx_count_distinct(x, rsd)`` with a constant rsd — which
    is ignored, as the generic evaluator ignores it — is "dcount" of x.  Each different argument or tuple is one of the
    ``MAX_DISTINCT`` pair states, shared by every aggregate over it."""
    out = []
    dargs = set()
    vargs = set()
    margs = set()
    pranks, pvals = set(), set()
    for ak, call in aggs.items():
        name = call.name
        approx = distinct_sums and name == "approx_count_distinct" and not call.distinct
        if name not in _SUPPORTED and not approx and not (picks and _PICK_ALIAS.get(name, name) in _PICKS):
            raise Ineligible(name)
        if call.distinct or approx:
            func, arg = "dcount", call.args[0] if call.args else None
            if approx:
                if len(call.args) not in (1, 2) or (len(call.args) == 2 and not isinstance(call.args[1], Literal)):
                    raise Ineligible(name)
            elif distinct_sums and name in ("sum", "avg") and len(call.args) == 1:
                func = "d" + name
            elif distinct_sums and name == "count" and not call.star and len(call.args) > 1:
                if len(call.args) > MAX_DISTINCT_COLS:
                    raise Ineligible("too many distinct columns")
                arg = tuple(call.args)
            elif name != "count" or call.star or len(call.args) != 1:
                raise Ineligible(f"{name} distinct")
            dargs.add(distinct_key(arg))
            if len(dargs) > MAX_DISTINCT:
                raise Ineligible("too many distinct arguments")
            out.append((ak, func, arg))
            continue
        if call.star or (name == "count" and not call.args):
            out.append((ak, "count_star", None))
            continue
        if name in _MOMENTS:
            if len(call.args) != (2 if name in _PAIRED else 1):
                raise Ineligible(name)
            if name in _PAIRED:
                margs.add(pair_keys(*call.args))
                if name == "corr":
                    vargs.update(pair_keys(*call.args))
            else:
                margs.add(call.args[0].key())
                vargs.add(call.args[0].key())
            if len(margs) > MAX_MOMENTS or len(vargs) > MAX_VARIANCE:
                raise Ineligible("too many moment arguments")
            out.append((ak, name, tuple(call.args) if name in _PAIRED else call.args[0]))
            continue
        name = _PICK_ALIAS.get(name, name)
        if name in _PICKS:
            keyed = name in _RING_ONLY
            if len(call.args) != (2 if keyed else 1):
                raise Ineligible(call.name)
            rank = (name, call.args[1].key()) if keyed else (name,)
            pranks.add(rank)
            pvals.add((rank, call.args[0].key()))
            if len(pranks) > MAX_PICK or len(pvals) > MAX_PICK:
                raise Ineligible("too many pick arguments")
            out.append((ak, name, tuple(call.args) if keyed else call.args[0]))
            continue
        if len(call.args) != 1:
            raise Ineligible(name)
        if name in _VARIANCE:
            vargs.add(call.args[0].key())
            if len(vargs) > MAX_VARIANCE:
                raise Ineligible("too many variance arguments")
        out.append((ak, "avg" if name == "mean" else "b" + _BOOL[name] if name in _BOOL else name, call.args[0]))
    return out


def _target_capacity(live: int, gcap: int, gmax: int) -> int:
    """The capacity a rebuild leaves the dictionary with: ``gcap``, doubled while more than half of it is live and
    ``gmax`` allows.  After growth the dictionary is at most half full, so at least ``target / 2`` new keys arrive
    before the next rebuild; at ``gmax`` a rebuild only recycles."""
    target = gcap
    while live > target // 2 and target < gmax:
        target = min(2 * target, gmax)
    return target


def _table_slots(gcap: int) -> int:
    """Hash-table slots for ``gcap`` groups: a power of two, at least twice the capacity."""
    return 1 << max(10, (2 * gcap - 1).bit_length())


def _pitch(pcap: int) -> int:
    """Bytes of one presence row: a byte per pair and the dump row, padded to the fold's 16-byte loads."""
    return (pcap + 1 + 15) // 16 * 16


def _distinct_arg(c):
    """A COUNT(DISTINCT x) argument as a pair-dictionary key column (what ``accumulate`` accepts as a group key)."""
    c = materialize(c)
    if isinstance(c, ConstColumn):
        c = c.materialize()
    if isinstance(c, PrimColumn):
        if is_decimal(c.dtype) or c.data.dim() != 1:
            raise Ineligible("argument type")
        if c.data.dtype == torch.float32:
            return PrimColumn(c.dtype, c.data.to(torch.float64), c.valid)
        if c.data.dtype not in (torch.int64, torch.float64):
            return PrimColumn(c.dtype, c.data.to(torch.int64), c.valid)
        return c
    if type(c) is not StrColumn:
        raise Ineligible("argument type")
    return c


def plan_layout(reqs, arg_types: Dict) -> Dict:
    """The accumulator layout of a statement (no device involved).  ``reqs``: ``_requests``' result;
    ``arg_types[arg key] = (column dtype, is float64)`` of every evaluated non-distinct argument and of the argument
    of every SUM / AVG(DISTINCT x).  Those two share x's ``dcount`` slot as their count slot and add sum slots of value
    kind -1 that only the distinct fold fills: ``dsum_words`` {x key: (u64 sum word, f64 sum word), -1 where absent};
    the key is absent from a layout without them.

    → ``slots`` [(key, agg_multi value kind, combine op)], ``order`` (slot per word, None for padding),
    ``line_ops`` (combine op per 8-word line), ``plan`` [(agg key, kind, slot, count slot, dtype)] and beside it
    ``as_f64`` (per ``plan`` entry: the finished words are doubles), ``fin`` / ``pfin`` (win_emit_kernel's (kind,
    word, count word) per aggregate / per partial state; a distinct count has no partial), ``m2desc`` and
    ``m2args`` (the variance arguments' words for win_combine_kernel and win_m2_kernel).  With skewness / kurtosis
    / corr / covar_*: their ``fin`` entries are (kind, word, count word, operand 2, operand 3), ``momdesc`` describes
    the words of the op-4 lines to win_combine_kernel and ``momargs`` [(x key, y key or None, count, sum x, sum y,
    word 0, word 1)] lists win_mom_kernel's jobs; a pair's slots are keyed by ``pair_keys``.

    A decimal argument's ``arg_types`` entry carries its ``DecimalType``.  SUM / AVG of decimal(p, s), p ≤
    ``SUM_PRECISION``, share three limb-sum slots per argument — Σ (lo & 0xffffffff), Σ (lo >> 32), Σ hi, in
    ``MA_ADD_U64`` lines with value kind -1 — and its count slot.  Each limb sum is exact while a group has fewer than
    2^31 rows in the window, and then the total is below 10^28 · 2^31 < 10^38: it cannot overflow the p + 10 digits
    of SUM's type (nor 128 bits), so unlike the paned path's ``decimal.agg_sum`` no ``fits`` test is needed.  Beyond
    28 digits Spark's sum type is capped at 38, overflow-to-NULL matters and the total can wrap: "decimal precision".
    MIN / MAX of a narrow decimal is the int64 slot with a decimal dtype; of a two-lane one a two-word order key, the
    hi lane in an ``MA_MAX`` slot and the lo lane's key in a slot of an ``MA_LOKEY`` line (``lodesc``: per such word
    its high word | 1 << 16).  A decimal result takes two ``fin`` rows (lo, then hi with ``_F_HI``), so ``rows`` gives
    per ``plan`` entry (first ``fin`` row, rows), and a decimal partial state in ``pfin`` is a list of two recipes.
    ``decargs`` [(arg key, job kind, word 0, word 1, word 2)] lists win_dec_kernel's jobs.  ``lodesc`` / ``decargs``
    are absent from a layout without such words.  The variance and moment families take a decimal argument as the
    double ``decimal.to_double`` gives (as Spark casts it).

    first / last / max_by / min_by (module docstring): a rank slot in an ``MA_PICK_RANK`` line, a payload and a
    validity slot per payload argument in ``MA_PICK_VAL`` lines, all with value kind -1, and for the keyed ones the
    ``MA_MAX`` slot of y.  ``pickdesc`` (per word of those lines: R word | (K word + 1) << 8 | last << 16 | in use <<
    17) is win_combine_kernel's, ``pickargs`` = (rank jobs [(K argument key or None, K value kind, K word or -1, R
    word, last)], payload jobs [(x key, R word, P word, V word, last)]) dxa_win_pick's, ``pick_x`` maps a pick's agg key
    to its payload argument.  All three are absent from a layout without picks.

    MIN / MAX of a string argument (``arg_types`` entry ("string", False)): one whole ``MA_STRKEY`` line per argument
    and direction — eight slots of value kind -1: six byte words, the length word, a spare — and the argument's
    ordinary count slot, which COUNT of the same argument shares.  Seven ``fin`` rows (``_F_STRW`` for the byte words,
    ``_F_I64`` for the length; ``_F_NOT`` for MIN), a ``plan`` entry of kind "str" and the partial states "v" (the seven
    recipes) and "cnt".  ``strdesc`` (per word of such a line its place in the tuple + 1) is win_combine_kernel's,
    ``strargs`` [(argument key, is MIN, first word)] dxa_win_strkey's; both are absent from a layout without string
    lines.  More than ``MAX_STRING`` jobs: "too many string arguments".  COUNT of a string reads its validity like any
    count; every other aggregate over one is "argument type" (``DenseWindow.accumulate``)."""
    # accumulator slots, packed into 8-word lines of one atomic kind (as groupby.aggregate_many packs them)
    slots, keyed = [], {}

    def slot(key, kind, op):
        s = keyed.get(key)
        if s is None:
            s = keyed[key] = len(slots)
            slots.append((key, kind, op))
        return s

    star = slot(("count", None), _MV_COUNT, _MA_ADD_F64)
    plan, fins, pfins, as_f64, rows = [], [], {}, [], []
    lo_of = {}                      # low key slot of a two-lane decimal MIN / MAX → its high key slot
    dec_jobs = {}                   # (job, argument key) → (argument key, win_dec_kernel job kind, its three slots)
    m2_of = {}                      # M2 slot → (count slot, sum slot) of the same argument
    mom_of = {}                     # M3 / M4 / Cxy slot → (kind, the slots its combine reads)
    mom_jobs = {}                   # argument key or pair keys → [x, y, count, sum x, sum y, word-0, word-1 slot]
    pick_of = {}                    # R / P / V slot of a row pick → (its R slot, its K slot or None, last among equals)
    pick_ranks = {}                 # R slot → (K slot's argument key or None, its value kind, K slot or None, last)
    pick_vals = {}                  # P slot → (x key, R slot, V slot, last)
    pick_x = {}                     # agg key of a pick → its payload argument's key
    str_jobs = {}                   # (func, argument key) of a string MIN / MAX → (argument key, is MIN, its 8 slots)

    def agg(ak, kind, s, c, dt, fkind, states, ops=(), f64=None):
        """One aggregate, described once and in slot terms (mapped to words after packing): its ``plan`` entry, its
        finishing recipe (emit kind, value slot, count slot[, operand slots]), its partial states {suffix: (emit
        kind, slot, count slot)} — ``distagg._partials``' suffixes: "cnt" a count, "v" the SUM / MIN / MAX value, "s"
        a raw double sum, "m2" / "m3" / "m4" centred sums, a pair's "sx", "sy", "cxy" (and corr's "m2x", "m2y") over
        its both-non-null rows; None: no mergeable partial — and whether its finished words are doubles.  ``fkind``
        may be a list of two whole recipes instead (``two``: a 128-bit result), and so may a partial state."""
        plan.append((ak, kind, s, c, dt))
        recipes = fkind if isinstance(fkind, list) else [(fkind, s, c, *ops)]
        rows.append((len(fins), len(recipes)))
        fins.extend(recipes)
        if states is not None:
            pfins[ak] = states
        as_f64.append(dt == "double" if f64 is None else f64)

    def count_of(c):
        return _F_COUNT, c, None

    def two(fkind, s, c, op2, op3):
        """The recipes of a 128-bit decimal result's two output rows: the low 64 bits, the signed high word."""
        return [(fkind, s, c, op2, op3), (fkind | _F_HI, s, c, op2, op3)]

    def numeric(dtype):
        return dtype in _NUMERIC or is_decimal(dtype)

    for ak, func, arg in reqs:
        if func == "count_star":
            agg(ak, "count", star, None, None, _F_COUNT, {"cnt": count_of(star)})
            continue
        if func == "dcount":
            # a count word no pane accumulates into (agg_multi's "unused" spec): 0 in every pane and block
            # slot, filled per batch by win_distinct_fold_kernel and finished by F_COUNT like any count
            agg(ak, "count", slot(("dcount", distinct_key(arg)), _MV_COUNT, _MA_ADD_F64), None, None, _F_COUNT, None)
            continue
        if func in ("dsum", "davg"):
            # SUM / AVG(DISTINCT x): the sum of x over the group's live pairs, added by the distinct fold beside the
            # count of the same pairs — the dcount word of x, which such an aggregate always has and which is its
            # count word ("count > 0 → valid": a group without a non-NULL x gives NULL).  The sum words are words no
            # pane accumulates into either (value kind -1): the exact wrapping int64 sum in a u64 add line for
            # SUM(DISTINCT integral), the f64 sum for SUM(DISTINCT float / double) and for every AVG(DISTINCT x)
            # (accumulated as doubles, as the plain AVG slot is).  No mergeable partial, as for the distinct count
            ck = arg.key()
            dtype = arg_types[ck][0]
            if is_decimal(dtype):
                raise Ineligible("argument type")
            if dtype not in _NUMERIC:
                raise Ineligible(f"{func[1:]} type")
            dc = slot(("dcount", ck), _MV_COUNT, _MA_ADD_F64)
            if func == "dsum" and dtype not in ("float", "double"):
                agg(ak, "sum", slot(("dsumi", ck), -1, _MA_ADD_U64), dc, "long", _F_I64, None)
            else:
                sm = slot(("dsumf", ck), -1, _MA_ADD_F64)
                agg(ak, func[1:], sm, dc, "double", _F_F64 if func == "dsum" else _F_AVG, None)
            continue
        if func in _PICKS:
            # a row pick: a rank word R (which row of the pane wins; shared by every pick of the same kind and y), and
            # per payload argument x that row's 64 bits P and its validity V as a double 1.0 / 0.0 — a count word to
            # win_emit_kernel, whose rule "count > 0 → valid" then makes a NULL x (or no row) a NULL result.  max_by /
            # min_by: and the key word K, the ordinary MAX slot of y (complemented for min_by) that MAX(y) / MIN(y) of
            # the same statement share; a double y is keyed by a copy with -0.0 → 0.0 (``pick_y_key``), which only
            # the picks read, so that equal zeros tie as in ``query._arg_extreme``
            x, y = arg if isinstance(arg, tuple) else (arg, None)
            for a in (x,) if y is None else (x, y):
                dt = arg_types[a.key()][0]
                if not (dt in _PICKABLE or (is_decimal(dt) and dt.narrow)):
                    raise Ineligible("argument type")
            xdt = arg_types[x.key()][0]
            last = func == "last"
            ks = yk = kkind = None
            rank = (func,)
            if y is not None:
                is_fy = arg_types[y.key()][0] in ("float", "double")
                yk = pick_y_key(y) if is_fy else y.key()
                kkind = (_MV_F64_ORD if is_fy else _MV_I64) | (_MV_NOT if func == "min_by" else 0)
                ks = slot((func[:3], yk), kkind, _MA_MAX)
                rank = (func, yk)
            r = slot(("pickr", rank), -1, _MA_PICK_RANK)
            pv = slot(("pickp", (rank, x.key())), -1, _MA_PICK_VAL)
            vv = slot(("pickv", (rank, x.key())), -1, _MA_PICK_VAL)
            for sl in (r, pv, vv):
                pick_of[sl] = (r, ks, last)
            pick_ranks[r] = (yk, kkind, ks, last)
            pick_vals[pv] = (x.key(), r, vv, last)
            pick_x[ak] = x.key()
            agg(ak, "pick", pv, vv, xdt, _F_I64, {"v": (_F_I64, pv, vv)} if y is None else None,
                f64=xdt in ("float", "double"))
            continue
        if func in _PAIRED:
            # (n, Σx, Σy, Cxy) over the rows where both arguments are non-null: count and sums of the pair's masked
            # columns, one Cxy word in an op-4 line; corr adds the masked columns' M2 words (the variance machinery)
            if not all(numeric(arg_types[a.key()][0]) for a in arg):
                raise Ineligible(f"{func} type")
            kx, ky = pair_keys(*arg)
            cnt = slot(("count", kx), _MV_COUNT, _MA_ADD_F64)
            sx = slot(("sumf", kx), _MV_F64, _MA_ADD_F64)
            sy = slot(("sumf", ky), _MV_F64, _MA_ADD_F64)
            cxy = slot(("cxy", (kx, ky)), -1, _MA_MOM)
            mom_of[cxy] = (_MOM_CXY, cnt, sx, sy)
            mom_jobs[(kx, ky)] = [kx, ky, cnt, sx, sy, cxy, None]
            states = {"sx": (_F_F64, sx, cnt), "sy": (_F_F64, sy, cnt), "cxy": (_F_F64, cxy, cnt),
                      "cnt": count_of(cnt)}
            m2x = m2y = None
            if func == "corr":
                m2x, m2y = slot(("m2", kx), -1, _MA_M2), slot(("m2", ky), -1, _MA_M2)
                m2_of[m2x], m2_of[m2y] = (cnt, sx), (cnt, sy)
                states.update(m2x=(_F_F64, m2x, cnt), m2y=(_F_F64, m2y, cnt))
            agg(ak, func, cxy, cnt, "double", _MOMENTS[func], states, (m2x, m2y))
            continue
        ck = arg.key()
        dtype, is_f = arg_types[ck]
        if func == "count_if":
            # the predicate mask (NULL counts as false) summed as int64; never NULL, so no count word
            cif = slot(("cif", ck), _MV_I64, _MA_ADD_U64)
            agg(ak, "cif", cif, None, "long", _F_I64, {"cnt": (_F_I64, cif, None)})
            continue
        if func in (*_MOMENTS, *_VARIANCE, "sum") and not numeric(dtype):
            raise Ineligible(f"{func} type")
        dec = dtype if is_decimal(dtype) else None
        if dtype == "string" and func not in ("count", "min", "max"):
            raise Ineligible("argument type")
        cnt = slot(("count", ck), _MV_COUNT, _MA_ADD_F64)
        if func == "count":
            agg(ak, "count", cnt, None, None, _F_COUNT, {"cnt": count_of(cnt)})
        elif dtype == "string":
            # MIN / MAX of a string: one whole line is its order key (six byte words, the length, a spare), which
            # agg_multi leaves at INT64_MIN (value kind -1) and dxa_win_strkey fills
            inv = func == "min"
            job = str_jobs.get((func, ck))
            if job is None:
                job = str_jobs[(func, ck)] = (ck, inv, [slot(("strk", (func, ck), q), -1, _MA_STRKEY)
                                                        for q in range(8)])
            w = job[2]
            flip = _F_NOT if inv else 0
            recipes = [(_F_STRW | flip, w[q], cnt) for q in range(6)] + [(_F_I64 | flip, w[6], cnt)]
            agg(ak, "str", w[0], cnt, "string", recipes, {"v": recipes, "cnt": count_of(cnt)}, f64=False)
        elif func in _MOMENTS or func in _VARIANCE:
            # (n, Σx, M2) of the argument: the count and sum words AVG of the same argument uses, and one M2 word
            # in a line only window_ring.hip combines (MA_M2); agg_multi leaves it at 0.0 (value kind -1) and
            # win_m2_kernel fills it in the pane's second pass
            sm = slot(("sumf", ck), _MV_F64, _MA_ADD_F64)
            m2 = slot(("m2", ck), -1, _MA_M2)
            m2_of[m2] = (cnt, sm)
            states = {"s": (_F_F64, sm, cnt), "m2": (_F_F64, m2, cnt), "cnt": count_of(cnt)}
            if func in _VARIANCE:
                agg(ak, func, m2, cnt, "double", _VARIANCE[func], states)
                continue
            # skewness / kurtosis: and an M3 word (kurtosis: and an M4 word, whose combine reads M3) in an op-4 line
            m3 = slot(("m3", ck), -1, _MA_MOM)
            mom_of[m3] = (_MOM_M3, cnt, sm, m2)
            job = mom_jobs.setdefault(ck, [ck, None, cnt, sm, None, m3, None])
            word = m3
            states["m3"] = (_F_F64, m3, cnt)
            if func == "kurtosis":
                word = job[6] = slot(("m4", ck), -1, _MA_MOM)
                mom_of[word] = (_MOM_M4, cnt, sm, m2, m3)
                states["m4"] = (_F_F64, word, cnt)
            agg(ak, func, word, cnt, "double", _MOMENTS[func], states, (m2, None))
        elif func in ("bmin", "bmax"):
            # bool_and / bool_or: MIN / MAX of the argument as int64, read back as "!= 0"; the partial is the value
            # alone (distagg._partials)
            val = slot((func[1:], ck), _MV_I64 | (_MV_NOT if func == "bmin" else 0), _MA_MAX)
            fkind = _F_I64 | (_F_NOT if func == "bmin" else 0)
            agg(ak, "i64", val, cnt, "boolean", fkind, {"v": (fkind, val, cnt)})
        elif dec is not None and func in ("avg", "sum"):
            # exact: three limb sums in u64 add words that agg_multi leaves at 0 (value kind -1) and win_dec_kernel
            # fills; SUM and AVG of one argument share them; the partial state of both is the sum, of SUM's type
            if dec.precision > SUM_PRECISION:
                raise Ineligible("decimal precision")
            w = [slot((f"dw{q}", ck), -1, _MA_ADD_U64) for q in range(3)]
            dec_jobs[("sum", ck)] = (ck, _DEC_SUM, *w)
            total = two(_F_DEC_SUM, w[0], cnt, w[1], w[2])
            if func == "sum":
                agg(ak, "dsum", w[0], cnt, Dec.result_sum(dec), total, {"v": total, "cnt": count_of(cnt)})
            else:
                agg(ak, "davg", w[0], cnt, Dec.result_avg(dec), two(_F_DEC_AVG, w[0], cnt, w[1], w[2]),
                    {f"davg_{dec.precision}_{dec.scale}": total, "cnt": count_of(cnt)})
        elif dec is not None and not dec.narrow:
            # MIN / MAX of a two-lane decimal: the hi lane in an ordinary MAX slot, the lo lane's order key in a
            # slot of an MA_LOKEY line that agg_multi leaves at INT64_MIN and win_dec_kernel fills
            inv = func == "min"
            hi = slot((func, ck), _MV_I64 | (_MV_NOT if inv else 0), _MA_MAX)
            lo = slot(("lo" + func, ck), -1, _MA_LOKEY)
            lo_of[lo] = hi
            dec_jobs[(func, ck)] = (ck, _DEC_KEY_MIN if inv else _DEC_KEY_MAX, lo, hi, None)
            both = two(_F_DEC_MM | (_F_NOT if inv else 0), hi, cnt, lo, None)
            agg(ak, "dmm", hi, cnt, dec, both, {"v": both, "cnt": count_of(cnt)})
        elif func == "avg":
            sm = slot(("sumf", ck), _MV_F64, _MA_ADD_F64)
            agg(ak, "avg", sm, cnt, "double", _F_AVG, {"s": (_F_F64, sm, cnt), "cnt": count_of(cnt)})
        elif func == "sum":
            val = slot(("sum", ck), _MV_F64 if is_f else _MV_I64, _MA_ADD_F64 if is_f else _MA_ADD_U64)
            fkind = _F_F64 if is_f else _F_I64
            agg(ak, "sum", val, cnt, "double" if is_f else "long", fkind,
                {"v": (fkind, val, cnt), "cnt": count_of(cnt)})
        else:
            val = slot((func, ck), (_MV_F64_ORD if is_f else _MV_I64) | (_MV_NOT if func == "min" else 0), _MA_MAX)
            fkind = (_F_F64_ORD if is_f else _F_I64) | (_F_NOT if func == "min" else 0)
            agg(ak, "f64" if is_f else "i64", val, cnt, dtype, fkind, {"v": (fkind, val, cnt), "cnt": count_of(cnt)},
                f64=is_f)
    order, line_ops = [], []
    if len(dec_jobs) > MAX_DECIMAL:
        raise Ineligible("too many decimal arguments")
    if len(pick_ranks) > MAX_PICK or len(pick_vals) > MAX_PICK:
        raise Ineligible("too many pick arguments")
    if len(str_jobs) > MAX_STRING:
        raise Ineligible("too many string arguments")
    for op in (_MA_ADD_U64, _MA_ADD_F64, _MA_MAX, _MA_M2, _MA_MOM, _MA_LOKEY, _MA_PICK_RANK, _MA_PICK_VAL,
               _MA_STRKEY):
        mine = [i for i, sl in enumerate(slots) if sl[2] == op]
        for k in range(0, len(mine), 8):
            chunk = mine[k:k + 8]
            line_ops.append(op)
            order.extend(chunk + [None] * (8 - len(chunk)))
    if len(order) > 64 or len(fins) > 64:
        raise Ineligible("too many aggregates")
    where = {i: pos for pos, i in enumerate(order) if i is not None}
    nslots = len(order)
    while nslots and order[nslots - 1] is None:
        nslots -= 1
    # the recipes' slots → words (an absent count or operand: -1)
    def words(kind, *ss):
        return (kind, *(-1 if s is None else where[s] for s in ss))

    fin = [words(*f) for f in fins]
    pfin = {ak: {suffix: [words(*h) for h in f] if isinstance(f, list) else words(*f) for suffix, f in states.items()}
            for ak, states in pfins.items()}
    stride = 8 * len(line_ops)
    # per M2 word: its argument's count word | sum word << 16 (win_combine_kernel); the same three words per
    # variance argument for win_m2_kernel
    m2desc = [0] * stride
    m2args = []
    for m2, (c, sm) in m2_of.items():
        m2desc[where[m2]] = where[c] | where[sm] << 16
        m2args.append((slots[m2][0][1], where[c], where[sm], where[m2]))
    dcount_word = {key[1]: where[i] for i, (key, _k, _o) in enumerate(slots) if key[0] == "dcount"}
    out = dict(slots=slots, order=order, nslots=nslots, line_ops=line_ops, stride=stride, plan=plan,
               count_word=where[star], fin=fin, pfin=pfin, m2desc=m2desc, m2args=m2args, dcount_word=dcount_word,
               as_f64=as_f64, rows=rows)
    dsums = {}
    for i, (key, _k, _o) in enumerate(slots):
        if key[0] in ("dsumi", "dsumf"):
            dsums.setdefault(key[1], [-1, -1])[key[0] == "dsumf"] = where[i]
    if dsums:
        # per distinct argument with a SUM / AVG(DISTINCT x): (its integer sum word, its f64 sum word), -1: none
        out["dsum_words"] = {ck: tuple(w) for ck, w in dsums.items()}
    if dec_jobs:
        # per decimal job the words of win_dec_kernel; per low key word its high word (win_combine_kernel)
        out["decargs"] = [(ck, kind, where[w0], where[w1], -1 if w2 is None else where[w2])
                          for ck, kind, w0, w1, w2 in dec_jobs.values()]
    if lo_of:
        lodesc = [0] * stride
        for lo, hi in lo_of.items():
            lodesc[where[lo]] = where[hi] | 1 << 16
        out["lodesc"] = lodesc
    if pick_of:
        # per word of the two pick ops: its R word | (its K word + 1) << 8 | last << 16 | in use (win_combine_kernel);
        # the rank jobs [(K argument key or None, K value kind, K word, R word, last)] and the payload jobs [(x key, R
        # word, P word, V word, last)] of win_pick_kernel / win_pick_gather_kernel
        pickdesc = [0] * stride
        for sl, (r, ks, last) in pick_of.items():
            pickdesc[where[sl]] = where[r] | (0 if ks is None else where[ks] + 1) << 8 | (_PICK_LAST if last else 0) | \
                _PICK_USED
        out["pickdesc"] = pickdesc
        out["pick_x"] = pick_x
        out["pickargs"] = ([(yk, kk or 0, -1 if ks is None else where[ks], where[r], int(last))
                            for r, (yk, kk, ks, last) in pick_ranks.items()],
                           [(xk, where[r], where[pv], where[vv], int(last))
                            for pv, (xk, r, vv, last) in pick_vals.items()])
    if str_jobs:
        # per word of a string line: its place in the line's 7-word tuple + 1 (win_combine_kernel; 0: the spare word);
        # the jobs [(argument key, is MIN, the line's first word)] of dxa_win_strkey.  A job's eight slots are created
        # together, so they fill exactly one line
        strdesc = [0] * stride
        for ck, inv, w in str_jobs.values():
            assert where[w[0]] % 8 == 0 and all(where[w[q]] == where[w[0]] + q for q in range(8))
            for q in range(7):
                strdesc[where[w[q]]] = q + 1
        out["strdesc"] = strdesc
        out["strargs"] = [(ck, inv, where[w[0]]) for ck, inv, w in str_jobs.values()]
    if mom_of:
        # per op-4 word: kind << 24 | the words it reads, 6 bits each (win_combine_kernel); per argument or pair the
        # words of its job in the pane's moment pass (win_mom_kernel)
        momdesc = [0] * stride
        for sl, (kind, *reads) in mom_of.items():
            momdesc[where[sl]] = kind << 24 | sum(where[r] << 6 * q for q, r in enumerate(reads))
        out["momdesc"] = momdesc
        out["momargs"] = [(kx, ky, where[c], where[sx], -1 if sy is None else where[sy], where[w0],
                           -1 if w1 is None else where[w1]) for kx, ky, c, sx, sy, w0, w1 in mom_jobs.values()]
    return out


class PairState:
    """One distinct argument of a statement: the persistent dictionary of its (group id, x) pairs and the presence
    ring ``pres`` — ``uint8 [ring slots][pitch]``, 1 where the slot's pane has a row of the pair.  ``pcap``: the
    dictionary's current capacity; ``rebuilds``: how often it was rebuilt (recycled, grown, or renumbered because
    the group dictionary was).  For count(DISTINCT a, b, …) the "pair" is the tuple (group id, a, b, …): ``keys``
    has one value column per argument after column 0.  ``isum`` / ``fsum``: the words SUM / AVG(DISTINCT x) of this
    argument are folded into (-1: none), read from value column 1."""

    def __init__(self, owner: "DenseWindow", k: int, arg_key):
        self.owner = owner
        self.arg_key = arg_key
        self.pcap = DENSE_PAIRS
        self.pmax = max(DENSE_PAIRS_MAX, DENSE_PAIRS)
        self.rebuilds = 0
        self.full = False               # the last status' "pair dictionary full"
        self.scal_ptr = owner.scal.data_ptr() + 16 * (1 + k)      # this state's counter and flags in the status
        self.word = self.isum = self.fsum = -1
        self.keys = self.pres = None
        self._alloc_table(self.pcap)
        N.call("dxa_win_init", N.ptr(self.htab), N.ptr(self.gid_of_slot), self.hcap, N.stream_handle(owner.device))

    @property
    def pitch(self) -> int:
        return _pitch(self.pcap)

    def _alloc_table(self, pcap: int) -> None:
        self.hcap = _table_slots(pcap)
        self.htab = torch.empty(self.hcap, dtype=torch.int64, device=self.owner.device)
        self.gid_of_slot = torch.empty(self.hcap, dtype=torch.int32, device=self.owner.device)

    def _bytes(self, pcap: int) -> int:
        o = self.owner
        x = 8 + 1 if self.keys is None else sum((_sizes()[2] + 4 if k[1] == 2 else 8) + 1 for k in self.keys[1:])
        return (o.R + o.NB) * _pitch(pcap) + (pcap + 1) * (9 + x) + 12 * _table_slots(pcap)

    def build(self, xs: List, word: int, sums=(-1, -1)) -> None:
        """Key columns (parent id, x[, …]) and the zeroed presence ring, once the first pane shows the types."""
        o = self.owner
        kinds = [(x.dtype, 2 if isinstance(x, StrColumn) else 1 if x.data.dtype == torch.float64 else 0) for x in xs]
        self.word = word
        self.isum, self.fsum = sums
        self.keys, self.dictcols = o._alloc_keys([("long", 0), *kinds], self.pcap)
        self.pres = torch.zeros((o.R + o.NB, self.pitch), dtype=torch.uint8, device=o.device)

    def insert(self, gid: torch.Tensor, n: int, xs: List, slot_idx: int, st) -> None:
        """The pane's rows into the pair dictionary (the group insert kernel, with the rows' group ids as key
        column 0) and the pairs they drew into presence row ``slot_idx``.  A row with a NULL in any of ``xs`` creates
        no pair: the validities are ANDed once."""
        o = self.owner
        dev = o.device
        gid64 = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        keep = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        pid = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        v = xs[0].valid
        for x in xs[1:]:
            if x.valid is not None:
                v = x.valid.to(torch.bool) if v is None else v.to(torch.bool) & x.valid.to(torch.bool)
        v = N.u8(v)
        if v is not None:
            v = v.contiguous()
        N.call("dxa_win_pair_prep", N.ptr(gid), n, o.gcap, N.ptr(v), N.ptr(gid64), N.ptr(keep), st)
        kc = key_cols([PrimColumn("long", gid64), *xs])
        if kc is None:
            raise Ineligible("argument columns")
        kc.ncols, kc.n = 1 + len(xs), n
        N.call("dxa_win_insert_fused", ctypes.addressof(kc), ctypes.addressof(self.dictcols), N.ptr(keep),
               N.ptr(self.htab), self.hcap, N.ptr(self.gid_of_slot), self.scal_ptr, N.ptr(pid), st)
        N.call("dxa_win_pair_mark", N.ptr(pid), n, self.pcap, N.ptr(self.pres), self.pitch, slot_idx, st)

    def rebuild(self, slots: List[int], remap: Optional[torch.Tensor], grow: bool) -> None:
        """Renumber the pairs over those with a byte set in the held pane slots ``slots`` (``DenseWindow.rebuild``
        dropped the dirty panes and cleared the block cache): key columns and presence columns gathered into
        fresh tensors — column 0 through ``remap`` when the group ids were renumbered; a live pair has rows in a
        held pane, so its group is live too — and the table refilled.  Off the hot path: torch indexing and one
        host read (the live count).  Raises ``Ineligible`` ("pair dictionary full" / "memory")."""
        o = self.owner
        dev = o.device
        if grow and self.pcap >= self.pmax:
            raise Ineligible("pair dictionary full")
        sl = torch.tensor(slots, dtype=torch.int64, device=dev)
        idx = torch.nonzero(self.pres[sl, :self.pcap].any(dim=0)).flatten()
        live = int(idx.shape[0])
        target = _target_capacity(live, self.pcap, self.pmax)
        if grow:
            target = min(max(target, 2 * self.pcap), self.pmax)
        try:
            if target != self.pcap and self._bytes(target) > torch.cuda.mem_get_info(dev)[0] // 2:
                raise Ineligible("memory")
            keys, dc = o._alloc_keys([(k[0], k[1]) for k in self.keys], target)
            pres = torch.zeros((o.R + o.NB, _pitch(target)), dtype=torch.uint8, device=dev)
            if target != self.pcap:
                self._alloc_table(target)
        except torch.cuda.OutOfMemoryError:
            raise Ineligible("memory") from None
        kw = _sizes()[2]
        for (_dt, kind, vals, lens, valid), (_d2, _k2, nvals, nlens, nvalid) in zip(self.keys, keys):
            if kind == 2:
                nvals.view(target + 1, kw)[:live] = vals.view(self.pcap + 1, kw)[idx]
                nlens[:live] = lens[idx]
            else:
                nvals[:live] = vals[idx]
            nvalid[:live] = valid[idx]
        if remap is not None:
            parents = keys[0][2]
            parents[:live] = remap[parents[:live].clamp(0, remap.shape[0] - 1)]
        pres[sl, :live] = self.pres[sl][:, idx]
        self.keys, self.dictcols, self.pres, self.pcap = keys, dc, pres, target
        N.call("dxa_win_rehash", ctypes.addressof(dc), N.ptr(self.htab), N.ptr(self.gid_of_slot), self.hcap, live,
               self.scal_ptr, N.stream_handle(dev))
        self.full = False
        self.rebuilds += 1


class DenseWindow:
    """Persistent state of one windowed statement (one fingerprint) on one device.  ``gcap``: the dictionary's
    current capacity; ``rebuilds``: how often it was rebuilt; ``disabled_reason``: None while the statement is
    answered here, else why it went to the paned path for good."""

    def __init__(self, device, reqs, ring_slots: int, global_form: bool = False):
        self.device = device
        self.reqs = reqs
        self.global_form = global_form  # no GROUP BY: one group under a constant key that is not emitted
        self._rebuilt: set = set()      # dictionaries rebuilt so far in the current dense_answer call
        self.gcap = DENSE_GROUPS
        self.gmax = max(DENSE_GROUPS_MAX, DENSE_GROUPS)
        self.rebuilds = 0
        self.disabled_reason: Optional[str] = None
        # The three fields below belong to the one answer in flight: they assume that a deferred answer is completed
        # (its ``finish`` run) before the next ``dense_answer`` for this fingerprint, which the processor guarantees
        # (it completes every pending table at the end of the batch's statements).  A deferred answer that is
        # dropped without being completed leaves ``dirty`` growing by one key per batch until the next clean status.
        self.rebuild_pending = False    # the last status read "dictionary full" and nothing else
        self.bad = 0                    # the last status' flags
        self.dirty: List[int] = []      # keys of the panes accumulated since the last clean status
        self.R = ring_slots + SCRATCH_SLOTS
        self.NB = ring_slots // BLOCK + 4              # block slots after the pane and scratch slots
        self.blocks: Dict[int, tuple] = {}             # block id → (member entry ids, block slot, entries)
        self.layout = None              # built from the first pane's evaluated argument types
        self.m2desc_t = self.m2desc_dev = None  # with variance arguments: win_combine_kernel's M2 descriptor
        self.momdesc_t = self.momdesc_dev = None        # with op-4 lines: its M3 / M4 / Cxy descriptor
        self.lodesc_t = self.lodesc_dev = None          # with low-key lines (two-lane decimal MIN / MAX): the high words
        self.pickdesc_t = self.pickdesc_dev = None      # with row picks: the R and K word of each pick word
        self.strdesc_t = self.strdesc_dev = None        # with string MIN / MAX lines: each word's place in its tuple
        # row picks combine slots by their place in the window's row order (``_enqueue``)
        self.has_picks = any(func in _PICKS for _, func, _arg in reqs)
        self.slot_of: Dict[int, tuple] = {}     # pane key → (ring slot, the pane, block id, pane key)
        self.free = list(range(ring_slots))    # free pane slots (a heap: the lowest is taken first)
        self.disabled = False
        # pinned staging rows for slot lists (_dev_slots), used in rotation and never waited for: one pass over the
        # window uploads at most one list per block slot (all of them right after a rebuild, which clears the block
        # cache) and one for the answer, a rebuild one more, and every pass and every rebuild ends in a status read
        # that drains the stream before the next begins — so NB + 2 rows are never rewritten while a copy is queued
        self._pinned = torch.empty((self.NB + 2, self.R), dtype=torch.int32, pin_memory=True)
        dkeys = []
        for _, func, arg in reqs:
            if func in _DISTINCT and distinct_key(arg) not in dkeys:
                dkeys.append(distinct_key(arg))
        nstat = 4 + 4 * len(dkeys)      # the outer status, then counter / flags / 2 pads per pair state
        self._scal_pin = [torch.empty(nstat, dtype=torch.int32, pin_memory=True) for _ in range(2)]
        self._scal_k = 0
        self._pin_k = 0
        cap = _table_slots(self.gcap)
        self.hcap = cap
        dev = device
        self.htab = torch.empty(cap, dtype=torch.int64, device=dev)
        self.gid_of_slot = torch.empty(cap, dtype=torch.int32, device=dev)
        self.scal = torch.zeros(nstat, dtype=torch.int32, device=dev)     # groups, bad flags, kept, pad[, pair states]
        N.call("dxa_win_init", N.ptr(self.htab), N.ptr(self.gid_of_slot), cap, N.stream_handle(dev))
        # one pair state per different distinct argument (or argument tuple), in order of first appearance
        self.pairs: List[PairState] = [PairState(self, k, dk) for k, dk in enumerate(dkeys)]
        self.keys = None                # dictionary key columns, built with the layout
        self.ring = None

    # ---- layout -------------------------------------------------------------------------------------------------
    def _alloc_keys(self, kinds: List[tuple], gcap: int):
        """Zero-filled dictionary key columns for ``gcap`` groups and the dump row → (keys, kernel descriptor)."""
        kw = _sizes()[2]
        dev = self.device
        dc = _DictCols()
        keys = []
        for j, (dtype, kind) in enumerate(kinds):
            if kind == 2:
                vals = torch.zeros((gcap + 1) * kw, dtype=torch.uint8, device=dev)
                lens = torch.zeros(gcap + 1, dtype=torch.int32, device=dev)
            else:
                vals = torch.zeros(gcap + 1, dtype=torch.int64, device=dev)
                lens = None
            valid = torch.zeros(gcap + 1, dtype=torch.uint8, device=dev)
            keys.append((dtype, kind, vals, lens, valid))
            dc.c[j] = _DictCol(vals.data_ptr(), 0 if lens is None else lens.data_ptr(), valid.data_ptr(), kind, 0)
        dc.ncols, dc.gcap = len(keys), gcap
        return keys, dc

    def _alloc_ring(self, gcap: int):
        """Ring, combined rows, keep flags and kept ids for ``gcap`` groups (the slot pitch is (gcap + 1) rows)."""
        dev = self.device
        rows = gcap + 1
        ring = torch.empty((self.R + self.NB, rows * self.stride), dtype=torch.int64, device=dev)
        acc = torch.zeros(rows * self.stride, dtype=torch.int64, device=dev)
        keep = torch.empty(gcap, dtype=torch.uint8, device=dev)
        out_idx = torch.empty(gcap, dtype=torch.int64, device=dev)
        return ring, acc, keep, out_idx

    def _bytes(self, gcap: int) -> int:
        """Device bytes of the ring, key columns and table at capacity ``gcap`` (what a growing rebuild allocates)."""
        kw = _sizes()[2]
        rows = gcap + 1
        total = (self.R + self.NB + 1) * rows * self.stride * 8 + 9 * gcap + 12 * _table_slots(gcap)
        for _dt, kind, *_ in self.keys:
            total += rows * ((kw + 4 if kind == 2 else 8) + 1)
        return total + sum(ps._bytes(ps.pcap) for ps in self.pairs)

    def _build_layout(self, key_cols_in: List, args: Dict, dargs: Dict):
        if not 1 <= len(key_cols_in) <= MAX_KEY_COLS:
            raise Ineligible("key count")
        kinds = [(k.dtype, 2 if isinstance(k, StrColumn) else 1 if k.data.dtype == torch.float64 else 0)
                 for k in key_cols_in]
        try:
            self.keys, self.dictcols = self._alloc_keys(kinds, self.gcap)
        except torch.cuda.OutOfMemoryError:
            raise Ineligible("memory") from None
        types = {k: (c.dtype, isinstance(c, PrimColumn) and c.data.dtype == torch.float64) for k, c in args.items()}
        for _, func, arg in self.reqs:
            if func in ("dsum", "davg"):        # the distinct sums' arguments, as ``_distinct_arg`` widened them
                c = dargs[arg.key()][0]
                types.setdefault(arg.key(), (c.dtype, isinstance(c, PrimColumn) and c.data.dtype == torch.float64))
        L = plan_layout(self.reqs, types)
        L["pspec_of"] = self._partial_spec
        # payload arguments stored as float32: their picks are kept as doubles and narrowed again in ``_finals``
        self.f32_args = {k for k, c in args.items() if isinstance(c, PrimColumn) and c.data.dtype == torch.float32}
        self.stride = L["stride"]
        self.layout = L
        # agg_multi (host ``line_ops_t``) sees an M2 line as an f64 add line of unused slots, so every pane starts
        # its M2 words at 0.0; the ring kernels (``line_ops_dev``) see MA_M2
        # and a low-key line as a max line of unused slots, so every pane starts its low key words at INT64_MIN; so do
        # a pick's rank words and the words of a string order key, and a pick's payload and validity words start at 0 as
        # unused u64 add words
        host_op = {_MA_M2: _MA_ADD_F64, _MA_MOM: _MA_ADD_F64, _MA_LOKEY: _MA_MAX, _MA_PICK_RANK: _MA_MAX,
                   _MA_PICK_VAL: _MA_ADD_U64, _MA_STRKEY: _MA_MAX}
        self.line_ops_t = torch.tensor([host_op.get(op, op) for op in L["line_ops"]], dtype=torch.int32)
        self.line_ops_dev = torch.tensor(L["line_ops"], dtype=torch.int32).to(self.device)
        self.m2desc_t = self.m2desc_dev = None
        self.momdesc_t = self.momdesc_dev = None
        self.lodesc_t = self.lodesc_dev = None
        self.pickdesc_t = self.pickdesc_dev = None
        self.strdesc_t = self.strdesc_dev = None
        if "strdesc" in L:
            self.strdesc_t = torch.tensor(L["strdesc"], dtype=torch.int32)
            self.strdesc_dev = self.strdesc_t.to(self.device)
        if "pickdesc" in L:
            self.pickdesc_t = torch.tensor(L["pickdesc"], dtype=torch.int32)
            self.pickdesc_dev = self.pickdesc_t.to(self.device)
        if "lodesc" in L:
            self.lodesc_t = torch.tensor(L["lodesc"], dtype=torch.int32)
            self.lodesc_dev = self.lodesc_t.to(self.device)
        if L["m2args"] or "momdesc" in L:
            self.m2desc_t = torch.tensor(L["m2desc"], dtype=torch.int32)
            self.m2desc_dev = self.m2desc_t.to(self.device)
        if "momdesc" in L:
            # the combine of a layout with op-4 lines takes both descriptors (``m2desc`` all zero without M2 words)
            self.momdesc_t = torch.tensor(L["momdesc"], dtype=torch.int32)
            self.momdesc_dev = self.momdesc_t.to(self.device)
        try:
            self.ring, self.acc, self.keep, self.out_idx = self._alloc_ring(self.gcap)
            for ps in self.pairs:
                ps.build(dargs[ps.arg_key], L["dcount_word"][ps.arg_key],
                         L.get("dsum_words", {}).get(ps.arg_key, (-1, -1)))
        except torch.cuda.OutOfMemoryError:
            self.layout = None
            raise Ineligible("memory") from None

    # ---- a full dictionary: recycle the ids of groups that left the window, grow when most are still live ------
    def release_expired(self, retained) -> None:
        """Ring slots of panes the store no longer retains go back to the free heap."""
        for k in [k for k in self.slot_of if k not in retained]:
            heapq.heappush(self.free, self.slot_of.pop(k)[0])

    def rebuild(self, retained, grow: bool) -> None:
        """Renumber the dictionary over the groups that still have rows in held panes (module docstring); raises
        ``Ineligible`` ("dictionary full" / "memory") when the statement has to leave the dense path.

        ``grow``: an earlier rebuild in this call was not enough (re-accumulating the dropped panes overflowed
        again), so the capacity has to double.  One host read (the live count).  Key columns always move into fresh
        tensors: output strings of earlier batches are views of the old arena and may still be rendering.  Peak
        extra memory: at an unchanged capacity only those key columns — each held pane slot is compacted through
        one of the ring's own scratch slots (refilled every batch, so dead here); when the capacity grows the ring's
        pitch changes, so a whole new ring, table and result buffers exist beside the old ones until the gather
        has been queued (checked against half the free memory first).  Block slots are not remapped: the block
        cache is cleared and complete blocks are combined again on next use."""
        self.rebuild_pending = False
        # with distinct counts the status says which dictionaries are full: the group dictionary is rebuilt only
        # when it is, a pair dictionary when it is or when the group ids it is keyed by were renumbered.  ``grow``
        # applies to a dictionary that this call already rebuilt once.
        outer_full = bool(self.bad & 2) or not self.pairs
        done = self._rebuilt
        grow_outer = grow and (not self.pairs or "outer" in done)
        if outer_full and grow_outer and self.gcap >= self.gmax:
            raise Ineligible("dictionary full")
        # panes accumulated since the last clean status sent some rows to the dump row: the caller's pane loop
        # accumulates them again after the rebuild
        for k in self.dirty:
            ent = self.slot_of.pop(k, None)
            if ent is not None:
                heapq.heappush(self.free, ent[0])
        self.dirty = []
        self.blocks.clear()
        self.release_expired(retained)
        slots = sorted(e[0] for e in self.slot_of.values())
        remap = None
        if outer_full:
            remap = self._rebuild_groups(slots, grow_outer)
            done.add("outer")
        for ps in self.pairs:
            if outer_full or ps.full:
                ps.rebuild(slots, remap, grow and ps in done)
                done.add(ps)

    def _rebuild_groups(self, slots: List[int], grow: bool) -> Optional[torch.Tensor]:
        """``rebuild``'s renumbering of the group dictionary over the held pane slots ``slots``.  With pair states:
        → the map old group id → new id (-1: dropped), for their key column 0."""
        L = self.layout
        dev = self.device
        st = N.stream_handle(dev)
        N.call("dxa_win_live", N.ptr(self.ring), self.gcap, self.stride, N.ptr(self._dev_slots(slots)), len(slots),
               N.ptr(self.line_ops_dev), L["count_word"], N.ptr(self.scal), N.ptr(self.acc), N.ptr(self.keep),
               N.ptr(self.out_idx), st)
        live = int(self.scal[2])
        target = _target_capacity(live, self.gcap, self.gmax)
        if grow:
            target = min(max(target, 2 * self.gcap), self.gmax)
        grown = target != self.gcap
        try:
            if grown and self._bytes(target) > torch.cuda.mem_get_info(dev)[0] // 2:
                raise Ineligible("memory")
            keys, dc = self._alloc_keys([(k[0], k[1]) for k in self.keys], target)
            ring, acc, keep, out_idx, htab, gid_of_slot, hcap = (self.ring, self.acc, self.keep, self.out_idx,
                                                                 self.htab, self.gid_of_slot, self.hcap)
            if grown:
                ring, acc, keep, out_idx = self._alloc_ring(target)
                hcap = _table_slots(target)
                htab = torch.empty(hcap, dtype=torch.int64, device=dev)
                gid_of_slot = torch.empty(hcap, dtype=torch.int32, device=dev)
        except torch.cuda.OutOfMemoryError:
            raise Ineligible("memory") from None
        N.call("dxa_win_remap_dict", ctypes.addressof(self.dictcols), ctypes.addressof(dc), N.ptr(self.out_idx), live,
               st)
        host_slots = (ctypes.c_int32 * max(1, len(slots)))(*slots)
        N.call("dxa_win_remap_ring", N.ptr(self.ring), N.ptr(ring), self.gcap, target, self.stride,
               ctypes.addressof(host_slots), len(slots), self.R - 1, N.ptr(self.line_ops_dev), N.ptr(self.out_idx),
               live, st)
        N.call("dxa_win_rehash", ctypes.addressof(dc), N.ptr(htab), N.ptr(gid_of_slot), hcap, live, N.ptr(self.scal),
               st)
        remap = None
        if self.pairs:
            remap = torch.full((self.gcap + 1,), -1, dtype=torch.int64, device=dev)
            remap[self.out_idx[:live]] = torch.arange(live, dtype=torch.int64, device=dev)
        self.keys, self.dictcols, self.gcap = keys, dc, target
        self.ring, self.acc, self.keep, self.out_idx = ring, acc, keep, out_idx
        self.htab, self.gid_of_slot, self.hcap = htab, gid_of_slot, hcap
        self.rebuilds += 1
        return remap

    # ---- one pane into one ring slot ----------------------------------------------------------------------------
    def accumulate(self, table, slot_idx: int, alias, where, gexprs, ctx):
        from .expr import Scope, evaluate, predicate_mask
        scope = Scope.of_table(table, alias)
        n = scope.length
        keep = None
        if where is not None:
            keep = N.u8(predicate_mask(evaluate(where, scope, ctx)).contiguous())
        keys = []
        for g in gexprs:
            k = materialize(evaluate(g, scope, ctx))
            if isinstance(k, PrimColumn):
                if is_decimal(k.dtype) or k.data.dim() != 1:
                    raise Ineligible("key type")
                if k.data.dtype == torch.bool:
                    k = PrimColumn(k.dtype, k.data.to(torch.int64), k.valid)
                elif k.data.dtype not in (torch.int64, torch.float64):
                    k = PrimColumn(k.dtype, k.data.to(torch.int64), k.valid)
            elif not isinstance(k, StrColumn) or type(k) is not StrColumn:
                raise Ineligible("key type")
            keys.append(k)
        if self.global_form:
            keys = [PrimColumn("long", torch.zeros(n, dtype=torch.int64, device=self.device))]
        args, dargs = {}, {}
        for _, func, arg in self.reqs:
            if func in _DISTINCT:
                if distinct_key(arg) not in dargs:
                    dargs[distinct_key(arg)] = [_distinct_arg(evaluate(a, scope, ctx))
                                                for a in (arg if isinstance(arg, tuple) else (arg,))]
                continue
            for a in arg if isinstance(arg, tuple) else () if arg is None else (arg,):
                # an argument evaluated for an earlier aggregate is checked again against this one's func: COUNT(name)
                # admits a string column that SUM(name) of the same statement must still refuse
                c = args.get(a.key())
                if c is None:
                    c = evaluate(a, scope, ctx)
                    if isinstance(c, ConstColumn):
                        c = c.materialize()
                if type(c) is StrColumn and c.dtype == "string":
                    # a plain string column: COUNT reads its validity, MIN / MAX keep its order key; nothing else
                    if func not in ("count", "min", "max"):
                        raise Ineligible("argument type")
                # a decimal argument keeps its storage: one int64 lane per row, or two for more than 18 digits
                elif not isinstance(c, PrimColumn) or \
                        c.data.dim() != (2 if is_decimal(c.dtype) and not c.dtype.narrow else 1):
                    raise Ineligible("argument type")
                args[a.key()] = c
            if func in ("max_by", "min_by"):
                # a double order key: the copy with -0.0 → 0.0 that the pick's K slot and win_pick_kernel read
                y = args[arg[1].key()]
                if y.dtype in ("float", "double") and pick_y_key(arg[1]) not in args:
                    d = y.data.to(torch.float64)
                    args[pick_y_key(arg[1])] = PrimColumn("double", torch.where(d == 0.0, torch.zeros_like(d), d),
                                                          y.valid)
            elif isinstance(arg, tuple) and pair_keys(*arg)[0] not in args:
                # a pair's columns: the arguments' data under the validity "both non-null", built once per pane
                x, y = args[arg[0].key()], args[arg[1].key()]
                both = x.valid if y.valid is None else y.valid if x.valid is None else \
                    x.valid.to(torch.bool) & y.valid.to(torch.bool)
                kx, ky = pair_keys(*arg)
                args[kx], args[ky] = PrimColumn(x.dtype, x.data, both), PrimColumn(y.dtype, y.data, both)
        # the arguments whose type shapes the layout: decimals (their words and win_dec_kernel's lanes follow the type)
        # and strings (their MIN / MAX have lines of their own)
        shaping_types = {k: str(c.dtype) for k, c in args.items() if is_decimal(c.dtype) or isinstance(c, StrColumn)}
        if self.layout is None:
            self._build_layout(keys, args, dargs)
            self.shaping_types = shaping_types
        else:
            if shaping_types != self.shaping_types:
                raise Ineligible("argument types changed")
            for (dt, kind, *_), k in zip(self.keys, keys):
                if (kind == 2) != isinstance(k, StrColumn) or str(dt) != str(k.dtype):
                    raise Ineligible("key types changed")
            for ps in self.pairs:
                for (dt, kind, *_), k in zip(ps.keys[1:], dargs[ps.arg_key]):
                    if (kind == 2) != isinstance(k, StrColumn) or str(dt) != str(k.dtype):
                        raise Ineligible("argument types changed")
        L = self.layout
        dev = self.device
        st = N.stream_handle(dev)
        kc = key_cols(keys)
        if kc is None:
            raise Ineligible("key columns")
        kc.ncols, kc.n = len(keys), n
        gid = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        # hash + dictionary lookup / claim + key store + verify: one launch (window_ring.hip win_insert_kernel)
        N.call("dxa_win_insert_fused", ctypes.addressof(kc), ctypes.addressof(self.dictcols), N.ptr(keep),
               N.ptr(self.htab), self.hcap, N.ptr(self.gid_of_slot), N.ptr(self.scal), N.ptr(gid), st)
        spec, hold = [], [gid, keep, kc]
        xs = {}                         # variance arguments: the (float64 values, validity) their sum slot reads
        # with row picks: word → the (values, validity) agg_multi reads for it (win_pick_kernel reads a K word's)
        fed = {} if "pickargs" in L else None
        for pos, i in enumerate(L["order"][:L["nslots"]]):
            if i is None:
                spec += [0, 0, -1]
                continue
            key, kind, _op = L["slots"][i]
            if kind == -1 or key[0] == "dcount":   # filled after agg_multi: the distinct fold / win_m2 / win_mom
                spec += [0, 0, -1]
                continue
            if key[1] is None:
                spec += [0, 0, kind]
                continue
            c = args[key[1]]
            if key[0] == "cif":                    # count_if: the predicate mask as int64, NULL → 0
                d = predicate_mask(c).to(torch.int64).contiguous()
                hold.append(d)
                spec += [d.data_ptr(), 0, kind]
                continue
            v = N.u8(c.valid)
            if v is not None:
                v = v.contiguous()
            if key[0] == "count":                  # a count reads only the validity: no value conversion
                hold.append(v)
                spec += [0, 0 if v is None else v.data_ptr(), kind]
                continue
            d = c.data
            if key[0] == "sumf" or (kind & 3) in (_MV_F64, _MV_F64_ORD):
                # (a decimal in the f64 families: the double Spark's cast gives)
                d = Dec.to_double(c).data if is_decimal(c.dtype) else d.to(torch.float64)
            elif d.dim() == 2:                     # MIN / MAX of a two-lane decimal: the high key is the hi lane
                d = d[:, 1]
            elif d.dtype != torch.int64:
                d = d.to(torch.int64)
            d = d.contiguous()
            hold += [d, v]
            if key[0] == "sumf":
                xs[key[1]] = (d, v)
            if fed is not None:
                fed[pos] = (d, v)
            spec += [d.data_ptr(), 0 if v is None else v.data_ptr(), kind]
        spec_t = torch.tensor(spec, dtype=torch.int64)
        ring_ptr = self.ring[slot_idx].data_ptr()
        N.call("dxa_aggregate_multi", N.ptr(gid), n, self.gcap + 1, L["nslots"], spec_t.data_ptr(),
               len(L["line_ops"]), self.line_ops_t.data_ptr(), ring_ptr, st)
        if L["m2args"] and n > 0:
            # the pane's second pass: the slot's counts and sums are complete, so every row's distance from its
            # group's mean goes into the M2 words (window_ring.hip win_m2_kernel), all variance arguments at once
            m = _M2Args()
            for k, (ck, cw, sw, mw) in enumerate(L["m2args"]):
                d, v = xs[ck]
                m.a[k] = _M2Arg(d.data_ptr(), 0 if v is None else v.data_ptr(), cw, sw, mw, 0)
            N.call("dxa_win_m2", self._second_pass(m, len(L["m2args"]), gid, ring_ptr, n), st)
        if L.get("momargs") and n > 0:
            # and the M3 / M4 / Cxy words from the same counts and sums (win_mom_kernel): one sweep per argument or pair
            m = _MomArgs()
            for k, (kx, ky, cw, sw, syw, w0, w1) in enumerate(L["momargs"]):
                d, v = xs[kx]
                m.a[k] = _MomArg(d.data_ptr(), 0 if ky is None else xs[ky][0].data_ptr(),
                                 0 if v is None else v.data_ptr(), cw, sw, syw, w0, w1, 0)
            N.call("dxa_win_mom", self._second_pass(m, len(L["momargs"]), gid, ring_ptr, n), st)
        if L.get("decargs") and n > 0:
            # the decimal pass: limb sums and low key words straight from the decimal columns' storage (win_dec_kernel
            # reads them in place with a lane stride of 1 or 2), all of the statement's jobs in one launch
            m = _DecArgs()
            for k, (ck, kind, w0, w1, w2) in enumerate(L["decargs"]):
                c = args[ck]
                d = c.data.contiguous()
                v = N.u8(c.valid)
                if v is not None:
                    v = v.contiguous()
                hold += [d, v]
                m.a[k] = _DecJob(d.data_ptr(), 0 if v is None else v.data_ptr(), d.dim(), kind, w0, w1, w2, 0)
            N.call("dxa_win_dec", self._second_pass(m, len(L["decargs"]), gid, ring_ptr, n), st)
        if L.get("pickargs") and n > 0:
            # the pick pass: the rank words from the finished key words (win_pick_kernel reads the very arrays agg_multi
            # read for them), then every payload argument's bits and validity at the winning rows, all jobs of the
            # statement in two launches of one call
            m = _PickArgs()
            ranks, vals = L["pickargs"]
            for k, (yk, kind, kw, rw, last) in enumerate(ranks):
                d, v = fed[kw] if yk is not None else (None, None)
                m.rank[k] = _PickRank(0 if d is None else d.data_ptr(), 0 if v is None else v.data_ptr(), kind, kw, rw,
                                      last)
            bits = {}
            for k, (xk, rw, pw, vw, last) in enumerate(vals):
                if xk not in bits:
                    c = args[xk]
                    d = c.data
                    d = d.to(torch.float64) if d.dtype == torch.float32 else d if d.dtype in (
                        torch.int64, torch.float64) else d.to(torch.int64)
                    v = N.u8(c.valid)
                    bits[xk] = (d.contiguous(), None if v is None else v.contiguous())
                d, v = bits[xk]
                m.val[k] = _PickVal(d.data_ptr(), 0 if v is None else v.data_ptr(), rw, pw, vw, last)
            hold.append(bits)
            m.gid, m.row, m.scal, m.n = gid.data_ptr(), ring_ptr, self.scal.data_ptr(), n
            m.gcap, m.stride, m.nrank, m.nval = self.gcap, self.stride, len(ranks), len(vals)
            N.call("dxa_win_pick", ctypes.addressof(m), st)
        if L.get("strargs") and n > 0:
            # the string pass: per job the pane's winning row per group (str_minmax.hip, under the pane's ids and WHERE
            # mask), then every job's packed order key into its line, all jobs of the statement in one call
            m = _StrKeyArgs()
            jobs = L["strargs"]
            best = torch.empty((len(jobs), self.gcap), dtype=torch.int64, device=dev)
            for k, (ck, inv, line) in enumerate(jobs):
                c = args[ck]
                v = N.u8(c.valid)
                parts = (c.arena, c.starts.contiguous(), c.lens.contiguous(), None if v is None else v.contiguous())
                hold.append(parts)
                m.a[k] = _StrJob(*(N.ptr(t) or None for t in parts), line, int(inv))
            hold.append(best)
            m.gid, m.keep, m.row, m.scal = gid.data_ptr(), N.ptr(keep) or None, ring_ptr, self.scal.data_ptr()
            m.best, m.n = best.data_ptr(), n
            m.gcap, m.stride, m.njobs = self.gcap, self.stride, len(jobs)
            N.call("dxa_win_strkey", ctypes.addressof(m), st)
        for ps in self.pairs:
            ps.insert(gid, n, dargs[ps.arg_key], slot_idx, st)
        del hold

    def _descs(self):
        """The combine's descriptors for ``dxa_win_answer`` / ``dxa_win_combine_block``: ``m2desc`` on the device and
        on the host, ``momdesc``, ``lodesc``, ``pickdesc`` and ``strdesc`` likewise; 0 where the layout has none, which
        picks the combine without that branch."""
        return (N.ptr(self.m2desc_dev), N.ptr(self.m2desc_t), N.ptr(self.momdesc_dev), N.ptr(self.momdesc_t),
                N.ptr(self.lodesc_dev), N.ptr(self.lodesc_t), N.ptr(self.pickdesc_dev), N.ptr(self.pickdesc_t),
                N.ptr(self.strdesc_dev), N.ptr(self.strdesc_t))

    def _second_pass(self, m, nargs: int, gid: torch.Tensor, ring_ptr: int, n: int) -> int:
        """The fields ``_M2Args`` and ``_MomArgs`` share, after their jobs: the pane's group ids and ring slot → the
        descriptor's address."""
        m.gid, m.row, m.n = gid.data_ptr(), ring_ptr, n
        m.gcap, m.stride, m.nargs = self.gcap, self.stride, nargs
        return ctypes.addressof(m)

    def _dev_slots(self, slots: List[int]) -> torch.Tensor:
        pin = self._pinned[self._pin_k]
        self._pin_k = (self._pin_k + 1) % self._pinned.shape[0]
        pin[:len(slots)] = torch.tensor(slots, dtype=torch.int32)
        return pin[:len(slots)].to(self.device, non_blocking=True)

    def block_slot(self, bid: int, mem: list) -> int:
        """The ring slot holding the pre-combined rows of a complete block of panes (combined once, when the block
        is first complete in a window; reused until a member leaves).  ``mem``: the members' slot entries."""
        # members by the identity of their slot entries: an entry is made once per pane assignment and lives in
        # slot_of while the pane is retained; the cache holds the entries too, so no id is reused while cached
        # (row picks: in the order given — the window's row order — and combined again should that order change)
        members = tuple(map(id, mem)) if self.has_picks else frozenset(map(id, mem))
        ent = self.blocks.get(bid)
        if ent is not None and ent[0] == members:
            return ent[1]
        used = {b[1] for k, b in self.blocks.items() if k != bid}
        free = [s for s in range(self.R, self.R + self.NB) if s not in used]
        if not free:
            raise Ineligible("block slots")
        dst = free[0]
        member_slots = [e[0] for e in (mem if self.has_picks else sorted(mem, key=lambda e: e[3]))]
        slots_dev = self._dev_slots(member_slots)
        st = N.stream_handle(self.device)
        N.call("dxa_win_combine_block", N.ptr(self.ring), self.gcap, self.stride, N.ptr(slots_dev), len(member_slots),
               N.ptr(self.line_ops_dev), dst, N.ptr(self.scal), *self._descs(), st)
        for ps in self.pairs:       # the members' presence rows ORed into the same block slot of the presence ring
            N.call("dxa_win_pair_or_block", N.ptr(ps.pres), ps.pitch, N.ptr(slots_dev), len(member_slots), dst, st)
        self.blocks[bid] = (members, dst, list(mem))
        return dst

    # ---- the window's answer --------------------------------------------------------------------------------------
    def answer(self, slots: List[int], partial_proto=None, defer: bool = False):
        """Combine ``slots`` → (key columns, {agg key → column}, groups), or None: a collision or an over-long key
        (the caller falls back for good) or a full dictionary (the caller rebuilds it and asks again).
        With ``partial_proto`` (an empty partial table of ``distagg.local_partials``' layout, and its plan) the
        result is instead this rank's window as a partial table of exactly that layout, for the key exchange.
        ``defer``: return a function that completes the answer later — the kernels are queued and the status is on
        its way to pinned memory, so the batch thread can plan independent statements while they run."""
        L = self.layout
        dev = self.device
        st = N.stream_handle(dev)
        slots_dev = self._dev_slots(slots)
        fin = L["pspec_of"](partial_proto) if partial_proto is not None else L["fin"]
        e, bufs = self._emit_args(fin)
        folds = None
        if self.pairs:
            # the same launches with one distinct fold per pair state between the combine and the keep pass
            folds = _PairFolds()
            for k, ps in enumerate(self.pairs):
                folds.p[k] = _PairFold(ps.pres.data_ptr(), ps.pitch, ps.keys[0][2].data_ptr(), ps.scal_ptr, ps.pcap,
                                       ps.word, ps.keys[1][2].data_ptr(), ps.keys[1][1], ps.isum, ps.fsum, 0)
            folds.n = len(self.pairs)
        # combine (the instantiation the layout's descriptors call for), folds, keep, compaction, output rows
        N.call("dxa_win_answer", N.ptr(self.ring), self.gcap, self.stride, N.ptr(slots_dev), len(slots),
               N.ptr(self.line_ops_dev), L["count_word"], N.ptr(self.scal), N.ptr(self.acc), N.ptr(self.keep),
               N.ptr(self.out_idx), ctypes.addressof(e), ctypes.addressof(self.dictcols),
               0 if folds is None else ctypes.addressof(folds), *self._descs(), st)
        if not defer:
            # the statement's one synchronising read
            return self._finish(self.scal.tolist(), bufs, fin, partial_proto)
        pin = self._scal_pin[self._scal_k]
        self._scal_k ^= 1
        pin.copy_(self.scal, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))

        def finish():
            ev.synchronize()
            return self._finish(pin.tolist(), bufs, fin, partial_proto)
        return finish

    def _finish(self, status, bufs, fin, partial_proto):
        L = self.layout
        ng_all, bad, nout = status[:3]
        # (the device's flag 8, "a winning string too long for its line", is 16 here: 8 is a pair dictionary's "full")
        bad = (bad & 7) | (16 if bad & 8 else 0)
        for k, ps in enumerate(self.pairs):
            # a pair dictionary's collision / over-long value joins the outer flags; its "full" is flag 8 here
            pflags = status[4 + 4 * k + 1]
            ps.full = bool(pflags & 2)
            bad |= (pflags & 5) | (8 if ps.full else 0)
        self.bad = bad
        if bad:
            # full dictionaries and nothing else: rebuilt before the next answer (dense_answer); a collision or an
            # over-long key or string value (never cleared on the device) sends the statement to the paned path for good
            self.rebuild_pending = not bad & (5 | 16)
            return None
        self.dirty = []
        okey, olen, ovalid, dst, dvalid = bufs
        if self.global_form and nout == 0:
            # no row passed the WHERE anywhere in the window: Spark's one row — counts 0, everything else NULL
            return [], self._finals([(torch.zeros(1, dtype=torch.int64, device=self.device),
                                      torch.zeros(1, dtype=torch.bool, device=self.device)) for _ in L["fin"]]), 1
        out_keys = []
        for j, (dt, kind, vals, lens, valid) in enumerate(self.keys):
            v = ovalid[j, :nout].view(torch.bool)
            if kind == 2:
                sc = StrColumn(vals, okey[j, :nout], olen[j, :nout], v)
                sc.max_len = _sizes()[2]               # a dictionary key slot: bytes per row are bounded
                out_keys.append(sc)
            else:
                d = okey[j, :nout]
                if kind == 1:
                    d = d.view(torch.float64)
                elif dt == "boolean":
                    d = d.to(torch.bool)
                out_keys.append(PrimColumn(dt, d, v))
        cols = [(dst[r, :nout], dvalid[r, :nout].view(torch.bool)) for r in range(len(fin))]
        if partial_proto is not None:
            return self._partials(cols, out_keys, nout, *partial_proto)
        return ([] if self.global_form else out_keys), self._finals(cols), nout

    def _finals(self, cols) -> Dict:
        """{agg key → column} from the emitted (int64 words, validity) per ``fin`` row: a count (no count slot)
        is a never-NULL long, everything else has the planned dtype ``dt`` over doubles (``as_f64``), booleans or the
        words as they are.  A ``plan`` entry with two rows is a 128-bit decimal (lo, hi), packed as ``dt`` stores it:
        lo alone for up to 18 digits, else [n, 2]."""
        L = self.layout
        finals = {}
        for (ak, kind, _s, c, dt), f64, (r0, nr) in zip(L["plan"], L["as_f64"], L["rows"]):
            v, ok = cols[r0]
            if kind == "str":   # a string MIN / MAX: six byte words and the length
                finals[ak] = str_column_of([cols[r0 + q][0] for q in range(6)], cols[r0 + 6][0], ok)
            elif nr == 2:
                finals[ak] = PrimColumn(dt, Dec.pack(cols[r0 + 1][0], v, dt), ok)
            elif c is None:
                finals[ak] = PrimColumn("long", v)
            else:
                finals[ak] = PrimColumn(dt, v.view(torch.float64) if f64 else v.to(torch.bool) if dt == "boolean"
                                        else v, ok)
                if L.get("pick_x", {}).get(ak) in self.f32_args:
                    finals[ak] = PrimColumn(dt, finals[ak].data.to(torch.float32), ok)
        return finals

    def _emit_args(self, fin):
        """The emit kernel's descriptor and this batch's output buffers ([gcap]-strided, fresh per batch: the
        previous batch's outputs may still be rendering on the output stream)."""
        g, dev = self.gcap, self.device
        nk, nr = len(self.keys), len(fin)
        words = torch.empty((nk + nr, g), dtype=torch.int64, device=dev)
        flags = torch.empty((nk + nr, g), dtype=torch.uint8, device=dev)
        olen = torch.empty((max(1, nk), g), dtype=torch.int32, device=dev)
        okey, dst = words[:nk], words[nk:]
        ovalid, dvalid = flags[:nk], flags[nk:]
        e = _EmitArgs()
        e.acc, e.stride, e.nreq = self.acc.data_ptr(), self.stride, nr
        for r, (k, pos, cnt, *ops) in enumerate(fin):
            e.kind[r], e.pos[r], e.cnt[r] = k, pos, cnt
            e.op2[r], e.op3[r] = ops or (-1, -1)
        e.dst, e.dvalid = dst.data_ptr(), dvalid.data_ptr()
        for j in range(nk):
            e.okey[j], e.olen[j], e.ovalid[j] = okey[j].data_ptr(), olen[j].data_ptr(), ovalid[j].data_ptr()
        e.out_idx, e.scal, e.gcap = self.out_idx.data_ptr(), self.scal.data_ptr(), g
        return e, (okey, olen, ovalid, dst, dvalid)

    def _partial_spec(self, partial_proto):
        """Finishing spec of the partial states, in the partial table's entry order."""
        _proto, pplan, _kn = partial_proto
        L = self.layout
        out = []
        for ak, entries in pplan.items():
            for nm, suffix, _op in entries:
                f = L["pfin"].get(ak, {}).get(suffix)
                if f is None:
                    raise Ineligible(f"partial {suffix}")
                out.extend(f if isinstance(f, list) else [f])      # (a 128-bit decimal state: two rows; a string: 7)
        return out

    def _partials(self, cols, out_keys, nout, proto, pplan, key_names):
        """This rank's kept groups as a partial table shaped like ``proto`` (column names, types, order)."""
        from .column import Table
        got = {nm: k for nm, k in zip(key_names, out_keys)}
        kind_of = {p[0]: p[1] for p in self.layout["plan"]}
        j = 0
        for ak, entries in pplan.items():
            for nm, suffix, _op in entries:
                like = proto.column(nm)
                v, ok = cols[j]
                j += 1
                state = self.layout["pfin"][ak][suffix]
                if kind_of[ak] == "str" and suffix == "v":
                    # a string MIN / MAX value: six byte words and the length
                    got[nm] = str_column_of([v, *(cols[j + q][0] for q in range(5))], cols[j + 5][0], ok)
                    j += 6
                elif isinstance(state, list):
                    # a 128-bit decimal state (lo, hi) as the prototype's type stores it
                    got[nm] = PrimColumn(like.dtype, Dec.pack(cols[j][0], v, like.dtype), ok)
                    j += 1
                elif suffix == "cnt":
                    got[nm] = PrimColumn(like.dtype, v)
                elif isinstance(like, PrimColumn) and like.data.dtype == torch.float64:
                    got[nm] = PrimColumn(like.dtype, v.view(torch.float64), ok)
                elif isinstance(like, PrimColumn) and like.data.dtype == torch.float32:     # (a float32 pick)
                    got[nm] = PrimColumn(like.dtype, v.view(torch.float64).to(torch.float32), ok)
                elif like.dtype == "boolean":
                    got[nm] = PrimColumn(like.dtype, v.to(torch.bool), ok)
                else:
                    got[nm] = PrimColumn(like.dtype, v, ok)
        return Table(list(proto.names), [got[nm] for nm in proto.names], nout, self.device)


def dense_partials(t, sel, alias: str, ctx, items, aggs: Dict, fp: str, empty):
    """Multi-rank window: this rank's window groups from the dense ring as a ``distagg.local_partials``-shaped
    partial table → (partial table, plan, key names, group exprs), or None.  The caller exchanges and merges the
    partials exactly as the paned path does, so both paths issue the same collectives (a rank that falls back
    stays in step with the others)."""
    from . import distagg as D
    from .query import _resolve_group_expr
    from .expr import Scope, evaluate
    states = t.store.__dict__.setdefault("_dense", {})
    st = states.get(fp)
    if st is not None and getattr(st, "disabled", False):
        return None
    proto_key = "_dense_proto_" + fp
    pp = t.store.__dict__.get(proto_key)
    if pp is None:
        scope = Scope.of_table(empty, alias)
        gx = [_resolve_group_expr(g, scope, items) for g in sel.group_by]
        keys = [materialize(evaluate(g, scope, ctx)) for g in gx]
        proto, plan, key_names = D.local_partials(gx, keys, aggs, scope, ctx)
        pp = t.store.__dict__[proto_key] = (proto, plan, key_names)
    got = dense_answer(t, sel, alias, ctx, items, aggs, fp, partial_proto=pp)
    if got is None:
        return None
    table, gexprs = got
    return table, pp[1], pp[2], gexprs


def dense_answer(t, sel, alias: str, ctx, items, aggs: Dict, fp: str, partial_proto=None, defer: bool = False):
    """The window statement's (key columns, finals, groups, group exprs) from the dense ring, or None.
    ``defer``: instead a function returning that tuple (or None: fall back) once the status read completes.
    None leaves the statement to the paned path: for good when the state is disabled (``disabled_reason``), for
    this one call when a deferred status reads "dictionary full" — the caller's re-run comes back here, rebuilds
    the dictionary and answers from the ring."""
    from .. import parallel as P
    from .query import _resolve_group_expr
    from .expr import Scope
    store = t.store
    dev = t._device
    distinct = any(c.distinct or c.name == "approx_count_distinct" for c in aggs.values())
    if dev.type != "cuda" or (partial_proto is None and P.active() and t.dist != P.REPLICATED):
        return None
    if not sel.group_by and not distinct:   # a global statement without a distinct count keeps the paned path
        return None
    # a distinct count has no mergeable partial, nor have max_by / min_by
    if partial_proto is not None and (distinct or any(c.name in ("max_by", "min_by") for c in aggs.values())):
        return None
    states = store.__dict__.setdefault("_dense", {})
    state = states.get(fp)
    if state is not None and state.disabled:
        return None
    pieces = t.pieces()
    if not pieces:
        return None
    try:
        if state is None:
            iv = max(1, store.interval_us)
            panes = store.conf.max_window_us // iv + store.conf.watermark_us // iv + 4
            state = states[fp] = DenseWindow(dev, _requests(aggs, picks=True, distinct_sums=True),
                                             max(panes, len(pieces) + 2),
                                             global_form=not sel.group_by)
        state._rebuilt = set()
        proto = pieces[0][0].table
        gexprs = [_resolve_group_expr(g, Scope.of_table(proto, alias), items) for g in sel.group_by]
        # A status that reads "dictionary full" (in this call, or in the deferred completion of the last one) is
        # answered by a rebuild and another pass over the window's panes, which accumulates the dropped panes
        # again.  Every rebuild after the first in one call doubles the capacity or gives up, so the loop ends
        # within log2(DENSE_GROUPS_MAX / DENSE_GROUPS) + 2 passes.  (With pair states: every pass rebuilds at least
        # one full dictionary, and a dictionary's second rebuild in one call doubles it or gives up — the same
        # bound per dictionary.)
        rebuilt = False
        while True:
            if state.rebuild_pending:
                state.rebuild(store.past, grow=rebuilt)
                rebuilt = True
            got = _enqueue(state, t, pieces, sel, alias, gexprs, ctx, partial_proto, defer)
            if got is not None or not state.rebuild_pending:
                break
    except Ineligible as why:
        state = states.get(fp)
        if state is not None:
            _disable(state, str(why))
        else:
            states[fp] = _Disabled(str(why))
        return None
    if callable(got):
        def finish():
            res = got()
            if res is None:
                if not state.rebuild_pending:   # else: the caller's re-run of the statement rebuilds and answers
                    _disable(state, _flag_reason(state.bad))
                return None
            out_keys, finals, ng = res
            return out_keys, finals, ng, gexprs
        return finish
    if got is None:
        _disable(state, _flag_reason(state.bad))
        return None
    if partial_proto is not None:
        return got, gexprs
    out_keys, finals, ng = got
    return out_keys, finals, ng, gexprs


def _flag_reason(bad: int) -> str:
    # an over-long key is stored with length 0, so later rows of that key also compare unequal (flag 1): 4 first
    return "key too long" if bad & 4 else "hash collision" if bad & 1 else "argument too long" if bad & 16 else \
        "dictionary full" if bad & 2 or not bad else "pair dictionary full"


def _disable(state, reason: str) -> None:
    state.disabled = True
    state.disabled_reason = reason
    state.ring = state.acc = None
    for ps in state.pairs:
        ps.pres = None


def _enqueue(state, t, pieces, sel, alias: str, gexprs, ctx, partial_proto, defer: bool):
    """One pass over the window's panes: new panes into ring slots, complete blocks combined, the answer queued →
    ``DenseWindow.answer``'s result."""
    store = t.store
    # ring slots: a pane keeps its slot while the store retains it (a pane's rows never change — its table is only
    # compacted once; the pane object guards a re-created pane), an expired pane's slot goes back to the free
    # heap.  One pass over the window's panes.
    slot_of = state.slot_of
    state.release_expired(store.past)
    scratch = list(range(state.R - SCRATCH_SLOTS, state.R))
    slots = []
    span = BLOCK * max(1, store.interval_us)
    by_block: Dict[int, list] = {}
    seq = [] if state.has_picks else None          # row picks: the window's row order — scratch slots and entries
    for pane, full in pieces:
        if full:                                   # (pieces' "full" includes every row having a timestamp)
            ent = slot_of.get(pane.key)
            if ent is None or ent[1] is not pane:
                if ent is not None:
                    heapq.heappush(state.free, ent[0])
                    del slot_of[pane.key]
                if not state.free:
                    raise Ineligible("ring full")
                sl = heapq.heappop(state.free)
                state.accumulate(pane.table, sl, alias, sel.where, gexprs, ctx)
                ent = slot_of[pane.key] = (sl, pane, pane.key // span, pane.key)
                state.dirty.append(pane.key)
            mem = by_block.get(ent[2])
            if mem is None:
                by_block[ent[2]] = [ent]
            else:
                mem.append(ent)
            if seq is not None:
                seq.append(ent)
        else:
            # a pane only partly inside the window: its in-range rows, re-aggregated into a scratch slot
            if not scratch:
                raise Ineligible("too many clipped panes")
            sl = scratch.pop(0)
            state.accumulate(t.clipped(pane), sl, alias, sel.where, gexprs, ctx)
            slots.append(sl)
            if seq is not None:
                seq.append(sl)
    # complete blocks of BLOCK consecutive panes: one pre-combined slot each (the per-batch combine then reads
    # ~20 block slots and the loose panes at the window's edges instead of 300 pane slots)
    for bid in [b for b in state.blocks if b not in by_block]:
        del state.blocks[bid]
    if seq is not None:
        return state.answer(_ordered_slots(state, seq, by_block), partial_proto,
                            defer=defer and partial_proto is None)
    for bid, mem in by_block.items():
        if len(mem) == BLOCK:
            slots.append(state.block_slot(bid, mem))
        else:
            state.blocks.pop(bid, None)
            slots.extend(e[0] for e in mem)
    return state.answer(slots, partial_proto, defer=defer and partial_proto is None)


def _ordered_slots(state, seq: list, by_block: Dict[int, list]) -> List[int]:
    """The combine's slots of a layout with row picks, in the window's row order (that of ``PanedTable.pieces``, which
    the materialised view concatenates in): ``seq`` holds, in that order, the scratch slots of the clipped panes and
    the slot entries of the whole ones.  A complete block goes in as its pre-combined slot where its members stand
    together — in the order they stand in, which is the order ``block_slot`` combines them in; the block that holds
    the current pane does not (the current pane comes first, the block's older members after the panes in between),
    so its members go in one by one, as those of an incomplete block do."""
    slots: List[int] = []
    used = set()
    k = 0
    while k < len(seq):
        ent = seq[k]
        if not isinstance(ent, tuple):
            slots.append(ent)
            k += 1
            continue
        bid = ent[2]
        run = k + 1
        while run < len(seq) and isinstance(seq[run], tuple) and seq[run][2] == bid:
            run += 1
        if run - k == BLOCK and len(by_block[bid]) == BLOCK:
            slots.append(state.block_slot(bid, seq[k:run]))
            used.add(bid)
        else:
            slots.extend(e[0] for e in seq[k:run])
        k = run
    for bid in [b for b in state.blocks if b not in used]:
        del state.blocks[bid]
    return slots


class _Disabled:
    disabled = True

    def __init__(self, reason: str):
        self.disabled_reason = reason
