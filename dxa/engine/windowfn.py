"""SQL window functions: ``f(args) OVER (PARTITION BY … ORDER BY … [ROWS|RANGE frame])``.

The reference runs these through Spark SQL inside a transform statement (CommonProcessorFactory.scala:249-294 hands
every statement to ``spark.sql``); here each window call is evaluated column-at-a-time over device tensors:

1. partition ids from the hash group-by kernel, then ONE permutation that sorts rows by (partition, order keys) with
   stable argsorts (least significant key first);
2. in sorted order, partition / peer boundaries become flag vectors and ``cummax``/``cummin`` scans give every row its
   partition start/end and peer-group start/end — no per-partition loops;
3. ranking functions are arithmetic on those positions; ``lag``/``lead``/``first_value``/``last_value``/
   ``nth_value`` are gathers; aggregates over a frame ``[a, b]`` use prefix sums for counts and integer / decimal
   sums (exact: int64 and 32-bit decimal limbs), power-of-two block sums for double sums (no prefix differences,
   which cancel catastrophically) and a sparse table for min/max (O(n log n) build, O(1) query);
   the variance and moment families (stddev / variance and their _pop / _samp forms, skewness, kurtosis, covar_pop,
   covar_samp, corr) take their frame's state — (n, mean, M2), (n, mean, M2, M3, M4) or (n, mean_x, mean_y, Cxy,
   M2x, M2y) — from the HIP kernels of ``ops/csrc/window_frames.hip``: one two-pass launch when the longest frame
   is at most ``FRAME_DIRECT_MAX`` rows, else one launch per power-of-two level with pairwise (Chan) merges; on a
   CPU device the same level algorithm runs as tensor operations (``_frame_state_tensor``).  The state is finished
   by the rules GROUP BY uses (``groupby.finish_variance``, ``query.finish_moments`` / ``finish_comoments``);
   the order statistics (percentile / median with linear interpolation, percentile_approx / approx_percentile — the
   smallest counted value whose rank reaches p·count, exact here) have no mergeable state: the ranks they read come
   from GROUP BY's own arithmetic (``query.percentile_ranks``) on the frame's count of non-NULL rows, and ONE
   primitive (``_frame_select``) turns all ranks of a window call into row positions — "the k-th smallest counted
   row of x[a[i] .. b[i]] in (order key, position) order" — from the HIP kernels of ``ops/csrc/window_select.hip``:
   one launch that ranks every candidate of its frame when the longest frame is at most
   ``FRAME_SELECT_DIRECT_MAX`` rows, else a wavelet matrix over the rows' global ranks (one stable radix sort, per
   bit a prefix count and a stable scatter, then one launch that answers every row and rank); on a CPU device the
   same wavelet build and query run as tensor operations (``_frame_select_tensor``).  The values at those
   positions are gathered and interpolated (``query.percentile_interpolate``);
   the distinct counts — ``approx_count_distinct(x[, rsd])`` (the exact count, as in GROUP BY and the dense ring; rsd
   is accepted and never read), ``count(DISTINCT x)`` and ``count(DISTINCT a, b, …)`` (a tuple counts where all its
   members are non-NULL) — are a long, never NULL, 0 for an empty frame.  Spark refuses DISTINCT in window
   functions; accepting ``count(DISTINCT …) OVER`` is a deliberate superset, and every other DISTINCT stays refused.
   A row's value id is GROUP BY's (``G.group_rows``: NaN equals NaN, -0.0 equals 0.0, any keyable type or tuple).
   One stable radix argsort of the ids and a neighbour compare give p[j], the position of the previous counted row
   with the same id (-1: none; n: row j is not counted), and the answer for the frame [a, b] is #{ j in [a, b] :
   p[j] < a } — every value counted at its first row inside the frame — from the HIP kernels of
   ``ops/csrc/window_distinct.hip``: one launch that scans p over the frame when the longest frame is at most
   ``FRAME_DISTINCT_DIRECT_MAX`` rows, else the wavelet matrix of the order statistics built over p and one launch
   that counts, per row, the frame's global ranks below a threshold; on a CPU device the same walk runs as tensor
   operations (``_frame_distinct_tensor``).  A previous occurrence in another partition lies before the frame, so
   neither path has a partition case;
   ``collect_list(x)`` / ``collect_set(x)`` give the frame's counted values as an array, never NULL, in the frame's
   sorted order — the set at every value's first row inside the frame, the rows with p[j] < a of the same array p —
   as a ``[K, n]`` matrix of row positions, K the largest per-frame count, from ``ops/csrc/collect.hip``
   (``dxa_frame_collect``, one launch) or, on a CPU device, tensor operations; one gather builds the elements;
4. the result is scattered back to input row order.

Known caveat, shared with GROUP BY: ``M2 > 0`` is tested on a rounded M2, so corr / skewness / kurtosis of a constant
frame whose values do not sum exactly can be a huge number where Spark gives NaN.

Distributed scopes are re-partitioned by the PARTITION BY keys (RCCL all-to-all) before evaluation, or gathered when
there is no PARTITION BY (see ``query._exec_select``).
"""
from __future__ import annotations

from typing import Callable, List

import torch

from ..ops import groupby as G
from ..ops import native as N
from ..sql import ast as A
from .column import Column, ConstColumn, PrimColumn, materialize

N.register_sigs({
    "dxa_frame_moments_direct": [N.c_p, N.c_p, N.c_p, N.c_p, N.c_p, N.c_i64, N.c_i32, N.c_p, N.c_p],
    "dxa_frame_moments_levels": [N.c_p, N.c_p, N.c_p, N.c_p, N.c_p, N.c_i64, N.c_i32, N.c_i64, N.c_p, N.c_p, N.c_p],
    "dxa_frame_select_direct": [N.c_p, N.c_p, N.c_p, N.c_p, N.c_i64, N.c_p, N.c_i32, N.c_p, N.c_p],
    "dxa_frame_select_tree": [N.c_p, N.c_p, N.c_p, N.c_p, N.c_p, N.c_i64, N.c_i32, N.c_p, N.c_i32, N.c_p, N.c_p],
    "dxa_wavelet_level": [N.c_p, N.c_p, N.c_i64, N.c_i32, N.c_p, N.c_p, N.c_p],
    "dxa_frame_distinct_direct": [N.c_p, N.c_p, N.c_p, N.c_i64, N.c_p, N.c_p],
    "dxa_frame_distinct_tree": [N.c_p, N.c_p, N.c_p, N.c_p, N.c_i64, N.c_i32, N.c_p, N.c_p],
})

RANKING = {"row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile"}
OFFSET = {"lag", "lead"}
VALUE = {"first_value", "last_value", "first", "last", "nth_value"}
FRAMED_AGGS = {"sum", "count", "avg", "mean", "min", "max"}
# state kinds of window_frames.hip: VAR (n, mean, M2), MOM (n, mean, M2, M3, M4), CO (n, mean_x, mean_y, Cxy, M2x, M2y)
KIND_VAR, KIND_MOM, KIND_CO = 0, 1, 2
STATE_WORDS = {KIND_VAR: 3, KIND_MOM: 5, KIND_CO: 6}
FRAME_MOMENTS = {"stddev": KIND_VAR, "std": KIND_VAR, "stddev_samp": KIND_VAR, "stddev_pop": KIND_VAR,
                 "variance": KIND_VAR, "var_samp": KIND_VAR, "var_pop": KIND_VAR, "skewness": KIND_MOM,
                 "kurtosis": KIND_MOM, "covar_pop": KIND_CO, "covar_samp": KIND_CO, "corr": KIND_CO}
# order statistics over a frame: True for the exact (interpolating) form, False for the approximate one
FRAME_SELECT = {"percentile": True, "median": True, "percentile_approx": False, "approx_percentile": False}
# distinct counts over a frame: approx_count_distinct(x[, rsd]) (exact here, as in GROUP BY) and count(DISTINCT …)
COUNT_DISTINCT = "count(DISTINCT …)"                    # the evaluator's own name for count(DISTINCT a, …)
FRAME_DISTINCT = {"approx_count_distinct", COUNT_DISTINCT}
# the frame's counted values as an array: the list in the frame's sorted order, the set at every value's first row
FRAME_COLLECT = {"collect_list", "collect_set"}
WINDOW_FUNCS = (RANKING | OFFSET | VALUE | FRAMED_AGGS | set(FRAME_MOMENTS) | set(FRAME_SELECT) | FRAME_DISTINCT
                | FRAME_COLLECT)

# The longest frame (rows) the one-launch two-pass kernel takes; longer frames go level by level.  The longest
# measured frame at which the direct entry was no slower than the levels entry for every state kind
# (profiles/window_frames/README.md).
FRAME_DIRECT_MAX = 48
# The longest frame (rows) the one-launch candidate-ranking kernel of window_select.hip takes; longer frames go
# through the wavelet matrix (profiles/window_percentile/README.md).
FRAME_SELECT_DIRECT_MAX = 32
SELECT_MAX_RANKS = 16          # ranks per call of the selection entry points
# The longest frame (rows) the one-launch linear scan of window_distinct.hip takes; longer frames go through the
# wavelet matrix.  The longest measured frame at which the scan, with the previous-occurrence array, was no slower
# than the matrix build and query for both value cardinalities: 0.92–0.94 ms against 1.18–1.28 ms at 2,048 rows,
# 1.38–1.40 ms against 1.18–1.23 ms at 4,096 (profiles/window_frame_distinct/README.md).
FRAME_DISTINCT_DIRECT_MAX = 2048
# collect_list / collect_set OVER keep K slots for every row, K the largest per-frame count: K · n is the size of the
# result itself.  Past this many slots the call is refused instead of allocated (a guard, not a tuned number).
FRAME_COLLECT_MAX_SLOTS = 1 << 27

_INT_TYPES = ("byte", "short", "int", "integer", "long", "bigint", "tinyint", "smallint")
_FLOAT_TYPES = ("float", "double")


class WindowError(Exception):
    pass


def window_calls(e: A.Expr) -> List[A.WindowCall]:
    return list(A.summary(e)[1])


def _sort_key(col: Column):
    from .query import _sort_key_tensor
    key, valid = _sort_key_tensor(col)
    return torch.where(valid, key, torch.zeros_like(key)), valid


def _literal_int(e: A.Expr, what: str) -> int:
    if isinstance(e, A.Literal) and e.type in ("int", "long"):
        return int(e.value)
    raise WindowError(f"{what} must be an integer literal")


def _rev_cummin(x: torch.Tensor) -> torch.Tensor:
    return torch.flip(torch.cummin(torch.flip(x, (0,)), 0).values, (0,))


def _minmax_frame(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, is_max: bool) -> torch.Tensor:
    """min/max of ``x[a[i] .. b[i]]`` for every i (frames assumed non-empty where used) via a sparse table."""
    n = x.shape[0]
    op = torch.maximum if is_max else torch.minimum
    levels = [x]
    k = 1
    while 2 * k <= n:
        prev = levels[-1]
        nxt = prev.clone()
        nxt[: n - k] = op(prev[: n - k], prev[k:])
        levels.append(nxt)
        k *= 2
    table = torch.stack(levels)                       # [L, n]
    length = (b - a + 1).clamp(min=1)
    lvl = torch.floor(torch.log2(length.to(torch.float64))).to(torch.int64).clamp(max=len(levels) - 1)
    # exact floor(log2) (float log2 can round up at powers of two minus epsilon)
    lvl = torch.where((1 << lvl) > length, lvl - 1, lvl)
    span = 1 << lvl
    ai = a.clamp(0, n - 1)
    bi = (b - span + 1).clamp(0, n - 1)
    return op(table[lvl, ai], table[lvl, bi])


def evaluate_window(wc: A.WindowCall, ev: Callable[[A.Expr], Column], n: int, dev) -> Column:
    """Evaluate one window call over ``n`` rows; ``ev`` evaluates a sub-expression over the same rows."""
    name = wc.func.name
    if name == "mean":
        name = "avg"
    if name not in WINDOW_FUNCS:
        raise WindowError(f"{name} is not supported as a window function")
    # count(DISTINCT a, …) is the one DISTINCT a window takes (a superset of Spark, which refuses them all)
    if wc.func.distinct:
        if name in FRAME_COLLECT:
            raise WindowError(f"{name}(DISTINCT …) is not supported as a window function")
        if name != "count" or wc.func.star or not wc.func.args:
            raise WindowError("DISTINCT is not supported in window aggregates")
        name = COUNT_DISTINCT
    i64 = torch.int64
    if n == 0 and name in FRAME_COLLECT:
        from .query import array_from_slots
        return array_from_slots(_collect_arg(name, wc, ev), None, 0, None, None)
    if n == 0:
        integral = name in RANKING - {"percent_rank", "cume_dist"} or name in FRAME_DISTINCT
        return ConstColumn(None, "long" if integral else "double", 0, dev)

    # -- one permutation: rows sorted by (partition, order keys) -----------------------------------------------
    if wc.partition:
        keys = [materialize(ev(p)) for p in wc.partition]
        gid = G.group_rows(keys).gid.to(i64)
    else:
        gid = torch.zeros(n, dtype=i64, device=dev)
    from ..ops.sort import argsort_words, sort_spec_words
    okeys = []
    specs = []
    for it in wc.order:
        col = materialize(ev(it.expr))
        okeys.append((it,) + _sort_key(col))
        nulls_first = it.nulls_first if it.nulls_first is not None else it.ascending
        specs.append((col, it.ascending, nulls_first))
    # one stable device radix argsort: partition id most significant, then the ORDER BY items
    words = sort_spec_words(specs) + [gid]
    perm = argsort_words(words)

    # -- partition / peer boundaries in sorted order ------------------------------------------------------------
    idx = torch.arange(n, device=dev, dtype=i64)
    sg = gid[perm]
    pnew = torch.ones(n, dtype=torch.bool, device=dev)
    pnew[1:] = sg[1:] != sg[:-1]
    pend_flag = torch.ones(n, dtype=torch.bool, device=dev)
    pend_flag[:-1] = pnew[1:]
    pstart = torch.cummax(torch.where(pnew, idx, torch.zeros_like(idx)), 0).values
    pend = _rev_cummin(torch.where(pend_flag, idx, torch.full_like(idx, n)))
    peer_new = pnew.clone()
    for _, key, valid in okeys:
        k, v = key[perm], valid[perm]
        if k.is_floating_point():
            same = (k[1:] == k[:-1]) | (torch.isnan(k[1:]) & torch.isnan(k[:-1]))
        else:
            same = k[1:] == k[:-1]
        peer_new[1:] |= ~same | (v[1:] != v[:-1])
    peer_end_flag = torch.ones(n, dtype=torch.bool, device=dev)
    peer_end_flag[:-1] = peer_new[1:]
    peer_start = torch.cummax(torch.where(peer_new, idx, torch.zeros_like(idx)), 0).values
    peer_end = _rev_cummin(torch.where(peer_end_flag, idx, torch.full_like(idx, n)))
    size = pend - pstart + 1
    pos = idx - pstart

    rkey = _range_key(wc, okeys, specs, perm) if _has_range_offsets(wc) else None
    res = _compute(name, wc, ev, perm, idx, pstart, pend, peer_new, peer_start, peer_end, size, pos, n, dev, rkey)
    inv = torch.empty_like(perm)
    inv[perm] = idx
    return res.take(inv)


def _has_range_offsets(wc) -> bool:
    return wc.frame is not None and wc.frame[0] == "range" and any(
        b[0] in ("preceding", "following") for b in wc.frame[1:])


def _range_key(wc, okeys, specs, perm):
    """The ORDER BY value of every row in sorted order, made ascending (DESC keys negated) with nulls mapped to the
    end of the range they sort to, for RANGE frames with value offsets (Spark: one numeric / date / timestamp
    ORDER BY expression; timestamp offsets are INTERVALs, in microseconds here)."""
    if len(wc.order) != 1:
        raise WindowError("a RANGE frame with value offsets needs exactly one ORDER BY expression")
    col, asc, nulls_first = specs[0]
    if not isinstance(col, PrimColumn) or col.dtype in ("string", "boolean"):
        raise WindowError("a RANGE frame with value offsets needs a numeric, date or timestamp ORDER BY")
    x = col.data[perm]
    valid = col.valid_mask()[perm]
    x = x.to(torch.float64) if x.is_floating_point() else x.to(torch.int64)
    if not asc:
        x = -x
    if x.is_floating_point():
        lo, hi = float("-inf"), float("inf")
    else:
        info = torch.iinfo(torch.int64)
        lo, hi = info.min, info.max
    x = torch.where(valid, x, torch.full_like(x, lo if nulls_first else hi))
    return x, valid


def _bound_search(key, lo, hi, v, strict: bool):
    """First index j in [lo, hi+1) with key[j] >= v (``strict``: key[j] > v), per row — a vectorised binary search
    inside every row's partition (key ascending within it)."""
    n = key.shape[0]
    L, R = lo.clone(), hi + 1
    for _ in range(max(1, int(n).bit_length() + 1)):
        active = L < R
        mid = (L + R) // 2
        km = key[mid.clamp(0, n - 1)]
        right = active & ((km <= v) if strict else (km < v))
        L = torch.where(right, mid + 1, L)
        R = torch.where(active & ~right, mid, R)
    return L


def _frame(wc, idx, pstart, pend, peer_start, peer_end, rkey=None):
    if wc.frame is None:
        if wc.order:
            return pstart, peer_end         # RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW
        return pstart, pend
    kind, lo, hi = wc.frame

    def bound(b, is_start):
        t, k = b
        if t == "unbounded_preceding":
            return pstart
        if t == "unbounded_following":
            return pend
        if t == "current":
            if kind == "range":
                return peer_start if is_start else peer_end
            return idx
        if kind == "range":
            key, valid = rkey
            off = -k if t == "preceding" else k
            if key.is_floating_point():
                v = key + float(off)
            else:
                if isinstance(off, float):
                    raise WindowError("an integral RANGE ORDER BY needs integral offsets")
                v = key + int(off)
            pos = (_bound_search(key, pstart, pend, v, strict=False) if is_start
                   else _bound_search(key, pstart, pend, v, strict=True) - 1)
            return torch.where(valid, pos, peer_start if is_start else peer_end)   # a null key: its peers
        if isinstance(k, float):
            raise WindowError("ROWS frame offsets must be integers")
        return idx - k if t == "preceding" else idx + k

    a = torch.maximum(bound(lo, True), pstart)
    b = torch.minimum(bound(hi, False), pend)
    return a, b


def _compute(name, wc, ev, perm, idx, pstart, pend, peer_new, peer_start, peer_end, size, pos, n, dev, rkey=None):
    from .expr import _select_by_conditions
    from .query import _take_nullable
    args = wc.func.args
    if name == "row_number":
        return PrimColumn("int", (pos + 1))
    if name == "rank":
        return PrimColumn("int", (peer_start - pstart + 1))
    if name == "dense_rank":
        cs = torch.cumsum(peer_new.to(torch.int64), 0)
        return PrimColumn("int", (cs - cs[pstart] + 1))
    if name == "percent_rank":
        r = (peer_start - pstart).to(torch.float64)
        d = (size - 1).to(torch.float64)
        return PrimColumn("double", torch.where(size > 1, r / d.clamp(min=1), torch.zeros_like(r)))
    if name == "cume_dist":
        return PrimColumn("double", (peer_end - pstart + 1).to(torch.float64) / size.to(torch.float64))
    if name == "ntile":
        if len(args) != 1:
            raise WindowError("ntile takes one argument")
        k = _literal_int(args[0], "ntile bucket count")
        if k <= 0:
            raise WindowError("ntile bucket count must be positive")
        base = size // k
        rem = size % k
        big = rem * (base + 1)
        bucket = torch.where(pos < big, pos // (base + 1), rem + (pos - big) // base.clamp(min=1))
        return PrimColumn("int", (bucket + 1))

    if name in OFFSET:
        if not 1 <= len(args) <= 3:
            raise WindowError(f"{name} takes 1 to 3 arguments")
        k = _literal_int(args[1], f"{name} offset") if len(args) > 1 else 1
        col = materialize(ev(args[0])).take(perm)
        src = idx - k if name == "lag" else idx + k
        ok = (src >= pstart) & (src <= pend)
        out = _take_nullable(col, torch.where(ok, src, torch.full_like(src, -1)))
        if len(args) == 3:
            dflt = ev(args[2])
            if not isinstance(dflt, ConstColumn):
                dflt = materialize(dflt).take(perm)
            out = _select_by_conditions([PrimColumn("boolean", ok)], [out], dflt, n, dev)
        return out

    if name in FRAME_SELECT:
        x, ps, is_array = _percentile_args(name, wc, ev, perm)
        a, b = _frame(wc, idx, pstart, pend, peer_start, peer_end, rkey)
        return _frame_percentile(name, x, ps, is_array, a, b, n, dev)

    if name in FRAME_DISTINCT:
        vid, counted = _distinct_args(name, wc, ev, perm)
        a, b = _frame(wc, idx, pstart, pend, peer_start, peer_end, rkey)
        return PrimColumn("long", _frame_distinct(vid, counted, a, b))

    if name in FRAME_COLLECT:
        x = _collect_arg(name, wc, ev).take(perm)
        a, b = _frame(wc, idx, pstart, pend, peer_start, peer_end, rkey)
        return _frame_collect(name, x, a, b)

    if name in FRAME_MOMENTS:
        cols = _moment_args(name, wc, ev, perm)
        a, b = _frame(wc, idx, pstart, pend, peer_start, peer_end, rkey)
        return _frame_moment_agg(name, cols, a, b, n, dev)

    if wc.func.star or (name == "count" and not args):
        x = None
    else:
        if len(args) != (2 if name == "nth_value" else 1):
            raise WindowError(f"wrong number of arguments to {name}")
        x = materialize(ev(args[0]))
        if isinstance(x, ConstColumn):
            x = x.materialize()
        x = x.take(perm)
    a, b = _frame(wc, idx, pstart, pend, peer_start, peer_end, rkey)
    nonempty = a <= b

    if name in VALUE:
        if name in ("first_value", "first"):
            at = a
        elif name in ("last_value", "last"):
            at = b
        else:
            at = a + _literal_int(args[1], "nth_value position") - 1
        ok = nonempty & (at <= b)
        return _take_nullable(x, torch.where(ok, at, torch.full_like(at, -1)))

    # framed aggregates
    if x is None:
        cnt = torch.where(nonempty, b - a + 1, torch.zeros_like(a))
        return PrimColumn("long", cnt)
    if not isinstance(x, PrimColumn):
        raise WindowError(f"{name} OVER needs a numeric argument")
    valid = x.valid_mask()
    c = torch.cumsum(valid.to(torch.int64), 0)

    def frame_sum(pref):
        zero = torch.zeros(1, dtype=pref.dtype, device=dev)
        pz = torch.cat([zero, pref])                     # pz[j] = sum of the first j values
        hi = pz[(b + 1).clamp(0, n)]
        lo = pz[a.clamp(0, n)]
        return torch.where(nonempty, hi - lo, torch.zeros_like(hi))

    cnt = frame_sum(c)
    if name == "count":
        return PrimColumn("long", cnt)
    has = cnt > 0
    from .decimal import is_decimal
    if is_decimal(x.dtype):
        return _decimal_frame_agg(name, x, valid, a, b, nonempty, cnt, has, n, dev)
    data = x.data
    if data.dtype == torch.bool:
        data = data.to(torch.int64)
    if name in ("sum", "avg"):
        integral = x.dtype in _INT_TYPES and not data.is_floating_point()
        if integral:
            # int64 prefix differences are exact (two's complement wraps, as Spark's long sum does)
            s = frame_sum(torch.cumsum(torch.where(valid, data.to(torch.int64), torch.zeros_like(data,
                                                                                                dtype=torch.int64)),
                                       0))
        else:
            s = _float_frame_sum(torch.where(valid, data.to(torch.float64), torch.zeros_like(data,
                                                                                              dtype=torch.float64)),
                                 a, b, nonempty)
        if name == "sum":
            return PrimColumn("long" if integral else "double", s, has)
        return PrimColumn("double", s.to(torch.float64) / cnt.clamp(min=1).to(torch.float64), has)
    is_max = name == "max"
    if data.is_floating_point():
        fill = float("-inf") if is_max else float("inf")
    else:
        info = torch.iinfo(data.dtype)
        fill = info.min if is_max else info.max
    masked = torch.where(valid, data, torch.full_like(data, fill))
    return PrimColumn(x.dtype, _minmax_frame(masked, a, b, is_max), has)


def _moment_args(name, wc, ev, perm):
    """The argument column(s) of a variance / moment window aggregate as double columns in sorted order."""
    from .decimal import is_decimal, to_double
    args = wc.func.args
    if wc.func.star or len(args) != (2 if FRAME_MOMENTS[name] == KIND_CO else 1):
        raise WindowError(f"wrong number of arguments to {name}")
    cols = []
    for e in args:
        x = materialize(ev(e))
        if isinstance(x, ConstColumn):
            x = x.materialize()
        if not isinstance(x, PrimColumn) or not (is_decimal(x.dtype) or x.dtype in _INT_TYPES + _FLOAT_TYPES):
            raise WindowError(f"{name} OVER needs a numeric argument")
        if is_decimal(x.dtype):
            x = to_double(x)                              # as Spark casts it
        cols.append(x.take(perm))
    return cols


def _frame_moment_agg(name, cols, a, b, n, dev):
    """stddev / variance / skewness / kurtosis / covar / corr of ``cols`` over the frames ``[a, b]``: the frame's
    moment state from ``_frame_state``, then the finishing rules GROUP BY uses."""
    from .column import and_valid
    from .query import finish_comoments, finish_moments
    kind = FRAME_MOMENTS[name]
    x = cols[0].data.to(torch.float64).contiguous()
    y = cols[1].data.to(torch.float64).contiguous() if kind == KIND_CO else None
    valid = cols[0].valid
    for c in cols[1:]:
        valid = and_valid(valid, c.valid)                 # a pair counts where both arguments are non-NULL
    length = torch.where(a <= b, b - a + 1, torch.zeros_like(a))
    maxlen = int(length.max())                            # one host read: the path choice and the level count
    if maxlen == 0:
        st = torch.zeros((STATE_WORDS[kind], n), dtype=torch.float64, device=dev)
    else:
        st = _frame_state(kind, x, y, valid, a, b, maxlen)
    if kind == KIND_VAR:
        return G.finish_variance(name, st[0], st[2])
    if kind == KIND_MOM:
        return finish_moments(name, st[0], st[2], m3=st[3], m4=st[4])
    return finish_comoments(name, st[0], st[3], st[4], st[5])


def _frame_state(kind, x, y, valid, a, b, maxlen) -> torch.Tensor:
    """The moment state of every frame ``x[a[i] .. b[i]]`` (``a > b``: empty) as f64 ``[words, n]``; ``maxlen`` ≥ 1
    is the longest frame length.  Native on the GPU, tensor operations on the CPU."""
    if N.use_native(x):
        return _frame_state_native(kind, x, y, valid, a, b, maxlen)
    return _frame_state_tensor(kind, x, y, valid, a, b, maxlen)


def _frame_state_native(kind, x, y, valid, a, b, maxlen) -> torch.Tensor:
    n = int(x.shape[0])
    words = STATE_WORDS[kind]
    out = torch.empty((words, n), dtype=torch.float64, device=x.device)
    v = None if valid is None else N.u8(valid).contiguous()
    a, b = a.contiguous(), b.contiguous()
    st = N.stream_handle(x.device)
    if maxlen <= FRAME_DIRECT_MAX:
        N.call("dxa_frame_moments_direct", N.ptr(x), N.ptr(y), N.ptr(v), N.ptr(a), N.ptr(b), n, kind, N.ptr(out), st)
    else:
        scratch = torch.empty((2, words, n), dtype=torch.float64, device=x.device)     # two ping-pong levels
        N.call("dxa_frame_moments_levels", N.ptr(x), N.ptr(y), N.ptr(v), N.ptr(a), N.ptr(b), n, kind, maxlen,
               N.ptr(scratch), N.ptr(out), st)
    return out


def _merge_states(kind, A, B):
    """Chan's pairwise merge of two moment states (lists of word tensors; A the left run, B the right); a side
    with n = 0 returns the other unchanged."""
    na, nb = A[0], B[0]
    n = na + nb
    sn = n.clamp(min=1)
    if kind == KIND_CO:
        dx, dy = B[1] - A[1], B[2] - A[2]
        f = na * nb / sn
        out = [n, A[1] + dx * nb / sn, A[2] + dy * nb / sn, A[3] + B[3] + dx * dy * f, A[4] + B[4] + dx * dx * f,
               A[5] + B[5] + dy * dy * f]
    else:
        d = B[1] - A[1]
        d2 = d * d
        out = [n, A[1] + d * nb / sn, A[2] + B[2] + d2 * na * nb / sn]
        if kind == KIND_MOM:
            n2 = sn * sn
            out.append(A[3] + B[3] + d2 * d * na * nb * (na - nb) / n2 + 3.0 * d * (na * B[2] - nb * A[2]) / sn)
            out.append(A[4] + B[4] + d2 * d2 * na * nb * (na * na - na * nb + nb * nb) / (n2 * sn)
                       + 6.0 * d2 * (na * na * B[2] + nb * nb * A[2]) / n2 + 4.0 * d * (na * B[3] - nb * A[3]) / sn)
    only_a, only_b = nb == 0, na == 0
    return [torch.where(only_a, wa, torch.where(only_b, wb, w)) for wa, wb, w in zip(A, B, out)]


def _frame_state_tensor(kind, x, y, valid, a, b, maxlen) -> torch.Tensor:
    """``_frame_state`` as vectorised tensor operations on any device — the level algorithm of
    ``window_frames.hip``: level k holds the state of the 2^k-row run starting at every row (clipped at n), every
    frame is cut into such runs by the bits of its length, lowest bit first, and states merge pairwise.  Nothing is
    computed as Σx² − (Σx)²/n, and only values inside a frame enter its state."""
    n = int(x.shape[0])
    zero = torch.zeros_like(x)
    ok = torch.ones_like(x, dtype=torch.bool) if valid is None else valid.to(torch.bool)

    def own(v):
        return torch.where(ok, v, zero)
    zx = x - x                                             # 0, or NaN for a non-finite value
    if kind == KIND_CO:
        zy = y - y
        level = [ok.to(torch.float64), own(x), own(y), own(zx * zy), own(zx), own(zy)]
    else:
        level = [ok.to(torch.float64), own(x)] + [own(zx)] * (STATE_WORDS[kind] - 2)
    lo, hi = a.clamp(min=0), b.clamp(max=n - 1)            # frames are clipped to [0, n)
    length = torch.where((a <= b) & (lo <= hi), hi - lo + 1, torch.zeros_like(a))
    acc = [zero] * STATE_WORDS[kind]
    k = 0
    while (1 << k) <= maxlen:
        step = 1 << k
        take = ((length >> k) & 1).to(torch.bool)
        pos = (lo + (length & (step - 1))).clamp(max=n - 1)
        run = [w[pos] for w in level]
        run[0] = torch.where(take, run[0], zero)           # bit k clear: merge the identity
        acc = _merge_states(kind, acc, run)
        if (step << 1) <= maxlen:
            pad = min(step, n)
            level = _merge_states(kind, level, [torch.cat([w[step:], zero[:pad]]) for w in level])
        k += 1
    return torch.stack(acc)


def _percentile_args(name, wc, ev, perm):
    """The arguments of a percentile window call: the numeric argument column in sorted order, the percentages as
    floats, and whether they came as ``array(...)``."""
    from .column import ArrayColumn
    from .decimal import is_decimal
    args = wc.func.args
    want = (1,) if name == "median" else (2,) if name == "percentile" else (2, 3)
    if wc.func.star or len(args) not in want:
        raise WindowError(f"wrong number of arguments to {name}")
    x = materialize(ev(args[0]))
    if isinstance(x, ConstColumn):
        x = x.materialize()
    if not isinstance(x, PrimColumn) or not (is_decimal(x.dtype) or x.dtype in _INT_TYPES + _FLOAT_TYPES):
        raise WindowError(f"{name} OVER needs a numeric argument")
    if len(args) == 3 and not isinstance(ev(args[2]), ConstColumn):
        raise WindowError(f"{name} accuracy must be a constant")             # accepted and ignored, as in GROUP BY
    if name == "median":
        return x.take(perm), [0.5], False
    p = ev(args[1])
    is_array = isinstance(p, ArrayColumn)
    consts = p.elements if is_array else [p]
    if not consts or not all(isinstance(c, ConstColumn) and c.value is not None for c in consts):
        raise WindowError(f"{name} percentage must be a constant or an array of constants")
    try:
        ps = [float(c.value) for c in consts]
    except (TypeError, ValueError):
        raise WindowError(f"{name} percentage must be a constant or an array of constants") from None
    if not all(0.0 <= q <= 1.0 for q in ps):
        raise WindowError("percentile must be in [0, 1]")
    return x.take(perm), ps, is_array


def _frame_percentile(name, x, ps, is_array, a, b, n, dev):
    """percentile / median / percentile_approx of ``x`` (sorted order) over the frames ``[a, b]`` for every
    percentage of ``ps``: GROUP BY's ranks on the frame's count of non-NULL rows, the rows at those ranks from
    ``_frame_select`` (all ranks of the call at once), then a gather — and, for the exact form, GROUP BY's
    interpolation on doubles (decimals through ``decimal.to_double``).  The approximate form returns an input value,
    so it keeps ``x``'s type."""
    from ..ops.sort import column_order_key
    from .column import ArrayColumn
    from .decimal import is_decimal, to_double
    from .query import _take_nullable, percentile_interpolate, percentile_ranks
    exact = FRAME_SELECT[name]
    key, valid = column_order_key(x)
    nonempty = a <= b
    vz = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(valid.to(torch.int64), 0)])
    cnt = torch.where(nonempty, vz[(b + 1).clamp(0, n)] - vz[a.clamp(0, n)], torch.zeros_like(a))
    has = cnt > 0
    plans = [percentile_ranks(q, cnt, exact) for q in ps]
    ranks = [r for plan in plans for r in plan[:2]]          # (lo, hi) per percentage, or (k,)
    length = torch.where(nonempty, b - a + 1, torch.zeros_like(a))
    maxlen = int(length.max())                               # one host read: the path choice
    at = _frame_select(key, valid, vz, a, b, ranks, maxlen)
    if exact:
        xd = to_double(x) if is_decimal(x.dtype) else PrimColumn("double", x.data.to(torch.float64), x.valid)
    out = []
    for j, plan in enumerate(plans):
        if exact:
            vl = _take_nullable(xd, at[2 * j]).data
            vh = _take_nullable(xd, at[2 * j + 1]).data
            out.append(PrimColumn("double", percentile_interpolate(vl, vh, plan[2]), has))
        else:
            out.append(_take_nullable(x, at[j]))             # -1 (no counted row): NULL
    if is_array:
        return ArrayColumn(out, n, None, False, dev)
    return out[0]


def _frame_select(key, valid, vz, a, b, ranks, maxlen):
    """For every rank tensor ``k`` of ``ranks``: the position of the ``k[i]``-th smallest counted row (0-based) of
    the frame ``[a[i], b[i]]`` (clipped to [0, n); ``a > b``: empty) in (``key`` unsigned, position) order, or -1
    where ``k[i]`` is negative or not below the frame's count.  ``key`` is one order-key word per row, ``valid`` the
    counted rows, ``vz`` their exclusive prefix count (n + 1 entries), ``maxlen`` the longest frame length.  Native
    on the GPU — ``SELECT_MAX_RANKS`` ranks per call — tensor operations on the CPU."""
    if maxlen == 0:
        return [torch.full_like(a, -1) for _ in ranks]
    if not N.use_native(key):
        return _frame_select_tensor(key, valid, vz, a, b, ranks)
    out = []
    tree = None
    for s in range(0, len(ranks), SELECT_MAX_RANKS):
        chunk = ranks[s:s + SELECT_MAX_RANKS]
        if maxlen <= FRAME_SELECT_DIRECT_MAX:
            out += _frame_select_direct(key, valid, a, b, chunk)
        else:
            tree = tree or _wavelet_build(key, valid)
            out += _frame_select_tree(tree, vz, a, b, chunk)
    return out


def _frame_select_direct(key, valid, a, b, ranks):
    n, m = int(key.shape[0]), len(ranks)
    k = torch.stack(ranks).contiguous()
    out = torch.empty((m, n), dtype=torch.int64, device=key.device)
    N.call("dxa_frame_select_direct", N.ptr(key.contiguous()), N.ptr(N.u8(valid).contiguous()), N.ptr(a.contiguous()),
           N.ptr(b.contiguous()), n, N.ptr(k), m, N.ptr(out), N.stream_handle(key.device))
    return list(out.unbind(0))


def _frame_select_tree(tree, vz, a, b, ranks):
    Z, perm = tree
    n, m = int(perm.shape[0]), len(ranks)
    k = torch.stack(ranks).contiguous()
    out = torch.empty((m, n), dtype=torch.int64, device=perm.device)
    N.call("dxa_frame_select_tree", N.ptr(Z), N.ptr(perm), N.ptr(vz.contiguous()), N.ptr(a.contiguous()),
           N.ptr(b.contiguous()), n, int(Z.shape[0]), N.ptr(k), m, N.ptr(out), N.stream_handle(perm.device))
    return list(out.unbind(0))


def _select_order(key, valid):
    """(perm, r): the stable sort permutation of the rows by (not counted, key unsigned) and its inverse, every
    row's global rank."""
    from ..ops.sort import argsort_words
    perm = argsort_words([key, (~valid).to(torch.int64)])
    r = torch.empty_like(perm)
    r[perm] = torch.arange(perm.shape[0], dtype=torch.int64, device=perm.device)
    return perm, r


def _wavelet_build(key, valid):
    """The wavelet matrix of window_select.hip over the rows' global ranks → (Z int32 [L, n + 1], perm): per level
    one prefix count of the zero bits (``torch.cumsum``) and one HIP launch that scatters the ranks into the next
    level's ordering and writes that level's zero flags.  No host read besides the radix sort's own."""
    perm, r = _select_order(key, valid)
    n = int(r.shape[0])
    dev = r.device
    L = (n - 1).bit_length()
    Z = torch.zeros((L, n + 1), dtype=torch.int32, device=dev)
    if L == 0:
        return Z, perm
    cur = r.to(torch.int32)
    nxt = torch.empty_like(cur)
    flags = ((cur >> (L - 1)) & 1) ^ 1
    st = N.stream_handle(dev)
    for lev in range(L):
        torch.cumsum(flags, 0, dtype=torch.int32, out=Z[lev, 1:])
        bit = L - 1 - lev
        if bit:
            N.call("dxa_wavelet_level", N.ptr(cur), N.ptr(Z[lev]), n, bit, N.ptr(nxt), N.ptr(flags), st)
            cur, nxt = nxt, cur
    return Z, perm


def _wavelet_build_tensor(key, valid):
    """``_wavelet_build`` as tensor operations on any device."""
    perm, cur = _select_order(key, valid)
    n = int(cur.shape[0])
    L = (n - 1).bit_length()
    Z = torch.zeros((L, n + 1), dtype=torch.int32, device=cur.device)
    idx = torch.arange(n, dtype=torch.int64, device=cur.device)
    for lev in range(L):
        bit = L - 1 - lev
        zero = ((cur >> bit) & 1) == 0
        zc = torch.cumsum(zero.to(torch.int64), 0)
        Z[lev, 1:] = zc.to(torch.int32)
        if bit:
            before = zc - zero.to(torch.int64)               # zeros among the earlier elements
            dst = torch.where(zero, before, zc[-1] + idx - before)
            nxt = torch.empty_like(cur)
            nxt[dst] = cur                                   # a stable partition: zeros first
            cur = nxt
    return Z, perm


def _frame_select_tensor(key, valid, vz, a, b, ranks, tree=None):
    """``_frame_select`` as vectorised tensor operations on any device — the wavelet-matrix walk of
    ``dxa_frame_select_tree``: per level, with c0 = Z[hi1] − Z[lo] zeros in the range, a rank below c0 goes left
    (lo = Z[lo], hi1 = Z[hi1]), else right (k −= c0, lo = z + lo − Z[lo], hi1 = z + hi1 − Z[hi1]); the bits taken
    are the answer's global rank, which the sort permutation turns into a row position."""
    Z, perm = tree if tree is not None else _wavelet_build_tensor(key, valid)
    n = int(perm.shape[0])
    lo, hi1 = a.clamp(min=0), (b + 1).clamp(max=n)           # frames are clipped to [0, n)
    empty = (a > b) | (lo >= hi1)
    lo = torch.where(empty, torch.zeros_like(lo), lo)
    hi1 = torch.where(empty, torch.zeros_like(hi1), hi1)
    cnt = vz[hi1] - vz[lo]
    Z = Z.to(torch.int64)
    out = []
    for k in ranks:
        ok = (k >= 0) & (k < cnt)
        zero = torch.zeros_like(lo)
        l, h, kk = torch.where(ok, lo, zero), torch.where(ok, hi1, zero), torch.where(ok, k, zero)
        rank = zero
        for lev in range(Z.shape[0]):
            z = Z[lev]
            zl, zh = z[l], z[h]
            c0 = zh - zl
            left = kk < c0
            l = torch.where(left, zl, z[n] + l - zl)
            h = torch.where(left, zh, z[n] + h - zh)
            kk = torch.where(left, kk, kk - c0)
            rank = rank * 2 + (~left).to(torch.int64)
        out.append(torch.where(ok, perm[rank.clamp(max=n - 1)], torch.full_like(rank, -1)))
    return out


def _distinct_args(name, wc, ev, perm):
    """The arguments of a distinct-count window call in sorted order: every row's value id — GROUP BY's own key
    equality (``G.group_rows``: NaN equals NaN, -0.0 equals 0.0; strings, decimals and tuples alike) — and the counted
    rows, those whose arguments are all non-NULL (``query._count_tuple``'s rule).  approx_count_distinct's rsd is
    never read, as GROUP BY never reads it: any expression is accepted there, constant or not."""
    from .column import StrColumn
    args = wc.func.args
    if name != COUNT_DISTINCT:
        if wc.func.star or len(args) not in (1, 2):
            raise WindowError(f"wrong number of arguments to {name}")
        args = args[:1]
    cols = []
    for e in args:
        x = materialize(ev(e))
        if isinstance(x, ConstColumn):
            x = x.materialize()
        if not isinstance(x, (PrimColumn, StrColumn)):
            raise WindowError(f"{name} OVER cannot count values of type {x.dtype}")
        cols.append(x)
    counted = cols[0].valid_mask()
    for c in cols[1:]:
        counted = counted & c.valid_mask()
    try:
        vid = G.group_rows(cols).gid.to(torch.int64)
    except TypeError as ex:
        raise WindowError(f"{name} OVER cannot count its argument: {ex}") from ex
    return vid[perm], counted[perm]


def _prev_occurrence(vid, counted) -> torch.Tensor:
    """int32 ``p``: for every counted row the position of the previous counted row with the same value id, -1 for
    a value's first counted occurrence, and the sentinel n for a row that is not counted.  ``vid`` holds dense ids
    in [0, n), as ``group_rows`` numbers them.  One stable radix argsort of the ids (rows that are not counted share
    an id of their own, n, which adds no byte to the sort) brings every value's rows together in position order; a
    neighbour compare does the rest."""
    from ..ops.sort import argsort_words
    n = int(vid.shape[0])
    ids = torch.where(counted, vid, torch.full_like(vid, n))
    order = argsort_words([ids])
    sid = ids[order]
    prev = torch.full_like(order, -1)
    prev[1:] = torch.where(sid[1:] == sid[:-1], order[:-1], prev[1:])
    prev = torch.where(sid == n, torch.full_like(prev, n), prev)
    p = torch.empty(n, dtype=torch.int32, device=vid.device)
    p[order] = prev.to(torch.int32)
    return p


def _frame_distinct(vid, counted, a, b, p=None) -> torch.Tensor:
    """The number of different value ids among the counted rows of every frame ``[a[i], b[i]]`` (clipped to [0, n);
    ``a > b``: empty, 0) as int64: with ``p`` the previous-occurrence array (computed here unless the caller has it),
    #{ j in the frame : p[j] < a[i] }.  Native on the GPU — a linear scan of ``p`` when the longest frame is at most
    ``FRAME_DISTINCT_DIRECT_MAX`` rows, else a wavelet matrix over ``p`` — tensor operations on the CPU."""
    length = torch.where(a <= b, b - a + 1, torch.zeros_like(a))
    maxlen = int(length.max())                               # one host read: the path choice
    if maxlen == 0:
        return torch.zeros_like(a)
    if p is None:
        p = _prev_occurrence(vid, counted)
    if not N.use_native(p):
        return _frame_distinct_tensor(p, counted, a, b)
    if maxlen <= FRAME_DISTINCT_DIRECT_MAX:
        return _frame_distinct_direct(p, a, b)
    return _frame_distinct_tree(_distinct_tree_build(p, counted), a, b)


def _frame_distinct_direct(p, a, b):
    n = int(p.shape[0])
    out = torch.empty(n, dtype=torch.int64, device=p.device)
    N.call("dxa_frame_distinct_direct", N.ptr(p), N.ptr(a.contiguous()), N.ptr(b.contiguous()), n, N.ptr(out),
           N.stream_handle(p.device))
    return out


def _distinct_tree_build(p, counted, tensor=False):
    """(Z, skey): the wavelet matrix of ``_wavelet_build`` with key p + 1 (unsigned, so -1 orders first) — global
    ranks order the rows by (not counted, p, position) — and the keys in that order, which ascend: a row that is not
    counted ranks last and its key, n + 1, is the largest."""
    key = p.to(torch.int64) + 1
    Z, perm = (_wavelet_build_tensor if tensor else _wavelet_build)(key, counted)
    return Z, key[perm]


def _distinct_threshold(skey, a):
    """T[i]: the number of counted rows of the whole array with p < lo[i], lo the clipped frame start — the global
    rank below which a row's previous occurrence lies before the frame.  A prefix count of p + 1 ≤ lo over the
    counted rows, read off the sorted keys by binary search (a histogram of p + 1 would put every first occurrence
    on one counter)."""
    n = int(skey.shape[0])
    return torch.searchsorted(skey, a.clamp(0, n - 1).contiguous(), right=True)


def _frame_distinct_tree(tree, a, b):
    Z, skey = tree
    n = int(skey.shape[0])
    T = _distinct_threshold(skey, a)
    out = torch.empty(n, dtype=torch.int64, device=skey.device)
    N.call("dxa_frame_distinct_tree", N.ptr(Z), N.ptr(T), N.ptr(a.contiguous()), N.ptr(b.contiguous()), n,
           int(Z.shape[0]), N.ptr(out), N.stream_handle(skey.device))
    return out


def _frame_distinct_tensor(p, counted, a, b, tree=None):
    """``_frame_distinct`` as vectorised tensor operations on any device — the wavelet-matrix walk of
    ``dxa_frame_distinct_tree``: count the frame's rows whose global rank is below T.  Per level, with c0 = Z[hi1] −
    Z[lo] zeros in the range: where T's bit is 1 add c0 and go right (lo = z + lo − Z[lo], hi1 = z + hi1 − Z[hi1]),
    where it is 0 go left (lo = Z[lo], hi1 = Z[hi1]).  T = 2^L (every row of a power-of-two array a counted first
    occurrence) is above every rank: the answer is the frame's length."""
    Z, skey = tree if tree is not None else _distinct_tree_build(p, counted, tensor=True)
    n = int(skey.shape[0])
    L = int(Z.shape[0])
    lo, hi1 = a.clamp(min=0), (b + 1).clamp(max=n)           # frames are clipped to [0, n)
    empty = (a > b) | (lo >= hi1)
    zero = torch.zeros_like(lo)
    l, h = torch.where(empty, zero, lo), torch.where(empty, zero, hi1)
    T = _distinct_threshold(skey, a)
    whole = T >= (1 << L)
    Z = Z.to(torch.int64)
    count = zero
    for lev in range(L):
        z = Z[lev]
        zl, zh = z[l], z[h]
        right = ((T >> (L - 1 - lev)) & 1).to(torch.bool)
        count = count + torch.where(right, zh - zl, zero)
        l = torch.where(right, z[n] + l - zl, zl)
        h = torch.where(right, z[n] + h - zh, zh)
    return torch.where(empty, zero, torch.where(whole, hi1 - lo, count))


def _collect_arg(name, wc, ev):
    """The one argument of collect_list / collect_set OVER, in input order: a primitive or string column (the types
    GROUP BY collects on the device, ``query.collectable``)."""
    from .query import collectable
    args = wc.func.args
    if wc.func.star or len(args) != 1:
        raise WindowError(f"{name} OVER takes one argument")
    x = materialize(ev(args[0]))
    if isinstance(x, ConstColumn):
        x = x.materialize()
    if not collectable(x):
        raise WindowError(f"{name} OVER cannot collect values of type {x.dtype}")
    return x


def _frame_collect(name, x, a, b):
    """collect_list / collect_set of ``x`` (sorted order) over every frame ``[a[i], b[i]]``: an array column, never
    NULL, empty where the frame is empty or holds no counted (non-NULL) row.  Elements stand in the frame's sorted
    order; the set keeps every value's first row inside the frame, by GROUP BY's equality (``G.group_rows``), so
    its size is ``count(DISTINCT x)`` over the same frame.  The slots are a ``[K, n]`` matrix of sorted-order
    positions (``_frame_collect_positions``), K the largest per-frame count — one host read beside the longest
    frame — and the element columns one gather of ``x``'s leaves over the flattened matrix."""
    from ..ops.gather import gather_many
    from .query import array_from_slots, slot_leaves
    n, dev = x.length, x.device
    as_set = name == "collect_set"
    counted = x.valid_mask()
    length = torch.where(a <= b, b - a + 1, torch.zeros_like(a))
    p = None
    if as_set:
        try:
            vid = G.group_rows([x]).gid.to(torch.int64)
        except TypeError as ex:
            raise WindowError(f"{name} OVER cannot collect its argument: {ex}") from ex
        p = _prev_occurrence(vid, counted)
        cnt = _frame_distinct(vid, counted, a, b, p)
    else:
        pz = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counted.to(torch.int64), 0)])
        cnt = torch.where(a <= b, pz[(b + 1).clamp(0, n)] - pz[a.clamp(0, n)], torch.zeros_like(a))
    maxlen, K, kmin = torch.stack([length.max(), cnt.max(), cnt.min()]).tolist()
    if K * n > FRAME_COLLECT_MAX_SLOTS:
        raise WindowError(f"{name} OVER: the frame is too long to collect: {n} rows of up to {K} elements need "
                          f"{K * n} slots, more than FRAME_COLLECT_MAX_SLOTS ({FRAME_COLLECT_MAX_SLOTS})")
    if K == 0:
        return array_from_slots(x, None, n, None, None)
    pos = _frame_collect_positions(a, b, counted, p, K, maxlen)
    flat = pos.reshape(-1)
    leaves = slot_leaves(x)
    if N.use_native(flat):
        # gather_many reads an index outside [-n, n) as zero: the absent slots
        mats = [t.view(K, n) for t in gather_many(leaves, torch.where(flat < 0, torch.full_like(flat, n), flat))]
    else:
        have = pos >= 0
        at = pos.clamp(min=0)
        mats = [torch.where(have, t[at], torch.zeros((), dtype=t.dtype, device=dev)) for t in leaves]
    ragged = kmin != K
    valid = (pos >= 0) if ragged else None
    return array_from_slots(x, mats, n, valid, valid.t().contiguous() if ragged else None)


def _frame_collect_positions(a, b, counted, p, K, maxlen) -> torch.Tensor:
    """``[K, n]`` int64: row i's column holds, top down, the positions j in ``[a[i], b[i]]`` (clipped to [0, n)) with
    ``counted[j]`` and — for the set, ``p`` the previous-occurrence array — ``p[j] < a[i]``; -1 below them.  Native
    on the GPU (``dxa_frame_collect``: one launch, one thread per row; a wave-per-row shape was measured and was
    never faster, profiles/collect/README.md); on a CPU device the list's positions come from the prefix count of
    ``counted`` and the set's from a scan over the frame offsets."""
    n, dev = int(a.shape[0]), a.device
    if N.use_native(a):
        out = torch.empty((K, n), dtype=torch.int64, device=dev)
        N.call("dxa_frame_collect", N.ptr(a.contiguous()), N.ptr(b.contiguous()), N.ptr(N.u8(counted.contiguous())),
               N.ptr(p), n, K, N.ptr(out), N.stream_handle(dev))
        return out
    lo, hi1 = a.clamp(min=0), (b + 1).clamp(max=n)             # frames are clipped to [0, n)
    empty = (a > b) | (lo >= hi1)
    zero = torch.zeros_like(lo)
    lo, hi1 = torch.where(empty, zero, lo), torch.where(empty, zero, hi1)
    if p is None:
        pz = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counted.to(torch.int64), 0)])
        cpos = torch.nonzero(counted).flatten()                # K > 0: at least one counted row
        k = torch.arange(K, dtype=torch.int64, device=dev)[:, None]
        have = k < (pz[hi1] - pz[lo])[None, :]
        at = cpos[(pz[lo][None, :] + k).clamp(max=int(cpos.shape[0]) - 1)]
        return torch.where(have, at, torch.full_like(at, -1))
    out = torch.full((K, n), -1, dtype=torch.int64, device=dev)
    s = torch.zeros_like(lo)
    p64 = p.to(torch.int64)
    for d in range(int(maxlen)):
        j = lo + d
        keep = (j < hi1) & (p64[j.clamp(max=n - 1)] < lo)      # a row that is not counted has p = n
        r = torch.nonzero(keep).flatten()
        out[s[r], r] = j[r]
        s = s + keep.to(torch.int64)
    return out


def _float_frame_sum(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, nonempty: torch.Tensor) -> torch.Tensor:
    """Σ x[a[i] .. b[i]] for doubles WITHOUT prefix-sum differences (those cancel catastrophically: a 2-row frame
    over values of 1.6e12 inherits the rounding of a prefix of 3e17).  Every frame is cut into aligned power-of-two
    blocks by the bits of its length, lowest bit first: level k holds the sums of the 2^k-row runs starting at every
    row (one add of level k-1 per level), so a frame sum adds at most log2(len) block sums — each the sum of values
    inside the frame only, and exact Spark order for frames of one or two rows.  Memory stays O(n): one level at a
    time."""
    n = x.shape[0]
    length = torch.where(nonempty, b - a + 1, torch.zeros_like(a))
    acc = torch.zeros_like(x)
    if n == 0:
        return acc
    maxlen = int(length.max())                                     # one host read (the level count)
    pos = a.clamp(0, n - 1)
    level = x
    k = 0
    while (1 << k) <= maxlen:
        take = ((length >> k) & 1).to(torch.bool)
        acc = acc + torch.where(take, level[pos], torch.zeros_like(acc))
        pos = torch.where(take, (pos + (1 << k)).clamp(max=n - 1), pos)
        step = 1 << k
        if (step << 1) <= maxlen:
            nxt = level.clone()
            nxt[: n - step] = level[: n - step] + level[step:]
            level = nxt
        k += 1
    return acc


def _decimal_frame_agg(name, x, valid, a, b, nonempty, cnt, has, n, dev):
    """Framed SUM / AVG / MIN / MAX over decimal(p, s) with Spark's result types: SUM → decimal(p+10, s), AVG →
    decimal(p+4, s+4) rounded HALF_UP, MIN / MAX → the input type.  Sums are exact: the unscaled 128-bit values are
    split into 32-bit limbs whose int64 prefix sums cannot overflow below 2^31 rows, so frame differences of those
    prefixes are exact; the limbs are then carried back together (as ``decimal.group_sum`` does per group)."""
    from . import decimal as D
    t = x.dtype
    h, l = D.lanes(x.data)
    if name in ("min", "max"):
        is_max = name == "max"
        if t.narrow:
            info = torch.iinfo(torch.int64)
            fill = info.min if is_max else info.max
            masked = torch.where(valid, x.data, torch.full_like(x.data, fill))
            return PrimColumn(t, _minmax_frame(masked, a, b, is_max), has)
        at = _argbest_frame(h, l ^ D.SIGN, valid, a, b, is_max)
        return PrimColumn(t, x.data[at], has)
    z = torch.zeros_like(l)
    h = torch.where(valid, h, z)
    l = torch.where(valid, l, z)
    parts = D._limbs(h, l)[:3] + [h >> 32]                   # three unsigned limbs + the signed top limb
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    sums = []
    for p in parts:
        pz = torch.cat([zero, torch.cumsum(p, 0)])
        d = pz[(b + 1).clamp(0, n)] - pz[a.clamp(0, n)]
        sums.append(torch.where(nonempty, d, torch.zeros_like(d)))
    c = torch.zeros_like(sums[0])
    out = []
    for k in range(3):
        v = sums[k] + c
        out.append(v & D.MASK32)
        c = v >> 32
    hi = (out[2] & D.MASK32) | ((sums[3] + c) << 32)
    lo = (out[0] & D.MASK32) | ((out[1] & D.MASK32) << 32)
    if name == "sum":
        ts = D.result_sum(t)
        return D.column(ts, hi, lo, has & D.fits(hi, lo, ts.precision))
    ta = D.result_avg(t)
    hh, ll, ovf = D.mul_pow10(hi, lo, ta.scale - t.scale)
    hh, ll = D.div_u_vec_half_up(hh, ll, cnt.clamp(min=1))
    return D.column(ta, hh, ll, has & ~ovf & D.fits(hh, ll, ta.precision))


def _argbest_frame(kh: torch.Tensor, kl: torch.Tensor, valid, a, b, is_max: bool) -> torch.Tensor:
    """Row index of the max / min (kh, kl) key (lexicographic, signed) inside every frame: a sparse table of
    row indices (wide decimals, whose order key is two words)."""
    n = kh.shape[0]
    big = torch.iinfo(torch.int64)
    fill = big.min if is_max else big.max
    kh = torch.where(valid, kh, torch.full_like(kh, fill))
    kl = torch.where(valid, kl, torch.full_like(kl, fill))

    def better(i, j):                               # index of the better of rows i, j (ties: the earlier)
        gt = (kh[j] > kh[i]) | ((kh[j] == kh[i]) & (kl[j] > kl[i]))
        lt = (kh[j] < kh[i]) | ((kh[j] == kh[i]) & (kl[j] < kl[i]))
        return torch.where(gt if is_max else lt, j, i)
    idx = torch.arange(n, device=kh.device)
    levels = [idx]
    k = 1
    while 2 * k <= n:
        prev = levels[-1]
        nxt = prev.clone()
        nxt[: n - k] = better(prev[: n - k], prev[k:])
        levels.append(nxt)
        k *= 2
    table = torch.stack(levels)
    length = (b - a + 1).clamp(min=1)
    lvl = torch.floor(torch.log2(length.to(torch.float64))).to(torch.int64).clamp(max=len(levels) - 1)
    lvl = torch.where((1 << lvl) > length, lvl - 1, lvl)
    span = 1 << lvl
    ai = a.clamp(0, n - 1)
    bi = (b - span + 1).clamp(0, n - 1)
    return better(table[lvl, ai], table[lvl, bi])
