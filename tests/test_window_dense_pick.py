"""first / last / max_by / min_by over sliding windows from the dense ring (window_dense.py ``plan_layout`` /
``DenseWindow.accumulate`` / ``_ordered_slots``, window_ring.hip win_pick_kernel / win_pick_gather_kernel /
win_combine_kernel's pick branch).  The oracle is the CPU evaluator over the materialised window (``ops/groupby``'s
first / last and ``query._arg_extreme``; no GPU code and no merge in it).

Everything compares exactly — equal dtype strings, equal values, NULL with NULL, NaN with NaN, and the sign of a zero —
because a pick copies bits.  The sums beside the picks (AVG of multiples of 0.25) are exact in any order, so they
compare exactly too.  Every GPU test asserts that the statement stayed on the ring (``disabled_reason is None``)
unless it tests a fallback: before row picks were eligible ``first`` disabled the state and ``max_by`` never reached
the ring, so no dense state existed for it."""
import math

import pytest
import torch

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from tests.window_dense_support import (S, Comparison, aggs_of, as_partitioned_world_of_one, churn_stream,
                                        dense_states, layout_of, materialised, new_store, on_the_ring, only_state,
                                        run_stream, set_caps, steady_state_launches, two_rows_per_id_stream)

BITS = Comparison("bits", order_by="deviceId")
D18 = "CAST(serial AS DECIMAL(18,2))"
YDEC = "CAST(y3 AS DECIMAL(10,1))"
Q_MIXED = ("SELECT deviceId, COUNT(*) AS c, first(serial) AS f, last(serial) AS l, max_by(serial, y3) AS mx, "
           "min_by(serial, y3) AS mn, AVG(hum) AS ah, MAX(y3) AS my, first(temp) AS ft, last_value(temp) AS lt, "
           "max_by(temp, y3) AS mt FROM W GROUP BY deviceId")
Q_TIES = ("SELECT deviceId, COUNT(*) AS c, max_by(serial, y3) AS mx, min_by(serial, y3) AS mn, first(serial) AS f, "
          "last(serial) AS l FROM W GROUP BY deviceId")
Q_WHERE = ("SELECT deviceId, COUNT(*) AS c, first(serial) AS f, last(serial) AS l, max_by(serial, y3) AS mx, "
           "min_by(serial, y3) AS mn FROM W WHERE keep = 1 GROUP BY deviceId")
Q_TYPES = (f"SELECT deviceId, COUNT(*) AS c, first(temp) AS ft, last(f) AS lf, max_by(flag, yd) AS bf, "
           f"min_by(ev, yd) AS ne, max_by({D18}, ev) AS xd, min_by(temp, {YDEC}) AS nt, max_by(temp, yd) AS xt, "
           "last(flag) AS lb FROM W GROUP BY deviceId")
Q_FIRST_LAST = ("SELECT deviceId, COUNT(*) AS c, first(serial) AS f, last(temp) AS lt, last(flag) AS lb, "
                f"first({D18}) AS fd, AVG(hum) AS ah FROM W GROUP BY deviceId")
Q_STR = "SELECT deviceId, COUNT(*) AS c, first(name) AS fn FROM W GROUP BY deviceId"
Q_STR_BY = "SELECT deviceId, COUNT(*) AS c, max_by(name, y3) AS mn FROM W GROUP BY deviceId"
Q_PLAIN = ("SELECT deviceId, COUNT(*) AS c, SUM(y3) AS s, MIN(y3) AS mn, MAX(y3) AS mx, AVG(hum) AS av "
           "FROM W GROUP BY deviceId")
NAN = float("nan")


def batch(rng, b, T, ids, spread, bait=False):
    """Batch ``b`` with the given device ids, event times within ``spread`` before ``T``.  ``serial`` is unique over the
    stream (so a wrong pick shows); ``y3`` is drawn from three values with NULLs (every group ties inside a pane and
    across panes); ``yd`` is a double from {-2.0, -0.0, 0.0, 1.5, NaN} with NULLs; ``temp`` a double with NULLs, NaN and
    -0.0; ``f`` a float; ``flag`` a boolean with NULLs; ``ev`` a timestamp from four values; ``hum`` a multiple of
    0.25.  Device 900 has NULL ``y3`` and ``yd`` in every row.  ``bait``: the first row of every device has the largest
    ``y3`` and the last row the smallest, both with ``keep`` = 0 — rows a WHERE on ``keep`` removes and that would
    otherwise win every pick."""
    import numpy as np
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    ts = T - rng.integers(0, spread, n)
    serial = b * 100_000 + np.arange(n)
    y3 = rng.choice([10, 20, 30], n)
    y3_ok = (rng.random(n) > 0.15) & (ids != 900)
    yd = rng.choice([-2.0, -0.0, 0.0, 1.5, NAN], n)
    yd_ok = (rng.random(n) > 0.15) & (ids != 900)
    temp = rng.integers(-40, 120, n) * 0.5
    temp[rng.random(n) < 0.1] = NAN
    temp[rng.random(n) < 0.1] = -0.0
    temp_ok = rng.random(n) > 0.2
    f = rng.integers(-1000, 1000, n) / 8.0
    flag = rng.random(n) > 0.5
    flag_ok = rng.random(n) > 0.2
    ev = T - rng.choice([0, 1, 2, 3], n) * 1000
    keep = np.ones(n, dtype=np.int64)
    if bait:
        for d in np.unique(ids):
            at = np.flatnonzero(ids == d)
            if len(at) >= 4:
                y3[at[0]], y3_ok[at[0]], keep[at[0]] = 99, True, 0
                y3[at[-1]], y3_ok[at[-1]], keep[at[-1]] = -99, True, 0
    name = strings_from_pylist([f"n{int(v) % 7}" for v in serial], "cpu")
    return Table(["ts", "deviceId", "serial", "y3", "yd", "temp", "f", "flag", "ev", "hum", "keep", "name"],
                 [PrimColumn("timestamp", torch.tensor(ts, dtype=torch.int64)),
                  PrimColumn("long", torch.tensor(ids, dtype=torch.int64)),
                  PrimColumn("long", torch.tensor(serial, dtype=torch.int64)),
                  PrimColumn("long", torch.tensor(y3, dtype=torch.int64), torch.tensor(y3_ok)),
                  PrimColumn("double", torch.tensor(yd, dtype=torch.float64), torch.tensor(yd_ok)),
                  PrimColumn("double", torch.tensor(temp, dtype=torch.float64), torch.tensor(temp_ok)),
                  PrimColumn("float", torch.tensor(f, dtype=torch.float64)),
                  PrimColumn("boolean", torch.tensor(flag), torch.tensor(flag_ok)),
                  PrimColumn("timestamp", torch.tensor(ev, dtype=torch.int64)),
                  PrimColumn("double", torch.tensor(rng.integers(0, 256, n) * 0.25, dtype=torch.float64)),
                  PrimColumn("long", torch.tensor(keep)), name], n, "cpu")


def small_stream(nb, groups=4, rows=40, whole=True, bait=False, seed=43):
    """``rows`` rows per batch over ``groups`` ids and two rows of device 900.  ``whole``: event times in the middle
    half of the batch's second, so a pane is wholly inside a window or wholly outside it; else spread over a whole
    second around the boundary before the batch time, so the panes at both edges of a window are clipped."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for b in range(nb):
        ids = np.concatenate([rng.integers(0, groups, rows), [900, 900]])
        rng.shuffle(ids)
        T = (100 + b) * S
        out.append((T, batch(rng, b, T - S // 4, ids, S // 2, bait) if whole else
                    batch(rng, b, T - S // 2, ids, S - 1, bait), ids))
    return out


def numbered(rng, T, ids):
    """``batch`` for the shared stream builders: batch ``T // S - 100``, event times over the whole second."""
    return batch(rng, T // S - 100, T, ids, S - 1)


def newest_first(view):
    """The same window with its newest pane listed first, as a view lists the current pane before the retained ones:
    the window's row order is then not the order of the pane keys.  (The store's own views never hold rows of the
    current pane — it keeps the rows at or after the window's end — so the order is made here.)"""
    from dxa.engine.windows import PanedTable
    inside = [p for p, _full in view.pieces()]
    if not inside:
        return view
    newest = max(inside, key=lambda p: p.key)
    panes = [newest] + [p for p in view.panes if p is not newest]
    return PanedTable(view.store, panes, view.lo, view.hi, view.names, view._device)


def _layout(aggs):
    import numpy as np
    reqs, _types, L = layout_of(aggs, batch(np.random.default_rng(0), 0, 100 * S, np.arange(4), S), picks=True)
    return reqs, L


def _words(L):
    where = {i: w for w, i in enumerate(L["order"]) if i is not None}
    return {k[0]: where[i] for i, k in enumerate(L["slots"])}


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_layout_of_single_picks():
    """first / last: a rank word in a line of the rank op and a payload and a validity word in a line of the value op,
    all unused by agg_multi, described by ``pickdesc``; the finishing recipe is the default kind over P with V as the
    count word; ``first`` has the partial state "v" of ``distagg._partials``.  max_by / min_by add the key word, an
    ordinary MAX slot of y (complemented for min_by), and have no partial."""
    from dxa.ops.groupby import (_F_I64, _MA_ADD_F64, _MA_MAX, _MA_PICK_RANK, _MA_PICK_VAL, _MV_I64, _MV_NOT,
                                 _PICK_LAST, _PICK_USED)
    for func, last in (("first", 0), ("last", _PICK_LAST), ("first_value", 0), ("last_value", _PICK_LAST)):
        aggs = aggs_of(f"{func}(temp)")
        reqs, L = _layout(aggs)
        assert reqs[0][1] == ("last" if last else "first")
        xk = reqs[0][2].key()
        rank = (reqs[0][1],)
        assert L["line_ops"] == [_MA_ADD_F64, _MA_PICK_RANK, _MA_PICK_VAL] and L["stride"] == 24
        assert [(s[0][0], s[1], s[2]) for s in L["slots"][1:]] == [
            ("pickr", -1, _MA_PICK_RANK), ("pickp", -1, _MA_PICK_VAL), ("pickv", -1, _MA_PICK_VAL)]
        w = _words(L)
        assert (w[("pickr", rank)], w[("pickp", (rank, xk))], w[("pickv", (rank, xk))]) == (8, 16, 17)
        want = [0] * 24
        want[8] = want[16] = want[17] = 8 | last | _PICK_USED
        assert L["pickdesc"] == want
        assert L["pickargs"] == ([(None, 0, -1, 8, int(bool(last)))], [(xk, 8, 16, 17, int(bool(last)))])
        assert L["fin"] == [(_F_I64, 16, 17)] and L["plan"][0][1:] == ("pick", 2, 3, "double") and L["as_f64"] == [True]
        assert L["pfin"] == {list(aggs)[0]: {"v": (_F_I64, 16, 17)}}
    for func, inv in (("max_by", 0), ("min_by", _MV_NOT)):
        aggs = aggs_of(f"{func}(serial, ts)")
        reqs, L = _layout(aggs)
        x, y = reqs[0][2]
        assert L["line_ops"] == [_MA_ADD_F64, _MA_MAX, _MA_PICK_RANK, _MA_PICK_VAL]
        assert L["slots"][1] == ((func[:3], y.key()), _MV_I64 | inv, _MA_MAX)
        want = [0] * 32
        want[16] = want[24] = want[25] = 16 | (8 + 1) << 8 | _PICK_USED
        assert L["pickdesc"] == want
        assert L["pickargs"] == ([(y.key(), _MV_I64 | inv, 8, 16, 0)], [(x.key(), 16, 24, 25, 0)])
        assert L["fin"] == [(_F_I64, 24, 25)] and L["plan"][0][4] == "long" and L["as_f64"] == [False]
        assert L["pfin"] == {}


def test_picks_share_rank_and_key_words():
    """max_by(a, y), max_by(b, y) and MAX(y) share K; the two picks share R and have a P and a V each; first(a) and
    first(b) share one R; min_by of the same y has a K and an R of its own; a double y is keyed by its normalised
    copy, which MAX(y) does not read."""
    from dxa.engine.window_dense import pick_y_key
    from dxa.ops.groupby import _MA_MAX, _MA_PICK_RANK, _MA_PICK_VAL, _MV_F64_ORD
    reqs, L = _layout(aggs_of("max_by(serial, ts)", "max_by(temp, ts)", "MAX(ts)", "first(serial)", "first(temp)",
                            "min_by(serial, ts)", "COUNT(*)"))
    ops = [s[2] for s in L["slots"]]
    assert ops.count(_MA_MAX) == 2 and ops.count(_MA_PICK_RANK) == 3 and ops.count(_MA_PICK_VAL) == 10
    w = _words(L)
    y = reqs[0][2][1].key()
    kmax, kmin = w[("max", y)], w[("min", y)]
    rmax, rfirst = w[("pickr", ("max_by", y))], w[("pickr", ("first",))]
    ranks, vals = L["pickargs"]
    assert sorted(r[2:4] for r in ranks) == sorted([(kmax, rmax), (-1, rfirst), (kmin, w[("pickr", ("min_by", y))])])
    assert len(vals) == 5 and [v[1] for v in vals].count(rmax) == 2 and [v[1] for v in vals].count(rfirst) == 2
    assert len({v[2] for v in vals} | {v[3] for v in vals}) == 10
    # MAX(ts) is finished from the shared key word
    assert L["fin"][2][1] == kmax
    used = [d for d in L["pickdesc"] if d]
    assert len(used) == 13 and sum(1 for d in used if (d >> 8) & 0xff == kmax + 1) == 5
    # a double y: the pick's key slot reads the copy with -0.0 → 0.0, MAX(yd) keeps its own slot
    reqs, L = _layout(aggs_of("max_by(serial, yd)", "MAX(yd)"))
    y = reqs[0][2][1]
    keys = [s[0] for s in L["slots"] if s[2] == _MA_MAX]
    assert keys == [("max", pick_y_key(y)), ("max", y.key())]
    assert L["pickargs"][0][0][:2] == (pick_y_key(y), _MV_F64_ORD)


def test_refusals_and_layouts_without_picks():
    from dxa.engine.window_dense import MAX_PICK, Ineligible, _requests
    assert MAX_PICK == 8
    # nine different order keys: nine rank jobs
    with pytest.raises(Ineligible, match="too many pick arguments"):
        _requests(aggs_of(*[f"max_by(serial, y3 + {k})" for k in range(9)]), picks=True)
    # one rank job, nine payload jobs
    with pytest.raises(Ineligible, match="too many pick arguments"):
        _requests(aggs_of(*[f"first(serial + {k})" for k in range(9)]), picks=True)
    _requests(aggs_of(*[f"first(serial + {k})" for k in range(8)]), picks=True)
    _requests(aggs_of("last(serial)", *[f"max_by(serial, y3 + {k})" for k in range(7)]), picks=True)
    # the two-argument form keeps the reason it had
    with pytest.raises(Ineligible, match="^first$"):
        _requests(aggs_of("first(temp, true)"), picks=True)
    with pytest.raises(Ineligible, match="^max_by$"):
        _requests(aggs_of("max_by(temp)"), picks=True)
    # a caller that does not promise the window's row order gets no picks
    for item in ("first(temp)", "max_by(temp, ts)"):
        with pytest.raises(Ineligible):
            _requests(aggs_of(item))
    # a two-lane decimal payload or order key
    for item in ("first(serial * 1.5)", "max_by(serial, serial * 1.5)", "min_by(serial * 1.5, y3)"):
        with pytest.raises(Ineligible, match="argument type"):
            _layout(aggs_of(item))
    _r, L = _layout(aggs_of("COUNT(*)", "SUM(y3)", "MIN(y3)", "AVG(hum)"))
    assert "pickdesc" not in L and "pickargs" not in L and not {6, 7} & set(L["line_ops"])
    assert L["fin"] == [(0, 8, -1), (1, 0, 9), (9, 16, 9), (3, 11, 10)]


def test_cpu_stream_takes_the_other_paths():
    """On a CPU device first / last are answered from pane partials and max_by / min_by by the generic evaluator: no
    dense state, and the streams' results equal the oracle (which guards the helpers)."""
    store = new_store(5)
    run_stream(small_stream(8, whole=False), [Q_MIXED, Q_TYPES], torch.device("cpu"), store, BITS)
    assert not dense_states(store)


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_statement(gpu):
    """4 groups, 40 rows per batch, a 5-s window, 12 batches: the four picks beside COUNT(*), AVG and MAX(y)."""
    store = new_store(5)
    run_stream(small_stream(12), [Q_MIXED], gpu, store, BITS)
    d, = on_the_ring(store)
    assert len(d.layout["pickargs"][0]) == 4 and d.pickdesc_dev is not None


@pytest.mark.gpu
def test_ties_inside_and_across_panes(gpu):
    """``y3`` has three values, so every group ties inside a pane and across panes, and ``serial`` shows which row was
    picked.  The window's newest pane is listed first (``newest_first``): a group's extreme ``y3`` is seen both there
    and in older panes, and then the newest pane's row must win although its key is the largest."""
    store = new_store(5)
    seen = {"newest": 0, "older": 0}

    def each(b, q, rows, view, table):
        first = view.pieces()[0][0].key // S - 100 if view.pieces() else -1
        for r in rows:
            if r["deviceId"] < 900 and r["mx"] is not None:
                seen["newest" if r["mx"] // 100_000 == first else "older"] += 1

    run_stream(small_stream(12), [Q_TIES], gpu, store, BITS, each, reorder=newest_first)
    on_the_ring(store)
    assert seen["newest"] > 12 and seen["older"] > 0, seen


@pytest.mark.gpu
def test_nulls(gpu):
    """Rows with NULL y are present and never win; device 900 has no non-NULL y (NULL max_by / min_by, but a first and
    a last); winning rows and first / last rows whose x is NULL give NULL."""
    store = new_store(5)
    q = ("SELECT deviceId, COUNT(*) AS c, COUNT(y3) AS ny, max_by(temp, y3) AS mt, min_by(flag, y3) AS nf, "
         "first(temp) AS ft, last(flag) AS lf, first(serial) AS f FROM W GROUP BY deviceId")
    seen = {"allnull": 0, "nullx": 0, "nullfirst": 0}

    def each(b, _q, rows, view, table):
        for r in rows:
            if r["deviceId"] == 900:
                assert r["ny"] == 0 and r["mt"] is None and r["nf"] is None and r["f"] is not None, r
                seen["allnull"] += 1
            elif r["ny"] > 0 and (r["mt"] is None or r["nf"] is None):
                seen["nullx"] += 1
            if r["ft"] is None or r["lf"] is None:
                seen["nullfirst"] += 1

    run_stream(small_stream(12), [q], gpu, store, BITS, each)
    on_the_ring(store)
    assert seen["allnull"] >= 10 and seen["nullx"] > 0 and seen["nullfirst"] > 0, seen


@pytest.mark.gpu
def test_clipped_panes(gpu):
    """Event times spread over the whole batch second: the panes at the window's edges are partly inside it and are
    accumulated into scratch slots, which take their panes' places in the window's order."""
    store = new_store(5)
    seen = {"clipped": 0}

    def each(b, q, rows, view, table):
        seen["clipped"] += sum(1 for _p, full in view.pieces() if not full)

    run_stream(small_stream(12, whole=False), [Q_MIXED], gpu, store, BITS, each)
    on_the_ring(store)
    assert seen["clipped"] >= 10, seen


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["store", "newest"])
def test_blocks_form_and_expire(gpu, order):
    """A 40-pane window over 66 batches of the tie-heavy stream, in the store's order and with the newest pane listed
    first: complete 16-pane blocks are pre-combined where their members stand together in the window's order — never
    the block whose newest member stands first, away from the others — and expire.  The run includes the batches in
    which the newest pane completes a block."""
    store = new_store(40)
    seen = {"blocks": set(), "most": 0}

    def each(b, q, rows, view, table):
        if not dense_states(store):                 # (the watermark keeps the first windows empty)
            return
        d = only_state(store)
        seen["blocks"] |= set(d.blocks)
        seen["most"] = max(seen["most"], len(d.blocks))
        seen["now"] = set(d.blocks)

    run_stream(small_stream(66), [Q_TIES], gpu, store, BITS, each,
               reorder=newest_first if order == "newest" else None)
    on_the_ring(store)
    assert len(seen["blocks"]) >= 3 and seen["most"] >= 2 and seen["blocks"] - seen["now"], seen


@pytest.mark.gpu
def test_straddles_the_lds_bound(gpu, monkeypatch):
    """About 1,500 groups — ids on both sides of the pick pass's LDS bound — and 3,000 rows per batch."""
    from dxa.engine import window_dense
    from dxa.ops import native as N
    L = N.lib().dxa_win_m2_lds_groups()
    assert 0 < L < 1500
    if 3000 > window_dense.DENSE_GROUPS:
        monkeypatch.setattr(window_dense, "DENSE_GROUPS", 4096)
    store = new_store(5)
    run_stream(two_rows_per_id_stream(numbered, 8, 1500), [Q_TIES], gpu, store, BITS)
    on_the_ring(store)


@pytest.mark.gpu
def test_rebuild_moves_the_pick_words(gpu, monkeypatch):
    """Ids drift through a 16-id dictionary that grows to 64 at most: every rebuild renumbers the rank, payload and
    validity words with the others."""
    set_caps(monkeypatch, 16, 64, block=2)
    store = new_store(5)
    run_stream(churn_stream(numbered, 30, rows=120), [Q_MIXED], gpu, store, BITS)
    d, = on_the_ring(store)
    assert d.rebuilds > 0 and d.gcap <= 64


@pytest.mark.gpu
def test_where_removes_the_would_be_winners(gpu):
    """Every device's first row has the largest y and its last row the smallest, and WHERE removes both: they go to
    the dump row and win nothing."""
    store = new_store(5)
    seen = {"bait": 0}

    def each(b, q, rows, view, table):
        mat = materialised(view)
        baits = {s for s, k in zip(mat.column("serial").to_pylist(), mat.column("keep").to_pylist()) if k == 0}
        seen["bait"] += len(baits)
        for r in rows:
            assert not {r["f"], r["l"], r["mx"], r["mn"]} & baits, r

    run_stream(small_stream(12, bait=True), [Q_WHERE], gpu, store, BITS, each)
    on_the_ring(store)
    assert seen["bait"] > 50, seen


@pytest.mark.gpu
def test_argument_types(gpu):
    """x: double (NaN, -0.0), float, boolean, timestamp, decimal(18,2); y: double (NaN the largest; -0.0 and 0.0 tie,
    and the first row wins), timestamp, decimal(10,1).  The results have x's type."""
    store = new_store(5)
    seen = {"nan": 0, "negzero": 0}

    def each(b, q, rows, view, table):
        for r in rows:
            for nm in ("ft", "xt", "nt"):
                v = r[nm]
                if isinstance(v, float):
                    seen["nan"] += math.isnan(v)
                    seen["negzero"] += v == 0.0 and math.copysign(1.0, v) < 0

    run_stream(small_stream(12, whole=False), [Q_TYPES], gpu, store, BITS, each)
    d, = on_the_ring(store)
    assert seen["nan"] > 0 and seen["negzero"] > 0, seen
    dts = [str(p[4]) for p in d.layout["plan"]]
    assert dts == ["None", "double", "float", "boolean", "timestamp", "decimal(18,2)", "double", "double", "boolean"]


@pytest.mark.gpu
def test_string_payload_falls_back(gpu):
    """first(name) of a string: the state is disabled with "argument type" and the paned path answers; max_by(name, y)
    is disabled likewise and the generic path answers.  Both equal the oracle."""
    store = new_store(5)
    run_stream(small_stream(8), [Q_STR, Q_STR_BY], gpu, store, BITS)
    states = list(dense_states(store).values())
    assert len(states) == 2
    for d in states:
        assert d.disabled and d.disabled_reason == "argument type"


@pytest.mark.gpu
@pytest.mark.parametrize("q,picks", [(Q_PLAIN, 0), (Q_TIES, 1)])
def test_one_pick_pass_per_accumulated_pane(gpu, monkeypatch, q, picks):
    """In steady state (one pane enters the window per batch, nothing is rebuilt) a statement without picks issues the
    entry points tests/test_window_dense_comoments.py pins and never ``dxa_win_pick``; a pick statement calls it once
    per accumulated pane, right after the multi-aggregate."""
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "BLOCK", 2)
    store = new_store(6)
    pane = ["dxa_win_insert_fused", "dxa_aggregate_multi", *["dxa_win_pick"] * picks]
    completed_seen = set()
    # the watermark and the 6-pane window: full from batch 7 on
    for b, native, completed in steady_state_launches(gpu, store, small_stream(14), q, BITS, 8):
        d, = on_the_ring(store)
        assert d.rebuilds == 0 and d.has_picks == bool(picks)
        completed_seen.add(completed)
        assert native == pane + ["dxa_win_combine_block"] * completed + ["dxa_win_answer"], (b, native)
    assert completed_seen == {0, 1}
    d = only_state(store)
    assert (d.pickdesc_dev is not None) == bool(picks)


@pytest.mark.gpu
def test_partials_at_world_size_one(gpu, monkeypatch):
    """The N-rank form at world size 1 (``as_partitioned_world_of_one``): for first / last the ring hands
    ``merge_partials`` the state "v" of ``distagg._partials``, with V as its validity, and the merged result equals
    the oracle."""
    calls, prepare = as_partitioned_world_of_one(monkeypatch)
    store = new_store(5)
    stream = small_stream(12, whole=False)
    run_stream(stream, [Q_FIRST_LAST], gpu, store, BITS, prepare=prepare)
    on_the_ring(store)
    assert calls["n"] >= len(stream) - 4          # (the watermark keeps the first windows empty)
