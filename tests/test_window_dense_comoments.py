"""CORR, COVAR_POP / COVAR_SAMP, SKEWNESS and KURTOSIS over sliding windows: from the dense ring (window_dense.py
``plan_layout`` / ``DenseWindow.accumulate``, window_ring.hip win_mom_kernel / win_combine_kernel's op-4 branch /
win_emit_kernel's new kinds) and from mergeable partial states (distagg.py).  The oracle is the CPU evaluator over the
materialised window (``query._moments``: two passes over all rows, no GPU code and no merge in it).

Keys, counts and NULL / NaN patterns compare exactly.  Covariances (and the variance family beside them) compare with
``rel=1e-9, abs=1e-12``; the dimensionless results (corr, skewness, kurtosis) with ``abs=1e-9`` and no relative test —
a near-zero skewness has no meaningful relative error.  Basis: merging random splits of ≤ 2048 rows per group with
the multi-way shift formulas deviates from a direct two-pass by at most 2e-15 absolute (dimensionless) and 5e-16
relative (covariances) for exactly summable values below 64, so the tolerances sit six orders above the arithmetic
and orders below a dropped term (``temp`` is skewed on purpose: M3 is far from 0).  The offset case (values + 1e9)
deviated by at most 2e-9 absolute and 3e-10 relative and uses ``rel=1e-6`` / ``abs=1e-6``.  Every stream prints the
largest deviations it saw (``-s``); the recorded ones are in profiles/window_comoments/README.md."""
import math

import pytest
import torch

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from dxa.engine.expr import EvalContext
from tests.window_dense_support import (S, Comparison, aggs_of, answer, as_partitioned_world_of_one, assumed_types,
                                        churn_stream, dense_states, layout_of, new_store, only_state, rows_of,
                                        run_stream, set_caps, small_stream, stable_stream, steady_state_launches,
                                        two_rows_per_id_stream)

REL, ABS = 1e-9, 1e-12
DIMLESS_ABS = 1e-9
DIMLESS = ("cr", "sk", "ku", "kh")           # result columns of corr / skewness / kurtosis, by name
Q_ALL = ("SELECT deviceId, COUNT(*) AS c, AVG(temp) AS av, STDDEV(temp) AS sd, VAR_POP(hum) AS vp, "
         "COUNT(DISTINCT kind) AS dk, corr(temp, hum) AS cr, covar_pop(temp, hum) AS cp, covar_samp(temp, hum) AS cs, "
         "skewness(temp) AS sk, kurtosis(temp) AS ku, kurtosis(hum * 2 + deviceId) AS kh "
         "FROM W WHERE kind != 'c' GROUP BY deviceId")
Q_EDGE = ("SELECT deviceId, COUNT(*) AS c, COUNT(temp) AS n, covar_pop(temp, hum) AS cp, covar_samp(temp, hum) AS cs, "
          "corr(temp, hum) AS cr, skewness(temp) AS sk, kurtosis(temp) AS ku FROM W GROUP BY deviceId")
Q_OFFSET = ("SELECT deviceId, corr(temp + 1000000000.0, hum + 1000000000.0) AS cr, "
            "covar_pop(temp + 1000000000.0, hum + 1000000000.0) AS cp, "
            "covar_samp(temp + 1000000000.0, hum + 1000000000.0) AS cs, skewness(temp + 1000000000.0) AS sk, "
            "kurtosis(hum + 1000000000.0) AS ku FROM W GROUP BY deviceId")
Q_FIVE = ("SELECT deviceId, COUNT(*) AS c, corr(temp, hum) AS cr, covar_pop(temp, hum) AS cp, "
          "covar_samp(hum, temp) AS cs, skewness(temp) AS sk, kurtosis(temp) AS ku FROM W GROUP BY deviceId")
Q_MOD = ("SELECT deviceId % 3 AS m, COUNT(*) AS c, corr(temp, hum) AS cr, skewness(temp) AS sk, kurtosis(hum) AS ku "
         "FROM W GROUP BY deviceId % 3")
Q_DGLOB = ("SELECT COUNT(DISTINCT deviceId) AS dd, corr(temp, hum) AS cr, covar_samp(temp, hum) AS cs, "
           "skewness(temp) AS sk, count_if(temp > 32) AS ci FROM W WHERE temp > 8")
Q_DNONE = ("SELECT COUNT(DISTINCT deviceId) AS dd, corr(temp, hum) AS cr, covar_samp(temp, hum) AS cs, "
           "skewness(temp) AS sk, count_if(temp > 32) AS ci FROM W WHERE temp > 1000")                  # never a row
Q_INT = ("SELECT deviceId, COUNT(*) AS c, SUM(temp) AS s, MIN(temp) AS mn, MAX(temp) AS mx, AVG(temp) AS av "
         "FROM W GROUP BY deviceId")
Q_SD = ("SELECT deviceId, COUNT(*) AS c, AVG(temp) AS av, STDDEV(temp) AS sd, VAR_POP(temp) AS vp FROM W "
        "GROUP BY deviceId")
NEAR = Comparison("tolerant", rel=REL, abs_=ABS, dimless=DIMLESS, dimless_abs=DIMLESS_ABS)


def batch(rng, t_us, ids, spread=S - 1, temp=None, temp_valid=None, hum_valid=None):
    """A batch with given device ids; event times within ``spread`` before the batch time.  ``temp`` is the square of
    a uniform multiple of 0.25 below 8 (a multiple of 1/16 below 64: exactly summable and visibly skewed), ``hum`` a
    multiple of 0.25 below 64 that depends on ``temp``; each has NULLs of its own."""
    import numpy as np
    n = len(ids)
    ts = torch.tensor([t_us - int(rng.integers(0, spread)) for _ in range(n)], dtype=torch.int64)
    tv = (rng.integers(0, 32, n) * 0.25) ** 2
    if temp is not None:
        tv = np.asarray(temp, dtype=np.float64)
    hv = np.floor(tv * 2) * 0.25 + rng.integers(0, 128, n) * 0.25
    tvalid = rng.random(n) > 0.1
    hvalid = rng.random(n) > 0.15
    if temp_valid is not None:
        tvalid = np.asarray(temp_valid)
    if hum_valid is not None:
        hvalid = np.asarray(hum_valid)
    kinds = strings_from_pylist([["a", "b", "c"][int(i) % 3] for i in rng.integers(0, 3, n)], "cpu")
    return Table(["ts", "deviceId", "kind", "temp", "hum"],
                 [PrimColumn("timestamp", ts), PrimColumn("long", torch.tensor(ids, dtype=torch.int64)), kinds,
                  PrimColumn("double", torch.tensor(tv, dtype=torch.float64), torch.tensor(tvalid)),
                  PrimColumn("double", torch.tensor(hv, dtype=torch.float64), torch.tensor(hvalid))], n, "cpu")


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_layout_of_the_comoment_aggregates():
    """``_requests`` accepts the five names; skewness, STDDEV and AVG of one argument share its count, sum and M2
    words; corr / covar_pop / covar_samp of one (x, y) share the pair's words; the new words sit in the one op-4
    line, unused by agg_multi and described to the combine by the words they read; ``pfin`` carries the partial
    states of ``distagg._partials``."""
    from dxa.engine.window_dense import MAX_VARIANCE, Ineligible, _requests, pair_keys, plan_layout
    from dxa.ops.groupby import (_F_CORR, _F_COUNT, _F_COVAR_POP, _F_COVAR_SAMP, _F_F64, _F_KURT, _F_SKEW, _F_SQRT,
                                 _F_VAR_SAMP, _MA_ADD_F64, _MA_M2, _MA_MOM, _MOM_CXY, _MOM_M3, _MOM_M4)
    aggs = aggs_of("COUNT(*)", "AVG(temp)", "STDDEV(temp)", "skewness(temp)", "kurtosis(temp)", "corr(temp, hum)",
                 "covar_pop(temp, hum)", "covar_samp(temp, hum)", "skewness(hum)")
    reqs = _requests(aggs)
    assert [f for _, f, _ in reqs] == ["count_star", "avg", "stddev", "skewness", "kurtosis", "corr", "covar_pop",
                                       "covar_samp", "skewness"]
    L = plan_layout(reqs, assumed_types(reqs))
    by_func = {}
    for j, (_, f, _a) in enumerate(reqs):
        by_func.setdefault(f, L["fin"][j])
    pby = {}
    for ak, f, _a in reqs:
        pby.setdefault(f, L["pfin"][ak])
    temp = reqs[1][2].key()
    px, py = pair_keys(*reqs[5][2])
    slot_keys = [s[0] for s in L["slots"]]
    # one count, sum, M2, M3 and M4 slot for temp, shared by AVG, STDDEV, skewness and kurtosis
    assert [k for k in slot_keys if k[1] == temp] == [("count", temp), ("sumf", temp), ("m2", temp), ("m3", temp),
                                                      ("m4", temp)]
    # one pair: count, two sums, Cxy and (for corr) two M2s, shared by the three two-argument aggregates
    assert [k for k in slot_keys if k[0] == "cxy"] == [("cxy", (px, py))]
    assert [k for k in slot_keys if k[1] in (px, py)] == [("count", px), ("sumf", px), ("sumf", py), ("m2", px),
                                                          ("m2", py)]
    assert L["line_ops"] == [_MA_ADD_F64, _MA_M2, _MA_MOM] and L["stride"] == 24
    where = {i: w for w, i in enumerate(L["order"]) if i is not None}
    word = {k: where[i] for i, k in enumerate(slot_keys)}
    new_words = sorted(w for k, w in word.items() if k[0] in ("m3", "m4", "cxy"))
    assert new_words == [16, 17, 18, 19]                                # temp's M3, M4, the pair's Cxy, hum's M3
    assert [w for w, d in enumerate(L["momdesc"]) if d] == new_words
    # agg_multi never accumulates into a new word
    assert all(s[1] == -1 for s in L["slots"] if s[0][0] in ("m3", "m4", "cxy"))
    c, sm, m2 = word[("count", temp)], word[("sumf", temp)], word[("m2", temp)]
    m3, m4 = word[("m3", temp)], word[("m4", temp)]
    assert L["momdesc"][m3] == _MOM_M3 << 24 | c | sm << 6 | m2 << 12
    assert L["momdesc"][m4] == _MOM_M4 << 24 | c | sm << 6 | m2 << 12 | m3 << 18
    pc, psx, psy, cxy = word[("count", px)], word[("sumf", px)], word[("sumf", py)], word[("cxy", (px, py))]
    assert L["momdesc"][cxy] == _MOM_CXY << 24 | pc | psx << 6 | psy << 12
    assert L["m2desc"][m2] == c | sm << 16 and L["m2desc"][word[("m2", py)]] == pc | psy << 16
    assert (temp, None, c, sm, -1, m3, m4) in L["momargs"] and (px, py, pc, psx, psy, cxy, -1) in L["momargs"]
    assert len(L["momargs"]) == 3
    # finishing kinds: existing ones stay 3-tuples, the new ones carry their operands
    assert by_func["stddev"] == (_F_VAR_SAMP | _F_SQRT, m2, c)
    assert by_func["skewness"] == (_F_SKEW, m3, c, m2, -1) and by_func["kurtosis"] == (_F_KURT, m4, c, m2, -1)
    assert by_func["corr"] == (_F_CORR, cxy, pc, word[("m2", px)], word[("m2", py)])
    assert by_func["covar_pop"] == (_F_COVAR_POP, cxy, pc, -1, -1)
    assert by_func["covar_samp"] == (_F_COVAR_SAMP, cxy, pc, -1, -1)
    # partial states, as distagg._partials names them
    assert pby["skewness"] == {"s": (_F_F64, sm, c), "m2": (_F_F64, m2, c), "m3": (_F_F64, m3, c),
                               "cnt": (_F_COUNT, c, -1)}
    assert pby["kurtosis"] == dict(pby["skewness"], m4=(_F_F64, m4, c))
    assert pby["covar_pop"] == {"sx": (_F_F64, psx, pc), "sy": (_F_F64, psy, pc), "cxy": (_F_F64, cxy, pc),
                                "cnt": (_F_COUNT, pc, -1)}
    assert pby["covar_samp"] == pby["covar_pop"]
    assert pby["corr"] == dict(pby["covar_pop"], m2x=(_F_F64, word[("m2", px)], pc),
                               m2y=(_F_F64, word[("m2", py)], pc))
    # a statement without a new aggregate keeps today's layout, word for word
    old = _requests(aggs_of("COUNT(*)", "AVG(temp)", "STDDEV(temp)"))
    Lo = plan_layout(old, assumed_types(old))
    assert Lo["line_ops"] == [_MA_ADD_F64, _MA_M2] and Lo["stride"] == 16
    assert Lo["fin"] == [(0, 0, -1), (3, 2, 1), (_F_VAR_SAMP | _F_SQRT, 8, 1)]
    assert Lo["m2desc"] == [0] * 8 + [1 | 2 << 16] + [0] * 7
    assert "momdesc" not in Lo and "momargs" not in Lo
    # DISTINCT forms, a boolean argument, a wrong argument count
    for bad in ("corr(DISTINCT temp, hum)", "skewness(DISTINCT temp)", "kurtosis(DISTINCT temp)",
                "covar_pop(DISTINCT temp, hum)", "covar_samp(DISTINCT temp, hum)", "corr(temp)", "skewness(temp, hum)"):
        with pytest.raises(Ineligible):
            _requests(aggs_of(bad))
    for bad in ("skewness(ok)", "kurtosis(ok)", "corr(ok, temp)", "covar_pop(temp, ok)", "covar_samp(ok, ok)"):
        r = _requests(aggs_of(bad))
        with pytest.raises(Ineligible):
            plan_layout(r, assumed_types(r, ("boolean", False)))
    # the new cap has a reason of its own; the variance cap keeps its own
    _requests(aggs_of(*[f"covar_pop(x{i}, y)" for i in range(8)]))
    with pytest.raises(Ineligible, match="too many moment arguments"):
        _requests(aggs_of(*[f"covar_pop(x{i}, y)" for i in range(9)]))
    with pytest.raises(Ineligible, match="too many moment arguments"):
        _requests(aggs_of(*[f"skewness(x{i})" for i in range(9)]))
    assert MAX_VARIANCE == 8
    with pytest.raises(Ineligible, match="too many variance arguments"):
        _requests(aggs_of(*[f"STDDEV(x{i})" for i in range(9)]))


def _call_text(name):
    """A call of the supported aggregate ``name`` over the columns of ``batch``."""
    from dxa.engine.window_dense import _BOOL, _PAIRED
    arg = "temp, hum" if name in _PAIRED else "temp > 8" if name in _BOOL or name == "count_if" else "temp"
    return f"{name}({arg})"


def test_partial_states_are_those_of_local_partials():
    """For every supported aggregate ``plan_layout``'s ``pfin`` holds exactly the suffixes that
    ``distagg.local_partials`` plans for the call (over an empty CPU table, as ``dense_partials`` builds its
    prototype), so ``_partial_spec`` finds a word for every partial column and carries no other.  COUNT(DISTINCT x)
    is not decomposable and has no entry in ``pfin`` at all."""
    from dxa.engine import distagg as D
    from dxa.engine.column import materialize
    from dxa.engine.expr import Scope, evaluate
    from dxa.engine.window_dense import _SUPPORTED
    from dxa.sql.parser import parse_select_item
    import numpy as np
    empty = batch(np.random.default_rng(0), 100 * S, np.arange(4)).take(torch.empty(0, dtype=torch.int64))
    ctx = EvalContext(now_us=0)
    scope = Scope.of_table(empty, "W")
    gx = [parse_select_item("deviceId").expr]
    keys = [materialize(evaluate(g, scope, ctx)) for g in gx]

    def layout(aggs):
        return layout_of(aggs, empty)[2]

    for text in ["COUNT(*)"] + [_call_text(name) for name in sorted(_SUPPORTED)]:
        aggs = aggs_of(text)
        (ak,) = aggs
        assert D.decomposable(aggs, ctx), text
        _partial, plan, _key_names = D.local_partials(gx, keys, aggs, scope, ctx)
        suffixes = [sfx for _nm, sfx, _op in plan[ak]]
        assert len(set(suffixes)) == len(suffixes) > 0, text
        assert set(layout(aggs)["pfin"][ak]) == set(suffixes), (text, suffixes)
    for text in ("COUNT(DISTINCT temp)", "COUNT(DISTINCT kind)"):
        aggs = aggs_of("AVG(temp)", text)
        avg, dc = aggs
        assert not D.decomposable(aggs, ctx) and aggs[dc].distinct
        L = layout(aggs)
        assert set(L["pfin"]) == {avg} and L["dcount_word"], text


Q_WHOLE = ("SELECT deviceId, COUNT(*) AS c, corr(temp, hum) AS cr, covar_pop(temp, hum) AS cp, "
           "covar_samp(temp, hum) AS cs, skewness(temp) AS sk, kurtosis(hum) AS ku, STDDEV(temp) AS sd "
           "FROM W GROUP BY deviceId")
_WHOLE_ITEMS = ["COUNT(*)", "corr(temp, hum)", "covar_pop(temp, hum)", "covar_samp(temp, hum)", "skewness(temp)",
                "kurtosis(hum)", "STDDEV(temp)"]
_WHOLE_NAMES = ["c", "cr", "cp", "cs", "sk", "ku", "sd"]


def _whole_table():
    """400 rows over 12 ids, plus id 77 with exactly three rows (rows 0, 1 and 2)."""
    import numpy as np
    rng = np.random.default_rng(41)
    ids = rng.integers(0, 12, 403)
    ids[:3] = 77
    return batch(rng, 100 * S, ids)


@pytest.mark.parametrize("nsub", [1, 2, 7])
def test_partials_merge_to_the_whole(nsub):
    """``local_partials`` of every row subset, concatenated, half of the parts pre-combined by ``combine_partials``,
    then ``merge_partials`` — equal to the statement over the whole table.  One subset is empty and (from 2 subsets
    on) one holds a single row of id 77."""
    from dxa.engine import distagg as D
    from dxa.engine.column import concat_tables, materialize
    from dxa.engine.expr import Scope, evaluate
    from dxa.sql.parser import parse_select_item
    whole = _whole_table()
    ctx = EvalContext(now_us=0)
    aggs = aggs_of(*_WHOLE_ITEMS)
    assert D.decomposable(aggs, ctx)
    assert all(D.decomposable(aggs_of(one), ctx) for one in ("corr(a, b)", "covar_pop(a, b)", "covar_samp(a, b)",
                                                           "skewness(a)", "kurtosis(a)"))
    gx = [parse_select_item("deviceId").expr]
    # subsets by row index: [0], the rest dealt round-robin (rows 1 and 2 of id 77 land elsewhere), and an empty one
    n = whole.length
    if nsub == 1:
        subsets = [list(range(n)), []]
    else:
        subsets = [[0]] + [list(range(1 + k, n, nsub - 1)) for k in range(nsub - 1)] + [[]]
    parts, meta = [], None
    for rows in subsets:
        sub = whole.take(torch.tensor(rows, dtype=torch.int64))
        scope = Scope.of_table(sub, "W")
        keys = [materialize(evaluate(g, scope, ctx)) for g in gx]
        partial, plan, key_names = D.local_partials(gx, keys, aggs, scope, ctx)
        parts.append(partial)
        meta = (plan, key_names)
    plan, key_names = meta
    assert [sfx for _nm, sfx, _op in plan[list(aggs)[1]]] == ["sx", "sy", "m2x", "m2y", "cxy", "cnt"]
    assert [sfx for _nm, sfx, _op in plan[list(aggs)[2]]] == ["sx", "sy", "cxy", "cnt"]
    assert [sfx for _nm, sfx, _op in plan[list(aggs)[4]]] == ["s", "m2", "m3", "cnt"]
    assert [sfx for _nm, sfx, _op in plan[list(aggs)[5]]] == ["s", "m2", "m3", "m4", "cnt"]
    half = (len(parts) + 1) // 2
    block = D.combine_partials(concat_tables(parts[:half]), plan, key_names, True)
    got = concat_tables([block] + parts[half:])
    out_keys, finals, ng = D.merge_partials(got, plan, key_names, aggs, True)
    cols = {"deviceId": out_keys[0].to_pylist()}
    for nm, ak in zip(_WHOLE_NAMES, aggs):
        cols[nm] = finals[ak].to_pylist()
    rows = sorted(({nm: v[i] for nm, v in cols.items()} for i in range(ng)), key=lambda r: r["deviceId"])
    NEAR.reset()
    NEAR((rows, None), rows_of(answer(Q_WHOLE, whole, ctx=ctx), order_by="deviceId"), nsub)
    NEAR.report()


def test_cpu_stream_takes_the_pane_partials():
    """On a CPU device the statements are answered from pane partials (no dense state is created) and equal the
    oracle; the window in which nothing passes the WHERE gives counts 0 and NULLs."""
    store = new_store(6)

    def each(b, q, rows, view, table):
        if q == Q_DNONE:
            assert rows == [{"dd": 0, "cr": None, "cs": None, "sk": None, "ci": 0}]

    run_stream(churn_stream(batch, 8), [Q_ALL, Q_FIVE, Q_DGLOB, Q_DNONE, Q_MOD], torch.device("cpu"), store, NEAR,
               each)
    assert not dense_states(store)


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spread", [S - 1, 3 * S])
@pytest.mark.parametrize("block", [16, 2])
def test_all_five_in_one_statement(gpu, monkeypatch, block, spread):
    """The five aggregates beside the variance family and COUNT(DISTINCT kind) in one grouped statement with a
    WHERE, NULLs in both columns, blocks of 2 panes or none, and (spread 3 S) panes clipped by the window's edge in
    scratch slots.  Before these aggregates were decomposable the statement had no dense state at all."""
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "BLOCK", block)
    store = new_store(8)
    seen = {"blocks": 0}

    def each(b, q, rows, view, table):
        for d in dense_states(store).values():
            if not d.disabled:
                seen["blocks"] = max(seen["blocks"], len(d.blocks))

    run_stream(stable_stream(batch, 24, True, spread=spread), [Q_ALL], gpu, store, NEAR, each)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert 4 in d.layout["line_ops"] and 3 in d.layout["line_ops"] and len(d.pairs) == 1
    assert (seen["blocks"] > 0) == (block < 8)


def _edge_stream(nb):
    """Per batch: 120 rows over 20 stable ids; one row (both valid) of an id seen in that batch alone; 5 rows of ids
    whose temp is always NULL; 6 rows of ids 8000-8002 in which temp and hum are never both non-null; 3 rows each of
    ids 7000 and 7001 whose temp is a constant (4.0 and 9.0)."""
    import numpy as np
    rng = np.random.default_rng(31)
    out = []
    for b in range(nb):
        ids = np.concatenate([rng.integers(0, 20, 120), [5000 + b], np.arange(9000, 9005),
                              np.repeat(np.arange(8000, 8003), 2), [7000] * 3, [7001] * 3])
        n = len(ids)
        tvalid = np.concatenate([rng.random(120) > 0.1, [True], [False] * 5, [True, False] * 3, [True] * 6])
        hvalid = np.concatenate([rng.random(120) > 0.15, [True], [True] * 5, [False, True] * 3, [True] * 6])
        temp = (rng.integers(0, 32, n) * 0.25) ** 2
        temp[-6:-3], temp[-3:] = 4.0, 9.0
        out.append(((100 + b) * S, batch(rng, (100 + b) * S, ids, temp=temp, temp_valid=tvalid, hum_valid=hvalid),
                    ids))
    return out


@pytest.mark.gpu
def test_edge_groups(gpu):
    store = new_store(6)
    nb = 14
    counts = {"one": 0, "null": 0, "apart": 0, "const": 0}

    def each(b, q, rows, view, table):
        for r in rows:
            i = r["deviceId"]
            if i >= 9000:
                assert r["c"] > 0 and r["n"] == 0
                assert all(r[k] is None for k in ("cp", "cs", "cr", "sk", "ku")), r
                counts["null"] += 1
            elif i >= 8000:
                assert r["n"] > 0 and all(r[k] is None for k in ("cp", "cs", "cr")), r
                assert r["sk"] is not None and r["ku"] is not None, r
                counts["apart"] += 1
            elif i >= 7000:
                assert r["n"] >= 3 and r["cp"] == 0.0 and r["cs"] == 0.0
                assert all(math.isnan(r[k]) for k in ("cr", "sk", "ku")), r
                counts["const"] += 1
            elif i >= 5000:
                assert r["c"] == 1 and r["n"] == 1 and r["cp"] == 0.0
                assert all(math.isnan(r[k]) for k in ("cs", "cr", "sk", "ku")), r
                counts["one"] += 1

    run_stream(_edge_stream(nb), [Q_EDGE], gpu, store, NEAR, each)
    assert not only_state(store).disabled
    assert all(v > nb for v in counts.values()), counts


@pytest.mark.gpu
def test_offset_values(gpu, monkeypatch):
    """Values near 1e9 with a spread of 64, blocks of two panes: every term stays centred, so the results hold to
    1e-6 (raw power sums would lose every digit)."""
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "BLOCK", 2)
    store = new_store(6)
    run_stream(stable_stream(batch, 14, False), [Q_OFFSET], gpu, store,
               Comparison("tolerant", rel=1e-6, abs_=ABS, dimless=DIMLESS, dimless_abs=1e-6))
    d = only_state(store)
    assert not d.disabled and 4 in d.layout["line_ops"]


@pytest.mark.gpu
def test_rebuild_moves_op4_lines(gpu, monkeypatch):
    """Ids drift through a 16-id dictionary that grows to 64 at most: every rebuild renumbers the op-4 line with the
    others, and the 2-pane blocks are combined again afterwards."""
    set_caps(monkeypatch, 16, 64, 1 << 16, 1 << 20, block=2)
    store = new_store(6)
    run_stream(churn_stream(batch, 40), [Q_FIVE], gpu, store, NEAR)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert d.rebuilds > 0 and d.gcap <= 64 and 4 in d.layout["line_ops"]


@pytest.mark.gpu
def test_straddles_the_lds_bound(gpu, monkeypatch):
    """Group ids on both sides of the second pass's LDS bound in one pane (two rows per id, several workgroups), and
    a second statement whose three groups are all privatised."""
    from dxa.engine import window_dense
    from dxa.ops import native as N
    L = N.lib().dxa_win_m2_lds_groups()
    assert L > 0
    if L + 200 > window_dense.DENSE_GROUPS:
        monkeypatch.setattr(window_dense, "DENSE_GROUPS", 2 * (L + 200))
    store = new_store(6)
    run_stream(two_rows_per_id_stream(batch, 9, L + 200), [Q_FIVE, Q_MOD], gpu, store, NEAR)
    states = list(dense_states(store).values())
    assert len(states) == 2 and not any(d.disabled for d in states)
    assert all(4 in d.layout["line_ops"] for d in states)


@pytest.mark.gpu
def test_global_form_with_count_distinct(gpu):
    """No GROUP BY: corr / covar_samp / skewness beside COUNT(DISTINCT deviceId), and the window in which nothing
    passes the WHERE (counts 0, the rest NULL)."""
    store = new_store(6)

    def each(b, q, rows, view, table):
        if q == Q_DNONE:
            assert rows == [{"dd": 0, "cr": None, "cs": None, "sk": None, "ci": 0}]

    run_stream(churn_stream(batch, 12), [Q_DGLOB, Q_DNONE], gpu, store, NEAR, each)
    states = list(dense_states(store).values())
    assert len(states) == 2 and not any(d.disabled for d in states)
    assert all(len(d.pairs) == 1 and 4 in d.layout["line_ops"] for d in states)


@pytest.mark.gpu
def test_partials_at_world_size_one(gpu, monkeypatch):
    """The N-rank form at world size 1 (``as_partitioned_world_of_one``): the ring hands
    ``merge_partials`` the states of ``distagg._partials``."""
    calls, prepare = as_partitioned_world_of_one(monkeypatch)
    store = new_store(6)
    stream = churn_stream(batch, 12)
    run_stream(stream, [Q_FIVE], gpu, store, NEAR, prepare=prepare)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert calls["n"] >= len(stream) - 4          # (the watermark keeps the first windows empty)


@pytest.mark.gpu
def test_plain_statements_have_no_op4_line(gpu):
    store = new_store(6)
    run_stream(churn_stream(batch, 12), [Q_INT, Q_SD], gpu, store, NEAR)
    states = list(dense_states(store).values())
    assert len(states) == 2 and not any(d.disabled for d in states)
    for d in states:
        assert 4 not in d.layout["line_ops"] and d.momdesc_dev is None and d.momdesc_t is None
        assert "momdesc" not in d.layout and "momargs" not in d.layout


# ---- one answer entry point: the dispatch arms and the launch sequences ---------------------------------------------
Q_CP = "SELECT deviceId, covar_pop(temp, hum) AS cp FROM W GROUP BY deviceId"
Q_CP_GLOB = "SELECT COUNT(DISTINCT deviceId) AS dd, covar_pop(temp, hum) AS cp FROM W"
Q_SK = "SELECT deviceId, skewness(temp) AS sk FROM W GROUP BY deviceId"
Q_DC = "SELECT deviceId, COUNT(*) AS c, COUNT(DISTINCT kind) AS dk FROM W GROUP BY deviceId"


@pytest.mark.gpu
@pytest.mark.parametrize("q", [Q_CP, Q_CP_GLOB])
def test_covar_pop_alone(gpu, monkeypatch, q):
    """An op-4 line and no M2 line: ``momdesc`` beside an all-zero ``m2desc``, through the per-batch combine and the
    2-pane block combine; grouped, and in global form beside COUNT(DISTINCT deviceId)."""
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "BLOCK", 2)
    store = new_store(6)
    seen = {"blocks": 0}

    def each(b, _q, rows, view, table):
        for d in dense_states(store).values():
            seen["blocks"] = max(seen["blocks"], len(d.blocks))

    run_stream(small_stream(batch, 14), [q], gpu, store, NEAR, each)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert d.momdesc_dev is not None and d.m2desc_dev is not None and not any(d.layout["m2desc"])
    assert 4 in d.layout["line_ops"] and 3 not in d.layout["line_ops"]
    assert len(d.pairs) == (q == Q_CP_GLOB) and seen["blocks"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("q,second_pass,pairs", [(Q_INT, [], 0), (Q_SD, ["dxa_win_m2"], 0),
                                                 (Q_SK, ["dxa_win_m2", "dxa_win_mom"], 0), (Q_DC, [], 1)])
def test_entry_points_per_steady_state_batch(gpu, monkeypatch, q, second_pass, pairs):
    """The native entry points of a batch in which one pane enters the window and nothing is rebuilt: the group
    insert, the multi-aggregate, the second passes the layout has, per pair state its insert, then — on a batch that
    completes a 2-pane block — one block combine and one presence OR per pair state, then the one answer.  A layout
    without a family issues none of its launches."""
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "BLOCK", 2)
    store = new_store(6)
    pane = ["dxa_win_insert_fused", "dxa_aggregate_multi", *second_pass,
            *["dxa_win_pair_prep", "dxa_win_insert_fused", "dxa_win_pair_mark"] * pairs]
    block = ["dxa_win_combine_block", *["dxa_win_pair_or_block"] * pairs]
    completed_seen = set()
    # the watermark and the 6-pane window: full from batch 7 on
    for b, native, completed in steady_state_launches(gpu, store, small_stream(batch, 14, mid_pane=True), q, NEAR, 8):
        d = only_state(store)
        assert not d.disabled and d.rebuilds == 0 and len(d.pairs) == pairs
        completed_seen.add(completed)
        assert native == pane + block * completed + ["dxa_win_answer"], (b, native)
    assert completed_seen == {0, 1}
