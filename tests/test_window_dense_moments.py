"""STDDEV / VARIANCE, count_if and bool_and / bool_or over sliding windows from the dense ring (window_dense.py
``plan_layout`` / ``DenseWindow.accumulate``, window_ring.hip win_m2_kernel / win_combine_kernel's M2 branch /
win_emit_kernel's variance kinds).  The oracle is the CPU evaluator over the materialised window (no GPU code in it).

Keys, counts and booleans compare exactly; doubles compare with NaN equal to NaN and ``rel=1e-9, abs=1e-12``:
``temp`` values are multiples of 0.25 in [0, 64) and a group holds at most about 2^11 rows in any window, every
operation rounds at 2^-53 and the longest dependent chain is about 2^11 adds, so the relative error of M2 stays below
about 3e-13 on either side — the tolerance is three orders above that bound and six below any wrong merge.  The offset
case (``temp + 1e9``) uses ``rel=1e-6``: a 1e-7 absolute error of a mean enters M2 only through n (Δ + e)² terms.
Every test prints the largest deviation it saw (``-s``)."""
import math

import pytest
import torch

from tests.window_dense_support import (S, Comparison, aggs_of, as_partitioned_world_of_one, assumed_types, batch,
                                        churn_stream, dense_states, new_store, only_state, run_stream, set_caps,
                                        stable_stream, two_rows_per_id_stream)

REL, ABS = 1e-9, 1e-12
NEAR = Comparison("tolerant", rel=REL, abs_=ABS)
Q_ALL = ("SELECT deviceId, COUNT(*) AS c, AVG(temp) AS av, STDDEV(temp) AS sd, VAR_POP(temp) AS vp, "
         "STDDEV_POP(temp) AS sp, VAR_SAMP(temp * 2 + deviceId) AS vs, count_if(temp > 32) AS ci, "
         "bool_and(temp > 1) AS ba, bool_or(kind = 'a') AS bo FROM W WHERE kind != 'c' GROUP BY deviceId")
Q_EDGE = ("SELECT deviceId, COUNT(*) AS c, COUNT(temp) AS n, STDDEV(temp) AS sd, VAR_SAMP(temp) AS vs, "
          "VAR_POP(temp) AS vp, STDDEV_POP(temp) AS sp, VARIANCE(temp) AS va, STD(temp) AS st, "
          "STDDEV_SAMP(temp) AS ss FROM W GROUP BY deviceId")
Q_OFFSET = ("SELECT deviceId, STDDEV(temp + 1000000000.0) AS sd, VAR_POP(temp + 1000000000.0) AS vp, "
            "AVG(temp + 1000000000.0) AS av FROM W GROUP BY deviceId")
Q_SD = "SELECT deviceId, COUNT(*) AS c, AVG(temp) AS av, STDDEV(temp) AS sd, VAR_POP(temp) AS vp FROM W GROUP BY deviceId"
Q_MOD = "SELECT deviceId % 3 AS m, COUNT(*) AS c, STDDEV(temp) AS sd, VAR_POP(temp) AS vp FROM W GROUP BY deviceId % 3"
Q_DGRP = ("SELECT deviceId, COUNT(DISTINCT kind) AS dk, STDDEV(temp) AS sd, AVG(temp) AS av, every(temp > 1) AS ev "
          "FROM W GROUP BY deviceId")
Q_DGLOB = ("SELECT COUNT(DISTINCT deviceId) AS dd, STDDEV(temp) AS sd, VAR_POP(temp) AS vp, count_if(temp > 32) AS ci "
           "FROM W WHERE temp > 8")
Q_DNONE = ("SELECT COUNT(DISTINCT deviceId) AS dd, STDDEV(temp) AS sd, VAR_POP(temp) AS vp, count_if(temp > 32) AS ci "
           "FROM W WHERE temp > 1000")                                                      # never a row
Q_INT = ("SELECT deviceId, COUNT(*) AS c, SUM(temp) AS s, MIN(temp) AS mn, MAX(temp) AS mx, AVG(temp) AS av "
         "FROM W GROUP BY deviceId")
Q_PART = ("SELECT deviceId, STDDEV(temp) AS sd, VAR_POP(temp) AS vp, count_if(temp > 32) AS ci, "
          "bool_or(kind = 'a') AS bo FROM W GROUP BY deviceId")


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_requests_and_layout_of_the_new_aggregates():
    """``_requests`` accepts the variance family, count_if and the boolean aggregates; AVG and STDDEV of one argument
    share its count and sum words; the M2 words sit in the layout's one op-3 line, described to the combine by the
    words of their argument; ``fin`` / ``pfin`` name the words ``distagg._partials``' suffixes need."""
    from dxa.engine.window_dense import MAX_VARIANCE, Ineligible, _requests, plan_layout
    from dxa.ops.groupby import (_F_COUNT, _F_F64, _F_I64, _F_NOT, _F_SQRT, _F_VAR_POP, _F_VAR_SAMP, _MA_ADD_F64,
                                 _MA_ADD_U64, _MA_M2, _MA_MAX)
    aggs = aggs_of("COUNT(*)", "AVG(temp)", "STDDEV(temp)", "VAR_POP(temp)", "variance(humidity)",
                   "count_if(temp > 3)", "bool_and(ok)", "some(ok)", "MIN(ok)")
    reqs = _requests(aggs)
    assert [f for _, f, _ in reqs] == ["count_star", "avg", "stddev", "var_pop", "variance", "count_if", "bmin", "bmax",
                                       "min"]
    types = assumed_types(reqs)
    for _, f, arg in reqs:
        if f in ("bmin", "bmax", "min", "count_if"):
            types[arg.key()] = ("boolean", False)
    L = plan_layout(reqs, types)
    by_func = {f: L["fin"][j] for j, (_, f, _) in enumerate(reqs)}
    pby = {f: L["pfin"][ak] for ak, f, _ in reqs}
    keys = [s[0][0] for s in L["slots"]]
    # one count, one sum and one M2 slot for temp, shared by AVG, STDDEV and VAR_POP
    temp = reqs[1][2].key()
    assert [s[0] for s in L["slots"] if s[0][1] == temp] == [("count", temp), ("sumf", temp), ("m2", temp)]
    assert keys.count("m2") == 2 and keys.count("sumf") == 2
    # the op-3 line: last, holding exactly the M2 words; no other line has that op
    assert L["line_ops"] == [_MA_ADD_U64, _MA_ADD_F64, _MA_MAX, _MA_M2] and L["stride"] == 32
    m2_words = [w for w, i in enumerate(L["order"]) if i is not None and L["slots"][i][0][0] == "m2"]
    assert m2_words == [24, 25]
    _, sum_w, cnt_w = by_func["avg"]
    assert by_func["stddev"] == (_F_VAR_SAMP | _F_SQRT, 24, cnt_w)
    assert by_func["var_pop"] == (_F_VAR_POP, 24, cnt_w)
    assert by_func["variance"][0] == _F_VAR_SAMP and by_func["variance"][1] == 25
    assert L["m2desc"][24] == cnt_w | sum_w << 16 and 8 <= cnt_w < 16 and 8 <= sum_w < 16
    assert [w for w, d in enumerate(L["m2desc"]) if d] == [24, 25]
    assert L["m2args"][0] == (temp, cnt_w, sum_w, 24)
    # agg_multi never accumulates into an M2 word
    assert all(s[1] == -1 for s in L["slots"] if s[0][0] == "m2")
    # partial states, as distagg._partials names them
    assert pby["stddev"] == {"s": (_F_F64, sum_w, cnt_w), "m2": (_F_F64, 24, cnt_w), "cnt": (_F_COUNT, cnt_w, -1)}
    assert by_func["count_if"][0] == _F_I64 and by_func["count_if"][2] == -1 and by_func["count_if"][1] < 8
    assert pby["count_if"] == {"cnt": by_func["count_if"]}
    assert by_func["bmin"][0] == _F_I64 | _F_NOT and by_func["bmax"][0] == _F_I64
    assert set(pby["bmin"]) == {"v"} and set(pby["bmax"]) == {"v"} and set(pby["min"]) == {"v", "cnt"}
    assert by_func["bmin"][1] == by_func["min"][1]          # bool_and(ok) and MIN(ok) share the slot
    plan = {f: p for (_, f, _), p in zip(reqs, L["plan"])}
    assert plan["bmin"][4] == "boolean" and plan["stddev"][4] == "double" and plan["count_if"][4] == "long"
    # a layout without the variance family has no op-3 line and no descriptor
    plain = _requests(aggs_of("COUNT(*)", "AVG(temp)", "MAX(temp)"))
    Lp = plan_layout(plain, assumed_types(plain))
    assert _MA_M2 not in Lp["line_ops"] and not Lp["m2args"] and not any(Lp["m2desc"])
    # variance of a non-numeric argument, DISTINCT forms, too many variance arguments
    with pytest.raises(Ineligible):
        of_bool = _requests(aggs_of("STDDEV(ok)"))
        plan_layout(of_bool, assumed_types(of_bool, ("boolean", False)))
    for bad in ("STDDEV(DISTINCT temp)", "count_if(DISTINCT ok)", "first(temp)", "last(temp)"):
        with pytest.raises(Ineligible):
            _requests(aggs_of(bad))
    assert MAX_VARIANCE == 8
    _requests(aggs_of(*[f"STDDEV(x{i})" for i in range(8)], "VAR_POP(x0)"))
    with pytest.raises(Ineligible, match="too many variance arguments"):
        _requests(aggs_of(*[f"STDDEV(x{i})" for i in range(9)]))


def test_cpu_device_takes_the_generic_path():
    """On a CPU device the statements run (the oracle's own path) and no dense state is created; the oracle's row for
    a window in which nothing passes the WHERE has counts 0 (count_if among them) and NULL variances."""
    store = new_store(6)

    def each(b, q, rows, view, table):
        if q == Q_DNONE:
            assert rows == [{"dd": 0, "sd": None, "vp": None, "ci": 0}]

    run_stream(churn_stream(batch, 8), [Q_ALL, Q_DGLOB, Q_DNONE, Q_MOD], torch.device("cpu"), store, NEAR, each)
    assert not dense_states(store)


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spread", [S - 1, 3 * S])
@pytest.mark.parametrize("block", [16, 2])
def test_every_new_aggregate(gpu, monkeypatch, block, spread):
    """All the new aggregates in one grouped statement with a WHERE, NULL arguments, blocks of 2 panes or none, and
    (spread 3 S) panes clipped by the window's edge in scratch slots."""
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
    assert 3 in d.layout["line_ops"]
    assert (seen["blocks"] > 0) == (block < 8)


def _edge_stream(nb):
    """Per batch: 120 rows over 20 stable ids, one row (valid temp) of an id seen in that batch alone, and 5 rows of
    ids whose temp is always NULL."""
    import numpy as np
    rng = np.random.default_rng(31)
    out = []
    for b in range(nb):
        ids = np.concatenate([rng.integers(0, 20, 120), [5000 + b], np.arange(9000, 9005)])
        valid = np.concatenate([rng.random(120) > 0.1, [True], [False] * 5])
        out.append(((100 + b) * S, batch(rng, (100 + b) * S, ids, temp_valid=valid.tolist()), ids))
    return out


@pytest.mark.gpu
def test_one_row_and_all_null_groups(gpu):
    store = new_store(6)
    counts = {"one": 0, "null": 0}

    def each(b, q, rows, view, table):
        for r in rows:
            if r["deviceId"] >= 9000:
                assert r["c"] > 0 and r["n"] == 0
                assert all(r[k] is None for k in ("sd", "vs", "vp", "sp", "va", "st", "ss")), r
                counts["null"] += 1
            elif r["deviceId"] >= 5000:
                assert r["c"] == 1 and r["n"] == 1
                assert all(math.isnan(r[k]) for k in ("sd", "vs", "va", "st", "ss")), r
                assert r["vp"] == 0.0 and r["sp"] == 0.0
                counts["one"] += 1

    run_stream(_edge_stream(14), [Q_EDGE], gpu, store, NEAR, each)
    assert not only_state(store).disabled
    assert counts["one"] > 14 and counts["null"] > 14


@pytest.mark.gpu
def test_offset_values(gpu, monkeypatch):
    """Values near 1e9 with a spread of 64: the centred two-pass form keeps STDDEV to rel 1e-6 (Σx² − (Σx)²/n would be
    off by orders of magnitude)."""
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "BLOCK", 2)
    store = new_store(6)
    run_stream(stable_stream(batch, 14, False), [Q_OFFSET], gpu, store, Comparison("tolerant", rel=1e-6, abs_=ABS))
    assert not only_state(store).disabled


@pytest.mark.gpu
def test_rebuild_moves_m2_lines(gpu, monkeypatch):
    """Ids drift through a 16-id dictionary that grows to 64 at most: every rebuild renumbers the op-3 line with the
    others, and the 2-pane blocks are combined again afterwards."""
    set_caps(monkeypatch, 16, 64, 1 << 16, 1 << 20, block=2)
    store = new_store(6)
    run_stream(churn_stream(batch, 40), [Q_SD], gpu, store, NEAR)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert d.rebuilds > 0 and d.gcap <= 64


@pytest.mark.gpu
def test_straddles_the_lds_bound(gpu, monkeypatch):
    """Group ids on both sides of win_m2_kernel's LDS bound in one pane (two rows per id, several workgroups), and a
    second statement whose three groups are all privatised."""
    from dxa.engine import window_dense
    from dxa.ops import native as N
    L = N.lib().dxa_win_m2_lds_groups()
    assert L > 0
    if L + 200 > window_dense.DENSE_GROUPS:
        monkeypatch.setattr(window_dense, "DENSE_GROUPS", 2 * (L + 200))
    store = new_store(6)
    run_stream(two_rows_per_id_stream(batch, 9, L + 200), [Q_SD, Q_MOD], gpu, store, NEAR)
    states = list(dense_states(store).values())
    assert len(states) == 2 and not any(d.disabled for d in states)


@pytest.mark.gpu
def test_mixed_with_count_distinct(gpu):
    """Variance beside COUNT(DISTINCT x): grouped, global, and the global form's empty-window row (counts 0,
    variance NULL)."""
    store = new_store(6)

    def each(b, q, rows, view, table):
        if q == Q_DNONE:
            assert rows == [{"dd": 0, "sd": None, "vp": None, "ci": 0}]

    run_stream(churn_stream(batch, 12), [Q_DGRP, Q_DGLOB, Q_DNONE], gpu, store, NEAR, each)
    states = list(dense_states(store).values())
    assert len(states) == 3 and not any(d.disabled for d in states)
    assert all(len(d.pairs) == 1 and 3 in d.layout["line_ops"] for d in states)


@pytest.mark.gpu
def test_plain_statement_has_no_m2_line(gpu):
    store = new_store(6)
    run_stream(churn_stream(batch, 12), [Q_INT], gpu, store, NEAR)
    d = only_state(store)
    assert not d.disabled and 3 not in d.layout["line_ops"] and d.m2desc_dev is None


@pytest.mark.gpu
def test_partials(gpu, monkeypatch):
    """The N-rank form at world size 1: the view is marked partitioned and ``dxa.parallel.active`` patched, so
    ``_paned_aggregate`` takes ``dense_partials`` → ``exchange_partials`` → ``merge_partials``.  The key exchange
    needs a process group, so it is replaced by what it is at world size 1: the identity."""
    calls, prepare = as_partitioned_world_of_one(monkeypatch)
    store = new_store(6)
    stream = churn_stream(batch, 12)
    run_stream(stream, [Q_PART], gpu, store, NEAR, prepare=prepare)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert calls["n"] >= len(stream) - 4          # (the watermark keeps the first windows empty)
