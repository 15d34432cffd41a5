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

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from dxa.engine.expr import EvalContext
from dxa.engine.query import Catalog, run_sql
from dxa.engine.windows import TimeWindowConf, WindowStore

S = 1_000_000
REL, ABS = 1e-9, 1e-12
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
STABLE = 200
SEEN = {"rel": 0.0, "abs": 0.0}


# ---- helpers (copies of tests/test_window_dense_distinct.py's; ``batch`` with the event-time spread as a parameter) --
def drifting_ids(rng, b, n):
    """Batch ``b``'s drifting ids: uniform in [4b, 4b + 12)."""
    return rng.integers(4 * b, 4 * b + 12, n)


def batch(rng, t_us, ids, spread=S - 1, temp_valid=None):
    """tests/test_windows.py::batch with given device ids and exactly summable temperatures; event times within
    ``spread`` before the batch time."""
    n = len(ids)
    ts = torch.tensor([t_us - int(rng.integers(0, spread)) for _ in range(n)], dtype=torch.int64)
    temp = torch.tensor(rng.integers(0, 256, n) * 0.25, dtype=torch.float64)
    valid = torch.tensor(rng.random(n) > 0.1)
    if temp_valid is not None:
        valid = torch.tensor(temp_valid)
    kinds = strings_from_pylist([["a", "b", "c"][int(i) % 3] for i in rng.integers(0, 3, n)], "cpu")
    return Table(["ts", "deviceId", "kind", "temp"],
                 [PrimColumn("timestamp", ts), PrimColumn("long", torch.tensor(ids, dtype=torch.int64)), kinds,
                  PrimColumn("double", temp, valid)], n, "cpu")


def churn_stream(nb, spread=S - 1):
    """200 rows per batch over the drifting ids → [(batch time, CPU table, ids)]."""
    import numpy as np
    rng = np.random.default_rng(23)
    out = []
    for b in range(nb):
        ids = drifting_ids(rng, b, 200)
        out.append(((100 + b) * S, batch(rng, (100 + b) * S, ids, spread), ids))
    return out


def stable_stream(nb, drift, spread=S - 1):
    """300 rows per batch: 200 over the stable ids and 100 over the drifting ids (or all 300 stable)."""
    import numpy as np
    rng = np.random.default_rng(29)
    out = []
    for b in range(nb):
        ids = rng.integers(1000, 1000 + STABLE, 300)
        if drift:
            ids[200:] = drifting_ids(rng, b, 100)
        out.append(((100 + b) * S, batch(rng, (100 + b) * S, ids, spread), ids))
    return out


def rows_of(t):
    """The table's rows as dicts of Python values (NULL as None), in a canonical order."""
    t = t.to("cpu")
    cols = {nm: t.column(nm).to_pylist() for nm in t.names}
    rows = [{nm: cols[nm][i] for nm in t.names} for i in range(t.length)]
    exact = [nm for nm in t.names if not any(isinstance(r[nm], float) for r in rows)]
    return sorted(rows, key=lambda r: tuple(repr(r[nm]) for nm in exact))


def oracle(q, view):
    """The CPU evaluator's rows for statement ``q`` over the materialised window ``view``."""
    mat = Table(view.names, view.columns, view.length, view._device)
    cat = Catalog()
    cat.register("W", mat.to("cpu"))
    return rows_of(run_sql(q, cat, EvalContext(now_us=0)))


def assert_rows(got, want, rel, abs_, what):
    """Keys, counts and booleans exactly; doubles with NaN equal to NaN and the given tolerances."""
    assert len(got) == len(want), (what, len(got), len(want))
    for g, w in zip(got, want):
        assert g.keys() == w.keys(), what
        for nm in w:
            a, b = g[nm], w[nm]
            if isinstance(a, float) and isinstance(b, float):
                if math.isnan(a) or math.isnan(b):
                    assert math.isnan(a) and math.isnan(b), (what, nm, g, w)
                    continue
                dev = abs(a - b)
                if dev > abs_:                      # (below the absolute tolerance a ratio says nothing)
                    SEEN["rel"] = max(SEEN["rel"], dev / abs(b) if b else math.inf)
                SEEN["abs"] = max(SEEN["abs"], dev)
                assert dev <= max(rel * abs(b), abs_), (what, nm, a, b, g, w)
            else:
                assert type(a) is type(b) and a == b, (what, nm, g, w)


def new_store(win=6):
    return WindowStore(TimeWindowConf({"W": win * S}, True, "ts", 2 * S, win * S, False))


def dense_states(store):
    return store.__dict__.get("_dense", {})


def set_caps(monkeypatch, groups, groups_max, pairs, pairs_max, block=None):
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "DENSE_GROUPS", groups)
    monkeypatch.setattr(window_dense, "DENSE_GROUPS_MAX", groups_max)
    monkeypatch.setattr(window_dense, "DENSE_PAIRS", pairs)
    monkeypatch.setattr(window_dense, "DENSE_PAIRS_MAX", pairs_max)
    if block is not None:
        monkeypatch.setattr(window_dense, "BLOCK", block)


def run_stream(stream, qs, dev, store, each=None, rel=REL, abs_=ABS, prepare=None):
    """Every statement over every batch's window equals the CPU oracle; ``each(b, q, rows)`` after each."""
    SEEN["rel"] = SEEN["abs"] = 0.0
    for b, (T, tbl, _ids) in enumerate(stream):
        views, _ = store.process(tbl.to(dev), T, S)
        if prepare is not None:
            prepare(views["W"])
        for q in qs:
            cat = Catalog()
            cat.register("W", views["W"])
            rows = rows_of(run_sql(q, cat, EvalContext(now_us=0, device=dev)))
            assert_rows(rows, oracle(q, views["W"]), rel, abs_, (b, q))
            if each is not None:
                each(b, q, rows)
    print(f"largest deviation from the oracle: relative {SEEN['rel']:.3e}, absolute {SEEN['abs']:.3e}")


def only_state(store):
    states = list(dense_states(store).values())
    assert len(states) == 1
    return states[0]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def _aggs(*select_items):
    from dxa.engine.query import _collect_aggs
    from dxa.sql.parser import parse_select_item
    aggs = {}
    for item in select_items:
        _collect_aggs(parse_select_item(item).expr, EvalContext(now_us=0), aggs)
    assert aggs
    return aggs


def test_requests_and_layout_of_the_new_aggregates():
    """``_requests`` accepts the variance family, count_if and the boolean aggregates; AVG and STDDEV of one argument
    share its count and sum words; the M2 words sit in the layout's one op-3 line, described to the combine by the
    words of their argument; ``fin`` / ``pfin`` name the words ``distagg._partials``' suffixes need."""
    from dxa.engine.window_dense import MAX_VARIANCE, Ineligible, _requests, plan_layout
    from dxa.ops.groupby import (_F_COUNT, _F_F64, _F_I64, _F_NOT, _F_SQRT, _F_VAR_POP, _F_VAR_SAMP, _MA_ADD_F64,
                                 _MA_ADD_U64, _MA_M2, _MA_MAX)
    aggs = _aggs("COUNT(*)", "AVG(temp)", "STDDEV(temp)", "VAR_POP(temp)", "variance(humidity)", "count_if(temp > 3)",
                 "bool_and(ok)", "some(ok)", "MIN(ok)")
    reqs = _requests(aggs)
    assert [f for _, f, _ in reqs] == ["count_star", "avg", "stddev", "var_pop", "variance", "count_if", "bmin", "bmax",
                                       "min"]
    types = {arg.key(): ("double", True) for _, f, arg in reqs if arg is not None}
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
    plain = _requests(_aggs("COUNT(*)", "AVG(temp)", "MAX(temp)"))
    Lp = plan_layout(plain, {a.key(): ("double", True) for _, _, a in plain if a is not None})
    assert _MA_M2 not in Lp["line_ops"] and not Lp["m2args"] and not any(Lp["m2desc"])
    # variance of a non-numeric argument, DISTINCT forms, too many variance arguments
    with pytest.raises(Ineligible):
        plan_layout(_requests(_aggs("STDDEV(ok)")), {_requests(_aggs("STDDEV(ok)"))[0][2].key(): ("boolean", False)})
    for bad in ("STDDEV(DISTINCT temp)", "count_if(DISTINCT ok)", "first(temp)", "last(temp)"):
        with pytest.raises(Ineligible):
            _requests(_aggs(bad))
    assert MAX_VARIANCE == 8
    _requests(_aggs(*[f"STDDEV(x{i})" for i in range(8)], "VAR_POP(x0)"))
    with pytest.raises(Ineligible, match="too many variance arguments"):
        _requests(_aggs(*[f"STDDEV(x{i})" for i in range(9)]))


def test_cpu_device_takes_the_generic_path():
    """On a CPU device the statements run (the oracle's own path) and no dense state is created; the oracle's row for
    a window in which nothing passes the WHERE has counts 0 (count_if among them) and NULL variances."""
    store = new_store()

    def each(b, q, rows):
        if q == Q_DNONE:
            assert rows == [{"dd": 0, "sd": None, "vp": None, "ci": 0}]

    run_stream(churn_stream(8), [Q_ALL, Q_DGLOB, Q_DNONE, Q_MOD], torch.device("cpu"), store, each)
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
    store = new_store(win=8)
    seen = {"blocks": 0}

    def each(b, q, rows):
        for d in dense_states(store).values():
            if not d.disabled:
                seen["blocks"] = max(seen["blocks"], len(d.blocks))

    run_stream(stable_stream(24, True, spread), [Q_ALL], gpu, store, each)
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
    store = new_store()
    counts = {"one": 0, "null": 0}

    def each(b, q, rows):
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

    run_stream(_edge_stream(14), [Q_EDGE], gpu, store, each)
    assert not only_state(store).disabled
    assert counts["one"] > 14 and counts["null"] > 14


@pytest.mark.gpu
def test_offset_values(gpu, monkeypatch):
    """Values near 1e9 with a spread of 64: the centred two-pass form keeps STDDEV to rel 1e-6 (Σx² − (Σx)²/n would be
    off by orders of magnitude)."""
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "BLOCK", 2)
    store = new_store()
    run_stream(stable_stream(14, False), [Q_OFFSET], gpu, store, rel=1e-6)
    assert not only_state(store).disabled


@pytest.mark.gpu
def test_rebuild_moves_m2_lines(gpu, monkeypatch):
    """Ids drift through a 16-id dictionary that grows to 64 at most: every rebuild renumbers the op-3 line with the
    others, and the 2-pane blocks are combined again afterwards."""
    set_caps(monkeypatch, 16, 64, 1 << 16, 1 << 20, block=2)
    store = new_store()
    run_stream(churn_stream(40), [Q_SD], gpu, store)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert d.rebuilds > 0 and d.gcap <= 64


@pytest.mark.gpu
def test_straddles_the_lds_bound(gpu, monkeypatch):
    """Group ids on both sides of win_m2_kernel's LDS bound in one pane (two rows per id, several workgroups), and a
    second statement whose three groups are all privatised."""
    from dxa.engine import window_dense
    from dxa.ops import native as N
    import numpy as np
    L = N.lib().dxa_win_m2_lds_groups()
    assert L > 0
    if L + 200 > window_dense.DENSE_GROUPS:
        monkeypatch.setattr(window_dense, "DENSE_GROUPS", 2 * (L + 200))
    rng = np.random.default_rng(37)
    stream = []
    for b in range(9):
        ids = np.repeat(np.arange(L + 200), 2)
        rng.shuffle(ids)
        stream.append(((100 + b) * S, batch(rng, (100 + b) * S, ids), ids))
    store = new_store()
    run_stream(stream, [Q_SD, Q_MOD], gpu, store)
    states = list(dense_states(store).values())
    assert len(states) == 2 and not any(d.disabled for d in states)


@pytest.mark.gpu
def test_mixed_with_count_distinct(gpu):
    """Variance beside COUNT(DISTINCT x): grouped, global, and the global form's empty-window row (counts 0,
    variance NULL)."""
    store = new_store()

    def each(b, q, rows):
        if q == Q_DNONE:
            assert rows == [{"dd": 0, "sd": None, "vp": None, "ci": 0}]

    run_stream(churn_stream(12), [Q_DGRP, Q_DGLOB, Q_DNONE], gpu, store, each)
    states = list(dense_states(store).values())
    assert len(states) == 3 and not any(d.disabled for d in states)
    assert all(len(d.pairs) == 1 and 3 in d.layout["line_ops"] for d in states)


@pytest.mark.gpu
def test_plain_statement_has_no_m2_line(gpu):
    store = new_store()
    run_stream(churn_stream(12), [Q_INT], gpu, store)
    d = only_state(store)
    assert not d.disabled and 3 not in d.layout["line_ops"] and d.m2desc_dev is None


@pytest.mark.gpu
def test_partials(gpu, monkeypatch):
    """The N-rank form at world size 1: the view is marked partitioned and ``dxa.parallel.active`` patched, so
    ``_paned_aggregate`` takes ``dense_partials`` → ``exchange_partials`` → ``merge_partials``.  The key exchange
    needs a process group, so it is replaced by what it is at world size 1: the identity."""
    from dxa import parallel as P
    from dxa.engine import distagg, window_dense
    monkeypatch.setattr(P, "active", lambda: True)
    monkeypatch.setattr(distagg, "exchange_partials", lambda partial, key_names, grouped: (partial, P.HASHED))
    calls = {"n": 0}
    real = window_dense.dense_partials

    def counted(*a, **k):
        got = real(*a, **k)
        calls["n"] += got is not None
        return got

    monkeypatch.setattr(window_dense, "dense_partials", counted)

    def prepare(view):
        view.dist = P.PARTITIONED

    store = new_store()
    stream = churn_stream(12)
    run_stream(stream, [Q_PART], gpu, store, prepare=prepare)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert calls["n"] >= len(stream) - 4          # (the watermark keeps the first windows empty)
