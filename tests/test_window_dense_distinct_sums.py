"""SUM / AVG(DISTINCT x), count(DISTINCT a, b, …) and approx_count_distinct over sliding windows from the dense ring
(window_dense.py ``PairState``, window_ring.hip ``win_distinct_fold_kernel<true>``): the pair dictionary of
COUNT(DISTINCT x) already holds every live pair's x, so the distinct fold adds the live pairs' values into sum words
beside the count, and a wider pair key — (group id, a, b, …) — counts distinct tuples.  The oracle is the CPU evaluator
over the materialised window (no GPU code in it).  Rows are compared value by value with ``==`` (NaN equal to NaN; a
zero sum may differ in sign from the generic path, which ``==`` does not see), result types included; ``t`` values are
multiples of 0.25 below 2^20, so every f64 sum is exact in any order."""
import math
import struct

import pytest
import torch

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from dxa.engine.expr import EvalContext
from tests.window_dense_support import (S, Comparison, aggs_of, answer, churn_stream, dense_states, materialised,
                                        new_store, only_state, oracle, rows_of, run_stream, set_caps,
                                        with_syncs_counted)

SAME = Comparison("tolerant", types=True)       # no tolerance: a float equals the oracle's under ==, NaN with NaN
Q_MIX = ("SELECT deviceId, COUNT(*) AS c, AVG(t) AS av, COUNT(DISTINCT k) AS dk, SUM(DISTINCT k) AS sk, "
         "AVG(DISTINCT k) AS ak, SUM(DISTINCT t) AS st, approx_count_distinct(k) AS ap, count(DISTINCT k, t) AS dkt, "
         "SUM(DISTINCT k) + 1 AS sk1 FROM W GROUP BY deviceId")
Q_GLOB = ("SELECT COUNT(DISTINCT t) AS dt, SUM(DISTINCT t) AS st, AVG(DISTINCT t) AS at, SUM(DISTINCT k) AS sk, "
          "approx_count_distinct(t, 0.05) AS ap, count(DISTINCT k, t) AS dkt FROM W")
Q_GRP = ("SELECT deviceId, COUNT(DISTINCT t) AS dt, SUM(DISTINCT t) AS st, AVG(DISTINCT t) AS at, SUM(DISTINCT k) AS sk, "
         "AVG(DISTINCT k) AS ak FROM W GROUP BY deviceId")
Q_NONE = ("SELECT COUNT(DISTINCT k) AS dk, SUM(DISTINCT k) AS sk, AVG(DISTINCT t) AS at, approx_count_distinct(k) AS ap, "
          "count(DISTINCT k, t) AS dkt FROM W WHERE t > 100000000")                      # never a row
# few values per id, so the pairs of a 64-id window fit small dictionaries: ``k`` has 3 values and ``kind`` follows it
Q_LIFE = ("SELECT deviceId, SUM(DISTINCT k) AS sk, AVG(DISTINCT k) AS ak, COUNT(DISTINCT k) AS dk, "
          "count(DISTINCT k, kind) AS dkk, COUNT(*) AS c FROM W GROUP BY deviceId")
Q_WIDE = ("SELECT deviceId, SUM(DISTINCT t) AS st, AVG(DISTINCT t) AS at, count(DISTINCT t, k) AS dtk, COUNT(*) AS c "
          "FROM W GROUP BY deviceId")
Q_COUNT_ONLY = "SELECT deviceId, COUNT(*) AS c, COUNT(DISTINCT k) AS dk FROM W GROUP BY deviceId"
Q_SUMS = ("SELECT deviceId, COUNT(*) AS c, COUNT(DISTINCT k) AS dk, SUM(DISTINCT k) AS sk, AVG(DISTINCT k) AS ak "
          "FROM W GROUP BY deviceId")


def table(T, n, ids, cols, mid_pane=False):
    """One batch: ``ts`` spread over the batch's second, every eighth row at the batch time itself — the one instant
    of the window's oldest pane that is still in range, so that pane is clipped into a scratch slot (``mid_pane``:
    over the second's middle half instead, so no pane is clipped); ``deviceId`` = ids and the given (name, dtype,
    values, validity or None) columns."""
    if mid_pane:
        ts = [T - S // 4 - (i * 7919) % (S // 2) for i in range(n)]
    else:
        ts = [T if i % 8 == 0 else T - (i * 7919) % (S - 1) for i in range(n)]
    names = ["ts", "deviceId"]
    out = [PrimColumn("timestamp", torch.tensor(ts, dtype=torch.int64)),
           PrimColumn("long", torch.tensor([int(i) for i in ids], dtype=torch.int64))]
    for name, dtype, vals, valid in cols:
        names.append(name)
        if dtype == "string":
            c = strings_from_pylist(list(vals), "cpu")
            if valid is not None:
                c.valid = torch.tensor(valid)
            out.append(c)
        else:
            td = {"long": torch.int64, "int": torch.int32, "double": torch.float64, "float": torch.float32}[dtype]
            out.append(PrimColumn(dtype, torch.tensor(vals, dtype=td), None if valid is None else torch.tensor(valid)))
    return Table(names, out, n, "cpu")


def batch(rng, T, ids, few=False, mid_pane=False):
    """A batch with given device ids: ``k`` long, ``t`` double multiples of 0.25 with |t| < 2^20, both with NULLs,
    ``kind`` a string.  ``few``: k takes three values and kind follows k, so an id has at most three (id, k) pairs and
    three (id, k, kind) tuples."""
    rows = len(ids)
    if few:
        k = (rng.integers(0, 3, rows) * 7 - 5).tolist()
        kind = ["abc"[(v + 5) // 7] for v in k]
    else:
        k = rng.integers(-40, 40, rows).tolist()
        kind = ["abc"[int(v)] for v in rng.integers(0, 3, rows)]
    t = (rng.integers(-(1 << 22) + 1, 1 << 22, rows) // (1 << 14) * (1 << 14) * 0.25).tolist()    # 512 values
    cols = [("k", "long", k, (rng.random(rows) > 0.1).tolist()),
            ("t", "double", t, (rng.random(rows) > 0.1).tolist()), ("kind", "string", kind, None)]
    return table(T, rows, ids, cols, mid_pane)


def as_tuples(rows):
    """``rows_of``'s rows as tuples in column order, NaN as a token, so rows compare with ==."""
    return [tuple("NaN" if isinstance(v, float) and v != v else v for v in r.values()) for r in rows]


def tuple_sets(stream, *cols):
    """Per batch, the set of (id, values of ``cols``) over its rows without a NULL among them."""
    out = []
    for _T, tbl, ids in stream:
        vals = [tbl.column(c).to_pylist() for c in cols]
        out.append({(int(i), *v) for i, v in zip(ids, zip(*vals)) if None not in v})
    return out


def most_in(sets, k):
    return max(len(set().union(*sets[b:b + k])) for b in range(len(sets)))


# ---- CPU ------------------------------------------------------------------------------------------------------------
NEW_FORMS = ("SUM(DISTINCT t)", "AVG(DISTINCT t)", "COUNT(DISTINCT k, t)", "count(DISTINCT k, t, kind, deviceId)",
             "approx_count_distinct(k)", "approx_count_distinct(k, 0.05)")


def test_requests_accept_the_new_forms_under_their_keyword_only():
    from dxa.engine.window_dense import Ineligible, _requests
    for form in NEW_FORMS:
        with pytest.raises(Ineligible):
            _requests(aggs_of(form))
        with pytest.raises(Ineligible):
            _requests(aggs_of(form), picks=True)
    reqs = _requests(aggs_of(*NEW_FORMS, "COUNT(DISTINCT t)", "SUM(DISTINCT t) + 1", "COUNT(*)"), distinct_sums=True)
    assert [f for _, f, _ in reqs] == ["dsum", "davg", "dcount", "dcount", "dcount", "dcount", "dcount", "count_star"]
    assert [len(a) for _, f, a in reqs if isinstance(a, tuple)] == [2, 4]
    # the one-argument forms of k share a key, rsd or not; a tuple is a key of its own
    from dxa.engine.window_dense import distinct_key
    assert len({distinct_key(a) for _, f, a in reqs if f != "count_star"}) == 4
    for bad, why in (("count(DISTINCT k, t, kind, deviceId, ts)", "too many distinct columns"),
                     ("approx_count_distinct(k, t)", "approx_count_distinct"),
                     ("approx_count_distinct(k, 0.05, 1)", "approx_count_distinct"),
                     ("MIN(DISTINCT t)", "min distinct"), ("stddev(DISTINCT t)", "stddev distinct"),
                     ("SUM(DISTINCT k, t)", "sum distinct")):
        with pytest.raises(Ineligible, match=why):
            _requests(aggs_of(bad), distinct_sums=True)
    with pytest.raises(Ineligible, match="too many distinct arguments"):
        _requests(aggs_of("SUM(DISTINCT k)", "AVG(DISTINCT t)", "COUNT(DISTINCT kind)", "approx_count_distinct(ts)",
                        "COUNT(DISTINCT k, t)"), distinct_sums=True)


def test_layout_shares_the_dcount_slot():
    """COUNT / SUM / AVG(DISTINCT t) and approx_count_distinct(t) have one dcount slot, which is the count word of the
    sum and the average; the sum words are words no pane accumulates into (value kind -1): an MA_ADD_F64 word for the
    double sum and every average, an MA_ADD_U64 word for the integral sum."""
    from dxa.engine.window_dense import _requests, plan_layout
    from dxa.ops.groupby import _F_AVG, _F_COUNT, _F_F64, _F_I64, _MA_ADD_F64, _MA_ADD_U64, _MV_COUNT
    reqs = _requests(aggs_of("COUNT(DISTINCT t)", "SUM(DISTINCT t)", "AVG(DISTINCT t)", "approx_count_distinct(t)",
                           "SUM(DISTINCT k)", "AVG(DISTINCT k)", "count(DISTINCT k, t)", "COUNT(*)"),
                     distinct_sums=True)
    kt, kk = ("id", "t"), ("id", "k")
    L = plan_layout(reqs, {kt: ("double", True), kk: ("long", False)})
    assert L["slots"] == [(("count", None), _MV_COUNT, _MA_ADD_F64), (("dcount", kt), _MV_COUNT, _MA_ADD_F64),
                          (("dsumf", kt), -1, _MA_ADD_F64), (("dcount", kk), _MV_COUNT, _MA_ADD_F64),
                          (("dsumi", kk), -1, _MA_ADD_U64), (("dsumf", kk), -1, _MA_ADD_F64),
                          (("dcount", ("dtuple", kk, kt)), _MV_COUNT, _MA_ADD_F64)]
    assert L["line_ops"] == [_MA_ADD_U64, _MA_ADD_F64] and L["stride"] == 16
    assert L["order"] == [4] + [None] * 7 + [0, 1, 2, 3, 5, 6, None, None]
    assert L["dcount_word"] == {kt: 9, kk: 11, ("dtuple", kk, kt): 13}
    assert L["dsum_words"] == {kt: (-1, 10), kk: (0, 12)}
    assert L["fin"] == [(_F_COUNT, 9, -1), (_F_F64, 10, 9), (_F_AVG, 10, 9), (_F_COUNT, 9, -1), (_F_I64, 0, 11),
                        (_F_AVG, 12, 11), (_F_COUNT, 13, -1), (_F_COUNT, 8, -1)]
    assert [p[4] for p in L["plan"]] == [None, "double", "double", None, "long", "double", None, None]
    assert L["as_f64"] == [False, True, True, False, False, True, False, False]
    assert L["pfin"] == {("call", "count", False, True): {"cnt": (_F_COUNT, 8, -1)}}     # no mergeable partial
    # a float argument sums as a double; an int argument as a long
    L = plan_layout(_requests(aggs_of("SUM(DISTINCT t)", "SUM(DISTINCT k)"), distinct_sums=True),
                    {kt: ("float", True), kk: ("int", False)})
    assert L["dsum_words"] == {kt: (-1, 10), kk: (0, -1)} and [p[4] for p in L["plan"]] == ["double", "long"]


def test_layout_refuses_other_argument_types():
    from dxa.engine.decimal import parse_decimal_type
    from dxa.engine.window_dense import Ineligible, _requests, plan_layout
    for item, dtype, why in (("SUM(DISTINCT kind)", "string", "sum type"), ("AVG(DISTINCT kind)", "string", "avg type"),
                             ("SUM(DISTINCT ts)", "timestamp", "sum type"), ("AVG(DISTINCT b)", "boolean", "avg type"),
                             ("SUM(DISTINCT d)", parse_decimal_type("decimal(10,2)"), "argument type"),
                             ("AVG(DISTINCT d)", parse_decimal_type("decimal(10,2)"), "argument type")):
        reqs = _requests(aggs_of(item), distinct_sums=True)
        with pytest.raises(Ineligible, match=why):
            plan_layout(reqs, {reqs[0][2].key(): (dtype, False)})


def test_count_distinct_layout_is_the_one_it_was():
    """A layout with only COUNT(DISTINCT …) beside plain aggregates: the literal values the layout had before the
    distinct sums existed (no ``dsum_words`` key, the same slots, words and recipes)."""
    from dxa.engine.window_dense import _requests, plan_layout
    reqs = _requests(aggs_of("COUNT(DISTINCT kind)", "COUNT(DISTINCT temp)", "COUNT(*)", "SUM(temp)", "AVG(temp)",
                           "MAX(temp)"), distinct_sums=True)
    L = plan_layout(reqs, {("id", "temp"): ("double", True)})
    L.pop("pfin")
    assert L == {
        "as_f64": [False, False, False, True, True, True],
        "count_word": 0,
        "dcount_word": {("id", "kind"): 1, ("id", "temp"): 2},
        "fin": [(0, 1, -1), (0, 2, -1), (0, 0, -1), (2, 4, 3), (3, 5, 3), (4, 8, 3)],
        "line_ops": [1, 2],
        "m2args": [],
        "m2desc": [0] * 16,
        "nslots": 9,
        "order": [0, 1, 2, 3, 4, 5, None, None, 6, None, None, None, None, None, None, None],
        "plan": [(("call", "count", True, False, ("id", "kind")), "count", 1, None, None),
                 (("call", "count", True, False, ("id", "temp")), "count", 2, None, None),
                 (("call", "count", False, True), "count", 0, None, None),
                 (("call", "sum", False, False, ("id", "temp")), "sum", 4, 3, "double"),
                 (("call", "avg", False, False, ("id", "temp")), "avg", 5, 3, "double"),
                 (("call", "max", False, False, ("id", "temp")), "f64", 6, 3, "double")],
        "rows": [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1)],
        "slots": [(("count", None), 0, 1), (("dcount", ("id", "kind")), 0, 1), (("dcount", ("id", "temp")), 0, 1),
                  (("count", ("id", "temp")), 0, 1), (("sum", ("id", "temp")), 2, 1),
                  (("sumf", ("id", "temp")), 2, 1), (("max", ("id", "temp")), 3, 2)],
        "stride": 16}


def test_cpu_device_takes_the_generic_path():
    """On a CPU device the statements equal the oracle and no dense state is created."""
    store = new_store(6)
    run_stream(churn_stream(batch, 8), [Q_MIX, Q_GLOB, Q_NONE], torch.device("cpu"), store, SAME)
    assert not dense_states(store)
    T, tbl, _ = churn_stream(batch, 1)[0]
    views, _ = new_store(6).process(tbl, T, S)
    assert as_tuples(oracle(Q_NONE, views["W"])[0]) == [(0, None, None, 0, 0)]


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_statement_stays_dense(gpu):
    """Plain aggregates, the three aggregates of one distinct argument, a double distinct sum, approx_count_distinct,
    a two-column distinct count and a distinct sum inside an expression: one state, three pair states (k, t and
    (k, t)), one fold each; some pane is clipped on the way."""
    store = new_store(6)
    seen = {"clipped": 0}

    def each(b, q, rows, view, table):
        seen["clipped"] += any(not full for _pane, full in view.pieces())

    run_stream(churn_stream(batch, 12), [Q_MIX], torch.device("cuda", 0), store, SAME, each)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert len(d.pairs) == 3 and [len(ps.keys) for ps in d.pairs] == [2, 2, 3]
    assert [(ps.isum >= 0, ps.fsum >= 0) for ps in d.pairs] == [(True, True), (False, True), (False, False)]
    assert seen["clipped"] > 0


@pytest.mark.gpu
def test_one_pair_state_for_the_three_aggregates_of_one_argument(gpu):
    store = new_store(6)
    run_stream(churn_stream(batch, 8), [Q_SUMS], torch.device("cuda", 0), store, SAME)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None and len(d.pairs) == 1


def _exact_stream(nb, npairs):
    """Every batch holds the same ``npairs`` rows: row i belongs to id i % 3 — consecutive pairs alternate between
    three parents — and has a k and a t of its own, so the window has exactly ``npairs`` live (id, k), (id, t) and
    (id, k, t) pairs under three parents, and as many under the one parent of the global form."""
    out = []
    for b in range(nb):
        T = (100 + b) * S
        ids = [i % 3 for i in range(npairs)]
        cols = [("k", "long", [3 * i - 700 for i in range(npairs)], None),
                ("t", "double", [0.25 * (5 * i - 1111) for i in range(npairs)], None)]
        out.append((T, table(T, npairs, ids, cols), ids))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("npairs", [15, 16, 17, 1025])
def test_wave_reduction_at_chunk_and_wave_boundaries(gpu, npairs):
    """15 / 16 / 17 live pairs straddle a lane's 16-pair chunk, 1025 a whole wave's 64 × 16: in the global form whole
    waves share the one parent, in the grouped form a ballot has three leaders."""
    assert npairs in (15, 16, 17) or npairs > 64 * 16
    store = new_store(6)
    stream = _exact_stream(8, npairs)

    def each(b, q, rows, view, table):
        if q == Q_GLOB and b == len(stream) - 1:
            assert rows[0]["dt"] == npairs and rows[0]["dkt"] == npairs

    run_stream(stream, [Q_GLOB, Q_GRP], torch.device("cuda", 0), store, SAME, each)
    states = list(dense_states(store).values())
    assert len(states) == 2
    for d in states:
        assert not d.disabled and d.disabled_reason is None
        assert all(int(d.scal[4 + 4 * j]) == npairs for j in range(len(d.pairs)))      # the pair counters


def _null_stream(nb):
    """64 rows per batch over 4 ids: id 0 never has a k; elsewhere k is NULL on some rows, t on others, both on a few."""
    out = []
    for b in range(nb):
        T = (100 + b) * S
        n = 64
        ids = [i % 4 for i in range(n)]
        kv = [i % 4 != 0 and (i + b) % 5 != 0 for i in range(n)]
        tv = [(i + b) % 3 != 0 for i in range(n)]
        cols = [("k", "long", [(i * 5 + b) % 9 - 4 for i in range(n)], kv),
                ("t", "double", [0.25 * ((i + 2 * b) % 7) for i in range(n)], tv)]
        out.append((T, table(T, n, ids, cols), ids))
        combos = {(a, c) for a, c, i in zip(kv, tv, ids) if i != 0}
        assert combos == {(True, True), (True, False), (False, True), (False, False)}
    return out


@pytest.mark.gpu
def test_nulls(gpu):
    """A group whose k is always NULL: SUM and AVG NULL, the counts 0; a tuple with a NULL in either place or both is
    not counted."""
    q = ("SELECT deviceId, SUM(DISTINCT k) AS sk, AVG(DISTINCT k) AS ak, COUNT(DISTINCT k) AS dk, "
         "approx_count_distinct(k) AS ap, count(DISTINCT k, t) AS dkt, count(DISTINCT t) AS dt FROM W GROUP BY deviceId")
    store = new_store(6)
    seen = []

    def each(b, _q, rows, view, table):
        seen.extend(r for r in as_tuples(rows) if r[0] == 0)

    run_stream(_null_stream(8), [q], torch.device("cuda", 0), store, SAME, each)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert seen and all(r[1:6] == (None, None, 0, 0, 0) and r[6] > 0 for r in seen)


def _special_stream(nb):
    """48 rows per batch over 6 string groups with their own sets of doubles: zeros of both signs, two NaN bit
    patterns, the infinities, alone and together with finite values; and longs whose distinct sum passes INT64_MAX."""
    nan2 = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000001))[0]
    inf = float("inf")
    sets = [[0.0, -0.0, 1.5], [float("nan"), nan2, 1.0], [inf, 2.0, -0.0], [-inf, 0.25], [inf, -inf, 3.0], [-0.0]]
    big = [(1 << 62) + 3, (1 << 62) + 5, (1 << 62) + 7, 11]
    out = []
    for b in range(nb):
        T = (100 + b) * S
        n = 48
        grp = [f"g{i % 6}" for i in range(n)]
        d = [sets[i % 6][(i // 6 + b) % len(sets[i % 6])] for i in range(n)]
        k = [big[(i // 6 + b) % 4] for i in range(n)]
        cols = [("grp", "string", grp, None), ("d", "double", d, [(i + b) % 11 != 0 for i in range(n)]),
                ("k", "long", k, None)]
        out.append((T, table(T, n, [0] * n, cols), None))
    return out


@pytest.mark.gpu
def test_special_doubles_and_wrapping_longs(gpu):
    """-0.0 sums as 0.0 and every NaN is one value (the dictionary's normalised bits): the sums equal the oracle's
    under ==, NaN with NaN; the long sum wraps as the oracle's does."""
    q = ("SELECT grp, SUM(DISTINCT d) AS sd, AVG(DISTINCT d) AS ad, COUNT(DISTINCT d) AS dd, SUM(DISTINCT k) AS sk, "
         "COUNT(DISTINCT k) AS dk, count(DISTINCT d, k) AS ddk FROM W GROUP BY grp")
    store = new_store(6)
    last = {}

    def each(b, _q, rows, view, table):
        last["rows"] = as_tuples(rows)

    run_stream(_special_stream(8), [q], torch.device("cuda", 0), store, SAME, each)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    by = {r[0]: r for r in last["rows"]}
    assert by["g0"][1:4] == (1.5, 0.75, 2) and by["g1"][1:4] == ("NaN", "NaN", 2)
    assert by["g2"][1] == math.inf and by["g3"][1] == -math.inf and by["g4"][1] == "NaN"
    assert by["g5"][1:4] == (0.0, 0.0, 1)
    wrapped = (3 * (1 << 62) + 15 + 11 + (1 << 63)) % (1 << 64) - (1 << 63)
    assert wrapped < 0 and all(r[4] == wrapped and r[5] == 4 for r in last["rows"])


@pytest.mark.gpu
def test_float_and_int_arguments(gpu):
    """SUM(DISTINCT float) is a double and SUM(DISTINCT int) a long (the generic path keeps the argument's storage,
    so only the values are compared here)."""
    import numpy as np
    rng = np.random.default_rng(5)
    q = "SELECT deviceId, SUM(DISTINCT f) AS sf, AVG(DISTINCT f) AS af, SUM(DISTINCT i) AS si, AVG(DISTINCT i) AS ai " \
        "FROM W GROUP BY deviceId"
    dev = torch.device("cuda", 0)
    store = new_store(6)
    for b in range(8):
        T = (100 + b) * S
        n = 64
        ids = rng.integers(0, 5, n)
        cols = [("f", "float", (rng.integers(-64, 64, n) * 0.25).tolist(), (rng.random(n) > 0.1).tolist()),
                ("i", "int", rng.integers(-30, 30, n).tolist(), (rng.random(n) > 0.1).tolist())]
        views, _ = store.process(table(T, n, ids, cols).to(dev), T, S)
        rows, types = rows_of(answer(q, views["W"], dev))
        if rows:
            assert list(types.values()) == ["long", "double", "double", "long", "double"]
        assert as_tuples(rows) == as_tuples(oracle(q, views["W"])[0]), b
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None and len(d.pairs) == 2


@pytest.mark.gpu
def test_pairs_recycle_with_sums_and_two_columns(gpu, monkeypatch):
    """At most 192 (id, k) pairs and as many (id, k, kind) tuples are live while 168 ids stream through a 64-id group
    dictionary and 256-pair dictionaries that may not grow: both pair states recycle, and every group rebuild
    renumbers their parents."""
    set_caps(monkeypatch, 64, 64, 256, 256)
    stream = churn_stream(batch, 40, few=True)
    for cols in (("k",), ("k", "kind")):
        sets = tuple_sets(stream, *cols)
        assert len(set().union(*sets)) > 256 and most_in(sets, 14) <= 192
    store = new_store(6)
    run_stream(stream, [Q_LIFE], torch.device("cuda", 0), store, SAME)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert len(d.pairs) == 2 and len(d.pairs[1].keys) == 3
    assert all(ps.rebuilds >= 1 and ps.pcap == 256 for ps in d.pairs)
    assert d.rebuilds >= 3 and d.gcap == 64


@pytest.mark.gpu
def test_pairs_grow_with_sums_and_two_columns(gpu, monkeypatch):
    """The (id, t) pairs and the (id, t, k) tuples outgrow 64: both dictionaries double (their value columns move)
    while the 64-id group dictionary recycles under them."""
    set_caps(monkeypatch, 64, 64, 64, 8192)
    stream = churn_stream(batch, 30)
    assert most_in(tuple_sets(stream, "t", "k"), 16) <= 4096
    store = new_store(6)
    run_stream(stream, [Q_WIDE], torch.device("cuda", 0), store, SAME)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert len(d.pairs) == 2 and d.rebuilds >= 1
    assert all(256 <= ps.pcap <= 8192 and ps.rebuilds >= 1 for ps in d.pairs)


@pytest.mark.gpu
def test_pair_blocks(gpu, monkeypatch):
    """A 12 s window of 2-pane blocks: the sums are folded from block slots' presence rows, and again after rebuilds."""
    set_caps(monkeypatch, 64, 128, 256, 512, block=2)
    store = new_store(12)
    seen = {"blocks": 0}

    def each(b, q, rows, view, table):
        for d in dense_states(store).values():
            if d.pairs and not d.disabled:
                seen["blocks"] = max(seen["blocks"], len(d.blocks))

    run_stream(churn_stream(batch, 36, few=True), [Q_LIFE], torch.device("cuda", 0), store, SAME, each)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert seen["blocks"] > 4
    assert d.rebuilds + sum(ps.rebuilds for ps in d.pairs) >= 1


@pytest.mark.gpu
def test_empty_window_of_the_global_form(gpu):
    """Nothing passes the WHERE: Spark's one row — the counts 0, the sum and the average NULL."""
    store = new_store(6)
    seen = []

    def each(b, q, rows, view, table):
        seen.append(as_tuples(rows))

    run_stream(churn_stream(batch, 6), [Q_NONE], torch.device("cuda", 0), store, SAME, each)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None and d.global_form
    assert seen[-1] == [(0, None, None, 0, 0)]


@pytest.mark.gpu
def test_deferred(gpu, monkeypatch):
    """ctx.defer_dense: a full pair or group dictionary is reported through the DeferredTable's completion; the
    re-run of the statement rebuilds and answers from the ring."""
    from dxa.engine.column import DeferredTable
    set_caps(monkeypatch, 64, 64, 256, 256)
    dev = torch.device("cuda", 0)
    store = new_store(6)
    through_deferred = 0

    def rebuilds():
        return sum(d.rebuilds + sum(p.rebuilds for p in d.pairs) for d in dense_states(store).values())

    for b, (T, tbl, _ids) in enumerate(churn_stream(batch, 40, few=True)):
        views, _ = store.process(tbl.to(dev), T, S)
        ctx = EvalContext(now_us=0, device=dev)
        ctx.defer_dense = True
        got = answer(Q_LIFE, views["W"], ctx=ctx)
        if b >= 4:
            assert isinstance(got, DeferredTable) and ctx.pending
        before = rebuilds()
        SAME.check(Q_LIFE, views["W"], got, b)
        through_deferred += rebuilds() > before
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None and len(d.pairs) == 2
    assert through_deferred >= 1


@pytest.mark.gpu
def test_pair_capacity_reached_falls_back_with_a_reason(gpu, monkeypatch):
    """The (id, t) pairs cannot fit 64 and may not grow: every batch still equals the oracle (the generic path), and
    the state says why."""
    set_caps(monkeypatch, 1 << 16, 1 << 20, 64, 64)
    store = new_store(6)
    run_stream(churn_stream(batch, 10), [Q_WIDE], torch.device("cuda", 0), store, SAME)
    d = only_state(store)
    assert d.disabled and d.disabled_reason == "pair dictionary full"


@pytest.mark.gpu
def test_arbitrary_doubles_within_the_reordering_bound(gpu):
    """Normal variates × 1e6: here the order of the adds matters.  Two recursive f64 summations of the same n values
    in different orders differ by at most (n − 1) · 2^-52 · Σ|x| (each is within (n − 1) · 2^-53 · Σ|x| of the exact
    sum, to first order — and the wave tree's error is below the recursive bound); the bound is computed per group
    from the window's own distinct values."""
    import numpy as np
    rng = np.random.default_rng(11)
    pool = rng.standard_normal(400) * 1e6
    q = "SELECT deviceId, SUM(DISTINCT x) AS sx, COUNT(DISTINCT x) AS dx FROM W GROUP BY deviceId"
    dev = torch.device("cuda", 0)
    store = new_store(6)
    worst = 0.0
    for b in range(8):
        T = (100 + b) * S
        n = 300
        ids = rng.integers(0, 3, n)
        x = pool[rng.integers(0, len(pool), n)].tolist()
        views, _ = store.process(table(T, n, ids, [("x", "double", x, None)]).to(dev), T, S)
        got, types = rows_of(answer(q, views["W"], dev))
        want, wtypes = oracle(q, views["W"])
        assert list(types.items()) == list(wtypes.items())
        got, want = as_tuples(got), as_tuples(want)
        assert [r[0] for r in got] == [r[0] for r in want]
        w = materialised(views["W"])
        values = {}
        for g, v in zip(w.column("deviceId").to_pylist(), w.column("x").to_pylist()):
            values.setdefault(g, set()).add(v)
        for (g, sx, dx), (_g, wsx, wdx) in zip(got, want):
            vals = values[g]
            bound = (len(vals) - 1) * 2.0 ** -52 * sum(abs(v) for v in vals)
            print(f"batch {b} group {g}: n {len(vals)} |got - want| {abs(sx - wsx):.3e} bound {bound:.3e}")
            assert dx == wdx == len(vals)
            assert abs(sx - wsx) <= bound, (b, g, sx, wsx, bound)
            worst = max(worst, len(vals))
    assert worst > 64                               # groups whose values span more than one lane's chunk and wave
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None


@pytest.mark.gpu
@pytest.mark.parametrize("q", [Q_COUNT_ONLY, Q_SUMS])
def test_entry_points_and_one_sync_per_steady_state_batch(gpu, monkeypatch, q):
    """The native entry points of a batch in which one pane enters the window and nothing is rebuilt are those of a
    COUNT(DISTINCT x) statement before the distinct sums existed — the group insert, the multi-aggregate, the pair
    state's prep / insert / mark, on a batch that completes a 2-pane block one block combine and one presence OR, then
    the one answer — with or without distinct sums: the fold differs only inside ``dxa_win_answer``.  And the batch
    makes one synchronising read (counted as tools/sync_audit.py counts them)."""
    from dxa.engine import window_dense
    from launch_count import count_launches
    monkeypatch.setattr(window_dense, "BLOCK", 2)
    dev = torch.device("cuda", 0)
    store = new_store(6)
    pane = ["dxa_win_insert_fused", "dxa_aggregate_multi", "dxa_win_pair_prep", "dxa_win_insert_fused",
            "dxa_win_pair_mark"]
    block = ["dxa_win_combine_block", "dxa_win_pair_or_block"]
    completed_seen = set()
    syncs = []
    for b, (T, tbl, _ids) in enumerate(churn_stream(batch, 16, rows=64, few=True, mid_pane=True)):
        views, _ = store.process(tbl.to(dev), T, S)
        states = list(dense_states(store).values())
        before = set(states[0].blocks) if states else set()
        torch.cuda.synchronize(dev)
        if b % 3:
            with count_launches() as log:
                out = answer(q, views["W"], dev)
        else:
            log = None
            out, n = with_syncs_counted(lambda: answer(q, views["W"], dev))
            syncs.append(n)
        SAME.check(q, views["W"], out, b)
        if b < 8 or log is None:                    # the watermark and the 6-pane window: full from batch 7 on
            continue
        d = only_state(store)
        assert not d.disabled and d.rebuilds == 0 and len(d.pairs) == 1
        completed = len(set(d.blocks) - before)
        completed_seen.add(completed)
        native = [nm for nm in log if nm.startswith("dxa_")]
        assert native == pane + block * completed + ["dxa_win_answer"], (b, native)
    assert completed_seen == {0, 1}
    print("synchronising calls per batch:", syncs)
    assert syncs[-3:] == [1, 1, 1]
