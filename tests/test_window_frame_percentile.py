"""Order statistics as window functions: percentile / median (linear interpolation, double) and percentile_approx /
approx_percentile (the smallest counted value whose rank reaches p·count, the argument's type) ``OVER (PARTITION BY …
ORDER BY … frame)``, with scalar and ``array(...)`` percentages.

The oracle is written here and holds no engine code: per row it takes a Python ``sorted`` of the frame's counted
values (NaN greatest) and applies, in Python floats, with c counted values v[0 .. c):

    exact:        pos = p·(c − 1), lo = ⌊pos⌋, hi = min(lo + 1, c − 1), v[lo] + (pos − lo)·(v[hi] − v[lo])
    approximate:  v[clamp(⌈p·c⌉ − 1, 0, c − 1)]

and NULL for c = 0.  Values are multiples of 0.25 in [0, 64), skewed so that ties are frequent, with 10 % NULLs.  For
p ∈ {0, 0.25, 0.5, 0.75, 1} every pos − lo is a multiple of 0.25 and every product exact, so those results are
compared with ``==``; for p ∈ {0.01, 0.9, 0.99} the exact form is held to the project's bound for doubles,
max(1e-9·|want|, 1e-12).  The approximate form returns an input value: always ``==``.  NaN equals NaN.

The selection primitive (the k-th smallest counted row of a frame, as a row POSITION) is compared with a brute-force
sort by (key, position) on hand-built frames: the tensor-operation wavelet matrix on the CPU, and the two entry points
of window_select.hip on the GPU.
"""
import bisect
import math
import random
from decimal import Decimal

import pytest
import torch

from dxa.engine import windowfn as W
from dxa.engine.column import Table
from dxa.engine.expr import EvalContext
from dxa.engine.query import Catalog, QueryError, run_sql
from dxa.engine.types import StructField, StructType

SCHEMA = StructType((StructField("id", "long"), StructField("k", "string"), StructField("t", "long"),
                     StructField("v", "double")))
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
NAN = float("nan")
INF = float("inf")
EXACT_P = (0.0, 0.25, 0.5, 0.75, 1.0)                # pos − lo is a multiple of 0.25: interpolation is exact
ROUNDED_P = (0.01, 0.9, 0.99)
SELECT_ENTRIES = ("dxa_frame_select_direct", "dxa_frame_select_tree")


def _run(rows, sql, device="cpu"):
    c = Catalog()
    c.register("T", Table.from_pylist(rows, SCHEMA, device))
    return run_sql(sql, c, EvalContext(now_us=0)).to_pylist()


# -- the oracle -------------------------------------------------------------------------------------------------------

def _ascending(values):
    return sorted(values, key=lambda v: (math.isnan(v), v))          # NaN orders greatest


def _exact(v, p):
    c = len(v)
    if c == 0:
        return None
    pos = p * (c - 1)
    lo = math.floor(pos)
    hi = min(lo + 1, c - 1)
    return v[lo] + (pos - lo) * (v[hi] - v[lo])


def _approx(v, p):
    c = len(v)
    if c == 0:
        return None
    return v[min(max(math.ceil(p * c) - 1, 0), c - 1)]


def _same(got, want, tolerant=False):
    if want is None or got is None:
        return got is None and want is None
    got, want = float(got), float(want)
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    if got == want:                                                   # infinities included
        return True
    return tolerant and abs(got - want) <= max(1e-9 * abs(want), 1e-12)


# A call is (sql, exact, percentages, array result); CALLS covers the five spellings, scalar and array p, and the
# ignored accuracy argument.  The widest call asks for 10 ranks, so each is one launch of an entry point.
CALLS = [("percentile(v, 0.5)", True, (0.5,), False),
         ("median(v)", True, (0.5,), False),
         ("percentile(v, array(0, 0.25, 0.5, 0.75, 1))", True, EXACT_P, True),
         ("percentile(v, array(0.01, 0.9, 0.99))", True, ROUNDED_P, True),
         ("percentile_approx(v, 0.9)", False, (0.9,), False),
         ("approx_percentile(v, array(0, 0.25, 0.5, 0.75, 1, 0.01, 0.9, 0.99), 100)", False, EXACT_P + ROUNDED_P, True),
         ("percentile_approx(v, 0.25, 50)", False, (0.25,), False),
         ("approx_percentile(v, 1.0)", False, (1.0,), False)]


def _expected(counted, calls):
    """The oracle's results of ``calls`` over one frame's counted values (any order)."""
    v = _ascending(counted)
    out = []
    for _, exact, ps, is_array in calls:
        r = [(_exact if exact else _approx)(v, p) for p in ps]
        out.append(r if is_array else r[0])
    return out


def _check(got, want, call, where):
    _, exact, ps, is_array = call
    if not is_array:
        got, want = [got], [want]
    assert isinstance(got, list) and len(got) == len(ps), (call[0], got, where)
    for g, w, p in zip(got, want, ps):
        assert _same(g, w, tolerant=exact and p in ROUNDED_P), (call[0], p, g, w, where)


# -- frames in Python -------------------------------------------------------------------------------------------------
# A window is (sql, order, frame): ``order`` names how a partition is sorted, ``frame(keys, p)`` gives the inclusive
# row range of position p from the partition's ascending ordering-axis values ``keys``.

def _sorted_partitions(rows, order):
    def axis(r):
        if order == "id":
            return r["id"]
        if order == "t":                                      # ASC NULLS FIRST
            return -INF if r["t"] is None else r["t"]
        return INF if r["t"] is None else -r["t"]             # "t_desc": DESC NULLS LAST, axis negated
    parts = {}
    for r in rows:
        parts.setdefault(r["k"], []).append(r)
    out = []
    for g in parts.values():
        g = sorted(g, key=lambda r: (axis(r), r["id"]))
        out.append((g, [axis(r) for r in g]))
    return out


def _rows_frame(lo_off, hi_off):
    def frame(keys, p):
        return max(0, p + lo_off), min(len(keys) - 1, p + hi_off)
    return frame


def _range_frame(lo_off, hi_off):
    def frame(keys, p):
        c = keys[p]
        lower, upper = (c, c) if math.isinf(c) else (c + lo_off, c + hi_off)        # a NULL key: its peers
        return bisect.bisect_left(keys, lower), bisect.bisect_right(keys, upper) - 1
    return frame


def _running_peers(keys, p):
    return 0, bisect.bisect_right(keys, keys[p]) - 1


def _whole(keys, p):
    return 0, len(keys) - 1


ROWS_GRID = {i: [(f"PARTITION BY k ORDER BY id ROWS BETWEEN {i} PRECEDING AND {j} FOLLOWING", "id", _rows_frame(-i, j))
                 for j in range(5)] for i in range(5)}
OTHER_WINDOWS = {
    "peers": ("PARTITION BY k ORDER BY t", "t", _running_peers),
    "whole": ("PARTITION BY k", "id", _whole),
    "range_asc": ("PARTITION BY k ORDER BY t RANGE BETWEEN 3 PRECEDING AND 2 FOLLOWING", "t", _range_frame(-3, 2)),
    "range_desc": ("PARTITION BY k ORDER BY t DESC RANGE BETWEEN 3 PRECEDING AND 2 FOLLOWING", "t_desc",
                   _range_frame(-3, 2)),
    "empty_near_end": ("PARTITION BY k ORDER BY id ROWS BETWEEN 3 FOLLOWING AND 5 FOLLOWING", "id", _rows_frame(3, 5)),
}
RUNNING = ("PARTITION BY k ORDER BY id", "id", _rows_frame(-10 ** 9, 0))


def _statement(spec, calls):
    return "SELECT id, " + ", ".join(f"{c[0]} OVER ({spec}) AS f{i}" for i, c in enumerate(calls)) + " FROM T"


_ORACLE = {}                      # (rows name, window sql) → {id: expected results of CALLS}: computed once, shared


def _oracle(name, rows, window):
    spec, order, frame = window
    if (name, spec) not in _ORACLE:
        want = {}
        for g, keys in _sorted_partitions(rows, order):
            for p, r in enumerate(g):
                lo, hi = frame(keys, p)
                want[r["id"]] = _expected([q["v"] for q in g[lo:hi + 1] if q["v"] is not None], CALLS)
        _ORACLE[(name, spec)] = want
    return _ORACLE[(name, spec)]


def _check_window(name, rows, window, device):
    """Run CALLS over one window on ``device`` and compare every row with the oracle; rows keep input order."""
    got = _run(rows, _statement(window[0], CALLS), device)
    assert [r["id"] for r in got] == [r["id"] for r in rows]
    want = _oracle(name, rows, window)
    for r in got:
        for i, call in enumerate(CALLS):
            _check(r[f"f{i}"], want[r["id"]][i], call, (window[0], r["id"]))


def _value(rnd):
    """A multiple of 0.25 in [0, 64), skewed towards 0 so that ties are frequent."""
    return int(256 * rnd.random() ** 2) / 4.0


def _random_rows(n, seed, keys, null_share, tmax):
    rnd = random.Random(seed)
    return [{"id": i, "k": rnd.choice(keys), "t": rnd.choice([None] + list(range(tmax))),
             "v": None if rnd.random() < null_share else _value(rnd)} for i in range(n)]


CPU_ROWS = _random_rows(300, 11, ["p", "q", "r", None], 0.1, 20)

# -- CPU: SQL surface -------------------------------------------------------------------------------------------------

SEVEN = [
    {"id": 1, "k": "a", "t": 10, "v": 1.0},
    {"id": 2, "k": "a", "t": 20, "v": 2.0},
    {"id": 3, "k": "a", "t": 20, "v": None},
    {"id": 4, "k": "a", "t": 30, "v": 4.0},
    {"id": 5, "k": "b", "t": 5, "v": 10.0},
    {"id": 6, "k": "b", "t": None, "v": 20.0},
    {"id": 7, "k": None, "t": 1, "v": 7.0},
]


def test_hand_computed_rows():
    """The statement of the issue, on seven rows."""
    got = _run(SEVEN, "SELECT id, percentile(v, 0.5) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 9 PRECEDING AND "
                      "CURRENT ROW) AS run, median(v) OVER (PARTITION BY k) AS med, percentile_approx(v, 0.5) OVER "
                      "(PARTITION BY k) AS ap, percentile(v, array(0, 0.25, 1)) OVER (PARTITION BY k) AS arr, "
                      "percentile(v, 0.5) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN CURRENT ROW AND CURRENT ROW) "
                      "AS own FROM T ORDER BY id")
    by = {r["id"]: r for r in got}
    # partition a by id: 1, 2, NULL, 4 — running frames {1}, {1, 2}, {1, 2}, {1, 2, 4}
    assert [by[i]["run"] for i in (1, 2, 3, 4)] == [1.0, 1.5, 1.5, 2.0]
    assert by[1]["med"] == 2.0 and by[1]["ap"] == 2.0 and by[1]["arr"] == [1.0, 1.5, 4.0]
    assert by[5]["med"] == 15.0 and by[6]["ap"] == 10.0 and by[5]["arr"] == [10.0, 12.5, 20.0]
    assert by[7]["med"] == 7.0 and by[7]["ap"] == 7.0 and by[7]["arr"] == [7.0, 7.0, 7.0]
    assert by[3]["own"] is None and by[2]["own"] == 2.0          # the one-row frame of a NULL holds no counted row


def test_result_types_and_input_order():
    c = Catalog()
    c.register("T", Table.from_pylist(SEVEN, SCHEMA))
    casts = ["CAST(v AS int)", "CAST(v AS long)", "v", "CAST(v AS decimal(10,2))", "CAST(v AS decimal(30,4))"]
    cols = [f"percentile_approx({e}, 0.5) OVER (PARTITION BY k) AS a{i}" for i, e in enumerate(casts)]
    cols += [f"percentile({e}, 0.5) OVER (PARTITION BY k) AS e{i}" for i, e in enumerate(casts)]
    cols += ["percentile(v, array(0.5, 1)) OVER (PARTITION BY k) AS arr",
             "approx_percentile(CAST(v AS decimal(30,4)), array(0.5, 1)) OVER (PARTITION BY k) AS darr"]
    out = run_sql("SELECT id, " + ", ".join(cols) + " FROM T", c, EvalContext(now_us=0))
    assert [str(col.dtype) for col in out.columns] == (
        ["long", "int", "long", "double", "decimal(10,2)", "decimal(30,4)"] + ["double"] * 5 +
        ["array<double>", "array<decimal(30,4)>"])
    got = out.to_pylist()
    assert [r["id"] for r in got] == [1, 2, 3, 4, 5, 6, 7]
    first = got[0]                                                # partition a: 1, 2, 4
    assert [first[f"a{i}"] for i in range(5)] == [2, 2, 2.0, Decimal("2.00"), Decimal("2.0000")]
    assert [first[f"e{i}"] for i in range(5)] == [2.0] * 5
    assert first["arr"] == [2.0, 4.0] and first["darr"] == [Decimal("2.0000"), Decimal("4.0000")]


@pytest.mark.parametrize("i", sorted(ROWS_GRID))
def test_rows_frames_vs_oracle(i):
    for window in ROWS_GRID[i]:
        _check_window("cpu", CPU_ROWS, window, "cpu")


@pytest.mark.parametrize("which", sorted(OTHER_WINDOWS) + ["running"])
def test_other_frames_vs_oracle(which):
    _check_window("cpu", CPU_ROWS, RUNNING if which == "running" else OTHER_WINDOWS[which], "cpu")


def test_typed_arguments_vs_oracle():
    """int / long (the cast truncates) and decimal(10,2) / decimal(30,4) (quarters are exact) arguments: the
    approximate form returns the argument's own values, the exact form interpolates their doubles."""
    spec, order, frame = ("PARTITION BY k ORDER BY id ROWS BETWEEN 6 PRECEDING AND 2 FOLLOWING", "id",
                          _rows_frame(-6, 2))
    kinds = [("int", math.trunc), ("long", math.trunc), ("decimal(10,2)", lambda v: v),
             ("decimal(30,4)", lambda v: v)]
    cols = []
    for j, (t, _) in enumerate(kinds):
        cols += [f"percentile_approx(CAST(v AS {t}), 0.75) OVER ({spec}) AS a{j}",
                 f"percentile(CAST(v AS {t}), array(0.25, 0.5)) OVER ({spec}) AS e{j}"]
    got = {r["id"]: r for r in _run(CPU_ROWS, "SELECT id, " + ", ".join(cols) + " FROM T")}
    for g, keys in _sorted_partitions(CPU_ROWS, order):
        for p, r in enumerate(g):
            lo, hi = frame(keys, p)
            for j, (t, cast) in enumerate(kinds):
                v = _ascending([float(cast(q["v"])) for q in g[lo:hi + 1] if q["v"] is not None])
                row = got[r["id"]]
                assert _same(row[f"a{j}"], _approx(v, 0.75)), (t, r["id"], row[f"a{j}"])
                if row[f"a{j}"] is not None:
                    assert isinstance(row[f"a{j}"], Decimal if t.startswith("decimal") else int), (t, row[f"a{j}"])
                assert all(_same(x, _exact(v, q)) for x, q in zip(row[f"e{j}"], (0.25, 0.5))), (t, r["id"], row)


def test_all_null_and_empty_frames_are_null():
    rows = [dict(r, v=None if r["k"] == "q" else r["v"]) for r in CPU_ROWS]
    calls = [CALLS[0], CALLS[1], CALLS[4], CALLS[2]]
    got = {r["id"]: r for r in _run(rows, _statement(OTHER_WINDOWS["whole"][0], calls))}
    for r in rows:
        if r["k"] == "q":                                   # an all-NULL partition; an array holds NULL elements
            assert [got[r["id"]][f"f{i}"] for i in range(4)] == [None, None, None, [None] * 5]
    got = {r["id"]: r for r in _run(CPU_ROWS, _statement(OTHER_WINDOWS["empty_near_end"][0], calls))}
    for g, _ in _sorted_partitions(CPU_ROWS, "id"):
        for r in g[-3:]:                                    # no row 3 FOLLOWING: an empty frame
            assert [got[r["id"]][f"f{i}"] for i in range(4)] == [None, None, None, [None] * 5]


SPECIAL_WINDOWS = [("PARTITION BY k ORDER BY id ROWS BETWEEN CURRENT ROW AND CURRENT ROW", "id", _rows_frame(0, 0)),
                   ("PARTITION BY k ORDER BY id ROWS BETWEEN 2 PRECEDING AND 1 FOLLOWING", "id", _rows_frame(-2, 1)),
                   ("PARTITION BY k ORDER BY id ROWS BETWEEN 40 PRECEDING AND CURRENT ROW", "id", _rows_frame(-40, 0)),
                   ("PARTITION BY k", "id", _whole)]
PATHS = [pytest.param("cpu", None, id="tensor"),
         pytest.param("cuda", 0, id="tree", marks=pytest.mark.gpu),
         pytest.param("cuda", 10 ** 9, id="direct", marks=pytest.mark.gpu)]


def _pin_path(monkeypatch, direct_max):
    if direct_max is not None:
        monkeypatch.setattr(W, "FRAME_SELECT_DIRECT_MAX", direct_max)


@pytest.mark.parametrize("device,direct_max", PATHS)
def test_nan_and_infinities_order_with_nan_greatest(device, direct_max, monkeypatch):
    _pin_path(monkeypatch, direct_max)
    rows = _random_rows(200, 3, ["p", "q"], 0.1, 20)
    for i, v in ((17, NAN), (90, INF), (91, -INF), (120, NAN), (121, -0.0), (160, INF)):
        rows[i]["v"] = v
    rows[17]["k"], rows[91]["k"], rows[120]["k"] = "p", "p", "q"                 # a NaN in both, −inf in p
    rows[150]["k"], rows[150]["v"] = "lone", NAN                                 # a one-row partition
    for n, window in enumerate(SPECIAL_WINDOWS):
        _check_window(f"special{n}", rows, window, device)
    got = _run(rows, "SELECT id, k, percentile_approx(v, 0.0) OVER (PARTITION BY k) AS lo, percentile_approx(v, 1.0) "
                     "OVER (PARTITION BY k) AS hi, percentile_approx(v, 1.0) OVER (PARTITION BY k ORDER BY id ROWS "
                     "BETWEEN CURRENT ROW AND CURRENT ROW) AS own FROM T", device)
    for r in got:
        assert math.isnan(r["hi"]), r                        # both big partitions hold a NaN, "lone" is one
        if r["k"] == "lone":
            assert math.isnan(r["lo"])
        elif r["k"] == "p":
            assert r["lo"] == -INF
    by = {r["id"]: r for r in got}
    assert by[90]["own"] == INF and by[91]["own"] == -INF and math.isnan(by[17]["own"])


def test_window_equals_group_by():
    """One whole-partition window and GROUP BY's percentile over the same rows agree under ``==``."""
    calls = ["percentile(v, 0.5)", "percentile(v, 0.01)", "median(v)", "percentile(v, array(0.25, 0.9, 1))",
             "percentile_approx(v, 0.9)", "approx_percentile(v, array(0, 0.33, 0.99), 100)",
             "percentile_approx(CAST(v AS decimal(30,4)), 0.75)", "percentile(CAST(v AS decimal(10,2)), 0.3)",
             "percentile_approx(CAST(v AS int), 0.5)"]
    rows = [dict(r, v=None if r["k"] == "r" else r["v"]) for r in CPU_ROWS]      # one group has no counted row
    grouped = _run(rows, "SELECT k, " + ", ".join(f"{c} AS f{i}" for i, c in enumerate(calls)) + " FROM T GROUP BY k")
    by_key = {r["k"]: r for r in grouped}
    assert len(by_key) == 4
    windowed = _run(rows, "SELECT k, " + ", ".join(f"{c} OVER (PARTITION BY k) AS f{i}" for i, c in enumerate(calls))
                    + " FROM T")
    assert len(windowed) == len(rows)
    for r in windowed:
        assert r == by_key[r["k"]], (r, by_key[r["k"]])
    assert by_key["r"]["f0"] is None and by_key["p"]["f0"] is not None


@pytest.mark.parametrize("sql,message", [
    ("SELECT percentile(k, 0.5) OVER (PARTITION BY k) AS x FROM T", "percentile OVER needs a numeric argument"),
    ("SELECT median(k) OVER () AS x FROM T", "median OVER needs a numeric argument"),
    ("SELECT percentile_approx(k, 0.5) OVER () AS x FROM T", "percentile_approx OVER needs a numeric argument"),
    ("SELECT percentile(v) OVER () AS x FROM T", "wrong number of arguments to percentile"),
    ("SELECT percentile(v, 0.5, 2) OVER () AS x FROM T", "wrong number of arguments to percentile"),
    ("SELECT median(v, 0.5) OVER () AS x FROM T", "wrong number of arguments to median"),
    ("SELECT percentile_approx(v) OVER () AS x FROM T", "wrong number of arguments to percentile_approx"),
    ("SELECT approx_percentile(v, 0.5, 100, 1) OVER () AS x FROM T", "wrong number of arguments to approx_percentile"),
    ("SELECT percentile(v, id * 0.1) OVER () AS x FROM T", "percentile percentage must be a constant"),
    ("SELECT percentile(v, array(0.5, id * 0.1)) OVER () AS x FROM T", "percentile percentage must be a constant"),
    ("SELECT percentile_approx(v, 0.5, id) OVER () AS x FROM T", "percentile_approx accuracy must be a constant"),
    ("SELECT percentile(v, 1.5) OVER () AS x FROM T", r"percentile must be in \[0, 1\]"),
    ("SELECT percentile_approx(v, array(0.5, -0.1)) OVER () AS x FROM T", r"percentile must be in \[0, 1\]"),
    ("SELECT percentile(DISTINCT v, 0.5) OVER (PARTITION BY k) AS x FROM T",
     "DISTINCT is not supported in window aggregates"),
])
def test_refusals(sql, message):
    with pytest.raises(QueryError, match=message):
        _run(SEVEN, sql)


@pytest.mark.parametrize("device", DEVICES)
def test_more_ranks_than_one_call_takes(device):
    """Nine percentages of the exact form are 18 ranks: more than one call of an entry point takes."""
    ps = (0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0)
    call = (f"percentile(v, array({', '.join(map(str, ps))}))", True, ps, True)
    spec, order, frame = OTHER_WINDOWS["whole"]
    got = {r["id"]: r["f0"] for r in _run(CPU_ROWS, _statement(spec, [call]), device)}
    for g, keys in _sorted_partitions(CPU_ROWS, order):
        want = _expected([q["v"] for q in g if q["v"] is not None], [call])[0]
        for r in g:
            # pos − lo is a multiple of 1/8 and the values of 1/4: every product is exact
            _check(got[r["id"]], want, call, r["id"])


# -- the selection primitive on hand-built frames ---------------------------------------------------------------------

def _hand_frames(n):
    """Single rows, length 2, even and odd lengths, the whole array, frames hanging over both ends, a > b."""
    mid = n // 2
    fr = [(0, 0), (n - 1, n - 1), (mid, mid), (0, 1), (n - 2, n - 1), (mid, mid + 1), (0, n - 1), (-4, n + 3),
          (-5, 1), (-2, -1), (n - 2, n + 6), (n, n + 2), (3, 2), (n - 1, 0), (1, 0)]
    for length in (3, 4, 5, 6, 7, 8, 9, 16, 17, 33, 64, 65, 129, 256):
        if length <= n:
            fr += [(0, length - 1), (n - length, n - 1), ((n - length) // 2, (n - length) // 2 + length - 1)]
    return fr


def _signed(word):
    return word - (1 << 64) if word >= (1 << 63) else word


def _select(impl, key, valid, a, b, ranks, cache):
    """The position tensors of one implementation, on the host; the wavelet matrix is built once per ``cache``."""
    vz = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(valid.to(torch.int64), 0)])
    if impl == "tensor":
        if "tree" not in cache:
            cache["tree"] = W._wavelet_build_tensor(key, valid)
        return W._frame_select_tensor(key, valid, vz, a, b, ranks, cache["tree"])
    dev = torch.device("cuda:0")
    key, valid, vz, a, b = (t.to(dev) for t in (key, valid, vz, a, b))
    ranks = [k.to(dev) for k in ranks]
    if impl == "direct":
        out = W._frame_select_direct(key, valid, a, b, ranks)
    else:
        if "tree" not in cache:
            cache["tree"] = W._wavelet_build(key, valid)
        out = W._frame_select_tree(cache["tree"], vz, a, b, ranks)
    return [o.cpu() for o in out]


IMPLS = ["tensor", pytest.param("direct", marks=pytest.mark.gpu), pytest.param("tree", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("keys", ["ties", "sign_bit"])
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 70, 300])
def test_positions_on_hand_built_frames(impl, keys, n):
    """8 and 9 straddle a level-count change, 70 and 300 are no powers of two, 300 is more than one workgroup.  The
    primitive answers one frame per row, so the frames go through it n at a time."""
    rnd = random.Random(n)
    if keys == "ties":
        words = [rnd.randrange(6) for _ in range(n)]
    else:                                                     # unsigned order: a set top bit is large, not negative
        words = [rnd.randrange(1 << 62) | ((1 << 63) if rnd.random() < 0.5 else 0) for _ in range(n)]
    key = torch.tensor([_signed(w) for w in words], dtype=torch.int64)
    frames = _hand_frames(n)
    frames += [(1, 0)] * (-len(frames) % n)
    for counted in ("all", "some", "none"):
        ok = [counted == "all" or (counted == "some" and rnd.random() < 0.7) for _ in range(n)]
        valid = torch.tensor(ok, dtype=torch.bool)
        cache = {}
        for s in range(0, len(frames), n):
            batch = frames[s:s + n]
            order = [sorted((words[j], j) for j in range(max(lo, 0), min(hi, n - 1) + 1) if ok[j]) if lo <= hi else []
                     for lo, hi in batch]
            ranks = [[0] * n, [len(o) - 1 for o in order], [len(o) for o in order], [-1] * n,
                     [len(o) // 2 for o in order]]
            a = torch.tensor([f[0] for f in batch], dtype=torch.int64)
            b = torch.tensor([f[1] for f in batch], dtype=torch.int64)
            got = _select(impl, key, valid, a, b, [torch.tensor(k, dtype=torch.int64) for k in ranks], cache)
            assert len(got) == len(ranks)
            for t, k in enumerate(ranks):
                want = [o[r][1] if 0 <= r < len(o) else -1 for o, r in zip(order, k)]
                assert got[t].tolist() == want, (counted, t, batch, k)


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments(gpu):
    from dxa.ops import native as N
    n = 4
    key = torch.zeros(n, dtype=torch.int64, device=gpu)
    ok = torch.ones(n, dtype=torch.uint8, device=gpu)
    a = torch.zeros(n, dtype=torch.int64, device=gpu)
    vz = torch.arange(n + 1, dtype=torch.int64, device=gpu)
    perm = torch.arange(n, dtype=torch.int64, device=gpu)
    ranks = torch.zeros((16, n), dtype=torch.int64, device=gpu)
    Z = torch.zeros((2, n + 1), dtype=torch.int32, device=gpu)
    out = torch.zeros((16, n), dtype=torch.int64, device=gpu)
    cur = torch.zeros(n, dtype=torch.int32, device=gpu)
    nxt = torch.zeros(n, dtype=torch.int32, device=gpu)
    flags = torch.zeros(n, dtype=torch.int32, device=gpu)
    st = N.stream_handle(gpu)
    p = N.ptr
    big = 1 << 31
    # (key, valid, a, b, n, ranks, m, out)
    bad_direct = [(0, p(ok), p(a), p(a), n, p(ranks), 1, p(out)), (p(key), p(ok), 0, p(a), n, p(ranks), 1, p(out)),
                  (p(key), p(ok), p(a), 0, n, p(ranks), 1, p(out)), (p(key), p(ok), p(a), p(a), n, 0, 1, p(out)),
                  (p(key), p(ok), p(a), p(a), n, p(ranks), 1, 0), (p(key), p(ok), p(a), p(a), -1, p(ranks), 1, p(out)),
                  (p(key), p(ok), p(a), p(a), big, p(ranks), 1, p(out)),
                  (p(key), p(ok), p(a), p(a), n, p(ranks), 0, p(out)),
                  (p(key), p(ok), p(a), p(a), n, p(ranks), 17, p(out))]
    for args in bad_direct:
        with pytest.raises(N.NativeError):
            N.call("dxa_frame_select_direct", *args, st)
    # (Z, perm, vcum, a, b, n, levels, ranks, m, out); n = 4 has two levels
    good = [p(Z), p(perm), p(vz), p(a), p(a), n, 2, p(ranks), 1, p(out)]
    bad_tree = []
    for slot, value in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (7, 0), (9, 0), (5, -1), (5, big), (8, 0), (8, 17),
                        (6, 1), (6, 3), (6, 0), (6, -2)):
        args = list(good)
        args[slot] = value
        bad_tree.append(args)
    for args in bad_tree:
        with pytest.raises(N.NativeError):
            N.call("dxa_frame_select_tree", *args, st)
    # (cur, Zl, n, bit, nxt, next_flags)
    bad_level = [(0, p(Z), n, 1, p(nxt), p(flags)), (p(cur), 0, n, 1, p(nxt), p(flags)),
                 (p(cur), p(Z), n, 1, 0, p(flags)), (p(cur), p(Z), n, 1, p(nxt), 0),
                 (p(cur), p(Z), -1, 1, p(nxt), p(flags)), (p(cur), p(Z), big, 1, p(nxt), p(flags)),
                 (p(cur), p(Z), n, 0, p(nxt), p(flags)), (p(cur), p(Z), n, 31, p(nxt), p(flags))]
    for args in bad_level:
        with pytest.raises(N.NativeError):
            N.call("dxa_wavelet_level", *args, st)
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0 and int(nxt.abs().sum()) == 0 and int(flags.abs().sum()) == 0
    # the same buffers, accepted: every frame is row 0 alone, rank 0 → position 0 (a refused call launched nothing,
    # an accepted one writes)
    out.fill_(-7)
    N.call("dxa_frame_select_direct", p(key), p(ok), p(a), p(a), n, p(ranks), 1, p(out), st)
    assert out[0].tolist() == [0] * n and out[1].tolist() == [-7] * n


# -- GPU: every window group through both entry points ----------------------------------------------------------------

def _gpu_rows():
    rows = _random_rows(3000, 21, ["p", "q", "r", "s", "t", None], 0.1, 50)      # 12 workgroups, ~500-row partitions
    rows[1234]["k"] = "lone"                                                     # a single-row partition
    return rows


GPU_ROWS = _gpu_rows()
GPU_GROUPS = {**{f"rows{i}": ROWS_GRID[i] for i in ROWS_GRID},
              "ordered": [OTHER_WINDOWS[w] for w in ("peers", "range_asc", "range_desc", "empty_near_end")],
              "long": [RUNNING, OTHER_WINDOWS["whole"]]}


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GPU_GROUPS))
@pytest.mark.parametrize("path", ["tree", "direct"])
def test_gpu_entry_points_vs_oracle(gpu, monkeypatch, path, group):
    from launch_count import count_launches
    monkeypatch.setattr(W, "FRAME_SELECT_DIRECT_MAX", 0 if path == "tree" else 10 ** 9)
    for window in GPU_GROUPS[group]:
        with count_launches() as log:
            _check_window("gpu", GPU_ROWS, window, "cuda")
        used = [e for e in log if e in SELECT_ENTRIES]
        assert used == [f"dxa_frame_select_{path}"] * len(CALLS), (window[0], used)      # once per window call


@pytest.mark.gpu
def test_gpu_path_choice_follows_the_bound(gpu):
    """Unpatched: a frame of FRAME_SELECT_DIRECT_MAX rows takes the direct entry, one row more the tree entry."""
    from launch_count import count_launches
    short = f"PARTITION BY k ORDER BY id ROWS BETWEEN {W.FRAME_SELECT_DIRECT_MAX - 1} PRECEDING AND CURRENT ROW"
    longer = f"PARTITION BY k ORDER BY id ROWS BETWEEN {W.FRAME_SELECT_DIRECT_MAX} PRECEDING AND CURRENT ROW"
    for spec, entry in ((short, "direct"), (longer, "tree")):
        with count_launches() as log:
            _run(GPU_ROWS, f"SELECT id, percentile(v, 0.5) OVER ({spec}) AS x FROM T", "cuda")
        assert [e for e in log if e in SELECT_ENTRIES] == [f"dxa_frame_select_{entry}"]
