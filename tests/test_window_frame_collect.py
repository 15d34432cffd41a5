"""``collect_list(x) OVER (…)`` and ``collect_set(x) OVER (…)``: the frame's counted (non-NULL) values as an array that
is never NULL — empty for an empty frame and for a frame with no counted row.  Elements stand in the frame's sorted order
(rows that tie on the ORDER BY keep their input order); the set keeps every value's first row inside the frame, by
GROUP BY's equality: every NaN is one value, -0.0 and 0.0 are one value.

The oracle is written here and holds no engine code: a plain Python loop over the sorted partitions, with the frame
arithmetic written out.  ``_same`` compares element for element: NaN equals NaN, a zero keeps its sign.

On the GPU every case runs through collect.hip's ``dxa_frame_collect`` and must equal the CPU result.  The entry point
has one launch shape, one thread per row: the wave-per-row shape was never faster where it was measured and was left
out (profiles/collect/README.md), so there is no ``FRAME_COLLECT_WAVE_MIN`` to patch.  The frame lengths around a
wave's 64 lanes stay as cases.
"""
import bisect
import decimal
import math
import random

import pytest

from dxa.engine import windowfn as W
from dxa.engine.column import Table
from dxa.engine.expr import EvalContext
from dxa.engine.query import Catalog, QueryError, run_sql
from dxa.engine.types import StructField, StructType

SCHEMA = StructType((StructField("id", "long"), StructField("k", "string"), StructField("t", "long"),
                     StructField("ts", "timestamp"), StructField("v", "double"), StructField("s", "string"),
                     StructField("m", "long")))
NAN = float("nan")
INF = float("inf")
SECOND = 1_000_000


def _run(rows, sql, device="cpu"):
    c = Catalog()
    c.register("T", Table.from_pylist(rows, SCHEMA, device))
    return run_sql(sql, c, EvalContext(now_us=0)).to_pylist()


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float):
        if math.isnan(a) or math.isnan(b):
            return math.isnan(a) and math.isnan(b)
        return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return type(a) is type(b) and a == b


# -- the oracle -------------------------------------------------------------------------------------------------------

def _one(v):
    """A value as a set member: every NaN is one value; -0.0 == 0.0 already holds."""
    return "NaN" if isinstance(v, float) and math.isnan(v) else v


def _dec(r):
    return None if r["m"] is None else decimal.Decimal(r["m"])


# A call is (sql, the row's value or None, set?).
CALLS = [("collect_list(v)", lambda r: r["v"], False),
         ("collect_set(v)", lambda r: r["v"], True),
         ("collect_list(s)", lambda r: r["s"], False),
         ("collect_set(s)", lambda r: r["s"], True),
         ("collect_list(CAST(m AS decimal(30,4)))", _dec, False),
         ("collect_set(CAST(m AS decimal(30,4)))", _dec, True),
         ("collect_set(m)", lambda r: r["m"], True)]


def _collect(values, as_set):
    out, seen = [], set()
    for v in values:
        if v is None or (as_set and _one(v) in seen):
            continue
        seen.add(_one(v))
        out.append(v)
    return out


def _sorted_partitions(rows, order, partitioned):
    def axis(r):
        if order == "id":
            return r["id"]
        if order == "ts":
            return r["ts"]
        if order == "t":                                      # ASC NULLS FIRST
            return -INF if r["t"] is None else r["t"]
        return INF if r["t"] is None else -r["t"]             # "t_desc": DESC NULLS LAST, axis negated
    parts = {}
    for r in rows:
        parts.setdefault(r["k"] if partitioned else 0, []).append(r)
    out = []
    for g in parts.values():
        g = sorted(g, key=lambda r: (axis(r), r["id"]))       # ties keep input order: ids ascend with the input
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


def _peers(keys, p):
    return bisect.bisect_left(keys, keys[p]), bisect.bisect_right(keys, keys[p]) - 1


def _whole(keys, p):
    return 0, len(keys) - 1


BIG = 10 ** 9
# A window is (sql, order, frame, partitioned).
WINDOWS = {
    "rows_0_0": ("PARTITION BY k ORDER BY id ROWS BETWEEN CURRENT ROW AND CURRENT ROW", "id", _rows_frame(0, 0), True),
    "rows_1_0": ("PARTITION BY k ORDER BY id ROWS BETWEEN 1 PRECEDING AND CURRENT ROW", "id", _rows_frame(-1, 0), True),
    "rows_2_3": ("PARTITION BY k ORDER BY id ROWS BETWEEN 2 PRECEDING AND 3 FOLLOWING", "id", _rows_frame(-2, 3), True),
    "rows_0_2": ("PARTITION BY k ORDER BY t ROWS BETWEEN CURRENT ROW AND 2 FOLLOWING", "t", _rows_frame(0, 2), True),
    "wide": ("PARTITION BY k ORDER BY id ROWS BETWEEN 40 PRECEDING AND 25 FOLLOWING", "id", _rows_frame(-40, 25), True),
    "running": ("PARTITION BY k ORDER BY id ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW", "id",
                _rows_frame(-BIG, 0), True),
    "rest": ("PARTITION BY k ORDER BY id ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING", "id",
             _rows_frame(0, BIG), True),
    "empty_near_end": ("PARTITION BY k ORDER BY id ROWS BETWEEN 2 FOLLOWING AND 3 FOLLOWING", "id", _rows_frame(2, 3),
                       True),
    "empty_near_start": ("PARTITION BY k ORDER BY id ROWS BETWEEN 3 PRECEDING AND 2 PRECEDING", "id",
                         _rows_frame(-3, -2), True),
    "default": ("PARTITION BY k ORDER BY t", "t", _running_peers, True),
    "whole": ("PARTITION BY k", "id", _whole, True),
    "peers": ("PARTITION BY k ORDER BY t RANGE BETWEEN CURRENT ROW AND CURRENT ROW", "t", _peers, True),
    "range_asc": ("PARTITION BY k ORDER BY t RANGE BETWEEN 3 PRECEDING AND 2 FOLLOWING", "t", _range_frame(-3, 2),
                  True),
    "range_desc": ("PARTITION BY k ORDER BY t DESC RANGE BETWEEN 3 PRECEDING AND 2 FOLLOWING", "t_desc",
                   _range_frame(-3, 2), True),
    "range_interval": ("PARTITION BY k ORDER BY ts RANGE BETWEEN INTERVAL 3 SECONDS PRECEDING AND INTERVAL 1 SECOND "
                       "FOLLOWING", "ts", _range_frame(-3 * SECOND, SECOND), True),
    "no_partition": ("ORDER BY id ROWS BETWEEN 5 PRECEDING AND 1 FOLLOWING", "id", _rows_frame(-5, 1), False),
    "no_partition_default": ("ORDER BY t", "t", _running_peers, False),
}


def _statement(spec, calls=CALLS):
    return "SELECT id, " + ", ".join(f"{c[0]} OVER ({spec}) AS f{i}" for i, c in enumerate(calls)) + " FROM T"


def _oracle(rows, window, calls=CALLS):
    _, order, frame, partitioned = window
    out = {}
    for part, keys in _sorted_partitions(rows, order, partitioned):
        for p, r in enumerate(part):
            lo, hi = frame(keys, p)
            inside = part[lo:hi + 1] if lo <= hi else []
            out[r["id"]] = {f"f{i}": _collect([val(x) for x in inside], as_set)
                            for i, (_, val, as_set) in enumerate(calls)}
    return out


def _table(n, seed, partitions=("a", "b", "", None)):
    """Seeded rows: partitions of different sizes — "solo" has one row — NULL order keys, peers, NULL arguments,
    NaN, both zeros, empty and multi-byte strings."""
    r = random.Random(seed)
    rows = []
    for i in range(n):
        rows.append({"id": i, "k": r.choice(partitions), "t": r.choice([None, r.randrange(12)]),
                     "ts": r.randrange(20) * SECOND // 2,
                     "v": r.choice([None, NAN, -0.0, 0.0, 1.5, r.randrange(4) / 2]),
                     "s": r.choice([None, "", "a", "é√", "日本", str(r.randrange(3))]),
                     "m": r.choice([None, -5, 0, 7, 10 ** 15, r.randrange(4)])})
    rows.append({"id": n, "k": "solo", "t": 3, "ts": 0, "v": 2.0, "s": "x", "m": 1})
    return rows


ROWS = _table(150, 1)
_CPU = {}


def _cpu_result(rows_name, rows, window_name, calls=CALLS):
    """The CPU result of a case, computed once: compared with the oracle, and the GPU's reference."""
    key = (rows_name, window_name)
    if key not in _CPU:
        _CPU[key] = _run(rows, _statement(WINDOWS[window_name][0], calls))
    return _CPU[key]


def _check(got, want):
    assert len(got) == len(want)
    for g in got:
        for f, w in want[g["id"]].items():
            assert g[f] is not None
            assert _same(g[f], w), (g["id"], f, g[f], w)


# -- CPU --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", list(WINDOWS))
def test_matches_python_loop(window):
    _check(_cpu_result("rows", ROWS, window), _oracle(ROWS, WINDOWS[window]))


def test_one_row_partition_and_null_arguments():
    got = {g["id"]: g for g in _cpu_result("rows", ROWS, "wide")}
    assert _same(got[150]["f0"], [2.0]) and got[150]["f3"] == ["x"]
    rows = [{"id": i, "k": "p", "t": i, "ts": 0, "v": None, "s": None, "m": None} for i in range(5)]
    got = _run(rows, _statement(WINDOWS["running"][0]))
    assert all(g[f"f{i}"] == [] for g in got for i in range(len(CALLS)))


@pytest.mark.parametrize("window", ["rows_2_3", "wide", "default", "range_asc", "whole", "empty_near_end"])
def test_size_of_set_is_count_distinct(window):
    spec = WINDOWS[window][0]
    for arg in ("v", "s", "m", "CAST(m AS decimal(30,4))"):
        # count(x) OVER takes numeric arguments only: the list's size is checked against it for those
        plain = "0" if arg == "s" else f"count({arg}) OVER ({spec})"
        got = _run(ROWS, f"SELECT id, size(collect_set({arg}) OVER ({spec})) AS a, count(DISTINCT {arg}) OVER ({spec}) "
                         f"AS b, size(collect_list({arg}) OVER ({spec})) AS c, {plain} AS d FROM T")
        assert got and all(g["a"] == g["b"] and (arg == "s" or g["c"] == g["d"]) for g in got), (window, arg)


def test_zero_rows():
    t = run_sql("SELECT id, collect_list(v) OVER (PARTITION BY k ORDER BY id) AS l, collect_set(s) OVER (ORDER BY id "
                "ROWS BETWEEN 1 PRECEDING AND CURRENT ROW) AS s FROM T WHERE id < 0",
                _catalog(ROWS), EvalContext(now_us=0))
    assert t.length == 0 and t.to_pylist() == []
    assert str(t.column("l").dtype.element) == "double" and str(t.column("s").dtype.element) == "string"


def _catalog(rows, device="cpu"):
    c = Catalog()
    c.register("T", Table.from_pylist(rows, SCHEMA, device))
    return c


@pytest.mark.parametrize("call, word", [("collect_list(v, s)", "collect_list"), ("collect_set(v, s)", "collect_set"),
                                        ("collect_list()", "collect_list"),
                                        ("collect_list(DISTINCT v)", "collect_list"),
                                        ("collect_set(DISTINCT v)", "collect_set"),
                                        ("collect_list(array(v))", "collect_list"),
                                        ("collect_set(array(v, 1.0))", "collect_set")])
def test_refusals(call, word):
    with pytest.raises(QueryError) as e:                      # the statement's error, raised from the WindowError
        _run(ROWS, f"SELECT {call} OVER (PARTITION BY k ORDER BY id) AS x FROM T")
    assert isinstance(e.value.__cause__, W.WindowError) and word in str(e.value)


def test_slot_cap(monkeypatch):
    monkeypatch.setattr(W, "FRAME_COLLECT_MAX_SLOTS", 1000)
    with pytest.raises(QueryError, match="too long to collect"):
        _run(ROWS, "SELECT collect_list(m) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 40 PRECEDING AND CURRENT ROW) "
                   "AS x FROM T")
    got = _run(ROWS, "SELECT collect_list(m) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 2 PRECEDING AND CURRENT ROW) "
                     "AS x FROM T")
    assert len(got) == len(ROWS)                             # 3 slots × 151 rows fit


# -- GPU: the same cases, and frames around 64 rows, through the kernel ------------------------------------------------

def _edge_tables():
    """One partition of 200 rows and 3 partitions of 70 rows, ordered by id; ``sparse`` counts only every 64th row of
    its partition (positions 63, 127, 191): a 64-row frame ending there keeps its last lane alone."""
    r = random.Random(4)

    def row(i, k, v):
        return {"id": i, "k": k, "t": i, "ts": 0, "v": v, "s": None if v is None else str(int(v) % 5),
                "m": None if v is None else int(v) % 7}
    dense = [row(i, "p", r.choice([None, float(r.randrange(40))])) for i in range(200)]
    sparse = [row(i, "p", float(i) if i % 64 == 63 else None) for i in range(200)]
    three = [row(i, "abc"[i % 3], r.choice([None, float(r.randrange(9))])) for i in range(210)]
    return {"dense": dense, "sparse": sparse, "three": three}


EDGE_TABLES = _edge_tables()
EDGE_CALLS = [CALLS[0], CALLS[1], CALLS[3], CALLS[6]]
for _len in (1, 63, 64, 65, 129):                             # frame lengths; most frames start off a multiple of 64
    WINDOWS[f"len_{_len}"] = (f"PARTITION BY k ORDER BY id ROWS BETWEEN {_len - 1} PRECEDING AND CURRENT ROW", "id",
                              _rows_frame(1 - _len, 0), True)
WINDOWS["centred_129"] = ("PARTITION BY k ORDER BY id ROWS BETWEEN 64 PRECEDING AND 64 FOLLOWING", "id",
                          _rows_frame(-64, 64), True)
EDGE_WINDOWS = [f"len_{n}" for n in (1, 63, 64, 65, 129)] + ["centred_129", "whole"]
SQL_CASES = [w for w in WINDOWS if not w.startswith(("len_", "centred"))]


@pytest.mark.parametrize("table", list(EDGE_TABLES))
@pytest.mark.parametrize("window", EDGE_WINDOWS)
def test_edge_shapes_match_python_loop(table, window):
    rows = EDGE_TABLES[table]
    _check(_cpu_result(table, rows, window, EDGE_CALLS), _oracle(rows, WINDOWS[window], EDGE_CALLS))


@pytest.mark.gpu
@pytest.mark.parametrize("window", SQL_CASES)
def test_gpu_equals_cpu(window, gpu):
    got = _run(ROWS, _statement(WINDOWS[window][0]), "cuda")
    want = _cpu_result("rows", ROWS, window)
    assert len(got) == len(want) and all(_same(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("table", list(EDGE_TABLES))
@pytest.mark.parametrize("window", EDGE_WINDOWS)
def test_gpu_edge_shapes_equal_cpu(table, window, gpu):
    rows = EDGE_TABLES[table]
    got = _run(rows, _statement(WINDOWS[window][0], EDGE_CALLS), "cuda")
    want = _cpu_result(table, rows, window, EDGE_CALLS)
    assert len(got) == len(want) and all(_same(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
def test_gpu_takes_the_kernel_and_zero_rows(gpu, monkeypatch):
    """Both calls go through the entry point on the device, and zero rows there give the empty column."""
    from dxa.ops import native as N
    seen = []
    real = N.call

    def spy(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(N, "call", spy)
    _run(EDGE_TABLES["three"], _statement(WINDOWS["len_65"][0], EDGE_CALLS[:2]), "cuda")
    assert seen.count("dxa_frame_collect") == 2
    t = run_sql("SELECT id, collect_set(s) OVER (PARTITION BY k ORDER BY id) AS s FROM T WHERE id < 0",
                _catalog(ROWS, "cuda"), EvalContext(now_us=0))
    assert t.to_pylist() == []
