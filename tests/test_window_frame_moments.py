"""Variance and moment aggregates as window functions: stddev / std / stddev_samp / stddev_pop / variance / var_samp
/ var_pop, skewness / kurtosis and covar_pop / covar_samp / corr ``OVER (PARTITION BY … ORDER BY … frame)``.

The oracle is written here and holds no engine code.  Every frame is a contiguous range of its partition in window
order, so per partition it keeps exact integer prefix sums of the counted values' powers (the test values are
multiples of 0.25, scaled by 4) and turns a range into the frame's central sums as exact ``fractions.Fraction``s;
the finishing rules are applied to those, with the NaN conditions tested on the exact M2.  A frame that holds a
non-finite counted value is NaN outright.

Tolerances (the project's own for the same merge formulas and value ranges, tests/test_window_dense_moments.py):
doubles within max(1e-9·|want|, 1e-12); the dimensionless corr / skewness / kurtosis within 1e-9 absolute; the
1e9-offset case rel 1e-6 (abs 1e-6 for the dimensionless ones).  Values are multiples of 0.25 in [0, 64), skewed.

Largest deviations seen (every test prints its own with ``-s``; ``rel`` for doubles, ``abs`` for the dimensionless
ones; CPU runs are the tensor-operation path, GPU runs the two entry points of window_frames.hip on an MI355X):

    CPU, 300 rows: ROWS frames rel 3.4e-15 abs 1.9e-15; peers / whole / RANGE / empty-near-end rel 1.1e-15
        abs 1.8e-15; non-finite 4.1e-16 / 1.4e-15; constant partition 1.4e-15 / 1.4e-15; decimal and int arguments
        3.2e-15 / 1.8e-15; state words (n = 1 … 300) rel 1.4e-14
    GPU levels, 3,000 rows: rel 1.9e-12 (a covariance close to 0, at the 1e-12 floor) abs 2.7e-15; state words 1.4e-14
    GPU direct, 3,000 rows: rel 8.0e-15 abs 1.6e-14; state words 6.8e-15
    values + 1e9 (bounds 1e-6): levels and CPU rel 1.1e-8 abs 1.7e-8; direct rel 1.2e-14 abs 9.6e-8
"""
import bisect
import math
import random
from fractions import Fraction

import pytest
import torch

from dxa.engine import windowfn as W
from dxa.engine.column import Table
from dxa.engine.expr import EvalContext
from dxa.engine.query import Catalog, QueryError, run_sql
from dxa.engine.types import StructField, StructType

SCHEMA = StructType((StructField("id", "long"), StructField("k", "string"), StructField("t", "long"),
                     StructField("v", "double"), StructField("u", "double")))
ONE_ARG = ["stddev", "std", "stddev_samp", "stddev_pop", "variance", "var_samp", "var_pop", "skewness", "kurtosis"]
TWO_ARG = ["covar_pop", "covar_samp", "corr"]
NAMES = ONE_ARG + TWO_ARG
DIMENSIONLESS = ("corr", "skewness", "kurtosis")
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
NAN = float("nan")


def _run(rows, sql, device="cpu"):
    c = Catalog()
    c.register("T", Table.from_pylist(rows, SCHEMA, device))
    return run_sql(sql, c, EvalContext(now_us=0)).to_pylist()


# -- the oracle -------------------------------------------------------------------------------------------------------

def _scaled(x):
    """A finite test value as an exact integer count of quarters."""
    q = x * 4
    assert q == int(q), x
    return int(q)


class _Partition:
    """Exact prefix sums over one partition in window order.  ``vals[p]`` is None (row not counted), or the tuple of
    the row's argument values (one or two)."""

    def __init__(self, vals):
        self.pairs = bool(vals) and any(v is not None and len(v) == 2 for v in vals)
        width = 5 if self.pairs else 4
        self.n = [0]
        self.bad = [0]
        self.s = [[0] * width]
        for v in vals:
            n, bad, s = self.n[-1], self.bad[-1], list(self.s[-1])
            if v is not None:
                n += 1
                if not all(math.isfinite(e) for e in v):
                    bad += 1
                elif self.pairs:
                    x, y = _scaled(v[0]), _scaled(v[1])
                    for j, m in enumerate((x, y, x * x, y * y, x * y)):
                        s[j] += m
                else:
                    x = _scaled(v[0])
                    for j in range(4):
                        s[j] += x ** (j + 1)
            self.n.append(n)
            self.bad.append(bad)
            self.s.append(s)
        self._memo = {}

    def state(self, lo, hi):
        """None: no counted row; "nan": a non-finite counted value; else the exact state of rows lo..hi as a dict."""
        if lo > hi:
            return None
        key = (lo, hi)
        if key not in self._memo:
            self._memo[key] = self._state(lo, hi)
        return self._memo[key]

    def _state(self, lo, hi):
        n = self.n[hi + 1] - self.n[lo]
        if n == 0:
            return None
        if self.bad[hi + 1] - self.bad[lo]:
            return "nan"
        s = [p - q for p, q in zip(self.s[hi + 1], self.s[lo])]
        if self.pairs:
            sx, sy, sxx, syy, sxy = s
            return {"n": n, "mx": Fraction(sx, 4 * n), "my": Fraction(sy, 4 * n),
                    "cxy": Fraction(n * sxy - sx * sy, 16 * n), "m2x": Fraction(n * sxx - sx * sx, 16 * n),
                    "m2y": Fraction(n * syy - sy * sy, 16 * n)}
        s1, s2, s3, s4 = s
        return {"n": n, "mean": Fraction(s1, 4 * n), "m2": Fraction(n * s2 - s1 * s1, 16 * n),
                "m3": Fraction(n * n * s3 - 3 * n * s1 * s2 + 2 * s1 ** 3, 64 * n * n),
                "m4": Fraction(n ** 3 * s4 - 4 * n * n * s1 * s3 + 6 * n * s1 * s1 * s2 - 3 * s1 ** 4, 256 * n ** 3)}


def _finish(name, st):
    """Spark's result of ``name`` from an exact state (None → NULL)."""
    if st is None:
        return None
    if st == "nan":
        return NAN
    n = st["n"]
    if name in ("stddev", "std", "stddev_samp", "variance", "var_samp"):
        if n == 1:
            return NAN
        var = float(st["m2"] / (n - 1))
        return math.sqrt(var) if name.startswith("std") else var
    if name in ("stddev_pop", "var_pop"):
        var = float(st["m2"] / n)
        return math.sqrt(var) if name.startswith("std") else var
    if name == "skewness":
        return math.sqrt(n) * float(st["m3"]) / float(st["m2"]) ** 1.5 if st["m2"] > 0 else NAN
    if name == "kurtosis":
        return float(n * st["m4"] / (st["m2"] * st["m2"]) - 3) if st["m2"] > 0 else NAN
    if name == "covar_pop":
        return float(st["cxy"] / n)
    if name == "covar_samp":
        return NAN if n == 1 else float(st["cxy"] / (n - 1))
    assert name == "corr"
    p = st["m2x"] * st["m2y"]
    return float(st["cxy"]) / math.sqrt(float(p)) if p > 0 else NAN


class _Worst:
    """Checks one result against the oracle and keeps the largest deviation seen."""

    def __init__(self, rel=1e-9, abs_=1e-12, dimensionless=1e-9):
        self.rel, self.abs, self.dimensionless = rel, abs_, dimensionless
        self.worst_rel = 0.0              # doubles: |got − want| / max(|want|, abs/rel)
        self.worst_dimensionless = 0.0    # corr / skewness / kurtosis: |got − want|
        self.checked = 0

    def check(self, name, got, want, where=""):
        self.checked += 1
        if want is None:
            assert got is None, (name, got, want, where)
            return
        assert got is not None, (name, got, want, where)
        if math.isnan(want):
            assert math.isnan(got), (name, got, want, where)
            return
        err = abs(got - want)
        if name in DIMENSIONLESS:
            self.worst_dimensionless = max(self.worst_dimensionless, err)
            assert err <= self.dimensionless, (name, got, want, where)
        else:
            self.worst_rel = max(self.worst_rel, err / max(abs(want), self.abs / self.rel))
            assert err <= max(self.rel * abs(want), self.abs), (name, got, want, where)

    def report(self, what):
        print(f"[deviation] {what}: {self.checked} results, doubles rel {self.worst_rel:.3g}, "
              f"dimensionless abs {self.worst_dimensionless:.3g}")


# -- frames in Python -------------------------------------------------------------------------------------------------
# A window is (sql, order, frame): ``order`` names how a partition is sorted, ``frame(keys, p)`` gives the inclusive
# row range of position p from the partition's ascending ordering-axis values ``keys``.

def _sorted_partitions(rows, order):
    inf = float("inf")

    def axis(r):
        if order == "id":
            return r["id"]
        if order == "t":                                      # ASC NULLS FIRST
            return -inf if r["t"] is None else r["t"]
        return inf if r["t"] is None else -r["t"]             # "t_desc": DESC NULLS LAST, axis negated
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


def _statement(spec, calls=None):
    calls = calls or [f"{f}(v)" for f in ONE_ARG] + [f"{f}(v, u)" for f in TWO_ARG]
    return "SELECT id, " + ", ".join(f"{c} OVER ({spec}) AS f{i}" for i, c in enumerate(calls)) + " FROM T"


def _check_window(rows, window, device, worst, names=NAMES, arg=lambda r: r["v"]):
    """Run all of ``names`` over one window on ``device`` and compare every row with the oracle."""
    spec, order, frame = window
    calls = [f"{f}(v)" if f in ONE_ARG else f"{f}(v, u)" for f in names]
    got = {r["id"]: r for r in _run(rows, _statement(spec, calls), device)}
    assert len(got) == len(rows)
    for g, keys in _sorted_partitions(rows, order):
        one = _Partition([None if arg(r) is None else (arg(r),) for r in g])
        two = _Partition([None if arg(r) is None or r["u"] is None else (arg(r), r["u"]) for r in g])
        for p, r in enumerate(g):
            lo, hi = frame(keys, p)
            for i, f in enumerate(names):
                st = (one if f in ONE_ARG else two).state(lo, hi)
                worst.check(f, got[r["id"]][f"f{i}"], _finish(f, st), (spec, r["id"]))


def _value(rnd):
    """A multiple of 0.25 in [0, 64), skewed towards 0 so that M3 is far from 0."""
    return int(256 * rnd.random() ** 2) / 4.0


def _random_rows(n, seed, keys, null_share, tmax):
    """``u`` depends on ``v`` (half of it plus a multiple of 0.25 below 32, NULLs of its own), as ``hum`` depends on
    ``temp`` in tests/test_window_dense_comoments.py whose tolerances these are: a covariance that cancels to almost
    nothing has no meaningful relative error."""
    rnd = random.Random(seed)
    rows = []
    for i in range(n):
        v = _value(rnd)
        u = math.floor(v * 2) * 0.25 + rnd.randrange(128) * 0.25
        rows.append({"id": i, "k": rnd.choice(keys), "t": rnd.choice([None] + list(range(tmax))),
                     "v": None if rnd.random() < null_share else v,
                     "u": None if rnd.random() < null_share else u})
    return rows


CPU_ROWS = _random_rows(300, 11, ["p", "q", "r", None], 0.15, 20)

# -- CPU: SQL surface -------------------------------------------------------------------------------------------------

SEVEN = [
    {"id": 1, "k": "a", "t": 10, "v": 1.0, "u": 1.0},
    {"id": 2, "k": "a", "t": 20, "v": 2.0, "u": 5.0},
    {"id": 3, "k": "a", "t": 20, "v": None, "u": None},
    {"id": 4, "k": "a", "t": 30, "v": 4.0, "u": None},
    {"id": 5, "k": "b", "t": 5, "v": 10.0, "u": 3.0},
    {"id": 6, "k": "b", "t": None, "v": 20.0, "u": 1.0},
    {"id": 7, "k": None, "t": 1, "v": 7.0, "u": 2.0},
]


def test_hand_computed_rows():
    got = _run(SEVEN, "SELECT id, stddev(v) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 1 PRECEDING AND CURRENT ROW) "
                      "AS sd, var_pop(v) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 1 PRECEDING AND CURRENT ROW) "
                      "AS vp, variance(v) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN CURRENT ROW AND CURRENT ROW) "
                      "AS own, corr(v, u) OVER (PARTITION BY k) AS c, covar_samp(v, u) OVER (PARTITION BY k) AS cs "
                      "FROM T ORDER BY id")
    by = {r["id"]: r for r in got}
    # partition a by id: frames {1}, {1, 2}, {2, NULL}, {NULL, 4}
    assert math.isnan(by[1]["sd"]) and by[1]["vp"] == 0.0
    assert by[2]["sd"] == pytest.approx(math.sqrt(0.5), rel=1e-15) and by[2]["vp"] == 0.25
    assert math.isnan(by[3]["sd"]) and by[3]["vp"] == 0.0
    assert math.isnan(by[4]["sd"]) and by[4]["vp"] == 0.0
    assert by[5]["vp"] == 0.0 and by[6]["sd"] == pytest.approx(math.sqrt(50.0), rel=1e-15) and by[6]["vp"] == 25.0
    # the one-row frame of a NULL holds no counted row: NULL; of a value: NaN (a sample statistic of one row)
    assert by[3]["own"] is None and math.isnan(by[2]["own"])
    # corr over partition b's two rows (10, 3), (20, 1): a falling line; partition a has two complete pairs (1, 1),
    # (2, 5): a rising one; the NULL key's single pair: NaN
    assert by[5]["c"] == pytest.approx(-1.0, abs=1e-15) and by[6]["cs"] == pytest.approx(-10.0, rel=1e-15)
    assert by[1]["c"] == pytest.approx(1.0, abs=1e-15) and by[4]["cs"] == pytest.approx(2.0, rel=1e-15)
    assert math.isnan(by[7]["c"]) and math.isnan(by[7]["cs"])


def test_result_type_is_double_and_rows_keep_input_order():
    c = Catalog()
    c.register("T", Table.from_pylist(SEVEN, SCHEMA))
    out = run_sql("SELECT id, kurtosis(t) OVER (PARTITION BY k) AS x, stddev_pop(1) OVER () AS one FROM T", c,
                  EvalContext(now_us=0))
    assert [str(col.dtype) for col in out.columns] == ["long", "double", "double"]
    got = out.to_pylist()
    assert [r["id"] for r in got] == [1, 2, 3, 4, 5, 6, 7]
    assert all(r["one"] == 0.0 for r in got)                                     # a constant argument
    # t of partition a: 10, 20, 20, 30 → M2 = 200, M4 = 20000 → 4·20000/200² − 3 = −1
    assert got[0]["x"] == pytest.approx(-1.0, abs=1e-12) and math.isnan(got[6]["x"])


@pytest.mark.parametrize("i", sorted(ROWS_GRID))
def test_rows_frames_vs_oracle(i):
    worst = _Worst()
    for window in ROWS_GRID[i]:
        _check_window(CPU_ROWS, window, "cpu", worst)
    worst.report(f"cpu rows frames {i} PRECEDING")


@pytest.mark.parametrize("which", sorted(OTHER_WINDOWS))
def test_other_frames_vs_oracle(which):
    worst = _Worst()
    _check_window(CPU_ROWS, OTHER_WINDOWS[which], "cpu", worst)
    worst.report(f"cpu {which}")


def test_empty_frames_are_null():
    got = _run(CPU_ROWS, _statement(OTHER_WINDOWS["empty_near_end"][0]))
    by = {r["id"]: r for r in got}
    for g, _ in _sorted_partitions(CPU_ROWS, "id"):
        for r in g[-3:]:                                     # no row 3 FOLLOWING: an empty frame
            assert all(by[r["id"]][f"f{i}"] is None for i in range(len(NAMES)))


@pytest.mark.parametrize("sql,message", [
    ("SELECT stddev(k) OVER (PARTITION BY k) AS x FROM T", "stddev OVER needs a numeric argument"),
    ("SELECT corr(v, k) OVER () AS x FROM T", "corr OVER needs a numeric argument"),
    ("SELECT stddev(DISTINCT v) OVER (PARTITION BY k) AS x FROM T", "DISTINCT is not supported in window aggregates"),
    ("SELECT corr(v) OVER () AS x FROM T", "wrong number of arguments to corr"),
    ("SELECT stddev(v, v) OVER () AS x FROM T", "wrong number of arguments to stddev"),
])
def test_refusals(sql, message):
    with pytest.raises(QueryError, match=message):
        _run(SEVEN, sql)


# -- special values, CPU (tensor operations) and GPU (both entry points) ----------------------------------------------

PATHS = [pytest.param("cpu", None, id="tensor"),
         pytest.param("cuda", 0, id="levels", marks=pytest.mark.gpu),
         pytest.param("cuda", 10 ** 9, id="direct", marks=pytest.mark.gpu)]


def _pin_path(monkeypatch, direct_max):
    if direct_max is not None:
        monkeypatch.setattr(W, "FRAME_DIRECT_MAX", direct_max)


SPECIAL_WINDOWS = [("PARTITION BY k ORDER BY id ROWS BETWEEN CURRENT ROW AND CURRENT ROW", "id", _rows_frame(0, 0)),
                   ("PARTITION BY k ORDER BY id ROWS BETWEEN 2 PRECEDING AND 1 FOLLOWING", "id", _rows_frame(-2, 1)),
                   ("PARTITION BY k ORDER BY id ROWS BETWEEN 40 PRECEDING AND CURRENT ROW", "id", _rows_frame(-40, 0)),
                   ("PARTITION BY k", "id", _whole)]


@pytest.mark.parametrize("device,direct_max", PATHS)
def test_non_finite_values_give_nan(device, direct_max, monkeypatch):
    _pin_path(monkeypatch, direct_max)
    rows = _random_rows(200, 3, ["p", "q"], 0.1, 20)
    rows[17]["v"] = NAN
    rows[90]["v"] = float("inf")
    rows[91]["u"] = float("-inf")
    rows[150]["k"], rows[150]["v"], rows[150]["u"] = "lone", float("inf"), 1.0       # a one-row partition
    worst = _Worst()
    for window in SPECIAL_WINDOWS:
        _check_window(rows, window, device, worst)
    got = {r["id"]: r for r in _run(rows, _statement(SPECIAL_WINDOWS[0][0]), device)}
    assert all(math.isnan(got[i][f"f{j}"]) for i in (17, 90, 150) for j in range(len(ONE_ARG)))
    assert all(math.isnan(got[150][f"f{j}"]) for j in range(len(NAMES)))
    worst.report(f"non-finite values {device} direct_max={direct_max}")


@pytest.mark.parametrize("device,direct_max", PATHS)
def test_constant_partition_has_zero_m2(device, direct_max, monkeypatch):
    _pin_path(monkeypatch, direct_max)
    rows = [{"id": i, "k": "c" if i % 3 else "d", "t": i, "v": 2.5 if i % 3 else _value(random.Random(i)),
             "u": 7.25 if i % 3 else float(i % 7)} for i in range(150)]
    worst = _Worst()
    for window in SPECIAL_WINDOWS:
        _check_window(rows, window, device, worst)
    got = _run(rows, "SELECT id, k, corr(v, u) OVER (PARTITION BY k) AS c, skewness(v) OVER (PARTITION BY k) AS s, "
                     "kurtosis(v) OVER (PARTITION BY k ORDER BY id) AS ku, var_pop(v) OVER (PARTITION BY k) AS vp, "
                     "covar_pop(v, u) OVER (PARTITION BY k ORDER BY id) AS cp FROM T", device)
    for r in got:
        if r["k"] == "c":
            assert math.isnan(r["c"]) and math.isnan(r["s"]) and math.isnan(r["ku"]), r
            assert r["vp"] == 0.0 and r["cp"] == 0.0, r
    worst.report(f"constant partition {device} direct_max={direct_max}")


@pytest.mark.parametrize("device,direct_max", PATHS)
def test_offset_values_keep_their_digits(device, direct_max, monkeypatch):
    """Values 1e9 + multiples of 0.25 with a spread of 64: Σx² − (Σx)²/n would be wrong in the leading digits.

    Near 1e9 a double's ulp is 1.2e-7, so the mean of a run is stored to about 6e-8 and a merge's δ-terms carry a
    relative error of about 1.2e-7 / δ.  The values are therefore uniform over the whole spread (a frame of values
    0.25 apart would sit at the 1e-6 bound by the number format alone), and ``u`` falls as ``v`` rises, so that no
    covariance cancels to almost nothing."""
    _pin_path(monkeypatch, direct_max)
    rnd = random.Random(5)
    rows = []
    for i in range(1500):
        v = rnd.randrange(256) * 0.25
        rows.append({"id": i, "k": rnd.choice(["p", "q", None]), "t": None,
                     "v": None if rnd.random() < 0.1 else 1e9 + v,
                     "u": None if rnd.random() < 0.1 else 1e9 + 63.75 - v + 0.25 * rnd.randrange(2)})
    worst = _Worst(rel=1e-6, abs_=1e-12, dimensionless=1e-6)
    for window in (ROWS_GRID[4][0], ("PARTITION BY k ORDER BY id ROWS BETWEEN 9 PRECEDING AND CURRENT ROW", "id",
                                     _rows_frame(-9, 0)), RUNNING, OTHER_WINDOWS["whole"]):
        _check_window(rows, window, device, worst)
    worst.report(f"offset 1e9 {device} direct_max={direct_max}")


@pytest.mark.parametrize("device,direct_max", PATHS)
def test_decimal_and_int_arguments(device, direct_max, monkeypatch):
    """decimal(10,2) and int arguments give the doubles their cast gives: the quarters are exact at scale 2, the int
    cast truncates."""
    _pin_path(monkeypatch, direct_max)
    rows = _random_rows(300, 9, ["p", "q", None], 0.1, 20)
    spec, order, frame = ("PARTITION BY k ORDER BY id ROWS BETWEEN 6 PRECEDING AND 2 FOLLOWING", "id",
                          _rows_frame(-6, 2))
    calls = ["stddev(CAST(v AS decimal(10,2)))", "kurtosis(CAST(v AS decimal(10,2)))",
             "corr(CAST(v AS decimal(10,2)), u)", "var_samp(CAST(v AS int))", "skewness(CAST(v AS int))",
             "covar_pop(CAST(v AS int), u)"]
    names = ["stddev", "kurtosis", "corr", "var_samp", "skewness", "covar_pop"]
    got = {r["id"]: r for r in _run(rows, _statement(spec, calls), device)}
    worst = _Worst()
    for g, keys in _sorted_partitions(rows, order):
        for cast, cols in ((lambda v: v, (0, 1, 2)), (lambda v: float(int(v)), (3, 4, 5))):
            one = _Partition([None if r["v"] is None else (cast(r["v"]),) for r in g])
            two = _Partition([None if r["v"] is None or r["u"] is None else (cast(r["v"]), r["u"]) for r in g])
            for p, r in enumerate(g):
                lo, hi = frame(keys, p)
                for c in cols:
                    st = (two if names[c] in TWO_ARG else one).state(lo, hi)
                    worst.check(names[c], got[r["id"]][f"f{c}"], _finish(names[c], st), (calls[c], r["id"]))
    worst.report(f"decimal / int arguments {device} direct_max={direct_max}")


# -- hand-built frames: the state words of the tensor path and of the two entry points --------------------------------

def _hand_frames(n):
    """n frames over n rows: lengths 2^k − 1, 2^k, 2^k + 1, a frame ending at row n − 1, empty frames (a > b),
    bounds outside [0, n) and the whole range."""
    fr = []
    k = 1
    while 2 ** k + 1 <= n:
        for length in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            fr.append((0, length - 1))
            fr.append((n - length, n - 1))                   # ends at the last row
            fr.append(((n - length) // 2, (n - length) // 2 + length - 1))
        k += 1
    fr = [(0, n - 1)] + fr + [(0, 0), (n - 1, n - 1), (3, 2), (n - 1, 0), (n, n + 4), (-7, -2), (-3, n + 5), (-2, 1),
           (n - 2, n + 9)]
    assert len(fr) <= n or n < 8
    fr = fr[:n]
    return fr + [(1, 0)] * (n - len(fr))


def _clip(lo, hi, n):
    if lo > hi:
        return 1, 0
    return max(lo, 0), min(hi, n - 1)


def _state_words(kind, st):
    words = W.STATE_WORDS[kind]
    if st is None:
        return [0.0] * words
    if st == "nan":
        return None
    order = {W.KIND_VAR: ("n", "mean", "m2"), W.KIND_MOM: ("n", "mean", "m2", "m3", "m4"),
             W.KIND_CO: ("n", "mx", "my", "cxy", "m2x", "m2y")}[kind]
    return [float(st[w]) for w in order]


def _states(impl, kind, x, y, valid, a, b, maxlen):
    """The [words, n] state tensor of one implementation, on the host."""
    if impl == "tensor":
        return W._frame_state_tensor(kind, x, y, valid, a, b, maxlen)
    from dxa.ops import native as N
    dev = torch.device("cuda:0")
    x, a, b = x.to(dev), a.to(dev), b.to(dev)
    y = None if y is None else y.to(dev)
    v = None if valid is None else valid.to(dev).view(torch.uint8)
    n = int(x.shape[0])
    words = W.STATE_WORDS[kind]
    out = torch.full((words, n), -12345.0, dtype=torch.float64, device=dev)
    st = N.stream_handle(dev)
    if impl == "direct":
        N.call("dxa_frame_moments_direct", N.ptr(x), N.ptr(y), N.ptr(v), N.ptr(a), N.ptr(b), n, kind, N.ptr(out), st)
    else:
        scratch = torch.empty((2, words, n), dtype=torch.float64, device=dev)
        N.call("dxa_frame_moments_levels", N.ptr(x), N.ptr(y), N.ptr(v), N.ptr(a), N.ptr(b), n, kind, maxlen,
               N.ptr(scratch), N.ptr(out), st)
    return out.cpu()


IMPLS = ["tensor", pytest.param("direct", marks=pytest.mark.gpu), pytest.param("levels", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("n", [1, 2, 3, 70, 300])
def test_state_words_on_hand_built_frames(impl, n):
    """n = 300 is more than one workgroup; 70 and 300 are no powers of two, so the top levels are clipped at n."""
    rnd = random.Random(n)
    xs = [_value(rnd) for _ in range(n)]
    ys = [_value(rnd) for _ in range(n)]
    frames = _hand_frames(n)
    a = torch.tensor([f[0] for f in frames], dtype=torch.int64)
    b = torch.tensor([f[1] for f in frames], dtype=torch.int64)
    x = torch.tensor(xs, dtype=torch.float64)
    y = torch.tensor(ys, dtype=torch.float64)
    clipped = [_clip(lo, hi, n) for lo, hi in frames]
    maxlen = max(1, max(hi - lo + 1 for lo, hi in clipped))
    worst = _Worst()
    for counted in ("all", "some", "none"):
        ok = [counted == "all" or (counted == "some" and rnd.random() < 0.7) for _ in range(n)]
        valid = None if counted == "all" else torch.tensor(ok, dtype=torch.bool)
        for kind in (W.KIND_VAR, W.KIND_MOM, W.KIND_CO):
            part = _Partition([None if not o else ((xv, yv) if kind == W.KIND_CO else (xv,))
                               for o, xv, yv in zip(ok, xs, ys)])
            got = _states(impl, kind, x, y if kind == W.KIND_CO else None, valid, a, b, maxlen)
            assert tuple(got.shape) == (W.STATE_WORDS[kind], n)
            for i, (lo, hi) in enumerate(clipped):
                want = _state_words(kind, part.state(lo, hi))
                row = got[:, i].tolist()
                assert row[0] == want[0], (kind, counted, frames[i], row, want)
                if want[0] == 0:
                    assert row == want, (kind, counted, frames[i], row)           # an empty frame: n = 0, zeros
                    continue
                for w in range(1, len(want)):
                    worst.check("word", row[w], want[w], (kind, counted, frames[i], w))
    worst.report(f"state words {impl} n={n}")


@pytest.mark.parametrize("impl", IMPLS)
def test_state_words_maxlen_one(impl):
    """Every frame is its own row (maxlen = 1: one level, no scratch read), a NULL row's frame is the identity."""
    n = 5
    x = torch.tensor([1.0, 2.5, float("inf"), 4.0, 7.75], dtype=torch.float64)
    valid = torch.tensor([True, False, True, True, True])
    a = torch.arange(n, dtype=torch.int64)
    for kind in (W.KIND_VAR, W.KIND_MOM, W.KIND_CO):
        got = _states(impl, kind, x, x.clone() if kind == W.KIND_CO else None, valid, a, a.clone(), 1)
        assert got[0].tolist() == [1.0, 0.0, 1.0, 1.0, 1.0]
        assert got[:, 1].tolist() == [0.0] * W.STATE_WORDS[kind]
        assert got[1, [0, 3, 4]].tolist() == [1.0, 4.0, 7.75]
        first_central = 3 if kind == W.KIND_CO else 2
        assert got[first_central:, [0, 3, 4]].abs().max() == 0.0
        assert torch.isnan(got[first_central:, 2]).all()              # inf − inf: the one-row frame of +inf is NaN


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments(gpu):
    from dxa.ops import native as N
    x = torch.zeros(4, dtype=torch.float64, device=gpu)
    a = torch.zeros(4, dtype=torch.int64, device=gpu)
    out = torch.zeros((6, 4), dtype=torch.float64, device=gpu)
    scratch = torch.zeros((2, 6, 4), dtype=torch.float64, device=gpu)
    st = N.stream_handle(gpu)
    p = N.ptr
    bad_direct = [(0, p(x), p(a), p(a), 4, 0, p(out)), (p(x), p(x), 0, p(a), 4, 0, p(out)),
                  (p(x), p(x), p(a), p(a), 4, 0, 0), (p(x), p(x), p(a), p(a), -1, 0, p(out)),
                  (p(x), p(x), p(a), p(a), 4, 3, p(out)), (p(x), 0, p(a), p(a), 4, W.KIND_CO, p(out))]
    for xx, yy, aa, bb, n, kind, oo in bad_direct:
        with pytest.raises(N.NativeError):
            N.call("dxa_frame_moments_direct", xx, yy, 0, aa, bb, n, kind, oo, st)
    bad_levels = [(p(x), p(a), 4, 0, 0, p(scratch)), (p(x), p(a), 4, 0, -3, p(scratch)),
                  (p(x), p(a), 4, 7, 2, p(scratch)), (p(x), p(a), 4, 0, 2, 0), (0, p(a), 4, 0, 2, p(scratch)),
                  (p(x), 0, 4, 0, 2, p(scratch))]
    for xx, aa, n, kind, maxlen, ss in bad_levels:
        with pytest.raises(N.NativeError):
            N.call("dxa_frame_moments_levels", xx, xx, 0, aa, aa, n, kind, maxlen, ss, p(out), st)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                      # a refused call launches nothing


# -- GPU: the twelve names through both entry points ------------------------------------------------------------------

GPU_ROWS = _random_rows(3000, 21, ["p", "q", "r", "s", "t", None], 0.1, 50)      # 12 workgroups, ~500-row partitions
GPU_GROUPS = {**{f"rows{i}": ROWS_GRID[i] for i in ROWS_GRID},
              "ordered": [OTHER_WINDOWS[w] for w in ("peers", "range_asc", "range_desc", "empty_near_end")],
              "long": [RUNNING, OTHER_WINDOWS["whole"]]}                          # ten levels


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GPU_GROUPS))
@pytest.mark.parametrize("path", ["levels", "direct"])
def test_gpu_entry_points_vs_oracle(gpu, monkeypatch, path, group):
    from launch_count import count_launches
    monkeypatch.setattr(W, "FRAME_DIRECT_MAX", 0 if path == "levels" else 10 ** 9)
    worst = _Worst()
    for window in GPU_GROUPS[group]:
        with count_launches() as log:
            _check_window(GPU_ROWS, window, "cuda", worst)
        used = [e for e in log if e.startswith("dxa_frame_moments_")]
        assert used == [f"dxa_frame_moments_{path}"] * len(NAMES), (window[0], used)     # once per window call
    worst.report(f"gpu {path} {group}")


@pytest.mark.gpu
def test_gpu_path_choice_follows_the_bound(gpu):
    """Unpatched: a frame of at most FRAME_DIRECT_MAX rows takes the direct entry, a longer one the levels entry, and
    one host read (the longest frame length) serves both."""
    from launch_count import count_launches
    short = f"PARTITION BY k ORDER BY id ROWS BETWEEN {W.FRAME_DIRECT_MAX - 1} PRECEDING AND CURRENT ROW"
    longer = f"PARTITION BY k ORDER BY id ROWS BETWEEN {W.FRAME_DIRECT_MAX} PRECEDING AND CURRENT ROW"
    for spec, entry in ((short, "direct"), (longer, "levels")):
        with count_launches() as log:
            _run(GPU_ROWS, f"SELECT id, stddev(v) OVER ({spec}) AS x FROM T", "cuda")
        assert [e for e in log if e.startswith("dxa_frame_moments_")] == [f"dxa_frame_moments_{entry}"]
