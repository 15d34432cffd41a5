"""Distinct counts as window functions: ``approx_count_distinct(x[, rsd])`` (exact here, as in GROUP BY),
``count(DISTINCT x)`` and ``count(DISTINCT a, b, …)`` ``OVER (PARTITION BY … ORDER BY … frame)``.  The result is a long
and never NULL: 0 for an empty frame and for a frame with no counted row.

The oracle is written here and holds no engine code: per row it builds a Python ``set`` of the frame's counted values
— NaN is one value, -0.0 and 0.0 are one value (they are equal and hash alike), a tuple is dropped where any member is
None — and takes its size.  The frame arithmetic is written here too.  Every comparison is ``==`` on integers.

The primitive (the number of different value ids among the counted rows of ``x[a .. b]``) is compared with a
brute-force set on hand-built frames: the tensor-operation wavelet walk on the CPU, and the two entry points of
window_distinct.hip on the GPU.

``approx_count_distinct(v, rsd)`` with an rsd that is no constant: GROUP BY never reads the rsd and so accepts it; the
window form mirrors that and accepts it too (``test_rsd_is_never_read_as_in_group_by``).
"""
import bisect
import math
import random

import pytest
import torch

from dxa.engine import windowfn as W
from dxa.engine.column import Table
from dxa.engine.expr import EvalContext
from dxa.engine.query import Catalog, QueryError, run_sql
from dxa.engine.types import StructField, StructType

SCHEMA = StructType((StructField("id", "long"), StructField("k", "string"), StructField("k2", "long"),
                     StructField("t", "long"), StructField("v", "double"), StructField("s", "string"),
                     StructField("m", "long")))
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
NAN = float("nan")
INF = float("inf")
ENTRIES = ("dxa_frame_distinct_direct", "dxa_frame_distinct_tree")


def _run(rows, sql, device="cpu"):
    c = Catalog()
    c.register("T", Table.from_pylist(rows, SCHEMA, device))
    return run_sql(sql, c, EvalContext(now_us=0)).to_pylist()


# -- the oracle -------------------------------------------------------------------------------------------------------

def _one(v):
    """A counted value as a set member (None: not counted): every NaN is one value; -0.0 == 0.0 already holds."""
    if isinstance(v, float) and math.isnan(v):
        return "NaN"
    return v


def _pair(r):
    return None if r["k2"] is None or r["v"] is None else (r["k2"], _one(r["v"]))


# A call is (sql, the row's counted value or None): the three spellings over the double, then a string, a long, a
# decimal and a pair.
CALLS = [("approx_count_distinct(v)", lambda r: _one(r["v"])),
         ("approx_count_distinct(v, 0.05)", lambda r: _one(r["v"])),
         ("count(DISTINCT v)", lambda r: _one(r["v"])),
         ("count(DISTINCT s)", lambda r: r["s"]),
         ("approx_count_distinct(m)", lambda r: r["m"]),
         ("count(DISTINCT CAST(m AS decimal(18,2)))", lambda r: r["m"]),
         ("count(DISTINCT k2, v)", _pair)]


def _distinct(values):
    return len(set(values) - {None})


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


def _peers(keys, p):
    return bisect.bisect_left(keys, keys[p]), bisect.bisect_right(keys, keys[p]) - 1


def _whole(keys, p):
    return 0, len(keys) - 1


ROWS_GRID = {i: [(f"PARTITION BY k ORDER BY id ROWS BETWEEN {i} PRECEDING AND {j} FOLLOWING", "id", _rows_frame(-i, j))
                 for j in range(4)] for i in range(4)}
WIDE = ("PARTITION BY k ORDER BY id ROWS BETWEEN 40 PRECEDING AND 25 FOLLOWING", "id", _rows_frame(-40, 25))
OTHER_WINDOWS = {
    "running": ("PARTITION BY k ORDER BY id ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW", "id",
                _rows_frame(-10 ** 9, 0)),
    "default": ("PARTITION BY k ORDER BY t", "t", _running_peers),
    "whole": ("PARTITION BY k", "id", _whole),
    "peers": ("PARTITION BY k ORDER BY t RANGE BETWEEN CURRENT ROW AND CURRENT ROW", "t", _peers),
    "range_asc": ("PARTITION BY k ORDER BY t RANGE BETWEEN 3 PRECEDING AND 2 FOLLOWING", "t", _range_frame(-3, 2)),
    "range_desc": ("PARTITION BY k ORDER BY t DESC RANGE BETWEEN 3 PRECEDING AND 2 FOLLOWING", "t_desc",
                   _range_frame(-3, 2)),
    "empty_near_end": ("PARTITION BY k ORDER BY id ROWS BETWEEN 2 FOLLOWING AND 3 FOLLOWING", "id", _rows_frame(2, 3)),
}
GROUPS = {**{f"rows{i}": ROWS_GRID[i] for i in ROWS_GRID},
          "ordered": [OTHER_WINDOWS[w] for w in ("default", "peers", "range_asc", "range_desc", "empty_near_end")],
          "long": [WIDE, OTHER_WINDOWS["running"], OTHER_WINDOWS["whole"]]}


def _statement(spec, calls):
    return "SELECT id, " + ", ".join(f"{c[0]} OVER ({spec}) AS f{i}" for i, c in enumerate(calls)) + " FROM T"


_ORACLE = {}                      # (rows name, window sql) → {id: expected results of CALLS}: computed once, shared


def _oracle(name, rows, window):
    spec, order, frame = window
    if (name, spec) not in _ORACLE:
        want = {}
        for g, keys in _sorted_partitions(rows, order):
            values = [[value(r) for r in g] for _, value in CALLS]
            for p, r in enumerate(g):
                lo, hi = frame(keys, p)
                want[r["id"]] = [_distinct(v[lo:hi + 1]) for v in values]
        _ORACLE[(name, spec)] = want
    return _ORACLE[(name, spec)]


def _check_window(name, rows, window, device):
    """Run CALLS over one window on ``device`` and compare every row with the oracle; rows keep input order."""
    got = _run(rows, _statement(window[0], CALLS), device)
    assert [r["id"] for r in got] == [r["id"] for r in rows]
    want = _oracle(name, rows, window)
    for r in got:
        assert [r[f"f{i}"] for i in range(len(CALLS))] == want[r["id"]], (window[0], r["id"])


def _value(rnd):
    """A multiple of 0.25 in [0, 8), skewed towards 0 so that ties are frequent — or NaN, 0.0, -0.0."""
    u = rnd.random()
    if u < 0.04:
        return NAN
    if u < 0.08:
        return -0.0
    if u < 0.12:
        return 0.0
    return int(32 * rnd.random() ** 2) / 4.0


def _random_rows(n, seed, keys, tmax):
    rnd = random.Random(seed)
    words = ["", "a", "ab", "abc", "ABC", "a much longer string than the others", "é", "b"]
    return [{"id": i, "k": rnd.choice(keys), "k2": rnd.choice([None, 0, 1, 2]),
             "t": rnd.choice([None] + list(range(tmax))), "v": None if rnd.random() < 0.1 else _value(rnd),
             "s": rnd.choice([None] + words), "m": rnd.choice([None, -3, 0, 1, 2, 5, 10 ** 12, 7, 7, 7])}
            for i in range(n)]


CPU_ROWS = _random_rows(300, 11, ["p", "q", "r", None], 20)


def _gpu_rows():
    rows = _random_rows(3000, 21, ["p", "q", "r", "s", "t", None], 50)      # 12 workgroups, ~500-row partitions
    rows[1234]["k"] = "lone"                                                # a single-row partition
    return rows


GPU_ROWS = _gpu_rows()

# -- SQL surface ------------------------------------------------------------------------------------------------------

SEVEN = [
    {"id": 1, "k": "a", "k2": 1, "t": 10, "v": 1.0, "s": "x", "m": 1},
    {"id": 2, "k": "a", "k2": 1, "t": 20, "v": 2.0, "s": "y", "m": 1},
    {"id": 3, "k": "a", "k2": None, "t": 20, "v": None, "s": "x", "m": 2},
    {"id": 4, "k": "a", "k2": 2, "t": 30, "v": 1.0, "s": None, "m": 1},
    {"id": 5, "k": "b", "k2": 1, "t": 5, "v": NAN, "s": "x", "m": None},
    {"id": 6, "k": "b", "k2": 1, "t": None, "v": NAN, "s": "x", "m": None},
    {"id": 7, "k": None, "k2": 3, "t": 1, "v": -0.0, "s": "z", "m": 4},
]


def test_hand_computed_rows():
    got = _run(SEVEN, "SELECT id, approx_count_distinct(v) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 1 PRECEDING "
                      "AND CURRENT ROW) AS two, count(DISTINCT v) OVER (PARTITION BY k) AS part, count(DISTINCT k2, v) "
                      "OVER (PARTITION BY k ORDER BY id) AS run, approx_count_distinct(s, 0.01) OVER () AS every, "
                      "count(DISTINCT m) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 1 FOLLOWING AND 2 FOLLOWING) "
                      "AS ahead FROM T ORDER BY id")
    by = {r["id"]: r for r in got}
    # partition a by id: 1, 2, NULL, 1 — two-row frames {1}, {1, 2}, {2}, {1}
    assert [by[i]["two"] for i in range(1, 8)] == [1, 2, 1, 1, 1, 1, 1]          # NaN counts, once; so does -0.0
    assert [by[i]["part"] for i in range(1, 8)] == [2, 2, 2, 2, 1, 1, 1]
    # pairs (1, 1), (1, 2), dropped, (2, 1) in a; (1, NaN) twice in b
    assert [by[i]["run"] for i in range(1, 8)] == [1, 2, 2, 3, 1, 1, 1]
    assert [by[i]["every"] for i in range(1, 8)] == [3] * 7
    # m of the next two rows: a → {1, 2}, {2, 1}, {1}, none; b → NULLs only, none; the NULL partition → none
    assert [by[i]["ahead"] for i in range(1, 8)] == [2, 2, 1, 0, 0, 0, 0]


def test_result_is_long_and_never_null():
    c = Catalog()
    c.register("T", Table.from_pylist(SEVEN, SCHEMA))
    out = run_sql("SELECT approx_count_distinct(v) OVER (PARTITION BY k) AS a, count(DISTINCT s) OVER (ORDER BY id ROWS "
                  "BETWEEN 5 FOLLOWING AND 9 FOLLOWING) AS b, count(DISTINCT k2, s) OVER () AS c FROM T",
                  c, EvalContext(now_us=0))
    assert [str(col.dtype) for col in out.columns] == ["long"] * 3
    for r in out.to_pylist():
        assert all(isinstance(r[x], int) for x in "abc"), r


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_frames_vs_oracle(group, device):
    rows = ("cpu", CPU_ROWS) if device == "cpu" else ("gpu", GPU_ROWS)
    for window in GROUPS[group]:
        _check_window(*rows, window, device)


@pytest.mark.parametrize("device", DEVICES)
def test_window_equals_group_by(device):
    """One whole-partition window and GROUP BY's distinct counts over the same rows agree under ``==``; partition r
    holds no counted v."""
    calls = [c[0] for c in CALLS]
    rows = [dict(r, v=None if r["k"] == "r" else r["v"]) for r in CPU_ROWS]
    grouped = _run(rows, "SELECT k, " + ", ".join(f"{c} AS f{i}" for i, c in enumerate(calls)) + " FROM T GROUP BY k",
                   device)
    by_key = {r["k"]: r for r in grouped}
    assert len(by_key) == 4
    windowed = _run(rows, "SELECT k, " + ", ".join(f"{c} OVER (PARTITION BY k) AS f{i}" for i, c in enumerate(calls))
                    + " FROM T", device)
    assert len(windowed) == len(rows)
    for r in windowed:
        assert r == by_key[r["k"]], (r, by_key[r["k"]])
    assert [by_key["r"][f"f{i}"] for i in (0, 1, 2, 6)] == [0, 0, 0, 0] and by_key["r"]["f3"] > 0
    assert by_key["p"]["f0"] > 1


@pytest.mark.parametrize("sql,message", [
    ("SELECT sum(DISTINCT v) OVER (PARTITION BY k) AS x FROM T", "DISTINCT is not supported in window aggregates"),
    ("SELECT avg(DISTINCT v) OVER (PARTITION BY k) AS x FROM T", "DISTINCT is not supported in window aggregates"),
    ("SELECT max(DISTINCT v) OVER (PARTITION BY k) AS x FROM T", "DISTINCT is not supported in window aggregates"),
    ("SELECT stddev(DISTINCT v) OVER (PARTITION BY k) AS x FROM T", "DISTINCT is not supported in window aggregates"),
    ("SELECT approx_count_distinct() OVER () AS x FROM T", "wrong number of arguments to approx_count_distinct"),
    ("SELECT approx_count_distinct(v, 0.05, 1) OVER () AS x FROM T",
     "wrong number of arguments to approx_count_distinct"),
    ("SELECT count(DISTINCT array(v, 1.0)) OVER () AS x FROM T", r"count\(DISTINCT …\) OVER cannot count"),
    ("SELECT approx_count_distinct(array(v, 1.0)) OVER () AS x FROM T", "approx_count_distinct OVER cannot count"),
    ("SELECT approx_count_distinct(named_struct('a', v)) OVER () AS x FROM T",
     "approx_count_distinct OVER cannot count"),
])
def test_refusals(sql, message):
    with pytest.raises(QueryError, match=message):
        _run(SEVEN, sql)


def test_rsd_is_never_read_as_in_group_by():
    """GROUP BY accepts an rsd that is no constant (it never reads it); so does the window form."""
    grouped = _run(SEVEN, "SELECT k, approx_count_distinct(v, id * 0.01) AS x FROM T GROUP BY k")
    by_key = {r["k"]: r["x"] for r in grouped}
    assert by_key == {"a": 2, "b": 1, None: 1}
    for r in _run(SEVEN, "SELECT k, approx_count_distinct(v, id * 0.01) OVER (PARTITION BY k) AS x FROM T"):
        assert r["x"] == by_key[r["k"]]


# -- the primitive on hand-built frames -------------------------------------------------------------------------------

def _hand_frames(n):
    """Single rows, length 2, lengths 3–9 and longer where they fit, the whole array, frames hanging over both ends,
    a > b."""
    mid = n // 2
    fr = [(0, 0), (n - 1, n - 1), (mid, mid), (0, 1), (n - 2, n - 1), (mid, mid + 1), (0, n - 1), (-4, n + 3),
          (-5, 1), (-2, -1), (n - 2, n + 6), (n, n + 2), (3, 2), (n - 1, 0), (1, 0)]
    for length in (3, 4, 5, 6, 7, 8, 9, 16, 17, 33, 64, 65, 129, 256):
        if length <= n:
            fr += [(0, length - 1), (n - length, n - 1), ((n - length) // 2, (n - length) // 2 + length - 1)]
    return fr


def _count(impl, vid, counted, a, b, cache):
    """The counts of one implementation, on the host; p and the wavelet matrix are built once per ``cache``."""
    if impl != "tensor":
        dev = torch.device("cuda:0")
        vid, counted, a, b = (t.to(dev) for t in (vid, counted, a, b))
    if "p" not in cache:
        cache["p"] = W._prev_occurrence(vid, counted)
        if impl != "direct":
            cache["tree"] = W._distinct_tree_build(cache["p"], counted, tensor=impl == "tensor")
    p = cache["p"]
    if impl == "tensor":
        return W._frame_distinct_tensor(p, counted, a, b, cache["tree"])
    if impl == "direct":
        return W._frame_distinct_direct(p, a, b).cpu()
    return W._frame_distinct_tree(cache["tree"], a, b).cpu()


IMPLS = ["tensor", pytest.param("direct", marks=pytest.mark.gpu), pytest.param("tree", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("ids", ["ties", "equal", "distinct"])
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 70, 300])
def test_counts_on_hand_built_frames(impl, ids, n):
    """8 and 9 straddle a level-count change, 70 and 300 are no powers of two, 300 is more than one workgroup; n = 8
    with distinct ids and every row counted has T = 2^L for every frame.  The primitive answers one frame per row,
    so the frames go through it n at a time."""
    rnd = random.Random(n)
    if ids == "ties":
        values = [rnd.randrange(min(6, n)) for _ in range(n)]          # value ids are dense: below n
    elif ids == "equal":
        values = [0] * n
    else:
        values = list(range(n))
        rnd.shuffle(values)
    vid = torch.tensor(values, dtype=torch.int64)
    frames = _hand_frames(n)
    frames += [(1, 0)] * (-len(frames) % n)
    for counted in ("all", "some", "none"):
        ok = [counted == "all" or (counted == "some" and rnd.random() < 0.7) for _ in range(n)]
        valid = torch.tensor(ok, dtype=torch.bool)
        cache = {}
        for s in range(0, len(frames), n):
            batch = frames[s:s + n]
            want = [len({values[j] for j in range(max(lo, 0), min(hi, n - 1) + 1) if ok[j]}) if lo <= hi else 0
                    for lo, hi in batch]
            a = torch.tensor([f[0] for f in batch], dtype=torch.int64)
            b = torch.tensor([f[1] for f in batch], dtype=torch.int64)
            got = _count(impl, vid, valid, a, b, cache)
            assert got.dtype == torch.int64 and got.tolist() == want, (counted, batch)
        # the previous-occurrence array itself: previous counted row of the same id, -1, or the sentinel n
        last, p_want = {}, []
        for j in range(n):
            p_want.append(last.get(values[j], -1) if ok[j] else n)
            if ok[j]:
                last[values[j]] = j
        assert cache["p"].dtype == torch.int32 and cache["p"].tolist() == p_want, counted


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments(gpu):
    from dxa.ops import native as N
    n = 4
    prev = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    a = torch.zeros(n, dtype=torch.int64, device=gpu)
    T = torch.ones(n, dtype=torch.int64, device=gpu)
    # the matrix of four counted first occurrences: global ranks 0, 1, 2, 3 in position order
    Z = torch.tensor([[0, 1, 2, 2, 2], [0, 1, 1, 2, 2]], dtype=torch.int32, device=gpu)
    out = torch.zeros(n, dtype=torch.int64, device=gpu)
    st = N.stream_handle(gpu)
    p = N.ptr
    big = 1 << 31
    # (p, a, b, n, out)
    good = [p(prev), p(a), p(a), n, p(out)]
    for slot, value in ((0, 0), (1, 0), (2, 0), (4, 0), (3, -1), (3, big)):
        args = list(good)
        args[slot] = value
        with pytest.raises(N.NativeError):
            N.call("dxa_frame_distinct_direct", *args, st)
    # (Z, T, a, b, n, levels, out); n = 4 has two levels
    good_tree = [p(Z), p(T), p(a), p(a), n, 2, p(out)]
    for slot, value in ((0, 0), (1, 0), (2, 0), (3, 0), (6, 0), (4, -1), (4, big), (5, 1), (5, 3), (5, 0), (5, -2)):
        args = list(good_tree)
        args[slot] = value
        with pytest.raises(N.NativeError):
            N.call("dxa_frame_distinct_tree", *args, st)
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0                       # a refused call launched nothing
    # the same buffers, accepted: every frame is row 0 alone, a first occurrence (p = -1 < 0; global rank 0, below
    # T = 1) → 1; n = 0 is accepted and idle
    out.fill_(-7)
    N.call("dxa_frame_distinct_direct", p(prev), p(a), p(a), 0, p(out), st)
    N.call("dxa_frame_distinct_tree", p(Z), p(T), p(a), p(a), 0, 0, p(out), st)
    assert out.tolist() == [-7] * n
    N.call("dxa_frame_distinct_direct", *good, st)
    assert out.tolist() == [1] * n
    out.fill_(-7)
    N.call("dxa_frame_distinct_tree", *good_tree, st)
    assert out.tolist() == [1] * n


# -- GPU: every window group through both entry points ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("path", ["tree", "direct"])
def test_gpu_entry_points_vs_oracle(gpu, monkeypatch, path, group):
    from launch_count import count_launches
    monkeypatch.setattr(W, "FRAME_DISTINCT_DIRECT_MAX", 0 if path == "tree" else 10 ** 9)
    for window in GROUPS[group]:
        with count_launches() as log:
            _check_window("gpu", GPU_ROWS, window, "cuda")
        used = [e for e in log if e in ENTRIES]
        assert used == [f"dxa_frame_distinct_{path}"] * len(CALLS), (window[0], used)    # once per window call


@pytest.mark.gpu
def test_gpu_path_choice_follows_the_bound(gpu):
    """Unpatched: a frame of FRAME_DISTINCT_DIRECT_MAX rows takes the direct entry, one row more the tree entry."""
    from launch_count import count_launches
    bound = W.FRAME_DISTINCT_DIRECT_MAX
    rows = GPU_ROWS if bound + 2 <= len(GPU_ROWS) else _random_rows(bound + 2, 5, ["p"], 50)
    short = f"ORDER BY id ROWS BETWEEN {bound - 1} PRECEDING AND CURRENT ROW"
    longer = f"ORDER BY id ROWS BETWEEN {bound} PRECEDING AND CURRENT ROW"
    for spec, entry in ((short, "direct"), (longer, "tree")):
        with count_launches() as log:
            got = _run(rows, f"SELECT id, count(DISTINCT v) OVER ({spec}) AS x FROM T", "cuda")
        assert [e for e in log if e in ENTRIES] == [f"dxa_frame_distinct_{entry}"]
        assert got[-1]["x"] == _distinct([_one(r["v"]) for r in rows[-(bound if entry == "direct" else bound + 1):]])


@pytest.mark.gpu
def test_gpu_empty_frames_launch_nothing(gpu):
    """Every frame empty: zeros, and neither entry point runs."""
    from launch_count import count_launches
    with count_launches() as log:
        got = _run(SEVEN, "SELECT count(DISTINCT v) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 7 FOLLOWING AND 9 "
                          "FOLLOWING) AS x FROM T", "cuda")
    assert [r["x"] for r in got] == [0] * 7 and not [e for e in log if e in ENTRIES]
