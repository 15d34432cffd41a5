"""Grouping and aggregation at special values and at the thresholds between implementations.

Every path — the CPU evaluator (groupby.py ``_agg_raw``), the LDS-privatised and the global-atomic per-aggregate
kernels, the fused multi-aggregate, the three group renumbering paths, the key hash / verify kernels and the dense
window ring — is compared with ``tests/agg_oracle.py`` (plain Python) or ``numpy.unique``; no path is compared with
another path.  Finite doubles are multiples of 0.25 below 2**20, so double sums are exact in any order and every
comparison is for equality (NaN as NaN, zeros with their sign).  Long values that reach ±2**63 sit in groups whose
double sum (AVG) is exact in any order as well: a few values of one sign, or only the two extremes.
"""
import functools
import math
import struct

import numpy as np
import pytest
import torch

from dxa.engine.column import PrimColumn, StrColumn, Table, strings_from_pylist
from dxa.engine.expr import EvalContext
from dxa.engine.query import Catalog, run_sql
from dxa.ops import groupby as G
from tests import agg_oracle as O
from tests.window_dense_support import S, dense_states, new_store, set_caps

NAN, INF = math.nan, math.inf
I_MIN, I_MAX = O.INT64_MIN, O.INT64_MAX
CPU = torch.device("cpu")


def f64_from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _mismatches(got, want, what, limit=6):
    bad = [(what, i, g, w) for i, (g, w) in enumerate(zip(got, want)) if not O.same(g, w)]
    assert len(got) == len(want), (what, len(got), len(want))
    return bad[:limit]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle itself
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_hand_cases():
    R = [("c", "count_star", None), ("n", "count", 1), ("s", "sum", 1), ("mn", "min", 1), ("mx", "max", 1),
         ("av", "avg", 1)]

    def one(vals):
        return O.group_by([(0, v) for v in vals], [0], R)[(0,)]

    r = one([NAN, 1.0, -2.0])                                  # Spark: NaN is the greatest double
    assert r["mn"] == -2.0 and r["mx"] != r["mx"] and r["s"] != r["s"] and r["c"] == 3
    r = one([-0.0, 0.0])                                       # -0.0 < 0.0
    assert O.same(r["mx"], 0.0) and O.same(r["mn"], -0.0) and O.same(r["s"], 0.0)
    assert O.same(one([-0.0, -0.0])["s"], 0.0)                 # the sum starts at +0.0
    r = one([INF, -INF])
    assert r["s"] != r["s"] and r["mn"] == -INF and r["mx"] == INF
    r = one([INF, 5.0])
    assert r["s"] == INF and r["av"] == INF and r["mn"] == 5.0
    r = one([None, None])
    assert r == {"c": 2, "n": 0, "s": None, "mn": None, "mx": None, "av": None}
    r = one([I_MAX, 1])                                        # integer sums wrap
    assert r["s"] == I_MIN and r["mx"] == I_MAX and r["av"] == 2.0**62
    assert one([I_MIN, -1])["s"] == I_MAX
    assert one([I_MIN, I_MAX]) == {"c": 2, "n": 2, "s": -1, "mn": I_MIN, "mx": I_MAX, "av": 0.0}
    r = one([True, False, None])
    assert r["mn"] is False and r["mx"] is True and r["n"] == 2
    assert one([0.25, 0.5, None])["av"] == 0.375
    # keys: one NaN group, one zero group, NULL is a key and "" is not NULL
    nan2 = f64_from_bits(0xfff8000000000001)
    keys = [NAN, nan2, 0.0, -0.0, 1.5, NAN, None, None]
    got = O.group_by([(k,) for k in keys], [0], [("c", "count_star", None)])
    assert got == {(O.NAN,): {"c": 3}, (0.0,): {"c": 2}, (1.5,): {"c": 1}, (None,): {"c": 2}}
    assert O.group_ids([(k,) for k in keys], [0]) == ([0, 0, 1, 1, 2, 0, 3, 3], [0, 2, 4, 6])
    assert len(O.group_by([("",), (None,), ("a",), ("",)], [0], [])) == 3
    assert not O.same(0.0, -0.0) and O.same(NAN, nan2) and not O.same(1, 1.0) and O.same(None, None)


# ---------------------------------------------------------------------------------------------------------------------
# the three CPU findings: grouping of NaN keys, MIN with a NaN, MAX of the two zeros
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_groups(gid, ng):
    gid = torch.tensor(gid, dtype=torch.int64)
    rep = torch.full((ng,), len(gid), dtype=torch.int64).scatter_reduce(0, gid, torch.arange(len(gid)), "amin")
    return G.Groups(gid, ng, rep)


def test_cpu_nan_keys_are_one_group():
    vals = [NAN, NAN, 0.0, -0.0, 1.5, NAN]
    g = G.group_rows([PrimColumn("double", torch.tensor(vals, dtype=torch.float64))])
    gid, rep = O.group_ids([(v,) for v in vals], [0])
    assert (g.ngroups, g.gid.tolist(), g.rep.tolist()) == (3, gid, rep)
    cat = Catalog()
    cat.register("T", Table(["k"], [PrimColumn("double", torch.tensor(vals, dtype=torch.float64))], len(vals), "cpu"))
    rows = run_sql("SELECT k, COUNT(*) AS c FROM T GROUP BY k", cat, EvalContext(now_us=0)).to_pylist()
    assert len(rows) == 3, rows
    assert {O.key_token(r["k"]): r["c"] for r in rows} == {O.NAN: 3, 0.0: 2, 1.5: 1}


def test_cpu_min_max_follow_the_total_order():
    col = PrimColumn("double", torch.tensor([NAN, 1.0, -2.0, -0.0, 0.0], dtype=torch.float64))
    g = _cpu_groups([0, 0, 0, 1, 1], 2)
    mn = G.aggregate(g, col, "min", 5).to_pylist()
    mx = G.aggregate(g, col, "max", 5).to_pylist()
    assert O.same(mn[0], -2.0) and O.same(mx[0], NAN), (mn, mx)
    assert O.same(mn[1], -0.0) and O.same(mx[1], 0.0), (mn, mx)


# ---------------------------------------------------------------------------------------------------------------------
# A. numbering paths and their thresholds
# ---------------------------------------------------------------------------------------------------------------------
BITMAP_ROWS = 524288
NUMBERING = [(524288, 4097, "bitmap"), (524288, 1, "bitmap"), (524289, 1, "bitonic"), (524289, 2, "bitonic"),
             (524289, 1000, "bitonic"), (524289, 4096, "bitonic"), (524289, 4097, "argsort")]


@functools.lru_cache(maxsize=None)
def numbering_case(n, ng):
    """int64 keys with exactly ``ng`` distinct values, some of whose first rows sit at chosen places: rows 63, 64,
    524224 and 524287 (word edges of the first-row bitmap) when n is a bitmap size, row n - 1 otherwise.  →
    (keys, gid, rep, the chosen rows) with gid / rep from numpy.unique."""
    rng = np.random.default_rng(n * 31 + ng)
    wanted = [63, 64, 524224, 524287] if n <= BITMAP_ROWS else [n - 1]
    wanted = wanted[max(0, len(wanted) - (ng - 1)):]
    nb = ng - len(wanted)
    lab = rng.permutation(n) % nb                       # every bulk label occurs n // nb >= 127 times
    for j, r in enumerate(wanted):
        later = rng.integers(r, n, 3)
        later = later[~np.isin(later, wanted)]
        lab[later] = nb + j
        lab[r] = nb + j
    keys = (lab.astype(np.int64) - 11) * 1_000_003
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    assert len(uniq) == ng
    order = np.argsort(first)
    rank = np.empty(ng, dtype=np.int64)
    rank[order] = np.arange(ng)
    rep = first[order]
    assert set(wanted) <= set(rep.tolist()) and rep[0] == 0
    return keys, rank[inv.reshape(-1)], rep, wanted


def check_numbering(n, ng, dev):
    assert (G._RENUMBER_BITMAP_ROWS, G._RENUMBER_MAX) == (BITMAP_ROWS, 4096)      # the thresholds the cases sit at
    keys, gid, rep, _ = numbering_case(n, ng)
    g = G.group_rows([PrimColumn("long", torch.from_numpy(keys).to(dev))])
    assert g.ngroups == ng
    assert np.array_equal(g.rep.cpu().numpy(), rep)
    assert np.array_equal(g.gid.cpu().numpy().astype(np.int64), gid)


@pytest.mark.gpu
@pytest.mark.parametrize("n,ng,path", NUMBERING)
def test_numbering_paths_gpu(gpu, n, ng, path):
    """dxa_group_renumber: renumber_bitmap_kernel for n <= 524288, renumber_sort_kernel (one-workgroup bitonic sort,
    padded to a power of two) for larger n with at most 4096 groups, torch.argsort above — chosen by (n, ngroups)."""
    check_numbering(n, ng, gpu)


def test_numbering_cpu():
    check_numbering(524289, 1000, CPU)


# ---------------------------------------------------------------------------------------------------------------------
# B. every aggregate path x special values
# ---------------------------------------------------------------------------------------------------------------------
# (double pattern, long pattern, boolean pattern): a special group's values at its (up to) three far-apart rows
SPECIALS = [
    ([NAN, 1.0, -2.0], [I_MAX, 1, None], [True, True, True]),              # NaN first, a number last; SUM wraps
    ([-2.0, 1.0, NAN], [I_MIN, -1, None], [True, False, None]),            # the reverse order
    ([NAN, NAN, NAN], [I_MIN, I_MAX, None], [False, False, False]),        # all NaN
    ([INF, -INF, None], [-5, -7, -1], [None, None, None]),                 # both infinities; negatives only
    ([INF, 5.0, None], [I_MAX, I_MAX, 2], [False, True, True]),
    ([-0.0, 0.0, None], [0, None, None], [None, True, None]),              # the zeros, both orders
    ([0.0, -0.0, None], [None, None, 7], [None, None, False]),
    ([-0.0, -0.0, -0.0], [I_MIN, I_MIN, None], [True, None, True]),        # all -0.0
    ([None, None, None], [None, None, None], [None, None, None]),          # all NULL
    ([-3.25], [I_MIN], [True]),                                            # a single row (its other rows are dropped)
    ([-1.5, -1024.75, -0.25], [-1, I_MIN, None], [False, None, None]),     # negatives only
    ([-INF, NAN, None], [I_MAX, None, None], [True, True, None]),
    ([None, NAN, None], [None, I_MIN, None], [None, False, None]),
]
AGG_GROUPS = [1, 7, 40, 4095, 4096, 8192, 8193]       # 40: every special group on the small-LDS launch shape
AGG_REQS = ([("n", "count_star", None)] +
            [(f"{f}_{c}", f, c) for c in ("d", "l") for f in ("count", "sum", "min", "max", "avg")] +
            [("min_b", "min", "b"), ("max_b", "max", "b")] +
            [(f"{f}_u", f, "u") for f in ("count", "sum", "min", "max", "avg")])
COLS = ("k", "d", "l", "b", "u")


@functools.lru_cache(maxsize=None)
def agg_case(ng):
    """Row p belongs to group p % ng, so groups are numbered by first appearance already.  A special group's pattern
    rows are ``stride`` >= 2100 > 256 * 8 rows apart (different workgroups of agg_lds_kernel: the flush merge sees
    them); its other rows are NULL in the masked columns d / l / b.  ``u`` is a double column WITHOUT a validity mask
    holding d's values (0.5 under a NULL).  → (numpy columns, gid, expected aggregates in group order)."""
    rng = np.random.default_rng(1000 + ng)
    stride = ng * -(-2100 // ng)
    n = max(3 * stride, 4096) + 3
    grp = np.arange(n) % ng
    d = rng.integers(-2**22 + 1, 2**22, n) * 0.25
    dv = rng.random(n) > 0.1
    l = rng.integers(-1000, 1000, n)
    lv = rng.random(n) > 0.1
    b = rng.random(n) > 0.5
    bv = rng.random(n) > 0.1
    keep = np.ones(n, dtype=bool)
    for g, (pd, pl, pb) in enumerate(SPECIALS[:ng]):
        mine = grp == g
        dv[mine] = lv[mine] = bv[mine] = False
        if len(pd) == 1:
            keep[mine] = False
        for m in range(len(pd)):
            p = g + m * stride
            keep[p] = True
            for arr, val, pat in ((d, dv, pd), (l, lv, pl), (b, bv, pb)):
                if pat[m] is not None:
                    arr[p], val[p] = pat[m], True
    u = np.where(dv, d, 0.5)
    cols = {"k": grp[keep] * 3 - 7, "d": d[keep], "dv": dv[keep], "l": l[keep], "lv": lv[keep], "b": b[keep],
            "bv": bv[keep], "u": u[keep]}
    lists = [cols["k"].tolist()] + [[v if ok else None for v, ok in zip(cols[c].tolist(), cols[c + "v"].tolist())]
                                    for c in "dlb"] + [cols["u"].tolist()]
    rows = list(zip(*lists))
    reqs = [(a, f, None if c is None else COLS.index(c)) for a, f, c in AGG_REQS]
    want = O.group_by(rows, [0], reqs)
    assert list(want) == [(g * 3 - 7,) for g in range(ng)]
    return cols, grp[keep], list(want.values())


def agg_inputs(ng, dev):
    cols, gid, want = agg_case(ng)
    t = {c: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for c, v in cols.items()}
    table = {"d": PrimColumn("double", t["d"], t["dv"]), "l": PrimColumn("long", t["l"], t["lv"]),
             "b": PrimColumn("boolean", t["b"], t["bv"]), "u": PrimColumn("double", t["u"])}
    n = len(gid)
    gt = torch.from_numpy(gid).to(dev)
    rep = torch.arange(ng, dtype=torch.int64, device=dev)          # group g's first row is row g
    groups = G.Groups(gt.to(torch.int32) if dev.type == "cuda" else gt, ng, rep)
    return table, groups, n, want


def check_aggregates(ng, dev, many):
    table, groups, n, want = agg_inputs(ng, dev)
    reqs = [(None if c is None else table[c], f) for _, f, c in AGG_REQS]
    if many:
        res = G.aggregate_many(groups, reqs, n)
    else:
        res = [G.aggregate(groups, c, f, n) for c, f in reqs]
    bad = []
    for (alias, _, _), col in zip(AGG_REQS, res):
        bad += _mismatches(col.to_pylist(), [w[alias] for w in want], alias, 3)
    assert not bad, bad[:12]           # (aggregate, group, got, expected)


@pytest.mark.gpu
@pytest.mark.parametrize("ng", AGG_GROUPS)
def test_single_aggregates_gpu(gpu, ng):
    """G.aggregate, one request at a time: agg_lds_kernel up to 8192 groups (exactly 64 KiB of LDS there),
    agg_global_kernel at 8193."""
    check_aggregates(ng, gpu, many=False)


@pytest.mark.gpu
@pytest.mark.parametrize("ng", AGG_GROUPS)
def test_many_aggregates_gpu(gpu, ng):
    """G.aggregate_many with 18 requests: agg_multi_kernel + agg_finish_kernel from 4096 groups, the per-aggregate
    kernels at 4095 and below."""
    assert G.FUSED_MIN_GROUPS == 4096
    check_aggregates(ng, gpu, many=True)


@pytest.mark.parametrize("ng", AGG_GROUPS)
def test_aggregates_cpu(ng):
    check_aggregates(ng, CPU, many=True)


# ---------------------------------------------------------------------------------------------------------------------
# C. key columns on group_rows
# ---------------------------------------------------------------------------------------------------------------------
NAN_BITS = (0x7ff8000000000000, 0xfff8000000000001)
KEY_STRINGS = (["", "a", "b"] +
               ["x" * (L - 1) + c for L in (7, 8, 9, 15, 16, 17, 47, 48, 49) for c in "pq"] +    # last byte differs
               ["prefix-" * 7, ("prefix-" * 7)[:48], ("prefix-" * 7)[:47], "prefix-", "prefix"] +  # prefixes
               ["é", "éé", "日本語のキー", "日本語のキ", "x" * 6 + "é", "x" * 7 + "é", "🙂" * 12, "🙂" * 12 + "a"])


def no_exact_groups(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("group_rows left the hashed path for _exact_groups")
    monkeypatch.setattr(G, "_exact_groups", boom)


def double_key_column(n, seed):
    """Doubles with two NaN bit patterns, both zeros, both infinities and NULLs → (numpy data, valid, Python values)."""
    rng = np.random.default_rng(seed)
    pool = np.array([f64_from_bits(NAN_BITS[0]), f64_from_bits(NAN_BITS[1]), -0.0, 0.0, INF, -INF, 1.5, -1.5, 2.0**-1074],
                    dtype=np.float64)
    bits = pool.view(np.uint64)[rng.integers(0, len(pool), n)]
    valid = rng.random(n) > 0.15
    data = bits.view(np.float64)
    assert {int(x) for x in bits} >= set(NAN_BITS)
    return data, valid, [v if ok else None for v, ok in zip(data.tolist(), valid.tolist())]


def string_key_column(n, seed, strings=KEY_STRINGS, dev=CPU):
    """A string column whose arena holds every string at every offset 0-7 modulo 8 (load_part's shift cases); NULL
    rows point at real bytes.  → (StrColumn, Python values)."""
    rng = np.random.default_rng(seed)
    blob = bytearray()
    at = {}                                       # (string index, offset mod 8) → start
    for off in range(8):
        for i, s in enumerate(strings):
            blob += b"#" * ((off - len(blob)) % 8)
            at[i, off] = len(blob)
            blob += s.encode("utf-8")
    assert {a % 8 for a in at.values()} == set(range(8))
    pick = rng.integers(0, len(strings), n)
    pick[:len(strings)] = np.arange(len(strings))
    off = rng.integers(0, 8, n)
    valid = rng.random(n) > 0.1
    starts = np.array([at[int(i), int(o)] for i, o in zip(pick, off)], dtype=np.int64)
    lens = np.array([len(strings[int(i)].encode("utf-8")) for i in pick], dtype=np.int32)
    arena = torch.from_numpy(np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8).copy())
    col = StrColumn(arena.to(dev), torch.from_numpy(starts).to(dev), torch.from_numpy(lens).to(dev),
                    torch.from_numpy(valid).to(dev))
    return col, [strings[int(i)] if ok else None for i, ok in zip(pick, valid.tolist())]


def check_groups(cols, values, monkeypatch):
    no_exact_groups(monkeypatch)
    g = G.group_rows(cols)
    gid, rep = O.group_ids(list(zip(*values)), list(range(len(values))))
    assert g.ngroups == len(rep)
    assert g.rep.cpu().tolist() == rep
    assert g.gid.cpu().tolist() == gid


def check_double_key(dev, monkeypatch):
    data, valid, vals = double_key_column(1500, 5)
    check_groups([PrimColumn("double", torch.from_numpy(data.copy()).to(dev), torch.from_numpy(valid).to(dev))],
                 [vals], monkeypatch)


def check_string_key(dev, monkeypatch):
    col, vals = string_key_column(1500, 6, dev=dev)
    assert None in vals and "" in vals
    check_groups([col], [vals], monkeypatch)


def check_pair_key(dev, monkeypatch):
    rng = np.random.default_rng(7)
    n = 1500
    col, svals = string_key_column(n, 8, strings=KEY_STRINGS[:9], dev=dev)
    ids = rng.integers(0, 4, n)
    iv = rng.random(n) > 0.2
    ivals = [int(v) if ok else None for v, ok in zip(ids, iv.tolist())]
    check_groups([PrimColumn("long", torch.from_numpy(ids).to(dev), torch.from_numpy(iv).to(dev)), col],
                 [ivals, svals], monkeypatch)
    # and a (double, long) pair: verify_multi_kernel's double branch
    data, valid, dvals = double_key_column(n, 9)
    check_groups([PrimColumn("double", torch.from_numpy(data.copy()).to(dev), torch.from_numpy(valid).to(dev)),
                  PrimColumn("long", torch.from_numpy(ids).to(dev), torch.from_numpy(iv).to(dev))],
                 [dvals, ivals], monkeypatch)


@pytest.mark.gpu
def test_double_key_gpu(gpu, monkeypatch):
    """hash_f64_kernel + verify_i64_kernel<true>: one NaN group, one zero group, no "collision"."""
    check_double_key(gpu, monkeypatch)


@pytest.mark.gpu
def test_string_key_gpu(gpu, monkeypatch):
    """hash_str_kernel + verify_str_kernel (load_part at every alignment)."""
    check_string_key(gpu, monkeypatch)


@pytest.mark.gpu
def test_pair_key_gpu(gpu, monkeypatch):
    """hash_multi_kernel + verify_multi_kernel: (long, string) and (double, long) with NULLs in either column."""
    check_pair_key(gpu, monkeypatch)


def test_double_key_cpu(monkeypatch):
    check_double_key(CPU, monkeypatch)


def test_string_key_cpu(monkeypatch):
    check_string_key(CPU, monkeypatch)


def test_pair_key_cpu(monkeypatch):
    check_pair_key(CPU, monkeypatch)


def test_exact_groups_normalises_double_keys():
    """The collision fallback itself: NaN is one key, the zeros are one key."""
    data, valid, vals = double_key_column(300, 11)
    g = G._exact_groups([PrimColumn("double", torch.from_numpy(data.copy()), torch.from_numpy(valid))], CPU)
    gid, rep = O.group_ids([(v,) for v in vals], [0])
    assert (g.ngroups, g.gid.tolist(), g.rep.tolist()) == (len(rep), gid, rep)


# ---------------------------------------------------------------------------------------------------------------------
# D. the dense window ring through SQL
# ---------------------------------------------------------------------------------------------------------------------
RING_AGGS = [("c", "count_star", None)] + [(f"{f}_{c}", f, c) for c in ("x", "y")
                                           for f in ("count", "sum", "min", "max", "avg")]


def agg_sql(reqs=RING_AGGS):
    return ", ".join("COUNT(*) AS c" if f == "count_star" else f"{f.upper()}({c}) AS {a}" for a, f, c in reqs)


# grouped by anything but id, the ±2**63 values of different ids meet in one group and the double sum behind AVG(y)
# would depend on the order: those statements leave AVG(y) out (SUM(y) wraps exactly in any order)
KEY_AGGS = [r for r in RING_AGGS if r[0] != "avg_y"]
Q_VALUES = f"SELECT id, {agg_sql()} FROM W GROUP BY id"
Q_DOUBLE = f"SELECT dk, {agg_sql(KEY_AGGS)} FROM W GROUP BY dk"
Q_STRING = f"SELECT sk, {agg_sql(KEY_AGGS)} FROM W GROUP BY sk"
Q_PAIR = f"SELECT id, sk, {agg_sql(KEY_AGGS)} FROM W GROUP BY id, sk"
Q_LONGKEY = f"SELECT sk49, {agg_sql(KEY_AGGS)} FROM W GROUP BY sk49"
NB = 14
LONGKEY_BATCH = 5
RING_STRINGS = [s for s in KEY_STRINGS if len(s.encode("utf-8")) <= 48]
# special ids of the value case: id → (x values, y values) cycled over the group's rows; 104 only in batch 3
RING_SPECIALS = {
    100: ([NAN, 1.0, -2.0], [I_MAX, 1, I_MAX]),
    101: ([INF, 5.0, -INF, -7.25], [I_MIN, -1, I_MIN]),
    102: ([-0.0, 0.0, -0.0], [I_MIN, I_MAX]),
    103: ([None], [None]),                              # argument NULL in every pane
    104: ([-4.5, NAN], [3, I_MAX]),
    105: ([-0.0], [None, 5]),
    106: ([-1.5, -1024.75, -INF, None], [-3, None]),    # negatives only
}


@functools.lru_cache(maxsize=None)
def ring_stream():
    """14 batches of about 300 rows: ids 0-39 with ordinary values (x: multiples of 0.25, 10 % NULL; y: small) plus
    two rows per batch of every special id (one id only in batch 3), a double key, a string key of at most 48 bytes,
    and ``sk49`` = that key with one 49-byte value from batch 5 on.  → [(batch time, CPU table)]."""
    rng = np.random.default_rng(41)
    out = []
    turn = {i: 0 for i in RING_SPECIALS}
    for b in range(NB):
        n = 280 + int(rng.integers(0, 40))
        ids = rng.integers(0, 40, n).tolist()
        x = (rng.integers(-2**20, 2**20, n) * 0.25).tolist()
        x = [None if rng.random() < 0.1 else v for v in x]
        y = [None if rng.random() < 0.1 else int(v) for v in rng.integers(-1000, 1000, n)]
        for sid, (xs, ys) in RING_SPECIALS.items():
            if sid == 104 and b != 3:
                continue
            for _ in range(2):
                at = int(rng.integers(0, len(ids) + 1))
                k = turn[sid]
                turn[sid] += 1
                ids.insert(at, sid)
                x.insert(at, xs[k % len(xs)])
                y.insert(at, ys[k % len(ys)])
        n = len(ids)
        ts = torch.tensor([(100 + b) * S - int(v) for v in rng.integers(0, S - 1, n)], dtype=torch.int64)
        dk, dkv, _ = double_key_column(n, 50 + b)
        sk, svals = string_key_column(n, 70 + b, strings=RING_STRINGS)
        vals49 = list(svals)
        if b >= LONGKEY_BATCH:
            vals49[n // 2] = "y" * 49
        sk49 = strings_from_pylist(vals49, "cpu")

        def prim(dt, vals, tdt):
            return PrimColumn(dt, torch.tensor([0 if v is None else v for v in vals], dtype=tdt),
                              torch.tensor([v is not None for v in vals]))
        cols = [PrimColumn("timestamp", ts), PrimColumn("long", torch.tensor(ids, dtype=torch.int64)),
                PrimColumn("double", torch.from_numpy(dk.copy()), torch.from_numpy(dkv)), sk, sk49,
                prim("double", x, torch.float64), prim("long", y, torch.int64)]
        out.append(((100 + b) * S, Table(["ts", "id", "dk", "sk", "sk49", "x", "y"], cols, n, "cpu")))
    return out


def window_rows(view):
    """The materialised window's rows pulled to Python → {column: list}."""
    mat = Table(view.names, view.columns, view.length, view._device).to("cpu")
    return {n: c.to_pylist() for n, c in zip(mat.names, mat.columns)}


def check_statement(q, keys, got, win, where):
    names = list(keys) + ["x", "y"]
    rows = list(zip(*[win[c] for c in names]))
    out = got.to_pylist()
    reqs = [(a, f, None if c is None else names.index(c)) for a, f, c in RING_AGGS if not out or a in out[0]]
    assert len(reqs) >= len(KEY_AGGS)
    want = O.group_by(rows, list(range(len(keys))), reqs)
    have = {O.key_tuple(r[k] for k in keys): r for r in out}
    assert len(have) == len(out), (where, "a key came out twice")
    assert set(have) == set(want), (where, set(have) ^ set(want))
    bad = [(k, a, have[k][a], w[a]) for k, w in want.items() for a in w if not O.same(have[k][a], w[a])]
    assert not bad, (where, bad[:8])


def run_ring(stream, statements, dev, store, each=None):
    for b, (T, tbl) in enumerate(stream):
        views, _ = store.process(tbl.to(dev), T, S)
        win = window_rows(views["W"])
        for q, keys in statements:
            cat = Catalog()
            cat.register("W", views["W"])
            got = run_sql(q, cat, EvalContext(now_us=0, device=dev))
            check_statement(q, keys, got, win, (b, q[:24]))
            if each is not None:
                each(b, q, win)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [16, 2])
def test_ring_values(gpu, monkeypatch, block):
    """win_insert / agg_multi_kernel into pane slots / win_combine<false> (and <true> for complete blocks with
    BLOCK = 2) / win_emit over NaN, ±inf, ±0.0, NULL-only and ±2**63 arguments; id 104 lives in one pane only."""
    set_caps(monkeypatch, 8192, 8192, block=block)
    store = new_store(6)
    seen = {}

    def each(b, q, win):
        d = next(iter(dense_states(store).values()), None)      # (no state before the window's first rows)
        seen[b] = len(d.blocks) if d is not None else 0

    run_ring(ring_stream(), [(Q_VALUES, ["id"])], gpu, store, each)
    (d,) = dense_states(store).values()
    assert not d.disabled and d.disabled_reason is None
    if block == 2:
        assert max(seen.values()) >= 1


@pytest.mark.gpu
def test_ring_keys(gpu, monkeypatch):
    """The ring's dictionary (win_insert_kernel store_key / key_differs, win_emit's key columns) over a double key
    (norm_f64_bits), a string key up to the 48-byte slot, and a (long, string) pair, NULLs in all of them."""
    set_caps(monkeypatch, 8192, 8192)
    store = new_store(6)
    run_ring(ring_stream(), [(Q_DOUBLE, ["dk"]), (Q_STRING, ["sk"]), (Q_PAIR, ["id", "sk"])], gpu, store)
    dense = dense_states(store)
    assert len(dense) == 3
    assert not any(d.disabled for d in dense.values())


@pytest.mark.gpu
def test_ring_key_too_long(gpu, monkeypatch):
    """A 49-byte key arrives in batch 5 and enters the window once the watermark has passed it: the statement then
    leaves the dense path saying why, and that batch and every later one still equal the oracle (the paned path
    answers them)."""
    set_caps(monkeypatch, 8192, 8192)
    store = new_store(6)
    state = {}

    def each(b, q, win):
        for d in dense_states(store).values():
            state[b] = (d.disabled, d.disabled_reason, "y" * 49 in win["sk49"])

    run_ring(ring_stream(), [(Q_LONGKEY, ["sk49"])], gpu, store, each)
    first = min(b for b, s in state.items() if s[2])              # the batch whose window first holds the key
    assert LONGKEY_BATCH <= first <= NB - 3
    assert all(state[b][:2] == (False, None) for b in state if b < first) and first - 1 in state
    assert all(state[b][:2] == (True, "key too long") for b in range(first, NB))


def test_window_statements_cpu():
    """The same stream and statements through the CPU evaluator (the oracle of the older ring tests)."""
    run_ring(ring_stream(), [(Q_VALUES, ["id"]), (Q_DOUBLE, ["dk"]), (Q_STRING, ["sk"]), (Q_PAIR, ["id", "sk"]),
                             (Q_LONGKEY, ["sk49"])], CPU, new_store(6))


@functools.lru_cache(maxsize=None)
def carry_stream():
    rng = np.random.default_rng(43)
    out = []
    for b in range(NB):
        ids = np.arange(4500) if b == 0 else rng.integers(0, 265, 300) * 17
        ids = rng.permutation(ids)
        n = len(ids)
        ts = torch.tensor([(100 + b) * S - int(v) for v in rng.integers(0, S - 1, n)], dtype=torch.int64)
        x = torch.from_numpy(rng.integers(-2**20, 2**20, n) * 0.25)
        y = torch.from_numpy(rng.integers(-1000, 1000, n))
        cols = [PrimColumn("timestamp", ts), PrimColumn("long", torch.from_numpy(ids.astype(np.int64))),
                PrimColumn("double", x, torch.from_numpy(rng.random(n) > 0.1)), PrimColumn("long", y)]
        out.append(((100 + b) * S, Table(["ts", "id", "x", "y"], cols, n, "cpu")))
    return out


@pytest.mark.gpu
def test_ring_compaction_carry(gpu, monkeypatch):
    """win_compact_kernel's running base across its 4096-group chunks: the dictionary keeps all 4500 ids of batch 0
    (no rebuild: the group counter stays at 4500), and once batch 0 has left the window only every 17th of them has
    rows, on both sides of group 4096."""
    set_caps(monkeypatch, 8192, 8192)
    store = new_store(6)
    after = {}

    def each(b, q, win):
        for d in dense_states(store).values():
            after[b] = (d.disabled, d.rebuilds, int(d.scal[0].item()), len(win["id"]))

    run_ring(carry_stream(), [(Q_VALUES, ["id"])], gpu, store, each)
    held = [b for b in after if after[b][3] >= 4500]             # batch 0 inside the window
    gone = [b for b in after if b > max(held) and after[b][3] > 0]
    assert held and len(gone) >= 3, after
    assert all(after[b][:3] == (False, 0, 4500) for b in gone), after
