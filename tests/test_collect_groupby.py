"""collect_list / collect_set per group for primitive and string arguments: slot matrices built on the table's device
(``query._collect_slots``; on the GPU one launch of collect.hip's ``dxa_collect_scatter``), against the row-by-row host
loop ``query._collect_host``.

Every statement runs twice over the same table: as the engine runs it, and with ``_collect_slots`` replaced by the host
loop.  The two results must hold the same lists, order included — ``_same`` below: NaN equals NaN, and a zero keeps
its sign — and the same ``present`` decision.  The one intended difference is the set's equality, GROUP BY's: several NaNs
of one group are one value, where the host loop (``nan != nan``) keeps each; groups with more than one NaN are left out
of the set's oracle comparison and have a test of their own.

The GPU tests run the same tables on the device and compare with the CPU result, element for element.
"""
import decimal
import math
import random

import pytest
import torch

from dxa.engine import query as Q
from dxa.engine.column import PrimColumn, StrColumn, Table, column_from_pylist
from dxa.engine.decimal import DecimalType
from dxa.engine.expr import EvalContext
from dxa.engine.query import Catalog, QueryError, run_sql

NAN = float("nan")


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


def _catalog(cols, device):
    """``cols``: name → (dtype, values)."""
    n = len(next(iter(cols.values()))[1])
    t = Table(list(cols), [column_from_pylist(v, dt, device) for dt, v in cols.values()], n, device)
    c = Catalog()
    c.register("T", t)
    return c


def _run(cols, sql, device="cpu", host=False):
    """The statement's result table; ``host``: with the host loop in place of the slot path."""
    real = Q._collect_slots
    if host:
        Q._collect_slots = Q._collect_host
    try:
        return run_sql(sql, _catalog(cols, device), EvalContext(now_us=0, device=torch.device(device)))
    finally:
        Q._collect_slots = real


# -- seeded tables ----------------------------------------------------------------------------------------------------

VALUES = {
    "long": ("long", lambda r: r.choice([None, -3, 0, 7, 7, 1 << 40, -(1 << 62), r.randrange(20)])),
    "int": ("int", lambda r: r.choice([None, -3, 0, 7, 2 ** 31 - 1, -2 ** 31, r.randrange(20)])),
    "double": ("double", lambda r: r.choice([None, NAN, -0.0, 0.0, 1.5, -2.25, float("inf"), r.randrange(6) / 4])),
    "boolean": ("boolean", lambda r: r.choice([None, True, False])),
    "timestamp": ("timestamp", lambda r: r.choice([None, 0, 1_700_000_000_123_456, r.randrange(10) * 1_000_000])),
    "decimal(10,2)": (DecimalType(10, 2), lambda r: r.choice([None, decimal.Decimal("-0.01"),
                                                              decimal.Decimal("12345678.90"),
                                                              decimal.Decimal(r.randrange(8)) / 4])),
    "decimal(30,4)": (DecimalType(30, 4), lambda r: r.choice([None, decimal.Decimal("-12345678901234567890123456.7891"),
                                                              decimal.Decimal("98765432109876543210.0001"),
                                                              decimal.Decimal(r.randrange(8)) / 4])),
    "string": ("string", lambda r: r.choice([None, "", "a", "é√", "日本語", "a", "x" * 40, str(r.randrange(8))])),
}


def _typed_table(kind, n=400, groups=11, seed=3):
    dt, gen = VALUES[kind]
    r = random.Random(seed)
    return {"g": ("long", [r.choice([None] + list(range(groups))) for _ in range(n)]),
            "v": (dt, [gen(r) for _ in range(n)])}


def _sized_table(sizes, kind):
    """One group per entry of ``sizes``, rows interleaved; every 7th argument is NULL and values repeat."""
    dt, gen = VALUES[kind]
    r = random.Random(len(sizes))
    keys = [g for g, s in enumerate(sizes) for _ in range(s)]
    r.shuffle(keys)
    vals = [None if i % 7 == 3 else gen(r) for i in range(len(keys))]
    return {"g": ("long", keys), "v": (dt, vals)}


def _shape_tables():
    r = random.Random(9)
    n = 300
    out = {
        "one_group": {"g": ("long", [4] * n), "v": ("long", [r.choice([None, r.randrange(9)]) for _ in range(n)])},
        "own_group": {"g": ("long", list(range(n))), "v": ("long", [r.choice([None, i % 5]) for i in range(n)])},
        "all_null_group": {"g": ("long", [i % 3 for i in range(n)]),
                           "v": ("string", [None if i % 3 == 1 else r.choice(["p", "q", ""]) for i in range(n)])},
        "all_null": {"g": ("long", [i % 3 for i in range(30)]), "v": ("long", [None] * 30)},
        "sizes_long": _sized_table([1, 63, 64, 65, 5000], "long"),
        "sizes_string": _sized_table([1, 63, 64, 65, 300], "string"),
        "groups_20000": {"g": ("long", [i % 20000 for i in range(50000)]),
                         "v": ("long", [None if i % 11 == 0 else i % 4 for i in range(50000)])},
        "equal_lengths": {"g": ("long", [i % 50 for i in range(400)]), "v": ("double", [float(i) for i in range(400)])},
        "equal_lengths_string": {"g": ("long", [i // 3 for i in range(300)]),
                                 "v": ("string", [str(i) for i in range(300)])},
    }
    return out


# the double table has more, smaller groups, so that some hold several NaNs and some at most one
TABLES = {**{f"type_{k}": _typed_table(k, groups=60 if k == "double" else 11) for k in VALUES}, **_shape_tables()}
SQL = "SELECT g, collect_list(v) AS l, collect_set(v) AS s FROM T GROUP BY g"
_CPU = {}


def _cpu_result(name):
    """The CPU slot path's result for a table: computed once, shared by the oracle and the GPU comparisons."""
    if name not in _CPU:
        t = _run(TABLES[name], SQL)
        _CPU[name] = (t, t.to_pylist())
    return _CPU[name]


def _multi_nan_groups(cols):
    seen = {}
    for g, v in zip(cols["g"][1], cols["v"][1]):
        if isinstance(v, float) and math.isnan(v):
            seen[g] = seen.get(g, 0) + 1
    return {g for g, c in seen.items() if c > 1}


# -- CPU: the slot path against the host loop -------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(TABLES))
def test_matches_host_loop(name):
    table, got = _cpu_result(name)
    want_table = _run(TABLES[name], SQL, host=True)
    want = want_table.to_pylist()
    skip = _multi_nan_groups(TABLES[name])
    if name == "type_double":
        assert skip and len(skip) < len(want)                 # both kinds of group are in the table
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a["g"] == b["g"]
        assert _same(a["l"], b["l"]), (name, a["g"], a["l"], b["l"])
        if a["g"] not in skip:
            assert _same(a["s"], b["s"]), (name, a["g"], a["s"], b["s"])
        assert a["l"] is not None and a["s"] is not None
    for col in ("l", "s"):
        new, old = table.column(col), want_table.column(col)
        assert new.dtype == old.dtype
        assert new.valid is None
        if not (col == "s" and skip):
            assert (new.present is None) == (old.present is None), (name, col)
            assert len(new.elements) == len(old.elements)


def test_present_mask_only_where_lengths_differ():
    for name in ("equal_lengths", "equal_lengths_string"):
        table, got = _cpu_result(name)
        assert table.column("l").present is None and table.column("s").present is None
        assert all(e.valid is None for e in table.column("l").elements)
        assert len({len(r["l"]) for r in got}) == 1
    table, got = _cpu_result("sizes_long")
    assert table.column("l").present is not None
    counts = {}
    for g, v in zip(TABLES["sizes_long"]["g"][1], TABLES["sizes_long"]["v"][1]):
        counts[g] = counts.get(g, 0) + (v is not None)
    assert {r["g"]: len(r["l"]) for r in got} == counts and max(counts.values()) > 3000
    table, got = _cpu_result("all_null")
    assert [r["l"] for r in got] == [[], [], []] and [r["s"] for r in got] == [[], [], []]
    assert tuple(table.column("l").present.shape) == (3, 1) and not bool(table.column("l").present.any())


@pytest.mark.parametrize("kind", ["long", "string", "double", "decimal(30,4)"])
@pytest.mark.parametrize("sql", ["SELECT g, collect_list(v) AS l, collect_set(v) AS s FROM T WHERE g > 99 GROUP BY g",
                                 "SELECT collect_list(v) AS l, collect_set(v) AS s FROM T WHERE g > 99"])
def test_zero_rows(kind, sql):
    cols = _typed_table(kind, n=20)
    got, want = _run(cols, sql), _run(cols, sql, host=True)
    assert got.to_pylist() == want.to_pylist()
    assert got.to_pylist() == ([] if "GROUP BY" in sql else [{"l": [], "s": []}])
    for col in ("l", "s"):
        assert got.column(col).dtype == want.column(col).dtype
        assert tuple(got.column(col).present.shape) == tuple(want.column(col).present.shape)


def test_set_collapses_nans_and_keeps_first_zero():
    cols = {"g": ("long", [1, 1, 1, 1, 2, 2, 2, 1]), "v": ("double", [NAN, 1.0, NAN, NAN, -0.0, 0.0, NAN, 1.0])}
    got = {r["g"]: r for r in _run(cols, SQL).to_pylist()}
    assert _same(got[1]["s"], [NAN, 1.0]) and _same(got[2]["s"], [-0.0, NAN])
    assert _same(got[1]["l"], [NAN, 1.0, NAN, NAN, 1.0]) and _same(got[2]["l"], [-0.0, 0.0, NAN])


@pytest.mark.parametrize("name", ["type_double", "type_string", "type_decimal(30,4)", "type_long", "sizes_string"])
def test_size_of_set_is_count_distinct(name):
    rows = _run(TABLES[name], "SELECT g, size(collect_set(v)) AS a, count(DISTINCT v) AS b, "
                              "size(collect_list(v)) AS c, count(v) AS d FROM T GROUP BY g").to_pylist()
    assert rows and all(r["a"] == r["b"] and r["c"] == r["d"] for r in rows), rows


def test_composes_with_explode_and_sort_array():
    cols = _typed_table("long")
    got = _run(cols, "SELECT g, explode(collect_list(v)) AS x FROM T GROUP BY g").to_pylist()
    want = [(g, v) for g, v in zip(cols["g"][1], cols["v"][1]) if v is not None]
    key = lambda p: (p[0] is None, p[0] or 0, p[1])
    assert sorted(((r["g"], r["x"]) for r in got), key=key) == sorted(want, key=key)
    got = _run(cols, "SELECT g, sort_array(collect_set(v)) AS x FROM T GROUP BY g").to_pylist()
    sets = {}
    for g, v in zip(cols["g"][1], cols["v"][1]):
        sets.setdefault(g, set())
        if v is not None:
            sets[g].add(v)
    assert {r["g"]: r["x"] for r in got} == {g: sorted(s) for g, s in sets.items()}


def test_slot_cap(monkeypatch):
    monkeypatch.setattr(Q, "COLLECT_MAX_SLOTS", 1000)
    cols = _sized_table([1, 2, 800], "long")                 # the long group keeps over 500 non-NULL rows, × 3 groups
    with pytest.raises(QueryError, match=r"collect_list: .* slots"):
        _run(cols, "SELECT g, collect_list(v) AS l FROM T GROUP BY g")
    assert len(_run(cols, "SELECT g, collect_set(v) AS s FROM T GROUP BY g").to_pylist()) == 3   # few values: fits


def test_nested_arguments_keep_the_host_loop(monkeypatch):
    cols = _typed_table("long", n=40)
    calls = []
    real = Q._collect_host
    monkeypatch.setattr(Q, "_collect_host", lambda *a: calls.append(1) or real(*a))
    sql = "SELECT g, collect_list(array(v, 1)) AS l FROM T GROUP BY g"
    got = _run(cols, sql).to_pylist()
    assert calls and len(got) == 12


# -- GPU: the same tables through dxa_collect_scatter -----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLES))
def test_gpu_equals_cpu(name, gpu):
    cpu_table, want = _cpu_result(name)
    table = _run(TABLES[name], SQL, "cuda")
    got = table.to_pylist()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert _same(a, b), (name, a["g"])
    for col in ("l", "s"):
        assert table.column(col).device.type == "cuda"
        assert (table.column(col).present is None) == (cpu_table.column(col).present is None)
        assert len(table.column(col).elements) == len(cpu_table.column(col).elements)


@pytest.mark.gpu
def test_gpu_zero_rows_and_nan_collapse(gpu):
    cols = _typed_table("string", n=20)
    for sql in ("SELECT g, collect_list(v) AS l FROM T WHERE g > 99 GROUP BY g",
                "SELECT collect_list(v) AS l, collect_set(v) AS s FROM T WHERE g > 99"):
        assert _run(cols, sql, "cuda").to_pylist() == _run(cols, sql).to_pylist()
    cols = {"g": ("long", [1, 1, 1, 1, 2, 2, 2, 1]), "v": ("double", [NAN, 1.0, NAN, NAN, -0.0, 0.0, NAN, 1.0])}
    got = {r["g"]: r for r in _run(cols, SQL, "cuda").to_pylist()}
    assert _same(got[1]["s"], [NAN, 1.0]) and _same(got[2]["s"], [-0.0, NAN])


@pytest.mark.gpu
def test_gpu_collect_never_reads_the_argument_on_the_host(gpu, monkeypatch):
    r = random.Random(2)
    n = 3000
    cols = {"g": ("long", [r.randrange(40) for _ in range(n)]),
            "v": ("long", [r.choice([None, r.randrange(100)]) for _ in range(n)]),
            "s": ("string", [r.choice([None, "", "dev-%d" % r.randrange(30)]) for _ in range(n)])}
    sql = "SELECT g, collect_list(v) AS l, collect_set(s) AS s FROM T GROUP BY g"
    want = _run(cols, sql).to_pylist()
    cat = _catalog(cols, "cuda")

    def refuse(self):
        raise AssertionError("to_pylist during collect")
    with monkeypatch.context() as m:
        m.setattr(PrimColumn, "to_pylist", refuse)
        m.setattr(StrColumn, "to_pylist", refuse)
        table = run_sql(sql, cat, EvalContext(now_us=0, device=gpu))
    got = table.to_pylist()
    assert len(got) == 40 and all(_same(a, b) for a, b in zip(got, want))
