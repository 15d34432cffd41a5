"""MIN / MAX over strings on the device: the arg-extreme kernel (dxa/ops/csrc/str_minmax.hip), ``groupby.aggregate``'s
string path, and the CPU side of the dense ring's string line (window_dense.py ``pack_str_words`` /
``unpack_str_words`` / ``plan_layout``).  String order is unsigned byte order of the UTF-8 bytes, a proper prefix
first — Python's ``str`` order on valid UTF-8, which the CPU evaluator (the oracle) uses.  Everything compares
exactly."""
import numpy as np
import pytest
import torch

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from tests.string_sets import STRINGS, draw
from tests.window_dense_support import Comparison, aggs_of, answer, layout_of, with_syncs_counted

BITS = Comparison("bits", order_by="id")
Q = "SELECT id, COUNT(name) AS c, MIN(name) AS mn, MAX(name) AS mx FROM W GROUP BY id"
LONG49, LONG300 = "5" * 49, "7" * 300


def table_of(ids, names):
    n = len(ids)
    cols = [PrimColumn("long", torch.tensor(np.asarray(ids), dtype=torch.int64)), strings_from_pylist(names, "cpu"),
            PrimColumn("long", torch.arange(n, dtype=torch.int64) * 7 % 1013)]
    return Table(["id", "name", "longcol"], cols, n, "cpu")


def many_groups():
    """2,200 rows over 1,100 ids — both sides of the kernel's 1,024-id LDS bound, two workgroups — with values of
    the shared set and NULLs; id 7 has only NULLs, id 8 only equal strings, id 1,050 likewise above the bound."""
    rng = np.random.default_rng(5)
    ids = np.repeat(np.arange(1100), 2)
    rng.shuffle(ids)
    names = draw(rng, len(ids))
    for i, g in enumerate(ids):
        if g == 7:
            names[i] = None
        elif g in (8, 1050):
            names[i] = "same"
    return ids, names


def one_group(descending):
    """4,096 rows of one group in ascending (or descending) order, a 49-byte and a 300-byte value among them."""
    names = sorted([f"{20 * i:05d}" for i in range(4094)] + [LONG49, LONG300])
    assert 0 < names.index(LONG49) < names.index(LONG300) < 4095
    return np.zeros(4096, dtype=np.int64), names[::-1] if descending else names


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_word_packing_round_trip_and_order():
    """``unpack(pack(s)) == s`` for the set and 2,000 random byte strings of 0-48 bytes; the tuple order of the packed
    words is the byte order of the values (reversed for MIN) on 2,000 random pairs and all pairs of the set; every
    packed value is above the identity."""
    from dxa.engine.window_dense import pack_str_words, unpack_str_words
    rng = np.random.default_rng(11)
    # short alphabets and shared prefixes, so that random pairs differ late, tie, or are prefixes of one another
    rand = [bytes(rng.choice([0, 1, 0x7f, 0x80, 0xff, 97], int(rng.integers(0, 49))).astype(np.uint8))
            for _ in range(2000)]
    fixed = [s.encode() for s in STRINGS]
    identity = (-(1 << 63),) * 7
    for b in fixed + rand:
        for mn in (False, True):
            w = pack_str_words(b, mn)
            assert len(w) == 7 and all(-(1 << 63) <= x < 1 << 63 for x in w)
            assert unpack_str_words(w, mn) == b and w > identity
    assert unpack_str_words(identity) is None and unpack_str_words(identity, True) is None
    pairs = [(a, b) for a in fixed for b in fixed]
    pairs += [(rand[int(i)], rand[int(j)]) for i, j in rng.integers(0, len(rand), (2000, 2))]
    for a, b in pairs:
        assert (pack_str_words(a) < pack_str_words(b)) == (a < b), (a, b)
        assert (pack_str_words(a, True) < pack_str_words(b, True)) == (a > b), (a, b)
        assert (pack_str_words(a) == pack_str_words(b)) == (a == b), (a, b)
    assert "ab".encode() < "ab\x00".encode() and "é".encode() > b"zz"


def test_str_column_of_words():
    """The emit side on the CPU: finished words (the mapping undone) → a string column, NULL where the count is 0."""
    from dxa.engine.window_dense import pack_str_words, str_column_of
    vals = [s.encode() for s in STRINGS] + [None]
    raw = [pack_str_words(b or b"") for b in vals]
    words = [torch.tensor([w[q] ^ -(1 << 63) for w in raw], dtype=torch.int64) for q in range(6)]
    lens = torch.tensor([w[6] for w in raw], dtype=torch.int64)
    ok = torch.tensor([b is not None for b in vals])
    assert str_column_of(words, lens, ok).to_pylist() == STRINGS + [None]


def test_layout_of_string_lines():
    """A string MIN / MAX is one op-8 line and 7 ``fin`` rows, shares the argument's count slot with COUNT(name) and
    has the partial states "v" / "cnt"; a layout without strings has no such line and no descriptor; nine string jobs
    are too many."""
    from dxa.engine.window_dense import Ineligible
    from dxa.ops.groupby import _F_I64, _F_NOT, _F_STRW, _MA_STRKEY
    names = [f"s{k}" for k in range(5)]
    t = Table(["id", "temp", *names],
              [PrimColumn("long", torch.zeros(2, dtype=torch.int64)), PrimColumn("double", torch.zeros(2).double()),
               *[strings_from_pylist(["a", "b"], "cpu") for _ in names]], 2, "cpu")
    aggs = aggs_of("COUNT(*)", "COUNT(s0)", "MAX(s0)", "AVG(temp)")
    _reqs, types, L = layout_of(aggs, t)
    assert types[[k for k in types if "s0" in str(k)][0]] == ("string", False)
    assert L["line_ops"].count(_MA_STRKEY) == 1 and L["stride"] == 8 * len(L["line_ops"])
    line = 8 * L["line_ops"].index(_MA_STRKEY)
    assert L["strdesc"][line:line + 8] == [1, 2, 3, 4, 5, 6, 7, 0] and sum(L["strdesc"]) == 28
    assert [(inv, w) for _k, inv, w in L["strargs"]] == [(False, line)]
    plan = {p[1]: p for p in L["plan"]}
    (r0, nr), = [r for p, r in zip(L["plan"], L["rows"]) if p[1] == "str"]
    cnt = [p for p in L["plan"] if p[1] == "count"][1]
    assert nr == 7 and plan["str"][3] == cnt[2] and plan["str"][4] == "string"
    cw = L["fin"][r0][2]
    assert L["fin"][r0:r0 + 7] == [(_F_STRW, line + q, cw) for q in range(6)] + [(_F_I64, line + 6, cw)]
    (ak,) = [p[0] for p in L["plan"] if p[1] == "str"]
    assert set(L["pfin"][ak]) == {"v", "cnt"} and L["pfin"][ak]["v"] == L["fin"][r0:r0 + 7]
    # MIN: the same line shape with every word complemented
    _r, _t, Lmin = layout_of(aggs_of("MIN(s0)", "MAX(s0)"), t)
    assert Lmin["line_ops"].count(_MA_STRKEY) == 2 and sorted(inv for _k, inv, _w in Lmin["strargs"]) == [False, True]
    assert {f[0] for f in Lmin["fin"]} == {_F_STRW, _F_STRW | _F_NOT, _F_I64, _F_I64 | _F_NOT}
    # no strings: no line, no descriptor
    _r, _t, Lnone = layout_of(aggs_of("COUNT(*)", "MAX(temp)", "AVG(temp)"), t)
    assert _MA_STRKEY not in Lnone["line_ops"] and "strdesc" not in Lnone and "strargs" not in Lnone
    # eight jobs pass the job bound and meet the row's 64 words (their lines fill it); a ninth job meets the job bound
    eight = [f"{f}({nm})" for nm in names[:4] for f in ("MIN", "MAX")]
    with pytest.raises(Ineligible, match="^too many aggregates$"):
        layout_of(aggs_of(*eight), t)             # 8 lines and the count line: more than 64 words
    with pytest.raises(Ineligible, match="^too many string arguments$"):
        layout_of(aggs_of(*eight, "MIN(s4)"), t)
    # everything else over a string keeps its reason
    with pytest.raises(Ineligible, match="^sum type$"):
        layout_of(aggs_of("SUM(s0)"), t)


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _no_host_loop(monkeypatch):
    from dxa.ops import groupby

    def refuse(*a, **k):
        raise AssertionError("string MIN / MAX took the host loop")
    monkeypatch.setattr(groupby, "_host_minmax", refuse)


@pytest.mark.gpu
def test_group_by_many_groups(gpu, monkeypatch):
    """MIN and MAX per id equal the CPU evaluator exactly, without the host loop, and the statement synchronises no
    more often than the same statement over a long column."""
    ids, names = many_groups()
    t = table_of(ids, names)
    want = BITS.rows(answer(Q, t))
    _no_host_loop(monkeypatch)
    dev_t = t.to(gpu)
    BITS(BITS.rows(answer(Q, dev_t, gpu)), want, "many groups")
    by_id = {r["id"]: r for r in want[0]}
    assert by_id[7]["mn"] is None and by_id[7]["mx"] is None and by_id[8]["mx"] == "same" == by_id[1050]["mn"]
    q_str = "SELECT id, MAX(name) AS mx FROM W GROUP BY id"
    q_long = "SELECT id, MAX(longcol) AS mx FROM W GROUP BY id"
    for q in (q_str, q_long):
        answer(q, dev_t, gpu)
    _out, syncs_str = with_syncs_counted(lambda: answer(q_str, dev_t, gpu))
    _out, syncs_long = with_syncs_counted(lambda: answer(q_long, dev_t, gpu))
    assert syncs_str <= syncs_long, (syncs_str, syncs_long)


@pytest.mark.gpu
@pytest.mark.parametrize("descending", [False, True])
def test_group_by_one_group(gpu, monkeypatch, descending):
    """4,096 rows of one group arriving in ascending and in descending order (every row, or only the first, beats the
    best before it), values of 49 and 300 bytes among them: strings may have any length here."""
    t = table_of(*one_group(descending))
    # and with the long values as the extremes
    q = "SELECT id, MIN(name) AS mn, MAX(name) AS mx FROM W WHERE name >= '55541' AND name <= '7777z' GROUP BY id"
    want, want_long = BITS.rows(answer(Q, t)), BITS.rows(answer(q, t))
    assert want[0][0]["mx"] == "81860" and want[0][0]["mn"] == "00000"
    assert want_long[0][0]["mn"] == LONG49 and want_long[0][0]["mx"] == LONG300
    _no_host_loop(monkeypatch)
    BITS(BITS.rows(answer(Q, t.to(gpu), gpu)), want, "one group")
    BITS(BITS.rows(answer(q, t.to(gpu), gpu)), want_long, "long extremes")


@pytest.mark.gpu
@pytest.mark.parametrize("copies", [1, 10])
def test_argext_rows(gpu, copies):
    """The kernel itself: the winning row index per group — the smallest index among equal strings — under a keep
    mask and with ids outside [0, ngroups), which are skipped; -1 for a group without a row.  2,200 rows are 2
    workgroups at the kernel's 8 rows per lane; ten copies of them — every string now ties with its copies, across
    workgroups — are 11."""
    from dxa.ops import native as N
    from dxa.ops.groupby import str_argext
    assert 0 < N.lib().dxa_win_m2_lds_groups() < 1100      # (the kernel's LDS bound: one constant for all such passes)
    ids, names = many_groups()
    rng = np.random.default_rng(6)
    ids, names = np.tile(ids, copies), names * copies
    ids[rng.random(len(ids)) < 0.05] = -1
    ids[rng.random(len(ids)) < 0.05] = 1100
    keep = rng.random(len(ids)) > 0.2
    col = strings_from_pylist(names, "cpu").to(gpu)
    gid = torch.tensor(ids, dtype=torch.int32, device=gpu)
    for func in ("min", "max"):
        for mask in (None, keep):
            want = [-1] * 1100
            for i, (g, s) in enumerate(zip(ids, names)):
                if s is None or not 0 <= g < 1100 or (mask is not None and not mask[i]):
                    continue
                b = want[g]
                if b < 0 or (s.encode() > names[b].encode() if func == "max" else s.encode() < names[b].encode()):
                    want[g] = i
            m = None if mask is None else torch.tensor(mask, device=gpu).view(torch.uint8)
            got = str_argext(gid, len(ids), 1100, col, func, m).cpu().tolist()
            assert got == want, (func, mask is not None)
