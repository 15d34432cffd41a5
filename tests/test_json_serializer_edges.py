"""The row serializers at their edges, against a pure-Python reference.

Every row the engine emits goes through ``dxa/ops/csrc/json_serialize.hip`` and the packed emitter in
``dxa_emit.h`` (GPU) or ``host_serialize.cpp`` (host).  The two share a node model and formatting code, so here both
are compared, byte for byte and line length for line length, with ``dxa.engine.serialize.table_to_json_lines_py``:
``json.dumps`` for strings, the ``repr``-based ``java_double_str`` for doubles, ``datetime`` for dates and timestamps.
It never calls the native library.  Each table is checked twice: the host serializer on the CPU (no marker, keeps the
reference honest where there is no GPU) and the device serializer (``gpu``).

The tables aim at what a lane-per-row text kernel gets wrong: records shorter than one 16-byte emitter word and
records at every (start, length) residue mod 16, the 8-byte escape scan at every load alignment with the special byte
at every position, digit-count boundaries of the integer and double formatters, floor division of negative
timestamps, null containers in every mode, empty segments of a render group, and the limits of the kernels (64 KiB
of render tables in LDS, 16 segments, 30 nesting levels), past which a table must still render.

String columns whose layout matters are built directly as ``StrColumn(arena, starts, lens)`` and moved to the GPU
tensor by tensor (``_to_dev``): ``StrColumn.to`` would repack the arena and lose the layout.

Known and left alone:

* Years <= 0 (and >= 10000): the host serializer writes ``%04lld`` (``-001``), the device ``put_i64`` (``-1``), and
  Python's ``datetime`` raises.  Such years are kept out of the inputs.
* ``Double.MIN_VALUE``: device, host and reference all write the shortest digits (``5.0E-324``), Java writes
  ``4.9E-324``.
"""
import datetime as dt
import decimal
import functools
import math
import random
import string

import numpy as np
import pytest
import torch

from dxa.engine.column import (ArrayColumn, ConstColumn, JsonColumn, PrimColumn, StrColumn, StructColumn, Table,
                               column_from_pylist)
from dxa.engine.decimal import parse_decimal_type
from dxa.engine.functions import format_timestamp_us
from dxa.engine.serialize import table_to_json_lines_py
from dxa.engine.types import MapType
from dxa.ops import serialize as S

Dec = decimal.Decimal
EPOCH = dt.datetime(1970, 1, 1)


# ----------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------

class _Ref:
    """The reference rendering of a table: encoded lines, their lengths and the newline-terminated blob."""

    def __init__(self, table):
        self.lines = [ln.encode("utf-8") for ln in table_to_json_lines_py(table)]
        self.lens = [len(ln) for ln in self.lines]
        self.blob = b"".join(ln + b"\n" for ln in self.lines)


def _check(jl, ref):
    """``jl`` (a JsonLines) equals the reference: every line's bytes and every line length."""
    lens, blob = jl.lens.tolist(), jl.blob
    assert len(lens) == len(ref.lines)
    if lens != ref.lens or blob != ref.blob:                # name the first line that differs
        off = 0
        for i, (n, want) in enumerate(zip(lens, ref.lines)):
            got = blob[off:off + n]
            assert got == want and blob[off + n:off + n + 1] == b"\n", f"line {i}: got {got!r}, want {want!r}"
            off += n + 1
    assert lens == ref.lens
    assert blob == ref.blob


def _host(table):
    st = S.Staged(table)
    assert not st.gpu
    return st.render()


def _to_dev(col, device):
    """The column on ``device`` with its string arenas copied as they are (same starts, same layout)."""
    if isinstance(col, Table):
        return Table(col.names, [_to_dev(c, device) for c in col.columns], col.length, device)
    v = None if col.valid is None else col.valid.to(device)
    if isinstance(col, ConstColumn):
        return col.to(device)
    if isinstance(col, StrColumn):
        return type(col)(col.arena.to(device), col.starts.to(device), col.lens.to(device), v, col.dtype)
    if isinstance(col, StructColumn):
        return StructColumn(col.names, [_to_dev(c, device) for c in col.children], col.length, v, col.is_map,
                            col.dtype, device)
    if isinstance(col, ArrayColumn):
        return ArrayColumn([_to_dev(c, device) for c in col.elements], col.length, v, col.drop_nulls, device)
    return PrimColumn(col.dtype, col.data.to(device), v)


def _mask(flags):
    return torch.tensor(list(flags), dtype=torch.bool)


def _prim(vals, dtype="long"):
    tdt = torch.float64 if dtype == "double" else torch.bool if dtype == "boolean" else torch.int64
    data = torch.tensor([0 if v is None else v for v in vals], dtype=tdt)
    valid = _mask(v is not None for v in vals) if any(v is None for v in vals) else None
    return PrimColumn(dtype, data, valid)


class _Arena:
    """A hand-laid string arena: rows are views (start, length) into one byte buffer."""

    def __init__(self):
        self.buf, self.starts, self.lens = bytearray(), [], []

    def add(self, data: bytes, offset=None):
        """Append ``data`` as a new row; with ``offset`` its start is padded to that residue mod 8."""
        if offset is not None:
            self.buf += b"#" * ((offset - len(self.buf)) % 8)
        self.view(len(self.buf), len(data))
        self.buf += data
        return self.starts[-1]

    def add_at_end(self, data: bytes, multiple: int):
        """Append ``data`` so that it ends at the arena's final byte and the arena's size is a multiple of
        ``multiple``."""
        self.buf += b"#" * (-(len(self.buf) + len(data)) % multiple)
        return self.add(data)

    def view(self, start, n):
        self.starts.append(start)
        self.lens.append(n)

    def column(self, cls=StrColumn):
        assert all(0 <= s and s + n <= len(self.buf) for s, n in zip(self.starts, self.lens))
        return cls(torch.tensor(list(self.buf), dtype=torch.uint8), torch.tensor(self.starts, dtype=torch.int64),
                   torch.tensor(self.lens, dtype=torch.int32), None, "string")


class _M:
    """What ``_build_plan`` / ``lds_estimate`` read of a staged table (the plan is host-side bookkeeping)."""

    def __init__(self, t):
        self.table, self.n = t, t.length


def _plan_bytes(tables):
    return len(S._build_plan([_M(t) for t in tables])[0][0])


def _estimate(t):
    return S.Staged.lds_estimate(_M(t))


# ----------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------

SHORT_ROWS = (1, 2, 255, 256, 257, 3001)


def _short_table(n):
    """{} and {"a":1} / {"a":22} rows: runs of 1..8 empty records put several records inside one 16-byte word."""
    vals, run, k = [], 1, 0
    while len(vals) < n:
        vals += [None] * run + [22 if k % 2 else 1]
        run, k = run % 8 + 1, k + 1
    return Table(["a"], [_prim(vals[:n])], n)


def _xs_table():
    """Row i holds "x" * (i % 40): line lengths sweep every residue mod 16.  The lengths of one 40-row cycle sum to
    4 mod 16, so alone they reach only 4 start residues per length; a null row ({}: 3 bytes) every 41 rows shifts
    the phase by an odd amount and every (start mod 16, length mod 16) pair occurs."""
    n = 3001
    a = _Arena()
    for i in range(n):
        a.add(b"x" * (i % 40))
    c = a.column()
    c.valid = _mask(i % 41 != 40 for i in range(n))
    return Table(["s"], [c], n)


SPECIALS = [bytes([b]) for b in (0x00, 0x01, 0x08, 0x09, 0x0a, 0x0c, 0x0d, 0x1f, 0x20, 0x22, 0x5c, 0x7f)] + \
           ["é".encode("utf-8"), "日".encode("utf-8")]


def _escape_table():
    """One arena; every (start offset mod 8, position mod 8, special) triple, every length 0..24 at every offset,
    strings of escapes only, a special right after a multibyte character, overlapping and backward views, and a
    last string that ends at the arena's final byte (arena size a multiple of 512, start = 509 mod 512)."""
    rnd = random.Random(11)
    a = _Arena()
    triples = set()
    for o in range(8):
        for n in range(25):
            a.add(b"a" * n, o)
        for si, sp in enumerate(SPECIALS):
            w = len(sp)
            for p in range(25 - w):
                n = p + w if rnd.random() < 0.35 else rnd.randint(p + w, 24)      # often the string's last byte
                a.add(b"a" * p + sp + b"a" * (n - p - w), o)
                triples.add((o, p % 8, si))
    assert len(triples) == 8 * 8 * len(SPECIALS)
    for k in range(1, 18):
        a.add(b'"' * k)
        a.add(b"\\" * k)
    for s in ("é\n", '日"', "日\\", "é\x01", "aé\ta", "日\x1f日", "ab日\r"):
        a.add(s.encode("utf-8"))
    s0 = a.add(b"overlapping-views-0123456789")
    a.view(s0, 12)
    a.view(s0 + 5, 12)
    s1 = a.add(b'alpha,be"ta,gamma')
    a.view(s1 + 12, 5)                                   # starts decrease, as split_part's views do
    a.view(s1 + 6, 5)
    a.view(s1, 5)
    last = a.add_at_end(b'z"\n', 512)
    assert last % 512 == 509 and len(a.buf) % 512 == 0 and last + 3 == len(a.buf)
    c = a.column()
    assert c.length <= 4000
    return Table(["s"], [c], c.length)


def _arena_end_table():
    """A 512-byte arena whose last rows end at its final byte at every start alignment; the last string starts at
    offset 509.  The same views once as strings and once as raw JSON (the tail of the arena is digits)."""
    buf = (b'ab"de\\gh' * 62) + b"1234567891234567"
    assert len(buf) == 512
    views = [(0, 8), (3, 13), (488, 9), (496, 16), (497, 15), (504, 8), (505, 7), (506, 6), (507, 5), (508, 4),
             (510, 2), (511, 1), (512, 0), (509, 3)]
    arena = torch.tensor(list(buf), dtype=torch.uint8)
    starts = torch.tensor([s for s, _ in views], dtype=torch.int64)
    lens = torch.tensor([n for _, n in views], dtype=torch.int32)
    raw_ok = _mask(s >= 496 and n > 0 for s, n in views)                 # only digit runs are JSON
    return Table(["s", "j"], [StrColumn(arena, starts, lens), JsonColumn(arena, starts, lens, raw_ok, "string")],
                 len(views))


def _fragment(n):
    if n == 0:
        return b""
    if n == 1:
        return b"7"
    if n % 2:
        return ("123456789" * 5)[:n].encode()
    return b'"' + (string.ascii_letters * 2)[:n - 2].encode() + b'"'


def _raw_table():
    """JsonColumn fragments of length 0..40 at every start offset mod 8, the last one ending at the arena's end."""
    a = _Arena()
    for o in range(8):
        for n in range(41):
            a.add(_fragment(n), o)
    a.add_at_end(b'{"k":[1,2.5,"x"]}', 64)
    c = a.column(JsonColumn)
    return Table(["j", "i"], [c, _prim(list(range(c.length)))], c.length)


def _decimal_table():
    """Decimal columns render through the raw path (exact digits at the scale; E-notation below 1E-6)."""
    d2 = [Dec("0"), Dec("0.01"), Dec("-0.01"), Dec("0.30"), Dec("2.35"), Dec("-7.99"), Dec("12345678.90"),
          Dec("-99999999.99"), None, Dec("99999999.99"), Dec("1.00"), Dec("-2.50")]
    d6 = [Dec("123456789012345678.12"), Dec("-99999999999999999999999999999999.999999"), Dec("0"), Dec("0.000001"),
          Dec("-0.000001"), None, Dec("0.333333"), Dec("99999999999999999999999999999999.999999"), Dec("1"),
          Dec("18446744073709551616"), Dec("-18446744073709551615.5"), Dec("9223372036854.775807")]
    d7 = [Dec("0.0000001"), Dec("-0.0000001"), Dec("0.0000012"), Dec("0.0000010"), Dec("0.0000099"), Dec("1.5"),
          None, Dec("0"), Dec("99.9999999"), Dec("-99.9999999"), Dec("0.0001000"), Dec("0.0000123")]
    cols = [column_from_pylist(v, parse_decimal_type(t)) for v, t in
            ((d2, "decimal(10,2)"), (d6, "decimal(38,6)"), (d7, "decimal(9,7)"))]
    return Table(["p", "w", "e"], cols, len(d2))


def _long_values():
    v = [0, 1, -1]
    for k in range(1, 19):
        v += [10 ** k - 1, -(10 ** k - 1), 10 ** k, -(10 ** k)]
    v += [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 10 ** 16 - 1, 10 ** 16 + 1, 2 ** 63 - 1, -2 ** 63]
    return v


def _longs_table():
    """Digit-count boundaries of put_u64 / put_fixed, and the same values clipped to int, short and byte."""
    v = _long_values()
    cols = [_prim(v)]
    for dtype, bits in (("int", 31), ("short", 15), ("byte", 7)):
        cols.append(_prim([max(-2 ** bits, min(2 ** bits - 1, x)) for x in v], dtype))
    return Table(["l", "i", "s", "b"], cols, len(v))


def _double_values():
    ulp_below = math.nextafter
    v = [1e-3, ulp_below(1e-3, 0.0), 9999999.999999998, 1e7, ulp_below(1e7, 0.0), 123456.7, 1e16,
         1.2345678901234567e16, 4.9e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 0.0, -0.0, float("nan"),
         float("inf"), float("-inf")]
    rnd = random.Random(7)
    for point in range(-2, 8):                              # 17 digits with `point` digits before the decimal point
        found = 0
        while found < 4:
            x = rnd.uniform(10.0 ** (point - 1), 10.0 ** point)
            digits = repr(x).replace(".", "").replace("-", "").split("e")[0].strip("0")
            if len(digits) == 17 and 10.0 ** (point - 1) <= x < 10.0 ** point:
                v += [x, -x]
                found += 1
    bits = np.random.default_rng(5).integers(0, 2 ** 64, 1000, dtype=np.uint64).view(np.float64)
    v += [float(x) for x in bits if math.isfinite(x) and x != 0.0]
    return v


def _doubles_table():
    """The layout switch points of put_java_double, 17-digit values at every point position, random bit patterns."""
    v = _double_values()
    return Table(["d"], [PrimColumn("double", torch.tensor(v, dtype=torch.float64))], len(v))


def _us(*a):
    return (dt.datetime(*a) - EPOCH) // dt.timedelta(microseconds=1)


def _timestamp_values():
    day = 86400 * 10 ** 6
    v = [0, 1, -1, 999, -999, 1000, -1000, 1001, -1001, -day, -day - 1, -day + 1, _us(2000, 2, 29), _us(1900, 2, 28),
         _us(1900, 3, 1), _us(2000, 2, 29, 23, 59, 59, 999999), -62135596800000000, 253402300799999999]
    for c in range(1, 100):                                 # one per century, years 101 .. 9949
        v.append(_us(100 * c + c % 50, 1 + c % 12, 1 + c % 28, c % 24, c % 60, (7 * c) % 60, (7919 * c) % 10 ** 6))
    return v


def _timestamps_table():
    """Floor division of negative microseconds, leap days, the first and last four-digit years."""
    v = _timestamp_values()
    assert format_timestamp_us(v[16]).startswith("0001-01-01T") and format_timestamp_us(v[17]).startswith("9999-12-31T")
    return Table(["t"], [_prim(v, "timestamp")], len(v))


def _dates_table():
    v = [0, -1, 59, 60, 11016, 11017, -719162, 2932896, None, 18321]
    return Table(["d"], [_prim(v, "date")], len(v))


MAP = MapType("string", "string")


def _nesting_table():
    """A struct inside a map inside a filterNull array inside a plain array; one bit of the row number per level
    decides whether that level (or leaf) is null, so every combination occurs: a null container in each mode
    (struct member: omitted, map member: null, array element: null, filterNull element: omitted) and containers all
    of whose members are null ({} / []).  Names that need escaping and a 40-byte non-ASCII name."""
    n = 128

    def bit(b):
        return _mask((r >> b) & 1 == 0 for r in range(n))

    def leaf(b, mul):
        return PrimColumn("long", torch.arange(n, dtype=torch.int64) * mul - 5, bit(b))

    sa = _Arena()
    for r in range(n):
        sa.add(("v%d\t" % r).encode())
    sv = sa.column()
    sv.valid = bit(1)
    st = StructColumn(["a", 'q"x'], [leaf(0, 3), sv], n, bit(2))
    mp = StructColumn(["k", "tab\t"], [st, leaf(0, 11)], n, bit(3), True, MAP)
    fa = ArrayColumn([leaf(1, 13), mp, leaf(0, 17)], n, bit(4), True)
    pa = ArrayColumn([fa, leaf(1, 19), fa], n, bit(5), False)
    top = StructColumn(["é" * 20, "n"], [pa, leaf(0, 23)], n, bit(6))
    return Table(['q"x', "tab\t", "é" * 20, "m", "z"], [top, st, leaf(1, 29), mp, pa], n)


def _chain(depth, n=None):
    """A column whose innermost leaf sits at nesting level ``depth`` (the column itself is level 0); the levels
    cycle through struct, map, array and filterNull array, each with a sibling leaf before or after the nested
    container, and row r has level r null."""
    n = depth + 2 if n is None else n
    col = _prim([7 * r - 3 for r in range(n)])
    for level in range(depth - 1, -1, -1):
        valid = _mask(r % (depth + 1) != level for r in range(n))
        side = _prim([None if (r + level) % 3 == 0 else level for r in range(n)])
        kind = level % 4
        if kind == 0:
            col = StructColumn(["n", "s"], [col, side], n, valid)
        elif kind == 1:
            col = StructColumn(["s", "n"], [side, col], n, valid, True, MAP)
        elif kind == 2:
            col = ArrayColumn([side, col], n, valid)
        else:
            col = ArrayColumn([col, side], n, valid, True)
    return col


def _depth30_table():
    """Exactly the deepest nesting the device serializer renders."""
    c = _chain(S.MAX_DEPTH)
    return Table(["c", "x"], [c, _prim(list(range(c.length)))], c.length)


def _depth31_table():
    """One level past the device serializer's limit."""
    c = _chain(S.MAX_DEPTH + 1)
    return Table(["c", "x"], [c, _prim(list(range(c.length)))], c.length)


def _deep_struct_table():
    """A 40-deep struct, 3 rows: all levels present, level 20 null, the leaf null."""
    n = 3
    col = _prim([42, 43, None])
    for level in range(39, -1, -1):
        col = StructColumn(["s%d" % level, "v"], [col, _prim([level, None, -level])], n,
                           _mask([True, False, True]) if level == 20 else None)
    return Table(["deep", "x"], [col, _prim([1, 2, 3])], n)


def _wide_table():
    """700 nullable long columns, 3 rows: more render tables than the kernels stage in LDS."""
    cols = [_prim([j, None if j % 3 == 0 else -j, 10 ** (j % 19)]) for j in range(700)]
    return Table(["column_%04d" % j for j in range(700)], cols, 3)


def _flat_table(n, seed, const):
    """A flat table (one node per column): the shape whose render plan is cached."""
    rnd = random.Random(seed)
    some = lambda f: [None if rnd.random() < 0.15 else f() for _ in range(n)]          # noqa: E731
    cols = [_prim(some(lambda: rnd.randint(-10 ** 12, 10 ** 12))),
            _prim(some(lambda: rnd.randint(-2 ** 31, 2 ** 31 - 1)), "int"),
            column_from_pylist(some(lambda: rnd.choice(["plain", 'q"uote', "tab\t", "unié", ""])), "string"),
            _prim(some(lambda: rnd.uniform(-1, 1) * 10 ** rnd.randint(-9, 9)), "double"),
            _prim(some(lambda: rnd.random() < 0.5), "boolean"),
            _prim(some(lambda: rnd.randint(-10 ** 15, 4 * 10 ** 15)), "timestamp"),
            _prim(some(lambda: rnd.randint(-700000, 2900000)), "date"),
            ConstColumn(const, "string", n, "cpu")]
    return Table(["l", "i", "s", "d", "b", "t", "dt", "c"], cols, n)


def _cached_a():
    return _flat_table(300, 1, "abcdefg")                   # the constant's text: 9 bytes


def _cached_b():
    return _flat_table(257, 2, "abcdefghijklmnopqrstuvw")   # 25 bytes: patched into the cached plan's pool


GROUP_ROWS = (1, 256, 257, 300)


def _group_table(k):
    """Small table number k of a render group: every k has its own schema."""
    if k < 0:
        return Table(["z"], [_prim([])], 0)
    n = GROUP_ROWS[k % 4]
    names = ["id%d" % k, "s"]
    cols = [_prim([None if r % (k + 2) == 0 else r * (k + 1) for r in range(n)]),
            column_from_pylist([None if r % 7 == k % 7 else "t%d-%d" % (k, r) for r in range(n)], "string")]
    if k % 3 == 0:
        names.append("d")
        cols.append(_prim([r / (k + 1.0) for r in range(n)], "double"))
    elif k % 3 == 1:
        names.append("t")
        cols.append(_prim([r * 10 ** 9 * (k - 9) for r in range(n)], "timestamp"))
    else:
        names.append("b")
        cols.append(_prim([r % 3 == 0 for r in range(n)], "boolean"))
    if k % 2:
        names.append("st")
        cols.append(StructColumn(["a", "b"], [cols[0], cols[1]], n, _mask(r % 5 != 1 for r in range(n))))
    if k % 5 == 0:
        names.append("c")
        cols.append(ConstColumn("c%d" % k, "string", n, "cpu"))
    return Table(names, cols, n)


GROUP_LIST = list(range(5)) + [-1] + list(range(5, 18))      # 18 tables and, in the middle, one of 0 rows

CJK_TABLES, CJK_COLUMNS = 4, 80


def _cjk_table(k):
    """80 long columns with 40-character CJK names (120 bytes of UTF-8 each), 3 rows."""
    names = ["".join(chr(0x4e00 + (31 * (CJK_COLUMNS * k + j) + 7 * i) % 4000) for i in range(40))
             for j in range(CJK_COLUMNS)]
    assert len(set(names)) == CJK_COLUMNS
    cols = [_prim([j + k, None if j % 2 else j, -j]) for j in range(CJK_COLUMNS)]
    return Table(names, cols, 3)


CASES = {
    **{"short_%d" % n: functools.partial(_short_table, n) for n in SHORT_ROWS},
    "xs": _xs_table, "escapes": _escape_table, "arena_end": _arena_end_table, "raw": _raw_table,
    "decimal": _decimal_table, "longs": _longs_table, "doubles": _doubles_table, "timestamps": _timestamps_table,
    "dates": _dates_table, "nesting": _nesting_table, "depth30": _depth30_table, "depth31": _depth31_table,
    "deep_struct": _deep_struct_table, "wide": _wide_table, "cached_a": _cached_a, "cached_b": _cached_b,
    **{"group_%d" % k: functools.partial(_group_table, k) for k in sorted(set(GROUP_LIST))},
    **{"cjk_%d" % k: functools.partial(_cjk_table, k) for k in range(CJK_TABLES)},
}
HOST_ONLY = ("depth31", "deep_struct", "wide")             # past the device serializer's limits


@functools.lru_cache(maxsize=None)
def _case(name):
    """(table on the CPU, its reference rendering): built once, shared by the CPU and the GPU tests."""
    t = CASES[name]()
    return t, _Ref(t)


# ----------------------------------------------------------------------------------------------------------------
# CPU: the reference itself, the host serializer, the plan bookkeeping
# ----------------------------------------------------------------------------------------------------------------

def test_format_timestamp_pads_the_year():
    assert format_timestamp_us(-62135596800000000) == "0001-01-01T00:00:00.000Z"
    assert format_timestamp_us(-62135596800000000, iso=False) == "0001-01-01 00:00:00"
    assert format_timestamp_us(_us(999, 12, 31, 23, 59, 59, 999000)) == "0999-12-31T23:59:59.999Z"
    assert format_timestamp_us(_us(999, 12, 31, 23, 59, 59, 120000), iso=False) == "0999-12-31 23:59:59.12"
    assert format_timestamp_us(253402300799999999) == "9999-12-31T23:59:59.999Z"
    assert format_timestamp_us(-1) == "1969-12-31T23:59:59.999Z"


def test_reference_spot_checks():
    """The reference against texts written out by hand (it is the oracle of everything below)."""
    assert _case("short_2")[1].lines == [b"{}", b'{"a":1}']
    assert _case("dates")[1].lines[:8] == [b'{"d":"1970-01-01"}', b'{"d":"1969-12-31"}', b'{"d":"1970-03-01"}',
                                           b'{"d":"1970-03-02"}', b'{"d":"2000-02-29"}', b'{"d":"2000-03-01"}',
                                           b'{"d":"0001-01-01"}', b'{"d":"9999-12-31"}']
    ts = _case("timestamps")[1].lines
    assert ts[2] == b'{"t":"1969-12-31T23:59:59.999Z"}' and ts[7] == b'{"t":"1970-01-01T00:00:00.001Z"}'
    assert ts[10] == b'{"t":"1969-12-30T23:59:59.999Z"}' and ts[16] == b'{"t":"0001-01-01T00:00:00.000Z"}'
    d = _case("doubles")[1].lines
    assert d[:5] == [b'{"d":0.001}', b'{"d":9.999999999999998E-4}', b'{"d":9999999.999999998}', b'{"d":1.0E7}',
                     b'{"d":9999999.999999998}']
    assert d[11:16] == [b'{"d":0.0}', b'{"d":-0.0}', b'{"d":"NaN"}', b'{"d":"Infinity"}', b'{"d":"-Infinity"}']
    lg = _case("longs")[1].lines
    assert lg[-1] == b'{"l":-9223372036854775808,"i":-2147483648,"s":-32768,"b":-128}'
    assert _case("decimal")[1].lines[0] == b'{"p":0.00,"w":123456789012345678.120000,"e":1E-7}'
    esc = _case("escapes")[1].lines
    assert esc[-1] == b'{"s":"z\\"\\n"}' and esc[-2] == b'{"s":"alpha"}' and esc[-4] == b'{"s":"gamma"}'
    nest = _case("nesting")[1].lines
    assert nest[0].startswith(b'{"q\\"x":{"\xc3\xa9') and nest[127] == b"{}"
    assert any(b'"m":{"k":null,"tab\\t":null}' in ln for ln in nest) and any(b'"z":[null,null,null]' in ln for ln in nest)
    assert any(b'"k":{}' in ln for ln in nest) and any(b"[[]," in ln for ln in nest)


def test_xs_lines_cover_every_word_phase():
    """Every (start mod 16, length mod 16) pair of a record in the output blob (the newline is part of the record)."""
    ref = _case("xs")[1]
    pairs, off = set(), 0
    for n in ref.lens:
        pairs.add((off % 16, (n + 1) % 16))
        off += n + 1
    assert len(pairs) == 256


@pytest.mark.parametrize("name", list(CASES))
def test_host_serializer_matches_python(name):
    t, ref = _case(name)
    _check(_host(t), ref)


@pytest.mark.parametrize("name", list(CASES))
def test_lds_estimate_bounds_the_real_plan(name):
    """``Staged.lds_estimate`` decides which tables share a launch pair: it must not undercount the render tables
    ``_build_plan`` produces (names are quoted UTF-8 in the pool, not characters)."""
    t = _case(name)[0]
    if name in ("depth31", "deep_struct"):
        with pytest.raises(S.PlanTooDeep):
            _plan_bytes([t])
        return
    assert _estimate(t) >= _plan_bytes([t])


def test_limit_cases_exceed_the_kernel_limits():
    """The sizes the limit tests rely on, from the real plans."""
    assert _plan_bytes([_case("wide")[0]]) > S._LDS_LIMIT
    assert _plan_bytes([_case("depth30")[0]]) <= S._LDS_LIMIT
    tables = [_case("cjk_%d" % k)[0] for k in range(CJK_TABLES)]
    real = _plan_bytes(tables)
    by_chars = sum(S.ctypes.sizeof(S.DevNode) + 32 + len(nm) + 16 for t in tables for nm in t.names)
    # counting a name's characters (as the estimate once did) lets the four tables share a group that cannot render
    assert by_chars < S._LDS_LIMIT < real
    assert all(_plan_bytes([t]) <= S._LDS_LIMIT for t in tables)
    assert sum(_estimate(t) for t in tables) >= real


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------

def _staged(name, gpu):
    st = S.Staged(_to_dev(_case(name)[0], gpu))
    assert st.gpu
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n not in HOST_ONLY and not n.startswith("cached_")])
def test_device_serializer_matches_python(gpu, name):
    before = S.STATS["launch_pairs"]
    _check(_staged(name, gpu).render(), _case(name)[1])
    assert S.STATS["launch_pairs"] == before + 1           # rendered by the kernels, not by the host


@pytest.mark.gpu
@pytest.mark.parametrize("name", HOST_ONLY)
def test_tables_past_the_kernel_limits_still_render(gpu, name):
    """700 columns (72 KiB of render tables), 31 and 40 nesting levels: no NativeError or ValueError reaches the
    caller; the rows come from the host serializer."""
    before = S.STATS["launch_pairs"]
    _check(_staged(name, gpu).render(), _case(name)[1])
    assert S.STATS["launch_pairs"] == before


@pytest.mark.gpu
def test_cached_plan_with_longer_constant(gpu):
    """The second render reuses the first one's plan; its constant's text is longer and is patched into the pool."""
    S._PLANS.clear()
    _check(_staged("cached_a", gpu).render(), _case("cached_a")[1])
    assert len(S._PLANS) == 1
    _check(_staged("cached_b", gpu).render(), _case("cached_b")[1])
    assert len(S._PLANS) == 1
    _check(_staged("cached_a", gpu).render(), _case("cached_a")[1])


@pytest.mark.gpu
def test_render_groups_of_16_and_2(gpu):
    names = ["group_%d" % k for k in GROUP_LIST]
    staged = [_staged(nm, gpu) for nm in names]
    S.link_render_groups(staged)
    groups = []
    for st in staged:
        if st.group is not None and st.group not in groups:
            groups.append(st.group)
    assert [len(g.members) for g in groups] == [16, 2]
    empty = staged[GROUP_LIST.index(-1)]
    assert empty.n == 0 and empty.group is None
    before = S.STATS["launch_pairs"]
    order = [i for i in range(len(staged)) if staged[i] is not empty]
    random.Random(3).shuffle(order)                        # any member may trigger its group's render
    for i in order:
        _check(staged[i].render(), _case(names[i])[1])
    assert S.STATS["launch_pairs"] == before + len(groups)
    _check(empty.render(), _case("group_-1")[1])


@pytest.mark.gpu
def test_empty_segment_inside_a_group(gpu):
    names = ["group_2", "group_-1", "group_3"]
    staged = [_staged(nm, gpu) for nm in names]
    before = S.STATS["launch_pairs"]
    S._render_members(staged)
    assert S.STATS["launch_pairs"] == before + 1
    for nm, st in zip(names, staged):
        _check(st.render(), _case(nm)[1])


@pytest.mark.gpu
def test_group_whose_real_plan_exceeds_lds(gpu):
    """Four tables with 40-character CJK names: together their render tables exceed 64 KiB.  Grouped by the
    estimate, no group exceeds it; forced into one group, they render in smaller groups.  Every member equals its
    reference either way."""
    names = ["cjk_%d" % k for k in range(CJK_TABLES)]
    staged = [_staged(nm, gpu) for nm in names]
    S.link_render_groups(staged)
    for g in {id(st.group): st.group for st in staged if st.group is not None}.values():
        assert _plan_bytes([m.table for m in g.members]) <= S._LDS_LIMIT
    for nm, st in zip(names, staged):
        _check(st.render(), _case(nm)[1])
    forced = [_staged(nm, gpu) for nm in names]
    S._close_group(forced)
    assert all(st.group is forced[0].group for st in forced)
    before = S.STATS["launch_pairs"]
    for nm, st in zip(names, forced):
        _check(st.render(), _case(nm)[1])
    assert S.STATS["launch_pairs"] >= before + 2
