"""Hand-assembled DEFLATE, LZ4-block and snappy-raw-block streams for ``tests/test_codec_vectors.py``.

Every stream is built from an explicit symbol list by a writer that follows the format description (RFC 1951, the
LZ4 block format, the snappy format description), and its expected bytes come from the writer's own plain expansion
of that list — never from a decoder.  This module runs no tests.

A valid vector is ``Vec(name, comp, expected)``.  A malformed one is ``Bad(name, comp, None, klass, cap)``: ``klass``
names the status class a decoder must report and ``cap`` is the output capacity it is given.  Malformed vectors are
chosen so that a decoder *without* the relevant check still stays near its slot: it reaches at most one byte before
the output, overruns it by a few bytes, and over-reads the input by fewer bytes than follow every member.  (The two
offset-0 vectors are the exception the formats force: what a decoder without that check reads is its own slot, but
a `x % 0` in its copy loop is not defined.)
"""
from __future__ import annotations

import functools
import random
import zlib
from typing import NamedTuple, Optional


class Vec(NamedTuple):
    name: str
    comp: bytes
    expected: bytes


class Bad(NamedTuple):
    name: str
    comp: bytes
    expected: Optional[bytes]     # always None
    klass: str                    # "trunc" | "offset" | "overflow" | "size" | "block" | "code"
    cap: int
    stream_ok: bool = False       # the stream itself is well-formed: only the capacity given with it is wrong


def noise(n: int, seed: int) -> bytes:
    return bytes(random.Random(seed).getrandbits(8) for _ in range(n))


# =====================================================================================================================
# DEFLATE (RFC 1951)
# =====================================================================================================================
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CLEN_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
# a complete code over all 19 code-length symbols (13/16 + 6/32 = 1); its last entry in CLEN_ORDER (15) is nonzero,
# so a header written with it has HCLEN = 19
DEFAULT_CL_LENS = [4] * 13 + [5] * 6


class BitWriter:
    """Fields go in LSB-first, Huffman codes MSB-first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.nacc = 0

    @property
    def bitpos(self) -> int:
        return len(self.buf) * 8 + self.nacc

    def bits(self, value: int, count: int) -> None:
        assert 0 <= value < (1 << count), (value, count)
        self.acc |= value << self.nacc
        self.nacc += count
        while self.nacc >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.nacc -= 8

    def code(self, code: int, length: int) -> None:
        assert length > 0 and 0 <= code < (1 << length), (code, length)
        rev = 0
        for i in range(length):
            rev |= ((code >> i) & 1) << (length - 1 - i)
        self.bits(rev, length)

    def align(self) -> None:
        if self.nacc:
            self.bits(0, 8 - self.nacc)

    def raw(self, data: bytes) -> None:
        assert self.nacc == 0
        self.buf += data

    def getvalue(self) -> bytes:
        return bytes(self.buf) + (bytes([self.acc]) if self.nacc else b"")


def kraft(lengths) -> float:
    return sum(2.0 ** -l for l in lengths if l)


def canonical_codes(lengths):
    """RFC 1951 3.2.2: code of every symbol with a nonzero length (None for the others)."""
    assert kraft(lengths) <= 1.0, "over-subscribed lengths have no canonical code"
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt = [0] * 16
    code = 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def len_sym(length: int):
    """(length symbol, extra) of a match length; 258 is symbol 285."""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    assert length - LEN_BASE[i] < (1 << LEN_EXTRA[i])
    return 257 + i, length - LEN_BASE[i]


def dist_sym(dist: int):
    assert 1 <= dist <= 32768
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, dist - DIST_BASE[i]


def M(length: int, dist: int):
    """Match tuple (length symbol, extra, distance symbol, extra)."""
    return len_sym(length) + dist_sym(dist)


def rle_code_lengths(lens):
    """Run-length code a list of code lengths with symbols 16, 17, 18 (greedy): [(symbol, extra)]."""
    out = []
    i = 0
    while i < len(lens):
        v = lens[i]
        j = i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
        i = j
    return out


def expand_code_lengths(cl_syms):
    out = []
    for s, e in cl_syms:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + e)
        elif s == 17:
            out += [0] * (3 + e)
        else:
            out += [0] * (11 + e)
    return out


class Deflate:
    """One raw-deflate member: block writers that emit the bits and expand the same symbols into ``out``."""

    def __init__(self):
        self.bw = BitWriter()
        self.out = bytearray()
        self.marks = []            # bit position after every symbol (to cut a stream in the middle of one)
        self.stored_align = []     # bit alignment at which each stored block's header starts
        self.cl_syms = None        # code-length symbols of the last dynamic header
        self.hclen = None

    # ---- blocks
    def stored(self, data: bytes, final=False, nlen=None):
        bw = self.bw
        self.stored_align.append(bw.bitpos % 8)
        bw.bits(int(final), 1)
        bw.bits(0, 2)
        bw.align()
        bw.bits(len(data), 16)
        bw.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        bw.raw(data)
        self.out += data
        return self

    def fixed(self, syms, final=False, eob=True):
        self.bw.bits(int(final), 1)
        self.bw.bits(1, 2)
        self._symbols(FIXED_LL, FIXED_D, syms, eob)
        return self

    def header(self, ll_lens, d_lens, final=False, rle=False, cl_syms=None, cl_lens=None, hclen=None, hlit=None):
        bw = self.bw
        bw.bits(int(final), 1)
        bw.bits(2, 2)
        bw.bits((len(ll_lens) if hlit is None else hlit) - 257, 5)
        bw.bits(len(d_lens) - 1, 5)
        lens = list(ll_lens) + list(d_lens)
        if cl_syms is None:
            cl_syms = rle_code_lengths(lens) if rle else [(l, 0) for l in lens]
            assert expand_code_lengths(cl_syms) == lens
        if cl_lens is None:
            cl_lens = DEFAULT_CL_LENS
        if hclen is None:
            hclen = max(4, 1 + max(i for i in range(19) if cl_lens[CLEN_ORDER[i]]))
        assert all(cl_lens[CLEN_ORDER[i]] == 0 for i in range(hclen, 19))
        bw.bits(hclen - 4, 4)
        for i in range(hclen):
            bw.bits(cl_lens[CLEN_ORDER[i]], 3)
        if cl_syms:
            codes = canonical_codes(cl_lens)
            for s, e in cl_syms:
                bw.code(codes[s], cl_lens[s])
                if s >= 16:
                    bw.bits(e, CLEN_EXTRA[s])
        self.cl_syms, self.hclen = cl_syms, hclen
        return self

    def dynamic(self, ll_lens, d_lens, syms, final=False, eob=True, **hdr):
        self.header(ll_lens, d_lens, final, **hdr)
        self._symbols(ll_lens, d_lens, syms, eob)
        return self

    def _symbols(self, ll_lens, d_lens, syms, eob):
        bw, out = self.bw, self.out
        llc, dc = canonical_codes(ll_lens), canonical_codes(d_lens)
        for s in list(syms) + ([256] if eob else []):
            if isinstance(s, int):
                bw.code(llc[s], ll_lens[s])
                if s < 256:
                    out.append(s)
            else:
                ls, le, ds, de = s
                bw.code(llc[ls], ll_lens[ls])
                if ls < 286:                      # 286 / 287 have a fixed code but no meaning: stop there
                    bw.bits(le, LEN_EXTRA[ls - 257])
                    bw.code(dc[ds], d_lens[ds])
                    if ds < 30:
                        bw.bits(de, DIST_EXTRA[ds])
                        length, dist = LEN_BASE[ls - 257] + le, DIST_BASE[ds] + de
                        if 1 <= dist <= len(out):
                            for _ in range(length):
                                out.append(out[-dist])
            self.marks.append(bw.bitpos)

    def finish(self):
        return self.bw.getvalue(), bytes(self.out)


def _ll(pairs, n=None):
    """Literal/length code lengths from {symbol: length}; n entries (default: up to the highest symbol, >= 257)."""
    n = n or max(257, max(pairs) + 1)
    lens = [0] * n
    for s, l in pairs.items():
        lens[s] = l
    return lens


LITS40 = bytes(range(0x30, 0x30 + 40))            # 40 distinct bytes


@functools.lru_cache(maxsize=None)
def inflate_vectors():
    """(valid, malformed) DEFLATE vectors."""
    V, B = [], []

    def add(name, d):
        comp, out = d.finish()
        V.append(Vec(name, comp, out))

    # ---- code lengths 1..15 in one literal/length code: lengths 1..14 once and 15 twice is a complete code
    ll = _ll({**{c: i + 1 for i, c in enumerate(b"ABCDEFGHIJKL")}, 256: 13, 257: 14, 284: 15, 285: 15}, 286)
    assert kraft(ll) == 1.0
    syms = list(b"ABCDEFGHIJKLLKJIHGFEDCBAIJIJJIHJ") + [(257, 0, 0, 0), ord("K"), (285, 0, 1, 0), ord("J"),
                                                       (284, 31, 0, 0), (284, 0, 1, 0)] + list(b"IJLA")
    add("ll_code_lengths_1_to_15", Deflate().dynamic(ll, [1, 1], syms, final=True))
    # ---- the same for distances: 8-bit (symbol 7) and 9-bit (symbol 8) codes side by side
    ll = _ll({**{c: 9 for c in range(256)}, 256: 2, **{s: 5 for s in range(257, 265)}})
    dl = list(range(1, 15)) + [15, 15]
    assert kraft(ll) == 1.0 and kraft(dl) == 1.0
    syms = []
    for k, (ds, de) in enumerate([(s, e) for s in range(16) for e in (0, (1 << DIST_EXTRA[s]) - 1)] +
                                 [(7, 1), (8, 6), (7, 0), (8, 0), (15, 63), (14, 63)]):
        syms += [(257 + k % 8, 0, ds, de), 0x80 + k]
    add("dist_code_lengths_1_to_15", Deflate().stored(noise(300, 1)).dynamic(ll, dl, syms, final=True))
    # ---- 258 in both encodings
    add("len_258_sym285_and_sym284_extra31",
        Deflate().fixed([ord("x"), ord("y"), ord("z"), (285, 0, 2, 0), (284, 31, 1, 0), (284, 31, 0, 0),
                         (285, 0, 0, 0)], final=True))
    # ---- every length symbol and every distance symbol, extra bits all-zero and all-one, over 32 KiB of history
    syms = []
    for i, (ds, de) in enumerate([(s, e) for s in range(30) for e in (0, 1)]):
        ls = 257 + i % 29
        le = ((1 << LEN_EXTRA[ls - 257]) - 1) if (i // 29) % 2 else 0
        syms.append((ls, le, ds, ((1 << DIST_EXTRA[ds]) - 1) if de else 0))
    # the first 29 matches use extra 0 and the next 29 extra all-one for each length symbol; close the loop
    syms += [(257 + k, 0 if k % 2 else (1 << LEN_EXTRA[k]) - 1, 29, 8191) for k in range(29)]
    d = Deflate().stored(noise(32768, 2)).fixed(syms, final=True)
    assert {(s[0], s[1] == 0) for s in syms} >= {(257 + k, z) for k in range(29) for z in (True, False)
                                                 if LEN_EXTRA[k] or z}
    assert {(s[2], bool(s[3])) for s in syms} >= {(k, z) for k in range(30) for z in (False, True)
                                                  if DIST_EXTRA[k] or not z}
    add("every_length_and_distance_symbol", d)
    add("dist_32768_equals_op", Deflate().stored(noise(32768, 3)).fixed([M(3, 32768), M(258, 32768), 7,
                                                                        M(17, 32768)], final=True))
    add("dist_equals_op_1", Deflate().fixed([ord("q"), M(3, 1), M(9, 4)], final=True))
    # ---- overlapping copies
    for dist in (1, 2, 3, 15, 16, 17):
        add(f"overlap_dist_{dist}", Deflate().fixed(list(LITS40[:20]) + [M(3, dist), 0x7B, M(18, dist), 0x7C,
                                                                         M(258, dist), 0x7D, M(33, dist)],
                                                    final=True))
    add("overlap_dist_eq_len", Deflate().fixed(list(LITS40) + [M(10, 10), M(40, 40), M(16, 16), M(17, 17), M(3, 3)],
                                               final=True))
    add("overlap_dist_eq_len_minus_1", Deflate().fixed(list(LITS40) + [M(11, 10), M(41, 40), M(17, 16), M(18, 17),
                                                                       M(4, 3), M(16, 15)], final=True))
    add("overlap_16_lt_dist_lt_len", Deflate().fixed(list(LITS40) + [M(40, 17), M(258, 20), M(100, 33), M(35, 31),
                                                                     M(34, 33)], final=True))
    # ---- a match whose source lies in a previous block of the member
    add("match_source_in_previous_block",
        Deflate().fixed(list(LITS40[:30])).fixed([M(30, 30), M(5, 60)]).stored(b"stored-history").fixed(
            [M(14, 14), M(40, 70)], final=True))
    # ---- stored blocks
    aligns = set()
    for j in range(8):
        nine = [144 + 13 * j + k for k in range(j)]           # j 9-bit literals shift the next block by j bits
        d = Deflate().fixed(nine).stored(b"").fixed(list(b"end"), final=True)
        aligns.add(d.stored_align[0])
        add(f"stored_empty_midstream_bit{d.stored_align[0]}", d)
        d = Deflate().fixed(nine + [ord("L")]).stored(b"", final=True)
        aligns.add(8 + d.stored_align[0])
        add(f"stored_empty_last_bit{d.stored_align[0]}", d)
    assert aligns == set(range(16)), aligns
    add("stored_len_1", Deflate().stored(b"\x5a", final=True))
    add("stored_len_65535", Deflate().stored(noise(65535, 4), final=True))
    add("stored_only_empty", Deflate().stored(b"", final=True))
    # ---- fixed blocks
    add("fixed_empty", Deflate().fixed([], final=True))
    add("fixed_9bit_literals_7bit_lengths",
        Deflate().fixed([144, 200, 255, 143, 0, (257, 0, 0, 0), (264, 0, 2, 0), (265, 1, 4, 1), (279, 15, 5, 0),
                         255, 254, (280, 0, 3, 0), (283, 31, 8, 7)], final=True))
    # ---- dynamic blocks
    d = Deflate().dynamic(_ll({97: 1, 256: 1}), [0], list(b"aaaaaaaaaa"), final=True)
    assert d.hclen == 19
    add("dynamic_hlit257_no_distance_code_hclen19", d)
    add("dynamic_one_distance_code_len1",
        Deflate().dynamic(_ll({97: 2, 98: 2, 256: 2, 257: 2}), [1], [97, 98, (257, 0, 0, 0), 97, (257, 0, 0, 0)],
                          final=True))
    # HCLEN = 4 gives lengths to 16, 17, 18 and 0 only, so every code length is 0 and there is no end-of-block code:
    # no valid block has it (see the malformed list).  The shortest valid header is HCLEN = 5 (lengths 0 and 8).
    cl = [0] * 19
    cl[0] = cl[8] = 1
    d = Deflate().dynamic([0] + [8] * 256, [0], list(range(1, 256)) + [1, 255, 128], final=True, cl_lens=cl)
    assert d.hclen == 5
    add("dynamic_hclen5", d)
    ll = [8] * 128 + [0] * 128 + [2] + [4] * 4
    assert kraft(ll) == 1.0
    d = Deflate().dynamic(ll, [4] * 16, list(b"run-coded") + [(257, 0, 0, 0), (260, 0, 5, 1), (258, 0, 7, 1)] +
                          list(b"header"), final=True, rle=True)
    # a symbol-16 run starts in the literal lengths and ends in the distance lengths
    pos, crossing = 0, False
    for s, e in d.cl_syms:
        n = 1 if s < 16 else (3 + e if s < 18 else 11 + e)
        crossing |= s == 16 and pos < len(ll) < pos + n
        pos += n
    assert crossing and (18, 117) in d.cl_syms
    add("dynamic_rle_16_across_lit_dist_boundary", d)
    ll = [7] * 64 + [0] * 192 + [1]
    d = Deflate().dynamic(ll, [0], list(range(64)) + [63, 0, 31], final=True, rle=True)
    assert (18, 127) in d.cl_syms
    add("dynamic_rle_18_with_138_zeros", d)
    # ---- members of five or more mixed blocks
    lld = _ll({**{c: 8 for c in range(0x20, 0x20 + 96)}, **{c: 8 for c in range(0xC0, 0xC0 + 32)},
               256: 3, 257: 4, 258: 4, 259: 4, 260: 4, 270: 4, 285: 4})
    assert kraft(lld) == 1.0
    dld = [2, 3, 3, 3, 3, 4, 4] + [0] * 13 + [4, 4]
    assert kraft(dld) == 1.0
    for k in range(3):
        d = Deflate()
        d.fixed(list(b"member %d starts with a fixed block; " % k))
        d.stored(noise(1600 + 37 * k, 10 + k))
        d.dynamic(lld, dld, list(b"dynamic ") + [(257, 0, 0, 0), (260, 0, 6, 3), (270, 3, 20, 100 * k)] +
                  list(b" text\xc0\xdf") + [(285, 0, 21, 0)], rle=bool(k % 2))
        d.stored(b"")
        d.fixed([M(50, 40 + k), M(258, 1), M(3, 2), 0xFE])
        if k:
            d.dynamic(lld, dld, [(258, 0, 1, 0), (259, 0, 2, 0)] + list(b"again"), rle=True)
        d.stored(noise(k, 20 + k))
        d.fixed([M(20, 19), M(19, 20)], final=True)
        add(f"member_mixed_blocks_{k}", d)

    # ---------------------------------------------------------------------------------------------- malformed
    def bad(name, d, klass, cap, stream_ok=False):
        B.append(Bad(name, d.finish()[0] if isinstance(d, Deflate) else d, None, klass, cap, stream_ok))

    d = Deflate()
    d.bw.bits(1, 1)
    d.bw.bits(3, 2)
    d.bw.bits(0, 13)
    bad("block_type_3", d, "block", 4)
    bad("stored_len_not_complement_of_nlen", Deflate().stored(b"abcd", final=True, nlen=4), "block", 4)
    cl = [0] * 19
    cl[0] = cl[1] = cl[2] = 1
    bad("oversubscribed_code_length_code", Deflate().header(_ll({97: 1, 256: 1}), [0], True, cl_syms=[], cl_lens=cl),
        "code", 4)
    bad("oversubscribed_literal_code", Deflate().header(_ll({97: 1, 98: 1, 256: 1}), [1], True), "code", 4)
    bad("oversubscribed_distance_code", Deflate().header(_ll({97: 1, 256: 1}), [1, 1, 1], True), "code", 4)
    bad("repeat_16_first", Deflate().header([0] * 257, [0], True, cl_syms=[(16, 0), (1, 0), (18, 127)]), "code", 4)
    bad("repeat_runs_past_hlit_plus_hdist",
        Deflate().header([0] * 257, [0], True, cl_syms=[(1, 0), (18, 127), (18, 109)]), "code", 4)    # 1+138+120
    bad("no_end_of_block_code", Deflate().header(_ll({97: 1, 98: 1}), [0], True), "code", 4)
    cl = [0] * 19
    cl[16] = cl[17] = cl[18] = cl[0] = 2
    d = Deflate().header([0] * 257, [0], True, cl_syms=[(18, 127), (18, 109)], cl_lens=cl)
    assert d.hclen == 4
    bad("hclen_4_leaves_no_end_of_block_code", d, "code", 4)
    for s in (286, 287):
        bad(f"fixed_length_symbol_{s}", Deflate().fixed([97, (s, 0, 0, 0)], final=True), "code", 16)
    for s in (30, 31):
        bad(f"fixed_distance_symbol_{s}", Deflate().fixed([97, (257, 0, s, 0)], final=True), "code", 16)
    bad("distance_op_plus_1", Deflate().fixed(list(b"abcde") + [(257, 0, 4, 1)], final=True), "offset", 8)
    bad("overflow_by_one_from_literal", Deflate().fixed(list(b"abcdef"), final=True), "overflow", 5, True)
    bad("overflow_by_one_from_match", Deflate().fixed(list(b"abc") + [M(5, 3)], final=True), "overflow", 7, True)
    bad("overflow_by_one_from_stored", Deflate().stored(b"0123456789", final=True), "overflow", 9, True)
    bad("capacity_one_larger_than_stream", Deflate().fixed(list(b"abcdef") + [M(4, 2)], final=True), "size", 11, True)
    # cut in the middle of a symbol; the zeros that follow decode as the 1-bit literal until the input runs out
    d = Deflate().dynamic(_ll({97: 1, 98: 3, 256: 3, 257: 2}), [1], [98] * 200, final=True, rle=True)
    first = d.marks[0] // 8 + 5
    cut = next(n for n in range(first, first + 20) if n * 8 not in d.marks)
    bad("cut_in_the_middle_of_a_symbol", d.finish()[0][:cut], "trunc", 200)
    for hlit in (287, 288):
        bad(f"hlit_{hlit}", Deflate().header([0] * 257, [0], True, cl_syms=[], hlit=hlit), "block", 4)
    return tuple(V), tuple(B)


def zlib_inflate(comp: bytes):
    """(output, reached the end of the stream) from zlib's raw inflate; raises zlib.error on a malformed stream."""
    d = zlib.decompressobj(-15)
    out = d.decompress(comp)
    return out, d.eof


# =====================================================================================================================
# LZ4 block format
# =====================================================================================================================
def py_lz4_block_decode(src: bytes) -> bytes:
    """Independent pure-Python LZ4 block decoder written from the format description (token / literal run /
    little-endian offset / match length extension)."""
    out = bytearray()
    i = 0
    while i < len(src):
        tok = src[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = src[i]
                i += 1
                lit += b
                if b != 255:
                    break
        out += src[i:i + lit]
        i += lit
        if i >= len(src):
            break
        off = src[i] | (src[i + 1] << 8)
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = src[i]
                i += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        assert 0 < off <= len(out)
        for _ in range(ml):
            out.append(out[-off])
    return bytes(out)


def lz4_ext(n: int) -> bytes:
    """Length extension of a nibble that is 15: n = length - 15 as 255s, then a byte below 255."""
    assert n >= 0
    return b"\xff" * (n // 255) + bytes([n % 255])


LZ4_TAIL = b"<-tail-12b->"       # a last literal run the reference decoder's end-of-block rules accept


def lz4_block(seqs, last: bytes = LZ4_TAIL):
    """(block, expansion) from [(literals, offset, match_len)] plus the final literal run."""
    comp, out = bytearray(), bytearray()
    for lits, off, ml in seqs:
        assert ml >= 4
        L, m = len(lits), ml - 4
        comp.append((min(L, 15) << 4) | min(m, 15))
        if L >= 15:
            comp += lz4_ext(L - 15)
        comp += lits
        out += lits
        assert 1 <= off <= len(out) and off <= 65535, (off, len(out))
        comp += off.to_bytes(2, "little")
        if m >= 15:
            comp += lz4_ext(m - 15)
        for _ in range(ml):
            out.append(out[-off])
    comp.append(min(len(last), 15) << 4)
    if len(last) >= 15:
        comp += lz4_ext(len(last) - 15)
    comp += last
    out += last
    return bytes(comp), bytes(out)


LZ4_LITERAL_SHAPES = (0, 1, 14, 15, 16, 270, 300)            # 15 -> extension byte 0; 270 -> 15 + 255 + 0
LZ4_MATCH_SHAPES = (4, 18, 19, 20, 273, 274, 532, 32, 33)    # nibble 0, 14, 15 + ext 0 / 1 / 254 / 255,0 / 255,255,3
LZ4_PREFIXES = range(71)
LZ4_CHAIN_SHAPES = ((14, 19), (0, 33), (3, 32))              # (literals, match length) behind a chain of short seqs


def _chain_sizes(p: int):
    """Split p compressed bytes into short sequences of 3 + L bytes (L < 15 literals; the first has L >= 1)."""
    sizes, rem = [], p
    while rem:
        s = min(17, rem)
        if 0 < rem - s < 3:
            s -= 3 - (rem - s)
        sizes.append(s)
        rem -= s
    assert sizes[0] >= 4 and all(3 <= s <= 17 for s in sizes) and sum(sizes) == p
    return sizes


@functools.lru_cache(maxsize=None)
def lz4_vectors():
    """(valid, malformed, names of the valid vectors that break the reference decoder's end-of-block rules)."""
    V, B, relaxed = [], [], set()

    def add(name, seqs, last=LZ4_TAIL, relax=False):
        comp, out = lz4_block(seqs, last)
        V.append(Vec(name, comp, out))
        if relax:
            relaxed.add(name)

    # ---- sweeps: the sequence under test follows P literal bytes (and the 4-byte match that ends their sequence)
    for p in LZ4_PREFIXES:
        pre = [(noise(p, 100 + p), 1, 4)] if p else []
        op0 = p + 4 if p else 0
        for L in LZ4_LITERAL_SHAPES:
            if op0 + L == 0:
                continue                                   # a first sequence without literals has no valid offset
            add(f"sweep_lit{L}_P{p}", pre + [(noise(L, 200 + L), min(op0 + L, 6), 8)])
        for ml in LZ4_MATCH_SHAPES:
            add(f"sweep_ml{ml}_P{p}", pre + [(b"\x11\x22", min(op0 + 2, 40), ml)])
    # ---- the same header positions reached through a chain of short sequences instead of one literal run
    for p in range(4, 71):
        pre, seed = [], 0
        for s in _chain_sizes(p):
            seed += 1
            pre.append((noise(s - 3, 300 + seed + p), 1 + (seed % 2 if pre else 0), 4))
        for L, ml in LZ4_CHAIN_SHAPES:
            add(f"chain_lit{L}_ml{ml}_P{p}", pre + [(noise(L, 400 + L), 5, ml)])
    # ---- offsets
    hist = noise(70, 5)
    for off in (1, 2, 3, 15, 16, 17, 63, 64, 65):
        add(f"offset_{off}", [(hist, off, 4), (b"", off, 20), (b"ab", off, 40), (noise(20, 6), off, 70),
                              (b"c", off, 32), (b"", off, 33), (b"", off, 5)])
    add("offset_65535", [(noise(65535, 7), 65535, 4), (b"", 65535, 40), (b"xy", 65535, 18), (noise(16, 8), 65535, 300)])
    add("offset_eq_match_len", [(hist[:40], 4, 4), (b"", 18, 18), (b"q", 32, 32), (b"", 33, 33),
                                (noise(15, 9), 40, 40)])
    add("offset_eq_match_len_minus_1", [(hist[:40], 4, 5), (b"", 17, 18), (b"q", 31, 32), (b"", 32, 33),
                                        (noise(15, 9), 39, 40), (b"", 16, 17), (b"", 15, 16)])
    add("offset_eq_op", [(b"abcdefgh", 8, 4), (b"", 12, 12), (b"ij", 26, 40), (noise(17, 10), 83, 83)])
    # ---- the delayed (pending) match store: A is pending when B's source is read
    a = [(b"ABCDEFGH", 8, 8)]                              # A: output [8, 16) pending, copies [0, 8)
    add("source_ends_at_start_of_pending_match", a + [(b"ij", 16, 6), (b"kl", 1, 4)])       # B reads [2, 8)
    add("source_ends_one_byte_into_pending_match", a + [(b"ij", 15, 6), (b"kl", 1, 4)])     # B reads [3, 9)
    add("source_inside_pending_match", a + [(b"", 4, 4), (b"", 4, 4), (b"z", 9, 8)])
    add("source_covers_pending_match_and_literals", a + [(b"ijk", 11, 11), (b"", 30, 30)])
    add("source_inside_own_literals", [(b"0123456789", 5, 5), (b"abcdefgh", 8, 8), (b"XYZ", 3, 9), (b"pq", 2, 30),
                                       (noise(16, 11), 16, 16), (noise(20, 12), 7, 35)])
    add("zero_literal_sequence_runs", [(b"0123456789abcdef", 16, 4)] + [(b"", o, m) for o, m in
                                       ((1, 4), (20, 5), (3, 18), (24, 19), (40, 32), (1, 33), (70, 4), (2, 4),
                                        (9, 9), (100, 20), (5, 4), (5, 4), (5, 4), (150, 31), (31, 31))])
    # the reference decoder wants 5 literals at the end and 12 bytes after the last match; the format itself and
    # this project's decoders do not
    # (it takes a last token 0x00 only as the whole block, "empty_block_token_only" below, and rejects the three
    # blocks marked relax, which therefore rest on the other two decoders alone)
    add("last_token_0x00", [(b"0123456789abcdef", 16, 8), (b"", 3, 4), (b"", 24, 12)], last=b"", relax=True)
    add("last_token_0x00_after_long_match", [(noise(20, 13), 20, 300)], last=b"", relax=True)
    add("last_literal_run_of_1", [(b"0123456789", 10, 6)], last=b"Z", relax=True)
    add("one_literal_only", [], last=b"Z")
    add("empty_block_token_only", [], last=b"")
    add("literals_only_300", [], last=noise(300, 14))
    for mult in (1, 2, 3):
        seqs = [(noise(9, 15 + k), 3 + k, 7 + k) for k in range(3 * mult)]
        base = len(lz4_block(seqs, b"")[0])                # token + nothing
        pad = 64 * mult - base
        assert pad >= 16, pad
        last = noise(pad if pad < 15 else pad - 1, 16)     # 15+ literals take one extension byte
        comp, _ = lz4_block(seqs, last)
        assert len(comp) == 64 * mult, len(comp)
        add(f"compressed_length_{64 * mult}", seqs, last=last)

    # ---------------------------------------------------------------------------------------------- malformed
    def bad(name, comp, klass, cap, stream_ok=False):
        B.append(Bad(name, bytes(comp), None, klass, cap, stream_ok))

    bad("offset_0", b"\x40abcd\x00\x00" + b"\x50tail.", "offset", 32)
    bad("offset_0_general_path", b"\xf0\x01" + noise(16, 17) + b"\x00\x00" + b"\x50tail.", "offset", 64)
    bad("offset_op_plus_1", b"\x50abcde\x06\x00" + b"\x50tail.", "offset", 32)
    bad("offset_op_plus_1_general_path", b"\xf0\x00" + noise(15, 18) + b"\x10\x00" + b"\x50tail.", "offset", 64)
    bad("literal_extension_cut_off", b"\xf0\xff", "trunc", 600)
    bad("literal_extension_missing", b"\xf0", "trunc", 600)
    bad("match_extension_cut_off", b"\x4fabcd\x01\x00\xff", "trunc", 600)
    bad("match_extension_missing", b"\x4fabcd\x01\x00", "trunc", 600)
    bad("literal_run_longer_than_input", b"\x50abc", "trunc", 32)
    bad("literal_run_longer_than_input_ext", b"\xf0\x05" + noise(19, 19), "trunc", 64)
    bad("one_offset_byte_left", b"\x10a\x01", "trunc", 32)
    for name, seqs, last in (("literals", [(b"abcd", 1, 4)], b"0123456789"),
                             ("long_literals", [(b"abcd", 1, 4)], noise(40, 20)),
                             ("match", [(b"abcdefgh", 8, 8), (b"ij", 3, 12)], None),
                             ("long_match", [(b"abcdefgh", 8, 8), (b"ij", 3, 60)], None),
                             ("extended_match", [(b"abcdefgh", 8, 8), (noise(20, 21), 3, 300)], None)):
        comp, out = lz4_block(seqs, last or b"")
        if last is None:
            comp = comp[:-1]                               # the block ends with the match
        bad(f"overflow_by_one_from_{name}", comp, "overflow", len(out) - 1, True)
    return tuple(V), tuple(B), frozenset(relaxed)


# =====================================================================================================================
# snappy raw block
# =====================================================================================================================
def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 128:
        out.append((n & 127) | 128)
        n >>= 7
    out.append(n)
    return bytes(out)


def snappy_block(elems, preamble=None):
    """(block, expansion) from elements ("lit", data, length bytes 0..4) | ("copy1"|"copy2"|"copy4", offset, length);
    the tag form is the caller's choice."""
    body, out = bytearray(), bytearray()
    for e in elems:
        if e[0] == "lit":
            _, data, form = e
            n = len(data) - 1
            assert n >= 0
            if form == 0:
                assert n < 60
                body.append(n << 2)
            else:
                assert 1 <= form <= 4 and n < (1 << (8 * form))
                body.append((59 + form) << 2)
                body += n.to_bytes(form, "little")
            body += data
            out += data
            continue
        kind, off, ln = e
        assert 1 <= off <= len(out), (off, len(out))
        if kind == "copy1":
            assert 4 <= ln <= 11 and off < 2048
            body.append(1 | ((ln - 4) << 2) | ((off >> 8) << 5))
            body.append(off & 255)
        elif kind == "copy2":
            assert 1 <= ln <= 64 and off < 65536
            body.append(2 | ((ln - 1) << 2))
            body += off.to_bytes(2, "little")
        else:
            assert kind == "copy4" and 1 <= ln <= 64
            body.append(3 | ((ln - 1) << 2))
            body += off.to_bytes(4, "little")
        for _ in range(ln):
            out.append(out[-off])
    return varint(len(out) if preamble is None else preamble) + bytes(body), bytes(out)


@functools.lru_cache(maxsize=None)
def snappy_vectors():
    V, B = [], []

    def add(name, elems):
        comp, out = snappy_block(elems)
        V.append(Vec(name, comp, out))

    for n in range(1, 61):
        add(f"literal_inline_{n}", [("lit", noise(n, 500 + n), 0)])
    for n, form in ((61, 1), (256, 1), (257, 2), (65536, 2), (65537, 3), (100, 4), (5, 1), (60, 2), (1, 3)):
        add(f"literal_{n}_with_{form}_length_bytes", [("lit", noise(n, 600 + form), form), ("copy2", min(n, 65535), 7),
                                                      ("lit", b"end", 0)])
    hist = ("lit", noise(2100, 30), 2)
    for off in (1, 255, 256, 2047):
        for ln in (4, 11):
            add(f"copy1_offset_{off}_len_{ln}", [hist, ("copy1", off, ln), ("lit", b"|", 0), ("copy1", off, ln)])
    big = ("lit", noise(65535, 31), 2)
    for off in (1, 65535):
        for ln in (1, 64):
            add(f"copy2_offset_{off}_len_{ln}", [big, ("copy2", off, ln), ("lit", b"|", 0), ("copy2", off, ln)])
    add("copy4_offset_70000", [("lit", noise(70000, 32), 3), ("copy4", 70000, 64), ("copy4", 65536, 1),
                               ("copy4", 69999, 33), ("copy4", 5, 20)])
    add("copy_offset_eq_len", [("lit", LITS40, 0), ("copy1", 4, 4), ("copy1", 11, 11), ("copy2", 40, 40),
                               ("copy2", 16, 16), ("copy2", 17, 17), ("copy2", 1, 1), ("copy2", 64, 64)])
    add("copy_offset_eq_len_minus_1", [("lit", LITS40, 0), ("copy1", 4, 5), ("copy1", 10, 11), ("copy2", 39, 40),
                                       ("copy2", 15, 16), ("copy2", 16, 17), ("copy2", 1, 2), ("copy2", 63, 64)])
    add("copy_offset_lt_16_lt_len", [("lit", LITS40, 0), ("copy2", 1, 17), ("copy2", 2, 33), ("copy2", 3, 64),
                                     ("copy2", 7, 40), ("copy2", 15, 31), ("copy4", 13, 64), ("copy2", 15, 17)])
    add("copy_source_in_previous_copy", [("lit", b"ABCDEFGH", 0), ("copy1", 8, 8), ("copy1", 10, 6), ("copy1", 4, 4),
                                         ("copy2", 3, 20), ("lit", b"x", 0), ("copy2", 21, 21)])
    add("preamble_1_byte", [("lit", noise(127, 33), 1)])
    add("preamble_2_bytes", [("lit", noise(128, 34), 1)])
    add("preamble_2_bytes_max", [("lit", noise(16383, 35), 2)])
    add("preamble_3_bytes", [("lit", noise(16384, 36), 2)])
    add("empty_block", [])
    preambles = {len(varint(len(v.expected))) for v in V}
    assert preambles >= {1, 2, 3}

    # ---------------------------------------------------------------------------------------------- malformed
    def bad(name, comp, klass, cap, stream_ok=False):
        B.append(Bad(name, bytes(comp), None, klass, cap, stream_ok))

    ok, out = snappy_block([("lit", b"0123456789", 0), ("copy1", 10, 6)])
    bad("preamble_smaller_than_capacity", ok, "size", len(out) + 1, True)
    bad("preamble_larger_than_capacity", ok, "size", len(out) - 1, True)
    bad("preamble_without_end_in_5_bytes", b"\x90\x80\x80\x80\x80\x00" + ok[1:], "size", 16)
    bad("offset_0", varint(14) + b"\x24" + b"0123456789" + b"\x01\x00", "offset", 14)
    bad("offset_0_copy2", varint(14) + b"\x24" + b"0123456789" + b"\x0e\x00\x00", "offset", 14)
    bad("offset_op_plus_1", varint(14) + b"\x24" + b"0123456789" + b"\x01\x0b", "offset", 14)
    bad("offset_op_plus_1_copy2", varint(14) + b"\x24" + b"0123456789" + b"\x0e\x0b\x00", "offset", 14)
    bad("copy4_offset_2_to_31", varint(14) + b"\x24" + b"0123456789" + b"\x0f\x00\x00\x00\x80", "offset", 14)
    bad("copy4_offset_all_ones", varint(14) + b"\x24" + b"0123456789" + b"\x0f\xff\xff\xff\xff", "offset", 14)
    bad("literal_length_bytes_cut_off", varint(300) + b"\xf4\x2b", "trunc", 300)
    bad("literal_length_byte_missing", varint(100) + b"\xf0", "trunc", 100)
    bad("literal_longer_than_input", varint(10) + b"\x24" + b"01234567", "trunc", 10)
    bad("literal_longer_than_input_1_length_byte", varint(100) + b"\xf0\x63" + noise(98, 37), "trunc", 100)
    bad("copy1_offset_byte_missing", varint(14) + b"\x24" + b"0123456789" + b"\x01", "trunc", 14)
    bad("copy2_offset_byte_missing", varint(14) + b"\x24" + b"0123456789" + b"\x0e\x01", "trunc", 14)
    bad("copy4_offset_byte_missing", varint(14) + b"\x24" + b"0123456789" + b"\x0f\x01\x00\x00", "trunc", 14)
    bad("overflow_by_one_from_literal", snappy_block([("lit", b"0123456789", 0)], preamble=9)[0], "overflow", 9)
    bad("overflow_by_one_from_copy", snappy_block([("lit", b"0123456789", 0), ("copy1", 10, 6)], preamble=15)[0],
        "overflow", 15)
    bad("overflow_by_one_from_long_copy", snappy_block([("lit", b"0123456789", 0), ("copy2", 3, 64)], preamble=73)[0],
        "overflow", 73)
    bad("output_one_byte_short", snappy_block([("lit", b"0123456789", 0), ("copy1", 10, 6)], preamble=17)[0],
        "size", 17)
    return tuple(V), tuple(B)


# =====================================================================================================================
# inputs for the independent encoders
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def encoder_inputs():
    rnd = random.Random(77)
    js = b"".join(b'{"deviceId":%d,"temperature":%d.%d,"status":"%s"}\n' %
                  (rnd.randrange(40), rnd.randrange(-40, 90), rnd.randrange(10), rnd.choice([b"ok", b"warn", b"off"]))
                  for _ in range(300))
    two = bytes(rnd.choice(b"ab") for _ in range(30000))
    # Fibonacci-weighted symbols: the rarest are ~2^-20 as likely as the commonest, which forces 15-bit codes
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    pool = list(range(0x40, 0x40 + 30))
    skew = bytes(rnd.choices(pool, weights=fib, k=69000)) + bytes(pool)
    return (("json", js), ("two_symbols", two), ("fibonacci", skew), ("random", noise(8000, 78)))


@functools.lru_cache(maxsize=None)
def zlib_streams():
    """Raw deflate streams from zlib over every strategy / level / memLevel / wbits, and with periodic flushes."""
    out = []
    strategies = (("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE),
                  ("default", zlib.Z_DEFAULT_STRATEGY))
    for dname, data in encoder_inputs():
        for sname, strat in strategies:
            for level in (0, 1, 9):
                for mem in (1, 9):
                    for wbits in (-9, -15):
                        c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strat)
                        out.append(Vec(f"zlib_{dname}_{sname}_l{level}_m{mem}_w{-wbits}",
                                       c.compress(data) + c.flush(), data))
        for fname, mode, step in (("sync", zlib.Z_SYNC_FLUSH, 300), ("full", zlib.Z_FULL_FLUSH, 700)):
            for sname, strat in strategies[2:]:
                c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strat)
                parts = []
                head = data[:12000]
                for i in range(0, len(head), step):
                    parts.append(c.compress(head[i:i + step]) + c.flush(mode))
                parts.append(c.flush())
                out.append(Vec(f"zlib_{dname}_{sname}_{fname}_flush", b"".join(parts), head))
    return tuple(out)
