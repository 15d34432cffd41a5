"""Hand-assembled DEFLATE, LZ4-block and snappy-raw-block streams and Zstandard frames for
``tests/test_codec_vectors.py``.

Every stream is built from an explicit symbol list by a writer that follows the format description (RFC 1951, the
LZ4 block format, the snappy format description, RFC 8878), and its expected bytes come from the writer's own plain
expansion of that list — never from a decoder.  This module runs no tests.

A valid vector is ``Vec(name, comp, expected)``.  A malformed one is ``Bad(name, comp, None, klass, cap)``: ``klass``
names the status class a decoder must report and ``cap`` is the output capacity it is given.  Malformed vectors are
chosen so that a decoder *without* the relevant check still stays near its slot: it reaches at most one byte before
the output, overruns it by a few bytes, and over-reads the input by fewer bytes than follow every member.  (The
offset-0 vectors, two for LZ4 and snappy and one for zstd, are the exception the formats force: what a decoder
without that check reads is its own slot, but a `x % 0` in its copy loop is not defined.)
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
    klass: str                    # "trunc" | "offset" | "overflow" | "size" | "block" | "code" | zstd's "z_..."
    cap: int
    stream_ok: bool = False       # the stream itself is well-formed: only the capacity given with it is wrong


def noise(n: int, seed: int) -> bytes:
    return random.Random(seed).randbytes(n)      # (one generator for all n bytes: a new one per byte repeats a byte)


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
# Zstandard frames (RFC 8878)
# =====================================================================================================================
ZSTD_MAGIC = 0xFD2FB528
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1,
          -1]
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
ZLL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                              32768, 65536]
ZLL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ZML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                 16387, 32771, 65539]
ZML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ZBLOCK_MAX = 128 * 1024
PRE, REP = "pre", "rep"            # sequence-table modes 0 and 3; RLE(sym) is mode 1 and FSE(norm, log) mode 2
ZSTD_KINDS = ("ll", "of", "ml")
ZSTD_DEFAULTS = {"ll": (LL_DEF, 6), "of": (OF_DEF, 5), "ml": (ML_DEF, 6)}
ZSTD_MAX_SYM = {"ll": 35, "of": 31, "ml": 52}
ZSTD_MAX_LOG = {"ll": 9, "of": 8, "ml": 9}


def RLE(sym):
    return ("rle", sym)


def FSE(norm, log, desc=None):
    """``desc`` replaces the table description written for ``norm`` (a malformed vector's own bytes)."""
    return ("fse", tuple(norm), log, desc)


def fse_table(norm, log):
    """RFC 8878 4.1.1 decoding table of a normalized distribution: [(symbol, nbits, baseline)] per state."""
    size = 1 << log
    sym = [0] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    nxt = [1 if c == -1 else c for c in norm]
    cells = []
    for c in range(size):
        s = sym[c]
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        cells.append((s, nb, (x << nb) - size))
    return cells


class BackWriter:
    """Bits written low to high; the decoder reads them high to low (a zstd backward bitstream)."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits

    def finish(self):
        self.put(1, 1)                                    # the end marker
        nbytes = (self.n + 7) // 8
        return self.v.to_bytes(nbytes, "little")


_XP = (11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261)
_M64 = (1 << 64) - 1


def xxh64(data: bytes, seed: int = 0) -> int:
    """XXH64 (the frame's content checksum is its low 32 bits), from the algorithm description."""
    p1, p2, p3, p4, p5 = _XP
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & _M64                    # noqa: E731
    rnd = lambda acc, v: (rotl((acc + v * p2) & _M64, 31) * p1) & _M64          # noqa: E731
    le = lambda i, k: int.from_bytes(data[i:i + k], "little")                  # noqa: E731
    n, i = len(data), 0
    if n >= 32:
        v = [(seed + p1 + p2) & _M64, (seed + p2) & _M64, seed, (seed - p1) & _M64]
        while i + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], le(i + 8 * k, 8))
            i += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & _M64
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * p1 + p4) & _M64
    else:
        h = (seed + p5) & _M64
    h = (h + n) & _M64
    while i + 8 <= n:
        h = (rotl(h ^ rnd(0, le(i, 8)), 27) * p1 + p4) & _M64
        i += 8
    if i + 4 <= n:
        h = (rotl(h ^ (le(i, 4) * p1) & _M64, 23) * p2 + p3) & _M64
        i += 4
    while i < n:
        h = (rotl(h ^ (data[i] * p5) & _M64, 11) * p1) & _M64
        i += 1
    h = ((h ^ (h >> 33)) * p2) & _M64
    h = ((h ^ (h >> 29)) * p3) & _M64
    return h ^ (h >> 32)


class FseDesc:
    """Writer of an FSE table description (RFC 8878 4.1.1), one field at a time: ``count`` a normalized count (-1 for
    "less than one"), ``zeros`` the repeat flags that follow a count of 0 (how many *more* symbols have count 0)."""

    def __init__(self, log, log_field=None):
        self.bw = BitWriter()
        self.bw.bits(log - 5 if log_field is None else log_field, 4)
        self.remaining, self.threshold, self.nbits = (1 << log) + 1, 1 << log, log + 1
        self.flags = []                                   # the zero-run values written

    def count(self, c):
        value, mx = c + 1, (2 * self.threshold - 1) - self.remaining
        assert 0 <= value <= self.remaining, (c, self.remaining)
        if value < mx:
            self.bw.bits(value, self.nbits - 1)
        elif value < self.threshold:
            self.bw.bits(value, self.nbits)
        else:
            self.bw.bits(value + mx, self.nbits)
        self.remaining -= abs(c)
        while self.remaining < self.threshold:
            self.nbits -= 1
            self.threshold >>= 1
        return self

    def zeros(self, more):
        self.flags.append(more)
        while more >= 3:                                  # sixteen 1-bits in a row are the "24 zeros" form
            self.bw.bits(3, 2)
            more -= 3
        self.bw.bits(more, 2)
        return self

    def finish(self):
        return self.bw.getvalue()


def fse_description(norm, log, info=None):
    """The description of ``norm`` (which ends with its last nonzero count); ``info``: a dict that takes the zero-run
    values written and the number of bits."""
    assert sum(abs(c) for c in norm) == 1 << log and norm[-1] != 0, (norm, log)
    d = FseDesc(log)
    s = 0
    while s < len(norm):
        d.count(norm[s])
        s += 1
        if norm[s - 1] == 0:
            more = 0
            while norm[s + more] == 0:
                more += 1
            d.zeros(more)
            s += more
    assert d.remaining == 1
    if info is not None:
        info.setdefault("zero_runs", []).extend(d.flags)
        info.setdefault("desc_bits", []).append(d.bw.bitpos)
    return d.finish()


def _state_of(table, symbol, then, rnd, want=None):
    """A state that decodes ``symbol`` and whose update can reach state ``then`` (for each symbol the cells' ranges
    [baseline, baseline + 2^nbits) tile the whole table, so one exists); any cell of the symbol if ``then`` is None."""
    cells = [i for i, c in enumerate(table) if c[0] == symbol and (then is None or c[2] <= then < c[2] + (1 << c[1]))]
    assert cells, ("no state", symbol, then)
    if want is not None:
        cells = [i for i in cells if want(table[i])] or cells
    return rnd.choice(cells)


def flat_norm(symbols, log):
    """A distribution over 0..max(symbols): 1 for every symbol present, the rest of 2^log to the commonest."""
    norm = [0] * (max(symbols) + 1)
    for s in set(symbols):
        norm[s] = 1
    top = max(set(symbols), key=lambda s: (symbols.count(s), -s))
    norm[top] += (1 << log) - sum(norm)
    assert norm[top] >= 1
    return norm


def huf_codes(weights):
    """{symbol: (code, nbits)} of a complete weight list (the last symbol's implied weight included), and the tree's
    depth: symbols of weight w take 2^(w-1) consecutive table cells, weights ascending, then symbol order."""
    total = sum(1 << (w - 1) for w in weights if w)
    maxb = total.bit_length() - 1
    assert total == 1 << maxb and 1 <= maxb <= 11 and weights[-1], (total, weights)
    codes, start = {}, 0
    for k in range(1, maxb + 1):
        for s, w in enumerate(weights):
            if w == k:
                codes[s] = (start >> (k - 1), maxb + 1 - k)
                start += 1 << (k - 1)
    return codes, maxb


def huf_stream(data, codes):
    w = BackWriter()
    for b in reversed(data):
        w.put(*codes[b])
    return w.finish(), w.n - 1


def huf_tree_direct(listed):
    assert 1 <= len(listed) <= 128
    ws = list(listed) + [0]
    return bytes([127 + len(listed)]) + bytes((ws[i] << 4) | ws[i + 1] for i in range(0, len(listed), 2))


def huf_tree_fse(listed, log, norm=None, log_field=None, rnd=None):
    """FSE-compressed weights: a table description, then one backward bitstream that two states read in turn.  The
    decoder stops when an update reads past the start of the stream: the stream ends exactly before the update that
    follows the last weight but one, which is taken from a cell that reads at least one bit."""
    rnd = rnd or random.Random(len(listed))
    n = len(listed)
    assert n >= 2
    norm = norm or flat_norm(list(listed), log)
    tab = fse_table(norm, log)
    st = [None] * n
    st[n - 1] = _state_of(tab, listed[n - 1], None, rnd)
    st[n - 2] = _state_of(tab, listed[n - 2], None, rnd, want=lambda c: c[1] >= 1)
    assert tab[st[n - 2]][1] >= 1
    for i in range(n - 3, -1, -1):
        st[i] = _state_of(tab, listed[i], st[i + 2], rnd)
    w = BackWriter()
    for i in range(n - 3, -1, -1):
        c = tab[st[i]]
        w.put(st[i + 2] - c[2], c[1])
    w.put(st[1], log)
    w.put(st[0], log)
    desc = fse_description(norm, log)
    if log_field is not None:
        desc = bytes([(desc[0] & 0xF0) | log_field]) + desc[1:]
    body = desc + w.finish()
    assert len(body) < 128, len(body)
    return bytes([len(body)]) + body


def zcode(value, base, bits):
    i = max(k for k in range(len(base)) if base[k] <= value)
    assert value - base[i] < (1 << bits[i]), value
    return i, value - base[i]


def OFF(offset):
    """Offset value of a real offset (values 1..3 are the repeat codes)."""
    return offset + 3


class ZFrame:
    """One frame: block writers that emit the bytes and expand the same description into ``out``.

    Literals: ("raw", data, header bytes 1..3) | ("rle", byte, count, header bytes)
    | ("huf", data, weights, streams, size format, "direct" | ("fse", log[, norm])) | ("treeless", data, streams,
    size format).  Sequences: (literal length, offset value, match length)."""

    def __init__(self, window=(10, 0), fcs=None, checksum=False, did=0, seed=1):
        self.window, self.fcs, self.checksum, self.did = window, fcs, checksum, did
        self.blocks = []
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.tabs = {}                   # kind -> (cells, log) of the last table
        self.huf = None                  # (codes, depth) of the last tree
        self.rnd = random.Random(seed)
        self.broken = False              # a sequence had no valid expansion (malformed vectors)
        self.info = {"cell_bits": set(), "marker_bit": [], "seq_bytes": [], "seq_bits": [], "rep_idx": set(),
                     "huf_stream_bytes": [], "huf_depth": []}

    # ---- blocks
    def _block(self, typ, size, payload):
        self.blocks.append((typ, size, bytes(payload)))
        return self

    def raw(self, data):
        self.out += data
        return self._block(0, len(data), data)

    def rle(self, byte, count):
        self.out += bytes([byte]) * count
        return self._block(1, count, bytes([byte]))

    def compressed(self, lits, seqs, ll=PRE, of=PRE, ml=PRE, size=None, **kw):
        sec, data = self._literals(lits)
        body = sec + self._sequences(seqs, data, {"ll": ll, "of": of, "ml": ml}, **kw)
        return self._block(2, len(body) if size is None else size, body)

    # ---- literals
    @staticmethod
    def _lit_header(lt, regen, hdr):
        if hdr == 1:                                      # (size format ?0: bit 3 is the size's lowest bit)
            assert regen < 32
            return bytes([lt | (regen << 3)])
        assert regen < (1 << (12 if hdr == 2 else 20))
        return (lt | ((1 if hdr == 2 else 3) << 2) | (regen << 4)).to_bytes(hdr, "little")

    def _literals(self, lits):
        kind = lits[0]
        if kind == "raw":
            data = lits[1]
            return self._lit_header(0, len(data), *lits[2:]) + data, data
        if kind == "rle":
            return self._lit_header(1, lits[2], *lits[3:]) + bytes([lits[1]]), bytes([lits[1]]) * lits[2]
        tree = b""
        if kind == "huf":
            _, data, weights, streams, sf, how = lits[:6]
            self.huf = huf_codes(weights)
            listed = weights[:-1]
            tree = huf_tree_direct(listed) if how == "direct" else huf_tree_fse(listed, *how[1:], rnd=self.rnd)
            opts = lits[6] if len(lits) > 6 else {}
        else:
            _, data, streams, sf = lits[:4]
            opts = lits[4] if len(lits) > 4 else {}
        tree = opts.get("tree", tree)
        assert (streams, sf) in ((1, 0), (4, 1), (4, 2), (4, 3))
        body = b""
        if self.huf is not None:
            codes = self.huf[0]
            self.info["huf_depth"].append(self.huf[1])
            if streams == 1:
                body, _ = huf_stream(data, codes)
                self.info["huf_stream_bytes"].append(len(body))
            else:
                per = (len(data) + 3) // 4
                parts = [huf_stream(data[k * per:(k + 1) * per if k < 3 else len(data)], codes)[0] for k in range(4)]
                self.info["huf_stream_bytes"] += [len(p) for p in parts]
                jump = opts.get("jump", [len(p) for p in parts[:3]])
                body = b"".join(j.to_bytes(2, "little") for j in jump) + b"".join(parts)
        body = opts.get("body", lambda b: b)(body)
        regen = len(data) + opts.get("regen_delta", 0)
        csize = len(tree) + len(body) + opts.get("csize_delta", 0)
        lt = 2 if kind == "huf" else 3
        width, nbytes = ((10, 3), (10, 3), (14, 4), (18, 5))[sf]
        assert regen < (1 << width) and csize < (1 << width), (regen, csize, sf)
        hdr = (lt | (sf << 2) | (regen << 4) | (csize << (4 + width))).to_bytes(nbytes, "little")
        return hdr + tree + body, data

    # ---- sequences
    def _table(self, kind, mode):
        """(mode number, bytes written for it); sets self.tabs[kind]."""
        if mode == PRE:
            norm, log = ZSTD_DEFAULTS[kind]
            self.tabs[kind] = (fse_table(norm, log), log)
            return 0, b""
        if mode == REP:
            return 3, b""
        if mode[0] == "rle":
            self.tabs[kind] = ([(mode[1], 0, 0)], 0)
            return 1, bytes([mode[1]])
        _, norm, log, desc = mode
        self.tabs[kind] = (fse_table(norm, log), log)
        return 2, fse_description(norm, log, self.info) if desc is None else desc

    def _expand(self, seqs, data):
        out, rep, lp = self.out, self.rep, 0
        for L, ofv, M in seqs:
            if self.broken or L > len(data) - lp:
                self.broken = True
                return
            out += data[lp:lp + L]
            lp += L
            if ofv > 3:
                off = ofv - 3
                rep[:] = [off, rep[0], rep[1]]
            else:
                idx = ofv - 1 + (L == 0)
                self.info["rep_idx"].add(idx)
                off = rep[0] - 1 if idx == 3 else rep[idx]
                if idx == 1:
                    rep[:] = [off, rep[0], rep[2]]
                elif idx >= 2:
                    rep[:] = [off, rep[0], rep[1]]
            if not 1 <= off <= len(out):
                self.broken = True
                return
            if off >= M:
                out += out[len(out) - off:len(out) - off + M]
            else:
                for _ in range(M):
                    out.append(out[-off])
        out += data[lp:]

    def _sequences(self, seqs, data, modes, count_bytes=None, reserved=0, pad_low=0, drop_low=0, tail=None):
        n = len(seqs)
        self._expand(seqs, data)
        if count_bytes is None:
            count_bytes = 1 if n < 128 else 2 if n < 0x7F00 else 3
        if count_bytes == 1:
            assert n < 128
            head = bytes([n])
        elif count_bytes == 2:
            assert n < 0x7F00
            head = bytes([128 + (n >> 8), n & 255])
        else:
            assert 0x7F00 <= n < 0x7F00 + 65536
            head = b"\xff" + (n - 0x7F00).to_bytes(2, "little")
        if n == 0:
            return head
        mb, descs = reserved, b""
        for k, kind in enumerate(ZSTD_KINDS):
            m, d = self._table(kind, modes[kind])
            mb |= m << (6 - 2 * k)
            descs += d
        head += bytes([mb]) + descs
        if tail is not None:                              # a malformed vector's own bitstream
            return head + tail
        tabs = [self.tabs[k][0] for k in ZSTD_KINDS]
        logs = [self.tabs[k][1] for k in ZSTD_KINDS]
        code = []
        for L, ofv, M in seqs:
            oc = ofv.bit_length() - 1
            lc, mc = zcode(L, ZLL_BASE, ZLL_BITS), zcode(M, ZML_BASE, ZML_BITS)
            code.append((lc + (ZLL_BITS[lc[0]],), (oc, ofv - (1 << oc), oc), mc + (ZML_BITS[mc[0]],)))
        # For each symbol the cells' ranges tile the table, so the state of the last sequence fixes every earlier
        # one.  Of the chains that end in each cell of the last symbol, take the one whose updates read the most
        # different bit counts (0 bits and `log` bits first).
        chains = []
        for k in range(3):
            cover = {}
            for idx, c in enumerate(tabs[k]):
                for t in range(c[2], c[2] + (1 << c[1])):
                    cover[(c[0], t)] = idx
            best = None
            for last in (idx for idx, c in enumerate(tabs[k]) if c[0] == code[n - 1][k][0]):
                chain = [last]
                for i in range(n - 2, -1, -1):
                    chain.append(cover[(code[i][k][0], chain[-1])])
                chain.reverse()
                read = {tabs[k][x][1] for x in chain[:-1]}
                score = (len(read & {0, logs[k]}), len(read), self.rnd.random())
                if best is None or score > best[0]:
                    best = (score, chain)
                if n > 1000:
                    break
            assert best is not None, ("no state decodes", ZSTD_KINDS[k], code[n - 1][k][0])
            chains.append(best[1])
        st = list(zip(*chains))
        w = BackWriter()
        w.put(0, pad_low)
        for i in range(n - 1, -1, -1):
            if i + 1 < n:                                 # state updates are read LL, ML, OF
                for k in (1, 2, 0):
                    c = tabs[k][st[i][k]]
                    w.put(st[i + 1][k] - c[2], c[1])
                    self.info["cell_bits"].add((ZSTD_KINDS[k], logs[k], c[1]))
            for k in (0, 2, 1):                           # extra bits are read OF, ML, LL
                w.put(code[i][k][1], code[i][k][2])
        for k in (2, 1, 0):                               # initial states are read LL, OF, ML
            w.put(st[0][k], logs[k])
        if drop_low:
            w.v >>= drop_low
            w.n -= drop_low
        self.info["marker_bit"].append(w.n % 8)
        self.info["seq_bits"].append(w.n)
        bits = w.finish()
        self.info["seq_bytes"].append(len(bits))
        return head + bits

    # ---- frame
    def finish(self, magic=ZSTD_MAGIC, fhd_or=0, did_value=0, fcs_delta=0, no_last=False, fcs_value=None):
        single = self.window is None
        fcs = self.fcs if self.fcs is not None else (1 if single else 0)
        assert fcs in (0, 1, 2, 4, 8) and (fcs != 1 or single) and (fcs != 0 or not single)
        n = (len(self.out) if fcs_value is None else fcs_value) + fcs_delta
        fhd = ({0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs] << 6) | (single << 5) | (self.checksum << 2) | \
            {0: 0, 1: 1, 2: 2, 4: 3}[self.did] | fhd_or
        f = bytearray(magic.to_bytes(4, "little") + bytes([fhd]))
        if not single:
            f.append((self.window[0] << 3) | self.window[1])
        f += did_value.to_bytes(self.did, "little")
        if fcs:
            f += (n - 256 if fcs == 2 else n).to_bytes(fcs, "little")
        self.header_len = len(f)
        for i, (typ, size, payload) in enumerate(self.blocks):
            last = i + 1 == len(self.blocks) and not no_last
            f += (int(last) | (typ << 1) | (size << 3)).to_bytes(3, "little") + payload
        if self.checksum:
            f += (xxh64(bytes(self.out)) & 0xFFFFFFFF).to_bytes(4, "little")
        return bytes(f), bytes(self.out)


def huf_chain(depth, syms):
    """Weights of a tree whose code lengths are 1, 2, .., depth, depth over ``syms`` (in that order)."""
    assert len(syms) == depth + 1 and len(set(syms)) == len(syms)
    w = [0] * (max(syms) + 1)
    for k, s in enumerate(syms):
        w[s] = max(depth - k, 1)
    return w


def huf_data(weights, n, seed):
    """n bytes over the symbols of ``weights`` (commoner for heavier ones), every symbol at least once."""
    syms = [s for s, w in enumerate(weights) if w]
    rnd = random.Random(seed)
    body = rnd.choices(syms, weights=[1 << weights[s] for s in syms], k=max(n - len(syms), 0)) + syms
    rnd.shuffle(body)
    return bytes(body[:n]) if n < len(syms) else bytes(body)


def znorm(log, counts, fill):
    """Normalized counts from {symbol: count}; ``fill`` takes what is left of 2^log."""
    norm = [0] * (max(list(counts) + [fill]) + 1)
    for s, c in counts.items():
        norm[s] = c
    norm[fill] += (1 << log) - sum(abs(c) for c in norm)
    assert norm[fill] >= 1 and norm[-1] != 0, norm
    return norm


def runs_norm(pairs):
    """Normalized counts from [(count, zero counts that follow it)]."""
    norm = []
    for c, z in pairs:
        norm += [c] + [0] * z
    return norm


def rle_history(f, total, seed, first=509):
    """``total`` bytes of history as RLE blocks of 509 bytes (4 bytes of frame each) with unrelated values: a match of
    more than 509 bytes always crosses a boundary, so a wrong offset shows."""
    rnd = random.Random(seed)
    left, size, prev = total, first, -1
    while left:
        n = min(size, left)
        v = rnd.choice([x for x in range(256) if x != prev])
        f.rle(v, n)
        prev, left, size = v, left - n, 509
    return f


ZH = noise(1100, 900)              # a raw first block: history for offsets up to 1100


@functools.lru_cache(maxsize=None)
def zstd_vectors():
    """(valid, malformed, coverage) Zstandard frames; ``coverage`` collects what the writers actually emitted."""
    V, B = [], []
    cov = {"cell_bits": set(), "marker_bit": set(), "seq_bytes": set(), "rep_idx": set(), "zero_runs": set(),
           "desc_bits": set(), "huf_stream_bytes": set(), "huf_depth": set()}

    def add(name, f, **kw):
        comp, out = f.finish(**kw)
        assert not f.broken, name
        assert len(out) <= 1 << 20, (name, len(out))
        V.append(Vec(name, comp, out))
        for k, v in f.info.items():
            if k in cov:
                cov[k] |= set(v)
        return f

    def bad(name, f, klass, cap, stream_ok=False, cut=None, **kw):
        comp = f if isinstance(f, bytes) else f.finish(**kw)[0]
        B.append(Bad(name, comp if cut is None else comp[:cut], None, klass, cap, stream_ok))

    h8, h16, h70 = ZH[:8], ZH[:16], ZH[:70]
    text = b"{\"deviceId\":17,\"temperature\":21.5,\"status\":\"ok\"}\n" * 4
    few = [(4, OFF(3), 5), (0, 1, 3), (2, 2, 40), (7, OFF(30), 9)]

    # ------------------------------------------------------------------------------------------------- frame
    add("fcs_1_byte_single_segment", ZFrame(window=None, fcs=1).raw(noise(100, 901)))
    add("fcs_2_bytes_at_256", ZFrame(fcs=2).raw(noise(256, 902)))
    add("fcs_2_bytes_at_65791_single_segment", ZFrame(window=None, fcs=2).raw(noise(65791, 903)))
    add("fcs_4_bytes", ZFrame(fcs=4).raw(h70).compressed(("raw", text[:31], 1), few))
    add("fcs_4_bytes_single_segment", ZFrame(window=None, fcs=4).raw(ZH).compressed(("raw", text[:31], 1), few))
    add("fcs_8_bytes", ZFrame(fcs=8).raw(h70).compressed(("raw", text[:31], 1), few))
    add("fcs_8_bytes_single_segment", ZFrame(window=None, fcs=8).raw(ZH).compressed(("raw", text[:31], 1), few))
    add("no_fcs_window_descriptor", ZFrame().raw(h70).compressed(("raw", text[:31], 1), few))
    add("window_descriptor_1_kib", ZFrame(window=(0, 0)).raw(h70).compressed(("raw", text[:31], 1), few))
    add("window_descriptor_mantissa_7", ZFrame(window=(3, 7), fcs=2).raw(ZH).compressed(("raw", text[:31], 1), few))
    add("checksum", ZFrame(checksum=True).raw(ZH).compressed(("raw", text[:31], 1), few).rle(0x33, 77))
    add("checksum_single_segment_fcs", ZFrame(window=None, fcs=4, checksum=True).raw(ZH).rle(9, 1))
    add("dictionary_id_0_in_1_byte", ZFrame(did=1).raw(h70))
    add("dictionary_id_0_in_2_bytes", ZFrame(did=2, fcs=4).raw(h70))
    add("dictionary_id_0_in_4_bytes", ZFrame(did=4, window=None, fcs=1).raw(h70))
    add("empty_frame_single_segment", ZFrame(window=None, fcs=1).raw(b""))
    add("empty_frame_window_descriptor", ZFrame().raw(b""))
    add("empty_frame_checksum", ZFrame(checksum=True).raw(b""))
    add("empty_frame_rle_block_of_0", ZFrame().rle(0x77, 0))
    add("one_raw_block", ZFrame().raw(noise(333, 904)))
    add("one_raw_block_of_1", ZFrame().raw(b"\x5a"))
    add("one_rle_block", ZFrame().rle(0x41, 333))
    add("one_rle_block_of_1", ZFrame().rle(0x41, 1))
    add("one_rle_block_of_block_maximum", ZFrame().rle(0x42, ZBLOCK_MAX))
    add("one_raw_block_of_block_maximum", ZFrame().raw(noise(ZBLOCK_MAX, 905)))
    f = ZFrame(fcs=2)
    for k in range(3):
        f.raw(noise(40 + k, 906 + k)).compressed(("raw", text[k:k + 20], 1), [(5, OFF(9 + k), 12), (3, 1, 4)])
        f.rle(0x61 + k, 19 * k).compressed(("rle", 0x2A, 6, 1), [(2, OFF(50), 33)], ml=RLE(30))
    add("raw_rle_compressed_interleaved", f)

    # ---------------------------------------------------------------------------------------------- literals
    for kind in ("raw", "rle"):
        for hdr, sizes in ((1, (0, 31)), (2, (0, 31, 32, 4095)), (3, (0, 31, 32, 4095, 4096))):
            for size in sizes:
                lits = ("raw", noise(size, 910 + size), hdr) if kind == "raw" else ("rle", 0x6B, size, hdr)
                add(f"literals_{kind}_{size}_header_{hdr}",
                    ZFrame().raw(h16).compressed(lits, [(min(size, 5), OFF(9), 4)]))
    w4 = huf_chain(3, [0x65, 0x20, 0x74, 0x61])
    add("huffman_1_stream", ZFrame().compressed(("huf", huf_data(w4, 300, 1), w4, 1, 0, "direct"), []))
    add("huffman_1_stream_1_literal", ZFrame().compressed(("huf", b"\x65", w4, 1, 0, "direct"), []))
    add("huffman_1_stream_1023", ZFrame().compressed(("huf", huf_data(w4, 1023, 2), w4, 1, 0, "direct"), []))
    for regen, sf in ((8, 1), (1023, 1), (1023, 2), (1024, 2), (16383, 2), (16383, 3), (16384, 3), (300, 3), (300, 2)):
        add(f"huffman_4_streams_{regen}_format_{sf}",
            ZFrame().raw(h8).compressed(("huf", huf_data(w4, regen, regen + sf), w4, 4, sf, "direct"),
                                        [(regen // 2, OFF(5), 6)]))
    w1 = [0] * 0x30 + [1, 1]
    for per, last, what in ((40, 40, "shorter_than_8"), (60, 60, "of_8"), (100, 100, "longer_than_8"),
                            (60, 57, "regen_not_multiple_of_4"), (2, 1, "of_1_byte_regen_7")):
        d = huf_data(w1, 3 * per + last, per + last)
        f = add(f"huffman_4_streams_{what}_bytes", ZFrame().compressed(("huf", d, w1, 4, 1, "direct"), []))
        want = {"shorter_than_8": {6}, "of_8": {8}, "longer_than_8": {13}, "regen_not_multiple_of_4": {8},
                "of_1_byte_regen_7": {1}}[what]
        assert set(f.info["huf_stream_bytes"]) == want, (what, f.info["huf_stream_bytes"])

    # ----------------------------------------------------------------------------------------- Huffman trees
    order = [0x41, 0x7A, 0x30, 0x0A, 0x55, 0xC3, 0x01, 0x99, 0x61, 0xFE, 0x10, 0x80]
    for depth in range(1, 12):
        w = huf_chain(depth, order[:depth + 1])
        how = "direct" if max(order[:depth + 1]) <= 128 else ("fse", 6 if depth % 2 else 5)
        streams, sf = ((1, 0), (4, 1))[depth % 2]
        add(f"huffman_depth_{depth}", ZFrame().raw(h8).compressed(
            ("huf", huf_data(w, 260 + depth, depth), w, streams, sf, how), [(100, OFF(3), 4)]))
    for nlisted, w in ((1, [1, 1]), (2, [2, 1, 1]), (127, [1] * 128), (128, [2] + [1] * 126 + [0, 8])):
        assert len(w) == nlisted + 1
        add(f"huffman_direct_{nlisted}_weights",
            ZFrame().compressed(("huf", huf_data(w, 400, nlisted), w, 4, 1, "direct"), []))
    for last_sym in (0x34, 0x35):                          # 52 and 53 weights listed: the loop ends on either state
        w = huf_chain(3, [0x30, 0x31, 0x33, last_sym])
        for log in (5, 6):
            add(f"huffman_fse_{last_sym}_weights_accuracy_{log}",
                ZFrame().compressed(("huf", huf_data(w, 200, last_sym), w, 1, 0, ("fse", log)), []))
    w = [1] * 256
    for log in (5, 6):
        add(f"huffman_fse_255_weights_accuracy_{log}",
            ZFrame().compressed(("huf", noise(500, 920 + log), w, 4, 1, ("fse", log, [1, (1 << log) - 1])), []))
    w = [0] * 200 + [4, 4, 4, 3, 2, 1] + [0] * 49 + [1]          # symbol 255 takes the implied weight
    add("huffman_fse_mixed_weights_symbol_255", ZFrame().compressed(
        ("huf", huf_data(w, 700, 5), w, 4, 1, ("fse", 6)), []))
    d = huf_data(w4, 120, 7)
    f = ZFrame().raw(h8).compressed(("huf", d, w4, 1, 0, "direct"), few)
    f.compressed(("treeless", d[:50], 1, 0), [(10, OFF(70), 5)])
    f.compressed(("raw", text[:20], 1), [(3, 1, 3)]).compressed(("treeless", d[10:110], 4, 1), [(50, 2, 9)])
    f.raw(b"between").rle(0x21, 13).compressed(("treeless", d[60:90], 4, 2), [])
    f.compressed(("rle", 0x7E, 9, 1), []).raw(b"").compressed(("treeless", d[:7], 4, 3), [(7, OFF(1), 30)])
    add("treeless_literals_across_compressed_raw_rle_blocks", f)

    # -------------------------------------------------------------------------------------- FSE descriptions
    def seqs_with(rnd, llc, ofc, mlc, n):
        """n sequences that use every given code (extras random; offsets stay inside ZH).  The last three use the
        first code of each list: a symbol with more than half of the table has its cells of 0 bits where the state
        value is smallest, and only a run of that symbol at the end of the block is free to pass through them."""
        out = []
        for i in range(n):
            j = 0 if i >= n - 3 else i
            a, b, c = llc[j % len(llc)], ofc[j % len(ofc)], mlc[j % len(mlc)]
            assert ZLL_BITS[a] <= 8 and b <= 9 and ZML_BITS[c] <= 8
            ofv = (1 << b) + rnd.getrandbits(b)
            if b < 2 and a == 0 and ofv == 3:
                ofv = 2                                    # (rep0 - 1 needs a known rep0: the repeat-offset vectors)
            out.append((ZLL_BASE[a] + rnd.getrandbits(ZLL_BITS[a]), ofv, ZML_BASE[c] + rnd.getrandbits(ZML_BITS[c])))
        return out

    def fse_frame(seed, ll, of, ml, n=48, **kw):
        rnd = random.Random(seed)
        tabs = {}
        for kind, mode in (("ll", ll), ("of", of), ("ml", ml)):
            norm = ZSTD_DEFAULTS[kind][0] if mode == PRE else mode[1]
            tabs[kind] = [s for s, c in enumerate(norm) if c and (kind != "ll" or ZLL_BITS[s] <= 8) and
                          (kind != "of" or s <= 9) and (kind != "ml" or ZML_BITS[s] <= 8)]
        seqs = seqs_with(rnd, tabs["ll"], tabs["of"], tabs["ml"], n)
        lits = noise(sum(s[0] for s in seqs) + 5, seed)
        return ZFrame(seed=seed).raw(ZH).compressed(("raw", lits, 3), seqs, ll=ll, of=of, ml=ml, **kw)

    for log in range(5, 10):
        half = (1 << (log - 1)) + 3                        # more than half the table: cells that read 0 bits
        lln = znorm(log, {0: half, 3: -1, 7: 2, 16: 1, 24: -1, 27: 1}, 1)
        mln = znorm(log, {0: half, 1: -1, 5: 1, 33: 2, 40: -1, 43: 1}, 2)
        add(f"fse_ll_accuracy_{log}", fse_frame(930 + log, FSE(lln, log), PRE, PRE))
        add(f"fse_ml_accuracy_{log}", fse_frame(940 + log, PRE, PRE, FSE(mln, log)))
        if log <= 8:
            ofn = znorm(log, {0: half, 2: 1, 3: -1, 5: 2, 9: -1}, 1)
            add(f"fse_of_accuracy_{log}", fse_frame(950 + log, PRE, FSE(ofn, log), PRE))
            add(f"fse_all_accuracy_{log}", fse_frame(960 + log, FSE(lln, log), FSE(ofn, log), FSE(mln, log), n=60))
    for kind in ZSTD_KINDS:                                # states with log bits and with 0 bits were both used
        for log in range(5, ZSTD_MAX_LOG[kind] + 1):
            assert {(kind, log, log), (kind, log, 0)} <= cov["cell_bits"], (kind, log)
    # zero runs of 0, 1, 2, 3, 4 and 30 more symbols (the last has the 16-bit form and ends at the last symbol, 52)
    mln = runs_norm([(20, 1), (5, 2), (5, 3), (5, 4), (3, 5), (7, 31), (19, 0)])
    assert len(mln) == 53
    add("fse_ml_every_zero_run_form", fse_frame(970, PRE, PRE, FSE(mln, 6)))
    lln = runs_norm([(9, 1), (-1, 0), (9, 4), (6, 25), (-1, 0), (6, 0)])   # 24 more: the 16-bit form and flag 0
    assert len(lln) == 36
    add("fse_ll_zero_run_of_24_more", fse_frame(971, FSE(lln, 5), PRE, PRE))
    ofn = runs_norm([(10, 4), (10, 1), (11, 23), (-1, 0)])
    assert len(ofn) == 32
    add("fse_of_zero_run_reaches_symbol_31", fse_frame(972, PRE, FSE(ofn, 5), PRE))
    assert cov["zero_runs"] >= {0, 1, 2, 3, 4, 22, 24, 30}, cov["zero_runs"]
    assert {b % 8 for b in cov["desc_bits"]} >= {0, 1, 3, 5}, cov["desc_bits"]       # ends mid-byte and on a byte
    add("fse_ll_highest_symbol_35_used", ZFrame().raw(h16).compressed(
        ("raw", noise(65540, 973), 3), [(65536 + 3, OFF(11), 4), (0, 1, 3)], ll=FSE(znorm(5, {0: 16}, 35), 5)))
    add("fse_ml_highest_symbol_52_used", ZFrame().raw(h16).compressed(
        ("raw", b"ab", 1), [(1, OFF(11), 65539 + 77), (1, 1, 3)], ml=FSE(znorm(5, {0: 16}, 52), 5)))
    # every cell belongs to a "less than one" symbol: libzstd accepts it (all cells read `log` bits)
    add("fse_ll_every_cell_less_than_one", fse_frame(974, FSE([-1] * 32, 5), PRE, PRE))
    add("fse_of_every_cell_less_than_one", fse_frame(975, PRE, FSE([-1] * 32, 5), PRE))
    add("fse_ml_every_cell_less_than_one", fse_frame(976, PRE, PRE, FSE([0] * 3 + [-1] * 32, 5)))

    # ------------------------------------------------------------------------------------------------- modes
    lln, ofn, mln = znorm(5, {0: 8, 2: 8, 5: -1}, 1), znorm(5, {1: 4, 4: 8, 6: -1}, 3), znorm(6, {0: 9, 1: 3, 9: -1}, 4)
    a = [(2, OFF(5), 7), (1, OFF(13), 3), (5, OFF(61), 12), (0, 2, 4)]
    f = ZFrame().raw(h70)
    f.compressed(("raw", text[:30], 1), a)                                              # predefined
    f.compressed(("raw", text[:30], 1), a, ll=REP, of=REP, ml=REP)                      # repeat after predefined
    r = [(3, OFF(6), 8)] * 3
    f.compressed(("raw", text[:9], 1), r, ll=RLE(3), of=RLE(3), ml=RLE(5))              # RLE
    f.compressed(("raw", text[:12], 1), r, ll=REP, of=REP, ml=REP)                      # repeat after RLE
    f.compressed(("raw", text[:30], 1), a, ll=FSE(lln, 5), of=FSE(ofn, 5), ml=FSE(mln, 6))
    f.compressed(("raw", text[:11], 1), [])                                             # no sequences: tables stay
    f.raw(b"raw").rle(0x0D, 5)
    f.compressed(("raw", text[:30], 1), a, ll=REP, of=REP, ml=REP)                      # repeat after FSE
    f.compressed(("raw", text[:30], 1), [(2, OFF(5), 7), (1, OFF(13), 7)], ll=PRE, of=REP, ml=RLE(4))
    f.compressed(("raw", text[:30], 1), [(2, OFF(9), 7)] * 2, ll=RLE(2), of=PRE, ml=REP)
    f.compressed(("raw", text[:30], 1), [(2, OFF(13), 7), (1, OFF(14), 3), (5, OFF(28), 12)], ll=FSE(lln, 5), of=RLE(4),
                 ml=PRE)
    f.compressed(("raw", text[:30], 1), [(5, OFF(15), 12)] * 3, ll=REP, of=REP, ml=FSE(mln, 6))
    add("every_mode_and_repeat_after_each", f)

    # ------------------------------------------------------------------------------------------------- codes
    for c in range(36):
        for ex in sorted({0, (1 << ZLL_BITS[c]) - 1}):
            n = min(ZLL_BASE[c] + ex, ZBLOCK_MAX - 16)
            lits = ("raw", noise(n + 2, 1000 + c), 1 if n + 2 < 32 else 2 if n + 2 < 4096 else 3)
            add(f"ll_code_{c}_length_{n}", ZFrame(seed=c).raw(h16).compressed(lits, [(n, OFF(7 + c), 3)]))
    for c in range(53):
        for ex in sorted({0, (1 << ZML_BITS[c]) - 1}):
            n = min(ZML_BASE[c] + ex, ZBLOCK_MAX - 2)
            add(f"ml_code_{c}_length_{n}", ZFrame(seed=c).raw(h16).compressed(("raw", b"xy", 1), [(2, OFF(5), n)]))
    f = rle_history(ZFrame(window=(11, 0)), 525000, 1100)
    seqs = [(1, 1, 520), (1, 2, 521), (1, 3, 522)]         # offset codes 0 and 1: the initial repeat offsets
    for c in range(2, 20):
        seqs += [(1, 1 << c, 520 + c)] + ([(1, (2 << c) - 1, 600 + c)] if c < 19 else [])
    add("offset_codes_0_to_19", f.compressed(("raw", noise(len(seqs), 1101), 2), seqs))
    f = rle_history(ZFrame(window=(11, 0)), (1 << 20) - 4, 1102, first=2)
    add("offset_code_19_extra_all_ones", f.compressed(("raw", b"", 1), [(0, (1 << 20) - 1, 3)]))
    # one sequence of 17 + 16 + 15 extra bits and 9 + 9 + 8 bits of state updates: the container reloads inside it
    lln, mln = znorm(9, {34: -1, 1: -1, 2: -1}, 0), znorm(9, {52: -1, 1: -1, 2: -1}, 0)
    ofn = znorm(8, {17: -1, 3: -1, 4: -1}, 2)
    f = rle_history(ZFrame(seed=5), 160000, 1103)
    seqs = [(2, OFF(9), 5), (32768 + 0x1ABC, (1 << 17) + 0xF0F3, 65539 + 8879), (1, OFF(13), 4), (2, OFF(2), 5)]
    f.compressed(("raw", noise(32768 + 0x1ABC + 9, 1104), 3), seqs, ll=FSE(lln, 9), of=FSE(ofn, 8), ml=FSE(mln, 9))
    add("sequence_of_74_bits", f)
    assert {("ll", 9, 9), ("ml", 9, 9), ("of", 8, 8)} <= set(f.info["cell_bits"])

    # --------------------------------------------------------------------------------------- sequence counts
    add("sequences_0_with_literals", ZFrame().compressed(("raw", text[:29], 1), []))
    add("sequences_0_without_literals", ZFrame().raw(h8).compressed(("raw", b"", 1), []).rle(1, 2))
    add("sequences_0_without_literals_only_block", ZFrame().compressed(("raw", b"", 1), []))
    add("sequences_1", ZFrame().compressed(("raw", text[:29], 1), [(9, OFF(4), 11)]))
    for n in (127, 128, 300):
        seqs = [(1, OFF(1 + i % 3), 3 + i % 5) for i in range(n)]
        add(f"sequences_{n}", ZFrame(seed=n).compressed(("raw", noise(n + 4, 1110 + n), 2), seqs))
    add("sequences_5_in_2_byte_count", ZFrame().compressed(("raw", text[:29], 1), [(3, OFF(2), 4)] * 5, count_bytes=2))
    add("sequences_127_in_2_byte_count", ZFrame().compressed(("raw", noise(127, 1115), 2), [(1, OFF(1), 3)] * 127,
                                                             count_bytes=2))
    # 32512 sequences of 0 bits each (all tables RLE): offset value 1 without literals swaps the first two repeat
    # offsets (1 and 4) every time
    f = ZFrame().raw(h8).compressed(("raw", b"", 1), [(0, 1, 3)] * 32512, ll=RLE(0), of=RLE(0), ml=RLE(0))
    assert len(f.finish()[1]) == 8 + 3 * 32512 and len(f.finish()[0]) < 40
    add("sequences_32512_in_3_byte_count", f)

    # -------------------------------------------------------------------------------------------- bitstreams
    llb = {ZLL_BITS[c]: c for c in range(35, 0, -1)}      # the lowest code above 0 for every number of extra bits
    mlb = {ZML_BITS[c]: c for c in range(52, -1, -1)}
    for total in list(range(8)) + [8 * k for k in range(1, 9)] + [13, 30, 66]:
        n, oc, lc, mc = min((n, ob, llb[lb], mlb[mb]) for n in (1, 2, 3, 4) for ob in range(10)
                            for lb in llb if lb <= 9 for mb in mlb if mb <= 9 if n * (ob + lb + mb) == total)
        rnd = random.Random(total)
        seqs = [(ZLL_BASE[lc] + rnd.getrandbits(ZLL_BITS[lc]), (1 << oc) + rnd.getrandbits(oc),
                 ZML_BASE[mc] + rnd.getrandbits(ZML_BITS[mc])) for _ in range(n)]
        f = ZFrame().raw(ZH).compressed(("raw", noise(sum(s[0] for s in seqs), 1120 + total), 2), seqs,
                                        ll=RLE(lc), of=RLE(oc), ml=RLE(mc))
        assert f.info["seq_bits"] == [total] and f.info["seq_bytes"] == [total // 8 + 1], (total, f.info)
        add(f"sequence_bitstream_of_{total}_bits", f)
    assert cov["marker_bit"] == set(range(8)) and cov["seq_bytes"] >= set(range(1, 10))

    # ---------------------------------------------------------------------------------------- repeat offsets
    f = ZFrame().raw(h70).compressed(("raw", noise(40, 1130), 2), [
        (4, OFF(10), 4), (1, OFF(20), 5), (2, OFF(30), 3),                  # history 30, 20, 10
        (3, 1, 5), (2, 2, 4), (1, 3, 6),                                    # literals: idx 0, 1, 2
        (0, 1, 3), (0, 2, 4), (0, 3, 5),                                    # none: idx 1, 2, 3 (rep0 - 1)
        (0, 3, 7), (5, 1, 3), (0, 1, 9), (0, 2, 4), (1, 3, 3), (0, 3, 4)])
    assert f.info["rep_idx"] == {0, 1, 2, 3}
    add("repeat_offsets_every_index", f)
    f = ZFrame().raw(h70).compressed(("raw", text[:20], 1), [(4, OFF(10), 4), (1, OFF(20), 5), (2, OFF(33), 3)])
    f.raw(b"raw block").compressed(("raw", text[:20], 1), [(3, 2, 5), (0, 2, 4)])
    f.rle(0x5F, 21).compressed(("raw", text[:20], 1), [(0, 3, 5), (4, 3, 4), (0, 1, 6)])
    f.compressed(("raw", text[:20], 1), []).compressed(("raw", text[:20], 1), [(1, 3, 8), (0, 3, 3)])
    add("repeat_offsets_across_compressed_raw_rle_blocks", f)
    add("initial_repeat_offsets_1_4_8", ZFrame().raw(ZH[:20]).compressed(("raw", text[:20], 1),
                                                                         [(1, 1, 5), (2, 2, 6), (3, 3, 7)]))
    add("initial_repeat_offsets_without_literals", ZFrame().raw(ZH[:20]).compressed(
        ("raw", text[:20], 1), [(0, 1, 5), (0, 2, 6), (0, 1, 4)]))
    add("initial_repeat_offset_8_at_position_8", ZFrame().compressed(("raw", text[:20], 1), [(8, 3, 5)]))

    # --------------------------------------------------------------------------------------- match execution
    lens = (3, 31, 32, 33, 64, 65)
    for off in list(range(1, 35)) + [63, 64, 65]:
        add(f"match_offset_{off}", ZFrame(seed=off).raw(h70).compressed(
            ("raw", noise(len(lens), 1200 + off), 1), [(1, OFF(off), m) for m in lens]))
    for d in (0, -1, 1):
        add(f"match_offset_equals_length{d:+d}".replace("+0", ""), ZFrame().raw(h70).compressed(
            ("raw", noise(len(lens), 1240 + d), 1), [(1, OFF(m + d), m) for m in lens]))
    add("match_chain_of_45", ZFrame().raw(h8).compressed(
        ("raw", noise(23, 1250), 1), [((i % 2), OFF(4 - i % 2), 4 + i % 4) for i in range(45)]))
    add("match_chain_of_45_rle_tables", ZFrame().raw(h8).compressed(
        ("raw", b"", 1), [(0, OFF(5), 4)] * 45, ll=RLE(0), of=RLE(3), ml=RLE(1)))
    add("match_source_straddles_completed_output", ZFrame().raw(h70).compressed(
        ("raw", noise(12, 1251), 1), [(5, OFF(50), 10), (0, OFF(12), 8), (3, OFF(40), 33), (0, OFF(35), 34),
                                      (4, OFF(70), 3), (0, OFF(5), 40)]))
    add("match_reads_literals_of_its_own_sequence", ZFrame().raw(h8).compressed(
        ("raw", noise(31, 1252), 1), [(8, OFF(4), 6), (20, OFF(20), 45), (3, OFF(1), 33)]))

    # ------------------------------------------------------------------------------------------ tail staging
    w5 = huf_chain(5, [0x65, 0x20, 0x74, 0x61, 0x6F, 0x6E])
    d = huf_data(w5, 500, 1260)
    for streams, sf in ((1, 0), (4, 1)):
        for pos in (0, 250, 500):
            add(f"huffman_{streams}_stream_block_with_one_match_at_{pos}",
                ZFrame().raw(h8).compressed(("huf", d, w5, streams, sf, "direct"), [(pos, OFF(5), 3)]))
        add(f"huffman_{streams}_stream_third_block", ZFrame().raw(h8).rle(0x20, 40).compressed(
            ("huf", d, w5, streams, sf, "direct"), [(17, OFF(45), 30), (400, 1, 3)]).raw(b"tail"))

    # --------------------------------------------------------------------------------------------- malformed
    ok = lambda: ZFrame().raw(h16).compressed(("raw", text[:20], 1), [(4, OFF(3), 5)])      # noqa: E731
    bad("bad_magic", ok(), "z_header", 64, magic=ZSTD_MAGIC ^ 0x100)
    bad("reserved_descriptor_bit", ok(), "z_header", 64, fhd_or=8)
    for did in (1, 2, 4):
        bad(f"dictionary_id_in_{did}_bytes", ZFrame(did=did).raw(h16), "z_header", 64, did_value=1 << (8 * did - 1))
    f = ZFrame(did=1, fcs=8).raw(h16)
    comp = f.finish()[0]
    assert f.header_len == 15
    for cut in range(1, 15):
        bad(f"header_cut_to_{cut}_bytes", comp, "z_header" if cut < 6 else "trunc", 64, cut=cut)
    f = ok()
    f.blocks.append((3, 5, b"12345"))
    bad("reserved_block_type", f, "z_block", 64)
    bad("raw_block_cut_short", ZFrame().raw(h16), "trunc", 64, cut=6 + 3 + 10)
    bad("rle_block_without_its_byte", ZFrame().raw(h16).rle(7, 5), "trunc", 64, cut=6 + 3 + 16 + 3)
    comp = ok().finish()[0]
    bad("compressed_block_cut_short", comp, "z_block", 64, cut=len(comp) - 2)
    bad("block_header_cut_short", comp, "trunc", 64, cut=6 + 3 + 16 + 2)
    bad("no_last_block", ok(), "trunc", 64, no_last=True)
    bad("compressed_block_larger_than_window", ZFrame(window=(0, 0)).compressed(("raw", noise(1022, 1300), 2), []),
        "z_block", 2048)
    bad("block_regenerates_more_than_window", ZFrame(window=(0, 0)).compressed(
        ("raw", text[:20], 1), [(10, OFF(1), 1015)]), "z_block", 1100)
    bad("block_regenerates_more_than_128_kib", ZFrame().raw(h16).compressed(
        ("rle", 0x11, ZBLOCK_MAX, 3), [(0, OFF(1), 3)]), "z_block", ZBLOCK_MAX + 32)
    # ---- literals
    bad("literals_regenerate_more_than_128_kib", ZFrame().compressed(("rle", 0x11, ZBLOCK_MAX + 1, 3), []),
        "z_lit", ZBLOCK_MAX + 8)
    bad("literals_raw_longer_than_block", ZFrame().compressed(("raw", text[:20], 1), [], size=15), "z_lit", 64)
    d = huf_data(w4, 100, 1310)
    bad("literals_compressed_size_past_block", ZFrame().compressed(
        ("huf", d, w4, 1, 0, "direct", {"csize_delta": 2}), []), "z_lit", 100)
    bad("literals_jump_table_larger_than_section", ZFrame().compressed(
        ("huf", d, w4, 4, 1, "direct", {"jump": [9, 9, 30]}), []), "z_lit", 100)
    bad("literals_4_streams_without_jump_table", ZFrame().compressed(
        ("huf", d, w4, 4, 1, "direct", {"body": lambda b: b[:5]}), []), "z_lit", 100)
    f = ZFrame().compressed(("raw", text[:20], 1), [])
    f.huf = huf_codes(w4)
    bad("treeless_literals_without_tree", f.compressed(("treeless", d, 1, 0), []), "z_huf", 120)
    tree = lambda ws: {"tree": huf_tree_direct(ws)}                                       # noqa: E731
    bad("huffman_weight_12", ZFrame().compressed(("huf", d, w4, 1, 0, "direct", tree([12, 1, 1])), []), "z_huf", 100)
    bad("huffman_weights_leave_no_power_of_two", ZFrame().compressed(
        ("huf", d, w4, 1, 0, "direct", tree([3, 1])), []), "z_huf", 100)
    bad("huffman_weights_sum_to_0", ZFrame().compressed(("huf", d, w4, 1, 0, "direct", tree([0, 0])), []),
        "z_huf", 100)
    bad("huffman_tree_cut_short", ZFrame().compressed(
        ("huf", b"", w4, 1, 0, "direct", {"tree": huf_tree_direct([1] * 127)[:20]}), []), "z_huf", 100)
    bad("huffman_stream_ends_with_zero_byte", ZFrame().compressed(
        ("huf", d, w4, 1, 0, "direct", {"body": lambda b: b[:-1] + b"\x00"}), []), "z_huf", 100)
    bad("huffman_1_of_4_streams_ends_with_zero_byte", ZFrame().compressed(
        ("huf", d, w4, 4, 1, "direct", {"body": lambda b: b[:-1] + b"\x00"}), []), "z_huf", 100)
    for streams, sf in ((1, 0), (4, 1)):
        bad(f"huffman_{streams}_stream_one_symbol_short", ZFrame().compressed(
            ("huf", d, w4, streams, sf, "direct", {"regen_delta": 1}), []), "z_huf", 101)
        bad(f"huffman_{streams}_stream_one_symbol_long", ZFrame().compressed(
            ("huf", d, w4, streams, sf, "direct", {"regen_delta": -1}), []), "z_huf", 100)
    wf = huf_chain(3, [0x30, 0x31, 0x33, 0x34])
    bad("huffman_weight_fse_accuracy_7", ZFrame().compressed(
        ("huf", huf_data(wf, 100, 1311), wf, 1, 0, "direct",
         {"tree": huf_tree_fse(wf[:-1], 6, log_field=2)}), []), "z_huf", 100)
    # ---- FSE descriptions
    a = [(2, OFF(5), 5), (1, OFF(13), 3)]

    def fse_bad(name, kind, desc, ends_block=False):
        """The sequences ``a`` behind the description ``desc`` of the table of ``kind`` (the other two predefined);
        ``ends_block``: the block ends with the description."""
        modes = {k: FSE(fse_ok[k], 5, desc) if k == kind else PRE for k in ZSTD_KINDS}
        f = ZFrame().raw(h70).compressed(("raw", text[:9], 1), a, tail=b"" if ends_block else None, **modes)
        bad(name, f, "z_fse", 100)

    fse_ok = {"ll": znorm(5, {0: 8, 2: 8}, 1), "of": znorm(5, {3: 8}, 4), "ml": znorm(5, {0: 8, 2: 8}, 1)}

    for kind in ZSTD_KINDS:
        mx, top = ZSTD_MAX_LOG[kind], ZSTD_MAX_SYM[kind]
        d = FseDesc(mx + 1)
        d.count(1 << mx).count(1 << mx)
        fse_bad(f"fse_{kind}_accuracy_{mx + 1}", kind, d.finish())
        # (a count can never overshoot the total: the field's largest value is what remains.  What a description
        # can do is run out of symbols before the total is reached.)
        d = FseDesc(6)
        for _ in range(top + 1):                           # one per symbol: 64 is not reached at the last symbol
            d.count(1)
        fse_bad(f"fse_{kind}_counts_stop_short_of_total", kind, d.finish() + b"\x00\x00")
        d = FseDesc(6)
        for _ in range(top + 1):
            d.count(1)
        d.count(63 - top)
        fse_bad(f"fse_{kind}_symbol_beyond_maximum", kind, d.finish())
        d = FseDesc(5).count(16).count(0).zeros(top).count(16)               # the run ends one past the last symbol
        fse_bad(f"fse_{kind}_zero_run_past_maximum", kind, d.finish())
        d = FseDesc(5).count(16).count(0).zeros(top + 30).count(16)
        fse_bad(f"fse_{kind}_long_zero_run_past_maximum", kind, d.finish())
        desc = fse_description(fse_ok[kind], 5)            # a good description without its last byte
        fse_bad(f"fse_{kind}_description_cut_short", kind, desc[:-1], ends_block=True)
        modes = {k: RLE(top + 1) if k == kind else RLE(2) for k in ZSTD_KINDS}
        bad(f"fse_{kind}_rle_symbol_{top + 1}", ZFrame().raw(h70).compressed(
            ("raw", text[:9], 1), [(2, OFF(5), 5)], tail=b"\x01", **modes), "z_fse", 100)
        modes = {k: REP if k == kind else PRE for k in ZSTD_KINDS}
        f = ZFrame().raw(h70)
        f.tabs = {k: (fse_table(*ZSTD_DEFAULTS[k]), ZSTD_DEFAULTS[k][1]) for k in ZSTD_KINDS}
        bad(f"fse_{kind}_repeat_without_table", f.compressed(("raw", text[:9], 1), a, **modes), "z_fse", 100)
    # ---- sequences
    s2 = [(4, OFF(3), 5), (18, OFF(9), 36)]
    bad("sequence_modes_reserved_bits", ZFrame().raw(h70).compressed(("raw", text[:30], 1), s2, reserved=1),
        "z_seq", 150)
    comp = ZFrame().raw(h70).compressed(("raw", text[:30], 1), s2).finish()[0]
    bad("sequence_stream_ends_with_zero_byte", comp[:-1] + b"\x00", "z_seq", 150)
    bad("sequence_stream_with_1_bit_left_over", ZFrame().raw(h70).compressed(("raw", text[:30], 1), s2, pad_low=1),
        "z_seq", 150)
    bad("sequence_stream_with_9_bits_left_over", ZFrame().raw(h70).compressed(("raw", text[:30], 1), s2, pad_low=9),
        "z_seq", 150)
    bad("sequence_stream_1_bit_short", ZFrame().raw(h70).compressed(("raw", text[:30], 1), s2, drop_low=1),
        "z_seq", 150)
    bad("sequence_section_missing", ZFrame().raw(h70).compressed(("raw", text[:30], 1), [], size=31), "trunc", 150)
    bad("sequence_count_cut_short", ZFrame().raw(h70).compressed(("raw", text[:30], 1), [], tail=b"",
                                                                 count_bytes=2, size=32), "trunc", 150)
    bad("sequence_modes_missing", ZFrame().raw(h70).compressed(("raw", text[:30], 1), s2, size=32), "trunc", 150)
    bad("literal_length_larger_than_literals_left", ZFrame().raw(h70).compressed(
        ("raw", text[:30], 1), [(4, OFF(3), 5), (27, OFF(9), 6)]), "overflow", 150)
    # ---- offsets
    bad("offset_one_past_output", ZFrame().raw(h16).compressed(("raw", text[:9], 1), [(4, OFF(21), 5)]),
        "offset", 64)
    bad("offset_one_past_output_first_block", ZFrame().compressed(("raw", text[:9], 1), [(4, OFF(5), 5)]),
        "offset", 64)
    bad("offset_0_from_repeat_offset_1_minus_1", ZFrame().raw(h16).compressed(("raw", text[:9], 1), [(0, 3, 5)]),
        "offset", 64)
    bad("initial_repeat_offset_4_at_position_2", ZFrame().compressed(("raw", text[:9], 1), [(2, 2, 5)]),
        "offset", 64)
    bad("initial_repeat_offset_8_at_position_7", ZFrame().compressed(("raw", text[:9], 1), [(7, 3, 5)]),
        "offset", 64)
    # offset code 31 with every extra bit set is offset 2^32 - 4: as a signed 32-bit number, -4.  The slot has 8
    # bytes after the write position, so a decoder that takes it for -4 still reads its own slot.
    bad("offset_code_31_extra_all_ones", ZFrame().compressed(
        ("raw", noise(30, 1320), 1), [(30, (1 << 32) - 1, 3)], of=RLE(31)), "offset", 30 + 3 + 8)
    bad("offset_code_31_extra_zero", ZFrame().compressed(
        ("raw", noise(30, 1321), 1), [(30, 1 << 31, 3)], of=RLE(31)), "offset", 30 + 3 + 8)
    bad("offset_code_30_extra_all_ones", ZFrame().compressed(
        ("raw", noise(30, 1322), 1), [(30, (1 << 31) - 1, 3)], of=RLE(30)), "offset", 30 + 3 + 8)
    # ---- capacity: well-formed frames, one byte more than the slot
    for name, f in (("raw_block", ZFrame().raw(h16).raw(h70)), ("rle_block", ZFrame().raw(h16).rle(3, 70)),
                    ("match", ZFrame().raw(h16).compressed(("raw", text[:9], 1), [(9, OFF(3), 40)])),
                    ("long_match", ZFrame().raw(h16).compressed(("raw", text[:9], 1), [(9, OFF(3), 400)]))):
        comp, out = f.finish()
        bad(f"capacity_one_short_in_{name}", comp, "overflow", len(out) - 1, True)
    for delta in (1, -1):
        for fcs, window in ((1, None), (2, (10, 0)), (4, (10, 0)), (8, None)):
            f = ZFrame(window=window, fcs=fcs).raw(ZH[:300] if fcs > 1 else h70).compressed(
                ("raw", text[:9], 1), [(9, OFF(3), 40)])
            bad(f"fcs_{fcs}_bytes_content{delta:+d}", f, "size", len(f.finish()[1]), fcs_delta=delta)
    return tuple(V), tuple(B), cov


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
