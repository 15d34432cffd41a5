"""Device inflate / LZ4 / snappy / zstd decoders on hand-assembled streams (``tests/codec_vectors.py``).

The CPU tests prove every vector first: zlib, pyarrow (whose zstd codec is libzstd), an independent pure-Python LZ4
decoder and this project's host decoders must all expand a valid vector to the bytes the builder's own expansion
gives, and must all reject a malformed one.  The GPU tests then put all vectors of a codec into one block table,
shuffled (so the lane groups that share a wave, four of 16 lanes or two zstd frames of 32, take different paths) and
in order, and call the kernels' entry points directly.  Every output slot lies between 0xA5 guards: a decoder that
writes outside its slot, or past the bytes it reports, fails an assertion (``zstd.hip`` stages Huffman literals in
the tail of its slot, so it may write anywhere inside the capacity it is given, and nowhere else).
Any change to ``lz4.hip``, ``inflate.hip``, ``snappy.hip`` or ``zstd.hip`` must keep this file green.
"""
import random
import zlib
from typing import NamedTuple, Optional

import numpy as np
import pytest
import torch

from dxa.io import kafka as K
from dxa.ops import lz4
from tests import codec_vectors as CV

FILL = 0xA5
GUARD = 512                    # untouched bytes before and after every output slot
SRC_GUARD = 64                 # bytes after what a kernel may read behind a member
EXTRA_CAP = 37
# status classes the three kernels' enums share (truncated / offset or distance / overflow / size), inflate's block
# error, and inflate's code errors (10 + which check)
KLASS = {"trunc": lambda s: s == 1, "offset": lambda s: s == 2, "overflow": lambda s: s == 3,
         "size": lambda s: s == 4, "block": lambda s: s == 6, "code": lambda s: s >= 10,
         # zstd.hip's own classes: frame header, Huffman tree or stream, FSE table, sequence section, literals
         # section, block
         "z_header": lambda s: s == 5, "z_huf": lambda s: s == 6, "z_fse": lambda s: s == 7,
         "z_seq": lambda s: s == 8, "z_lit": lambda s: s == 9, "z_block": lambda s: s == 10}
COUNTS = {"inflate": (45, 21), "lz4": (1364, 16), "snappy": (91, 20), "zlib": 208, "zstd": (334, 98)}


# ======================================================================================================== CPU tests
def test_vector_counts():
    """A builder bug cannot silently empty a sweep: the number of vectors per codec is fixed."""
    iv, ib = CV.inflate_vectors()
    lv, lb, relaxed = CV.lz4_vectors()
    sv, sb = CV.snappy_vectors()
    zv, zb, _ = CV.zstd_vectors()
    got = {"inflate": (len(iv), len(ib)), "lz4": (len(lv), len(lb)), "snappy": (len(sv), len(sb)),
           "zlib": len(CV.zlib_streams()), "zstd": (len(zv), len(zb))}
    print("codec vectors (valid, malformed):", got)
    assert got == COUNTS
    shapes = len(CV.LZ4_LITERAL_SHAPES) + len(CV.LZ4_MATCH_SHAPES)
    assert sum(v.name.startswith("sweep_") for v in lv) == shapes * len(CV.LZ4_PREFIXES) - 1    # lit0 at P0
    assert sum(v.name.startswith("chain_") for v in lv) == len(CV.LZ4_CHAIN_SHAPES) * 67
    assert len(relaxed) == 3
    for vs in (iv, ib, lv, lb, sv, sb, CV.zlib_streams(), zv, zb):
        assert len({v.name for v in vs}) == len(vs)
    assert max(len(v.expected) for v in iv + lv + sv + CV.zlib_streams()) <= 71000
    assert max(len(v.expected) for v in zv) == (1 << 20) - 1            # offset code 19 with every extra bit set
    assert sum(len(v.expected) < 4096 for v in zv) > 0.8 * len(zv)


def test_noise_is_not_one_repeated_byte():
    """Match sources are cut from it: over a run of one byte every offset copies the same thing."""
    assert len(set(CV.noise(4096, 1))) == 256 and CV.noise(64, 1) != CV.noise(64, 2)
    assert CV.noise(64, 1)[:32] == CV.noise(32, 1)


def test_bit_writer_and_canonical_codes():
    """RFC 1951 3.2.6's fixed code, and 3.2.2's worked example (lengths 3,3,3,3,3,2,4,4)."""
    c = CV.canonical_codes(CV.FIXED_LL)
    assert (c[0], c[143], c[144], c[255], c[256], c[279], c[280], c[287]) == \
        (0b00110000, 0b10111111, 0b110010000, 0b111111111, 0, 0b0010111, 0b11000000, 0b11000111)
    assert CV.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]
    w = CV.BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    w.code(0b0010, 4)         # MSB first: the bits 0,0,1,0 follow the three header bits
    assert w.bitpos == 7 and w.getvalue() == bytes([0b0100_011])
    # the writer's shortest fixed block is zlib's: BFINAL, type 1, the 7-bit end-of-block code
    assert CV.Deflate().fixed([], final=True).finish()[0] == b"\x03\x00"
    assert CV.zlib_inflate(b"\x03\x00") == (b"", True)
    assert CV.lz4_ext(0) == b"\x00" and CV.lz4_ext(254) == b"\xfe" and CV.lz4_ext(255) == b"\xff\x00"
    assert CV.lz4_ext(255 + 255 + 3) == b"\xff\xff\x03"
    assert [len(CV.varint(n)) for n in (0, 127, 128, 16383, 16384)] == [1, 1, 2, 2, 3]


def test_inflate_vectors_decode_with_zlib():
    valid, _ = CV.inflate_vectors()
    for v in valid + CV.zlib_streams():
        assert CV.zlib_inflate(v.comp) == (v.expected, True), v.name


def test_inflate_malformed_vectors_rejected_by_zlib():
    _, malformed = CV.inflate_vectors()
    for b in malformed:
        assert b.expected is None and b.klass in KLASS
        if b.stream_ok:                                   # capacity cases: zlib yields a different length
            out, eof = CV.zlib_inflate(b.comp)
            assert eof and len(out) != b.cap, b.name
            assert len(out) - b.cap == (-1 if b.klass == "size" else 1), b.name
        elif b.klass == "trunc":                          # the stream ends before its end-of-block code
            out, eof = CV.zlib_inflate(b.comp)
            assert not eof and len(out) < b.cap, b.name
        else:
            with pytest.raises(zlib.error):
                CV.zlib_inflate(b.comp)


def test_lz4_vectors_decode_with_independent_and_host_decoders():
    valid, _, _ = CV.lz4_vectors()
    for v in valid:
        assert CV.py_lz4_block_decode(v.comp) == v.expected, v.name
        assert lz4.decompress_block(v.comp, len(v.expected)) == v.expected, v.name
        assert lz4.decompress_block(v.comp, len(v.expected) + EXTRA_CAP) == v.expected, v.name


def test_lz4_vectors_decode_with_pyarrow():
    """pyarrow's ``lz4_raw`` is the reference decoder, which also enforces the *encoder's* end-of-block rules (a
    last literal run of five bytes or more): it may reject the three vectors that end otherwise, and nothing else."""
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("lz4_raw")
    valid, _, relaxed = CV.lz4_vectors()
    for v in valid:
        try:
            got = codec.decompress(v.comp, decompressed_size=len(v.expected), asbytes=True)
        except OSError:
            assert v.name in relaxed, v.name
            continue
        assert got == v.expected, v.name


def test_lz4_malformed_vectors_rejected_by_host_decoder():
    _, malformed, _ = CV.lz4_vectors()
    for b in malformed:
        assert b.expected is None and b.klass in KLASS
        with pytest.raises(lz4.Lz4Error):
            lz4.decompress_block(b.comp, b.cap)
        if b.stream_ok:                                   # well-formed, one byte more than the capacity
            assert len(CV.py_lz4_block_decode(b.comp)) == b.cap + 1, b.name
            assert len(lz4.decompress_block(b.comp, b.cap + 1)) == b.cap + 1, b.name


def test_snappy_vectors_decode_with_host_decoder():
    valid, _ = CV.snappy_vectors()
    for v in valid:
        assert K.snappy_decompress(v.comp) == v.expected, v.name


def test_snappy_vectors_decode_with_pyarrow():
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("snappy")
    valid, _ = CV.snappy_vectors()
    for v in valid:
        assert codec.decompress(v.comp, decompressed_size=len(v.expected), asbytes=True) == v.expected, v.name


def test_snappy_malformed_vectors_rejected_by_host_decoder():
    _, malformed = CV.snappy_vectors()
    for b in malformed:
        assert b.expected is None and b.klass in KLASS
        if b.stream_ok:                                   # a consistent block given with the wrong capacity
            assert len(K.snappy_decompress(b.comp)) != b.cap, b.name
        else:
            with pytest.raises(K.KafkaError):
                K.snappy_decompress(b.comp)


def test_zstd_writers():
    """The checksum against XXH64's published value for the empty input (libzstd verifies it on every frame that has
    one), the shortest frame against the 9 bytes libzstd writes for no input, and what the writers covered."""
    assert CV.xxh64(b"") == 0xEF46DB3751D8E999
    assert CV.ZFrame(window=None, fcs=1).raw(b"").finish()[0] == bytes.fromhex("28b52ffd2000010000")
    assert CV.fse_description(CV.LL_DEF, 6)[0] & 15 == 1 and len(CV.fse_table(CV.ML_DEF, 6)) == 64
    # RFC 8878 3.1.1.3.2.1.1: the sequence count's three forms
    f = CV.ZFrame()
    assert f._sequences([], b"", {}) == b"\x00" and f._sequences([], b"", {}, count_bytes=2) == b"\x80\x00"
    _, _, cov = CV.zstd_vectors()
    assert cov["marker_bit"] == set(range(8)) and cov["seq_bytes"] >= set(range(1, 10))
    assert cov["rep_idx"] == {0, 1, 2, 3} and cov["huf_depth"] == set(range(1, 12))
    assert cov["zero_runs"] >= {0, 1, 2, 3, 4, 24, 30}
    assert {1, 6, 8, 13} <= cov["huf_stream_bytes"]
    for kind, top in (("ll", 9), ("of", 8), ("ml", 9)):
        for log in range(5, top + 1):
            assert {(kind, log, log), (kind, log, 0)} <= cov["cell_bits"], (kind, log)


def test_zstd_vectors_decode_with_libzstd_and_host_decoder():
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("zstd")
    valid, _, _ = CV.zstd_vectors()
    for v in valid:
        assert codec.decompress(v.comp, decompressed_size=len(v.expected), asbytes=True) == v.expected, v.name
        assert K.zstd_decompress(v.comp) == v.expected, v.name


def test_zstd_malformed_vectors_rejected_by_libzstd_and_host_decoder():
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("zstd")
    _, malformed, _ = CV.zstd_vectors()
    for b in malformed:
        assert b.expected is None and b.klass in KLASS
        if b.stream_ok:                                   # a well-formed frame of one byte more than the capacity
            assert len(codec.decompress(b.comp, decompressed_size=b.cap + 1, asbytes=True)) == b.cap + 1, b.name
            assert len(K.zstd_decompress(b.comp)) == b.cap + 1, b.name
        else:
            with pytest.raises(K.KafkaError):
                K.zstd_decompress(b.comp)
        with pytest.raises(OSError):                      # (pyarrow also refuses any size but the one it is given)
            codec.decompress(b.comp, decompressed_size=b.cap, asbytes=True)
        if not b.stream_ok:                               # ... so let it try the sizes around the capacity too
            for size in (b.cap + 1, max(b.cap - 1, 0), b.cap + 8, 1 << 18):
                with pytest.raises(OSError):
                    codec.decompress(b.comp, decompressed_size=size, asbytes=True)


def test_zstd_offset_code_31_vector_separates_the_signed_from_the_unsigned_check():
    """The index arithmetic of ``zstd.hip``'s match copy on the offset-code-31 vector.  Compared as a signed 32-bit
    number the offset 2^32 - 4 is -4 and passes ``offset > position``; the copy then reads three bytes 4 after the
    write position (C's ``c % -4`` is ``c`` for c < 4) and writes three at it, all inside the vector's own slot, and
    the frame ends with status 0.  So of all malformed vectors, this one alone tells the two checks apart, and a
    decoder with the signed check fails on its status, not on a guard."""
    _, malformed, _ = CV.zstd_vectors()
    by_name = {b.name: b for b in malformed}
    b = by_name["offset_code_31_extra_all_ones"]
    op, ml, off = 30, 3, (1 << 32) - 4                    # after the 30 literals; the vector's sequence
    signed = off - (1 << 32)
    assert signed == -4 and not signed > op and off > op  # the signed check passes it, the unsigned one does not
    src = [op - signed + c for c in range(ml)]            # c % -4 == c
    assert min(src) >= 0 and max(src) < b.cap and op + ml <= b.cap
    # every other malformed offset is below 2^31: both comparisons reject it
    assert b.comp[-8:-6] == bytes([0x10, 31])             # modes: the offset table is RLE, with symbol 31
    for name, off in (("offset_code_31_extra_zero", (1 << 31) - 3), ("offset_code_30_extra_all_ones", (1 << 31) - 4)):
        assert name in by_name and 30 < off < (1 << 31)


# ======================================================================================================== GPU tests
class Entry(NamedTuple):
    name: str
    comp: bytes
    cap: int
    expected: Optional[bytes]     # None: malformed
    klass: Optional[str]
    align: int                    # comp_off & 3
    stream_ok: bool = False


def _entries(valid, malformed, aligns, extra_cap=0):
    out = []
    for i, v in enumerate(valid):
        for a in (aligns if aligns else (i % 4,)):
            out.append(Entry(v.name, v.comp, len(v.expected) + extra_cap, v.expected, None, a))
    for i, b in enumerate(malformed):
        for a in (aligns if aligns else (i % 4,)):
            out.append(Entry(b.name, b.comp, b.cap, None, b.klass, a, b.stream_ok))
    return out


class Table:
    """Source and destination layout of a block table.  After each member come the bytes its kernel may read
    (``readable``) and a guard; every output slot has GUARD bytes of 0xA5 on both sides and starts at a different
    ``out_off & 15``."""

    def __init__(self, entries, readable, src_fill, gpu):
        src = bytearray([src_fill]) * 16
        self.entries = entries
        self.co, self.oo = [], []
        pos = 0
        for i, e in enumerate(entries):
            while len(src) % 4 != e.align:
                src.append(src_fill)
            self.co.append(len(src))
            src += e.comp
            src += bytes([src_fill]) * (readable + SRC_GUARD)
            pos = (pos + GUARD + 15) // 16 * 16 + i % 16
            self.oo.append(pos)
            pos += e.cap
        self.total = pos + GUARD
        n = len(entries)
        if n >= 64:
            assert {o & 15 for o in self.oo} == set(range(16)) and {c & 3 for c in self.co} == {0, 1, 2, 3}
        dev = lambda xs, dt: torch.tensor(xs, dtype=dt, device=gpu)                  # noqa: E731
        self.gpu = gpu
        self.n = n
        self.src = torch.frombuffer(src, dtype=torch.uint8).to(gpu)
        self.t_co = dev(self.co, torch.int64)
        self.t_cl = dev([len(e.comp) for e in entries], torch.int32)
        self.t_oo = dev(self.oo, torch.int64)
        self.t_cap = dev([e.cap for e in entries], torch.int64)
        self.status = torch.full((n,), -1, dtype=torch.int32, device=gpu)
        self.produced = torch.full((n,), -7, dtype=torch.int64, device=gpu)
        self.out = torch.full((self.total,), FILL, dtype=torch.uint8, device=gpu)

    def kind(self, k):
        self.t_kind = torch.full((self.n,), k, dtype=torch.uint8, device=self.gpu)
        return self.t_kind

    def results(self):
        torch.cuda.synchronize(self.gpu)     # every operand tensor is still held by self here
        return self.status.tolist(), self.produced.tolist(), self.out.cpu().numpy()


def _decode_into(gpu, entry_point, kind, entries, readable, src_fill):
    from dxa.ops import native as N
    t = Table(entries, readable, src_fill, gpu)
    rc = N.call(entry_point, N.ptr(t.src), N.ptr(t.t_co), N.ptr(t.t_cl), N.ptr(t.kind(kind)), N.ptr(t.t_oo),
                N.ptr(t.t_cap), t.n, N.ptr(t.out), N.ptr(t.produced), N.ptr(t.status), N.stream_handle(gpu))
    assert not rc, rc
    return t, t.results()


def _check_memory(t, out, whole_slot=False):
    """Only [slot, slot + true size) of a valid vector and [slot, slot + capacity) of a malformed one may change;
    ``whole_slot``: a valid vector's whole capacity too (a decoder that uses its slot as scratch space)."""
    frozen = np.ones(t.total, dtype=bool)
    for e, o in zip(t.entries, t.oo):
        frozen[o:o + (len(e.expected) if e.expected is not None and not whole_slot else e.cap)] = False
    touched = np.flatnonzero(frozen & (out != FILL))
    if touched.size:
        q = int(touched[0])
        i = int(np.searchsorted(np.asarray(t.oo), q, side="right")) - 1
        lo, hi = t.entries[max(i, 0)], t.entries[min(i + 1, t.n - 1)]
        raise AssertionError(f"{touched.size} bytes outside the writable output changed, first at {q} "
                             f"(slot of {lo.name!r} at {t.oo[max(i, 0)]} cap {lo.cap}; next slot {hi.name!r})")


def _check(t, status, produced, out, valid_status=0, check_produced=True, whole_slot=False):
    _check_memory(t, out, whole_slot)
    raw = out.tobytes()
    for i, (e, o) in enumerate(zip(t.entries, t.oo)):
        what = (e.name, e.align, i)
        if e.expected is None:
            assert status[i] != 0 and KLASS[e.klass](status[i]), (what, e.klass, status[i])
            continue
        assert status[i] == valid_status, (what, status[i])
        if produced is not None and check_produced:
            assert produced[i] == len(e.expected), (what, produced[i], len(e.expected))
        if valid_status == 0 or check_produced:
            got = raw[o:o + len(e.expected)]
            if got != e.expected:
                k = next(j for j in range(len(got)) if got[j] != e.expected[j])
                raise AssertionError((what, f"byte {k} of {len(got)}: {got[k]:#x} != {e.expected[k]:#x}"))


def _ordered(entries, order):
    entries = list(entries)
    if order == "shuffled":
        random.Random(20240521).shuffle(entries)
    return entries


def _pyarrow_blocks(codec):
    pa = pytest.importorskip("pyarrow")
    c = pa.Codec(codec)
    return tuple(CV.Vec(f"pyarrow_{codec}_{name}", c.compress(data, asbytes=True), data)
                 for name, data in CV.encoder_inputs())


# ---- inflate
def _inflate_run(gpu, entries):
    return _decode_into(gpu, "dxa_inflate_into", 2, entries, 8, 0)      # the gzip trailer: 8 readable bytes (zeros)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["shuffled", "original"])
def test_device_inflate_vectors(gpu, order):
    valid, malformed = CV.inflate_vectors()
    entries = _ordered(_entries(valid, malformed, (0, 1, 2, 3)) + _entries(CV.zlib_streams(), (), None), order)
    t, (status, produced, out) = _inflate_run(gpu, entries)
    _check(t, status, produced, out)


@pytest.mark.gpu
def test_device_inflate_reports_size_error_for_larger_capacity(gpu):
    valid, _ = CV.inflate_vectors()
    t, (status, produced, out) = _inflate_run(gpu, _entries(valid, (), None, EXTRA_CAP))
    _check(t, status, produced, out, valid_status=4)


# ---- LZ4
def _lz4_entries(order="original", extra=()):
    valid, malformed, _ = CV.lz4_vectors()
    return _ordered(_entries(valid + tuple(extra), malformed, (0, 1, 2, 3)), order)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["shuffled", "original"])
def test_device_lz4_decode_into_vectors(gpu, order):
    t, (status, produced, out) = _decode_into(gpu, "dxa_lz4_decode_into", 0, _lz4_entries(order), 16, 0xEE)
    _check(t, status, produced, out)


@pytest.mark.gpu
def test_device_lz4_decode_into_reports_true_size_for_larger_capacity(gpu):
    valid, _, _ = CV.lz4_vectors()
    t, (status, produced, out) = _decode_into(gpu, "dxa_lz4_decode_into", 0, _entries(valid, (), None, EXTRA_CAP),
                                              16, 0xEE)
    _check(t, status, produced, out)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["shuffled", "original"])
def test_device_lz4_decode_known_sizes(gpu, order):
    """``dxa_lz4_decode`` takes exact sizes: every vector, and a size one off either way for every 20th."""
    from dxa.ops import native as N
    valid, _, _ = CV.lz4_vectors()
    off_by_one = []
    for v in valid[::20]:
        off_by_one.append(CV.Bad(v.name + "_size_plus_1", v.comp, None, "size", len(v.expected) + 1, True))
        if len(v.expected):
            off_by_one.append(CV.Bad(v.name + "_size_minus_1", v.comp, None, "overflow", len(v.expected) - 1, True))
    assert len(off_by_one) > 100
    entries = _ordered(_lz4_entries() + _entries((), off_by_one, None), order)
    t = Table(entries, 16, 0xEE, gpu)
    rc = N.call("dxa_lz4_decode", N.ptr(t.src), N.ptr(t.t_co), N.ptr(t.t_cl), N.ptr(t.kind(0)), N.ptr(t.t_oo),
                N.ptr(t.t_cap), t.n, max(e.cap for e in entries), N.ptr(t.out), N.ptr(t.status),
                N.stream_handle(gpu))
    assert not rc, rc
    status, _, out = t.results()
    _check(t, status, None, out)


@pytest.mark.gpu
def test_device_lz4_block_sizes(gpu):
    """The size pass over the same table: the true size of every valid vector, a nonzero status for every malformed
    stream.  (It takes one capacity for the whole table, so the well-formed blocks of the capacity cases are sized
    like any other: one byte more than the capacity they come with.)"""
    from dxa.ops import native as N
    entries = _lz4_entries("shuffled")
    t = Table(entries, 16, 0xEE, gpu)
    rc = N.call("dxa_lz4_block_sizes", N.ptr(t.src), N.ptr(t.t_co), N.ptr(t.t_cl), N.ptr(t.kind(0)), t.n,
                max(e.cap for e in entries) + 1, N.ptr(t.produced), N.ptr(t.status), N.stream_handle(gpu))
    assert not rc, rc
    status, sizes, out = t.results()
    assert (out == FILL).all()
    for i, e in enumerate(entries):
        if e.expected is not None:
            assert (status[i], sizes[i]) == (0, len(e.expected)), (e.name, e.align, status[i], sizes[i])
        elif e.stream_ok:
            assert (status[i], sizes[i]) == (0, e.cap + 1), (e.name, e.align, status[i], sizes[i])
        else:
            assert KLASS[e.klass](status[i]) and sizes[i] == 0, (e.name, e.align, e.klass, status[i], sizes[i])


# ---- snappy
@pytest.mark.gpu
@pytest.mark.parametrize("order", ["shuffled", "original"])
def test_device_snappy_vectors(gpu, order):
    valid, malformed = CV.snappy_vectors()
    entries = _ordered(_entries(valid, malformed, (0, 1, 2, 3)), order)
    t, (status, produced, out) = _decode_into(gpu, "dxa_snappy_decode_into", 3, entries, 0, 0xEE)
    _check(t, status, produced, out)


@pytest.mark.gpu
def test_device_snappy_reports_size_error_for_larger_capacity(gpu):
    valid, _ = CV.snappy_vectors()
    t, (status, produced, out) = _decode_into(gpu, "dxa_snappy_decode_into", 3, _entries(valid, (), None, EXTRA_CAP),
                                              0, 0xEE)
    _check(t, status, produced, out, valid_status=4, check_produced=False)


# ---- blocks from pyarrow's encoders
@pytest.mark.gpu
def test_device_decodes_pyarrow_lz4_raw_blocks(gpu):
    blocks = _pyarrow_blocks("lz4_raw")
    entries = _entries(blocks, (), (0, 1, 2, 3))
    t, (status, produced, out) = _decode_into(gpu, "dxa_lz4_decode_into", 0, entries, 16, 0xEE)
    _check(t, status, produced, out)
    from dxa.ops import native as N
    rc = N.call("dxa_lz4_block_sizes", N.ptr(t.src), N.ptr(t.t_co), N.ptr(t.t_cl), N.ptr(t.t_kind), t.n,
                max(e.cap for e in entries), N.ptr(t.produced), N.ptr(t.status), N.stream_handle(gpu))
    assert not rc, rc
    status, sizes, _ = t.results()
    assert status == [0] * t.n and sizes == [e.cap for e in entries]


@pytest.mark.gpu
def test_device_decodes_pyarrow_snappy_blocks(gpu):
    entries = _entries(_pyarrow_blocks("snappy"), (), (0, 1, 2, 3))
    t, (status, produced, out) = _decode_into(gpu, "dxa_snappy_decode_into", 3, entries, 0, 0xEE)
    _check(t, status, produced, out)


# ---- zstd
def _zstd_entries(valid, malformed, extra_cap=0):
    return _entries(valid, malformed, (0, 1, 2, 3), extra_cap)


def _zstd_run(gpu, entries):
    return _decode_into(gpu, "dxa_zstd_decode_into", 4, entries, 0, 0xEE)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["shuffled", "original"])
def test_device_zstd_vectors(gpu, order):
    valid, malformed, _ = CV.zstd_vectors()
    t, (status, produced, out) = _zstd_run(gpu, _ordered(_zstd_entries(valid, malformed), order))
    _check(t, status, produced, out, whole_slot=True)


@pytest.mark.gpu
def test_device_zstd_reports_true_size_for_larger_capacity(gpu):
    """The Kafka case: a capacity slot larger than the frame's content, with or without a content size in the
    header."""
    valid, _, _ = CV.zstd_vectors()
    t, (status, produced, out) = _zstd_run(gpu, _ordered(_zstd_entries(valid, (), EXTRA_CAP), "shuffled"))
    _check(t, status, produced, out, whole_slot=True)


@pytest.mark.gpu
def test_device_decodes_pyarrow_zstd_frames(gpu):
    t, (status, produced, out) = _zstd_run(gpu, _entries(_pyarrow_blocks("zstd"), (), (0, 1, 2, 3)))
    _check(t, status, produced, out, whole_slot=True)
