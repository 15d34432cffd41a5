"""Decimal texts at and near the rounding boundaries of doubles, for the tests of decimal → double conversion
(tests/test_number_rounding.py).  Fixed seed; positive texts only (the tests add signs); every text is a valid JSON
number.  The only oracle is ``float(Decimal(text))`` compared as a 64-bit pattern: CPython's conversion is correctly
rounded and shares nothing with the project.

``cases()`` returns ``(family, text)`` pairs.  The builders below also keep what the self-test needs: the exact
midpoint a text was made from, and for ``layouts`` which texts denote one value.
"""
import random
import struct
from decimal import Decimal
from fractions import Fraction
from functools import lru_cache

SEED = 20240607
ND = (17, 19, 20, 25, 30, 34, 38, 45)
DBL_MAX = 1.7976931348623157e308


def f2b(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def b2f(b: int) -> float:
    return struct.unpack("<d", struct.pack("<q", b))[0]


@lru_cache(maxsize=None)
def oracle_bits(text: str) -> int:
    return f2b(float(Decimal(text)))


def midpoint(bits: int) -> Fraction:
    """Exact midpoint of the finite double with this bit pattern and its successor (2^1024 after DBL_MAX)."""
    lo = Fraction(b2f(bits))
    hi = Fraction(2) ** 1024 if bits == f2b(DBL_MAX) else Fraction(b2f(bits + 1))
    return (lo + hi) / 2


def exact_digits(fr: Fraction):
    """A dyadic rational as (digit string without trailing zeros, exponent of its last digit)."""
    den = fr.denominator
    k = den.bit_length() - 1
    assert den == 1 << k and fr > 0
    n, e = fr.numerator * 5 ** k, -k
    while n % 10 == 0:
        n //= 10
        e += 1
    return str(n), e


def truncated_digits(fr: Fraction, nd: int):
    """The first nd significant digits of fr > 0 (truncated), as (digit string, exponent of its last digit)."""
    e = len(str(fr.numerator)) - len(str(fr.denominator)) - nd          # within 1 of the right exponent
    while True:
        n = fr / Fraction(10) ** e
        n = n.numerator // n.denominator
        if len(str(n)) == nd:
            return str(n), e
        e += 1 if len(str(n)) > nd else -1


def value_of(text: str) -> Fraction:
    return Fraction(Decimal(text))


def scan(text: str):
    """(head, e10, tail, nt, sticky) of a text as the kernels' digit scanners deliver them: the first 19 significant
    digits, the decimal exponent of the last of them, the next nt ≤ 19 digits, and whether a non-zero digit follows."""
    mant, _, ex = text.lower().partition("e")
    head = tail = nd = nt = e10 = 0
    sticky = frac = False
    for ch in mant:
        if ch == ".":
            frac = True
            continue
        d = int(ch)
        if nd < 19:
            head = head * 10 + d
            nd += head != 0
            e10 -= frac
        else:
            e10 += not frac
            if nt < 19:
                tail, nt = tail * 10 + d, nt + 1
            else:
                sticky |= d != 0
    return head, e10 + (int(ex) if ex else 0), tail, nt, sticky


# ---------------------------------------------------------------------------------------------------------------
# layouts of (digits, exponent of the last digit): all denote int(digits) × 10^e
# ---------------------------------------------------------------------------------------------------------------
def _exp(e: int, sign: str = "") -> str:
    return "" if e == 0 and not sign else "e" + (sign if e >= 0 else "") + str(e)


def sci(ds: str, e: int) -> str:
    return ds[0] + ("." + ds[1:] if len(ds) > 1 else "") + "e" + str(e + len(ds) - 1)


def with_int_digits(ds: str, e: int, k: int) -> str:
    """k integer digits, the rest after the point, the exponent making up for it."""
    if len(ds) <= k:
        return ds + "0" * (k - len(ds)) + _exp(e - (k - len(ds)))
    return ds[:k] + "." + ds[k:] + _exp(e + len(ds) - k)


def leading_zeros(ds: str, e: int, z: int) -> str:
    return "0." + "0" * z + ds + _exp(e + len(ds) + z)


def trailing_zeros(ds: str, e: int, z: int) -> str:
    return ds + "0" * z + _exp(e - z)


def digits_then_exp(ds: str, e: int) -> str:
    return ds + "e" + str(e)


def small_fraction_exp(ds: str, e: int) -> str:
    return "0.000" + ds + "e+" + str(e + len(ds) + 3) if e + len(ds) + 3 >= 0 else "0.000" + ds + "e" + str(
        e + len(ds) + 3)


def plain(ds: str, e: int) -> str:
    """Positional, no exponent."""
    if e >= 0:
        return ds + "0" * e
    if -e < len(ds):
        return ds[:e] + "." + ds[e:]
    return "0." + "0" * (-e - len(ds)) + ds


# ---------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------
def _subnormal_bits(rnd, n):
    """n subnormal bit patterns of every width in turn."""
    return [rnd.randrange(1, 1 << (1 + i % 52)) for i in range(n)]


def _normal_bits(rnd, n):
    out = []
    while len(out) < n:
        b = rnd.getrandbits(63)
        if 0 < (b >> 52) < 0x7FF:
            out.append(b)
    return out


@lru_cache(maxsize=None)
def near_ties():
    """(text, midpoint, nd, side): side −1 for the truncated midpoint (below it, or on it when the expansion ends
    early), +1 for the last digit raised by one (above it)."""
    rnd = random.Random(SEED + 1)
    edge = 1 << 52                                       # bit pattern of 2^-1022
    classes = [_normal_bits(rnd, 150), _subnormal_bits(rnd, 156), list(range(edge - 10, edge + 10))]
    out = []
    for cls in classes:
        for bits in cls:
            mid = midpoint(bits)
            for nd in ND:
                ds, e = truncated_digits(mid, nd)
                out.append((sci(ds, e), mid, nd, -1))
                out.append((sci(str(int(ds) + 1), e), mid, nd, +1))
    # odd integers of 55 … 64 bits: one away from the midpoint of their neighbours (a multiple of two that is not
    # one of four, and so on): 17 … 20 digit texts a quarter of a gap or less from a tie
    for nbits in range(55, 65):
        for _ in range(12):
            gap = 1 << (nbits - 53)
            m = rnd.randrange(1 << 52, 1 << 53) * gap + gap // 2          # a midpoint
            for side in (-1, +1):
                n = m + side
                out.append((str(n), Fraction(m), len(str(n)), side))
    return out


@lru_cache(maxsize=None)
def exact_ties():
    """(text, midpoint) with the midpoint written out completely; (short, long): up to 38 digits, 39 … 60."""
    rnd = random.Random(SEED + 2)
    short, long_ = [], []

    def odd54():
        return 2 * rnd.randrange(1 << 52, 1 << 53) + 1                     # 2m + 1 in [2^53, 2^54)

    for j in range(0, 11):                                                 # integers of 16 … 20 digits
        for _ in range(6):
            n = odd54() << j
            short.append((str(n), Fraction(n)))
    for j in (1, 2, 3):                                                    # x.5, x.25 … x.875: 17 … 19 digits
        for _ in range(12):
            fr = Fraction(odd54(), 1 << j)
            ds, e = exact_digits(fr)
            assert 16 <= len(ds) <= 19
            short.append((plain(ds, e), fr))
    short.append(("1479079736107336.625", Fraction(1479079736107336625, 1000)))
    short.append(("7.878157860768404483795166015625e9", value_of("7.878157860768404483795166015625e9")))
    for j in list(range(4, 31, 2)) + list(range(-70, -11, 4)):             # up to 38 digits, both directions
        for _ in range(3):
            fr = Fraction(odd54()) / Fraction(2) ** j
            ds, e = exact_digits(fr)
            if len(ds) <= 38:
                short.append((sci(ds, e) if rnd.random() < 0.5 else plain(ds, e), fr))
    for j in list(range(33, 63, 2)) + list(range(-145, -74, 5)):           # 39 … 60 digits
        for _ in range(5):
            fr = Fraction(odd54()) / Fraction(2) ** j
            ds, e = exact_digits(fr)
            if 39 <= len(ds) <= 60:
                long_.append((sci(ds, e) if rnd.random() < 0.5 else plain(ds, e), fr))
    return short, long_


@lru_cache(maxsize=None)
def tie_sticky():
    """(text, midpoint, side): a tie, zeros out to 40 / 45 / 60 digits, then a 1 (above); the tie with its last digit
    lowered by one, then nines out to that many digits (below)."""
    out = []
    short, _ = exact_ties()
    for text, fr in short:
        ds, e = exact_digits(fr)
        integer = "." not in text and "e" not in text
        for total in (40, 45, 60):
            up = ds + "0" * (total - len(ds)) + "1"
            dn = str(int(ds) - 1).rjust(len(ds), "0") + "9" * (total - len(ds))
            for s, side in ((up, +1), (dn, -1)):
                ee = e - (len(s) - len(ds))
                out.append((plain(s, ee) if integer else sci(s, ee), fr, side))
    return out


@lru_cache(maxsize=None)
def shortest():
    from dxa.ops.serialize import java_double
    rnd = random.Random(SEED + 3)
    xs = [b2f(b) for b in _subnormal_bits(rnd, 5000)]
    xs += [b2f(b) for b in _normal_bits(rnd, 5000)]
    out = []
    for x in xs:
        out += [repr(x), java_double(x)]
    for k in range(-1074, 1024):
        x = 2.0 ** k
        out += [repr(x), java_double(x)]
    out += ["1e%d" % k for k in range(-323, 309)]
    return out


@lru_cache(maxsize=None)
def limits():
    out = ["1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308",
           "7.4109846876186981626485318930233205854759e-324", "2.4703282292062328e-324", "2.4703282292062327e-324",
           "2.2250738585072011e-308", "2.2250738585072012e-308", "2.2250738585072014e-308", "4.9e-324", "5e-324",
           "2.4e-324", "2.5e-324", "1e-324", "1e309", "1.8e308", "0.0", "0e0", "0.000e-400", "0e400"]
    top = midpoint(f2b(DBL_MAX))                          # DBL_MAX + half an ulp: rounds to infinity
    ds, e = exact_digits(top)
    out += [plain(ds, e), sci(ds, e)]
    for nd in (17, 19, 20, 30, 38, 45):
        t, te = truncated_digits(top, nd)
        out += [sci(t, te), sci(str(int(t) + 1), te)]
    half = Fraction(1, 2 ** 1075)                         # half of the least subnormal: a tie between 0 and 5e-324
    ds, e = exact_digits(half)
    out += [sci(ds, e), sci(str(int(ds) - 1), e), sci(str(int(ds) + 1), e), sci(ds + "0" * 30 + "1", e - 31)]
    for nd in (17, 19, 20, 30, 38, 45):
        t, te = truncated_digits(half, nd)
        out += [sci(t, te), sci(str(int(t) + 1), te)]
    # a 19-digit head whose exponent lies on either side of the table's ends (−348, 308): results 0, subnormals,
    # DBL_MAX and infinity
    for head in ("1000000000000000000", "2470328229206232721", "4940656458412465442", "9999999999999999999",
                 "1797693134862315708", "1797693134862315807", "1797693134862315900"):
        for e in (-350, -349, -348, -347, -343, -342, -341, -340, -330, 288, 289, 290, 291, 300, 307, 308, 309, 310):
            out.append(digits_then_exp(head, e))
            out.append(digits_then_exp(head + "5", e - 1))               # one digit in the tail
    return out


@lru_cache(maxsize=None)
def layouts():
    """Groups of texts of one value each: 300 cases of the other families in every layout."""
    rnd = random.Random(SEED + 4)
    short, long_ = exact_ties()
    pool = ([t for t, *_ in near_ties()] + [t for t, _ in short + long_] + [t for t, *_ in tie_sticky()]
            + shortest()[:20000:7] + limits())
    groups = []
    for i, text in enumerate(rnd.sample(pool, 300)):
        d = Decimal(text)
        if d == 0:
            continue
        _, dig, e = d.as_tuple()
        ds = "".join(map(str, dig)).lstrip("0")
        g = [text, sci(ds, e), digits_then_exp(ds, e), small_fraction_exp(ds, e)]
        # k integer digits: with 11 … 18 the 19-digit boundary falls at each of the eight places of a chunk of
        # the fraction's digit run, and the run lengths take every residue
        for k in {1 + i % 25, 11 + i % 8, 19 + i % 7, rnd.randint(1, 25)}:
            g.append(with_int_digits(ds, e, k))
        z = -(e + len(ds))
        for zz in {z if 0 <= z <= 340 else rnd.randint(0, 340), rnd.randint(0, 340), i % 9}:
            g.append(leading_zeros(ds, e, zz))
        for zz in {e if 0 <= e <= 300 else rnd.randint(0, 300), rnd.randint(1, 300), 1 + i % 8}:
            g.append(trailing_zeros(ds, e, zz))
        groups.append(g)
    return groups


@lru_cache(maxsize=None)
def cases():
    short, long_ = exact_ties()
    out = [("near-tie", t) for t, *_ in near_ties()]
    out += [("exact-tie", t) for t, _ in short + long_]
    out += [("tie+sticky", t) for t, *_ in tie_sticky()]
    out += [("shortest", t) for t in shortest()]
    out += [("limits", t) for t in limits()]
    out += [("layouts", t) for g in layouts() for t in g]
    assert len(out) < 60000 and all(len(t) < 790 for _, t in out)         # records stay under 800 bytes
    return out
