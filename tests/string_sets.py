"""The strings every MIN / MAX-over-strings test uses (tests/test_str_minmax.py, tests/test_window_dense_strings.py):
the lengths around the 8-byte compare step and the ring's 48-byte line, pairs that first differ at bytes 7, 8 and 9, a
string against itself with a trailing NUL, and bytes ≥ 0x80, which must sort above ASCII.  All are at most 48 bytes."""

_BASE = "mmmmmmmmmmmm"


def _differ_at(k):
    return _BASE[:k] + "a" + _BASE[k + 1:], _BASE[:k] + "z" + _BASE[k + 1:]


LENGTHS = ["", "q", "q" * 7, "q" * 8, "q" * 9, "q" * 16, "q" * 47, "q" * 48]
PAIRS = [s for k in (7, 8, 9) for s in _differ_at(k)]
PREFIX = ["ab", "ab\x00"]
NON_ASCII = ["é", "中", "\U0001F600", "zz"]
STRINGS = LENGTHS + PAIRS + PREFIX + NON_ASCII
assert all(len(s.encode()) <= 48 for s in STRINGS)


def draw(rng, n, null_rate=0.1):
    """``n`` values from ``STRINGS`` (uniform), a ``null_rate`` share of them None."""
    picks = rng.integers(0, len(STRINGS), n)
    nulls = rng.random(n) < null_rate
    return [None if z else STRINGS[int(i)] for i, z in zip(picks, nulls)]
