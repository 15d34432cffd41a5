"""A plain GROUP BY oracle over lists of Python values: no torch, no numpy, nothing from ``dxa.ops`` or
``dxa.engine``.  Every grouping / aggregation path of the engine is compared with this, never with another path.

Rules, each with its source:

* Keys.  NULL is a key value with a group of its own; ``""`` is not NULL.  Among double keys every NaN is one group
  and -0.0 groups with 0.0 (hash_groupby.hip ``norm_f64_bits`` / ``hash_f64_kernel``, window_ring.hip
  ``norm_f64_bits``).  The sign of an emitted zero key is not part of the contract (a path may emit its first row's
  sign or the normalised one), so :func:`key_token` maps NaN to a token and both zeros to 0.0.
* NULL arguments are ignored; a group without a non-NULL argument gives NULL, except COUNT, which gives 0.
* MIN / MAX of doubles follow ``java.lang.Double.compare``: -inf < … < -0.0 < 0.0 < … < +inf < NaN (hash_groupby.hip
  ``f64_ordered``, "as Spark orders it").  The sign of a zero result and NaN-ness are part of the result.
* SUM of doubles is an IEEE sum started at +0.0: any NaN → NaN, both infinities → NaN, one infinity → that infinity,
  otherwise ``math.fsum`` (the tests' finite doubles are multiples of 0.25 below 2**20, so any order is exact).
* SUM of integers wraps modulo 2**64 into signed 64 bits (Spark 2.4 without ANSI; the ``MA_ADD_U64`` accumulator).
* AVG is the double sum (integers converted to doubles first) divided by the count.
* MIN / MAX of integers and booleans are plain.
"""
import math
import struct

NAN = ("NaN",)            # the key token of every NaN
INT64_MIN = -2**63
INT64_MAX = 2**63 - 1


def key_token(v):
    if isinstance(v, float):
        if v != v:
            return NAN
        if v == 0.0:
            return 0.0
    return v


def key_tuple(vals):
    return tuple(key_token(v) for v in vals)


def double_order(x: float) -> int:
    """Position of a double in Double.compare's total order."""
    if x != x:
        return 0x7ff8000000000000
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b if b >= 0 else b ^ 0x7fffffffffffffff


def double_sum(xs) -> float:
    if any(x != x for x in xs):
        return math.nan
    pos = any(x == math.inf for x in xs)
    neg = any(x == -math.inf for x in xs)
    if pos and neg:
        return math.nan
    if pos or neg:
        return math.inf if pos else -math.inf
    return 0.0 + math.fsum(xs)


def wrap64(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _agg(func, vals):
    """One aggregate over the group's argument values (NULLs still inside); ``count_star`` gets the rows."""
    if func == "count_star":
        return len(vals)
    vals = [v for v in vals if v is not None]
    if func == "count":
        return len(vals)
    if not vals:
        return None
    is_f = isinstance(vals[0], float)
    if func == "sum":
        return double_sum(vals) if is_f else wrap64(sum(int(v) for v in vals))
    if func == "avg":
        return double_sum([float(v) for v in vals]) / len(vals)
    if func in ("min", "max"):
        pick = min if func == "min" else max
        return pick(vals, key=double_order) if is_f else pick(vals)
    raise ValueError(func)


def group_by(rows, key_pos, reqs):
    """``rows``: list of tuples; ``key_pos``: positions of the key columns; ``reqs``: [(alias, func, arg position or
    None)] with func in count_star | count | sum | min | max | avg  →  {key tuple: {alias: value}}, groups in order
    of first appearance."""
    groups = {}
    for r in rows:
        groups.setdefault(key_tuple(r[p] for p in key_pos), []).append(r)
    return {k: {alias: _agg(func, rs if arg is None else [r[arg] for r in rs]) for alias, func, arg in reqs}
            for k, rs in groups.items()}


def group_ids(rows, key_pos):
    """First-appearance numbering: (gid per row, first row per group)."""
    seen, gid, rep = {}, [], []
    for i, r in enumerate(rows):
        k = key_tuple(r[p] for p in key_pos)
        g = seen.get(k)
        if g is None:
            g = seen[k] = len(rep)
            rep.append(i)
        gid.append(g)
    return gid, rep


def same(a, b) -> bool:
    """Result equality: NULL is NULL, NaN is NaN, zeros compare with their sign, no tolerance."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) or isinstance(b, float):
        if not (isinstance(a, float) and isinstance(b, float)):
            return False
        if a != a or b != b:
            return a != a and b != b
        return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)
    return a == b
