"""Exact decimal SUM / AVG / MIN / MAX over sliding windows from the dense ring (window_dense.py ``plan_layout`` /
``DenseWindow.accumulate``, window_ring.hip win_dec_kernel / win_combine_kernel's low-key branch / win_emit_kernel's
decimal kinds).  The oracle is the CPU evaluator over the materialised window (``decimal.aggregate``: limb
scatter-adds and a Python ``decimal`` division per group, no GPU code and no merge in it).

Decimal results compare exactly, in three ways: equal ``Decimal`` values, equal ``str()`` (so the scale and the
trailing zeros agree) and equal column dtype strings.  No tolerance is involved: the ring's sums are integer adds,
independent of arrival order.  Only the variance / moment families over a decimal argument are doubles (the
argument goes through ``decimal.to_double``, as in the paned path) and compare with the tolerances of
tests/test_window_dense_comoments.py: ``rel=1e-9, abs=1e-12``, the dimensionless ones (corr, skewness) ``abs=1e-9``.

AVG ties: at scale s + 4 the quotient of a group of 32 rows is sum · 312.5, an exact half for every odd unscaled sum;
of 64 rows it is sum · 156.25, an exact half when the sum is 2 mod 4 (an odd sum ends in .25 or .75, the rounding
next to a tie).  The tie stream has groups of both sizes with odd sums of both signs and, for 64 rows, sums that
are 2 mod 4 as well."""
import decimal as pd

import pytest
import torch

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from dxa.engine.expr import EvalContext
from tests.window_dense_support import (S, Comparison, aggs_of, as_partitioned_world_of_one, churn_stream,
                                        dense_states, layout_of, new_store, only_state, run_stream, set_caps,
                                        small_stream, stable_stream, steady_state_launches, two_rows_per_id_stream)

REL, ABS = 1e-9, 1e-12
DIMLESS_ABS = 1e-9
DIMLESS = ("cr", "sk")
N18 = "CAST(temp AS DECIMAL(18,2))"
WIDE = "temp * 1.8 + 32"
Q_ALL = (f"SELECT deviceId, COUNT(*) AS c, SUM({N18}) AS sn, AVG({N18}) AS an, MIN({N18}) AS mnn, MAX({N18}) AS mxn, "
         f"SUM({WIDE}) AS sw, AVG({WIDE}) AS aw, MIN({WIDE}) AS mnw, MAX({WIDE}) AS mxw, AVG(hum) AS ah, "
         "COUNT(DISTINCT kind) AS dk FROM W GROUP BY deviceId")
Q_FAM = (f"SELECT deviceId, COUNT({WIDE}) AS n, count_if(temp * 1.8 > 50) AS ci, STDDEV({WIDE}) AS sd, "
         f"VAR_POP({N18}) AS vp, corr(temp * 1.8, hum) AS cr, skewness({N18}) AS sk, covar_pop({N18}, hum) AS cp "
         "FROM W GROUP BY deviceId")
B18 = "CAST(big AS DECIMAL(18,0))"
W28 = "CAST(wtxt AS DECIMAL(28,3))"
Q_CARRY = (f"SELECT deviceId, COUNT(*) AS c, SUM({B18}) AS sb, AVG({B18}) AS ab, MIN({B18}) AS mnb, MAX({B18}) AS mxb, "
           f"SUM({W28}) AS sw, AVG({W28}) AS aw, MIN({W28}) AS mnw, MAX({W28}) AS mxw FROM W GROUP BY deviceId")
N0 = "CAST(temp AS DECIMAL(18,0))"              # unscaled value: temp
W15 = "temp * 1.5"                              # decimal(23,1), two lanes; unscaled value: 15 · temp
Q_TIES = (f"SELECT deviceId, COUNT(*) AS c, COUNT({N0}) AS n, SUM({N0}) AS s, AVG({N0}) AS a, SUM({W15}) AS sw, "
          f"AVG({W15}) AS aw FROM W GROUP BY deviceId")
Q_SMALL = (f"SELECT deviceId, COUNT(*) AS c, SUM({N18}) AS sn, AVG({WIDE}) AS aw, MIN({WIDE}) AS mnw, "
           f"MAX({WIDE}) AS mxw FROM W GROUP BY deviceId")
Q_MOD = (f"SELECT deviceId % 3 AS m, COUNT(*) AS c, SUM({WIDE}) AS sw, AVG({N18}) AS an, MAX({WIDE}) AS mxw, "
         f"MIN({WIDE}) AS mnw FROM W GROUP BY deviceId % 3")
Q_P30 = "SELECT deviceId, COUNT(*) AS c, SUM(CAST(temp AS DECIMAL(30,2))) AS s FROM W GROUP BY deviceId"
Q_INT = ("SELECT deviceId, COUNT(*) AS c, SUM(temp) AS s, MIN(temp) AS mn, MAX(temp) AS mx, AVG(temp) AS av "
         "FROM W GROUP BY deviceId")
TYPED = Comparison("tolerant", rel=REL, abs_=ABS, dimless=DIMLESS, dimless_abs=DIMLESS_ABS, types=True)


def batch(rng, t_us, ids, spread=S - 1, temp=None, temp_valid=None, big=None, wide=None):
    """A batch with given device ids; event times within ``spread`` before the batch time.  ``temp`` is a long in
    [-40, 120) with NULLs, ``hum`` a double multiple of 0.25, ``big`` a long (default: near ±(10^18 − 1)) and
    ``wtxt`` the text of a decimal at scale 3 whose unscaled value is ``wide`` (default: near ±10^27)."""
    import numpy as np
    n = len(ids)
    ts = torch.tensor([t_us - int(rng.integers(0, spread)) for _ in range(n)], dtype=torch.int64)
    tv = rng.integers(-40, 120, n) if temp is None else np.asarray(temp, dtype=np.int64)
    tvalid = rng.random(n) > 0.1 if temp_valid is None else np.asarray(temp_valid)
    hv = rng.integers(0, 256, n) * 0.25
    if big is None:
        big = [int(s) * (10 ** 18 - 1 - int(k)) for s, k in zip(rng.choice([-1, 1], n), rng.integers(0, 1000, n))]
    if wide is None:
        wide = [int(s) * (10 ** 27 - int(k)) for s, k in zip(rng.choice([-1, 1], n), rng.integers(0, 10 ** 9, n))]
    kinds = strings_from_pylist([["a", "b", "c"][int(i) % 3] for i in rng.integers(0, 3, n)], "cpu")
    wtxt = strings_from_pylist([wide_text(int(v)) for v in wide], "cpu")
    return Table(["ts", "deviceId", "kind", "temp", "hum", "big", "wtxt"],
                 [PrimColumn("timestamp", ts), PrimColumn("long", torch.tensor(ids, dtype=torch.int64)), kinds,
                  PrimColumn("long", torch.tensor(tv, dtype=torch.int64), torch.tensor(tvalid)),
                  PrimColumn("double", torch.tensor(hv, dtype=torch.float64)),
                  PrimColumn("long", torch.tensor([int(v) for v in big], dtype=torch.int64)), wtxt], n, "cpu")


def wide_text(u):
    """The text of the decimal with unscaled value ``u`` at scale 3."""
    return ("-" if u < 0 else "") + f"{abs(u) // 1000}.{abs(u) % 1000:03d}"


# ---- the streams of the edge cases ----------------------------------------------------------------------------------
HI = 1 << 64
HALF = 1 << 63


def carry_stream(nb):
    """Per batch: 60 rows over ids 0-5 with ``big`` near ±(10^18 − 1) and wide values near ±10^27, signs mixed inside
    every group (the low limb sums carry, the high one counts the negatives); 6 rows of id 100 whose values are all
    negative; and the two-lane MIN / MAX cases, whose candidates move from pane to pane:
      id 200: hi word 5 in every row, lo on both sides of 2^63;
      id 201: hi word -3 in every row (negative values), lo on both sides of 2^63;
      id 202: in even batches hi word 5 with a small lo, in odd batches hi word 4 with lo near 2^64 — the maximum is
              the small lo under the larger hi, the minimum the large lo under the smaller hi."""
    import numpy as np
    rng = np.random.default_rng(47)
    out = []
    for b in range(nb):
        ids = np.concatenate([rng.integers(0, 6, 60), [100] * 6, [200] * 4, [201] * 4, [202] * 2])
        n = len(ids)
        big = [int(s) * (10 ** 18 - 1 - int(k)) for s, k in zip(rng.choice([-1, 1], n), rng.integers(0, 1000, n))]
        wide = [int(s) * (10 ** 27 - int(k)) for s, k in zip(rng.choice([-1, 1], n), rng.integers(0, 10 ** 9, n))]
        for i in range(60, 66):
            big[i], wide[i] = -abs(big[i]), -abs(wide[i])
        los = [HALF + (b * 37) % 11 - 5, HALF - 1 - b, (b * 7919) % 1000, HI - 1 - (b * 31) % 17]
        for j, lo in enumerate(los):
            wide[66 + j] = 5 * HI + lo
            wide[70 + j] = -3 * HI + lo
        wide[74] = 5 * HI + 10 + b if b % 2 == 0 else 4 * HI + (HI - 1 - b)
        wide[75] = 5 * HI + 20 + b if b % 2 == 0 else 4 * HI + (HI - 40 - b)
        out.append(((100 + b) * S, batch(rng, (100 + b) * S, ids, temp_valid=[True] * n, big=big, wide=wide), ids))
    return out


def ties_stream(nb):
    """Per batch: 40 rows over ids 0-3; one row of an id seen in that batch alone; 5 rows of ids 9000-9004 whose
    ``temp`` is always NULL.  In batches 4-7 also the tie groups, a quarter of their rows in each of the four panes
    (ids 32xx have 32 rows, ids 64xx have 64): 3201 / 6401 an odd positive sum of ``temp``, 3202 / 6402 the same
    values negated, 6403 / 6404 sums that are 2 mod 4, positive and negative."""
    import numpy as np
    rng = np.random.default_rng(53)
    tie = {}
    for gid, rows, unit, odd in ((3201, 32, 2, 1), (6401, 64, 2, 1), (6403, 64, 4, 2)):
        vals = [unit * int(v) for v in rng.integers(1, 25, rows)]
        vals[5] += odd
        tie[gid] = vals
        tie[gid + 1] = [-v for v in vals]
    out = []
    for b in range(nb):
        ids = list(rng.integers(0, 4, 40)) + [2000 + b] + list(range(9000, 9005))
        temp = list(rng.integers(-40, 120, 46))
        valid = [True] * 41 + [False] * 5
        if 4 <= b < 8:
            for gid, vals in tie.items():
                q = len(vals) // 4
                ids += [gid] * q
                temp += vals[(b - 4) * q:(b - 3) * q]
                valid += [True] * q
        T = (100 + b) * S
        out.append((T, batch(rng, T - S // 4, np.asarray(ids), S // 2, temp=temp, temp_valid=valid), ids))
    return out


def tie_checker(seen):
    def each(b, q, rows, view, table):
        if q != Q_TIES:
            return
        for r in rows:
            i = r["deviceId"]
            if i >= 9000:
                assert r["c"] > 0 and r["n"] == 0 and all(r[k] is None for k in ("s", "a", "sw", "aw")), r
                seen["null"] += 1
            elif 2000 <= i < 3000:
                assert r["c"] == 1
                if r["n"] == 1:
                    assert r["a"] == r["s"] and str(r["a"]) == str(r["s"]) + ".0000" and r["aw"] == r["sw"], r
                    seen["one"] += 1
            elif 3200 <= i < 7000 and r["c"] == (32 if i < 6400 else 64):
                # the whole group is in the window: the quotient at scale s + 4 is an exact half (ids 6401 / 6402: a
                # quarter next to it), and the result is the one rounded away from zero — for the narrow argument
                # (unscaled sum Σ temp) and for the two-lane one (15 · Σ temp: odd, or 2 mod 4, with it)
                for total, avg, scale in ((r["s"], r["a"], 0), (r["sw"], r["aw"], 1)):
                    u = int(total.scaleb(scale))
                    exact = pd.Decimal(u) * 10000 / r["c"]
                    frac = abs(exact) % 1
                    assert frac == (pd.Decimal("0.5") if i < 6400 or i >= 6403 else frac) and frac in (
                        pd.Decimal("0.25"), pd.Decimal("0.5"), pd.Decimal("0.75")), (r, exact)
                    want = int(abs(exact) + pd.Decimal("0.5")) * (1 if u > 0 else -1)
                    assert int(avg.scaleb(scale + 4)) == want, (r, exact)
                seen["tie"].add(i)
    return each


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_layout_of_the_decimal_aggregates():
    """The three limb sums of a decimal SUM / AVG argument sit in ``MA_ADD_U64`` lines with value kind -1 and are
    shared by SUM and AVG; MIN of a two-lane decimal has its high key in an ``MA_MAX`` line and its low key in a line
    of the new op, named to the combine by ``lodesc``; a narrow MIN is a plain int64 slot with a decimal dtype;
    ``pfin`` has exactly the suffixes of ``distagg._partials``; SUM of decimal(30,2) is ineligible with a reason of
    its own; a layout without decimals has no decimal job and no ``lodesc``."""
    from dxa.engine import distagg as D
    from dxa.engine.column import materialize
    from dxa.engine.decimal import DecimalType
    from dxa.engine.expr import Scope, evaluate
    from dxa.engine.window_dense import Ineligible
    from dxa.ops.groupby import (_DEC_KEY_MAX, _DEC_KEY_MIN, _DEC_SUM, _F_COUNT, _F_DEC_AVG, _F_DEC_MM, _F_DEC_SUM,
                                 _F_HI, _F_I64, _F_NOT, _MA_ADD_F64, _MA_ADD_U64, _MA_LOKEY, _MA_MAX, _MV_I64, _MV_NOT)
    from dxa.sql.parser import parse_select_item
    import numpy as np
    empty = batch(np.random.default_rng(0), 100 * S, np.arange(4)).take(torch.empty(0, dtype=torch.int64))
    ctx = EvalContext(now_us=0)
    scope = Scope.of_table(empty, "W")

    def layout(aggs):
        return layout_of(aggs, empty)

    items = ["COUNT(*)", f"SUM({N18})", f"AVG({N18})", f"MIN({N18})", f"SUM({WIDE})", f"AVG({WIDE})", f"MIN({WIDE})",
             f"MAX({WIDE})", f"STDDEV({WIDE})", "AVG(hum)"]
    aggs = aggs_of(*items)
    reqs, types, L = layout(aggs)
    n18, wide = reqs[1][2].key(), reqs[4][2].key()
    assert types[n18] == (DecimalType(18, 2), False) and types[wide] == (DecimalType(24, 1), False)
    slot_keys = [s[0] for s in L["slots"]]
    where = {i: w for w, i in enumerate(L["order"]) if i is not None}
    word = {k: where[i] for i, k in enumerate(slot_keys)}
    kind_of = {s[0]: (s[1], s[2]) for s in L["slots"]}
    # one set of limb words per argument, shared by SUM and AVG, unused by agg_multi, in u64 add lines
    for ck in (n18, wide):
        assert [k for k in slot_keys if k[1] == ck and k[0].startswith("dw")] == [("dw0", ck), ("dw1", ck), ("dw2", ck)]
        for q in range(3):
            assert kind_of[(f"dw{q}", ck)] == (-1, _MA_ADD_U64)
            assert L["line_ops"][word[(f"dw{q}", ck)] >> 3] == _MA_ADD_U64
    assert L["line_ops"] == [_MA_ADD_U64, _MA_ADD_F64, _MA_MAX, 3, _MA_LOKEY] and L["stride"] == 40
    cn, cw = word[("count", n18)], word[("count", wide)]
    n0, n1, n2 = (word[(f"dw{q}", n18)] for q in range(3))
    w0, w1, w2 = (word[(f"dw{q}", wide)] for q in range(3))
    assert L["rows"] == [(0, 1), (1, 2), (3, 2), (5, 1), (6, 2), (8, 2), (10, 2), (12, 2), (14, 1), (15, 1)]
    assert L["fin"][1:3] == [(_F_DEC_SUM, n0, cn, n1, n2), (_F_DEC_SUM | _F_HI, n0, cn, n1, n2)]
    assert L["fin"][3:5] == [(_F_DEC_AVG, n0, cn, n1, n2), (_F_DEC_AVG | _F_HI, n0, cn, n1, n2)]
    assert L["fin"][6:8] == [(_F_DEC_SUM, w0, cw, w1, w2), (_F_DEC_SUM | _F_HI, w0, cw, w1, w2)]
    # the narrow MIN: the int64 MIN slot, one row, the argument's type
    assert kind_of[("min", n18)] == (_MV_I64 | _MV_NOT, _MA_MAX)
    assert L["fin"][5] == (_F_I64 | _F_NOT, word[("min", n18)], cn)
    # the two-lane MIN / MAX: high key in a MAX line, low key in a line of the new op and unused by agg_multi
    for func, inv in (("min", True), ("max", False)):
        hi, lo = word[(func, wide)], word[("lo" + func, wide)]
        assert kind_of[(func, wide)] == (_MV_I64 | (_MV_NOT if inv else 0), _MA_MAX)
        assert kind_of[("lo" + func, wide)] == (-1, _MA_LOKEY)
        assert L["line_ops"][hi >> 3] == _MA_MAX and L["line_ops"][lo >> 3] == _MA_LOKEY
        assert L["lodesc"][lo] == hi | 1 << 16
        k = _F_DEC_MM | (_F_NOT if inv else 0)
        r0 = 10 if inv else 12
        assert L["fin"][r0:r0 + 2] == [(k, hi, cw, lo, -1), (k | _F_HI, hi, cw, lo, -1)]
    assert sum(1 for d in L["lodesc"] if d) == 2
    assert sorted(L["decargs"]) == sorted([
        (n18, _DEC_SUM, n0, n1, n2), (wide, _DEC_SUM, w0, w1, w2),
        (wide, _DEC_KEY_MIN, word[("lomin", wide)], word[("min", wide)], -1),
        (wide, _DEC_KEY_MAX, word[("lomax", wide)], word[("max", wide)], -1)])
    # result types: those of the paned path
    dts = [str(p[4]) for p in L["plan"]]
    assert dts[1:8] == ["decimal(28,2)", "decimal(22,6)", "decimal(18,2)", "decimal(34,1)", "decimal(28,5)",
                        "decimal(24,1)", "decimal(24,1)"] and dts[8] == "double"
    # partial states: the suffixes distagg._partials produces for the same calls; 128-bit states are two recipes
    gx = [parse_select_item("deviceId").expr]
    keys = [materialize(evaluate(g, scope, ctx)) for g in gx]
    assert D.decomposable(aggs, ctx)
    _partial, plan, _kn = D.local_partials(gx, keys, aggs, scope, ctx)
    for ak in aggs:
        assert set(L["pfin"][ak]) == {sfx for _nm, sfx, _op in plan[ak]}, ak
    aks = list(aggs)
    total_n = [(_F_DEC_SUM, n0, cn, n1, n2), (_F_DEC_SUM | _F_HI, n0, cn, n1, n2)]
    assert L["pfin"][aks[1]] == {"v": total_n, "cnt": (_F_COUNT, cn, -1)}
    assert L["pfin"][aks[2]] == {"davg_18_2": total_n, "cnt": (_F_COUNT, cn, -1)}
    assert set(L["pfin"][aks[5]]) == {"davg_24_1", "cnt"}
    assert L["pfin"][aks[6]]["v"] == L["fin"][10:12]
    # the variance family over a decimal: the ordinary f64 words
    assert ("sumf", wide) in word and ("m2", wide) in word
    # more than 28 digits: Spark's sum type is capped, the total can overflow
    with pytest.raises(Ineligible, match="decimal precision"):
        layout(aggs_of("SUM(CAST(temp AS DECIMAL(30,2)))"))
    with pytest.raises(Ineligible, match="decimal precision"):
        layout(aggs_of("AVG(CAST(temp AS DECIMAL(29,2)))"))
    layout(aggs_of("SUM(CAST(temp AS DECIMAL(28,2)))", "MIN(CAST(temp AS DECIMAL(38,2)))"))
    # a statement without decimals keeps its layout and has no decimal job and no low-key descriptor
    _r, _t, Lo = layout(aggs_of("COUNT(*)", "SUM(temp)", "MIN(temp)", "AVG(hum)"))
    assert "decargs" not in Lo and "lodesc" not in Lo and _MA_LOKEY not in Lo["line_ops"]
    assert Lo["rows"] == [(j, 1) for j in range(4)] and Lo["fin"] == [(0, 8, -1), (1, 0, 9), (9, 16, 9), (3, 11, 10)]


def test_cpu_stream_takes_the_pane_partials():
    """On a CPU device the decimal statements are answered from pane partials (no dense state is created) and equal
    the oracle — which guards the oracle and the streams: the tie groups are seen whole, with exact halves."""
    store = new_store(6)
    run_stream(stable_stream(batch, 8), [Q_ALL, Q_FAM], torch.device("cpu"), store, TYPED)
    run_stream(carry_stream(8), [Q_CARRY], torch.device("cpu"), new_store(6), TYPED)
    seen = {"null": 0, "one": 0, "tie": set()}
    run_stream(ties_stream(12), [Q_TIES], torch.device("cpu"), new_store(6), TYPED, tie_checker(seen))
    assert seen["tie"] == {3201, 3202, 6401, 6402, 6403, 6404} and seen["null"] > 12 and seen["one"] > 6, seen
    assert not dense_states(store)


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("block", [16, 2])
def test_all_decimal_aggregates_in_one_statement(gpu, monkeypatch, block):
    """SUM, AVG, MIN and MAX over a narrow and a two-lane decimal beside COUNT(*), a double AVG and COUNT(DISTINCT
    kind), with blocks of 2 panes or none; and COUNT, count_if and the f64 families over decimal arguments.  Before
    decimals were eligible both statements were disabled with "argument type"."""
    from dxa.engine import window_dense
    from dxa.ops.groupby import _MA_LOKEY
    monkeypatch.setattr(window_dense, "BLOCK", block)
    store = new_store(6)
    seen = {"blocks": 0}

    def each(b, q, rows, view, table):
        for d in dense_states(store).values():
            if not d.disabled:
                seen["blocks"] = max(seen["blocks"], len(d.blocks))

    run_stream(stable_stream(batch, 14), [Q_ALL, Q_FAM], gpu, store, TYPED, each)
    states = list(dense_states(store).values())
    assert len(states) == 2
    for d in states:
        assert not d.disabled and d.disabled_reason is None
    d = states[0]
    assert _MA_LOKEY in d.layout["line_ops"] and d.lodesc_dev is not None and len(d.layout["decargs"]) == 4
    assert len(d.pairs) == 1 and "decargs" not in states[1].layout
    assert (seen["blocks"] > 0) == (block == 2)


@pytest.mark.gpu
def test_carries_and_signs(gpu, monkeypatch):
    """Limb sums that carry, negatives in the high limb, a group of negatives only, and two-lane MIN / MAX whose
    extremes share the high word (lo on both sides of 2^63) or differ in it, with candidates in different panes and
    2-pane blocks, so both combines apply the "slots whose high word is the extreme" rule."""
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "BLOCK", 2)
    store = new_store(6)
    seen = {"lo": 0, "split": 0}

    def each(b, q, rows, view, table):
        for r in rows:
            if r["deviceId"] == 100:
                assert r["sb"] < 0 and r["mxb"] < 0 and r["sw"] < 0 and r["mxw"] < 0 and r["aw"] < 0, r
            if r["deviceId"] in (200, 201):
                hi = 5 if r["deviceId"] == 200 else -3
                mx, mn = int(r["mxw"].scaleb(3)), int(r["mnw"].scaleb(3))
                assert mx >> 64 == hi and mn >> 64 == hi and (mx & (HI - 1)) >= HALF > (mn & (HI - 1)), r
                seen["lo"] += 1
            if r["deviceId"] == 202 and r["c"] >= 4:
                mx, mn = int(r["mxw"].scaleb(3)), int(r["mnw"].scaleb(3))
                assert mx >> 64 == 5 and (mx & (HI - 1)) < 100 and mn >> 64 == 4 and (mn & (HI - 1)) > HALF, r
                seen["split"] += 1

    run_stream(carry_stream(14), [Q_CARRY], gpu, store, TYPED, each)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert seen["lo"] > 14 and seen["split"] > 6, seen


@pytest.mark.gpu
def test_avg_ties_round_away_from_zero(gpu):
    """Groups of exactly 32 and 64 rows over four panes whose quotient at scale s + 4 is an exact half (or, 64 rows
    and an odd sum, a quarter), positive and negative; a one-row group; a group whose argument is always NULL."""
    store = new_store(6)
    seen = {"null": 0, "one": 0, "tie": set()}
    run_stream(ties_stream(14), [Q_TIES], gpu, store, TYPED, tie_checker(seen))
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert seen["tie"] == {3201, 3202, 6401, 6402, 6403, 6404} and seen["null"] > 14 and seen["one"] > 7, seen


@pytest.mark.gpu
def test_straddles_the_lds_bound(gpu, monkeypatch):
    """Group ids on both sides of the decimal pass's LDS bound in one pane (two rows per id, several workgroups), and
    a second statement whose three groups are all summed in LDS."""
    from dxa.engine import window_dense
    from dxa.ops import native as N
    L = N.lib().dxa_win_m2_lds_groups()
    assert L > 0
    if L + 200 > window_dense.DENSE_GROUPS:
        monkeypatch.setattr(window_dense, "DENSE_GROUPS", 2 * (L + 200))
    store = new_store(6)
    run_stream(two_rows_per_id_stream(batch, 9, L + 200), [Q_SMALL, Q_MOD], gpu, store, TYPED)
    states = list(dense_states(store).values())
    assert len(states) == 2 and not any(d.disabled for d in states)
    assert all(len(d.layout["decargs"]) == 4 for d in states)


@pytest.mark.gpu
def test_rebuild_moves_the_decimal_words(gpu, monkeypatch):
    """Ids drift through a 16-id dictionary that grows to 64 at most: every rebuild renumbers the limb words and the
    low-key line with the others, and the 2-pane blocks are combined again afterwards."""
    from dxa.ops.groupby import _MA_LOKEY
    set_caps(monkeypatch, 16, 64, 1 << 16, 1 << 20, block=2)
    store = new_store(6)
    run_stream(churn_stream(batch, 40), [Q_SMALL], gpu, store, TYPED)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert d.rebuilds > 0 and d.gcap <= 64 and _MA_LOKEY in d.layout["line_ops"]


@pytest.mark.gpu
def test_partials_at_world_size_one(gpu, monkeypatch):
    """The N-rank form at world size 1 (``as_partitioned_world_of_one``): the ring hands ``merge_partials`` the
    decimal states of ``distagg._partials``, two-lane ones as [n, 2]."""
    calls, prepare = as_partitioned_world_of_one(monkeypatch)
    store = new_store(6)
    stream = churn_stream(batch, 12)
    q = Q_ALL.replace(", COUNT(DISTINCT kind) AS dk", "")       # (a distinct count has no mergeable partial)
    run_stream(stream, [q], gpu, store, TYPED, prepare=prepare)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert calls["n"] >= len(stream) - 4          # (the watermark keeps the first windows empty)


@pytest.mark.gpu
def test_sum_beyond_28_digits_keeps_the_paned_path(gpu):
    store = new_store(6)
    run_stream(churn_stream(batch, 10), [Q_P30], gpu, store, TYPED)
    d = only_state(store)
    assert d.disabled and d.disabled_reason == "decimal precision"


@pytest.mark.gpu
@pytest.mark.parametrize("q,dec", [(Q_SMALL, 1), (Q_INT, 0)])
def test_one_decimal_pass_per_accumulated_pane(gpu, monkeypatch, q, dec):
    """In steady state (one pane enters the window per batch, nothing is rebuilt) a layout with decimal words calls
    ``dxa_win_dec`` once per accumulated pane, right after the multi-aggregate, and nothing more per answer; a layout
    without them never calls it and hands the combine no low-key descriptor."""
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "BLOCK", 2)
    store = new_store(6)
    pane = ["dxa_win_insert_fused", "dxa_aggregate_multi", *["dxa_win_dec"] * dec]
    completed_seen = set()
    # the watermark and the 6-pane window: full from batch 7 on
    for b, native, completed in steady_state_launches(gpu, store, small_stream(batch, 14, mid_pane=True), q, TYPED, 8):
        d = only_state(store)
        assert not d.disabled and d.rebuilds == 0
        completed_seen.add(completed)
        assert native == pane + ["dxa_win_combine_block"] * completed + ["dxa_win_answer"], (b, native)
    assert completed_seen == {0, 1}
    d = only_state(store)
    assert (d.lodesc_dev is not None) == bool(dec) and ("decargs" in d.layout) == bool(dec)
