"""COUNT / MIN / MAX of a string argument over sliding windows from the dense ring (window_dense.py ``plan_layout`` /
``DenseWindow.accumulate`` / ``str_column_of``, window_ring.hip dxa_win_strkey / win_combine_kernel's string branch /
win_emit_kernel's F_STRW, str_minmax.hip).  The oracle is the CPU evaluator over the materialised window (Python's
``str`` order; no GPU code in it).  Everything compares exactly.  Every test asserts that the statement stayed on the
ring unless it tests a fallback: before string arguments were eligible each of these statements disabled its state
with "argument type"."""
import numpy as np
import pytest
import torch

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from tests.string_sets import draw
from tests.window_dense_support import (S, Comparison, _stream, as_partitioned_world_of_one, churn_stream,
                                        dense_states, materialised, new_store, on_the_ring, only_state, run_stream,
                                        set_caps, steady_state_launches, two_rows_per_id_stream)

BITS = Comparison("bits")
AGGS = ("COUNT(*) AS c, COUNT(name) AS cn, MIN(name) AS mn, MAX(name) AS mx, AVG(temp) AS av, "
        "COUNT(DISTINCT name) AS dn")
Q_BY_ID = f"SELECT deviceId, {AGGS} FROM W GROUP BY deviceId"
Q_BY_KIND = f"SELECT kind, {AGGS} FROM W GROUP BY kind"
Q_MERGEABLE = ("SELECT deviceId, COUNT(*) AS c, COUNT(name) AS cn, MIN(name) AS mn, MAX(name) AS mx, AVG(temp) AS av "
               "FROM W GROUP BY deviceId")
Q_WHERE = ("SELECT deviceId, COUNT(*) AS c, COUNT(name) AS cn, MIN(name) AS mn, MAX(name) AS mx FROM W WHERE keep = 1 "
           "GROUP BY deviceId")
Q_GLOBAL = f"SELECT {AGGS} FROM W WHERE keep = 1"
Q_MAX = "SELECT deviceId, COUNT(*) AS c, MAX(name) AS mx, AVG(temp) AS av FROM W GROUP BY deviceId"
Q_PLAIN = "SELECT deviceId, COUNT(*) AS c, MAX(temp) AS mt, AVG(temp) AS av FROM W GROUP BY deviceId"
ALL_NULL, ALL_EQUAL = 900, 901          # devices whose names are all NULL / all the same string
TOP, BOTTOM = "\U0010FFFF", ""          # above / below every other value of the set
TOO_LONG = TOP * 12 + "z"               # 49 bytes, one more than a line holds, and above every value: it wins MAX
assert len(TOO_LONG.encode()) == 49


def batch(rng, T, ids, spread=S - 1, names=None, keep=None):
    """The given device ids with event times within ``spread`` before ``T``; ``name`` drawn from the shared string
    set with NULLs (device 900: all NULL, device 901: all "same"); ``kind`` a string key; ``temp`` a multiple of
    0.25."""
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    ts = T - rng.integers(0, spread, n)
    drawn = draw(rng, n)
    if names is not None:
        drawn = [d if s is ... else s for d, s in zip(drawn, names)]
    drawn = [None if g == ALL_NULL else "same" if g == ALL_EQUAL else s for g, s in zip(ids, drawn)]
    kinds = strings_from_pylist([["a", "b", "é"][int(g) % 3] for g in ids], "cpu")
    return Table(["ts", "deviceId", "kind", "temp", "name", "keep"],
                 [PrimColumn("timestamp", torch.tensor(ts, dtype=torch.int64)),
                  PrimColumn("long", torch.tensor(ids, dtype=torch.int64)), kinds,
                  PrimColumn("double", torch.tensor(rng.integers(0, 256, n) * 0.25, dtype=torch.float64)),
                  strings_from_pylist(drawn, "cpu"),
                  PrimColumn("long", torch.tensor(np.ones(n, dtype=np.int64) if keep is None else keep))], n, "cpu")


def string_stream(nb, whole=False, edit=None):
    """The shared stream builder over this file's schema: 40 rows per batch over 4 ids and two rows each of devices 900
    and 901.  Event times spread over a whole second around the boundary before the batch time, so the panes at both
    edges of a window are clipped; ``whole``: in the middle half of the second, so every pane is wholly inside a window
    or outside it.  ``edit(b, ids)`` → (names, keep) overrides per row (``...``: keep the drawn name)."""
    def ids_of(rng, b):
        ids = np.concatenate([rng.integers(0, 4, 40), [ALL_NULL, ALL_NULL, ALL_EQUAL, ALL_EQUAL]])
        rng.shuffle(ids)
        return ids

    def placed(rng, T, ids):
        names, keep = edit(T // S - 100, ids) if edit is not None else (None, None)
        return batch(rng, T - S // 4, ids, S // 2, names, keep) if whole else \
            batch(rng, T - S // 2, ids, S - 1, names, keep)

    return _stream(43, nb, ids_of, placed)


def _special_groups(rows):
    for r in rows:
        if r.get("deviceId") == ALL_NULL:
            assert r["cn"] == 0 and r["mn"] is None and r["mx"] is None and r["c"] > 0, r
        if r.get("deviceId") == ALL_EQUAL:
            assert r["mn"] == "same" == r["mx"], r


@pytest.mark.gpu
def test_mixed_statement(gpu):
    """COUNT(*), COUNT(name), MIN, MAX, AVG(temp) and COUNT(DISTINCT name) grouped by id and by a string key: 12
    batches, a 5-pane window, panes clipped at both edges; every value of the shared set wins somewhere."""
    store = new_store(5)
    seen = {"clipped": 0, "values": set()}

    def each(b, q, rows, view, table):
        seen["clipped"] += sum(1 for _p, full in view.pieces() if not full)
        seen["values"] |= {r["mn"] for r in rows} | {r["mx"] for r in rows}
        _special_groups(rows)

    run_stream(string_stream(12), [Q_BY_ID, Q_BY_KIND], gpu, store, BITS, each)
    for d in on_the_ring(store, 2):
        assert len(d.layout["strargs"]) == 2 and d.strdesc_dev is not None
    assert seen["clipped"] >= 10 and {"", None, "same", "\U0001F600"} <= seen["values"], seen


@pytest.mark.gpu
def test_value_leaves_the_window(gpu):
    """Batch 4 alone holds device 0's maximum (a value above the whole set): the result drops back to the next value
    when that pane expires."""
    def edit(b, ids):
        names = [...] * len(ids)
        if b == 4:
            names[int(np.flatnonzero(ids == 0)[0])] = TOP
        return names, None

    store = new_store(5)
    held = {}

    def each(b, q, rows, view, table):
        for r in rows:
            if r["deviceId"] == 0:
                held[b] = r["mx"] == TOP

    run_stream(string_stream(14, whole=True, edit=edit), [Q_MERGEABLE], gpu, store, BITS, each)
    on_the_ring(store)
    with_top = [b for b, top in held.items() if top]
    assert len(with_top) == 5 and with_top == list(range(with_top[0], with_top[0] + 5)), held
    assert with_top[0] - 1 in held and max(with_top) < max(held), held


@pytest.mark.gpu
def test_straddles_the_lds_bound(gpu):
    """1,100 groups, two rows each per batch: ids on both sides of the arg-extreme kernel's LDS bound in every pane."""
    from dxa.ops import native as N
    assert 0 < N.lib().dxa_win_m2_lds_groups() < 1100
    store = new_store(5)
    run_stream(two_rows_per_id_stream(batch, 6, 1100), [Q_MERGEABLE], gpu, store, BITS)
    on_the_ring(store)


@pytest.mark.gpu
def test_blocks_complete(gpu, monkeypatch):
    """``BLOCK`` = 2 and a 6-pane window: complete blocks are pre-combined by the string branch and expire."""
    set_caps(monkeypatch, block=2)
    store = new_store(6)
    seen = {"blocks": set()}

    def each(b, q, rows, view, table):
        if dense_states(store):
            seen["blocks"] |= set(only_state(store).blocks)
            seen["now"] = set(only_state(store).blocks)
        _special_groups(rows)

    run_stream(string_stream(14, whole=True), [Q_BY_ID], gpu, store, BITS, each)
    on_the_ring(store)
    assert len(seen["blocks"]) >= 3 and seen["blocks"] - seen["now"], seen


@pytest.mark.gpu
def test_where_removes_the_would_be_winners(gpu):
    """Every batch holds, per device, the greatest and the smallest string of all in rows that WHERE removes: they go
    to the dump row and win nothing."""
    def edit(b, ids):
        names, keep = [...] * len(ids), np.ones(len(ids), dtype=np.int64)
        for g in range(4):
            at = np.flatnonzero(ids == g)
            if len(at) >= 4:
                names[at[0]], names[at[-1]] = TOP, BOTTOM
                keep[at[0]] = keep[at[-1]] = 0
        return names, keep

    store = new_store(5)
    seen = {"bait": 0}

    def each(b, q, rows, view, table):
        mat = materialised(view)
        seen["bait"] += sum(1 for k in mat.column("keep").to_pylist() if k == 0)
        for r in rows:
            assert r["mx"] != TOP, r            # (the set's own "" may still win MIN in a row that is kept)

    run_stream(string_stream(12, edit=edit), [Q_WHERE], gpu, store, BITS, each)
    on_the_ring(store)
    assert seen["bait"] > 50, seen


@pytest.mark.gpu
def test_global_form(gpu):
    """No GROUP BY: one group under a constant key; while nothing in the window passes the WHERE the one output row has
    counts 0 and NULL strings."""
    def edit(b, ids):
        return None, np.full(len(ids), int(b >= 7), dtype=np.int64)

    store = new_store(5)
    seen = {"empty": 0, "full": 0}

    def each(b, q, rows, view, table):
        (r,) = rows
        if r["c"] == 0:
            assert r["mn"] is None and r["mx"] is None and r["cn"] == 0 and r["dn"] == 0, r
            seen["empty"] += bool(dense_states(store))
        else:
            assert r["mn"] is not None and r["mx"] is not None, r
            seen["full"] += 1

    run_stream(string_stream(16, edit=edit), [Q_GLOBAL], gpu, store, BITS, each)
    d, = on_the_ring(store)
    assert d.global_form and seen["empty"] >= 3 and seen["full"] >= 5, seen


@pytest.mark.gpu
def test_rebuild_moves_the_string_lines(gpu, monkeypatch):
    """Ids drift through a 16-id dictionary that grows to 64 at most: every rebuild renumbers the string lines with the
    other words, and a new id starts from the line's identity."""
    set_caps(monkeypatch, 16, 64, block=2)
    store = new_store(5)
    run_stream(churn_stream(batch, 30, rows=120), [Q_BY_ID], gpu, store, BITS)
    d, = on_the_ring(store)
    assert d.rebuilds > 0 and d.gcap <= 64


@pytest.mark.gpu
def test_value_too_long(gpu):
    """A 49-byte value that wins MAX — one byte more than a line holds — arrives in batch 5: from the batch whose window first holds it the state is
    disabled with "argument too long" and the paned path answers; every batch equals the oracle."""
    nb = 12

    def edit(b, ids):
        names = [...] * len(ids)
        if b == 5:
            names[int(np.flatnonzero(ids == 0)[0])] = TOO_LONG
        return names, None

    store = new_store(5)
    state = {}

    def each(b, q, rows, view, table):
        for d in dense_states(store).values():
            state[b] = (d.disabled, d.disabled_reason, TOO_LONG in materialised(view).column("name").to_pylist())

    run_stream(string_stream(nb, edit=edit), [Q_MERGEABLE], gpu, store, BITS, each)
    first = min(b for b, s in state.items() if s[2])              # the batch whose window first holds the value
    assert 5 <= first <= nb - 3
    assert all(state[b][:2] == (False, None) for b in state if b < first) and first - 1 in state
    assert all(state[b][:2] == (True, "argument too long") for b in range(first, nb))


@pytest.mark.gpu
def test_partials_at_world_size_one(gpu, monkeypatch):
    """The N-rank form at world size 1: the ring hands ``merge_partials`` the states "v" (a string column) and "cnt"
    of ``distagg._partials``, the merge runs the device MIN / MAX, and the merged rows equal the oracle's."""
    from dxa.ops import groupby

    real = groupby._host_minmax

    def host_only(groups, col, func, device):       # (the oracle runs on the CPU, where the host loop is the path)
        assert torch.device(device).type == "cpu", "the merge took the host loop"
        return real(groups, col, func, device)
    monkeypatch.setattr(groupby, "_host_minmax", host_only)
    calls, prepare = as_partitioned_world_of_one(monkeypatch)
    store = new_store(5)
    stream = string_stream(12)

    def each(b, q, rows, view, table):
        _special_groups(rows)

    run_stream(stream, [Q_MERGEABLE], gpu, store, BITS, each, prepare=prepare)
    on_the_ring(store)
    assert calls["n"] >= len(stream) - 4          # (the watermark keeps the first windows empty)


@pytest.mark.gpu
@pytest.mark.parametrize("q,strings", [(Q_PLAIN, 0), (Q_MAX, 1)])
def test_one_string_pass_per_accumulated_pane(gpu, monkeypatch, q, strings):
    """In steady state a statement without string MIN / MAX issues the entry points it always issued and never
    ``dxa_win_strkey``; one with a string MAX calls it once per accumulated pane, right after the multi-aggregate."""
    set_caps(monkeypatch, block=2)
    store = new_store(6)
    pane = ["dxa_win_insert_fused", "dxa_aggregate_multi", *["dxa_win_strkey"] * strings]
    completed_seen = set()
    # the watermark and the 6-pane window: full from batch 7 on
    for b, native, completed in steady_state_launches(gpu, store, string_stream(14, whole=True), q, BITS, 8):
        d, = on_the_ring(store)
        assert d.rebuilds == 0
        completed_seen.add(completed)
        assert native == pane + ["dxa_win_combine_block"] * completed + ["dxa_win_answer"], (b, native)
    assert completed_seen == {0, 1}
    d = only_state(store)
    assert (d.strdesc_dev is not None) == bool(strings) and ("strargs" in d.layout) == bool(strings)
