"""The dense window path over key sets that come and go (window_dense.py ``DenseWindow.rebuild``, window_ring.hip
dxa_win_live / dxa_win_remap_dict / dxa_win_remap_ring / dxa_win_rehash): when the group dictionary fills it is
rebuilt over the groups that still have rows in retained panes, and grown when most of them do, so the statement
stays on the dense path.  The oracle is the CPU evaluator over the materialised window (no GPU code in it); ``temp``
values are multiples of 0.25 in [0, 64), so every double sum is exact in any order and rows compare exactly."""
import json

import pytest
import torch

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from dxa.engine.expr import EvalContext
from dxa.engine.query import Catalog, run_sql
from dxa.engine.serialize import table_to_json_lines
from dxa.engine.windows import TimeWindowConf, WindowStore

S = 1_000_000
AGGS = "COUNT(*) AS c, SUM(temp) AS s, MIN(temp) AS mn, MAX(temp) AS mx, AVG(temp) AS av"
Q_INT = f"SELECT deviceId, {AGGS} FROM W GROUP BY deviceId"
STR_KEY = "concat('dev-', CAST(deviceId AS STRING))"
Q_STR = f"SELECT {STR_KEY} AS dev, {AGGS} FROM W WHERE temp > 8 GROUP BY {STR_KEY}"
STABLE = 200                       # stable ids 1000 .. 1199 (tests 2 and 3)


def drifting_ids(rng, b, n):
    """Batch ``b``'s drifting ids: uniform in [4b, 4b + 12)."""
    return rng.integers(4 * b, 4 * b + 12, n)


def batch(rng, t_us, ids):
    """tests/test_windows.py::batch with given device ids and exactly summable temperatures."""
    n = len(ids)
    ts = torch.tensor([t_us - int(rng.integers(0, S - 1)) for _ in range(n)], dtype=torch.int64)
    temp = torch.tensor(rng.integers(0, 256, n) * 0.25, dtype=torch.float64)
    valid = torch.tensor(rng.random(n) > 0.1)
    kinds = strings_from_pylist([["a", "b", "c"][int(i) % 3] for i in rng.integers(0, 3, n)], "cpu")
    return Table(["ts", "deviceId", "kind", "temp"],
                 [PrimColumn("timestamp", ts), PrimColumn("long", torch.tensor(ids, dtype=torch.int64)), kinds,
                  PrimColumn("double", temp, valid)], n, "cpu")


def churn_stream(nb):
    """Test 1's stream: 200 rows per batch over the drifting ids → [(batch time, CPU table, ids)]."""
    import numpy as np
    rng = np.random.default_rng(23)
    out = []
    for b in range(nb):
        ids = drifting_ids(rng, b, 200)
        out.append(((100 + b) * S, batch(rng, (100 + b) * S, ids), ids))
    return out


def stable_stream(nb, drift):
    """300 rows per batch: 200 over the stable ids and 100 over the drifting ids (or all 300 stable)."""
    import numpy as np
    rng = np.random.default_rng(29)
    out = []
    for b in range(nb):
        ids = rng.integers(1000, 1000 + STABLE, 300)
        if drift:
            ids[200:] = drifting_ids(rng, b, 100)
        out.append(((100 + b) * S, batch(rng, (100 + b) * S, ids), ids))
    return out


def _canon(t):
    out = []
    for r in (json.loads(x) for x in table_to_json_lines(t)):
        out.append(tuple(sorted((k, round(v, 6) if isinstance(v, float) else v) for k, v in r.items())))
    return sorted(out)


def oracle(q, view):
    """The CPU evaluator's rows for statement ``q`` over the materialised window ``view``."""
    mat = Table(view.names, view.columns, view.length, view._device)
    cat = Catalog()
    cat.register("W", mat.to("cpu"))
    return _canon(run_sql(q, cat, EvalContext(now_us=0)))


def new_store(win=6):
    return WindowStore(TimeWindowConf({"W": win * S}, True, "ts", 2 * S, win * S, False))


def dense_states(store):
    return store.__dict__.get("_dense", {})


def set_caps(monkeypatch, groups, groups_max, block=None):
    from dxa.engine import window_dense
    monkeypatch.setattr(window_dense, "DENSE_GROUPS", groups)
    monkeypatch.setattr(window_dense, "DENSE_GROUPS_MAX", groups_max, raising=False)
    if block is not None:
        monkeypatch.setattr(window_dense, "BLOCK", block)


def run_stream(stream, qs, dev, store, each=None):
    """Every statement over every batch's window equals the CPU oracle; ``each(b, q, got)`` after each."""
    for b, (T, tbl, _ids) in enumerate(stream):
        views, _ = store.process(tbl.to(dev), T, S)
        for q in qs:
            cat = Catalog()
            cat.register("W", views["W"])
            got = run_sql(q, cat, EvalContext(now_us=0, device=dev))
            rows = _canon(got)
            assert rows == oracle(q, views["W"]), (b, q)
            if each is not None:
                each(b, q, got, rows)


def test_target_capacity_policy():
    """Double while more than half is live and the maximum allows: the issue's five cases."""
    from dxa.engine.window_dense import _target_capacity
    assert _target_capacity(10, 64, 64) == 64
    assert _target_capacity(33, 64, 1024) == 128
    assert _target_capacity(200, 64, 1024) == 512
    assert _target_capacity(600, 64, 1024) == 1024
    assert _target_capacity(48, 64, 64) == 64


@pytest.mark.gpu
def test_churn_recycles_the_dictionary(gpu, monkeypatch):
    """168 distinct ids stream through a 64-id dictionary that may not grow; no ten consecutive batches hold more
    than 48, so recycling alone keeps both statements (integer key; string key with a WHERE) on the dense path."""
    set_caps(monkeypatch, 64, 64)
    stream = churn_stream(40)
    ids = [set(int(i) for i in s[2]) for s in stream]
    assert len(set().union(*ids)) == 168
    assert max(len(set().union(*ids[b:b + 10])) for b in range(len(ids))) <= 48
    store = new_store()
    run_stream(stream, [Q_INT, Q_STR], torch.device("cuda", 0), store)
    dense = dense_states(store)
    assert len(dense) == 2
    for d in dense.values():
        assert not d.disabled and d.disabled_reason is None
        assert d.rebuilds >= 3 and d.gcap == 64


@pytest.mark.gpu
def test_growth_when_most_groups_stay_live(gpu, monkeypatch):
    """200 stable ids beside the drifting ones: the live set is larger than the initial capacity, so the rebuild
    doubles it (more than once in the first batch) and block slots are combined again after a rebuild."""
    set_caps(monkeypatch, 64, 1024, block=2)
    store = new_store()
    run_stream(stable_stream(24, True), [Q_STR, Q_INT], torch.device("cuda", 0), store)
    dense = dense_states(store)
    assert len(dense) == 2
    for d in dense.values():
        assert not d.disabled and d.rebuilds >= 1
        assert 256 <= d.gcap <= 1024
    assert any(d.blocks for d in dense.values())


@pytest.mark.gpu
def test_rebuild_recombines_more_than_four_blocks(gpu, monkeypatch):
    """A 12 s window of 2-pane blocks holds five or more complete blocks, and a rebuild clears the block cache: the
    next pass combines all of them again back to back, each with its own member list staged through pinned memory
    (a sliding window otherwise stages one block's list and the answer's per batch).  Rows equal the oracle through
    every rebuild."""
    set_caps(monkeypatch, 64, 128, block=2)
    store = new_store(win=12)
    seen = {"rebuilds": 0, "blocks": 0}

    def each(b, q, got, rows):
        d = next(iter(dense_states(store).values()), None)
        if d is not None and d.rebuilds > seen["rebuilds"]:
            seen["rebuilds"] = d.rebuilds
            seen["blocks"] = max(seen["blocks"], len(d.blocks))

    run_stream(churn_stream(60), [Q_INT], torch.device("cuda", 0), store, each)
    d = next(iter(dense_states(store).values()))
    assert not d.disabled and d.gcap == 128 and d.rebuilds >= 3
    assert seen["blocks"] > 4


@pytest.mark.gpu
def test_capacity_reached_falls_back_with_a_reason(gpu, monkeypatch):
    """200 live ids cannot fit 64 and the dictionary may not grow: the retry loop ends, the paned path answers
    every batch, and the state says why."""
    set_caps(monkeypatch, 64, 64)
    store = new_store()
    run_stream(stable_stream(8, False), [Q_INT], torch.device("cuda", 0), store)
    dense = dense_states(store)
    assert len(dense) == 1
    for d in dense.values():
        assert d.disabled and d.disabled_reason == "dictionary full"


@pytest.mark.gpu
def test_earlier_outputs_survive_a_rebuild(gpu, monkeypatch):
    """Output strings are views of the dictionary arena: the table of batch b - 1 renders the same rows after batch
    b rebuilt the dictionary (key columns move into fresh tensors, never in place)."""
    set_caps(monkeypatch, 64, 64)
    store = new_store()
    prev = {}
    seen = []

    def each(b, q, got, rows):
        rebuilds = sum(d.rebuilds for d in dense_states(store).values())     # (no state before the first rows)
        if prev and rebuilds > prev["rebuilds"]:
            assert _canon(prev["table"]) == prev["rows"], b
            seen.append(b)
        prev.update(table=got, rows=rows, rebuilds=rebuilds)

    run_stream(churn_stream(40), [Q_STR], torch.device("cuda", 0), store, each)
    assert seen


@pytest.mark.gpu
def test_deferred_overflow_rebuilds_in_the_same_batch(gpu, monkeypatch):
    """ctx.defer_dense: the "dictionary full" status arrives through the DeferredTable's completion; its re-run of
    the statement rebuilds and answers from the ring, and the state stays enabled."""
    from dxa.engine.column import DeferredTable
    set_caps(monkeypatch, 64, 64)
    dev = torch.device("cuda", 0)
    store = new_store()
    through_deferred = 0
    for b, (T, tbl, _ids) in enumerate(churn_stream(40)):
        views, _ = store.process(tbl.to(dev), T, S)
        ctx = EvalContext(now_us=0, device=dev)
        ctx.defer_dense = True
        cat = Catalog()
        cat.register("W", views["W"])
        got = run_sql(Q_INT, cat, ctx)
        if b >= 4:
            assert isinstance(got, DeferredTable) and ctx.pending
        before = sum(d.rebuilds for d in dense_states(store).values())
        assert _canon(got) == oracle(Q_INT, views["W"]), b
        through_deferred += sum(d.rebuilds for d in dense_states(store).values()) > before
    dense = dense_states(store)
    assert len(dense) == 1 and not any(d.disabled for d in dense.values())
    assert through_deferred >= 1
