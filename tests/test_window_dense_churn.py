"""The dense window path over key sets that come and go (window_dense.py ``DenseWindow.rebuild``, window_ring.hip
dxa_win_live / dxa_win_remap_dict / dxa_win_remap_ring / dxa_win_rehash): when the group dictionary fills it is
rebuilt over the groups that still have rows in retained panes, and grown when most of them do, so the statement
stays on the dense path.  The oracle is the CPU evaluator over the materialised window (no GPU code in it); ``temp``
values are multiples of 0.25 in [0, 64), so every double sum is exact in any order and rows compare exactly."""
import pytest
import torch

from dxa.engine.expr import EvalContext
from tests.window_dense_support import (S, Comparison, answer, batch, churn_stream, dense_states, new_store, run_stream,
                                        set_caps, stable_stream)

JSON = Comparison("json")
AGGS = "COUNT(*) AS c, SUM(temp) AS s, MIN(temp) AS mn, MAX(temp) AS mx, AVG(temp) AS av"
Q_INT = f"SELECT deviceId, {AGGS} FROM W GROUP BY deviceId"
STR_KEY = "concat('dev-', CAST(deviceId AS STRING))"
Q_STR = f"SELECT {STR_KEY} AS dev, {AGGS} FROM W WHERE temp > 8 GROUP BY {STR_KEY}"


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
    stream = churn_stream(batch, 40)
    ids = [set(int(i) for i in s[2]) for s in stream]
    assert len(set().union(*ids)) == 168
    assert max(len(set().union(*ids[b:b + 10])) for b in range(len(ids))) <= 48
    store = new_store(6)
    run_stream(stream, [Q_INT, Q_STR], torch.device("cuda", 0), store, JSON)
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
    store = new_store(6)
    run_stream(stable_stream(batch, 24, True), [Q_STR, Q_INT], torch.device("cuda", 0), store, JSON)
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
    store = new_store(12)
    seen = {"rebuilds": 0, "blocks": 0}

    def each(b, q, rows, view, got):
        d = next(iter(dense_states(store).values()), None)
        if d is not None and d.rebuilds > seen["rebuilds"]:
            seen["rebuilds"] = d.rebuilds
            seen["blocks"] = max(seen["blocks"], len(d.blocks))

    run_stream(churn_stream(batch, 60), [Q_INT], torch.device("cuda", 0), store, JSON, each)
    d = next(iter(dense_states(store).values()))
    assert not d.disabled and d.gcap == 128 and d.rebuilds >= 3
    assert seen["blocks"] > 4


@pytest.mark.gpu
def test_capacity_reached_falls_back_with_a_reason(gpu, monkeypatch):
    """200 live ids cannot fit 64 and the dictionary may not grow: the retry loop ends, the paned path answers
    every batch, and the state says why."""
    set_caps(monkeypatch, 64, 64)
    store = new_store(6)
    run_stream(stable_stream(batch, 8, False), [Q_INT], torch.device("cuda", 0), store, JSON)
    dense = dense_states(store)
    assert len(dense) == 1
    for d in dense.values():
        assert d.disabled and d.disabled_reason == "dictionary full"


@pytest.mark.gpu
def test_earlier_outputs_survive_a_rebuild(gpu, monkeypatch):
    """Output strings are views of the dictionary arena: the table of batch b - 1 renders the same rows after batch
    b rebuilt the dictionary (key columns move into fresh tensors, never in place)."""
    set_caps(monkeypatch, 64, 64)
    store = new_store(6)
    prev = {}
    seen = []

    def each(b, q, rows, view, got):
        rebuilds = sum(d.rebuilds for d in dense_states(store).values())     # (no state before the first rows)
        if prev and rebuilds > prev["rebuilds"]:
            assert JSON.rows(prev["table"]) == prev["rows"], b
            seen.append(b)
        prev.update(table=got, rows=rows, rebuilds=rebuilds)

    run_stream(churn_stream(batch, 40), [Q_STR], torch.device("cuda", 0), store, JSON, each)
    assert seen


@pytest.mark.gpu
def test_deferred_overflow_rebuilds_in_the_same_batch(gpu, monkeypatch):
    """ctx.defer_dense: the "dictionary full" status arrives through the DeferredTable's completion; its re-run of
    the statement rebuilds and answers from the ring, and the state stays enabled."""
    from dxa.engine.column import DeferredTable
    set_caps(monkeypatch, 64, 64)
    dev = torch.device("cuda", 0)
    store = new_store(6)
    through_deferred = 0
    for b, (T, tbl, _ids) in enumerate(churn_stream(batch, 40)):
        views, _ = store.process(tbl.to(dev), T, S)
        ctx = EvalContext(now_us=0, device=dev)
        ctx.defer_dense = True
        got = answer(Q_INT, views["W"], ctx=ctx)
        if b >= 4:
            assert isinstance(got, DeferredTable) and ctx.pending
        before = sum(d.rebuilds for d in dense_states(store).values())
        JSON.check(Q_INT, views["W"], got, b)
        through_deferred += sum(d.rebuilds for d in dense_states(store).values()) > before
    dense = dense_states(store)
    assert len(dense) == 1 and not any(d.disabled for d in dense.values())
    assert through_deferred >= 1
