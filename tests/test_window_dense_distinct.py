"""COUNT(DISTINCT x) over sliding windows from the dense ring (window_dense.py ``PairState``, window_ring.hip
win_pair_mark / win_distinct_fold / win_pair_or): a distinct count is a count of live (group, x) pairs, kept in a
second persistent dictionary with one presence byte per ring slot.  The oracle is the CPU evaluator over the
materialised window (no GPU code in it); ``temp`` values are multiples of 0.25, so every row compares exactly."""
import struct

import pytest
import torch

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from dxa.engine.expr import EvalContext
from tests.window_dense_support import (S, Comparison, aggs_of, answer, batch, churn_stream, dense_states, new_store,
                                        only_state, oracle, run_stream, set_caps, with_syncs_counted)

JSON = Comparison("json")
Q_GRP = ("SELECT deviceId, COUNT(DISTINCT kind) AS dk, COUNT(DISTINCT temp) AS dt, COUNT(*) AS c, MAX(temp) AS mx, "
         "AVG(temp) AS av FROM W GROUP BY deviceId")
Q_GLOB = "SELECT COUNT(DISTINCT deviceId) AS dd, MAX(ts) AS last FROM W WHERE temp > 8"
Q_NONE = "SELECT COUNT(DISTINCT deviceId) AS dd, MAX(ts) AS last FROM W WHERE temp > 1000"   # never a row
Q_KIND = "SELECT deviceId, COUNT(DISTINCT kind) AS dk, SUM(temp) AS s FROM W GROUP BY deviceId"
Q_INT = ("SELECT deviceId, COUNT(*) AS c, SUM(temp) AS s, MIN(temp) AS mn, MAX(temp) AS mx, AVG(temp) AS av "
         "FROM W GROUP BY deviceId")
ALL = [Q_GRP, Q_GLOB, Q_NONE, Q_KIND]


def pair_sets(stream, col):
    """Per batch, the set of (id, value of ``col``) over its rows (NULL values as None)."""
    out = []
    for _T, tbl, ids in stream:
        vals = tbl.column(col).to_pylist()
        out.append({(int(i), v) for i, v in zip(ids, vals)})
    return out


def most_in(sets, k):
    return max(len(set().union(*sets[b:b + k])) for b in range(len(sets)))


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_requests_accept_count_distinct_only():
    """COUNT(DISTINCT x) is a request of its own beside the five plain aggregates; every other distinct form and
    approx_count_distinct stay ineligible."""
    from dxa.engine.window_dense import Ineligible, _requests
    reqs = _requests(aggs_of("COUNT(DISTINCT kind)", "COUNT(DISTINCT temp)", "COUNT(*)", "COUNT(temp)", "SUM(temp)",
                           "MIN(temp)", "MAX(temp)", "AVG(temp)", "COUNT(DISTINCT kind) + 1"))
    funcs = [f for _, f, _ in reqs]
    assert funcs.count("dcount") == 2 and set(funcs) == {"dcount", "count_star", "count", "sum", "min", "max", "avg"}
    for bad in ("SUM(DISTINCT temp)", "AVG(DISTINCT temp)", "COUNT(DISTINCT deviceId, kind)",
                "approx_count_distinct(kind)"):
        with pytest.raises(Ineligible):
            _requests(aggs_of(bad))


def test_cpu_device_takes_the_generic_path():
    """On a CPU device the four statements equal the oracle and no dense state is created."""
    store = new_store(6)
    run_stream(churn_stream(batch, 8), ALL, torch.device("cpu"), store, JSON)
    assert not dense_states(store)
    T, tbl, _ = churn_stream(batch, 1)[0]
    views, _ = new_store(6).process(tbl, T, S)
    assert oracle(Q_NONE, views["W"], JSON.rows) == [(("dd", 0),)]


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("q,npairs", [(Q_GRP, 2), (Q_GLOB, 1), (Q_NONE, 1)])
def test_stays_dense(gpu, q, npairs):
    store = new_store(6)
    run_stream(churn_stream(batch, 12), [q], torch.device("cuda", 0), store, JSON)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert len(d.pairs) == npairs


@pytest.mark.gpu
def test_pairs_recycle(gpu, monkeypatch):
    """504 (id, kind) pairs stream through a 256-pair dictionary that may not grow, and 168 ids through a 64-id
    group dictionary: both recycle, and every group rebuild renumbers the pairs' parents."""
    set_caps(monkeypatch, 64, 64, 256, 256)
    stream = churn_stream(batch, 40)
    pairs = pair_sets(stream, "kind")
    assert len(set().union(*pairs)) == 504
    assert most_in(pairs, 14) <= 192
    store = new_store(6)
    run_stream(stream, [Q_KIND], torch.device("cuda", 0), store, JSON)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert d.pairs[0].rebuilds >= 1 and d.pairs[0].pcap == 256
    assert d.rebuilds >= 3 and d.gcap == 64


@pytest.mark.gpu
def test_pairs_grow(gpu, monkeypatch):
    """The (id, temp) pairs outgrow 64: the temp pair state's capacity doubles; the (id, kind) pairs still fit."""
    set_caps(monkeypatch, 64, 64, 64, 8192)
    stream = churn_stream(batch, 40)
    pairs = pair_sets(stream, "temp")
    assert len(set().union(*pairs)) <= 6795
    assert most_in(pairs, 16) <= 2754
    store = new_store(6)
    run_stream(stream, [Q_GRP], torch.device("cuda", 0), store, JSON)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    kind, temp = d.pairs
    assert 256 <= temp.pcap <= 8192 and temp.rebuilds >= 1
    assert kind.pcap <= 8192 and kind.pcap <= temp.pcap


@pytest.mark.gpu
def test_pair_blocks(gpu, monkeypatch):
    """A 12 s window of 2-pane blocks: presence rows are ORed into block slots, and again after every rebuild."""
    set_caps(monkeypatch, 64, 128, 256, 512, block=2)
    store = new_store(12)
    seen = {"blocks": 0}

    def each(b, q, rows, view, got):
        for d in dense_states(store).values():     # (no state before the first rows)
            if d.pairs and not d.disabled:
                seen["blocks"] = max(seen["blocks"], len(d.blocks))

    run_stream(churn_stream(batch, 60), [Q_KIND], torch.device("cuda", 0), store, JSON, each)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None
    assert seen["blocks"] > 4
    assert d.rebuilds + d.pairs[0].rebuilds >= 1


@pytest.mark.gpu
def test_pair_capacity_reached_falls_back_with_a_reason(gpu, monkeypatch):
    """The temp pairs cannot fit 64 and may not grow: every batch still equals the oracle (the generic path), and
    the state says why."""
    set_caps(monkeypatch, 1 << 16, 1 << 20, 64, 64)
    store = new_store(6)
    run_stream(churn_stream(batch, 12), [Q_GRP], torch.device("cuda", 0), store, JSON)
    d = only_state(store)
    assert d.disabled and d.disabled_reason == "pair dictionary full"


def _special_stream(long_len):
    """6 batches of 64 rows (the watermark keeps the first windows empty, so 3 would show one window), string group
    key; a double with 0.0 / -0.0 / two NaN bit patterns / inf / NULL and a string with "" / a ``long_len``-byte
    value / NULL as distinct arguments."""
    nan2 = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000001))[0]
    dvals = [0.0, -0.0, float("nan"), nan2, float("inf"), 1.5, -float("inf"), 0.25]
    svals = ["", "x" * long_len, "y", "", "x" * long_len, "z" * 7, "y", "é" * 3]
    out = []
    for b in range(6):
        n = 64
        T = (100 + b) * S
        ts = torch.tensor([T - 1000 * i for i in range(n)], dtype=torch.int64)
        grp = strings_from_pylist([f"g{(i + b) % 5}" for i in range(n)], "cpu")
        d = torch.tensor([dvals[(i * 3 + b) % 8] for i in range(n)], dtype=torch.float64)
        dvalid = torch.tensor([(i + b) % 7 != 0 for i in range(n)])
        s = strings_from_pylist([svals[(i + 2 * b) % 8] for i in range(n)], "cpu")
        s.valid = torch.tensor([(i + b) % 6 != 0 for i in range(n)])
        out.append((T, Table(["ts", "grp", "d", "s"], [PrimColumn("timestamp", ts), grp, PrimColumn("double", d, dvalid),
                                                       s], n, "cpu"), None))
    return out


Q_SPECIAL = "SELECT grp, COUNT(DISTINCT d) AS dd, COUNT(DISTINCT s) AS ds, COUNT(*) AS c FROM W GROUP BY grp"


@pytest.mark.gpu
def test_special_values(gpu):
    """-0.0 counts with 0.0, every NaN as one, NULLs never; "" and a 48-byte string are values of their own."""
    store = new_store(6)
    run_stream(_special_stream(48), [Q_SPECIAL], torch.device("cuda", 0), store, JSON)
    d = only_state(store)
    assert not d.disabled and d.disabled_reason is None and len(d.pairs) == 2


@pytest.mark.gpu
def test_special_values_too_long(gpu):
    """A 49-byte string does not fit a dictionary slot: the statement leaves the dense path, rows still exact."""
    store = new_store(6)
    run_stream(_special_stream(49), [Q_SPECIAL], torch.device("cuda", 0), store, JSON)
    d = only_state(store)
    assert d.disabled and d.disabled_reason == "key too long"


@pytest.mark.gpu
def test_deferred(gpu, monkeypatch):
    """ctx.defer_dense: a full pair or group dictionary is reported through the DeferredTable's completion; the
    re-run of the statement rebuilds and answers from the ring."""
    from dxa.engine.column import DeferredTable
    set_caps(monkeypatch, 64, 64, 256, 256)
    dev = torch.device("cuda", 0)
    store = new_store(6)
    through_deferred = 0

    def rebuilds():
        return sum(d.rebuilds + sum(p.rebuilds for p in d.pairs) for d in dense_states(store).values())

    for b, (T, tbl, _ids) in enumerate(churn_stream(batch, 40)):
        views, _ = store.process(tbl.to(dev), T, S)
        ctx = EvalContext(now_us=0, device=dev)
        ctx.defer_dense = True
        got = answer(Q_KIND, views["W"], ctx=ctx)
        if b >= 4:
            assert isinstance(got, DeferredTable) and ctx.pending
        before = rebuilds()
        JSON.check(Q_KIND, views["W"], got, b)
        through_deferred += rebuilds() > before
    d = only_state(store)
    assert not d.disabled and len(d.pairs) == 1
    assert through_deferred >= 1


@pytest.mark.gpu
def test_one_sync_per_batch_and_plain_statements_unchanged(gpu):
    """A steady-state batch of Q_KIND makes one synchronising read (counted as tools/sync_audit.py counts them), and
    a statement without a distinct count on the same store gets a state with no pair states."""
    dev = torch.device("cuda", 0)
    store = new_store(6)
    counts = []
    for b, (T, tbl, _ids) in enumerate(churn_stream(batch, 12)):
        views, _ = store.process(tbl.to(dev), T, S)
        torch.cuda.synchronize(dev)
        got, syncs = with_syncs_counted(lambda: answer(Q_KIND, views["W"], dev))
        counts.append(syncs)
        JSON.check(Q_KIND, views["W"], got, b)
        JSON.check(Q_INT, views["W"], answer(Q_INT, views["W"], dev), b)
    print("synchronising calls per batch:", counts)
    assert counts[-4:] == [1, 1, 1, 1]
    states = list(dense_states(store).values())
    assert len(states) == 2 and not any(d.disabled for d in states)
    assert sorted(len(d.pairs) for d in states) == [0, 1]
