"""What the dense-window test files (tests/test_window_dense_*.py) share: the store and its dense states, the CPU oracle
over the materialised window, the row comparison, the random streams, and the loops that run a stream against the
oracle.  A family's test file holds its statements, the ``batch`` function of its schema, its special streams and its
assertions; everything a file would otherwise copy from its neighbour is here, once."""
import json
import math
import warnings

import torch

from dxa.engine.column import PrimColumn, Table, strings_from_pylist
from dxa.engine.expr import EvalContext
from dxa.engine.query import Catalog, run_sql
from dxa.engine.serialize import table_to_json_lines
from dxa.engine.windows import TimeWindowConf, WindowStore

S = 1_000_000


# ---- the store and its dense states ---------------------------------------------------------------------------------
def new_store(win):
    """A store with one sliding window ``W`` of ``win`` seconds, a 2 s watermark and 1 s batches."""
    return WindowStore(TimeWindowConf({"W": win * S}, True, "ts", 2 * S, win * S, False))


def dense_states(store):
    return store.__dict__.get("_dense", {})


def only_state(store):
    states = list(dense_states(store).values())
    assert len(states) == 1
    return states[0]


def on_the_ring(store, n=1):
    """The store's ``n`` dense states, none of them disabled."""
    states = list(dense_states(store).values())
    assert len(states) == n, len(states)
    for d in states:
        assert d.disabled_reason is None and not d.disabled, d.disabled_reason
    return states


def set_caps(monkeypatch, groups=None, groups_max=None, pairs=None, pairs_max=None, block=None):
    """Patch the given dictionary capacities (initial and maximum, of groups and of pairs) and the block size."""
    from dxa.engine import window_dense
    for name, value in (("DENSE_GROUPS", groups), ("DENSE_GROUPS_MAX", groups_max), ("DENSE_PAIRS", pairs),
                        ("DENSE_PAIRS_MAX", pairs_max), ("BLOCK", block)):
        if value is not None:
            monkeypatch.setattr(window_dense, name, value)


# ---- requests and layouts -------------------------------------------------------------------------------------------
def aggs_of(*select_items):
    """The aggregate calls of the given select items, as ``query._collect_aggs`` finds them."""
    from dxa.engine.query import _collect_aggs
    from dxa.sql.parser import parse_select_item
    aggs = {}
    for item in select_items:
        _collect_aggs(parse_select_item(item).expr, EvalContext(now_us=0), aggs)
    assert aggs
    return aggs


def assumed_types(reqs, kind=("double", True)):
    """``plan_layout``'s argument types with every argument of ``reqs`` taken to be of ``kind``."""
    out = {}
    for _, _f, arg in reqs:
        for a in arg if isinstance(arg, tuple) else () if arg is None else (arg,):
            out[a.key()] = kind
    return out


def layout_of(aggs, table, **request_flags):
    """``_requests`` of ``aggs``, the types of their arguments evaluated over an empty table of ``table``'s schema (as
    ``dense_partials`` builds its prototype), and ``plan_layout`` of both → (reqs, types, layout)."""
    from dxa.engine.column import ConstColumn
    from dxa.engine.expr import Scope, evaluate
    from dxa.engine.window_dense import _requests, plan_layout
    ctx = EvalContext(now_us=0)
    scope = Scope.of_table(table.take(torch.empty(0, dtype=torch.int64)), "W")
    reqs = _requests(aggs, **request_flags)
    types = {}
    for _, f, arg in reqs:
        for a in arg if isinstance(arg, tuple) else () if arg is None or f == "dcount" else (arg,):
            c = evaluate(a, scope, ctx)
            c = c.materialize() if isinstance(c, ConstColumn) else c
            types[a.key()] = (c.dtype, getattr(c, "data", torch.empty(0)).dtype == torch.float64)
    return reqs, types, plan_layout(reqs, types)


# ---- the oracle and the row comparison ------------------------------------------------------------------------------
def materialised(view):
    """The window's rows as one CPU table."""
    return Table(view.names, view.columns, view.length, view._device).to("cpu")


def answer(q, table, dev="cpu", ctx=None):
    """Statement ``q`` over ``table`` registered as ``W``, on ``dev`` (or under the given context)."""
    cat = Catalog()
    cat.register("W", table)
    return run_sql(q, cat, ctx or EvalContext(now_us=0, device=dev))


def rows_of(t, order_by=None):
    """The table's rows as dicts of Python values (NULL as None) in a canonical order — by the columns that hold no
    float, or by the values of column ``order_by`` — and its column dtypes as strings."""
    t = t.to("cpu")
    cols = {nm: t.column(nm).to_pylist() for nm in t.names}
    rows = [{nm: cols[nm][i] for nm in t.names} for i in range(t.length)]
    if order_by is None:
        exact = [nm for nm in t.names if not any(isinstance(r[nm], float) for r in rows)]
        rows.sort(key=lambda r: tuple(repr(r[nm]) for nm in exact))
    else:
        rows.sort(key=lambda r: r[order_by])
    return rows, {nm: str(t.column(nm).dtype) for nm in t.names}


def oracle(q, view, rows_of=rows_of):
    """The CPU evaluator's rows for statement ``q`` over the materialised window ``view`` (no GPU code in it)."""
    return rows_of(answer(q, materialised(view)))


class Comparison:
    """One rule for comparing a result with the oracle's: ``rows(table)`` makes a table comparable and calling the
    rule asserts that two such results agree.  The levels, from the loosest:

    * ``"json"``: the sorted ``table_to_json_lines`` rows with floats rounded to 6 places, compared with ``==``;
    * ``"tolerant"``: ``rows_of``; column names and order, NULLs, NaNs and every value that is no float exactly (type
      and value); a float within ``max(rel · |want|, abs_)``, or within ``dimless_abs`` with no relative test if its
      column is named in ``dimless``.  ``types``: also equal ``str()`` of the exact values and equal dtype strings;
    * ``"bits"``: ``rows_of``; as ``"tolerant"`` with ``types``, and a float equal in value and in the sign of zero.

    A tolerant rule keeps the largest deviations it saw since ``reset()``; ``report()`` prints them."""

    def __init__(self, level, rel=0.0, abs_=0.0, dimless=(), dimless_abs=0.0, types=False, order_by=None):
        assert level in ("json", "tolerant", "bits")
        self.level, self.rel, self.abs_, self.dimless, self.dimless_abs = level, rel, abs_, dimless, dimless_abs
        self.types = types or level == "bits"
        self.order_by = order_by
        self.reset()

    def reset(self):
        self.seen = {"rel": 0.0, "abs": 0.0, "dimless": 0.0}

    def report(self):
        if self.level == "tolerant":
            print(f"largest deviation from the oracle: relative {self.seen['rel']:.3e}, absolute "
                  f"{self.seen['abs']:.3e}" + (f", dimensionless (absolute) {self.seen['dimless']:.3e}"
                                               if self.dimless else ""))

    def rows(self, t):
        if self.level != "json":
            return rows_of(t, self.order_by)
        out = []
        for r in (json.loads(x) for x in table_to_json_lines(t)):
            out.append(tuple(sorted((k, round(v, 6) if isinstance(v, float) else v) for k, v in r.items())))
        return sorted(out)

    def check(self, q, view, table, what):
        """``table``, statement ``q``'s result over ``view``, agrees with the oracle's → its comparable rows."""
        got = self.rows(table)
        self(got, oracle(q, view, self.rows), what)
        return got

    def __call__(self, got, want, what):
        if self.level == "json":
            assert got == want, what
            return
        (got, gtypes), (want, wtypes) = got, want
        if self.types:
            assert list(gtypes.items()) == list(wtypes.items()), (what, gtypes, wtypes)
        assert len(got) == len(want), (what, len(got), len(want))
        for g, w in zip(got, want):
            assert list(g) == list(w), what
            for nm in w:
                a, b = g[nm], w[nm]
                if not (isinstance(a, float) and isinstance(b, float)):
                    assert type(a) is type(b) and a == b and (not self.types or str(a) == str(b)), (what, nm, g, w)
                elif math.isnan(a) or math.isnan(b):
                    assert math.isnan(a) and math.isnan(b), (what, nm, g, w)
                elif self.level == "bits":
                    assert a == b and math.copysign(1.0, a) == math.copysign(1.0, b), (what, nm, g, w)
                else:
                    self._near(a, b, nm, (what, nm, a, b, g, w))

    def _near(self, a, b, nm, what):
        if a == b:                                  # (equal infinities have no difference, and rel · inf no meaning)
            return
        dev = abs(a - b)
        if nm in self.dimless:
            self.seen["dimless"] = max(self.seen["dimless"], dev)
            assert dev <= self.dimless_abs, what
            return
        if dev > self.abs_:                         # (below the absolute tolerance a ratio says nothing)
            self.seen["rel"] = max(self.seen["rel"], dev / abs(b) if b else math.inf)
        self.seen["abs"] = max(self.seen["abs"], dev)
        assert dev <= max(self.rel * abs(b), self.abs_), what


# ---- streams: [(batch time, CPU table, ids)] ------------------------------------------------------------------------
def batch(rng, t_us, ids, spread=S - 1, temp_valid=None):
    """tests/test_windows.py::batch with given device ids and exactly summable temperatures (multiples of 0.25 in
    [0, 64), a tenth of them NULL unless ``temp_valid`` says which); event times within ``spread`` before the batch
    time.  The schema of the churn, distinct and moments files."""
    n = len(ids)
    ts = torch.tensor([t_us - int(rng.integers(0, spread)) for _ in range(n)], dtype=torch.int64)
    temp = torch.tensor(rng.integers(0, 256, n) * 0.25, dtype=torch.float64)
    valid = torch.tensor(rng.random(n) > 0.1)
    if temp_valid is not None:
        valid = torch.tensor(temp_valid)
    kinds = strings_from_pylist([["a", "b", "c"][int(i) % 3] for i in rng.integers(0, 3, n)], "cpu")
    return Table(["ts", "deviceId", "kind", "temp"],
                 [PrimColumn("timestamp", ts), PrimColumn("long", torch.tensor(ids, dtype=torch.int64)), kinds,
                  PrimColumn("double", temp, valid)], n, "cpu")


def drifting_ids(rng, b, n):
    """Batch ``b``'s drifting ids: uniform in [4b, 4b + 12)."""
    return rng.integers(4 * b, 4 * b + 12, n)


def _stream(seed, nb, ids_of, batch, **kw):
    """``nb`` one-second batches from time 100 s on: ``ids_of(rng, b)`` draws batch b's ids and ``batch(rng, T, ids,
    **kw)`` — the calling file's own — the rest of its table, from one generator."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for b in range(nb):
        ids = ids_of(rng, b)
        out.append(((100 + b) * S, batch(rng, (100 + b) * S, ids, **kw), ids))
    return out


def churn_stream(batch, nb, rows=200, **kw):
    """``rows`` rows per batch over the drifting ids."""
    return _stream(23, nb, lambda rng, b: drifting_ids(rng, b, rows), batch, **kw)


def stable_stream(batch, nb, drift=True, **kw):
    """300 rows per batch: 200 over the stable ids 1000 .. 1199 and 100 over the drifting ids (or all 300 stable)."""
    def ids_of(rng, b):
        ids = rng.integers(1000, 1200, 300)
        if drift:
            ids[200:] = drifting_ids(rng, b, 100)
        return ids
    return _stream(29, nb, ids_of, batch, **kw)


def two_rows_per_id_stream(batch, nb, nids, **kw):
    """Every batch holds ids 0 .. ``nids`` - 1 twice each, shuffled: with ``nids`` above a second pass's LDS bound,
    group ids on both sides of it in every pane, over several workgroups."""
    import numpy as np

    def ids_of(rng, b):
        ids = np.repeat(np.arange(nids), 2)
        rng.shuffle(ids)
        return ids
    return _stream(37, nb, ids_of, batch, **kw)


def small_stream(batch, nb, mid_pane=False, groups=4, rows=40):
    """40 rows per batch over 4 ids.  ``mid_pane``: event times in the middle half of the batch's second, so a pane is
    wholly inside a window or wholly outside it (none is clipped into a scratch slot) and exactly one pane enters
    the window per batch."""
    import numpy as np
    rng = np.random.default_rng(43)
    out = []
    for b in range(nb):
        ids = rng.integers(0, groups, rows)
        T = (100 + b) * S
        out.append((T, batch(rng, T - S // 4, ids, spread=S // 2) if mid_pane else batch(rng, T, ids), ids))
    return out


# ---- running a stream against the oracle ----------------------------------------------------------------------------
def run_stream(stream, qs, dev, store, compare, each=None, prepare=None, reorder=None):
    """Every statement over every batch's window equals the CPU oracle under ``compare``.  ``reorder(view)`` gives
    the view both sides read, ``prepare(view)`` marks it, and ``each(b, q, rows, view, table)`` runs after each
    comparison with the statement's comparable rows and its result table."""
    compare.reset()
    for b, (T, tbl, _ids) in enumerate(stream):
        views, _ = store.process(tbl.to(dev), T, S)
        view = views["W"] if reorder is None else reorder(views["W"])
        if prepare is not None:
            prepare(view)
        for q in qs:
            table = answer(q, view, dev)
            got = compare.check(q, view, table, (b, q))
            if each is not None:
                each(b, q, got[0] if isinstance(got, tuple) else got, view, table)
    compare.report()


def as_partitioned_world_of_one(monkeypatch):
    """The N-rank form at world size 1: ``dxa.parallel.active`` is patched and the returned ``prepare`` marks a view
    partitioned, so ``_paned_aggregate`` takes ``dense_partials`` → ``exchange_partials`` → ``merge_partials``.  The
    key exchange needs a process group, so it is replaced by what it is at world size 1: the identity.  →
    (``calls``, ``prepare``); ``calls["n"]`` counts the calls ``dense_partials`` answered."""
    from dxa import parallel as P
    from dxa.engine import distagg, window_dense
    monkeypatch.setattr(P, "active", lambda: True)
    monkeypatch.setattr(distagg, "exchange_partials", lambda partial, key_names, grouped: (partial, P.HASHED))
    calls = {"n": 0}
    real = window_dense.dense_partials

    def counted(*a, **k):
        got = real(*a, **k)
        calls["n"] += got is not None
        return got

    monkeypatch.setattr(window_dense, "dense_partials", counted)

    def prepare(view):
        view.dist = P.PARTITIONED

    return calls, prepare


def with_syncs_counted(run):
    """``run()`` → (its result, the synchronising calls it made, counted as tools/sync_audit.py counts them)."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = run()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return out, sum("prototype feature" not in str(w.message) for w in caught)


def steady_state_launches(dev, store, stream, q, compare, from_batch):
    """Statement ``q`` over every batch's window, compared with the oracle; from batch ``from_batch`` on yields per
    batch (b, the ``dxa_*`` entry points the statement called, in order, the number of blocks it completed)."""
    from launch_count import count_launches
    for b, (T, tbl, _ids) in enumerate(stream):
        views, _ = store.process(tbl.to(dev), T, S)
        states = list(dense_states(store).values())
        before = set(states[0].blocks) if states else set()
        with count_launches() as log:
            out = answer(q, views["W"], dev)
        compare.check(q, views["W"], out, (b, q))
        if b >= from_batch:
            yield b, [nm for nm in log if nm.startswith("dxa_")], len(set(only_state(store).blocks) - before)
