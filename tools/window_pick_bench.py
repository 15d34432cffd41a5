"""first / last / max_by / min_by on the dense window ring: a windowed statement per batch, with and without the ring.

A ``--panes``-pane (default 300) sliding window at ``--rows`` rows per batch (default 20 K), device ids uniform over
``--groups`` ids (default 200 and 50 000), ``--batches`` batches (default 330: the window is full after panes + 2), and
the statements

* ``last``:    ``SELECT deviceId, last(temp) … GROUP BY deviceId``;
* ``max_by``:  ``SELECT deviceId, max_by(temp, ts) …``;
* ``both``:    ``last(temp), max_by(temp, ts), AVG(temp)``;
* ``control``: ``AVG(temp)`` alone — no pick: the statement whose time must not move.

Every statement runs twice: ``ring`` as the engine runs it, and ``fallback`` with the dense ring switched off for the
run (``window_dense.dense_answer`` answers None), which is the path the statement took before picks were eligible: the
pane partials for ``last`` (about panes / 16 block partials and the loose panes concatenated and re-grouped per
batch), the generic evaluator for ``max_by`` (the window materialised and sorted by (group, y) per batch).

One JSON line per run: the median per-batch time of the last ``--tail`` batches (device events after each batch, read
after a final synchronise), the wall time, and whether a dense state answered.  The script uses only ``WindowStore``
and ``run_sql``, so ``--runs control --modes ring`` runs on older trees too.

    python tools/window_pick_bench.py [--runs last,max_by,both,control] [--groups 200,50000] [--modes ring,fallback]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dxa.engine.column import PrimColumn, Table  # noqa: E402
from dxa.engine.expr import EvalContext  # noqa: E402
from dxa.engine.query import Catalog, run_sql  # noqa: E402
from dxa.engine.windows import TimeWindowConf, WindowStore  # noqa: E402

S = 1_000_000
SQL = {
    "last": "SELECT deviceId, last(temp) AS lt FROM W GROUP BY deviceId",
    "max_by": "SELECT deviceId, max_by(temp, ts) AS mt FROM W GROUP BY deviceId",
    "both": "SELECT deviceId, last(temp) AS lt, max_by(temp, ts) AS mt, AVG(temp) AS av FROM W GROUP BY deviceId",
    "control": "SELECT deviceId, AVG(temp) AS av FROM W GROUP BY deviceId",
}


def batches(nb, rows, groups, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    out = []
    for b in range(nb):
        T = (1000 + b) * S
        ids = torch.randint(0, groups, (rows,), generator=g, device=dev, dtype=torch.int64)
        ts = T - torch.randint(0, S - 1, (rows,), generator=g, device=dev, dtype=torch.int64)
        temp = torch.randint(-400, 1200, (rows,), generator=g, device=dev, dtype=torch.int64).to(torch.float64) / 8
        out.append((T, Table(["ts", "deviceId", "temp"],
                             [PrimColumn("timestamp", ts), PrimColumn("long", ids), PrimColumn("double", temp)], rows,
                             dev)))
    torch.cuda.synchronize(dev)
    return out


def stream(name, mode, data, groups, panes, tail, dev):
    from dxa.engine import window_dense
    real = window_dense.dense_answer
    if mode == "fallback":
        window_dense.dense_answer = lambda *a, **k: None
    try:
        nb = len(data)
        store = WindowStore(TimeWindowConf({"W": panes * S}, True, "ts", 2 * S, panes * S, False))
        ctx = EvalContext(now_us=0, device=dev)
        events = [torch.cuda.Event(enable_timing=True) for _ in range(nb + 1)]
        out_rows = 0
        t0 = time.perf_counter()
        events[0].record()
        for b, (T, tbl) in enumerate(data):
            views, _ = store.process(tbl, T, S)
            cat = Catalog()
            cat.register("W", views["W"])
            out_rows = run_sql(SQL[name], cat, ctx).length
            events[b + 1].record()
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t0
    finally:
        window_dense.dense_answer = real
    per_batch = [events[b].elapsed_time(events[b + 1]) for b in range(nb)]
    states = list(store.__dict__.get("_dense", {}).values())
    st = states[0] if states else None
    return {"run": name, "mode": mode, "groups": groups, "batches": nb, "rows_per_batch": data[0][1].length,
            "panes": panes, "median_ms_last": round(statistics.median(per_batch[-tail:]), 3),
            "wall_s": round(wall, 3), "rows_last": out_rows, "dense": bool(st is not None and not st.disabled),
            "disabled_reason": getattr(st, "disabled_reason", None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000, help="rows per batch")
    ap.add_argument("--groups", default="200,50000")
    ap.add_argument("--batches", type=int, default=330)
    ap.add_argument("--panes", type=int, default=300)
    ap.add_argument("--tail", type=int, default=20, help="batches at the end whose median is reported")
    ap.add_argument("--runs", default="last,max_by,both,control")
    ap.add_argument("--modes", default="ring,fallback")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_pick_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    for groups in map(int, args.groups.split(",")):
        data = batches(args.batches, args.rows, groups, dev)
        for name in args.runs.split(","):
            for mode in args.modes.split(","):
                print(json.dumps(stream(name, mode, data, groups, args.panes, min(args.tail, args.batches), dev)),
                      flush=True)


if __name__ == "__main__":
    main()
