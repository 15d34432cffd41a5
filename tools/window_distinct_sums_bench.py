"""Per-batch time of windowed statements with SUM / AVG / COUNT(DISTINCT x).

A 300-pane sliding window (300 s window, 2 s watermark, 1 s batches) at 20 K rows per batch, 330 batches (the window
is full after 302); ids uniform over a fixed set of 10 K — the flagship window flow's group count —, ``x`` a long
over 16 values (160 K live pairs).  Two statements, both ``GROUP BY deviceId``:

* ``sums``:  ``SUM(DISTINCT x), AVG(DISTINCT x), COUNT(DISTINCT x)``;
* ``count``: ``COUNT(DISTINCT x)`` alone (the control: its fold is the instantiation without the value adds).

Prints one JSON line per run: the median per-batch time of the last 20 batches (device events recorded after each
batch, read after a final synchronise; a batch ends in the statement's status read or result length, so the gap
between two events is the batch's wall time), the whole run's wall time, whether a dense state answered, and its
pair capacity and rebuild counts.  Uses only ``WindowStore``, ``run_sql`` and synthetic device batches, so the same
file runs on older trees (where ``sums`` takes the generic path and no dense state exists: nulls).

    python tools/window_distinct_sums_bench.py [--batches 330] [--rows 20000] [--panes 300] [--values 16]
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
    "sums": "SELECT deviceId, SUM(DISTINCT x) AS sx, AVG(DISTINCT x) AS ax, COUNT(DISTINCT x) AS dx FROM W "
            "GROUP BY deviceId",
    "count": "SELECT deviceId, COUNT(DISTINCT x) AS dx FROM W GROUP BY deviceId",
}


def batches(nb, rows, values, dev):
    """The run's batches, generated on the device before anything is timed."""
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    out = []
    for b in range(nb):
        T = (1000 + b) * S
        ids = torch.randint(0, 10_000, (rows,), generator=g, device=dev, dtype=torch.int64)
        ts = T - torch.randint(0, S - 1, (rows,), generator=g, device=dev, dtype=torch.int64)
        x = torch.randint(0, values, (rows,), generator=g, device=dev, dtype=torch.int64) * 3 - 7
        out.append((T, Table(["ts", "deviceId", "x"],
                             [PrimColumn("timestamp", ts), PrimColumn("long", ids), PrimColumn("long", x)], rows, dev)))
    torch.cuda.synchronize(dev)
    return out


def run(name, nb, rows, panes, values, tail, dev):
    data = batches(nb, rows, values, dev)
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
    per_batch = [events[b].elapsed_time(events[b + 1]) for b in range(nb)]
    states = list(store.__dict__.get("_dense", {}).values())
    st = states[0] if states else None
    pairs = list(getattr(st, "pairs", None) or [])
    return {"run": name, "batches": nb, "rows_per_batch": rows, "panes": panes, "values": values,
            "median_ms_last": round(statistics.median(per_batch[-tail:]), 3),
            "wall_s": round(wall, 3), "rows_last": out_rows,
            "dense": bool(st is not None and not st.disabled),
            "pcap": [p.pcap for p in pairs] or None, "pair_rebuilds": [p.rebuilds for p in pairs] or None,
            "rebuilds": getattr(st, "rebuilds", None), "gcap": getattr(st, "gcap", None),
            "disabled_reason": getattr(st, "disabled_reason", None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=330)
    ap.add_argument("--rows", type=int, default=20_000)
    ap.add_argument("--panes", type=int, default=300)
    ap.add_argument("--values", type=int, default=16, help="distinct values of x")
    ap.add_argument("--tail", type=int, default=20, help="batches at the end whose median is reported")
    ap.add_argument("--runs", default="sums,count")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_distinct_sums_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    for name in args.runs.split(","):
        print(json.dumps(run(name, args.batches, args.rows, args.panes, args.values, min(args.tail, args.batches),
                             dev)), flush=True)


if __name__ == "__main__":
    main()
