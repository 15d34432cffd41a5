"""Per-batch time of windowed statements with CORR, SKEWNESS and KURTOSIS.

The stream of tools/window_moments_bench.py with a second measurement ``hum``: a 60-pane sliding window (60 s window,
2 s watermark, 1 s batches) at 200 K rows per batch, 160 batches; ids uniform over a fixed set of 10 K, ``kind`` over
16 values.  Four statements:

* ``grouped``:  ``SELECT deviceId, AVG(temp), corr(temp, hum), skewness(temp), kurtosis(temp) … GROUP BY deviceId``
  (10 K groups);
* ``few``:      the same ``… GROUP BY kind`` (16 groups: every row of a pane lands on 16 rows of words, the contended
  shape of the pane's second passes);
* ``variance``: window_moments_bench.py's ``grouped`` statement (AVG and STDDEV by deviceId: nothing in it is new);
* ``control``:  AVG only.

Prints one JSON line per run: the median per-batch time of the last 100 batches (device events recorded after each
batch, read after a final synchronise; a batch ends in the statement's status read or result length, so the gap
between two events is the batch's wall time), the whole run's wall time, and whether a dense state answered.  Uses
only ``WindowStore``, ``run_sql`` and synthetic device batches, so the same file runs on older trees (where the first
two statements re-group the materialised window every batch: ``dense`` false, no state at all).

    python tools/window_comoments_bench.py [--batches 160] [--rows 200000] [--panes 60]
                                           [--runs grouped,few,variance,control]
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
_NEW = "AVG(temp) AS av, corr(temp, hum) AS cr, skewness(temp) AS sk, kurtosis(temp) AS ku"
SQL = {
    "grouped": f"SELECT deviceId, {_NEW} FROM W GROUP BY deviceId",
    "few": f"SELECT kind, {_NEW} FROM W GROUP BY kind",
    "variance": "SELECT deviceId, AVG(temp) AS av, STDDEV(temp) AS sd FROM W GROUP BY deviceId",
    "control": "SELECT deviceId, AVG(temp) AS av FROM W GROUP BY deviceId",
}


def batches(nb, rows, dev):
    """The run's batches, generated on the device before anything is timed (window_moments_bench.py's draws, then
    ``hum``: half of ``temp`` rounded down to a multiple of 0.25 plus a uniform multiple of 0.25 below 32)."""
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    out = []
    for b in range(nb):
        T = (1000 + b) * S
        ids = torch.randint(0, 10_000, (rows,), generator=g, device=dev, dtype=torch.int64)
        ts = T - torch.randint(0, S - 1, (rows,), generator=g, device=dev, dtype=torch.int64)
        temp = torch.randint(0, 256, (rows,), generator=g, device=dev, dtype=torch.int64).to(torch.float64) * 0.25
        kind = torch.randint(0, 16, (rows,), generator=g, device=dev, dtype=torch.int64)
        noise = torch.randint(0, 128, (rows,), generator=g, device=dev, dtype=torch.int64).to(torch.float64) * 0.25
        hum = torch.floor(temp * 2) * 0.25 + noise
        out.append((T, Table(["ts", "deviceId", "kind", "temp", "hum"],
                             [PrimColumn("timestamp", ts), PrimColumn("long", ids), PrimColumn("long", kind),
                              PrimColumn("double", temp), PrimColumn("double", hum)], rows, dev)))
    torch.cuda.synchronize(dev)
    return out


def run(name, nb, rows, panes, tail, dev):
    data = batches(nb, rows, dev)
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
    return {"run": name, "batches": nb, "rows_per_batch": rows, "panes": panes,
            "median_ms_last": round(statistics.median(per_batch[-tail:]), 3),
            "wall_s": round(wall, 3), "rows_last": out_rows,
            "dense": bool(st is not None and not st.disabled),
            "rebuilds": getattr(st, "rebuilds", None), "gcap": getattr(st, "gcap", None),
            "disabled_reason": getattr(st, "disabled_reason", None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=160)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--panes", type=int, default=60)
    ap.add_argument("--tail", type=int, default=100, help="batches at the end whose median is reported")
    ap.add_argument("--runs", default="grouped,few,variance,control")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_comoments_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    for name in args.runs.split(","):
        print(json.dumps(run(name, args.batches, args.rows, args.panes, min(args.tail, args.batches), dev)),
              flush=True)


if __name__ == "__main__":
    main()
