"""The driver the tools/window_*_bench.py scripts share: their common options, the one timed loop, and the result line.

A script holds its synthetic schema (``batches``), its statements (``SQL``), its defaults and any option of its own; it
gets its parser from ``options``, parses with ``parse`` (which exits when there is no GPU) and prints ``lines``.  The
timed loop uses only ``WindowStore``, ``run_sql`` and the batches it is given, so a script runs on older trees too
(where a statement the ring does not answer reports ``dense`` false, and a state without an attribute reports null).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dxa.engine.expr import EvalContext  # noqa: E402
from dxa.engine.query import Catalog, run_sql  # noqa: E402
from dxa.engine.windows import TimeWindowConf, WindowStore  # noqa: E402

S = 1_000_000


def options(batches, rows, panes, tail, runs, modes="ring"):
    """The parser with the options every script has, at the script's defaults."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=batches)
    ap.add_argument("--rows", type=int, default=rows, help="rows per batch")
    ap.add_argument("--panes", type=int, default=panes)
    ap.add_argument("--tail", type=int, default=tail, help="batches at the end whose median is reported")
    ap.add_argument("--runs", default=runs)
    ap.add_argument("--modes", default=modes, help="ring: as the engine runs the statement; fallback: with the dense "
                                                   "ring switched off for the run")
    return ap


def parse(ap):
    """→ (the arguments, ``--tail`` capped at ``--batches``; cuda:0), or exit when there is no GPU."""
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit(f"{os.path.basename(sys.argv[0])} measures on a GPU; none found")
    args.tail = min(args.tail, args.batches)
    return args, torch.device("cuda", 0)


def timed_stream(sql, data, panes, tail, dev, mode="ring"):
    """Statement ``sql`` over a ``panes``-second sliding window (2 s watermark, 1 s batches) after each of ``data``'s
    (batch time, device table) batches.  A device event is recorded after each batch and read after a final
    synchronise; a batch ends in the statement's status read or result length, so the gap between two events is the
    batch's wall time.  ``mode="fallback"`` switches the dense ring off for the run (``window_dense.dense_answer``
    answers None), so the statement takes the path it took before the ring answered it.  → the result line: the
    median per-batch time of the last ``tail`` batches, the run's wall time, the last result's length, and the dense
    state's condition (``dense`` false when there is none)."""
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
            out_rows = run_sql(sql, cat, ctx).length
            events[b + 1].record()
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t0
    finally:
        window_dense.dense_answer = real
    per_batch = [events[b].elapsed_time(events[b + 1]) for b in range(nb)]
    states = list(store.__dict__.get("_dense", {}).values())
    st = states[0] if states else None
    pairs = list(getattr(st, "pairs", None) or [])
    return {"mode": mode, "batches": nb, "rows_per_batch": data[0][1].length, "panes": panes,
            "median_ms_last": round(statistics.median(per_batch[-tail:]), 3), "wall_s": round(wall, 3),
            "rows_last": out_rows, "dense": bool(st is not None and not st.disabled),
            **({"pcap": [p.pcap for p in pairs], "pair_rebuilds": [p.rebuilds for p in pairs]} if pairs else {}),
            "rebuilds": getattr(st, "rebuilds", None), "gcap": getattr(st, "gcap", None),
            "disabled_reason": getattr(st, "disabled_reason", None)}


def lines(args, dev, sql, data_of, **labels):
    """The result line of every (run, mode) of ``--runs`` × ``--modes``, labelled with the run's name and ``labels``;
    ``data_of(run)`` makes the run's batches, once for all its modes."""
    for name in args.runs.split(","):
        data = data_of(name)
        for mode in args.modes.split(","):
            yield {"run": name, **labels, **timed_stream(sql[name], data, args.panes, args.tail, dev, mode)}


def emit(line):
    print(json.dumps(line), flush=True)
