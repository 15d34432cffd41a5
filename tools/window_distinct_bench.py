"""Per-batch time of windowed statements with COUNT(DISTINCT x).

A 60-pane sliding window (60 s window, 2 s watermark, 1 s batches) at 200 K rows per batch, 160 batches; ids uniform
over a fixed set of 10 K, ``kind`` over 16 values, ``minute`` over about 60 values per window.  Two statements:

* ``grouped``: ``SELECT deviceId, COUNT(DISTINCT kind), SUM(temp) … GROUP BY deviceId`` (160 K live pairs);
* ``global``:  ``SELECT COUNT(DISTINCT minute), MAX(ts) … WHERE temp > 8`` (the reference IoT sample's shape: every
  pair under one group).

Prints one JSON line per run: the median per-batch time of the last 100 batches (device events recorded after each
batch, read after a final synchronise; a batch ends in the statement's status read or result length, so the gap
between two events is the batch's wall time), the whole run's wall time, whether a dense state answered, and its
pair capacity and rebuild counts.  Uses only ``WindowStore``, ``run_sql`` and synthetic device batches, so the same
file runs on older trees (where the statements take the generic path and no dense state exists: nulls).

    python tools/window_distinct_bench.py [--batches 160] [--rows 200000] [--panes 60] [--modes ring,fallback]
"""
import torch

from window_bench import S, emit, lines, options, parse      # (first: it puts the repository on sys.path)

from dxa.engine.column import PrimColumn, Table

SQL = {
    "grouped": "SELECT deviceId, COUNT(DISTINCT kind) AS dk, SUM(temp) AS s FROM W GROUP BY deviceId",
    "global": "SELECT COUNT(DISTINCT minute) AS minutes, MAX(ts) AS last FROM W WHERE temp > 8",
}


def batches(nb, rows, panes, dev):
    """The run's batches, generated on the device before anything is timed."""
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    out = []
    for b in range(nb):
        T = (1000 + b) * S
        ids = torch.randint(0, 10_000, (rows,), generator=g, device=dev, dtype=torch.int64)
        ts = T - torch.randint(0, S - 1, (rows,), generator=g, device=dev, dtype=torch.int64)
        temp = torch.randint(0, 256, (rows,), generator=g, device=dev, dtype=torch.int64).to(torch.float64) * 0.25
        kind = torch.randint(0, 16, (rows,), generator=g, device=dev, dtype=torch.int64)
        minute = torch.div(ts, max(1, panes // 60) * S, rounding_mode="floor")     # ~60 values per window
        out.append((T, Table(["ts", "deviceId", "kind", "minute", "temp"],
                             [PrimColumn("timestamp", ts), PrimColumn("long", ids), PrimColumn("long", kind),
                              PrimColumn("long", minute), PrimColumn("double", temp)], rows, dev)))
    torch.cuda.synchronize(dev)
    return out


def main():
    args, dev = parse(options(batches=160, rows=200_000, panes=60, tail=100, runs="grouped,global"))
    for line in lines(args, dev, SQL, lambda name: batches(args.batches, args.rows, args.panes, dev)):
        emit(line)


if __name__ == "__main__":
    main()
