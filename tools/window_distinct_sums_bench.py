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
                                               [--modes ring,fallback]
"""
import torch

from window_bench import S, emit, lines, options, parse      # (first: it puts the repository on sys.path)

from dxa.engine.column import PrimColumn, Table

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


def main():
    ap = options(batches=330, rows=20_000, panes=300, tail=20, runs="sums,count")
    ap.add_argument("--values", type=int, default=16, help="distinct values of x")
    args, dev = parse(ap)
    for line in lines(args, dev, SQL, lambda name: batches(args.batches, args.rows, args.values, dev),
                      values=args.values):
        emit(line)


if __name__ == "__main__":
    main()
