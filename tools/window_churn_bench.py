"""Per-batch time of a windowed GROUP BY whose keys come and go, against one whose keys stay.

A 60-pane sliding window (60 s window, 2 s watermark, 1 s batches) at 200 K rows per batch, 160 batches, twice:

* ``fixed``: ids uniform over a fixed set of 10 K;
* ``drift``: ids uniform over [2000 b, 2000 b + 10000) for batch b, so the stream passes 65,536 distinct ids after
  about 30 batches and the window holds about 130 K at a time.

Prints one JSON line per run: the median per-batch time of the last 100 batches (device events recorded after each
batch, read after a final synchronise; a batch ends in the statement's status read, so the gap between two events
is the batch's wall time), the whole run's wall time, and the dense state's ``rebuilds`` / capacity / whether it is
still enabled.  Uses only ``WindowStore``, ``run_sql`` and synthetic device batches, so the same file runs on older
trees (where the state has no ``rebuilds``: printed as null).

    python tools/window_churn_bench.py [--batches 160] [--rows 200000] [--panes 60] [--runs fixed,drift]
                                       [--modes ring,fallback]
"""
import torch

from window_bench import S, emit, lines, options, parse      # (first: it puts the repository on sys.path)

from dxa.engine.column import PrimColumn, Table

SQL = ("SELECT deviceId, COUNT(*) AS c, SUM(temp) AS s, MIN(temp) AS mn, MAX(temp) AS mx, AVG(temp) AS av "
       "FROM W GROUP BY deviceId")


def batches(kind, nb, rows, dev):
    """The run's batches, generated on the device before anything is timed."""
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    out = []
    for b in range(nb):
        T = (1000 + b) * S
        lo = 2000 * b if kind == "drift" else 0
        ids = torch.randint(lo, lo + 10_000, (rows,), generator=g, device=dev, dtype=torch.int64)
        ts = T - torch.randint(0, S - 1, (rows,), generator=g, device=dev, dtype=torch.int64)
        temp = torch.randint(0, 256, (rows,), generator=g, device=dev, dtype=torch.int64).to(torch.float64) * 0.25
        out.append((T, Table(["ts", "deviceId", "temp"], [PrimColumn("timestamp", ts), PrimColumn("long", ids),
                                                         PrimColumn("double", temp)], rows, dev)))
    torch.cuda.synchronize(dev)
    return out


def main():
    args, dev = parse(options(batches=160, rows=200_000, panes=60, tail=100, runs="fixed,drift"))
    for line in lines(args, dev, dict.fromkeys(("fixed", "drift"), SQL),
                      lambda kind: batches(kind, args.batches, args.rows, dev)):
        line["groups_last"] = line.pop("rows_last")
        emit(line)


if __name__ == "__main__":
    main()
