"""Per-batch time of windowed statements with STDDEV.

The stream of tools/window_distinct_bench.py: a 60-pane sliding window (60 s window, 2 s watermark, 1 s batches) at
200 K rows per batch, 160 batches; ids uniform over a fixed set of 10 K, ``kind`` over 16 values.  Three statements:

* ``grouped``: ``SELECT deviceId, AVG(temp), STDDEV(temp) … GROUP BY deviceId`` (10 K groups: the z-score alert);
* ``few``:     the same ``… GROUP BY kind`` (16 groups: every row of a pane lands on 16 M2 words, the contended shape
  of win_m2_kernel);
* ``control``: the grouped statement without STDDEV (nothing in it is new).

Prints one JSON line per run: the median per-batch time of the last 100 batches (device events recorded after each
batch, read after a final synchronise; a batch ends in the statement's status read or result length, so the gap
between two events is the batch's wall time), the whole run's wall time, and whether a dense state answered.  Uses
only ``WindowStore``, ``run_sql`` and synthetic device batches, so the same file runs on older trees (where the
STDDEV statements take the paned path: ``dense`` false, ``disabled_reason`` "stddev").

    python tools/window_moments_bench.py [--batches 160] [--rows 200000] [--panes 60] [--runs grouped,few,control]
                                         [--modes ring,fallback]
"""
import torch

from window_bench import S, emit, lines, options, parse      # (first: it puts the repository on sys.path)

from dxa.engine.column import PrimColumn, Table

SQL = {
    "grouped": "SELECT deviceId, AVG(temp) AS av, STDDEV(temp) AS sd FROM W GROUP BY deviceId",
    "few": "SELECT kind, AVG(temp) AS av, STDDEV(temp) AS sd FROM W GROUP BY kind",
    "control": "SELECT deviceId, AVG(temp) AS av FROM W GROUP BY deviceId",
}


def batches(nb, rows, dev):
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
        out.append((T, Table(["ts", "deviceId", "kind", "temp"],
                             [PrimColumn("timestamp", ts), PrimColumn("long", ids), PrimColumn("long", kind),
                              PrimColumn("double", temp)], rows, dev)))
    torch.cuda.synchronize(dev)
    return out


def main():
    args, dev = parse(options(batches=160, rows=200_000, panes=60, tail=100, runs="grouped,few,control"))
    for line in lines(args, dev, SQL, lambda name: batches(args.batches, args.rows, dev)):
        emit(line)


if __name__ == "__main__":
    main()
