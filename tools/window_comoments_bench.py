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
                                           [--runs grouped,few,variance,control] [--modes ring,fallback]
"""
import torch

from window_bench import S, emit, lines, options, parse      # (first: it puts the repository on sys.path)

from dxa.engine.column import PrimColumn, Table
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


def main():
    args, dev = parse(options(batches=160, rows=200_000, panes=60, tail=100, runs="grouped,few,variance,control"))
    for line in lines(args, dev, SQL, lambda name: batches(args.batches, args.rows, dev)):
        emit(line)


if __name__ == "__main__":
    main()
