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
import torch

from window_bench import S, emit, lines, options, parse      # (first: it puts the repository on sys.path)

from dxa.engine.column import PrimColumn, Table

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


def main():
    ap = options(batches=330, rows=20_000, panes=300, tail=20, runs="last,max_by,both,control", modes="ring,fallback")
    ap.add_argument("--groups", default="200,50000")
    args, dev = parse(ap)
    for groups in map(int, args.groups.split(",")):
        data = batches(args.batches, args.rows, groups, dev)
        for line in lines(args, dev, SQL, lambda name: data, groups=groups):
            emit(line)


if __name__ == "__main__":
    main()
