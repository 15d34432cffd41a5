"""COUNT / MAX over a string argument on the dense window ring: a windowed statement per batch, with and without the ring.

A ``--panes``-pane (default 300) sliding window at ``--rows`` rows per batch (default 20 K), device ids uniform over
``--groups`` ids (default 200 and 50 000), ``--batches`` batches (default 330: the window is full after panes + 2), a
string column ``name`` of 8-40 bytes drawn from 4,096 different values, and the statements

* ``max``:     ``SELECT deviceId, MAX(name) … GROUP BY deviceId``;
* ``count``:   ``SELECT deviceId, COUNT(name) …``;
* ``both``:    ``MAX(name), COUNT(name), AVG(temp)``;
* ``control``: ``AVG(temp)`` alone — no string argument: the statement whose time must not move.

Every statement runs twice: ``ring`` as the engine runs it, and ``fallback`` with the dense ring switched off for the
run (``window_dense.dense_answer`` answers None), which is the path the statement took before string arguments were
eligible: the pane partials (about panes / 16 block partials and the loose panes concatenated and re-grouped per batch),
with ``groupby.aggregate``'s MIN / MAX over strings per pane and per merge.

One JSON line per run: the median per-batch time of the last ``--tail`` batches (device events after each batch, read
after a final synchronise), the wall time, and whether a dense state answered.  The script uses only ``WindowStore``
and ``run_sql``, so it runs on older trees too.

    python tools/window_strings_bench.py [--runs max,count,both,control] [--groups 200,50000] [--modes ring,fallback]
"""
import torch

from window_bench import S, emit, lines, options, parse      # (first: it puts the repository on sys.path)

from dxa.engine.column import PrimColumn, Table, strings_from_pylist

SQL = {
    "max": "SELECT deviceId, MAX(name) AS mx FROM W GROUP BY deviceId",
    "count": "SELECT deviceId, COUNT(name) AS cn FROM W GROUP BY deviceId",
    "both": "SELECT deviceId, MAX(name) AS mx, COUNT(name) AS cn, AVG(temp) AS av FROM W GROUP BY deviceId",
    "control": "SELECT deviceId, AVG(temp) AS av FROM W GROUP BY deviceId",
}
POOL = 4096


def batches(nb, rows, groups, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    pool = strings_from_pylist([f"fw-{k * 2654435761 % 1000003:07d}" + "-abcdefghijklmnopqrstuvwxyz0123"[:k % 31]
                                for k in range(POOL)], "cpu").to(dev)
    out = []
    for b in range(nb):
        T = (1000 + b) * S
        ids = torch.randint(0, groups, (rows,), generator=g, device=dev, dtype=torch.int64)
        ts = T - torch.randint(0, S - 1, (rows,), generator=g, device=dev, dtype=torch.int64)
        temp = torch.randint(-400, 1200, (rows,), generator=g, device=dev, dtype=torch.int64).to(torch.float64) / 8
        name = pool.take(torch.randint(0, POOL, (rows,), generator=g, device=dev, dtype=torch.int64)).compact()
        out.append((T, Table(["ts", "deviceId", "temp", "name"],
                             [PrimColumn("timestamp", ts), PrimColumn("long", ids), PrimColumn("double", temp), name],
                             rows, dev)))
    torch.cuda.synchronize(dev)
    return out


def main():
    ap = options(batches=330, rows=20_000, panes=300, tail=20, runs="max,count,both,control", modes="ring,fallback")
    ap.add_argument("--groups", default="200,50000")
    args, dev = parse(ap)
    for groups in map(int, args.groups.split(",")):
        data = batches(args.batches, args.rows, groups, dev)
        for line in lines(args, dev, SQL, lambda name: data, groups=groups):
            emit(line)


if __name__ == "__main__":
    main()
