"""Decimal aggregates on the dense window ring: the pane's decimal pass alone, and a windowed statement per batch.

``--mode kernels`` (this tree only): one pane of ``--rows`` rows (default 1 M), group ids uniform over ``--groups``
ids (16: every id below the LDS bound; 100 000: nearly every id above it, global adds), one SUM argument.  Times

* ``dec_narrow`` / ``dec_wide``: ``dxa_win_dec`` with one DEC_SUM job over a one-lane / two-lane decimal column;
* ``multi_f64``: ``dxa_aggregate_multi`` with one f64 SUM slot over the same group ids (its launch includes the
  slot's initialisation, as in the ring), the cost of a double SUM on the same pane.

Each figure is the time between two device events around ``--reps`` back-to-back launches on one stream, divided by
``--reps``, after ``--warmup`` launches; one JSON line per (groups, kernel).

``--mode stream``: tools/window_comoments_bench.py's stream with a long ``temp``: a 60-pane sliding window at 200 K
rows per batch over 10 K ids, 160 batches, and the statements

* ``decimal``: ``SELECT deviceId, AVG(temp * 1.8 + 32) … GROUP BY deviceId`` (the argument is decimal(24,1); the
  product of a decimal(20,0) and a literal is evaluated row by row on the host, in every tree);
* ``narrow``:  ``AVG(CAST(temp AS DECIMAL(18,2)))`` — a one-lane argument evaluated on the device;
* ``wide``:    ``AVG(CAST(temp AS DECIMAL(24,1))), MAX(CAST(temp AS DECIMAL(24,1)))`` — a two-lane one, likewise;
* ``control``: ``AVG(temp)`` over the long itself.

One JSON line per run: the median per-batch time of the last 100 batches (device events after each batch, read after
a final synchronise), whether a dense state answered, and under ``path`` the ``--modes`` entry (ring or fallback; the
line's ``mode`` is this script's own).  This mode uses only ``WindowStore`` and ``run_sql``, so the
same file runs on older trees (where ``decimal`` is answered by the paned path: ``dense`` false, "argument type").

    python tools/window_decimal_bench.py --mode kernels [--rows 1000000] [--groups 16,100000]
    python tools/window_decimal_bench.py --mode stream [--runs decimal,control] [--modes ring,fallback]
"""
import ctypes

import torch

from window_bench import S, emit, lines, options, parse      # (first: it puts the repository on sys.path)

from dxa.engine.column import PrimColumn, Table

SQL = {
    "decimal": "SELECT deviceId, AVG(temp * 1.8 + 32) AS av FROM W GROUP BY deviceId",
    "narrow": "SELECT deviceId, AVG(CAST(temp AS DECIMAL(18,2))) AS av FROM W GROUP BY deviceId",
    "wide": ("SELECT deviceId, AVG(CAST(temp AS DECIMAL(24,1))) AS av, MAX(CAST(temp AS DECIMAL(24,1))) AS mx "
             "FROM W GROUP BY deviceId"),
    "control": "SELECT deviceId, AVG(temp) AS av FROM W GROUP BY deviceId",
}


def _timed(launch, warmup, reps, dev):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        launch()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def kernels(rows, groups, warmup, reps, dev):
    from dxa.engine import window_dense as W
    from dxa.ops import native as N
    from dxa.ops.groupby import _DEC_SUM, _MA_ADD_F64, _MV_F64
    W._sizes()
    g = torch.Generator(device=dev)
    g.manual_seed(19)
    st = N.stream_handle(dev)
    stride = 8
    gcap = max(groups, 1 << 10)
    gid = torch.randint(0, groups, (rows,), generator=g, device=dev, dtype=torch.int64).to(torch.int32)
    narrow = torch.randint(-10 ** 17, 10 ** 17, (rows,), generator=g, device=dev, dtype=torch.int64)
    wide = torch.stack([narrow * 7 + 3, torch.randint(-5 * 10 ** 8, 5 * 10 ** 8, (rows,), generator=g, device=dev,
                                                      dtype=torch.int64)], 1).contiguous()
    f64 = narrow.to(torch.float64)
    row = torch.zeros((gcap + 1) * stride, dtype=torch.int64, device=dev)
    out = []

    def dec(col):
        m = W._DecArgs()
        m.a[0] = W._DecJob(col.data_ptr(), 0, col.dim(), _DEC_SUM, 0, 1, 2, 0)
        m.gid, m.row, m.n = gid.data_ptr(), row.data_ptr(), rows
        m.gcap, m.stride, m.nargs = gcap, stride, 1
        return lambda: N.call("dxa_win_dec", ctypes.addressof(m), st)

    spec = torch.tensor([f64.data_ptr(), 0, _MV_F64], dtype=torch.int64)
    ops = torch.tensor([_MA_ADD_F64], dtype=torch.int32)

    def multi():
        N.call("dxa_aggregate_multi", N.ptr(gid), rows, gcap + 1, 1, spec.data_ptr(), 1, ops.data_ptr(), N.ptr(row), st)

    for name, launch in (("dec_narrow", dec(narrow)), ("dec_wide", dec(wide)), ("multi_f64", multi)):
        out.append({"mode": "kernels", "kernel": name, "rows": rows, "groups": groups, "reps": reps,
                    "ms_per_launch": round(_timed(launch, warmup, reps, dev), 4)})
    # the limb sums of the last timed series against torch's: warmup + reps launches of the wide column after zeroing
    row.zero_()
    dec(wide)()
    torch.cuda.synchronize(dev)
    want = torch.zeros(gcap + 1, dtype=torch.int64, device=dev).index_add_(0, gid.to(torch.int64), wide[:, 1])
    assert torch.equal(row.view(gcap + 1, stride)[:, 2], want), "win_dec_kernel's high limb sums differ from torch's"
    return out


def batches(nb, rows, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    out = []
    for b in range(nb):
        T = (1000 + b) * S
        ids = torch.randint(0, 10_000, (rows,), generator=g, device=dev, dtype=torch.int64)
        ts = T - torch.randint(0, S - 1, (rows,), generator=g, device=dev, dtype=torch.int64)
        temp = torch.randint(-40, 120, (rows,), generator=g, device=dev, dtype=torch.int64)
        out.append((T, Table(["ts", "deviceId", "temp"],
                             [PrimColumn("timestamp", ts), PrimColumn("long", ids), PrimColumn("long", temp)], rows,
                             dev)))
    torch.cuda.synchronize(dev)
    return out


def main():
    ap = options(batches=160, rows=None, panes=60, tail=100, runs="decimal,control")
    ap.add_argument("--mode", choices=("kernels", "stream"), required=True)
    ap.add_argument("--groups", default="16,100000")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    args, dev = parse(ap)           # --rows: per pane (kernels: 1 M by default) or per batch (stream: 200 K)
    if args.mode == "kernels":
        for groups in map(int, args.groups.split(",")):
            for line in kernels(args.rows or 1_000_000, groups, args.warmup, args.reps, dev):
                emit(line)
        return
    for line in lines(args, dev, SQL, lambda name: batches(args.batches, args.rows or 200_000, dev)):
        emit({"mode": "stream", "path": line.pop("mode"), **line})


if __name__ == "__main__":
    main()
