"""Time percentile / percentile_approx over window frames: one statement over seeded rows on cuda:0, per path.

    python tools/window_percentile_bench.py --rows 1000000 --partitions 1000 \
        --frame 4,8,16,32,64,256,1024,running --path direct,tree,tensor

``--frame N`` is ``ROWS BETWEEN N-1 PRECEDING AND CURRENT ROW`` (N rows), ``running`` the default frame of an ordered
window.  ``--call`` picks the call shapes: ``median`` is ``percentile(v, 0.5)`` (2 ranks), ``three`` is
``percentile(v, array(0.5, 0.95, 0.99))`` (6 ranks), ``approx`` is ``percentile_approx(v, 0.95)`` (1 rank).
``--path`` pins how ``windowfn`` selects: ``direct`` and ``tree`` are the two entry points of
``ops/csrc/window_select.hip`` (``FRAME_SELECT_DIRECT_MAX`` set above / below every frame), ``tensor`` the
tensor-operation wavelet matrix on the same device (``_frame_select_tensor``), ``auto`` the engine's own choice.  The
direct entry is quadratic in the frame length, so frames longer than ``--direct-cap`` rows are not run through it.
The paths of one shape are alternated, after ``--warmup`` unmeasured rounds, and every call is timed with device
events around a synchronise: ``stmt_ms`` is the whole statement (partition ids, sort, frame bounds, selection, gather,
scatter), ``select_ms`` the selection primitive alone, and for ``tree`` ``build_ms`` (radix sort, prefix counts and
scatters of the wavelet matrix) and ``query_ms`` (the one query launch).  One JSON line per (call, frame, path):
medians, and the min / max of the repeats as the spread."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dxa.engine import windowfn as W  # noqa: E402
from dxa.engine.column import PrimColumn, Table  # noqa: E402
from dxa.engine.expr import EvalContext  # noqa: E402
from dxa.engine.query import Catalog, run_sql  # noqa: E402

CALLS = {"median": "percentile(v, 0.5)", "three": "percentile(v, array(0.5, 0.95, 0.99))",
         "approx": "percentile_approx(v, 0.95)"}


def table(rows, partitions, seed, dev):
    """id 0 .. rows-1, k one of ``partitions`` keys, v a multiple of 0.25 in [0, 64) (skewed), 10 % NULLs."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, partitions, (rows,), generator=g)
    v = torch.floor(256 * torch.rand(rows, generator=g, dtype=torch.float64) ** 2) / 4
    ok = torch.rand(rows, generator=g) > 0.1
    cols = [PrimColumn("long", torch.arange(rows)), PrimColumn("long", k), PrimColumn("double", v, ok)]
    return Table(["id", "k", "v"], [c.to(dev) for c in cols], rows, dev)


def statement(call, frame):
    spec = "" if frame == "running" else f" ROWS BETWEEN {int(frame) - 1} PRECEDING AND CURRENT ROW"
    return f"SELECT id, {CALLS[call]} OVER (PARTITION BY k ORDER BY id{spec}) AS x FROM T"


def _timed(fn, marks):
    def wrapper(*a, **kw):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn(*a, **kw)
        t1.record()
        marks.append((t0, t1))
        return out
    return wrapper


def timed_call(sql, cat, ctx, path, dev):
    """One call of ``sql`` with the selection taken by ``path`` → dict of milliseconds."""
    real = (W._frame_select, W._wavelet_build, W._frame_select_tree, W.FRAME_SELECT_DIRECT_MAX)
    select, build, query = [], [], []
    if path == "tensor":
        def inner(key, valid, vz, a, b, ranks, maxlen):
            return W._frame_select_tensor(key, valid, vz, a, b, ranks)
    else:
        inner = real[0]
    W._frame_select = _timed(inner, select)
    W._wavelet_build = _timed(real[1], build)
    W._frame_select_tree = _timed(real[2], query)
    if path in ("direct", "tree"):
        W.FRAME_SELECT_DIRECT_MAX = 1 << 62 if path == "direct" else 0
    try:
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = run_sql(sql, cat, ctx)
        col = out.columns[1]                                 # the window column is materialised
        _ = col.elements[0].data if hasattr(col, "elements") else col.data
        t1.record()
        torch.cuda.synchronize(dev)
    finally:
        W._frame_select, W._wavelet_build, W._frame_select_tree, W.FRAME_SELECT_DIRECT_MAX = real

    def total(marks):
        return sum(s.elapsed_time(e) for s, e in marks)
    t = {"stmt_ms": t0.elapsed_time(t1), "select_ms": total(select)}
    if build or query:
        t["build_ms"], t["query_ms"] = total(build), total(query)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--partitions", type=int, default=1000)
    ap.add_argument("--frame", default="64", help="comma list of frame lengths in rows, or 'running'")
    ap.add_argument("--call", default="median,three,approx", help="comma list of " + ", ".join(CALLS))
    ap.add_argument("--path", default="direct,tree,tensor", help="comma list of direct, tree, tensor, auto")
    ap.add_argument("--direct-cap", type=int, default=256, help="longest frame (rows) run through the direct entry")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_percentile_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    cat = Catalog()
    cat.register("T", table(args.rows, args.partitions, args.seed, dev))
    ctx = EvalContext(now_us=0, device=dev)
    for call in args.call.split(","):
        for frame in args.frame.split(","):
            sql = statement(call, frame)
            paths = [p for p in args.path.split(",")
                     if p != "direct" or (frame != "running" and int(frame) <= args.direct_cap)]
            times = {p: [] for p in paths}
            for r in range(args.warmup + args.repeats):
                for p in paths:                                # alternated: every round takes each path once
                    t = timed_call(sql, cat, ctx, p, dev)
                    if r >= args.warmup:
                        times[p].append(t)
            for p in paths:
                line = {"call": call, "frame": frame, "path": p, "rows": args.rows, "partitions": args.partitions,
                        "repeats": args.repeats}
                for what in times[p][0]:
                    vals = [t[what] for t in times[p]]
                    stem = what[:-3]
                    line[what] = round(statistics.median(vals), 4)
                    line[stem + "_min_ms"] = round(min(vals), 4)
                    line[stem + "_max_ms"] = round(max(vals), 4)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
