"""Time a variance / moment window aggregate over frames: one statement over seeded rows on cuda:0, per path.

    python tools/window_frames_bench.py --rows 1000000 --partitions 1000 --func stddev,kurtosis \
        --frame 4,16,64,256,1024,running --path direct,levels,tensor

``--frame N`` is ``ROWS BETWEEN N-1 PRECEDING AND CURRENT ROW`` (N rows), ``running`` the default frame of an ordered
window.  ``--path`` pins how ``windowfn`` gets the frame states: ``direct`` and ``levels`` are the two entry points
of ``ops/csrc/window_frames.hip`` (``FRAME_DIRECT_MAX`` set above / below every frame), ``tensor`` the tensor-operation
formulation on the same device (``_frame_state_tensor``), ``auto`` the engine's own choice.  The paths of one shape
are alternated, after ``--warmup`` unmeasured rounds, and every call is timed with device events around a
synchronise: ``stmt_ms`` is the whole statement (partition ids, sort, frame bounds, states, finishing, scatter),
``state_ms`` the frame states alone.  One JSON line per (func, frame, path): medians, and the min / max of the
repeats as the spread."""
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


def table(rows, partitions, seed, dev):
    """id 0 .. rows-1, k one of ``partitions`` keys, v and u multiples of 0.25 in [0, 64) (v skewed), 10 % NULLs."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, partitions, (rows,), generator=g)
    v = torch.floor(256 * torch.rand(rows, generator=g, dtype=torch.float64) ** 2) / 4
    u = torch.floor(v * 2) * 0.25 + torch.randint(0, 128, (rows,), generator=g) * 0.25
    ok = torch.rand(rows, generator=g) > 0.1
    cols = [PrimColumn("long", torch.arange(rows)), PrimColumn("long", k), PrimColumn("double", v, ok),
            PrimColumn("double", u)]
    return Table(["id", "k", "v", "u"], [c.to(dev) for c in cols], rows, dev)


def statement(func, frame):
    call = f"{func}(v, u)" if W.FRAME_MOMENTS[func] == W.KIND_CO else f"{func}(v)"
    spec = "" if frame == "running" else f" ROWS BETWEEN {int(frame) - 1} PRECEDING AND CURRENT ROW"
    return f"SELECT id, {call} OVER (PARTITION BY k ORDER BY id{spec}) AS x FROM T"


def timed_call(sql, cat, ctx, path, dev):
    """One call of ``sql`` with the frame states taken by ``path`` → (statement ms, frame-state ms)."""
    real_state, real_max = W._frame_state, W.FRAME_DIRECT_MAX
    inner = W._frame_state_tensor if path == "tensor" else real_state
    marks = []

    def state(*a):
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
        out = inner(*a)
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
        return out
    W._frame_state = state
    if path in ("direct", "levels"):
        W.FRAME_DIRECT_MAX = 1 << 62 if path == "direct" else 0
    try:
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = run_sql(sql, cat, ctx)
        _ = out.columns[1].data                             # the window column is materialised
        t1.record()
        torch.cuda.synchronize(dev)
    finally:
        W._frame_state, W.FRAME_DIRECT_MAX = real_state, real_max
    return t0.elapsed_time(t1), marks[0].elapsed_time(marks[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--partitions", type=int, default=1000)
    ap.add_argument("--frame", default="64", help="comma list of frame lengths in rows, or 'running'")
    ap.add_argument("--func", default="stddev", help="comma list of window aggregates")
    ap.add_argument("--path", default="direct,levels,tensor", help="comma list of direct, levels, tensor, auto")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_frames_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    cat = Catalog()
    cat.register("T", table(args.rows, args.partitions, args.seed, dev))
    ctx = EvalContext(now_us=0, device=dev)
    paths = args.path.split(",")
    for func in args.func.split(","):
        for frame in args.frame.split(","):
            sql = statement(func, frame)
            times = {p: [] for p in paths}
            for r in range(args.warmup + args.repeats):
                for p in paths:                                # alternated: every round takes each path once
                    t = timed_call(sql, cat, ctx, p, dev)
                    if r >= args.warmup:
                        times[p].append(t)
            for p in paths:
                stmt, state = [t[0] for t in times[p]], [t[1] for t in times[p]]
                print(json.dumps({"func": func, "frame": frame, "path": p, "rows": args.rows,
                                  "partitions": args.partitions, "repeats": args.repeats,
                                  "stmt_ms": round(statistics.median(stmt), 4),
                                  "stmt_min_ms": round(min(stmt), 4), "stmt_max_ms": round(max(stmt), 4),
                                  "state_ms": round(statistics.median(state), 4),
                                  "state_min_ms": round(min(state), 4), "state_max_ms": round(max(state), 4)}),
                      flush=True)


if __name__ == "__main__":
    main()
