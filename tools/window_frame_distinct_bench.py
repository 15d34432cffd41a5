"""Time approx_count_distinct / count(DISTINCT …) over window frames: one statement over seeded rows on cuda:0, per path.

    python tools/window_frame_distinct_bench.py --rows 1000000 --partitions 1000 \
        --frame 4,16,64,256,1024,4096,running --card low,high --path direct,tree,tensor

``--frame N`` is ``ROWS BETWEEN N-1 PRECEDING AND CURRENT ROW`` (N rows), ``running`` the default frame of an ordered
window.  ``--card`` picks the argument: ``low`` has about 16 different values, ``high`` nearly as many as rows; both
have 10 % NULLs.  ``--path`` pins how ``windowfn`` counts: ``direct`` and ``tree`` are the two entry points of
``ops/csrc/window_distinct.hip`` (``FRAME_DISTINCT_DIRECT_MAX`` set above / below every frame), ``tensor`` the
tensor-operation wavelet walk on the same device (``_frame_distinct_tensor``), ``auto`` the engine's own choice.  The
direct entry is linear in the frame length; a shape whose frames (at most a partition's rows) are longer than
``--direct-cap`` is not run through it.  The paths of one shape are alternated, after ``--warmup`` unmeasured rounds,
and every call is timed with device events around a synchronise: ``stmt_ms`` is the whole statement (partition ids,
sort, frame bounds, value ids, counting, scatter), ``count_ms`` the counting primitive alone (``_frame_distinct``: the
previous-occurrence array and the path's own work), ``p_ms`` the previous-occurrence array, ``build_ms`` the wavelet
matrix (radix sort, prefix counts and scatters) and ``query_ms`` the path's query (the threshold tensor and the one
launch for ``tree``, the one launch for ``direct``, the level walk for ``tensor``).  One JSON line per (card, frame,
path): medians, and the min / max of the repeats as the spread."""
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

CARDS = {"low": "lo", "high": "hi"}
HOOKS = ("_frame_distinct", "_prev_occurrence", "_distinct_tree_build", "_frame_distinct_tree",
         "_frame_distinct_direct", "_frame_distinct_tensor")


def table(rows, partitions, seed, dev):
    """id 0 .. rows-1, k one of ``partitions`` keys, lo one of 16 longs, hi one of 2^40 longs; 10 % NULLs in both."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, partitions, (rows,), generator=g)
    lo = torch.randint(0, 16, (rows,), generator=g)
    hi = torch.randint(0, 1 << 40, (rows,), generator=g)
    ok = torch.rand(rows, generator=g) > 0.1
    cols = [PrimColumn("long", torch.arange(rows)), PrimColumn("long", k), PrimColumn("long", lo, ok),
            PrimColumn("long", hi, ok)]
    return Table(["id", "k", "lo", "hi"], [c.to(dev) for c in cols], rows, dev)


def statement(card, frame):
    spec = "" if frame == "running" else f" ROWS BETWEEN {int(frame) - 1} PRECEDING AND CURRENT ROW"
    return f"SELECT id, approx_count_distinct({CARDS[card]}) OVER (PARTITION BY k ORDER BY id{spec}) AS x FROM T"


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
    """One call of ``sql`` with the counting taken by ``path`` → (dict of milliseconds, the result column)."""
    real = {h: getattr(W, h) for h in HOOKS}
    bound = W.FRAME_DISTINCT_DIRECT_MAX
    marks = {h: [] for h in HOOKS}
    if path == "tensor":
        def whole(vid, counted, a, b):
            p = W._prev_occurrence(vid, counted)
            return W._frame_distinct_tensor(p, counted, a, b, W._distinct_tree_build(p, counted, tensor=True))
    else:
        whole = real["_frame_distinct"]
    for h in HOOKS:
        setattr(W, h, _timed(whole if h == "_frame_distinct" else real[h], marks[h]))
    if path in ("direct", "tree"):
        W.FRAME_DISTINCT_DIRECT_MAX = 1 << 62 if path == "direct" else 0
    try:
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = run_sql(sql, cat, ctx)
        x = out.columns[1].data                              # the window column is materialised
        t1.record()
        torch.cuda.synchronize(dev)
    finally:
        for h in HOOKS:
            setattr(W, h, real[h])
        W.FRAME_DISTINCT_DIRECT_MAX = bound

    def total(h):
        return sum(s.elapsed_time(e) for s, e in marks[h])
    t = {"stmt_ms": t0.elapsed_time(t1), "count_ms": total("_frame_distinct"), "p_ms": total("_prev_occurrence")}
    if path != "direct":
        t["build_ms"] = total("_distinct_tree_build")
    queries = {"direct": ("_frame_distinct_direct",), "tree": ("_frame_distinct_tree",),
               "tensor": ("_frame_distinct_tensor",), "auto": ("_frame_distinct_direct", "_frame_distinct_tree")}
    t["query_ms"] = sum(total(h) for h in queries[path])
    return t, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--partitions", type=int, default=1000)
    ap.add_argument("--frame", default="4,16,64,256,1024,4096,running",
                    help="comma list of frame lengths in rows, or 'running'")
    ap.add_argument("--card", default="low,high", help="comma list of " + ", ".join(CARDS))
    ap.add_argument("--path", default="direct,tree,tensor", help="comma list of direct, tree, tensor, auto")
    ap.add_argument("--direct-cap", type=int, default=8192, help="longest frame (rows) run through the direct entry")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_frame_distinct_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    cat = Catalog()
    cat.register("T", table(args.rows, args.partitions, args.seed, dev))
    ctx = EvalContext(now_us=0, device=dev)
    per_partition = -(-args.rows // args.partitions)
    for card in args.card.split(","):
        for frame in args.frame.split(","):
            sql = statement(card, frame)
            longest = per_partition if frame == "running" else min(int(frame), per_partition)
            paths = [p for p in args.path.split(",") if p != "direct" or longest <= args.direct_cap]
            times = {p: [] for p in paths}
            answers = {}
            for r in range(args.warmup + args.repeats):
                for p in paths:                                # alternated: every round takes each path once
                    t, x = timed_call(sql, cat, ctx, p, dev)
                    answers[p] = x
                    if r >= args.warmup:
                        times[p].append(t)
            same = all(bool(torch.equal(answers[p], answers[paths[0]])) for p in paths)
            for p in paths:
                line = {"card": card, "frame": frame, "path": p, "rows": args.rows, "partitions": args.partitions,
                        "repeats": args.repeats, "paths_agree": same}
                for what in times[p][0]:
                    vals = [t[what] for t in times[p]]
                    stem = what[:-3]
                    line[what] = round(statistics.median(vals), 4)
                    line[stem + "_min_ms"] = round(min(vals), 4)
                    line[stem + "_max_ms"] = round(max(vals), 4)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
