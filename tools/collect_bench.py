"""Time collect_list / collect_set on cuda:0: per group, and over window frames.

    python tools/collect_bench.py --rows 1000000
    python tools/collect_bench.py --rows 100000 --steps groupby --host-loop

Steps (``--steps`` takes a comma list of prefixes; default: all):

``groupby:<long|string>:<size>``  ``SELECT g, collect_list(v) …`` and ``collect_set(v)`` ``FROM T GROUP BY g`` with
    ``rows / size`` groups of ``size`` rows, rows of a group scattered over the table.  ``v`` is a long out of 2^20
    values or a string out of 4,096 ("dev-…"); nothing is NULL, so every list has ``size`` elements.  ``--host-loop``
    puts the row-by-row host loop (``query._collect_host``) in place of the device path; on a checkout from before
    the device path the statement takes that loop by itself, so the same steps give the baseline there.
``frame:<k>``  (k from ``--frames``) the two calls ``OVER (PARTITION BY g ORDER BY t ROWS BETWEEN k PRECEDING AND
    CURRENT ROW)`` over 1,000 partitions (fewer where a partition would not hold four frames).  The slot matrix has
    ``(k + 1) · rows`` entries: a step whose matrix would pass ``windowfn.FRAME_COLLECT_MAX_SLOTS`` runs on the
    largest row count that fits, and prints it.  ``dxa_frame_collect`` has one launch shape, one thread per row; the
    wave-per-row shape this tool once timed beside it (profiles/collect/README.md) was never faster and is gone.

Every step is a process of its own, started under ``--step-timeout`` seconds, and the run stops at the first step that
fails or is killed.  A call is timed with device events around a synchronise, after ``--warmup`` unmeasured rounds:
``stmt_ms`` is the whole statement, ``collect_ms`` the aggregate alone (``query._collect`` / ``windowfn._frame_collect``)
and, for frames, ``pos_ms`` the position matrix (``_frame_collect_positions``: the one launch).  One JSON line per
measurement: medians, and the min / max of the repeats as the spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPBY_STEPS = [f"groupby:{kind}:{size}" for kind in ("long", "string") for size in (8, 1000)]
PARTITIONS = 1000


def _timed(fn, marks):
    import torch

    def wrapper(*a, **kw):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn(*a, **kw)
        t1.record()
        marks.append((t0, t1))
        return out
    return wrapper


def _measure(run, hooks, warmup, repeats):
    """``run()`` executes one statement; ``hooks``: label → (module, function name) timed inside it → list of dicts."""
    import torch
    out = []
    for r in range(warmup + repeats):
        marks = {label: [] for label in hooks}
        real = {label: getattr(mod, fn) for label, (mod, fn) in hooks.items()}
        for label, (mod, fn) in hooks.items():
            setattr(mod, fn, _timed(real[label], marks[label]))
        try:
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run()
            t1.record()
            torch.cuda.synchronize()
        finally:
            for label, (mod, fn) in hooks.items():
                setattr(mod, fn, real[label])
        if r >= warmup:
            t = {"stmt_ms": t0.elapsed_time(t1)}
            for label in hooks:
                t[label] = sum(s.elapsed_time(e) for s, e in marks[label])
            out.append(t)
    return out


def _line(head, times):
    line = dict(head)
    for what in times[0]:
        vals = [t[what] for t in times]
        stem = what[:-3]
        line[what] = round(statistics.median(vals), 4)
        line[stem + "_min_ms"] = round(min(vals), 4)
        line[stem + "_max_ms"] = round(max(vals), 4)
    print(json.dumps(line), flush=True)


def _value_column(kind, rows, gen, dev):
    import torch
    from dxa.engine.column import PrimColumn, column_from_pylist
    if kind == "long":
        return PrimColumn("long", torch.randint(0, 1 << 20, (rows,), generator=gen).to(dev))
    names = column_from_pylist([f"dev-{i:04d}" for i in range(4096)], "string", dev)
    return names.take(torch.randint(0, 4096, (rows,), generator=gen).to(dev))


def step_groupby(kind, size, args):
    import torch
    from dxa.engine import query as Q
    from dxa.engine.column import PrimColumn, Table
    from dxa.engine.expr import EvalContext
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(args.seed)
    rows = args.rows // size * size
    g = (torch.randperm(rows, generator=gen) % (rows // size)).to(dev)
    t = Table(["g", "v"], [PrimColumn("long", g), _value_column(kind, rows, gen, dev)], rows, dev)
    cat = Q.Catalog()
    cat.register("T", t)
    ctx = EvalContext(now_us=0, device=dev)
    if args.host_loop:
        Q._collect_slots = Q._collect_host
    for func in ("collect_list", "collect_set"):
        sql = f"SELECT g, {func}(v) AS a FROM T GROUP BY g"
        times = _measure(lambda: run_sql_sync(Q, sql, cat, ctx), {"collect_ms": (Q, "_collect")}, args.warmup,
                         args.repeats)
        _line({"step": f"groupby:{kind}:{size}", "func": func, "rows": rows, "groups": rows // size,
               "path": "host" if args.host_loop else "engine", "repeats": args.repeats}, times)


def run_sql_sync(Q, sql, cat, ctx):
    out = Q.run_sql(sql, cat, ctx)
    return out.columns[-1].elements[0]                        # the array column is materialised


def step_frame(k, args):
    import torch
    from dxa.engine import query as Q
    from dxa.engine import windowfn as W
    from dxa.engine.column import PrimColumn, Table
    from dxa.engine.expr import EvalContext
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(args.seed)
    rows = min(args.rows, W.FRAME_COLLECT_MAX_SLOTS // (k + 1))
    partitions = max(1, min(PARTITIONS, rows // (4 * (k + 1))))          # a partition holds about four frames or more
    g = torch.randint(0, partitions, (rows,), generator=gen).to(dev)
    t = Table(["g", "t", "v"], [PrimColumn("long", g), PrimColumn("long", torch.arange(rows, device=dev)),
                                _value_column("long", rows, gen, dev)], rows, dev)
    cat = Q.Catalog()
    cat.register("T", t)
    ctx = EvalContext(now_us=0, device=dev)
    hooks = {"collect_ms": (W, "_frame_collect"), "pos_ms": (W, "_frame_collect_positions")}
    for func in ("collect_list", "collect_set"):
        sql = (f"SELECT t, {func}(v) OVER (PARTITION BY g ORDER BY t ROWS BETWEEN {k} PRECEDING AND CURRENT ROW) AS a "
               "FROM T")
        times = _measure(lambda: run_sql_sync(Q, sql, cat, ctx), hooks, args.warmup, args.repeats)
        _line({"step": f"frame:{k}", "func": func, "rows": rows, "partitions": partitions, "frame": k + 1,
               "repeats": args.repeats}, times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", default="groupby,frame", help="comma list of step-name prefixes")
    ap.add_argument("--frames", default="7,63,255", help="comma list of k, the frame steps' rows PRECEDING")
    ap.add_argument("--host-loop", action="store_true", help="GROUP BY steps through query._collect_host")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds for one step's process")
    ap.add_argument("--one", help="run this one step in this process (what the driver starts)")
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("collect_bench.py measures on a GPU; none found")
        what = args.one.split(":")
        if what[0] == "groupby":
            step_groupby(what[1], int(what[2]), args)
        else:
            step_frame(int(what[1]), args)
        return
    frame_steps = [f"frame:{int(k)}" for k in args.frames.split(",")]
    wanted = [s for s in GROUPBY_STEPS + frame_steps if any(s.startswith(p) for p in args.steps.split(","))]
    for step in wanted:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", step,
               "--rows", str(args.rows), "--warmup", str(args.warmup), "--repeats", str(args.repeats),
               "--seed", str(args.seed)] + (["--host-loop"] if args.host_loop else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"step {step} ended with status {rc}; nothing further was started")


if __name__ == "__main__":
    main()
