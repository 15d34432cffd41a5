"""MIN / MAX over a string column per group: the device kernel (str_minmax.hip through ``groupby.aggregate``) against
the host loop it replaces (``groupby._host_minmax``: a copy of every row to the host and a Python loop).

``--rows`` rows (default 1 M) of 8-40 bytes — eight distinguishing digits and a pad of 0-32 bytes —, group ids uniform
over ``--groups`` ids (default 1, 200 and 50 000), in two row orders: ``random``, and ``ascending`` (every row's string
is greater than the one before it, so under MAX every row beats the best its group held: the longest compare-and-swap
chain).  One JSON line per shape: the device time of MAX and of MIN (median of ``--reps`` runs between device events)
and, unless ``--no-host``, the wall time of one run of the host loop for MAX, with the results compared.

    python tools/str_minmax_bench.py [--rows 1000000] [--groups 1,200,50000] [--reps 9] [--no-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dxa.engine.column import StrColumn  # noqa: E402
from dxa.ops import groupby as G  # noqa: E402


def strings(n, ascending, rng):
    """``n`` strings: the digits of a row's rank (ascending: the row index; else a permutation of them) and a pad."""
    rank = np.arange(n) if ascending else rng.permutation(n)
    lens = 8 + rng.integers(0, 33, n)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    arena = np.full(int(lens.sum()), ord("x"), dtype=np.uint8)
    digits = (rank[:, None] // 10 ** np.arange(7, -1, -1)[None, :] % 10 + ord("0")).astype(np.uint8)
    arena[(starts[:, None] + np.arange(8)[None, :]).ravel()] = digits.ravel()
    return torch.from_numpy(arena), torch.from_numpy(starts.astype(np.int64)), torch.from_numpy(lens.astype(np.int32))


def device_ms(run, reps, dev):
    run()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--groups", default="1,200,50000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("str_minmax_bench.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    n = args.rows
    for order in ("random", "ascending"):
        arena, starts, lens = strings(n, order == "ascending", rng)
        col = StrColumn(arena.to(dev), starts.to(dev), lens.to(dev))
        for ngroups in map(int, args.groups.split(",")):
            gid = torch.from_numpy(rng.integers(0, ngroups, n).astype(np.int32)).to(dev)
            groups = G.Groups(gid, ngroups, torch.zeros(ngroups, dtype=torch.int64, device=dev))
            line = {"rows": n, "groups": ngroups, "order": order}
            for func in ("max", "min"):
                med, lo, hi = device_ms(lambda: G.aggregate(groups, col, func, n), args.reps, dev)
                line.update({f"device_{func}_ms": med, f"device_{func}_ms_range": [lo, hi]})
            if not args.no_host:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                want = G._host_minmax(groups, col, "max", dev)
                torch.cuda.synchronize(dev)
                line["host_max_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                line["equal"] = want.to_pylist() == G.aggregate(groups, col, "max", n).to_pylist()
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
