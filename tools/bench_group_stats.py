#!/usr/bin/env python3
"""Times dsh_group_stats*  against the dense path it is built on, in ONE process, alternating arms,
device-resident sketches, every call synchronous (each waits for the device), medians of --reps:
  A        dist_rows_device over the full triangle (the dense path; its sources are hashed into the output)
  S_dense  group_stats_device, dense route: the dense path per band plus k_gs_rows and k_gs_cols
  S_pairs  group_stats_device, pairs route: the intra-group pairs enumerated and computed directly
for labellings of equal groups (label = slot // s) whose intra-group pairs P_in are about 0.01 %, 0.1 %, 1 %, 5 %, 20 % and
100 % of the triangle: s = 1 + f (n - 1).  The two routes' outputs are compared byte for byte once per labelling.  One JSON
line per shape on stdout (and into --out DIR/bench_group_stats.jsonl), with the crossover: the fraction at which
S_pairs = S_dense, interpolated linearly in log(f) between the two fractions around it.  --fracs and --arms restrict the
run (a run of its own per step, each under its own time limit; a kernel trace of one arm).

  python tools/bench_group_stats.py --shapes c2,100k --reps 5 --out profiles/stats1"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_threshold import collection, source_hashes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fracs", default="0.0001,0.001,0.01,0.05,0.2,1", help="P_in as fractions of the triangle")
    ap.add_argument("--arms", default="A,S_dense,S_pairs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import dashing_amd as D

    torch.cuda.init()
    dev = torch.device("cuda:0")
    ctx = D.Context(0)
    kw = dict(result_type=D.MASH_DIST, k=31)
    arms = a.arms.split(",")
    routes = [r for r in ("dense", "pairs") if "S_" + r in arms]
    for shape in a.shapes.split(","):
        regs, n, p, _ = collection(torch, dev, shape)
        ctx.attach_device(regs.data_ptr(), n, p)
        span = D.tri_span(n, 0, n)
        dense = torch.empty(span, dtype=torch.float32, device=dev) if "A" in arms else None
        out = {r: [torch.empty(n, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64, torch.float32)] for r in routes}
        ptrs = {r: [t.data_ptr() for t in out[r]] for r in routes}
        if dense is not None:
            ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)  # warm-up
        labs, p_in = {}, {}
        for f in [float(x) for x in a.fracs.split(",")]:
            s = min(max(int(round(1 + f * (n - 1))), 1), n)
            lab = (np.arange(n, dtype=np.int64) // s).astype(np.uint32)
            name = "%g%%" % (100 * f)
            labs[name] = lab
            sizes = np.bincount(lab).astype(np.int64)
            p_in[name] = int((sizes * (sizes - 1) // 2).sum())
            for r in routes:  # warm-up, and the routes held to each other
                ctx.group_stats_device(lab, *ptrs[r], route=r, **kw)
            torch.cuda.synchronize()
            if len(routes) == 2:
                assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out["dense"], out["pairs"])), name
        times = {**({"A": []} if dense is not None else {}), **{"S_%s %s" % (r, k): [] for k in labs for r in routes}}
        for _ in range(a.reps):
            if dense is not None:
                t0 = time.perf_counter()
                ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)
                times["A"].append(time.perf_counter() - t0)
            for name, lab in labs.items():
                for r in routes:
                    t0 = time.perf_counter()
                    ctx.group_stats_device(lab, *ptrs[r], route=r, **kw)
                    times["S_%s %s" % (r, name)].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
        rec = {"shape": shape, "n": n, "p": p, "pairs": span, "reps": a.reps, "measure": "MASH_DIST k=31", "p_in": p_in,
               "p_in_fraction": {k: round(v / span, 6) for k, v in p_in.items()},
               "ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
               "median_ms": {k: round(v, 3) for k, v in med.items()}, "dense_sources_sha256": source_hashes()}
        if dense is not None and "dense" in routes:
            rec["S_dense_minus_A_ms"] = {k: round(med["S_dense " + k] - med["A"], 3) for k in labs}
            rec["spread_A_ms"] = round((max(times["A"]) - min(times["A"])) * 1e3, 3)
        if len(routes) == 2:  # the first fraction at which the pairs route is the slower one
            names = list(labs)
            diff = [med["S_pairs " + k] - med["S_dense " + k] for k in names]
            fr = [p_in[k] / span for k in names]
            cross = None
            for x in range(1, len(names)):
                if diff[x - 1] <= 0 < diff[x] and fr[x - 1] > 0:
                    w = -diff[x - 1] / (diff[x] - diff[x - 1])
                    cross = math.exp(math.log(fr[x - 1]) + w * (math.log(fr[x]) - math.log(fr[x - 1])))
                    break
            rec["crossover_fraction"] = None if cross is None else round(cross, 5)
            rec["pairs_faster_at"] = [k for k, d in zip(names, diff) if d <= 0]
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_group_stats.jsonl"), "a") as f:
                f.write(line + "\n")
        del dense, regs, out
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
