#!/usr/bin/env python3
"""Times the greedy representatives against the dense path they are built on and against the threshold clusters (DESIGN.md
4.11), in ONE process, alternating arms, device-resident sketches, a synchronise inside every timed region, medians of
--reps:
  A  dist_rows_device over the full triangle (the dense path; its sources are hashed into the output)
  C  cluster_threshold_device: reads each band once, the yardstick for G - A at the same hit rate
  G  greedy_threshold_device: reads each band once and adds the sequential diagonal (k_greedy_diag)
at thresholds giving about 0.1 %, 1 % and 50 % hits, and one that nothing passes: the worst case for G -- every row is a
representative, k_greedy_diag scans every in-band value and k_greedy_band walks every row.  One JSON line per shape on
stdout (and into --out DIR/bench_greedy.jsonl).  --rates none restricts the run to one rate, for a kernel trace of it.

  python tools/bench_greedy.py --shapes c2,100k --reps 5 --out profiles/greedy1"""
import argparse
import json
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
    ap.add_argument("--rates", default="0.1%,1%,50%,none", help="hit rates to time (a kernel trace of one rate alone)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import dashing_amd as D

    torch.cuda.init()
    dev = torch.device("cuda:0")
    ctx = D.Context(0)
    kw = dict(result_type=D.MASH_DIST, k=31)
    for shape in a.shapes.split(","):
        regs, n, p, _ = collection(torch, dev, shape)
        ctx.attach_device(regs.data_ptr(), n, p)
        span = D.tri_span(n, 0, n)
        dense = torch.empty(span, dtype=torch.float32, device=dev)
        rp = torch.empty(n + 1, dtype=torch.int64, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)  # warm-up, and the thresholds' source
        sample = dense[:: max(span // (1 << 24), 1)].cpu().numpy()
        ts = {name: float(np.quantile(sample, q)) for name, q in (("0.1%", 0.001), ("1%", 0.01), ("50%", 0.5))}
        ts["none"] = -1.0  # a Mash distance is never negative: nothing passes
        ts = {k: v for k, v in ts.items() if k in a.rates.split(",")}
        hits, clusters, reps = {}, {}, {}
        for name, t in ts.items():
            ctx.dist_threshold_device(rp.data_ptr(), 0, 0, 0, t, 0, n, **kw)
            hits[name] = int(rp[-1].item())
            clusters[name] = ctx.cluster_threshold_device(labels.data_ptr(), t, **kw)  # warm-up of C
            reps[name] = ctx.greedy_threshold_device(labels.data_ptr(), t, **kw)  # warm-up of G
            assert reps[name] >= clusters[name]
        assert "none" not in ts or (hits["none"] == 0 and reps["none"] == n)
        torch.cuda.synchronize()
        times = {"A": [], **{"C " + k: [] for k in ts}, **{"G " + k: [] for k in ts}}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)  # (synchronous, as C and G are: each waits for the device)
            times["A"].append(time.perf_counter() - t0)
            for name, t in ts.items():
                t0 = time.perf_counter()
                nc = ctx.cluster_threshold_device(labels.data_ptr(), t, **kw)
                times["C " + name].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                nr = ctx.greedy_threshold_device(labels.data_ptr(), t, **kw)
                times["G " + name].append(time.perf_counter() - t0)
                assert nc == clusters[name] and nr == reps[name]
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
        rec = {"shape": shape, "n": n, "p": p, "pairs": span, "reps": a.reps, "measure": "MASH_DIST k=31", "thresholds": ts,
               "hits": hits, "clusters": clusters, "representatives": reps,
               "ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
               "median_ms": {k: round(v, 3) for k, v in med.items()},
               "C_minus_A_ms": {k: round(med["C " + k] - med["A"], 3) for k in ts},
               "G_minus_A_ms": {k: round(med["G " + k] - med["A"], 3) for k in ts},
               "spread_A_ms": round((max(times["A"]) - min(times["A"])) * 1e3, 3), "dense_sources_sha256": source_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_greedy.jsonl"), "a") as f:
                f.write(line + "\n")
        del dense, regs, labels
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
