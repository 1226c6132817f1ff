#!/usr/bin/env python3
"""Times the threshold clusters against the dense path they are built on, in ONE process, alternating
arms, device-resident sketches, a synchronise inside every timed region, medians of --reps:
  A  dist_rows_device over the full triangle (the dense path; its sources are hashed into the output)
  B  dist_threshold_device (emit) + the hits' way to the host + cluster_csr over them: what a client pays today
     (left out, and said so, where the hits exceed --max-hits)
  C  cluster_threshold_device
  R  a device-to-device copy of the dense span: one read and one write of it, the yardstick for C - A
at thresholds giving about 0.1 %, 1 % and 50 % hits.  B and C must give the same labels.  One JSON line per shape on
stdout (and into --out DIR/bench_cluster.jsonl).

  python tools/bench_cluster.py --shapes c2,100k --reps 5 --out profiles/cluster1"""
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
    ap.add_argument("--max-hits", type=int, default=1 << 28)
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
        copy = torch.empty(span, dtype=torch.float32, device=dev)
        rp = torch.empty(n + 1, dtype=torch.int64, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)  # warm-up, and the thresholds' source
        sample = dense[:: max(span // (1 << 24), 1)].cpu().numpy()
        ts = {name: float(np.quantile(sample, q)) for name, q in (("0.1%", 0.001), ("1%", 0.01), ("50%", 0.5))}
        bufs, clusters = {}, {}
        for name, t in ts.items():
            ctx.dist_threshold_device(rp.data_ptr(), 0, 0, 0, t, 0, n, **kw)
            hits = int(rp[-1].item())
            emit = hits <= a.max_hits
            bufs[name] = (hits, torch.empty(max(hits, 1) if emit else 1, dtype=torch.int32, device=dev),
                          torch.empty(max(hits, 1) if emit else 1, dtype=torch.float32, device=dev), emit)
            clusters[name] = ctx.cluster_threshold_device(labels.data_ptr(), t, **kw)  # warm-up of C
        torch.cuda.synchronize()
        times = {"A": [], "R": [], **{"B " + k: [] for k, v in bufs.items() if v[3]}, **{"C " + k: [] for k in ts}}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)
            times["A"].append(time.perf_counter() - t0)
            for name, t in ts.items():
                hits, col, val, emit = bufs[name]
                t0 = time.perf_counter()
                nc = ctx.cluster_threshold_device(labels.data_ptr(), t, **kw)
                times["C " + name].append(time.perf_counter() - t0)
                assert nc == clusters[name]
                if not emit:
                    continue
                lab_c = labels.cpu().numpy().view(np.uint32)
                t0 = time.perf_counter()
                got = ctx.dist_threshold_device(rp.data_ptr(), col.data_ptr(), val.data_ptr(), hits, t, 0, n, **kw)
                lab_b, nb = ctx.cluster_csr(n, rp.cpu().numpy().view(np.uint64), col[:hits].cpu().numpy().view(np.uint32))
                times["B " + name].append(time.perf_counter() - t0)
                assert got == hits and nb == nc and np.array_equal(lab_b, lab_c)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            copy.copy_(dense)
            torch.cuda.synchronize()
            times["R"].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
        rec = {"shape": shape, "n": n, "p": p, "pairs": span, "reps": a.reps, "measure": "MASH_DIST k=31", "thresholds": ts,
               "hits": {k: v[0] for k, v in bufs.items()}, "clusters": clusters,
               "B_left_out": [k for k, v in bufs.items() if not v[3]],
               "ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
               "median_ms": {k: round(v, 3) for k, v in med.items()},
               "C_minus_A_ms": {k: round(med["C " + k] - med["A"], 3) for k in ts},
               "B_minus_A_ms": {k: round(med["B " + k] - med["A"], 3) for k in ts if "B " + k in med},
               "spread_A_ms": round((max(times["A"]) - min(times["A"])) * 1e3, 3), "dense_sources_sha256": source_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_cluster.jsonl"), "a") as f:
                f.write(line + "\n")
        del dense, copy, regs, labels
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
