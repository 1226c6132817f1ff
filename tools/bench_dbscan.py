#!/usr/bin/env python3
"""Times the density clusters and the degrees against the dense path and the components they are built on,
in ONE process, alternating arms, device-resident sketches, a synchronise inside every timed region, medians of --reps:
  A  dist_rows_device over the full triangle (the dense path; its sources are hashed into the output)
  C  cluster_threshold_device
  G  degree_threshold_device (walk 1 alone)
  D  dbscan_threshold_device with --min-pts (5), labels, kinds and degrees into device buffers
  R  a device-to-device copy of the dense span: one read and one write of it, the yardstick for D - A
at thresholds giving about 0.1 %, 1 % and 50 % hits.  Before timing, D at min_pts 1 and C must give the same labels.  The two
expectations the record answers by itself:
  one band (c2):  D - A <= (C - A) + two reads of the span (R) + the spread of A
  every shape:    G - A and D - A do not grow with the hit rate by more than the spread of A
One JSON line per shape on stdout (and into --out DIR/bench_dbscan.jsonl).

  python tools/bench_dbscan.py --shapes c2,100k --reps 5 --out profiles/dbscan1"""
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
    ap.add_argument("--min-pts", type=int, default=5)
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
        labels_c = torch.empty(n, dtype=torch.int32, device=dev)
        degree = torch.empty(n, dtype=torch.int32, device=dev)
        kind = torch.empty(n, dtype=torch.uint8, device=dev)
        ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)  # warm-up, and the thresholds' source
        sample = dense[:: max(span // (1 << 24), 1)].cpu().numpy()
        ts = {name: float(np.quantile(sample, q)) for name, q in (("0.1%", 0.001), ("1%", 0.01), ("50%", 0.5))}
        hits, clusters, dbs = {}, {}, {}
        for name, t in ts.items():
            ctx.dist_threshold_device(rp.data_ptr(), 0, 0, 0, t, 0, n, **kw)
            hits[name] = int(rp[-1].item())
            # D at min_pts 1 is C, byte for byte
            nc = ctx.cluster_threshold_device(labels_c.data_ptr(), t, **kw)
            n1, noise1 = ctx.dbscan_threshold_device(labels.data_ptr(), t, 1, **kw)
            assert n1 == nc and noise1 == 0 and torch.equal(labels, labels_c), name
            ctx.degree_threshold_device(degree.data_ptr(), t, **kw)  # warm-up of G; every hit has two ends
            assert int(degree.to(torch.int64).sum().item()) == 2 * hits[name], name
            clusters[name] = nc
            dbs[name] = ctx.dbscan_threshold_device(labels.data_ptr(), t, a.min_pts, kind_ptr=kind.data_ptr(), degree_ptr=degree.data_ptr(), **kw)
            dbs[name] += tuple(int(x) for x in torch.bincount(kind.to(torch.int64), minlength=3).tolist())
        torch.cuda.synchronize()
        times = {"A": [], "R": [], **{arm + " " + k: [] for arm in "CGD" for k in ts}}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)
            times["A"].append(time.perf_counter() - t0)
            for name, t in ts.items():
                t0 = time.perf_counter()
                nc = ctx.cluster_threshold_device(labels_c.data_ptr(), t, **kw)
                times["C " + name].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                ctx.degree_threshold_device(degree.data_ptr(), t, **kw)
                times["G " + name].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                got = ctx.dbscan_threshold_device(labels.data_ptr(), t, a.min_pts, kind_ptr=kind.data_ptr(), degree_ptr=degree.data_ptr(), **kw)
                times["D " + name].append(time.perf_counter() - t0)
                assert nc == clusters[name] and got == dbs[name][:2]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            copy.copy_(dense)
            torch.cuda.synchronize()
            times["R"].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
        spread = (max(times["A"]) - min(times["A"])) * 1e3
        over = {arm: {k: med[arm + " " + k] - med["A"] for k in ts} for arm in "CGD"}
        bands = -(-span * 4 // (1 << 30))  # (about: bands hold whole rows)
        rec = {"shape": shape, "n": n, "p": p, "pairs": span, "reps": a.reps, "measure": "MASH_DIST k=31", "min_pts": a.min_pts,
               "thresholds": ts, "hits": hits, "clusters": clusters,
               "dbscan": {k: dict(zip(("n_clusters", "n_noise", "noise", "border", "core"), v)) for k, v in dbs.items()},
               "ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
               "median_ms": {k: round(v, 3) for k, v in med.items()},
               "C_minus_A_ms": {k: round(v, 3) for k, v in over["C"].items()},
               "G_minus_A_ms": {k: round(v, 3) for k, v in over["G"].items()},
               "D_minus_A_ms": {k: round(v, 3) for k, v in over["D"].items()},
               "D_over_A": {k: round(med["D " + k] / med["A"], 3) for k in ts},
               "spread_A_ms": round(spread, 3), "bands_about": int(bands),
               # the two expectations (the first is the one-band claim: on a shape of several bands D is about 2 A by design)
               "D_within_C_plus_two_reads": {k: bool(over["D"][k] <= over["C"][k] + med["R"] + spread) for k in ts},
               "growth_with_hits_ms": {arm: round(max(over[arm].values()) - min(over[arm].values()), 3) for arm in "GD"},
               "growth_within_spread": {arm: bool(max(over[arm].values()) - min(over[arm].values()) <= spread) for arm in "GD"},
               "dense_sources_sha256": source_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_dbscan.jsonl"), "a") as f:
                f.write(line + "\n")
        del dense, copy, regs, labels, labels_c, degree, kind
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
