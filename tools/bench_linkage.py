#!/usr/bin/env python3
"""Times the complete- and average-linkage clusters against the single-linkage components they are partitioned by
(DESIGN.md 4.15), in ONE process, alternating arms, device-resident sketches, every call synchronous, medians of --reps:
  A  cluster_threshold_device: the components (exists before this call did; the reference point)
  L  linkage_threshold_device for COMPLETE and AVERAGE under "linkage_route" 0 (dense) and 1 (pairs)
  H  (--host, 10 000 sketches only) what the call replaces: dist_rows to the host + scipy linkage + fcluster
at thresholds giving about 0.1 %, 1 % and 50 % hits.  A case that ends in the budget refusal (DSH_ENOMEM: one component's
matrix beyond "linkage_budget_bytes") is recorded as such, not timed.  Per case also the largest component of A's labels and
L - A per merge step of it.  One JSON line per shape on stdout (and into --out DIR/bench_linkage.jsonl).

  python tools/bench_linkage.py --shapes c2,100k --reps 5 --host --out profiles/linkage1"""
import argparse
import hashlib
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

LINKAGE_SOURCES = ("linkage.h", "linkage.hip", "kernels_linkage.hip", "cluster.hip", "kernels_cluster.hip")


def linkage_hashes():
    out = {}
    for f in LINKAGE_SOURCES:
        with open(os.path.join(ROOT, "dashing_amd", "csrc", f), "rb") as h:
            out[f] = hashlib.sha256(h.read()).hexdigest()[:16]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hits", default="0.001,0.01,0.5", help="hit fractions the thresholds are taken at")
    ap.add_argument("--host", action="store_true", help="also time the host route (scipy) where n <= 10 000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import dashing_amd as D

    torch.cuda.init()
    dev = torch.device("cuda:0")
    ctx = D.Context(0)
    kw = dict(result_type=D.MASH_DIST, k=31)
    arms = [(name, route) for name in ("complete", "average") for route in (0, 1)]
    for shape in a.shapes.split(","):
        regs, n, p, _ = collection(torch, dev, shape)
        ctx.attach_device(regs.data_ptr(), n, p)
        span = D.tri_span(n, 0, n)
        dense = torch.empty(span, dtype=torch.float32, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)  # warm-up, and the thresholds' source
        sample = dense[:: max(span // (1 << 24), 1)].cpu().numpy()
        del dense
        torch.cuda.empty_cache()
        ts = {"%g%%" % (100 * float(q)): float(np.quantile(sample, float(q))) for q in a.hits.split(",")}
        largest, clusters, refused = {}, {}, {}

        def run(name, route, t):
            ctx.set_option("linkage_route", route)
            try:
                return ctx.linkage_threshold_device(labels.data_ptr(), t, name, **kw)
            finally:
                ctx.set_option("linkage_route", -1)

        for tn, t in ts.items():  # warm-up of every arm; which cases the budget refuses
            ctx.cluster_threshold_device(labels.data_ptr(), t, **kw)
            largest[tn] = int(np.bincount(labels.cpu().numpy().view(np.uint32)).max())
            for name, route in arms:
                key = "L %s %s %s" % (name, "pairs" if route else "dense", tn)
                try:
                    clusters[key] = run(name, route, t)
                except D.DshError as e:
                    if e.code != -12:
                        raise
                    refused[key] = str(e)
        times = {"A " + tn: [] for tn in ts}
        times.update({k: [] for k in clusters})
        for _ in range(a.reps):
            for tn, t in ts.items():
                t0 = time.perf_counter()
                ctx.cluster_threshold_device(labels.data_ptr(), t, **kw)
                times["A " + tn].append(time.perf_counter() - t0)
                for name, route in arms:
                    key = "L %s %s %s" % (name, "pairs" if route else "dense", tn)
                    if key not in clusters:
                        continue
                    t0 = time.perf_counter()
                    nc = run(name, route, t)
                    times[key].append(time.perf_counter() - t0)
                    assert nc == clusters[key]
        host = {}
        if a.host and n <= 10_000:
            from scipy.cluster import hierarchy

            for tn, t in ts.items():
                for method in ("complete", "average"):
                    t0 = time.perf_counter()
                    tri = ctx.dist_rows(**kw)
                    flat = hierarchy.fcluster(hierarchy.linkage(tri.astype(np.float64), method=method), t, criterion="distance")
                    host["H %s %s" % (method, tn)] = round((time.perf_counter() - t0) * 1e3, 3)
                    del tri, flat
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items() if v}
        rec = {"shape": shape, "n": n, "p": p, "pairs": span, "reps": a.reps, "measure": "MASH_DIST k=31", "thresholds": ts,
               "largest_component": largest, "clusters": clusters, "budget_refusals": refused,
               "median_ms": {k: round(v, 3) for k, v in med.items()},
               "L_minus_A_ms": {k: round(v - med["A " + k.rsplit(" ", 1)[1]], 3) for k, v in med.items() if k.startswith("L ")},
               "L_minus_A_us_per_step_of_largest": {k: round((v - med["A " + k.rsplit(" ", 1)[1]]) * 1e3 / max(largest[k.rsplit(" ", 1)[1]] - 1, 1), 3)
                                                    for k, v in med.items() if k.startswith("L ")},
               "host_once_ms": host, "ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
               "dense_sources_sha256": source_hashes(), "linkage_sources_sha256": linkage_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_linkage.jsonl"), "a") as f:
                f.write(line + "\n")
        del regs, labels
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
