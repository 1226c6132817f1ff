#!/usr/bin/env python3
"""Times dsh_dist_histogram_device against the dense path it is built on, in ONE process, alternating
arms, device-resident sketches, every call synchronous (each waits for the device), medians of --reps:
  A   dist_rows_device over the full triangle (the dense path; its sources are hashed into the output)
  H   dist_histogram_device over the same rows: the dense path per band plus k_hist
for 2, 101 and 4096 edges, each in three placements and each with and without labels:
  oneclass   edges spread evenly over [2, 3], above every value: ONE class holds everything, the case in which the
             wave-level aggregation of k_hist has to work (a real collection, J = 0 across clusters, is close to it)
  uniform    edges spread evenly over [0, 1]
  quantile   edges at quantiles of the values (of a strided sample; ties removed, filled up from the distinct values): the
             values spread over the classes as evenly as their ties allow
Labels are equal groups of 16 slots.  Every record carries the share of the largest class, so that the placements can be
told apart in the output.  Shapes: c2 and 100k (tools/bench_threshold.py), in which about half of the values are ONE
value (unrelated sketches), and `spread`: 20 000 x p=12 sketches that all share one core (synth.related_sketches with one
cluster), whose values are continuous, so that its quantile placement is a uniform spread over the classes.  One JSON line
per shape on stdout (and into --out DIR/bench_hist.jsonl).

  python tools/bench_hist.py --shapes c2,100k,spread --reps 5 --out profiles/hist1"""
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


def quantile_edges(sample, ne):
    """ne strictly increasing float32 edges at quantiles of the finite values of `sample`"""
    fin = np.sort(sample[np.isfinite(sample)]).astype(np.float32)
    if not fin.size:
        fin = np.array([0.0, 1.0], np.float32)
    e = np.unique(fin[np.round(np.linspace(0, fin.size - 1, ne + 2)[1:-1]).astype(np.int64)])
    if e.size < ne:  # ties: fill up from the distinct values, then with the floats that follow the largest one
        u = np.unique(fin)
        e = np.unique(np.concatenate([e, u[np.round(np.linspace(0, u.size - 1, min(u.size, ne))).astype(np.int64)]]))[:ne]
    if e.size < ne:
        base = e[-1] if e[-1] > 0 else np.float32(0)
        e = np.concatenate([e, (np.array([base], np.float32).view(np.uint32)[0] + np.arange(1, ne - e.size + 1, dtype=np.uint32)).view(np.float32)])
    assert e.size == ne and (np.diff(e) > 0).all()
    return e.astype(np.float32)


def shape_collection(torch, dev, shape):
    if shape == "spread":  # every pair shares the core: no clamp to J = 0, values without a dominating tie
        from dashing_amd import synth

        n, p = 20_000, 12
        return torch.from_numpy(synth.related_sketches(n, p, seed=0x5EED4000, cluster=n)[0]).to(dev), n, p, None
    return collection(torch, dev, shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--edges", default="2,101,4096")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import dashing_amd as D

    torch.cuda.init()
    dev = torch.device("cuda:0")
    ctx = D.Context(0)
    kw = dict(result_type=D.MASH_DIST, k=31)
    for shape in a.shapes.split(","):
        regs, n, p, _ = shape_collection(torch, dev, shape)
        ctx.attach_device(regs.data_ptr(), n, p)
        span = D.tri_span(n, 0, n)
        dense = torch.empty(span, dtype=torch.float32, device=dev)
        ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)  # warm-up, and the quantiles' source
        torch.cuda.synchronize()
        sample = dense[:: max(span // (1 << 22), 1)].cpu().numpy()
        lab = (np.arange(n, dtype=np.int64) // 16).astype(np.uint32)
        arms, largest = {}, {}
        for ne in [int(x) for x in a.edges.split(",")]:
            for place, edges in (("oneclass", np.linspace(2, 3, ne).astype(np.float32)), ("uniform", np.linspace(0, 1, ne).astype(np.float32)),
                                 ("quantile", quantile_edges(sample, ne))):
                for lname, labels in (("plain", None), ("labels", lab)):
                    name = "H %d %s %s" % (ne, place, lname)
                    planes = 1 if labels is None else 2
                    buf = torch.empty(planes * (ne + 2), dtype=torch.int64, device=dev)
                    arms[name] = (edges, labels, buf)
                    ctx.dist_histogram_device(buf.data_ptr(), edges, labels=labels, **kw)  # warm-up, and the counts held to the pairs
                    torch.cuda.synchronize()
                    c = buf.cpu().numpy().reshape(planes, ne + 2)
                    assert int(c.sum()) == span, name
                    largest[name] = round(float(c.sum(axis=0).max()) / span, 6)
        times = {"A": [], **{k: [] for k in arms}}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)
            times["A"].append(time.perf_counter() - t0)
            for name, (edges, labels, buf) in arms.items():
                t0 = time.perf_counter()
                ctx.dist_histogram_device(buf.data_ptr(), edges, labels=labels, **kw)
                times[name].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
        rec = {"shape": shape, "n": n, "p": p, "pairs": span, "reps": a.reps, "measure": "MASH_DIST k=31",
               "ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
               "median_ms": {k: round(v, 3) for k, v in med.items()},
               "H_minus_A_ms": {k: round(med[k] - med["A"], 3) for k in arms},
               "largest_class_share": largest,
               "spread_A_ms": round((max(times["A"]) - min(times["A"])) * 1e3, 3), "dense_sources_sha256": source_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_hist.jsonl"), "a") as f:
                f.write(line + "\n")
        del dense, regs, arms
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
