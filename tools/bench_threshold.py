#!/usr/bin/env python3
"""Times the thresholded output against the dense path it is built on, in ONE process, alternating,
device-resident sketches, a synchronise inside every timed region:
  A  dist_rows_device over the full triangle (the dense path; its sources are hashed into the output)
  B  dist_threshold_device over the same rows at thresholds giving about 0.1 %, 1 % and 50 % hits
  C  a device-to-device copy of the dense span, twice: the floor of the selection's two reads
One JSON line per shape on stdout (and into --out DIR/bench_threshold.jsonl).

  python tools/bench_threshold.py --shapes c2,100k --reps 5 --out profiles/thr1"""
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

DENSE_SOURCES = ["kernels_compare.hip", "engine.hip", "plan.cpp", "plan.h", "estimators.h"]


def source_hashes():
    out = {}
    for f in DENSE_SOURCES:
        with open(os.path.join(ROOT, "dashing_amd", "csrc", f), "rb") as h:
            out[f] = hashlib.sha256(h.read()).hexdigest()[:16]
    return out


def collection(torch, dev, shape):
    from dashing_amd import synth

    if shape == "c2":  # BASELINE configs[2]
        return torch.from_numpy(synth.survey_sketches(10_000, 14, seed=0x5EED0000)[0]).to(dev), 10_000, 14, None
    from test_gpu_configs import derived_collection

    if shape == "100k":
        return derived_collection(torch, dev, 100_000, 10, 4_000, seed=0x5EED1000), 100_000, 10, None
    if shape == "60k":  # a 60 000-row slice at p = 14: the first 6 000 rows of it
        return derived_collection(torch, dev, 60_000, 14, 4_000, seed=0x5EED3000), 60_000, 14, 6_000
    raise SystemExit("unknown shape %s" % shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import dashing_amd as D

    torch.cuda.init()
    dev = torch.device("cuda:0")
    ctx = D.Context(0)
    for shape in a.shapes.split(","):
        regs, n, p, rows = collection(torch, dev, shape)
        re = n if rows is None else rows
        ctx.attach_device(regs.data_ptr(), n, p)
        span = D.tri_span(n, 0, re)
        dense = torch.empty(span, dtype=torch.float32, device=dev)
        copy = torch.empty(span, dtype=torch.float32, device=dev)
        rp = torch.empty(re + 1, dtype=torch.int64, device=dev)
        ctx.dist_rows_device(dense.data_ptr(), 0, re, result_type=D.MASH_DIST, k=31)  # warm-up, and the thresholds' source
        sample = dense[:: max(span // (1 << 24), 1)].cpu().numpy()
        ts = {name: float(np.quantile(sample, q)) for name, q in (("0.1%", 0.001), ("1%", 0.01), ("50%", 0.5))}
        bufs = {}
        for name, t in ts.items():
            try:
                ctx.dist_threshold_device(rp.data_ptr(), 0, 0, 0, t, 0, re, result_type=D.MASH_DIST, k=31)
                hits = int(rp[-1].item())
            except D.DshError as e:
                raise SystemExit(str(e))
            bufs[name] = (hits, torch.empty(max(hits, 1), dtype=torch.int32, device=dev), torch.empty(max(hits, 1), dtype=torch.float32, device=dev))
        torch.cuda.synchronize()
        times = {"A": [], "C": [], **{"B " + k: [] for k in ts}}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.dist_rows_device(dense.data_ptr(), 0, re, result_type=D.MASH_DIST, k=31)
            times["A"].append(time.perf_counter() - t0)
            for name, t in ts.items():
                hits, col, val = bufs[name]
                t0 = time.perf_counter()
                got = ctx.dist_threshold_device(rp.data_ptr(), col.data_ptr(), val.data_ptr(), hits, t, 0, re, result_type=D.MASH_DIST, k=31)
                times["B " + name].append(time.perf_counter() - t0)
                assert got == hits
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            copy.copy_(dense)
            copy.copy_(dense)
            torch.cuda.synchronize()
            times["C"].append(time.perf_counter() - t0)
        rec = {"shape": shape, "n": n, "p": p, "rows": re, "pairs": span, "reps": a.reps, "measure": "MASH_DIST k=31",
               "thresholds": ts, "hits": {k: v[0] for k, v in bufs.items()},
               "ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
               "median_ms": {k: round(float(np.median(v)) * 1e3, 3) for k, v in times.items()},
               "spread_A_ms": round((max(times["A"]) - min(times["A"])) * 1e3, 3), "dense_sources_sha256": source_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_threshold.jsonl"), "a") as f:
                f.write(line + "\n")
        del dense, copy, regs
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
