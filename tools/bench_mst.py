#!/usr/bin/env python3
"""Times the minimum spanning tree of the pair values against the threshold clusters and the dense path they are both built
on, in ONE process, alternating arms, device-resident sketches, a synchronise inside every timed region,
medians of --reps:
  A  dist_rows_device over the full triangle (the dense path; its sources are hashed into the output)
  C  cluster_threshold_device at the median value: one dense pass + k_cc_band.  k_cc_band's own time is not measured by the
     library: C - A stands for it, as in tools/bench_cluster.py
  M  mst (no cutoff): `rounds` rounds of labels + k_mst_band over every band + picks + emit, and the sort on the host
and, in a second pass with profiling on (its timers wait after every band, so its totals are not used), the device time of
the k_mst_band launches of one call (dsh_get_info "mst_band_us").  Per shape one JSON line on stdout (and into
--out DIR/bench_mst.jsonl): rounds, edges, the medians, k_mst_band per round, M against rounds x C.

  python tools/bench_mst.py --shapes c2,100k --reps 5 --out profiles/mst1"""
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
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)  # warm-up, and the threshold's source
        sample = dense[:: max(span // (1 << 24), 1)].cpu().numpy()
        t = float(np.quantile(sample, 0.5))
        clusters = ctx.cluster_threshold_device(labels.data_ptr(), t, **kw)  # warm-up of C
        lhs, rhs, val = ctx.mst(**kw)  # warm-up of M
        rounds = ctx.info("mst_rounds")
        torch.cuda.synchronize()
        times = {"A": [], "C": [], "M": []}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)
            times["A"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            nc = ctx.cluster_threshold_device(labels.data_ptr(), t, **kw)
            times["C"].append(time.perf_counter() - t0)
            assert nc == clusters
            t0 = time.perf_counter()
            again = ctx.mst(**kw)
            times["M"].append(time.perf_counter() - t0)
            assert ctx.info("mst_rounds") == rounds and all(np.array_equal(x, y) for x, y in zip(again, (lhs, rhs, val)))
        ctx.set_profiling(True)
        ctx.mst(**kw)
        band_ms = ctx.info("mst_band_us") / 1e3
        ctx.set_profiling(False)
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
        rec = {"shape": shape, "n": n, "p": p, "pairs": span, "reps": a.reps, "measure": "MASH_DIST k=31", "threshold_C": t,
               "clusters_C": clusters, "mst_edges": int(lhs.size), "mst_rounds": rounds,
               "one_band": bool(span * 4 <= (1 << 30)),
               "ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
               "median_ms": {k: round(v, 3) for k, v in med.items()},
               "C_minus_A_ms": round(med["C"] - med["A"], 3),
               "k_mst_band_ms_per_call": round(band_ms, 3), "k_mst_band_ms_per_round": round(band_ms / max(rounds, 1), 3),
               "k_mst_band_over_C_minus_A": round(band_ms / max(rounds, 1) / max(med["C"] - med["A"], 1e-9), 3),
               "rounds_x_C_ms": round(rounds * med["C"], 3), "M_over_rounds_x_C": round(med["M"] / max(rounds * med["C"], 1e-9), 3),
               "spread_A_ms": round((max(times["A"]) - min(times["A"])) * 1e3, 3), "dense_sources_sha256": source_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_mst.jsonl"), "a") as f:
                f.write(line + "\n")
        del dense, regs, labels
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
