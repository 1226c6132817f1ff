#!/usr/bin/env python3
"""Times dsh_greedy_extend*  against the full greedy call it continues and the dense path both are built on,
in ONE process, alternating arms, device-resident sketches, a synchronise inside every timed region (every call waits for
the device at its end), medians of --reps:
  A      dist_rows_device over the full triangle (the dense path; its sources are hashed into the output)
  G      greedy_threshold_device on all n slots: the yardstick
  E10    greedy_extend_device, FIRST, the last 10 % of the slots new, fed the first 90 % of G's labels
  E1     the same with 1 % new
  B      greedy_extend_device, BEST, from scratch (first_new = 0), against G
  EB10   greedy_extend_device, BEST, 10 % new, fed the first 90 % of B's labels
at thresholds giving about 0.1 %, 1 % and 50 % hits, and one that nothing passes.  Beside E / G the output carries the
pair-count ratio (m (n - m) + (n - m)^2 / 2) / (n^2 / 2) -- 0.19 and 0.02 -- which E / G would equal if a pair cost the same
in a rectangle as in the triangle, and the share of the old rows the bands of phase 1 compute.  Every extend arm's labels
are compared with the full call's before anything is timed.  One JSON line per shape on stdout (and into
--out DIR/bench_greedy_extend.jsonl).  --rates restricts the run to some rates, --arms to some arms, for a kernel trace.

  python tools/bench_greedy_extend.py --shapes c2,100k --reps 5 --out profiles/greedy_extend1"""
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
    ap.add_argument("--rates", default="0.1%,1%,50%,none")
    ap.add_argument("--arms", default="A,G,E10,E1,B,EB10")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import dashing_amd as D

    torch.cuda.init()
    dev = torch.device("cuda:0")
    ctx = D.Context(0)
    kw = dict(result_type=D.MASH_DIST, k=31)
    arms = a.arms.split(",")
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
        m10, m1 = n - n // 10, n - n // 100
        ratio = {str(m): (m * (n - m) + (n - m) * (n - m - 1) / 2) / (n * (n - 1) / 2) for m in (m10, m1)}

        def host_labels():
            return labels.cpu().numpy().view(np.uint32).copy()

        hits, reps, full, fullb, old_rows, differ = {}, {}, {}, {}, {}, {}
        for name, t in ts.items():  # warm-up of every arm, and the inputs and expectations of the extend arms
            ctx.dist_threshold_device(rp.data_ptr(), 0, 0, 0, t, 0, n, **kw)
            hits[name] = int(rp[-1].item())
            reps[name] = ctx.greedy_threshold_device(labels.data_ptr(), t, **kw)
            full[name] = host_labels()
            assert ctx.greedy_extend_device(labels.data_ptr(), t, 0, None, "best", **kw) == reps[name]
            fullb[name] = host_labels()
            differ[name] = int((fullb[name] != full[name]).sum())
            for m in (m10, m1):
                assert ctx.greedy_extend_device(labels.data_ptr(), t, m, full[name][:m], "first", **kw) == reps[name]
                assert np.array_equal(host_labels(), full[name]), (shape, name, m)
                r = np.flatnonzero(full[name][:m] == np.arange(m))
                old_rows[name + " " + str(m)] = int(r.size)
            assert ctx.greedy_extend_device(labels.data_ptr(), t, m10, fullb[name][:m10], "best", **kw) == reps[name]
            assert np.array_equal(host_labels(), fullb[name]), (shape, name, "best")
        assert "none" not in ts or (hits["none"] == 0 and reps["none"] == n)
        torch.cuda.synchronize()

        def run(arm, name, t):
            if arm == "A":
                return ctx.dist_rows_device(dense.data_ptr(), 0, n, **kw)
            if arm == "G":
                return ctx.greedy_threshold_device(labels.data_ptr(), t, **kw)
            if arm == "E10":
                return ctx.greedy_extend_device(labels.data_ptr(), t, m10, full[name][:m10], "first", **kw)
            if arm == "E1":
                return ctx.greedy_extend_device(labels.data_ptr(), t, m1, full[name][:m1], "first", **kw)
            if arm == "B":
                return ctx.greedy_extend_device(labels.data_ptr(), t, 0, None, "best", **kw)
            if arm == "EB10":
                return ctx.greedy_extend_device(labels.data_ptr(), t, m10, fullb[name][:m10], "best", **kw)
            raise ValueError(arm)

        times = {"A": []} if "A" in arms else {}
        times.update({arm + " " + k: [] for k in ts for arm in arms if arm != "A"})
        for _ in range(a.reps):
            if "A" in arms:
                t0 = time.perf_counter()
                run("A", None, None)  # (synchronous, as every arm is: each waits for the device)
                times["A"].append(time.perf_counter() - t0)
            for name, t in ts.items():
                for arm in arms:
                    if arm == "A":
                        continue
                    t0 = time.perf_counter()
                    nr = run(arm, name, t)
                    times[arm + " " + name].append(time.perf_counter() - t0)
                    assert nr == reps[name]
        med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}

        def per_rate(f):
            out = {}
            for k in ts:
                try:
                    out[k] = round(f(k), 4)
                except KeyError:
                    pass
            return out

        rec = {"shape": shape, "n": n, "p": p, "pairs": span, "reps": a.reps, "measure": "MASH_DIST k=31", "thresholds": ts,
               "hits": hits, "representatives": reps, "labels_best_differs_from_first": differ,
               "first_new": {"E10": m10, "E1": m1}, "pair_count_ratio": {"E10": round(ratio[str(m10)], 4), "E1": round(ratio[str(m1)], 4)},
               "old_representatives": old_rows,
               "ms": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
               "median_ms": {k: round(v, 3) for k, v in med.items()},
               "E10_over_G": per_rate(lambda k: med["E10 " + k] / med["G " + k]),
               "E1_over_G": per_rate(lambda k: med["E1 " + k] / med["G " + k]),
               "EB10_over_B": per_rate(lambda k: med["EB10 " + k] / med["B " + k]),
               "B_minus_G_ms": per_rate(lambda k: med["B " + k] - med["G " + k]),
               "G_minus_A_ms": per_rate(lambda k: med["G " + k] - med["A"]),
               "dense_sources_sha256": source_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_greedy_extend.jsonl"), "a") as f:
                f.write(line + "\n")
        del dense, regs, labels
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
