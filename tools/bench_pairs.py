#!/usr/bin/env python3
"""Times the explicit pair list against the dense path, in ONE process, alternating, device-resident
sketches, a synchronise inside every timed region:
  A  dist_rows_device over the full triangle (the dense path, unchanged; its sources are hashed into the output)
  B  dist_pairs_device for the hits of dist_threshold_device at about 0.01 %, 0.1 %, 1 % and 10 % of all pairs, in CSR
     order (runs of equal rhs) and shuffled, with one measure and with four
A list is cut at --max-pairs pairs (the rate is what is measured; the time of the whole share follows from it).  Per
point: pairs/s, bytes/s of the byte model (2 * 2^p per pair) and the break-even share = the share of all pairs at which
B, at that rate, takes as long as A.  One JSON line per shape on stdout (and into --out DIR/bench_pairs.jsonl).

  python tools/bench_pairs.py --shapes c2,100k --reps 5 --out profiles/pairs1"""
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

SOURCES = ["kernels_compare.hip", "engine.hip", "plan.cpp", "plan.h", "estimators.h", "kernels_pairs.hip", "pairs.hip"]
SHARES = (("0.01%", 1e-4), ("0.1%", 1e-3), ("1%", 1e-2), ("10%", 1e-1))


def source_hashes():
    out = {}
    for f in SOURCES:
        with open(os.path.join(ROOT, "dashing_amd", "csrc", f), "rb") as h:
            out[f] = hashlib.sha256(h.read()).hexdigest()[:16]
    return out


def collection(torch, dev, shape):
    from dashing_amd import synth

    if shape == "c2":  # BASELINE configs[2]
        return torch.from_numpy(synth.survey_sketches(10_000, 14, seed=0x5EED0000)[0]).to(dev), 10_000, 14
    from test_gpu_configs import derived_collection

    if shape == "100k":
        return derived_collection(torch, dev, 100_000, 10, 4_000, seed=0x5EED1000), 100_000, 10
    raise SystemExit("unknown shape %s" % shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-pairs", type=int, default=4_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import dashing_amd as D

    torch.cuda.init()
    dev = torch.device("cuda:0")
    ctx = D.Context(0)
    one, four = (D.JI,), (D.JI, D.MASH_DIST, 5, 2)
    for shape in a.shapes.split(","):
        regs, n, p = collection(torch, dev, shape)
        ctx.attach_device(regs.data_ptr(), n, p)
        span = D.tri_span(n, 0, n)
        dense = torch.empty(span, dtype=torch.float32, device=dev)
        rp = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ctx.dist_rows_device(dense.data_ptr(), 0, n, result_type=D.MASH_DIST, k=31)  # warm-up, and the thresholds' source
        sample = dense[:: max(span // (1 << 24), 1)].cpu().numpy()
        lists = {}
        for name, share in SHARES:
            t = float(np.quantile(sample, share))
            ctx.dist_threshold_device(rp.data_ptr(), 0, 0, 0, t, 0, n, result_type=D.MASH_DIST, k=31)
            hits = int(rp[-1].item())
            col = torch.empty(max(hits, 1), dtype=torch.int32, device=dev)
            val = torch.empty(max(hits, 1), dtype=torch.float32, device=dev)
            ctx.dist_threshold_device(rp.data_ptr(), col.data_ptr(), val.data_ptr(), hits, t, 0, n, result_type=D.MASH_DIST, k=31)
            m = min(hits, a.max_pairs)
            rows = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), (rp[1:] - rp[:-1]))[:m].contiguous()
            col = col[:m].contiguous()
            perm = torch.randperm(m, device=dev)
            # the CSR round trip on the way: Mash distance of the listed pairs is `val`
            chk = torch.empty(m, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
            ctx.dist_pairs_device(col.data_ptr(), rows.data_ptr(), m, chk.data_ptr(), (D.MASH_DIST,), k=31)
            assert torch.equal(chk.view(torch.int32), val[:m].view(torch.int32)), "pairs differ from the thresholded values"
            lists[name] = {"hits": hits, "m": m, "csr": (col, rows), "shuffled": (col[perm].contiguous(), rows[perm].contiguous()),
                           "out": torch.empty(4 * m, dtype=torch.float32, device=dev)}
            del val
        torch.cuda.synchronize()
        # the first pairs call after the sketches changed also computes the path's cardinalities of all n sketches
        cold = []
        for _ in range(a.reps):
            ctx.attach_device(regs.data_ptr(), n, p)
            lhs, rhs = lists["0.01%"]["csr"]
            t0 = time.perf_counter()
            torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
            ctx.dist_pairs_device(lhs.data_ptr(), rhs.data_ptr(), lists["0.01%"]["m"], lists["0.01%"]["out"].data_ptr(), one, k=31)
            cold.append(time.perf_counter() - t0)
        times = {"A": []}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.dist_rows_device(dense.data_ptr(), 0, n, result_type=D.MASH_DIST, k=31)
            times["A"].append(time.perf_counter() - t0)
            for name, L in lists.items():
                for order in ("csr", "shuffled"):
                    for tn, types in (("1", one), ("4", four)):
                        lhs, rhs = L[order]
                        t0 = time.perf_counter()
                        torch.cuda.synchronize()  # (torch fills its buffers on a stream of its own)
                        ctx.dist_pairs_device(lhs.data_ptr(), rhs.data_ptr(), L["m"], L["out"].data_ptr(), types, k=31)
                        times.setdefault("B %s %s x%s" % (name, order, tn), []).append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        points = {}
        for key, s in med.items():
            if key == "A":
                continue
            m = lists[key.split()[1]]["m"]
            rate = m / s
            points[key] = {"pairs": m, "ms": round(s * 1e3, 3), "pairs_per_s": round(rate), "model_GBps": round(rate * 2 * (1 << p) / 1e9, 1),
                           "break_even_share": round(med["A"] * rate / span, 5)}
        rec = {"shape": shape, "n": n, "p": p, "all_pairs": span, "reps": a.reps, "A_measure": "MASH_DIST k=31",
               "hits": {k: v["hits"] for k, v in lists.items()}, "median_A_ms": round(med["A"] * 1e3, 3),
               "spread_A_ms": round((max(times["A"]) - min(times["A"])) * 1e3, 3), "A_ms": [round(x * 1e3, 3) for x in times["A"]],
               "first_call_0.01%_ms": round(float(np.median(cold)) * 1e3, 3), "B": points, "sources_sha256": source_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "bench_pairs.jsonl"), "a") as f:
                f.write(line + "\n")
        del dense, regs, lists
        ctx.alloc(2, 10)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
