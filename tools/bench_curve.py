#!/usr/bin/env python3
"""Times the union growth curve (dsh_union_curve_device) in ONE process, device-resident inputs, HIP events
on the context's stream around every call, warm-up, the arms alternating, median of the repeats:
  10 000 x p=14, one order and 100 permutations; 100 000 x p=10, one order and 20 permutations
Each shape is timed three ways:
  plan    the planner's segments ("curve_segment" = 0)
  single  one segment per order ("curve_segment" = len): the walk alone, no segment unions
  copy    device-to-device copies of n_orders x len x 2^p bytes (dsh_copy_sketches_device, n_orders times): the bytes the
          walk cannot avoid reading
No time is gated.  The one rule: at each shape `plan` must not be slower than `single` by more than three times the range
of the repeated runs (the larger of the two arms' ranges).  One JSON line per shape on stdout and into --out DIR/bench.jsonl
(with a README.md that tabulates them).

  python tools/bench_curve.py --reps 3 --out DIR"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_derive import law_on_device  # noqa: E402

SOURCES = ["kernels_curve.hip", "curve.hip", "curve_plan.h"]
SHAPES = [(10_000, 14, 1), (10_000, 14, 100), (100_000, 10, 1), (100_000, 10, 20)]


def source_hashes():
    out = {}
    for f in SOURCES:
        with open(os.path.join(ROOT, "dashing_amd", "csrc", f), "rb") as h:
            out[f] = hashlib.sha256(h.read()).hexdigest()[:16]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the row counts (a rehearsal; figures are then of no use)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import dashing_amd as D

    torch.cuda.init()
    dev = torch.device("cuda:0")
    ctx = D.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream, device=dev)

    def timed(fn):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record(stream)
        fn()
        end.record(stream)
        end.synchronize()
        return beg.elapsed_time(end)

    lines = []
    regs, have = None, None
    for n0, p, n_orders in SHAPES:
        n = max(int(n0 * a.scale), 2)
        if have != (n, p):
            del regs
            torch.cuda.empty_cache()
            regs = law_on_device(torch, dev, n, p, 7 + p)
            cpy = torch.empty(n << p, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.attach_device(regs.data_ptr(), n, p)
            have = (n, p)
        orders = np.concatenate([np.arange(n, dtype=np.uint32)[None], D.curve_permutations(n, n_orders - 1, 1)])
        d_ord = torch.from_numpy(orders.view(np.int32).copy()).to(dev)
        d_card = torch.zeros(n_orders * n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def curve(seg):
            ctx.set_option("curve_segment", seg)
            ctx.union_curve_device(d_ord.data_ptr(), n, n_orders, d_card.data_ptr())

        def copies():
            for _ in range(n_orders):
                ctx.copy_sketches_device(cpy.data_ptr())

        arms = {"plan": lambda: curve(0), "single": lambda: curve(n), "copy": copies}
        for _ in range(a.warmup):
            for fn in arms.values():
                fn()
        t = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                t[k].append(timed(fn))
        ctx.set_option("curve_segment", 0)
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = max(max(t[k]) - min(t[k]) for k in ("plan", "single"))
        row_bytes = n_orders * n << p
        rec = {"point": "%d x p=%d, %d order%s" % (n, p, n_orders, "" if n_orders == 1 else "s"), "n": n, "p": p, "n_orders": n_orders,
               "row_bytes": row_bytes, "delta_bytes": n_orders * n * 256, "reps": a.reps,
               "plan_ms": round(med["plan"], 4), "single_ms": round(med["single"], 4), "copy_ms": round(med["copy"], 4),
               "plan_to_copy": round(med["plan"] / med["copy"], 3), "plan_row_TBps": round(row_bytes / med["plan"] / 1e9, 3),
               "range_ms": round(spread, 4), "plan_not_slower": med["plan"] <= med["single"] + 3 * spread,
               "final_card": float(d_card[n - 1].item()),
               "ms_all": {k: [round(x, 4) for x in v] for k, v in t.items()}, "sources_sha256": source_hashes()}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del d_ord, d_card
    ctx.alloc(2, 10)
    ctx.close()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(a.out, "README.md"), "w") as f:
            f.write("Union growth curves (DESIGN.md section 4.18), one MI355X.\n"
                    "- `bench.jsonl`: `python tools/bench_curve.py --reps %d --out %s` -- per shape the median time of\n"
                    "  dsh_union_curve_device (HIP events on the context's stream) with the planner's segments and with one segment\n"
                    "  per order, the time of device-to-device copies of the rows the walk reads in the same run, and the rule: the\n"
                    "  planner's choice is not slower than one segment by more than three times the range of the repeats\n"
                    "\n| shape | plan ms | single ms | copy ms | plan / copy | range ms | rule holds |\n|---|---|---|---|---|---|---|\n" % (a.reps, a.out))
            for line in lines:
                r = json.loads(line)
                f.write("| %s | %.3f | %.3f | %.3f | %.2f | %.3f | %s |\n" % (r["point"], r["plan_ms"], r["single_ms"], r["copy_ms"], r["plan_to_copy"],
                                                                             r["range_ms"], "yes" if r["plan_not_slower"] else "NO"))


if __name__ == "__main__":
    main()
