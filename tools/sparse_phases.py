#!/usr/bin/env python3
"""Where k_sparse_count_lds spends its time, and what a run length costs: the counting kernel's own time (HIP events:
set_profiling, info sparse_plane_us) on the bench workload per option set, best of three calls on a freshly attached matrix.

    python tools/sparse_phases.py [--shapes 10000x14,5000x15] [--runs 1,2,4,8,16] [--words 0] [--caps 1280] [--stops 0] [--reps 3]

--words: the table words a workgroup stages (option sparse_words: 1, 2, or 0 = the library's choice, which also measures a
library from before the option).

--stops 1,2,3,0 needs the measuring build (make -C dashing_amd/csrc SPCUT=1: the kernel reads DSH_SPARSE_STOP at every
launch and leaves each item after the fill / the walk / the lanes' addition; results are then meaningless).  On the product
library the variable does nothing and every stop gives the whole kernel.  One JSON line per (shape, cap, run, stop)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import dashing_amd  # noqa: E402
from dashing_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="10000x14")
ap.add_argument("--runs", default="1,2,4,8,16")
ap.add_argument("--words", default="0")
ap.add_argument("--caps", default="1280")
ap.add_argument("--stops", default="0")
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()


def info(ctx, key):
    try:
        return ctx.info(key)
    except Exception:
        return None


for shape in args.shapes.split(","):
    n, p = (int(x) for x in shape.split("x"))
    regs = torch.from_numpy(synth.survey_sketches(n, p)[0]).cuda()
    out = torch.empty(n * (n - 1) // 2, dtype=torch.float32, device="cuda")
    for cap in (int(x) for x in args.caps.split(",")):
        ctx = dashing_amd.Context(0)
        ctx.set_profiling(True)
        ctx.set_option("sparse_cap", cap)  # (before the matrix is attached: the per-sketch pass runs at this cap)
        for run, words in ((int(x), int(y)) for x in args.runs.split(",") for y in args.words.split(",")):
            if run:  # (0: the library's default, and a library from before the option can be measured)
                ctx.set_option("sparse_run", run)
            if words:
                ctx.set_option("sparse_words", words)
            for stop in (int(x) for x in args.stops.split(",")):
                os.environ["DSH_SPARSE_STOP"] = str(stop)
                best, pair = 1e9, 1e9
                for _ in range(args.reps):
                    ctx.attach_device(regs.data_ptr(), n, p)
                    ctx.dist_rows_device(out.data_ptr(), 0, n, 2)
                    ctx.synchronize()
                    best = min(best, ctx.info("sparse_plane_us") / 1000.0)
                    pair = min(pair, ctx.last_kernel_ms()["pair_ms"])
                print(json.dumps({"n": n, "p": p, "sparse_cap": cap, "sparse_run": info(ctx, "sparse_run"), "sparse_words": info(ctx, "sparse_words"),
                                  "stop(1 fill,2 +walk,3 +lanes,0 all)": stop,
                                  "sparse_count_ms": round(best, 4), "pair_ms": round(pair, 3), "sparse_items": ctx.info("sparse_items"),
                                  "sparse_transposed_items": ctx.info("sparse_transposed_items"), "sparse_slabs": ctx.info("sparse_slabs"),
                                  "sparse_table_fills": info(ctx, "sparse_table_fills"), "bands": ctx.info("bands")}), flush=True)
        os.environ.pop("DSH_SPARSE_STOP", None)
        ctx.close()
