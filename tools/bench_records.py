#!/usr/bin/env python3
"""Per-record sketching rate (dsh_sketch_records_device) against the same records sketched as one genome each through
dsh_sketch_batch_device over rows cleared in the same timed call, bases already in HBM (as tools/bench_sketch.py).  One
JSON line per case: both rates (bases/s, records/s, median of --reps calls after one warm-up), the speed-up, and a
bit-exact check of a sample of records against the oracle.

    python tools/bench_records.py [--reps 5] [--cases all|NAME,...] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {  # name: (records, length or None for the log-uniform mix, p)
    "1M_x_150bp_p10": (1_000_000, 150, 10),
    "1M_x_1kbp_p10": (1_000_000, 1000, 10),
    "200k_x_1kbp_p14": (200_000, 1000, 14),
    "20k_x_10kbp_p14": (20_000, 10_000, 14),
    "100_x_5Mbp_p10": (100, 5_000_000, 10),
    "mix_100bp_1Mbp_p10": (2000, None, 10),
    "mix_100bp_1Mbp_p14": (2000, None, 14),
}


def timed(fn, ctx, reps):
    fn()
    ctx.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="all")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import dashing_amd
    from oracle import oracle_c

    torch.cuda.init()
    dev = torch.device("cuda", 0)
    names = list(CASES) if args.cases == "all" else args.cases.split(",")
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    out = open(args.out, "a") if args.out else None
    with dashing_amd.Context(0) as ctx:
        for name in names:
            n, L, p = CASES[name]
            rng = np.random.default_rng(7)
            if L is None:
                lens = np.exp(rng.uniform(np.log(100), np.log(1_000_000), n)).astype(np.uint64)
            else:
                lens = np.full(n, L, np.uint64)
            off = np.zeros(n + 1, np.uint64)
            off[1:] = np.cumsum(lens)
            total = int(off[-1])
            torch.manual_seed(1)
            seq = lut[torch.randint(0, 4, (total + 256,), device=dev)]
            torch.cuda.synchronize()
            ctx.alloc(n, p)
            t_rec = timed(lambda: ctx.sketch_records_device(seq.data_ptr(), off, 0, args.k, True), ctx, args.reps)
            # bit-exact sample against the oracle (rows of the records path)
            pick = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, args.sample)]))
            got = np.stack([ctx.download(int(i), 1)[0] for i in pick])
            sub = [seq[int(off[i]):int(off[i + 1])].cpu().numpy() for i in pick]
            soff = np.zeros(len(sub) + 1, np.uint64)
            soff[1:] = np.cumsum([s.size for s in sub])
            want = oracle_c.sketch_batch(np.concatenate(sub), soff, args.k, p, True)
            exact = bool((got == want).all())
            # (the baseline max-merges: like for like, its timed call clears the rows first, as the records path
            # overwrites them)
            def base():
                ctx.clear()
                ctx.sketch_batch_device(seq.data_ptr(), off, 0, args.k, True)

            t_base = timed(base, ctx, args.reps)
            r = {"case": name, "records": n, "bases": total, "p": p, "k": args.k,
                 "records_s": t_rec, "records_bases_per_s": total / t_rec, "records_per_s": n / t_rec,
                 "batch_s": t_base, "batch_bases_per_s": total / t_base, "batch_records_per_s": n / t_base,
                 "speedup": t_base / t_rec, "sample": int(pick.size), "bit_exact": exact}
            line = json.dumps(r)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
            del seq
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
