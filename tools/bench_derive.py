#!/usr/bin/env python3
"""Times the derived-sketch kernels against a device-to-device copy of the same source bytes, in ONE
process, alternating, device-resident inputs far larger than the caches, HIP events on the context's stream around every
call, warm-up, median of the repeats:
  fold   100 000 x p=14 -> 10 and 10 000 x p=17 -> 14                         (dsh_fold_device)
  union  100 000 x p=14 into 1 000 groups of 100, and into one group of 50 000 plus 50 000 singletons
                                                                                (dsh_union_groups_device)
  copy   dsh_copy_sketches_device of the same rows (hipMemcpyAsync device to device on the same stream)
Byte model: a copy moves 2 bytes per source byte, fold 1 + 2^-d, union 1 + groups/members.  The bound each point is held
against: its time is at most the copy's.  One JSON line per point on stdout and into --out DIR/bench.jsonl (with a README.md that tabulates them).

  python tools/bench_derive.py --reps 7 --out DIR"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOURCES = ["kernels_derive.hip", "derive.hip"]


def source_hashes():
    out = {}
    for f in SOURCES:
        with open(os.path.join(ROOT, "dashing_amd", "csrc", f), "rb") as h:
            out[f] = hashlib.sha256(h.read()).hexdigest()[:16]
    return out


def law_on_device(torch, dev, n, p, seed):
    """n rows of the register law of synth.hll_registers (cardinalities 0.5 .. 4 x 2^p), drawn on the device"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    m = 1 << p
    out = torch.empty((n, m), dtype=torch.uint8, device=dev)
    step = max((1 << 26) // m, 1)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        u = torch.rand((r1 - r0, m), generator=g, device=dev, dtype=torch.float32).clamp_(1e-30, 1 - 1e-7)
        card = (0.5 + 3.5 * torch.rand((r1 - r0, 1), generator=g, device=dev)) * m
        v = torch.ceil(torch.log2((card / m) / (-torch.log(u))))
        out[r0:r1] = v.clamp_(0, 64 - p + 1).to(torch.uint8)
    return out


def csr(groups_sizes, members):
    gp = np.zeros(len(groups_sizes) + 1, np.uint64)
    gp[1:] = np.cumsum(groups_sizes)
    return gp, np.ascontiguousarray(members, np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
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

    def measure(arms):
        """arms: name -> callable; alternating; ms per repeat"""
        for _ in range(a.warmup):
            for fn in arms.values():
                fn()
        t = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                t[k].append(timed(fn))
        return t

    lines = []

    def report(name, n, p, src_bytes, moved, t, extra):
        ms, cp = float(np.median(t["op"])), float(np.median(t["copy"]))
        rec = {"point": name, "n": n, "p": p, "source_bytes": src_bytes, "model_bytes": moved, "reps": a.reps,
               "ms": round(ms, 4), "copy_ms": round(cp, 4), "ratio_to_copy": round(ms / cp, 3), "within_bound": ms <= cp,
               "TBps": round(moved / ms / 1e9, 3), "copy_TBps": round(2 * src_bytes / cp / 1e9, 3),
               "ms_all": [round(x, 4) for x in t["op"]], "copy_ms_all": [round(x, 4) for x in t["copy"]],
               "sources_sha256": source_hashes()}
        rec.update(extra)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for n, p, new_p, seed in ((int(100_000 * a.scale), 14, 10, 1), (int(10_000 * a.scale), 17, 14, 2)):
        regs = law_on_device(torch, dev, n, p, seed)
        src_bytes = n << p
        out = torch.empty(n << new_p, dtype=torch.uint8, device=dev)
        cpy = torch.empty(src_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.attach_device(regs.data_ptr(), n, p)
        t = measure({"op": lambda: ctx.fold_device(out.data_ptr(), new_p), "copy": lambda: ctx.copy_sketches_device(cpy.data_ptr())})
        report("fold %dx p=%d->%d" % (n, p, new_p), n, p, src_bytes, src_bytes + (n << new_p), t, {"new_p": new_p})
        if p == 14:  # the unions run over the same matrix
            rng = np.random.default_rng(3)
            perm = rng.permutation(n)
            ng = max(n // 100, 1)
            shapes = {"union %d x p=14, %d groups of %d" % (n, ng, n // ng): csr([n // ng] * ng, perm[: ng * (n // ng)]),
                      "union %d x p=14, one group of %d + %d singletons" % (n, n // 2, n - n // 2): csr([n // 2] + [1] * (n - n // 2), perm)}
            del out
            for name, (gp, mem) in shapes.items():
                groups, members = gp.size - 1, int(gp[-1])
                uout = torch.empty(groups << p, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                read = members << p
                cview = cpy[:read]
                t = measure({"op": lambda: ctx.union_groups_device(uout.data_ptr(), gp, mem),
                             "copy": lambda: ctx.copy_sketches_device(cview.data_ptr(), 0, members)})
                report(name, n, p, read, read + (groups << p), t, {"groups": groups, "members": members})
                del uout
        ctx.alloc(2, 10)
        del regs, cpy
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bench.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(a.out, "README.md"), "w") as f:
            f.write("Derived sketches (DESIGN.md section 4.9), one MI355X.\n"
                    "- `bench.jsonl`: `python tools/bench_derive.py --reps %d --out %s` -- per point the median call time (HIP events on\n"
                    "  the context's stream), the time of a device-to-device copy of the same source bytes in the same run, their\n"
                    "  ratio (the bound: at most 1), the bytes of the traffic model and the achieved TB/s, with the hashes of the sources\n"
                    "\n| point | ms | copy ms | ratio | TB/s | within the bound |\n|---|---|---|---|---|---|\n" % (a.reps, a.out))
            for line in lines:
                r = json.loads(line)
                f.write("| %s | %.3f | %.3f | %.2f | %.2f | %s |\n" % (r["point"], r["ms"], r["copy_ms"], r["ratio_to_copy"], r["TBps"],
                                                                  "yes" if r["within_bound"] else "NO"))


if __name__ == "__main__":
    main()
