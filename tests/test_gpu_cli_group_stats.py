"""GPU: `dashing-amd dist --cluster T --stats` and `--representatives T --assign best --stats`, text and -b, parsed back and
held to Context.group_stats on the same sketches and labels; the output without --stats is a byte-exact prefix of the
output with it (so every byte the other CLI tests expect stays); the refusals."""
import os

import numpy as np
import pytest

import dashing_amd
from test_gpu_cli_greedy import cli, hlls  # noqa: F401  (hlls: the 40 .hll files of that module)
from test_gpu_cli_greedy_extend import load_regs

pytestmark = pytest.mark.gpu
D = dashing_amd
CASES = [((), D.JI, (0.5, 0.02, 1.5)), (("-M",), D.MASH_DIST, (0.03, 0.2, -1.0))]
MODES = [("--cluster", ()), ("--representatives", ("--assign", "best"))]


def parse_stats_bin(raw, n):
    """u64 n, u64 count, u32 labels[n] | u32 medoid[n], u32 cnt[n], i64 sum[n], f32 worst[n]"""
    assert len(raw) == 16 + 4 * n + 20 * n and int(np.frombuffer(raw[:8], np.uint64)[0]) == n
    at = 16
    out = []
    for dt in (np.uint32, np.uint32, np.uint32, np.int64, np.float32):
        out.append(np.frombuffer(raw[at : at + n * np.dtype(dt).itemsize], dt))
        at += n * np.dtype(dt).itemsize
    return out


@pytest.mark.parametrize("mode,extra", MODES)
@pytest.mark.parametrize("flags,rt,ts", CASES)
def test_stats_equal_the_api(ctx, hlls, tmp_path, flags, rt, ts, mode, extra):
    """per threshold four runs of the tool (text and -b, with and without --stats); the thresholds: one that joins the
    families, one that nothing passes (every input alone: '-' and nan)"""
    d, names = hlls
    n = len(names)
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", *names, *flags]
    ctx.set_sketches(load_regs(d, names))
    sizes = set()
    for t in ts[1:]:
        plain_bin, with_bin = tmp_path / "plain.bin", tmp_path / "stats.bin"
        cli(*common, mode, t, *extra, "-b", "-O", plain_bin, "-o", os.devnull, cwd=d)
        cli(*common, mode, t, *extra, "--stats", "-b", "-O", with_bin, "-o", os.devnull, cwd=d)
        raw = with_bin.read_bytes()
        assert raw[: 16 + 4 * n] == plain_bin.read_bytes()  # without --stats every byte stays
        lab, med, cnt, sm, worst = parse_stats_bin(raw, n)
        want = ctx.group_stats(lab, estim=2, result_type=rt, k=31)
        for got, w in zip((med, cnt, sm, worst), want):
            assert got.tobytes() == w.tobytes(), (mode, t)
        sizes.add(np.unique(lab).size)
        # text: the fields of the run without --stats, then the medoid's name, the mean, the worst value
        plain = cli(*common, mode, t, *extra, "-o", os.devnull, cwd=d).stdout.decode().split("\n")
        out = cli(*common, mode, t, *extra, "--stats", "-o", os.devnull, cwd=d).stdout.decode().split("\n")
        assert out[-1] == "" and len(out) == n + 2 and out[0] == plain[0] and len(plain) == len(out)
        for x, (line, before) in enumerate(zip(out[1:-1], plain[1:-1])):
            f = line.split("\t")
            assert "\t".join(f[:-3]) == before and f[0] == names[x], line
            assert f[-3] == names[int(want.medoid[x])], line
            assert f[-2] == ("-" if want.cnt[x] == 0 else "%.6g" % want.mean[x]), line
            assert f[-1] == "%.6g" % want.worst[x], line
    assert max(sizes) == n and min(sizes) < n  # (every input alone, and real groups)


def test_refusals(hlls):
    d, names = hlls
    base = ["dist", "--presketched", "-S", 10, "-o", os.devnull]
    r = cli(*base, "--stats", *names[:5], cwd=d, ok=False)
    assert b"--stats goes with --cluster or --representatives" in r.stderr
    r = cli(*base, "--threshold", 0.5, "--stats", *names[:5], cwd=d, ok=False)
    assert b"--stats goes with --cluster or --representatives" in r.stderr
    for mode in ("--cluster", "--representatives"):
        r = cli(*base, mode, 0.5, "--stats", "--sizes", *names[:5], cwd=d, ok=False)
        assert b"--stats does not go with --sizes" in r.stderr
    assert b"--stats" in cli("dist", "--help", ok=False).stderr
