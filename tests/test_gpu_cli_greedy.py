"""GPU: `dashing-amd dist --representatives` against the sequential reference (tests/greedy_ref.py) over the pairs
`--threshold -b` emits for the same command line: text (names, cluster numbers, representatives, values) and -b."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import greedy_ref
from dashing_amd import synth
from test_gpu_cli_threshold import parse_bin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dashing_amd", "dashing-amd")


def cli(*args, cwd=None, ok=True):
    r = subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return r


def want_text(names, lab, rp, col, val, measure, op, t):
    """the value column is --threshold's value of the pair (label, x): hit of row `label` with column x"""
    reps = sorted(set(lab.tolist()))
    index = {r: i for i, r in enumerate(reps)}
    out = ["#Representatives\t%s\t%s\t%s" % (measure, op, "%.6g" % np.float32(t))]
    for x in range(len(names)):
        l = int(lab[x])
        if l == x:
            v = "-"
        else:
            h = int(rp[l]) + int(np.flatnonzero(col[int(rp[l]) : int(rp[l + 1])] == x)[0])
            v = "%.6g" % val[h]
        out.append("%s\t%d\t%s\t%s" % (names[x], index[l], names[l], v))
    return out


def parse_reps_bin(raw, n):
    hdr = np.frombuffer(raw[:16], np.uint64)
    assert int(hdr[0]) == n and len(raw) == 16 + 4 * n
    return np.frombuffer(raw[16:], np.uint32), int(hdr[1])


def check(common, names, flags, rt_name, op, thresholds, tmp_path, cwd=None):
    """for every threshold: the representatives equal the sequential pass over --threshold's pairs"""
    n = len(names)
    counts = []
    for t in thresholds:
        b = tmp_path / "thr.bin"
        cli(*common, *flags, "--threshold", t, "-b", "-O", b, "-o", os.devnull, cwd=cwd)
        rp, col, val = parse_bin(b.read_bytes())
        assert rp.size == n + 1
        lab, nr = greedy_ref.labels(n, rp, col)
        out = cli(*common, *flags, "--representatives", t, "-o", os.devnull, cwd=cwd).stdout.decode().split("\n")
        assert out[-1] == "" and out[:-1] == want_text(names, lab, rp, col, val, rt_name, op, t), t
        rb = tmp_path / "reps.bin"
        cli(*common, *flags, "--representatives", t, "-b", "-O", rb, "-o", os.devnull, cwd=cwd)
        got, gr = parse_reps_bin(rb.read_bytes(), n)
        assert np.array_equal(got, lab) and gr == nr, t
        counts.append(nr)
    return counts


@pytest.fixture(scope="module")
def hlls(tmp_path_factory):
    """40 .hll files at p = 10 in 8 families of 5: close inside a family, far between families (the recipe of
    tests/test_gpu_cli_cluster.py)"""
    host = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    host.dshh_write_hll.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    d = tmp_path_factory.mktemp("grhll")
    names = []
    for f in range(8):
        core = synth.hll_registers(0xC1A0 + f, 4000, 10)
        for i in range(5):
            name = "f%dm%d.hll" % (f, i)
            regs = np.maximum(core, synth.hll_registers(0x900 + 8 * f + i, 150 * (i + 1), 10))
            assert host.dshh_write_hll(str(d / name).encode(), regs.ctypes.data, 10, 2) == 0
            names.append(name)
    order = np.random.default_rng(3).permutation(len(names))  # families interleaved: a representative is not a neighbour
    return d, [names[i] for i in order]


@pytest.mark.parametrize("flags,rt_name,op,ts", [((), "JI", ">=", (0.5, 0.02, 1.5)), (("-M",), "MASH_DIST", "<=", (0.03, 0.2, -1.0))])
def test_presketched(hlls, tmp_path, flags, rt_name, op, ts):
    d, names = hlls
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", *names]
    counts = check(common, names, flags, rt_name, op, ts, tmp_path, cwd=d)
    assert 1 <= counts[0] < len(names) and counts[2] == len(names)  # some are covered; nothing passes


def test_groups_share_the_path(hlls, tmp_path):
    d, names = hlls
    groups = ["g%d" % (i % 10) for i in range(len(names))]
    (tmp_path / "groups.tsv").write_text("".join("%s\t%s\n" % (s, g) for s, g in zip(names, groups)))
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", "--groups", tmp_path / "groups.tsv", *names]
    check(common, ["g%d" % i for i in range(10)], ("-M",), "MASH_DIST", "<=", (0.05, 0.5), tmp_path, cwd=d)


def test_dist_by_seq(tmp_path):
    base = synth.synthetic_genomes(6, 30000, seed=0xB5E0)
    f = tmp_path / "multi.fna"
    f.write_bytes(b"".join(synth.to_fasta(g[: 20000 + 900 * i], "rec%d" % i) for i, g in enumerate(base)) + synth.to_fasta(base[1][:20900], "again"))
    names = ["rec%d" % i for i in range(6)] + ["again"]
    counts = check(["dist_by_seq", f], names, ("-M",), "MASH_DIST", "<=", (0.0, 0.1), tmp_path)
    assert counts[0] < 7  # rec1 and `again` are the same sequence: Mash 0


@pytest.mark.parametrize("extra,msg", [(("--cluster", "0.1"), "--cluster"), (("--threshold", "0.1"), "--threshold"),
                                       (("--nearest-neighbors", "2"), "--nearest-neighbors"), (("--pairs", "pairs.tsv"), "--pairs"),
                                       (("-Q", "q.txt"), "-Q"), (("-U",), "-U"), (("-T",), "-T"), (("--ngpus", "2"), "one device")])
def test_refusals(hlls, tmp_path, extra, msg):
    d, names = hlls
    (tmp_path / "q.txt").write_text(names[0] + "\n")
    (tmp_path / "pairs.tsv").write_text("%s\t%s\n" % (names[0], names[1]))
    r = cli("dist", "--presketched", "-S", 10, "--representatives", "0.1",
            *[str(tmp_path / e) if e.endswith(".txt") or e.endswith(".tsv") else e for e in extra], "-o", os.devnull, *names[:3], cwd=d, ok=False)
    assert "--representatives" in r.stderr.decode() and msg in r.stderr.decode()
    assert b"--representatives" in cli("dist", "--representatives", "abc", *names[:3], cwd=d, ok=False).stderr
