"""GPU: `dashing-amd dist --union-curve [--curve-permutations N] [--curve-seed S]`, text and -b, held byte for byte to a
Python rendering of Context.union_curve + curve_permutations on the same sketches; the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import dashing_amd
from dashing_amd import synth
from test_gpu_cli_greedy import cli

pytestmark = pytest.mark.gpu
D = dashing_amd
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 10
ESTIMS = [((), D.ESTIM_ERTL_MLE, "ERTL_MLE"), (("-E",), D.ESTIM_ORIGINAL, "ORIGINAL"), (("-I",), D.ESTIM_ERTL_IMPROVED, "ERTL_IMPROVED")]


@pytest.fixture(scope="module")
def hlls(tmp_path_factory):
    """12 small .hll files at p = 10: overlapping genomes, one empty, one repeated"""
    host = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    host.dshh_write_hll.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    d = tmp_path_factory.mktemp("curvehll")
    core = synth.hll_registers(0xC0DE, 3000, P)
    regs = np.stack([np.maximum(core, synth.hll_registers(0x700 + i, 200 * (i + 1), P)) for i in range(12)])
    regs[4] = 0
    regs[9] = regs[2]
    names = ["g%02d.hll" % i for i in range(12)]
    for nm, row in zip(names, regs):
        assert host.dshh_write_hll(str(d / nm).encode(), np.ascontiguousarray(row).ctypes.data, P, 2) == 0
    return d, names, regs


def render(names, estim_name, curves, n_perm, seed):
    out = ["#UnionCurve\t%s\tpermutations=%d\tseed=%d" % (estim_name, n_perm, seed),
           "#step\tname\tunion_size\tnew" + ("\tperm_mean\tperm_min\tperm_max" if n_perm else "")]
    own = curves[0]
    for i, nm in enumerate(names):
        line = "%d\t%s\t%.3f\t%.3f" % (i + 1, nm, own[i], own[i] - own[i - 1] if i else own[i])
        if n_perm:
            total = 0.0
            for r in range(n_perm):  # summed in the permutations' order, divided once
                total += float(curves[1 + r][i])
            line += "\t%.3f\t%.3f\t%.3f" % (total / n_perm, curves[1:, i].min(), curves[1:, i].max())
        out.append(line)
    return "\n".join(out) + "\n"


@pytest.mark.parametrize("flags,estim,estim_name", ESTIMS)
def test_the_curve_equals_the_api(ctx, hlls, tmp_path, flags, estim, estim_name):
    d, names, regs = hlls
    n = len(names)
    ctx.set_sketches(regs)
    common = ["dist", "--presketched", "-S", P, "--avoid-sorting", *names, *flags, "-o", os.devnull]
    for extra, n_perm, seed in (((), 0, 0), (("--curve-permutations", 7, "--curve-seed", 11), 7, 11), (("--curve-permutations", 2), 2, 0)):
        orders = np.concatenate([np.arange(n, dtype=np.uint32)[None], D.curve_permutations(n, n_perm, seed)])
        curves = ctx.union_curve(orders, estim=estim)
        assert cli(*common, "--union-curve", *extra, cwd=d).stdout.decode() == render(names, estim_name, curves, n_perm, seed)
        ob = tmp_path / "curve.bin"
        cli(*common, "--union-curve", *extra, "-b", "-O", ob, cwd=d)
        raw = ob.read_bytes()
        assert np.frombuffer(raw[:16], np.uint64).tolist() == [n, n_perm]
        assert raw[16:] == curves.tobytes()
    # the repeated genome adds nothing, the empty one neither
    own = ctx.union_curve(np.arange(n, dtype=np.uint32), estim=estim)
    assert own[4] == own[3] and own[9] == own[8]


def test_refusals(hlls, tmp_path):
    d, names, _ = hlls
    base = ["dist", "--presketched", "-S", P, "-o", os.devnull]
    qf = tmp_path / "queries.txt"
    qf.write_text("".join("%s\n" % nm for nm in names[5:7]))
    gf = tmp_path / "groups.txt"
    gf.write_text("".join("%s\tg%d\n" % (nm, i % 2) for i, nm in enumerate(names[:5])))
    pf = tmp_path / "pairs.txt"
    pf.write_text("%s\t%s\n" % (names[0], names[1]))
    for other, what in ((("--threshold", 0.5), b"--union-curve does not go with --threshold"),
                        (("--cluster", 0.5), b"--union-curve does not go with --cluster"),
                        (("--representatives", 0.5), b"--union-curve does not go with --representatives"),
                        (("--nearest-neighbors", 3), b"--union-curve does not go with --nearest-neighbors"),
                        (("--histogram", "0:1:10"), b"--union-curve does not go with --histogram"),
                        (("--mst",), b"--union-curve does not go with --mst"),
                        (("--pairs", pf), b"--union-curve does not go with --pairs"),
                        (("--groups", gf), b"--union-curve does not go with --groups"),
                        (("-Q", qf), b"--union-curve does not go with -Q"),
                        (("-U",), b"--union-curve does not go with -U"), (("-T",), b"--union-curve does not go with -T"),
                        (("--ngpus", 2), b"--union-curve runs on one device")):
        r = cli(*base, "--union-curve", *other, *names[:5], cwd=d, ok=False)
        assert what in r.stderr, r.stderr
    r = cli("dist_by_seq", "-S", P, "--union-curve", "x.fa", cwd=d, ok=False)
    assert b"--union-curve does not go with dist_by_seq" in r.stderr, r.stderr
    for flag, what in ((("--curve-permutations", 3), b"--curve-permutations goes with --union-curve only"),
                       (("--curve-seed", 3), b"--curve-seed goes with --union-curve only")):
        r = cli(*base, *flag, *names[:5], cwd=d, ok=False)
        assert what in r.stderr, r.stderr
    for flag in (("--curve-permutations", "-1"), ("--curve-permutations", "x"), ("--curve-seed", "1.5")):
        r = cli(*base, "--union-curve", *flag, *names[:5], cwd=d, ok=False)
        assert b"needs a count" in r.stderr, r.stderr
    assert b"--union-curve" in cli("dist", "--help", ok=False).stderr
