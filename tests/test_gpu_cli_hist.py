"""GPU: `dashing-amd dist --histogram SPEC [--histogram-labels FILE]`, text and -b, parsed back and held to
Context.dist_histogram / Context.dist_rect_histogram on the same sketches, edges and labels; the refusals."""
import os

import numpy as np
import pytest

import dashing_amd
from test_gpu_cli_greedy import cli, hlls  # noqa: F401  (hlls: the 40 .hll files of that module)
from test_gpu_cli_greedy_extend import load_regs

pytestmark = pytest.mark.gpu
D = dashing_amd
F = np.float32
CASES = [((), D.JI, "JI", ">="), (("-M",), D.MASH_DIST, "MASH_DIST", "<=")]


def spec_edges(lo, hi, nbins):
    return np.array([F(lo + (hi - lo) * i / nbins) for i in range(nbins + 1)], F)


def parse_hist_bin(raw):
    """u64 n_edges, u64 planes, f32 edges[n_edges] padded to 8 bytes, u64 counts[planes][n_edges + 2]"""
    ne, planes = (int(x) for x in np.frombuffer(raw[:16], np.uint64))
    eb = (4 * ne + 7) // 8 * 8
    assert len(raw) == 16 + eb + 8 * planes * (ne + 2)
    return np.frombuffer(raw[16 : 16 + 4 * ne], F), np.frombuffer(raw[16 + eb :], np.uint64).reshape(planes, ne + 2)


def check_text(out, edges, counts, measure, op):
    lines = out.split("\n")
    ne = edges.size
    assert lines[-1] == "" and len(lines) == ne + 2 + 2 and lines[0] == "#Histogram\t%s\t%s" % (measure, op)
    lows = ["-inf"] + ["%.6g" % e for e in edges] + ["nan"]
    highs = ["%.6g" % e for e in edges] + ["inf", "nan"]
    for b, line in enumerate(lines[1:-1]):
        assert line.split("\t") == [lows[b], highs[b]] + [str(int(c)) for c in counts[:, b]], (b, line)


@pytest.mark.parametrize("flags,rt,measure,op", CASES)
def test_histogram_equals_the_api(ctx, hlls, tmp_path, flags, rt, measure, op):
    d, names = hlls
    n = len(names)
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", *names, *flags, "-o", os.devnull]
    ctx.set_sketches(load_regs(d, names))
    kw = dict(estim=2, result_type=rt, k=31)
    edges = spec_edges(0.0, 1.0, 50)
    want = ctx.dist_histogram(edges, **kw)
    assert int(want.sum()) == n * (n - 1) // 2 and (want > 0).sum() > 1
    check_text(cli(*common, "--histogram", "0:1:50", cwd=d).stdout.decode(), edges, want, measure, op)
    hb = tmp_path / "hist.bin"
    cli(*common, "--histogram", "0:1:50", "-b", "-O", hb, cwd=d)
    got_e, got = parse_hist_bin(hb.read_bytes())
    assert got_e.tobytes() == edges.tobytes() and got.tobytes() == want.tobytes()
    # a comma list (an odd number of edges: padded in -b) and @FILE
    few = np.array([-np.inf, 0.0, 0.25, 0.5, np.inf], F)
    cli(*common, "--histogram", "-inf,0,0.25,0.5,inf", "-b", "-O", hb, cwd=d)
    got_e, got = parse_hist_bin(hb.read_bytes())
    assert got_e.tobytes() == few.tobytes() and got.tobytes() == ctx.dist_histogram(few, **kw).tobytes()
    ef = tmp_path / "edges.txt"
    ef.write_text("".join("%.9g\n" % e for e in edges[::5]))
    check_text(cli(*common, "--histogram", "@%s" % ef, cwd=d).stdout.decode(), edges[::5], ctx.dist_histogram(edges[::5], **kw), measure, op)
    # split by the labels of --cluster -b
    t = 0.5 if rt == D.JI else 0.03
    lb = tmp_path / "labels.bin"
    cli(*common, "--cluster", t, "-b", "-O", lb, cwd=d)
    lab = np.frombuffer(lb.read_bytes()[16:], np.uint32)
    assert lab.size == n and 1 < np.unique(lab).size < n
    want2 = ctx.dist_histogram(edges, labels=lab, **kw)
    assert want2[0].any() and want2[1].any() and np.array_equal(want2[0] + want2[1], want[0])
    check_text(cli(*common, "--histogram", "0:1:50", "--histogram-labels", lb, cwd=d).stdout.decode(), edges, want2, measure, op)
    cli(*common, "--histogram", "0:1:50", "--histogram-labels", lb, "-b", "-O", hb, cwd=d)
    got_e, got = parse_hist_bin(hb.read_bytes())
    assert got_e.tobytes() == edges.tobytes() and got.tobytes() == want2.tobytes()


@pytest.mark.parametrize("flags,rt,measure,op", CASES + [(("--containment-index",), D.CONTAINMENT_INDEX, "CONTAINMENT_INDEX", ">=")])
def test_queries_make_it_the_rectangle(ctx, hlls, tmp_path, flags, rt, measure, op):
    d, names = hlls
    n, nr = len(names), 25
    qf = tmp_path / "queries.txt"
    qf.write_text("".join("%s\n" % nm for nm in names[nr:]))
    common = ["dist", "--presketched", "-S", 10, *names[:nr], "-Q", qf, *flags, "-o", os.devnull]
    ctx.set_sketches(load_regs(d, names))  # references first, then the queries
    edges = spec_edges(0.0, 1.0, 50)
    want = ctx.dist_rect_histogram(edges, nr, n, 0, nr, estim=2, result_type=rt, k=31)
    assert int(want.sum()) == (n - nr) * nr
    check_text(cli(*common, "--histogram", "0:1:50", cwd=d).stdout.decode(), edges, want, measure, op)
    hb = tmp_path / "hist.bin"
    cli(*common, "--histogram", "0:1:50", "-b", "-O", hb, cwd=d)
    got_e, got = parse_hist_bin(hb.read_bytes())
    assert got_e.tobytes() == edges.tobytes() and got.tobytes() == want.tobytes()


def test_refusals(hlls, tmp_path):
    d, names = hlls
    base = ["dist", "--presketched", "-S", 10, "-o", os.devnull]
    for other, what in ((("--threshold", 0.5), b"--histogram does not go with --threshold"),
                        (("--cluster", 0.5), b"--histogram does not go with --cluster"),
                        (("--representatives", 0.5), b"--histogram does not go with --representatives"),
                        (("--nearest-neighbors", 3), b"--histogram does not go with --nearest-neighbors"),
                        (("-U",), b"--histogram does not go with -U"), (("-T",), b"--histogram does not go with -T"),
                        (("--ngpus", 2), b"--histogram runs on one device")):
        r = cli(*base, "--histogram", "0:1:10", *other, *names[:5], cwd=d, ok=False)
        assert what in r.stderr, r.stderr
    for spec, what in (("0:1", b"not lo:hi:nbins"), ("0:1:0", b"bins"), ("1:0:4", b"lo < hi"), ("0.5,0.25", b"increase strictly"),
                       ("0.1,x", b"not a number"), ("nan", b"not a number"), ("1:1.0000001:8", b"increase strictly"),
                       ("0:1:4096", b"bins"), ("", b"not a number")):
        r = cli(*base, "--histogram", spec, *names[:5], cwd=d, ok=False)
        assert what in r.stderr, (spec, r.stderr)
    r = cli(*base, "--histogram-labels", "x.bin", *names[:5], cwd=d, ok=False)
    assert b"--histogram-labels goes with --histogram only" in r.stderr
    short = tmp_path / "short.bin"
    cli(*base, "--cluster", 0.5, "-b", "-O", short, *names[:4], cwd=d)
    r = cli(*base, "--histogram", "0:1:10", "--histogram-labels", short, *names[:5], cwd=d, ok=False)
    assert b"labels 4 inputs but this run has 5" in r.stderr
    assert b"--histogram SPEC" in cli("dist", "--help", ok=False).stderr
