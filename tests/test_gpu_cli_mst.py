"""GPU: `dashing-amd dist --mst [--mst-cutoff FLOAT] [--dendrogram]` against the Python call (Context.mst_tri, mst_linkage)
and the literal model (tests/mst_ref.py) over the dense values `dist -b` writes for the same command line: text and -b."""
import os
import subprocess

import numpy as np
import pytest

import dashing_amd
import mst_ref as R
from dashing_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dashing_amd", "dashing-amd")


def cli(*args, cwd=None, ok=True):
    r = subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """12 small FASTA genomes: two overlapping cuts of six sequences"""
    d = tmp_path_factory.mktemp("mstfa")
    paths = []
    for i, g in enumerate(synth.synthetic_genomes(6, 30000, seed=0x357)):
        for v in range(2):
            p = d / ("g%d_%d.fna" % (i, v))
            p.write_bytes(synth.to_fasta(g[2000 * v : 22000 + 2000 * v], "g%d_%d" % (i, v)))
            paths.append(str(p))
    return paths


def parse_bin(raw, n, columns):
    hdr = np.frombuffer(raw[:16], np.uint64)
    m = int(hdr[1])
    assert int(hdr[0]) == n and len(raw) == 16 + 4 * m * len(columns)
    return [np.frombuffer(raw[16 + 4 * m * x : 16 + 4 * m * (x + 1)], dt) for x, dt in enumerate(columns)]


@pytest.mark.parametrize("flags,rt_name,desc,cut", [((), "JI", 1, 0.3), (("-M",), "MASH_DIST", 0, 0.03)])
def test_edges_and_dendrogram_equal_the_python_call(ctx, genomes, tmp_path, flags, rt_name, desc, cut):
    paths, n = genomes, len(genomes)
    common = ["dist", "--avoid-sorting", *flags, "-o", os.devnull]
    b = tmp_path / "dense.bin"
    cli(*common, "-b", "-O", b, *paths)
    dense = np.frombuffer(b.read_bytes()[9:], np.float32)
    assert dense.size == R.span(n)
    for extra, cutoff in (((), None), (("--mst-cutoff", cut), cut)):
        lhs, rhs, val = ctx.mst_tri(dense, desc, cutoff)
        want = R.kruskal(n, dense, desc, R.no_cutoff(desc) if cutoff is None else cutoff)
        assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip((lhs, rhs, val), want))
        assert 0 < lhs.size <= n - 1 and (cutoff is None) == (lhs.size == n - 1)
        out = cli(*common, "--mst", *extra, *paths).stdout.decode().split("\n")
        assert out[-1] == "" and out[0] == "#MST\t%s\t%d\t%d" % (rt_name, n, lhs.size)
        assert out[1:-1] == ["%s\t%s\t%s" % (paths[i], paths[j], "%.6g" % v) for i, j, v in zip(lhs, rhs, val)]
        mb = tmp_path / "mst.bin"
        cli(*common, "--mst", *extra, "-b", "-O", mb, *paths)
        got = parse_bin(mb.read_bytes(), n, (np.uint32, np.uint32, np.float32))
        assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, (lhs, rhs, val)))
        za, zb, zv, zs = dashing_amd.mst_linkage(n, lhs, rhs, val)
        out = cli(*common, "--mst", "--dendrogram", *extra, *paths).stdout.decode().split("\n")
        assert out[-1] == "" and out[0] == "#Dendrogram\t%s\t%d\t%d" % (rt_name, n, za.size)
        assert out[1:-1] == ["%d\t%d\t%s\t%d" % (a, b_, "%.6g" % v, s) for a, b_, v, s in zip(za, zb, zv, zs)]
        cli(*common, "--mst", "--dendrogram", *extra, "-b", "-O", mb, *paths)
        got = parse_bin(mb.read_bytes(), n, (np.uint32, np.uint32, np.float32, np.uint32))
        assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, (za, zb, zv, zs)))


@pytest.mark.parametrize("extra,msg", [(("--threshold", "0.1"), "--threshold"), (("--nearest-neighbors", "2"), "--nearest-neighbors"),
                                       (("--pairs", "pairs.tsv"), "--pairs"), (("-Q", "q.txt"), "-Q"), (("-U",), "-U"), (("-T",), "-T"),
                                       (("--ngpus", "2"), "one device"), (("--cluster", "0.1"), "--cluster"),
                                       (("--representatives", "0.1"), "--representatives"), (("--histogram", "0:1:4"), "--histogram"),
                                       (("--cluster", "0.1", "--stats"), "--cluster")])
def test_refusals(genomes, tmp_path, extra, msg):
    (tmp_path / "q.txt").write_text(genomes[0] + "\n")
    (tmp_path / "pairs.tsv").write_text("%s\t%s\n" % (genomes[0], genomes[1]))
    r = cli("dist", "--mst", *[str(tmp_path / e) if e.endswith(".txt") or e.endswith(".tsv") else e for e in extra], "-o", os.devnull,
            *genomes[:3], ok=False)
    assert "--mst" in r.stderr.decode() and msg in r.stderr.decode()


def test_flags_that_need_mst(genomes):
    assert b"--mst" in cli("dist", "--dendrogram", *genomes[:3], ok=False).stderr
    assert b"--mst" in cli("dist", "--mst-cutoff", "0.5", *genomes[:3], ok=False).stderr
    assert b"--mst-cutoff" in cli("dist", "--mst", "--mst-cutoff", "abc", *genomes[:3], ok=False).stderr
    assert b"--stats" in cli("dist", "--mst", "--stats", *genomes[:3], ok=False).stderr
