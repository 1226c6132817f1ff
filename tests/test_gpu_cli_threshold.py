"""GPU: `dashing-amd dist --threshold` / `dist_by_seq --threshold` against the numpy reference (tests/thr_ref.py) applied
to the dense -b output of the same command line without the flag: names, order and number text."""
import os
import subprocess

import numpy as np
import pytest

import thr_ref
from dashing_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dashing_amd", "dashing-amd")
NAMES = {0: "MASH_DIST", 1: "JI", 5: "CONTAINMENT_INDEX"}


def cli(*args, ok=True):
    r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("thr")
    base = synth.synthetic_genomes(12, 60000, seed=0x7E57)
    paths = []
    for i, g in enumerate(base):
        p = d / ("t%02d.fna" % i)
        p.write_bytes(synth.to_fasta(g[: 40000 + 1500 * i], "t%d" % i))
        paths.append(str(p))
    (d / "dup.fna").write_bytes(synth.to_fasta(base[0][:40000], "dup"))  # equal to t00: an exact tie at JI 1 / Mash 0
    paths.append(str(d / "dup.fna"))
    return d, paths


def text_lines(names_r, names_c, csr, op, measure, t):
    rp, col, val = csr
    out = ["#Threshold\t%s\t%s\t%s" % (measure, op, "%.6g" % np.float32(t))]
    for r in range(len(rp) - 1):
        for h in range(int(rp[r]), int(rp[r + 1])):
            out.append("%s\t%s\t%s" % (names_r[r], names_c[col[h]], "%.6g" % val[h]))
    return out


def parse_bin(raw):
    n, nnz = np.frombuffer(raw[:16], np.uint64)
    n, nnz = int(n), int(nnz)
    o = 16
    rp = np.frombuffer(raw[o : o + 8 * (n + 1)], np.uint64)
    o += 8 * (n + 1)
    col = np.frombuffer(raw[o : o + 4 * nnz], np.uint32)
    o += 4 * nnz
    val = np.frombuffer(raw[o : o + 4 * nnz], np.float32)
    assert o + 4 * nnz == len(raw)
    return rp, col, val


@pytest.mark.parametrize("flags,rt,ts", [((), 1, (0.05, 1.0, 0.0)), (("-M",), 0, (0.1, 0.0, 1.0)), (("-M", "-k", "21", "-S", "12"), 0, (0.15,))])
def test_dist_threshold_text_and_binary(files, tmp_path, flags, rt, ts):
    d, paths = files
    n = len(paths)
    dense_f = tmp_path / "dense.bin"
    sizes, sizes0 = tmp_path / "sizes.txt", tmp_path / "sizes0.txt"
    cli("dist", "--avoid-sorting", "-b", "-O", dense_f, "-o", sizes0, *flags, *paths)
    raw = dense_f.read_bytes()
    dense = np.frombuffer(raw[9:], np.float32)
    assert dense.size == n * (n - 1) // 2
    for t in ts:
        want = thr_ref.tri(dense, n, 0, n, t, rt)
        out = cli("dist", "--avoid-sorting", "--threshold", t, "-o", sizes, *flags, *paths).stdout.decode().split("\n")
        assert out[-1] == "" and out[:-1] == text_lines(paths, paths, want, "<=" if rt == 0 else ">=", NAMES[rt], t)
        assert sizes.read_bytes() == sizes0.read_bytes()  # sizes are emitted as without the flag
        b = tmp_path / "thr.bin"
        cli("dist", "--avoid-sorting", "--threshold", t, "-b", "-O", b, "-o", os.devnull, *flags, *paths)
        assert thr_ref.same(parse_bin(b.read_bytes()), want)
    assert want[1].size > 0


def test_dist_threshold_query_reference(files, tmp_path):
    d, paths = files
    refs, qs = paths[:8], paths[8:]
    (tmp_path / "r.txt").write_text("\n".join(refs) + "\n")
    (tmp_path / "q.txt").write_text("\n".join(qs) + "\n")
    for flags, rt, t in ((("--containment-index",), 5, 0.1), ((), 1, 1.0), (("-M",), 0, 0.12)):
        common = ["dist", "--avoid-sorting", *flags, "-F", tmp_path / "r.txt", "-Q", tmp_path / "q.txt", "-o", os.devnull]
        dense_f = tmp_path / "qr.bin"
        cli(*common, "-b", "-O", dense_f)
        dense = np.frombuffer(dense_f.read_bytes(), np.float32).reshape(len(qs), len(refs))
        want = thr_ref.rect(dense, 0, t, rt)
        out = cli(*common, "--threshold", t).stdout.decode().split("\n")
        assert out[:-1] == text_lines(qs, refs, want, "<=" if rt == 0 else ">=", NAMES[rt], t)
        b = tmp_path / "qr_thr.bin"
        cli(*common, "--threshold", t, "-b", "-O", b)
        assert thr_ref.same(parse_bin(b.read_bytes()), want)
    assert want[1].size > 0


@pytest.mark.parametrize("extra,msg", [(("--nearest-neighbors", "2"), "--nearest-neighbors"), (("-U",), "-U"), (("-T",), "-T"),
                                       (("--ngpus", "2"), "one device")])
def test_refusals(files, extra, msg):
    d, paths = files
    r = cli("dist", "--threshold", "0.1", *extra, "-o", os.devnull, *paths[:3], ok=False)
    assert "--threshold" in r.stderr.decode() and msg in r.stderr.decode()
    assert cli("dist", "--threshold", "abc", *paths[:3], ok=False).stderr


def test_dist_by_seq_threshold(tmp_path):
    base = synth.synthetic_genomes(6, 30000, seed=0xB5E0)
    f = tmp_path / "multi.fna"
    f.write_bytes(b"".join(synth.to_fasta(g[: 20000 + 900 * i], "rec%d" % i) for i, g in enumerate(base)) + synth.to_fasta(base[1][:20900], "again"))
    names = ["rec%d" % i for i in range(6)] + ["again"]
    dense_f = tmp_path / "d.bin"
    cli("dist_by_seq", "-M", "-b", "-O", dense_f, "-o", os.devnull, f)
    dense = np.frombuffer(dense_f.read_bytes()[9:], np.float32)
    for t in (0.0, 0.1):
        want = thr_ref.tri(dense, 7, 0, 7, t, 0)
        out = cli("dist_by_seq", "-M", "--threshold", t, "-o", os.devnull, f).stdout.decode().split("\n")
        assert out[:-1] == text_lines(names, names, want, "<=", "MASH_DIST", t)
        assert want[1].size > 0
