"""GPU: the by-seq subcommands of the CLI end to end -- sketch_by_seq and dist_by_seq -- against the oracle sketching
every record alone, with the records' kseq names as labels."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from dashing_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dashing_amd", "dashing-amd")
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def run(*args):
    r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    return r


def wrap(s, w):
    return b"\n".join(s[i:i + w].tobytes() for i in range(0, len(s), w)) if len(s) else b""


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """three files: multi-line FASTA with empty and short records, multi-line FASTQ, gzip FASTA; related records"""
    d = tmp_path_factory.mktemp("byseq")
    rng = np.random.default_rng(0xB5)
    temps = synth.synthetic_genomes(4, 6000, seed=0xB6)
    recs = []  # (name, sequence) in input order

    def rec(i):
        a = temps[i % 4][: int(rng.integers(200, 6000))].copy()
        m = rng.integers(0, a.size, int(rng.integers(0, 300)))
        a[m] = LETTERS[rng.integers(0, 4, m.size)]
        return a

    fa = b""
    for i in range(12):
        s = rec(i) if i not in (3, 7) else (np.zeros(0, np.uint8) if i == 3 else LETTERS[rng.integers(0, 4, 20)])
        name = "fa_%d" % i
        recs.append((name, s))
        fa += (">%s some description\n" % name).encode() + wrap(s, 60) + b"\n"
    (d / "a.fa").write_bytes(fa)
    fq = b""
    for i in range(8):
        s = rec(i + 1)
        name = "fq_%d" % i
        recs.append((name, s))
        q = np.full(s.size, ord("I"), np.uint8)
        q[:1] = ord("@")
        fq += ("@%s\tx\n" % name).encode() + wrap(s, 80) + b"\n+\n" + wrap(q, 80) + b"\n"
    (d / "b.fq").write_bytes(fq)
    gz = b""
    for i in range(6):
        s = rec(i + 2)
        name = "gz_%d" % i
        recs.append((name, s))
        gz += (">%s\n" % name).encode() + wrap(s, 70) + b"\n"
    with gzip.open(d / "c.fa.gz", "wb") as f:
        f.write(gz)
    paths = [str(d / "a.fa"), str(d / "b.fq"), str(d / "c.fa.gz")]
    return paths, recs


def oracle_regs(oracle, recs, k, p, canon=True):
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for _, s in recs])
    seq = np.concatenate([s for _, s in recs]) if off[-1] else np.zeros(1, np.uint8)
    return oracle.sketch_batch(seq, off, k, p, canon)


@pytest.mark.parametrize("S,k,canon", [(10, 31, True), (14, 21, False)])
def test_sketch_by_seq_stream_and_labels(inputs, oracle, tmp_path, S, k, canon):
    paths, recs = inputs
    out = str(tmp_path / "recs.hll")
    run("sketch_by_seq", "-k", k, "-S", S, *([] if canon else ["-C"]), "-o", out, *paths)
    want = oracle_regs(oracle, recs, k, S, canon)
    raw = gzip.open(out).read()
    rec = 28 + (1 << S)
    assert len(raw) == len(recs) * rec
    for i in range(len(recs)):
        assert raw[i * rec + 28:(i + 1) * rec] == want[i].tobytes(), recs[i][0]
    assert gzip.open(out + ".labels.gz").read().decode().split("\n")[:-1] == [n for n, _ in recs]
    assert not want[3].any() and not want[7].any()  # the empty record and the one shorter than k


def parse_ut(text, n):
    lines = text.decode().split("\n")
    names = lines[0].split("\t")[1:]
    vals = []
    for i in range(n):
        f = lines[1 + i].split("\t")
        assert f[0] == names[i] and f[1:2 + i] == ["-"] * (i + 1)
        vals += [float(x) for x in f[2 + i:]]
    return names, np.array(vals)


def test_dist_by_seq_default_and_presketched(inputs, oracle, tmp_path):
    paths, recs = inputs
    names = [n for n, _ in recs]
    out, sizes = tmp_path / "d.tsv", tmp_path / "s.tsv"
    run("dist_by_seq", "-k", 31, "-S", 10, "-O", out, "-o", sizes, *paths)
    regs = oracle_regs(oracle, recs, 31, 10)
    got_names, got = parse_ut(out.read_bytes(), len(recs))
    assert got_names == names
    want = np.array([float("%.6g" % x) for x in oracle.dist_tri(regs)])
    assert np.allclose(got, want, rtol=2e-6, atol=1e-12, equal_nan=True)
    assert [ln.split("\t")[0] for ln in sizes.read_text().split("\n")[1:-1]] == names
    # --presketched over sketch_by_seq's output: byte for byte the same
    hll = str(tmp_path / "r.hll")
    run("sketch_by_seq", "-k", 31, "-S", 10, "-o", hll, *paths)
    out2, sizes2 = tmp_path / "d2.tsv", tmp_path / "s2.tsv"
    run("dist_by_seq", "-k", 31, "-S", 10, "--presketched", "-O", out2, "-o", sizes2, hll)
    assert out2.read_bytes() == out.read_bytes() and sizes2.read_bytes() == sizes.read_bytes()


@pytest.mark.parametrize("flags,rt", [(["-M"], 0), ([], 1)])
def test_dist_by_seq_binary_with_labels(inputs, oracle, tmp_path, flags, rt):
    paths, recs = inputs
    out = tmp_path / "d.bin"
    run("dist_by_seq", "-k", 21, "-S", 12, "-b", "-O", out, "-o", os.devnull, *flags, *paths)
    raw = out.read_bytes()
    n = len(recs)
    assert raw[0] == 0 and struct.unpack("<Q", raw[1:9])[0] == n and len(raw) == 9 + 4 * n * (n - 1) // 2
    want = oracle.dist_tri(oracle_regs(oracle, recs, 21, 12), 2, rt, 21)
    assert np.allclose(np.frombuffer(raw[9:], np.float32), want, rtol=1e-6, atol=1e-12, equal_nan=True)
    assert (tmp_path / "d.bin.labels").read_text().split("\n")[:-1] == [nm for nm, _ in recs]


def test_dist_by_seq_nearest_neighbors(inputs, oracle, tmp_path):
    paths, recs = inputs
    out = tmp_path / "nn.tsv"
    run("dist_by_seq", "--nearest-neighbors", 3, "-M", "-O", out, "-o", os.devnull, *paths)
    regs = oracle_regs(oracle, recs, 31, 10)
    wi, wv = oracle.knn(regs, 3, result_type=oracle.MASH_DIST, k=31)
    lines = out.read_text().split("\n")
    for i, (name, _) in enumerate(recs):
        f = lines[1 + i].split("\t")
        assert f[0] == name and len(f) == 4
        for j, cell in enumerate(f[1:]):
            a, b = cell.split(":")
            assert int(a) == wi[i, j]
            if np.isfinite(wv[i, j]):
                assert abs(float(b) - float("%g" % wv[i, j])) <= 2e-6 * max(abs(wv[i, j]), 1e-9)


def test_refusals(inputs, tmp_path):
    paths, _ = inputs
    r = subprocess.run([CLI, "dist_by_seq", "-Q", paths[0], *paths[1:]], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"-Q" in r.stderr
    r = subprocess.run([CLI, "sketch_by_seq", *paths], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"-o FILE" in r.stderr
    r = subprocess.run([CLI, "dist_by_seq", "-W", *paths], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"-W" in r.stderr
    r = subprocess.run([CLI, "dist_by_seq", "--devices", "0,0", *paths], capture_output=True, timeout=120)
    assert r.returncode != 0 and b"one device" in r.stderr


def test_sketch_by_seq_follows_kseq_on_damaged_inputs(oracle, tmp_path):
    """a lone '\\r' in a sequence line and in a header, text before the first header, and a FASTQ whose quality goes wrong
    at a later record: the rows are the oracle's registers of the records kseq reads (tests/kseq_ref.py), the labels are
    kseq's names, and the record that fails ends its file"""
    from kseq_ref import parse as kseq_parse  # (tests/kseq_ref.py)

    g = [bytes(x) for x in synth.synthetic_genomes(3, 6000, seed=0xB7)]
    fa = b"xx>pre\n>a\rcomment\n" + g[0][:3000] + b"\r" + g[0][3000:] + b"\n>b\n" + g[1][:2000] + b"\r\r\n" + g[1][2000:4000] + b"\n"
    fq = b"".join(b"@q%d\n%s\n+\n%s\n" % (i, g[2][i * 500 : (i + 1) * 500], b"I" * (500 if i != 6 else 499)) for i in range(10))
    paths = []
    for name, t in (("d.fa", fa), ("d.fq", fq)):
        (tmp_path / name).write_bytes(t)
        paths.append(str(tmp_path / name))
    recs = [(n.decode(), np.frombuffer(s, np.uint8)) for t in (fa, fq) for n, s in kseq_parse(t)[0]]
    assert [n for n, _ in recs] == ["pre", "a", "b"] + ["q%d" % i for i in range(6)]
    out = str(tmp_path / "recs.hll")
    run("sketch_by_seq", "-k", 21, "-S", 10, "-o", out, *paths)
    want = oracle_regs(oracle, recs, 21, 10)
    raw = gzip.open(out).read()
    rec = 28 + (1 << 10)
    assert len(raw) == len(recs) * rec
    for i in range(len(recs)):
        assert raw[i * rec + 28:(i + 1) * rec] == want[i].tobytes(), recs[i][0]
    assert gzip.open(out + ".labels.gz").read().decode().split("\n")[:-1] == [n for n, _ in recs]
