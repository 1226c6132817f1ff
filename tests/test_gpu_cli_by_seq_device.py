"""GPU: sketch_by_seq and dist_by_seq with the parse on the device (DSH_DEVICE_PARSE=1: plain files go through
dsh_sketch_fastx_records, compressed and refused ones through the host parser) write byte for byte what the host path
(DSH_HOST_PARSE=1) writes -- the .hll container, FILE.labels.gz and dist_by_seq's text --, slots and labels in the inputs'
order; the labels are kseq's names."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from fastx_gen import fasta, fastq  # (tests/fastx_gen.py)
from kseq_ref import parse as kseq_parse  # (tests/kseq_ref.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dashing_amd", "dashing-amd")
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def run(env, *args):
    e = dict(os.environ)
    for name in ("DSH_HOST_PARSE", "DSH_DEVICE_PARSE", "DSH_TIMING"):
        e.pop(name, None)
    e.update(env)
    r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """plain FASTA, plain four-line FASTQ, gzip FASTA, a FASTQ with two-line sequences (the device refuses it), plain FASTA"""
    d = tmp_path_factory.mktemp("byseq_device")
    rng = np.random.default_rng(0xD5)
    g = LETTERS[rng.integers(0, 4, 60_000)].tobytes()
    texts = [
        fasta(rng, [(b"fa_%d some text" % i, g[i * 2000: i * 2000 + 300 + 150 * i]) for i in range(9)] + [(b"fa_empty", b""), (b"fa_short", b"ACGT")], 60),
        fastq(rng, [g[20_000 + i * 200: 20_000 + i * 200 + 40 + 9 * i] for i in range(15)]),
        fasta(rng, [(b"gz_%d" % i, g[30_000 + i * 1500: 30_000 + i * 1500 + 1400]) for i in range(5)], 70),
        b"".join(b"@two_%d x\n%s\n%s\n+\n%s\n" % (i, g[40_000 + i * 300: 40_100 + i * 300], g[40_100 + i * 300: 40_200 + i * 300], b"I" * 200) for i in range(6)),
        fasta(rng, [(b"last_%d\tt" % i, g[50_000 + i * 900: 50_000 + i * 900 + 800]) for i in range(4)], 0, eol=b"\r\n"),
    ]
    paths = [str(d / n) for n in ("a.fa", "b.fq", "c.fa.gz", "d.fq", "e.fa")]
    for pth, t in zip(paths, texts):
        with (gzip.open(pth, "wb") if pth.endswith(".gz") else open(pth, "wb")) as f:
            f.write(t)
    names = [n for t in texts for n, _ in kseq_parse(t)[0]]
    return paths, names


def test_sketch_by_seq_device_path_equals_host_path(inputs, tmp_path):
    paths, names = inputs
    dev, host = tmp_path / "dev.hll", tmp_path / "host.hll"
    r = run({"DSH_DEVICE_PARSE": "1", "DSH_TIMING": "1"}, "sketch_by_seq", "-k", 21, "-S", 10, "-o", dev, *paths)
    run({"DSH_HOST_PARSE": "1"}, "sketch_by_seq", "-k", 21, "-S", 10, "-o", host, *paths)
    m = re.search(rb"by_seq: (\d+) files \((\d+) records\) decoded on the device, (\d+) files \((\d+) records\) on the host", r.stderr)
    assert m, r.stderr.decode()
    assert (int(m.group(1)), int(m.group(3))) == (3, 2) and int(m.group(2)) + int(m.group(4)) == len(names)
    assert dev.read_bytes() == host.read_bytes()
    assert (tmp_path / "dev.hll.labels.gz").read_bytes() == (tmp_path / "host.hll.labels.gz").read_bytes()
    assert gzip.decompress((tmp_path / "dev.hll.labels.gz").read_bytes()).split(b"\n")[: len(names)] == names


def test_dist_by_seq_device_path_equals_host_path(inputs, tmp_path):
    paths, names = inputs
    out = {}
    for tag, env in (("dev", {"DSH_DEVICE_PARSE": "1"}), ("host", {"DSH_HOST_PARSE": "1"})):
        run(env, "dist_by_seq", "-k", 21, "-S", 10, "-o", tmp_path / (tag + ".sizes"), "-O", tmp_path / (tag + ".dist"), *paths)
        out[tag] = ((tmp_path / (tag + ".sizes")).read_bytes(), (tmp_path / (tag + ".dist")).read_bytes())
    assert out["dev"] == out["host"]
    assert out["dev"][1].split(b"\n")[0].split(b"\t")[1:] == names  # ("##Names" and the labels, in input order)


def test_no_records_ends_the_run_on_either_path(tmp_path):
    p = tmp_path / "none.fa"
    p.write_bytes(b">")
    for env in ({"DSH_DEVICE_PARSE": "1"}, {"DSH_HOST_PARSE": "1"}):
        e = dict(os.environ, **env)
        r = subprocess.run([CLI, "sketch_by_seq", "-o", str(tmp_path / "x.hll"), str(p)], capture_output=True, timeout=300, env=e)
        assert r.returncode != 0 and b"No sequence records in the inputs." in r.stderr
