"""GPU: the row-block loop of `dashing-amd dist` across block edges.  DSH_BLOCK_VALS caps a block's values; by the
library's contract any cut of the rows gives the same bytes, so every output equals the run without the variable, and
the `[timing] rows ...` line of DSH_TIMING says how many blocks and page-locked buffers the loop really used.  With 8
genomes (28 values, rows of 7, 6, ... 1, 0 values): 1 = one row per block but the last, [6, 8) with one value; 7 and
13 = ragged blocks; 27 = two blocks, where the second buffer starts to exist; 28 = one block.  The workers of the
multi-device file writer get rows of their own only beyond one 128-row tile row: 700 sketches on three contexts (several
blocks and both buffers each), and 129 on two, where the second worker's range [128, 129) is one block of no value.
And the text headers of the four selections that print `<=` or `>=`, for all nine measures."""
import ctypes as C
import os
import re
import subprocess

import pytest

import dashing_amd
from dashing_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dashing_amd", "dashing-amd")

FORMATS = {"tsv": [], "phylip_mash": ["-U", "-M"], "full_tsv": ["-T"], "binary": ["-b"], "binary_mash": ["-b", "-M"]}


def dist(block_vals, flags, out, inputs, timing=False):
    """one `dist` run with DSH_BLOCK_VALS = block_vals (None: unset) -> the bytes of its -O file and, with DSH_TIMING,
    the (first row, end row, blocks, cap, buffers) of every `[timing] rows` line, sorted"""
    env = {k: v for k, v in os.environ.items() if k not in ("DSH_BLOCK_VALS", "DSH_TIMING")}
    if block_vals is not None:
        env["DSH_BLOCK_VALS"] = str(block_vals)
    if timing:
        env["DSH_TIMING"] = "1"
    r = subprocess.run([CLI, "dist", *[str(f) for f in flags], "-O", str(out), "-o", os.devnull, *inputs], capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr.decode()
    loops = re.findall(r"\[timing\] rows \[(\d+), (\d+)\): (\d+) blocks of at most (\d+) values, (\d+) buffers", r.stderr.decode())
    return out.read_bytes(), sorted(tuple(int(x) for x in m) for m in loops)


def model_cuts(n, r0, r1, cap):
    """the cut rule: a block takes rows while its values stay within cap, and at least one row"""
    cuts = [r0]
    while cuts[-1] < r1:
        rb = cuts[-1]
        re_, span = rb + 1, n - 1 - rb
        while re_ < r1 and span + (n - 1 - re_) <= cap:
            span += n - 1 - re_
            re_ += 1
        cuts.append(re_)
    return cuts


def want_loop(n, r0, r1, cap):
    nblocks = len(model_cuts(n, r0, r1, cap)) - 1
    return (r0, r1, nblocks, cap, 2 if nblocks > 1 else 1)


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    d = tmp_path_factory.mktemp("genomes")
    lens = [60000, 52000, 71000, 45000, 66000, 58000, 49000, 64000]
    paths = []
    for i, (g, L) in enumerate(zip(synth.synthetic_genomes(len(lens), 80000, seed=0xB10C), lens)):
        paths.append(str(d / ("g%d.fna" % i)))
        with open(paths[-1], "wb") as f:
            f.write(synth.to_fasta(g[:L], "g%d" % i))
    return paths


@pytest.fixture(scope="module")
def plain(genomes, tmp_path_factory):
    """every format on one device without the variable"""
    out = tmp_path_factory.mktemp("plain") / "plain.out"
    got = {name: dist(None, ["--avoid-sorting", *flags], out, genomes)[0] for name, flags in FORMATS.items()}
    n = len(genomes)
    assert n == 8 and len(got["binary"]) == 9 + 4 * n * (n - 1) // 2 and got["binary"] != got["binary_mash"]
    return got


# DSH_BLOCK_VALS -> the blocks of 8 inputs, by hand from the rows' 7, 6, 5, 4, 3, 2, 1, 0 values
CUTS = {1: [0, 1, 2, 3, 4, 5, 6, 8], 7: [0, 1, 2, 3, 5, 8], 13: [0, 2, 5, 8], 27: [0, 6, 8], 28: [0, 8]}


@pytest.mark.parametrize("block_vals", sorted(CUTS))
def test_any_cut_of_the_rows_gives_the_same_bytes(genomes, plain, tmp_path, block_vals):
    assert model_cuts(8, 0, 8, block_vals) == CUTS[block_vals]
    nblocks = len(CUTS[block_vals]) - 1
    for name in ("tsv", "phylip_mash", "binary"):
        got, loops = dist(block_vals, ["--avoid-sorting", *FORMATS[name]], tmp_path / "cut.out", genomes, timing=True)
        assert got == plain[name], name
        assert loops == [(0, 8, nblocks, block_vals, 2 if nblocks > 1 else 1)], name  # the variable is read, the blocks are these
    # -T takes dsh_dist_rows, not the block loop: the variable changes nothing there
    got, loops = dist(block_vals, ["--avoid-sorting", "-T"], tmp_path / "cut.out", genomes, timing=True)
    assert got == plain["full_tsv"] and loops == []


@pytest.mark.parametrize("block_vals", [1, 7, None])
def test_multi_device_file_of_8_inputs(genomes, plain, tmp_path, block_vals):
    """contexts on GPU 0, one process at a time.  8 inputs are one tile row: the first worker has all rows in several
    blocks, the others run the loop over an empty range"""
    cap = block_vals or 256 << 20
    got, loops = dist(block_vals, ["--avoid-sorting", "--devices", "0,0", "-b"], tmp_path / "two.bin", genomes, timing=True)
    assert got == plain["binary"] and loops == sorted([want_loop(8, 0, 8, cap), (8, 8, 0, cap, 1)])
    got, loops = dist(block_vals, ["--avoid-sorting", "--devices", "0,0,0", "-b", "-M"], tmp_path / "three.bin", genomes, timing=True)
    assert got == plain["binary_mash"] and loops == sorted([want_loop(8, 0, 8, cap), (8, 8, 0, cap, 1), (8, 8, 0, cap, 1)])


@pytest.fixture(scope="module")
def hlls(tmp_path_factory):
    """700 .hll files at p = 10 (the shape of test_multi_device_presketched_large)"""
    d = tmp_path_factory.mktemp("hlls")
    n, p = 700, 10
    regs = synth.synthetic_sketches(n, p, seed=2025)
    host = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    host.dshh_write_hll.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    paths = []
    for i in range(n):
        paths.append(str(d / ("s%04d.hll" % i)))
        assert host.dshh_write_hll(paths[-1].encode(), regs[i].ctypes.data, p, 2) == 0
    return paths


def test_every_worker_with_several_blocks_and_both_buffers(hlls, tmp_path):
    n, cap = len(hlls), 20000
    common = ["--presketched", "-S", 10, "-b", "-p", 8]
    one, loops = dist(None, common, tmp_path / "1.bin", hlls, timing=True)
    assert len(one) == 9 + 4 * n * (n - 1) // 2 and loops == [(0, n, 1, 256 << 20, 1)]
    bounds = [int(b) for b in dashing_amd.balance_rows(n, 3)]
    assert bounds == [0, 128, 384, 700]
    want = [want_loop(n, bounds[d], bounds[d + 1], cap) for d in range(3)]
    assert [w[2] for w in want] == [5, 6, 3]  # 81 344, 113 536 and 49 770 values in blocks of at most 20 000
    three, loops = dist(cap, [*common, "--devices", "0,0,0"], tmp_path / "3.bin", hlls, timing=True)
    assert three == one and loops == sorted(want)


def test_a_worker_whose_only_block_has_no_value(hlls, tmp_path):
    """129 inputs on two contexts: the second worker's rows are [128, 129), the last row, which has no value;
    dsh_dist_rows_async answers that block with DSH_OK and no work, and nothing is written for it"""
    n, cap = 129, 3000
    common = ["--presketched", "-S", 10, "-b"]
    assert [int(b) for b in dashing_amd.balance_rows(n, 2)] == [0, 128, 129] and model_cuts(n, 128, 129, cap) == [128, 129]
    one, _ = dist(None, common, tmp_path / "1.bin", hlls[:n])
    two, loops = dist(cap, [*common, "--devices", "0,0"], tmp_path / "2.bin", hlls[:n], timing=True)
    assert two == one and loops == sorted([want_loop(n, 0, 128, cap), (128, 129, 1, cap, 1)])
    # the same on one device: one input, one block of no value
    got, loops = dist(cap, common, tmp_path / "single.bin", hlls[:1], timing=True)
    assert got == b"\0" + (1).to_bytes(8, "little") and loops == [(0, 1, 1, cap, 1)]


@pytest.mark.parametrize("bad", ["0", "many", "-5", "7x", ""])
def test_a_value_that_is_no_positive_integer_is_ignored(genomes, plain, tmp_path, bad):
    for name in ("tsv", "binary"):
        got, loops = dist(bad, ["--avoid-sorting", *FORMATS[name]], tmp_path / "bad.out", genomes, timing=True)
        assert got == plain[name] and loops == [(0, 8, 1, 256 << 20, 1)], name  # the default cap


# flag, the measure's name in the header, the operator of --threshold's test: `<=` for the five *_DIST measures
MEASURES = [
    ((), "JI", ">="),
    (("-M",), "MASH_DIST", "<="),
    (("-l",), "FULL_MASH_DIST", "<="),
    (("--sizes",), "SIZES", ">="),
    (("--containment-index",), "CONTAINMENT_INDEX", ">="),
    (("--containment-dist",), "CONTAINMENT_DIST", "<="),
    (("--full-containment-dist",), "FULL_CONTAINMENT_DIST", "<="),
    (("--symmetric-containment-index",), "SYMMETRIC_CONTAINMENT_INDEX", ">="),
    (("--symmetric-containment-dist",), "SYMMETRIC_CONTAINMENT_DIST", "<="),
]


@pytest.mark.parametrize("flags,measure,op", MEASURES, ids=[m[1] for m in MEASURES])
def test_headers_name_the_measure_and_its_operator(genomes, tmp_path, flags, measure, op):
    for selection, want in ((["--threshold", "0.5"], "#Threshold\t%s\t%s\t0.5" % (measure, op)),
                            (["--cluster", "0.5"], "#Cluster\t%s\t%s\t0.5" % (measure, op)),
                            (["--representatives", "0.5"], "#Representatives\t%s\t%s\t0.5" % (measure, op)),
                            (["--histogram", "0:1:4"], "#Histogram\t%s\t%s" % (measure, op))):
        out, _ = dist(None, ["--avoid-sorting", *flags, *selection], tmp_path / "sel.out", genomes[:3])
        assert out.split(b"\n")[0].decode() == want, selection
