"""GPU, through the CLI: `dist --presketched` over .hll files of DIFFERENT precisions.  A file above -S is folded on the
device while it is loaded (dsh_upload_sketches_folded); the output equals, byte for byte, that over copies folded on the
host with the `fold` subcommand; a file below -S still ends with the message it always did."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dashing_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dashing_amd", "dashing-amd")
NAMES = ["g%d.hll" % i for i in range(6)]
PS = (12, 14, 14, 12, 14, 12)


def run(*args, cwd=None, ok=True):
    r = subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """mixed/: six files at p = 12 and 14; folded/: the same names, folded to p = 10 by the host's `fold`"""
    host = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    host.dshh_write_hll.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    root = tmp_path_factory.mktemp("mixedp")
    mixed, folded = root / "mixed", root / "folded"
    mixed.mkdir()
    folded.mkdir()
    core = {p: synth.hll_registers(0xC0 + p, 3000, p) for p in set(PS)}
    for i, (name, p) in enumerate(zip(NAMES, PS)):
        regs = np.maximum(core[p], synth.hll_registers(0x51 + i, 500 * (i + 1), p))  # (related: distances below 1)
        assert host.dshh_write_hll(str(mixed / name).encode(), regs.ctypes.data, p, 2) == 0
        run("fold", "-p", 10, "-o", folded / name, mixed / name)
    return mixed, folded


@pytest.mark.parametrize("flags", [(), ("-b",), ("-M",)])
def test_mixed_p_equals_host_folded_files(files, tmp_path, flags):
    mixed, folded = files
    outs = []
    for k, d in enumerate((mixed, folded)):
        dist, sizes = tmp_path / ("dist%d" % k), tmp_path / ("sizes%d" % k)
        run("dist", "--presketched", "-S", 10, "--avoid-sorting", *flags, "-O", dist, "-o", sizes, *NAMES, cwd=d)
        outs.append((dist.read_bytes(), sizes.read_bytes()))
    assert outs[0][0] == outs[1][0] and len(outs[0][0]) > 0
    assert outs[0][1] == outs[1][1]


def test_mixed_p_queries(files, tmp_path):
    mixed, folded = files
    outs = []
    for k, d in enumerate((mixed, folded)):
        dist, qf = tmp_path / ("q%d" % k), tmp_path / ("queries%d.txt" % k)
        qf.write_text("\n".join(NAMES[4:]) + "\n")
        run("dist", "--presketched", "-S", 10, "--avoid-sorting", "-O", dist, "-o", os.devnull, "-Q", qf, *NAMES[:4], cwd=d)
        outs.append(dist.read_bytes())
    assert outs[0] == outs[1] and outs[0]


def test_a_file_below_S_still_fails(files, tmp_path):
    mixed, _ = files
    low = tmp_path / "low.hll"
    run("fold", "-p", 8, "-o", low, mixed / NAMES[0])
    r = run("dist", "--presketched", "-S", 10, "-O", os.devnull, "-o", os.devnull, low, mixed / NAMES[1], ok=False)
    assert b"has p=8 but -S is 10" in r.stderr


# ---- dist --groups FILE: the unions of named groups are compared instead of the inputs

GROUPS = {"alpha": (0, 3, 4), "beta": (1, 2), "gamma": (5, 6, 7, 8)}  # (order of first appearance: input 0, 1, 5)


@pytest.fixture(scope="module")
def grouped(tmp_path_factory):
    """inputs/: nine p = 10 sketches and groups.tsv; unions/: one file per group, named as the group, made by the host's
    `union` subcommand"""
    host = C.CDLL(os.path.join(ROOT, "dashing_amd", "libdashing_host.so"))
    host.dshh_write_hll.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    root = tmp_path_factory.mktemp("groups")
    inputs, unions = root / "inputs", root / "unions"
    inputs.mkdir()
    unions.mkdir()
    names = ["s%d.hll" % i for i in range(9)]
    core = synth.hll_registers(0x6A, 2500, 10)
    for i, name in enumerate(names):
        regs = np.maximum(core, synth.hll_registers(0x6B + i, 300 * (i + 1), 10))
        assert host.dshh_write_hll(str(inputs / name).encode(), regs.ctypes.data, 10, 2) == 0
    of = {i: g for g, mem in GROUPS.items() for i in mem}
    (inputs / "groups.tsv").write_text("".join("%s\t%s\n" % (names[i], of[i]) for i in range(9)))
    for g, mem in GROUPS.items():
        run("union", "-o", unions / g, *[inputs / names[i] for i in mem])
    return inputs, unions, names


@pytest.mark.parametrize("flags", [(), ("-b",), ("-U",), ("-T", "-M"), ("--threshold", "0.5"), ("--nearest-neighbors", "2"),
                                   ("--containment-index",)])
def test_groups_equal_the_host_unions(grouped, tmp_path, flags):
    inputs, unions, names = grouped
    outs = []
    for k, (d, args) in enumerate(((inputs, ["--groups", "groups.tsv"] + names), (unions, list(GROUPS)))):
        dist, sizes = tmp_path / ("dist%d" % k), tmp_path / ("sizes%d" % k)
        run("dist", "--presketched", "-S", 10, "--avoid-sorting", *flags, "-O", dist, "-o", sizes, *args, cwd=d)
        labels = tmp_path / ("dist%d.labels" % k)
        outs.append((dist.read_bytes(), sizes.read_bytes(), labels.read_bytes() if labels.exists() else b""))
    assert outs[0] == outs[1] and outs[0][0] and outs[0][1]
    assert all(g.encode() in outs[0][1] for g in GROUPS) and b"s0.hll" not in outs[0][1]  # labels are the group names
    if flags == ("-b",):
        assert outs[0][2].split() == [g.encode() for g in GROUPS]


def test_groups_refusals(grouped, tmp_path):
    inputs, _, names = grouped
    base = ["--presketched", "-S", 10, "-O", os.devnull, "-o", os.devnull, "--groups", "groups.tsv"]
    (inputs / "pairs.tsv").write_text("%s\t%s\n" % (names[0], names[1]))
    (inputs / "q.txt").write_text(names[8] + "\n")
    for sub, extra in (("dist", ["--pairs", "pairs.tsv"] + names), ("dist", ["-Q", "q.txt"] + names[:8]),
                       ("dist", ["--devices", "0,0"] + names), ("dist_by_seq", names[:1])):
        r = run(sub, *base, *extra, cwd=inputs, ok=False)
        assert b"--groups" in r.stderr, (sub, extra, r.stderr)
    # a name that is no input, an input without a group, an input named twice: errors that name it
    for text, word in (("nope.hll\talpha\n", b"nope.hll"), ("".join("%s\tg\n" % s for s in names[:8]), names[8].encode()),
                       ("".join("%s\tg\n" % s for s in names + names[:1]), names[0].encode())):
        (inputs / "bad.tsv").write_text(text)
        r = run("dist", "--presketched", "-S", 10, "-O", os.devnull, "-o", os.devnull, "--groups", "bad.tsv", *names, cwd=inputs, ok=False)
        assert word in r.stderr
