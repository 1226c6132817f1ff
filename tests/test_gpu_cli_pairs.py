"""GPU: `dashing-amd dist --pairs FILE [--measures LIST]` / `dist_by_seq --pairs`: one line per listed pair, in the
list's order, whose values are -- as text -- the cells of the upper-triangular TSV the same command line writes without
the flag."""
import os
import subprocess

import numpy as np
import pytest

from dashing_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dashing_amd", "dashing-amd")
FLAG = {"JI": (), "MASH_DIST": ("-M",), "CONTAINMENT_INDEX": ("--containment-index",), "SIZES": ("--sizes",),
        "SYMMETRIC_CONTAINMENT_DIST": ("--symmetric-containment-dist",)}


def cli(*args, ok=True):
    r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs")
    base = synth.synthetic_genomes(10, 60000, seed=0x9A12)
    paths = []
    for i, g in enumerate(base):
        p = d / ("g%02d.fna" % i)
        p.write_bytes(synth.to_fasta(g[: 40000 + 1500 * i], "g%d" % i))
        paths.append(str(p))
    return d, paths


def tsv_cells(text, names):
    """{(i, j > i): cell text} of the upper-triangular TSV"""
    lines = text.split("\n")
    assert lines[0] == "##Names\t" + "\t".join(names)
    cells = {}
    for i, name in enumerate(names):
        f = lines[1 + i].split("\t")
        assert f[0] == name
        for j in range(i + 1, len(names)):
            cells[(i, j)] = f[1 + j]
    return cells


def some_pairs(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < 25:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            out.append((a, b))
    return out + [out[0], out[3]]  # repeated pairs are legal


def measure_cells(tmp_path, measure, names, extra, sub="dist"):
    # (an asymmetric measure without -Q makes the tool compare all with all as queries x references: the symmetric
    # reading of its cells is taken from the measures whose TSV is a triangle)
    out = tmp_path / ("dense_%s.tsv" % measure)
    cli(sub, *extra, *FLAG[measure], "-O", out, "-o", os.devnull)
    return tsv_cells(out.read_text(), names)


@pytest.mark.parametrize("presketched", (False, True))
def test_dist_pairs_equals_the_tsv_cells(files, tmp_path, presketched):
    d, paths = files
    n = len(paths)
    if presketched:
        cache = tmp_path / "cache"
        cache.mkdir()
        cli("dist", "-W", "-P", cache, "-S", "11", "-k", "21", "-O", os.devnull, "-o", os.devnull, *paths)
        names = [str(cache / (os.path.basename(p) + ".w.21.spacing.11.hll")) for p in paths]
        assert all(os.path.exists(x) for x in names)
        extra = ["--presketched", "-S", "11", "-k", "21", *names]
    else:
        names = paths
        extra = ["--avoid-sorting", *paths]
    pairs = some_pairs(n, 5 + presketched)
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join("%s\t%s\n" % (names[a], names[b]) for a, b in pairs))
    # default: the measure the other flags select
    for measure in ("JI", "MASH_DIST"):
        cells = measure_cells(tmp_path, measure, names, extra)
        out = cli("dist", *extra, *FLAG[measure], "--pairs", lst, "-o", os.devnull).stdout.decode().split("\n")
        assert out[-1] == "" and len(out) == len(pairs) + 1
        for line, (a, b) in zip(out, pairs):
            assert line == "%s\t%s\t%s" % (names[a], names[b], cells[(min(a, b), max(a, b))])
    # --measures with three names: one column each, in the order given
    three = ("MASH_DIST", "SYMMETRIC_CONTAINMENT_DIST", "SIZES")
    cells = [measure_cells(tmp_path, m, names, extra) for m in three]
    out = cli("dist", *extra, "--pairs", lst, "--measures", ",".join(three), "-o", os.devnull).stdout.decode().split("\n")
    assert out[-1] == "" and len(out) == len(pairs) + 1
    for line, (a, b) in zip(out, pairs):
        key = (min(a, b), max(a, b))
        assert line == "\t".join([names[a], names[b]] + [c[key] for c in cells])


def test_sizes_are_emitted_as_without_the_flag(files, tmp_path):
    d, paths = files
    (tmp_path / "p.txt").write_text("%s\t%s\n" % (paths[1], paths[0]))
    s0, s1 = tmp_path / "s0.txt", tmp_path / "s1.txt"
    cli("dist", "--avoid-sorting", "-o", s0, "-O", os.devnull, *paths)
    cli("dist", "--avoid-sorting", "-o", s1, "-O", os.devnull, "--pairs", tmp_path / "p.txt", *paths)
    assert s0.read_bytes() == s1.read_bytes()


@pytest.mark.parametrize("extra,msg", [(("--nearest-neighbors", "2"), "--pairs does not go with --nearest-neighbors"),
                                       (("--threshold", "0.1"), "--pairs does not go with --threshold"),
                                       (("-b",), "--pairs does not go with -b"), (("--ngpus", "2"), "--pairs runs on one device")])
def test_refusals(files, tmp_path, extra, msg):
    d, paths = files
    (tmp_path / "p.txt").write_text("%s\t%s\n" % (paths[1], paths[0]))
    r = cli("dist", "--pairs", tmp_path / "p.txt", *extra, "-o", os.devnull, *paths[:3], ok=False)
    assert msg in r.stderr.decode()


def test_refused_with_queries_and_bad_lists(files, tmp_path):
    d, paths = files
    good = tmp_path / "p.txt"
    good.write_text("%s\t%s\n" % (paths[1], paths[0]))
    (tmp_path / "q.txt").write_text(paths[3] + "\n")
    r = cli("dist", "--pairs", good, "-Q", tmp_path / "q.txt", "-o", os.devnull, *paths[:3], ok=False)
    assert "--pairs does not go with -Q" in r.stderr.decode()
    for text, msg in (("%s\tnobody.fna\n" % paths[0], "nobody.fna"), ("%s\n" % paths[0], "line 1"),
                      ("%s\t%s\n%s\t%s\t%s\n" % (paths[0], paths[1], paths[0], paths[1], paths[2]), "line 2")):
        bad = tmp_path / "bad.txt"
        bad.write_text(text)
        r = cli("dist", "--pairs", bad, "-o", os.devnull, *paths[:3], ok=False)
        assert msg in r.stderr.decode(), r.stderr.decode()
    assert "missing.txt" in cli("dist", "--pairs", tmp_path / "missing.txt", "-o", os.devnull, *paths[:3], ok=False).stderr.decode()
    r = cli("dist", "--pairs", good, "--measures", "JI,NOPE", "-o", os.devnull, *paths[:3], ok=False)
    assert "NOPE" in r.stderr.decode()
    r = cli("dist", "--pairs", good, "--measures", "JI,", "-o", os.devnull, *paths[:3], ok=False)
    assert "unknown measure ''" in r.stderr.decode()
    r = cli("dist", "--measures", "JI", "-o", os.devnull, *paths[:3], ok=False)
    assert "--measures goes with --pairs only" in r.stderr.decode()


def test_orientation_under_an_asymmetric_measure(files, tmp_path):
    """the first name is lhs, the second rhs: under --containment-index the run without --pairs compares all inputs as
    queries x references (-b: float32 [query][reference], value = result_cmp(lhs = reference, rhs = query)), and --pairs
    itself does not switch to that form"""
    d, paths = files
    n = len(paths)
    dense_f = tmp_path / "ci.bin"
    cli("dist", "--avoid-sorting", "--containment-index", "-b", "-O", dense_f, "-o", os.devnull, *paths)
    dense = np.frombuffer(dense_f.read_bytes(), np.float32).reshape(n, n)
    pairs = [(a, b) for a in range(n) for b in range(n)]
    lst = tmp_path / "all.txt"
    lst.write_text("".join("%s\t%s\n" % (paths[a], paths[b]) for a, b in pairs))
    want = ["%s\t%s\t%s" % (paths[a], paths[b], "%.6g" % dense[b, a]) for a, b in pairs]
    out = cli("dist", "--avoid-sorting", "--containment-index", "--pairs", lst, "-o", os.devnull, *paths).stdout.decode().split("\n")
    assert out[:-1] == want
    out = cli("dist", "--avoid-sorting", "--pairs", lst, "--measures", "CONTAINMENT_INDEX", "-o", os.devnull, *paths).stdout.decode().split("\n")
    assert out[:-1] == want


def test_dist_by_seq_pairs(tmp_path):
    base = synth.synthetic_genomes(6, 30000, seed=0xB5E1)
    f = tmp_path / "multi.fna"
    f.write_bytes(b"".join(synth.to_fasta(g[: 20000 + 900 * i], "rec%d" % i) for i, g in enumerate(base)))
    names = ["rec%d" % i for i in range(6)]
    dense = tmp_path / "d.tsv"
    cli("dist_by_seq", "-M", "-O", dense, "-o", os.devnull, f)
    cells = tsv_cells(dense.read_text(), names)
    pairs = [(5, 0), (1, 2), (3, 3 - 1), (0, 5)]
    lst = tmp_path / "p.txt"
    lst.write_text("".join("rec%d\trec%d\n" % ab for ab in pairs))
    out = cli("dist_by_seq", "-M", "--pairs", lst, "-o", os.devnull, f).stdout.decode().split("\n")
    assert out[:-1] == ["rec%d\trec%d\t%s" % (a, b, cells[(min(a, b), max(a, b))]) for a, b in pairs]
    r = cli("dist_by_seq", "--pairs", lst, "--ngpus", "2", "-o", os.devnull, f, ok=False)
    assert "one device" in r.stderr.decode()
