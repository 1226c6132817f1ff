"""GPU: `dashing-amd dist --cluster FLOAT --linkage single|complete|average` -- single, given or not, is `--cluster` byte for
byte; complete and average equal the numpy model (tests/linkage_ref.py) over the values `--threshold` emits for the same
command line; the combination with --stats; the refusals."""
import os

import numpy as np
import pytest

import linkage_ref as R
from dashing_amd import synth
from test_gpu_cli_cluster import cli, hlls, parse_cluster_bin, want_text  # noqa: F401  (hlls: the fixture)
from test_gpu_cli_threshold import parse_bin

pytestmark = pytest.mark.gpu


def dense_tri(common, flags, n, tmp_path, cwd, everything):
    """the triangle's values through --threshold at a value everything finite passes (what does not pass stays NaN)"""
    b = tmp_path / "all.bin"
    cli(*common, *flags, "--threshold", everything, "-b", "-O", b, "-o", os.devnull, cwd=cwd)
    rp, col, val = parse_bin(b.read_bytes())
    assert rp.size == n + 1
    v = np.full((n, n), np.nan, np.float32)
    rows = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    v[rows, col] = val
    v[col, rows] = val
    return R.tri_of(v)


def check(common, names, flags, rt_name, op, desc, thresholds, tmp_path, cwd=None, single=True):
    """at every threshold complete and average equal the model, in text and with -b; at the first one, with `single`, also:
    --linkage single is --cluster byte for byte, and the clusters lie inside the components.  (Every step is a process of
    its own, so the steps are few.)"""
    n = len(names)
    tri = dense_tri(common, flags, n, tmp_path, cwd, "-1e30" if desc else "1e30")
    out = {}
    for x, t in enumerate(thresholds):
        comps = None
        if single and x == 0:
            plain = cli(*common, *flags, "--cluster", t, "-o", os.devnull, cwd=cwd).stdout
            assert cli(*common, *flags, "--cluster", t, "--linkage", "single", "-o", os.devnull, cwd=cwd).stdout == plain
            pb, sb = tmp_path / "plain.bin", tmp_path / "single.bin"
            cli(*common, *flags, "--cluster", t, "-b", "-O", pb, "-o", os.devnull, cwd=cwd)
            cli(*common, *flags, "--cluster", t, "--linkage", "single", "-b", "-O", sb, "-o", os.devnull, cwd=cwd)
            assert pb.read_bytes() == sb.read_bytes()
            comps, _ = parse_cluster_bin(pb.read_bytes(), n)
        for name in ("complete", "average"):
            lab, nc = R.labels(n, tri, desc, t, R.NAMES[name])
            if x == 0:
                text = cli(*common, *flags, "--cluster", t, "--linkage", name, "-o", os.devnull, cwd=cwd).stdout.decode().split("\n")
                want = want_text(names, lab, rt_name, op, t)
                want[0] += "\t" + name
                assert text[-1] == "" and text[:-1] == want, (t, name)
            cb = tmp_path / "cl.bin"
            cli(*common, *flags, "--cluster", t, "--linkage", name, "-b", "-O", cb, "-o", os.devnull, cwd=cwd)
            got, gc = parse_cluster_bin(cb.read_bytes(), n)
            assert np.array_equal(got, lab) and gc == nc, (t, name)
            if comps is not None:
                assert np.array_equal(comps[got], comps)  # inside the components
            out[(t, name)] = (lab, nc)
    return out


def test_presketched(hlls, tmp_path):
    d, names = hlls
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", *names]
    res = check(common, names, ("-M",), "MASH_DIST", "<=", 0, (0.03, 0.2), tmp_path, cwd=d)
    assert res[(0.03, "complete")][1] >= 8  # at least the families
    res = check(common, names, (), "JI", ">=", 1, (0.5,), tmp_path, cwd=d, single=False)
    assert res[(0.5, "complete")][1] >= 8


def test_groups_and_stats(hlls, tmp_path):
    d, names = hlls
    groups = ["g%d" % (i % 10) for i in range(len(names))]
    (tmp_path / "groups.tsv").write_text("".join("%s\t%s\n" % (s, g) for s, g in zip(names, groups)))
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", "--groups", tmp_path / "groups.tsv", *names]
    check(common, ["g%d" % i for i in range(10)], ("-M",), "MASH_DIST", "<=", 0, (0.05,), tmp_path, cwd=d, single=False)
    # --stats: every line gains its three fields behind the same first three; -b appends behind the same labels
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", "-M", *names]
    for name in ("complete",):  # (--stats sees labels, whatever made them: one linkage)
        plain = cli(*common, "--cluster", 0.2, "--linkage", name, "-o", os.devnull, cwd=d).stdout.decode().split("\n")
        stats = cli(*common, "--cluster", 0.2, "--linkage", name, "--stats", "-o", os.devnull, cwd=d).stdout.decode().split("\n")
        assert stats[0] == plain[0] and len(stats) == len(plain)
        cluster_of = {}
        for a, b in zip(plain[1:-1], stats[1:-1]):
            fa, fb = a.split("\t"), b.split("\t")
            assert fb[:3] == fa and len(fb) == 6
            cluster_of[fa[0]] = fa[1]
        for b in stats[1:-1]:
            fb = b.split("\t")
            assert cluster_of[fb[3]] == fb[1]  # the medoid is a member of the cluster
            if name == "complete" and fb[4] != "-":  # ('-': the input has no other member)
                assert float(fb[5]) <= 0.2 * (1 + 1e-5)  # the worst value inside a complete-linkage cluster passes (%.6g)
        pb, sb = tmp_path / "p.bin", tmp_path / "s.bin"
        cli(*common, "--cluster", 0.2, "--linkage", name, "-b", "-O", pb, "-o", os.devnull, cwd=d)
        cli(*common, "--cluster", 0.2, "--linkage", name, "--stats", "-b", "-O", sb, "-o", os.devnull, cwd=d)
        assert sb.read_bytes()[: len(pb.read_bytes())] == pb.read_bytes() and len(sb.read_bytes()) == len(pb.read_bytes()) + 20 * len(names)


def test_dist_by_seq(tmp_path):
    base = synth.synthetic_genomes(6, 30000, seed=0xB5E0)
    f = tmp_path / "multi.fna"
    f.write_bytes(b"".join(synth.to_fasta(g[: 20000 + 900 * i], "rec%d" % i) for i, g in enumerate(base)) + synth.to_fasta(base[1][:20900], "again"))
    names = ["rec%d" % i for i in range(6)] + ["again"]
    res = check(["dist_by_seq", f], names, ("-M",), "MASH_DIST", "<=", 0, (0.0,), tmp_path, single=False)
    assert res[(0.0, "complete")][1] < 7  # rec1 and `again` are the same sequence: Mash 0


def test_refusals(hlls):
    d, names = hlls
    common = ["dist", "--presketched", "-S", 10, *names[:3]]
    r = cli(*common, "--linkage", "complete", "-o", os.devnull, cwd=d, ok=False)
    assert b"--linkage goes with --cluster" in r.stderr
    r = cli(*common, "--cluster", "0.1", "--linkage", "ward", "-o", os.devnull, cwd=d, ok=False)
    assert b"single, complete or average" in r.stderr
    r = cli(*common, "--cluster", "0.1", "--linkage", "average", "--sizes", "-o", os.devnull, cwd=d, ok=False)
    assert b"--sizes" in r.stderr
    r = cli(*common, "--cluster", "0.1", "--linkage", "complete", "--threshold", "0.1", "-o", os.devnull, cwd=d, ok=False)
    assert b"--cluster" in r.stderr and b"--threshold" in r.stderr
    r = cli(*common, "--cluster", "0.1", "--linkage", "complete", "--representatives", "0.1", "-o", os.devnull, cwd=d, ok=False)
    assert b"--representatives" in r.stderr
