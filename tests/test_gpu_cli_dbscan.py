"""GPU: `dashing-amd dist --cluster FLOAT --min-pts N [--assign first|best]` -- the text and -b outputs over a small FASTA set
against Context.dbscan_threshold over the same sketches; over .hll files, groups and records against the numpy model
(tests/dbscan_ref.py) over the pairs `--threshold` emits for the same command line; the combination with --stats; the refusals;
and a run without --min-pts is `--cluster` as it was, byte for byte."""
import os

import numpy as np
import pytest

import cluster_ref
import dbscan_ref
from dashing_amd import synth
from test_gpu_cli_cluster import cli, hlls, parse_cluster_bin, want_text  # noqa: F401  (hlls: the fixture)
from test_gpu_cli_threshold import parse_bin

pytestmark = pytest.mark.gpu
KINDS = ("noise", "border", "core")


def want_dbscan_text(names, res, measure, op, t, min_pts, assign):
    lab, kind, deg = res[:3]
    heads = sorted(x for x in range(len(names)) if kind[x] == dbscan_ref.CORE and lab[x] == x)  # numbered by ascending label
    index = {r: i for i, r in enumerate(heads)}
    out = ["#Cluster\t%s\t%s\t%s\tdbscan\t%d\t%s" % (measure, op, "%.6g" % np.float32(t), min_pts, assign)]
    for x, name in enumerate(names):
        where = "-\t-" if kind[x] == dbscan_ref.NOISE else "%d\t%s" % (index[int(lab[x])], names[int(lab[x])])
        out.append("%s\t%s\t%s\t%d" % (name, where, KINDS[kind[x]], deg[x]))
    return out


def parse_dbscan_bin(raw, n, extra=0):
    """u64 n, u64 n_clusters, u32 labels[n], u32 degree[n], u8 kind[n] (and `extra` bytes of --stats behind)"""
    hdr = np.frombuffer(raw[:16], np.uint64)
    assert int(hdr[0]) == n and len(raw) == 16 + 9 * n + extra
    return (np.frombuffer(raw[16 : 16 + 4 * n], np.uint32), np.frombuffer(raw[16 + 8 * n : 16 + 9 * n], np.uint8),
            np.frombuffer(raw[16 + 4 * n : 16 + 8 * n], np.uint32), int(hdr[1]))


def check_outputs(common, names, flags, res, measure, op, t, min_pts, assign, tmp_path, cwd=None):
    args = (*common, *flags, "--cluster", t, "--min-pts", min_pts) + (("--assign", assign) if assign != "first" else ())
    text = cli(*args, "-o", os.devnull, cwd=cwd).stdout.decode().split("\n")
    assert text[-1] == "" and text[:-1] == want_dbscan_text(names, res, measure, op, t, min_pts, assign), (t, min_pts, assign)
    b = tmp_path / "db.bin"
    cli(*args, "-b", "-O", b, "-o", os.devnull, cwd=cwd)
    lab, kind, deg, nc = parse_dbscan_bin(b.read_bytes(), len(names))
    assert np.array_equal(lab, res[0]) and np.array_equal(kind, res[1]) and np.array_equal(deg, res[2]) and nc == res[3], (t, min_pts, assign)


def model_of_threshold(common, flags, n, t, min_pts, assign, desc, tmp_path, cwd):
    """the model over the pairs --threshold emits for the same command line"""
    b = tmp_path / "thr.bin"
    cli(*common, *flags, "--threshold", t, "-b", "-O", b, "-o", os.devnull, cwd=cwd)
    rp, col, val = parse_bin(b.read_bytes())
    assert rp.size == n + 1
    return dbscan_ref.dbscan(n, *cluster_ref.csr_edges(rp, col), val, min_pts, assign, desc)


@pytest.fixture(scope="module")
def fastas(tmp_path_factory):
    """cuts of three genomes that slide along them (neighbouring cuts are close, cuts further apart less so) and two genomes of
    their own"""
    d = tmp_path_factory.mktemp("dbfa")
    base = synth.synthetic_genomes(5, 60000, seed=0xDB5C)
    paths, raws = [], []
    for g, cuts in ((0, 6), (1, 4), (2, 2), (3, 1), (4, 1)):
        for v in range(cuts):
            raw = synth.to_fasta(base[g][2000 * v : 40000 + 2000 * v], "g%d_%d" % (g, v))
            p = d / ("g%d_%d.fna" % (g, v))
            p.write_bytes(raw)
            paths.append(str(p))
            raws.append(raw)
    order = np.random.default_rng(11).permutation(len(paths))  # a cluster's smallest core is not its first member
    return [paths[i] for i in order], [raws[i] for i in order]


def test_fasta_inputs_against_the_context(ctx, fastas, tmp_path):
    paths, raws = fastas
    n = len(paths)
    ctx.alloc(n, 10)
    ctx.clear()
    assert not ctx.sketch_fastx_batch(raws, k=31).any()
    seen = np.zeros(3, np.int64)
    for flags, rt, measure, op, t, min_pts, assign in (((), 1, "JI", ">=", 0.8, 4, "first"), ((), 1, "JI", ">=", 0.7, 5, "best"),
                                                       (("-M",), 0, "MASH_DIST", "<=", 0.01, 3, "best")):
        res = ctx.dbscan_threshold(t, min_pts, assign, estim=2, result_type=rt, k=31)
        seen += np.bincount(res[1], minlength=3)
        check_outputs(["dist", "--avoid-sorting", *paths], paths, flags, res, measure, op, t, min_pts, assign, tmp_path)
    assert seen.min() > 0, seen  # the set shows every kind
    # without --min-pts: --cluster as it was, the documented format over dsh_cluster_threshold's labels
    lab, nc = ctx.cluster_threshold(0.8, estim=2, result_type=1, k=31)
    text = cli("dist", "--avoid-sorting", *paths, "--cluster", 0.8, "-o", os.devnull).stdout.decode().split("\n")
    assert text[-1] == "" and text[:-1] == want_text(paths, lab, "JI", ">=", 0.8)
    b = tmp_path / "cl.bin"
    cli("dist", "--avoid-sorting", *paths, "--cluster", 0.8, "-b", "-O", b, "-o", os.devnull)
    got, gc = parse_cluster_bin(b.read_bytes(), n)
    assert np.array_equal(got, lab) and gc == nc


def test_presketched_groups_and_stats(hlls, tmp_path):
    d, names = hlls
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", *names]
    res = model_of_threshold(common, ("-M",), len(names), 0.2, 4, "best", False, tmp_path, d)
    check_outputs(common, names, ("-M",), res, "MASH_DIST", "<=", 0.2, 4, "best", tmp_path, cwd=d)
    # --stats: every line gains its three fields behind the same five; -b appends behind the same bytes
    args = (*common, "-M", "--cluster", 0.2, "--min-pts", 4, "--assign", "best")
    plain = cli(*args, "-o", os.devnull, cwd=d).stdout.decode().split("\n")
    stats = cli(*args, "--stats", "-o", os.devnull, cwd=d).stdout.decode().split("\n")
    assert stats[0] == plain[0] and len(stats) == len(plain)
    for a, b in zip(plain[1:-1], stats[1:-1]):
        fa, fb = a.split("\t"), b.split("\t")
        assert fb[:5] == fa and len(fb) == 8
        assert fa[3] != "noise" or (fb[5] == fa[0] and fb[6] == "-")  # a noise point is a group of its own
    pb, sb = tmp_path / "p.bin", tmp_path / "s.bin"
    cli(*args, "-b", "-O", pb, "-o", os.devnull, cwd=d)
    cli(*args, "--stats", "-b", "-O", sb, "-o", os.devnull, cwd=d)
    assert sb.read_bytes()[: len(pb.read_bytes())] == pb.read_bytes() and len(sb.read_bytes()) == len(pb.read_bytes()) + 20 * len(names)
    # --groups: the unions take the inputs' place
    groups = ["g%d" % (i % 10) for i in range(len(names))]
    (tmp_path / "groups.tsv").write_text("".join("%s\t%s\n" % (s, g) for s, g in zip(names, groups)))
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", "--groups", tmp_path / "groups.tsv", *names]
    res = model_of_threshold(common, ("-M",), 10, 0.05, 3, "first", False, tmp_path, d)
    check_outputs(common, ["g%d" % i for i in range(10)], ("-M",), res, "MASH_DIST", "<=", 0.05, 3, "first", tmp_path, cwd=d)


def test_dist_by_seq(tmp_path):
    base = synth.synthetic_genomes(6, 30000, seed=0xB5E0)
    f = tmp_path / "multi.fna"
    f.write_bytes(b"".join(synth.to_fasta(g[: 20000 + 900 * i], "rec%d" % i) for i, g in enumerate(base)) + synth.to_fasta(base[1][:20900], "again"))
    names = ["rec%d" % i for i in range(6)] + ["again"]
    res = model_of_threshold(["dist_by_seq", f], ("-M",), 7, 0.0, 2, "first", False, tmp_path, None)
    assert res[3] >= 1 and res[4] >= 1  # rec1 and `again` are the same sequence: two cores at Mash 0; the others are noise
    check_outputs(["dist_by_seq", f], names, ("-M",), res, "MASH_DIST", "<=", 0.0, 2, "first", tmp_path)


@pytest.mark.parametrize("extra,msgs", [
    (("--min-pts", "3"), ("--min-pts goes with --cluster",)),
    (("--cluster", "0.1", "--min-pts", "3", "--linkage", "complete"), ("--min-pts", "--linkage")),
    (("--cluster", "0.1", "--min-pts", "3", "--linkage", "average"), ("--min-pts", "--linkage")),
    (("--cluster", "0.1", "--min-pts", "0"), ("--min-pts", "at least 1")),
    (("--cluster", "0.1", "--min-pts", "-2"), ("--min-pts", "at least 1")),
    (("--cluster", "0.1", "--min-pts", "three"), ("--min-pts", "at least 1")),
    (("--cluster", "0.1", "--min-pts", "3", "--assign", "nearest"), ("--assign", "'first' or 'best'")),
    (("--cluster", "0.1", "--assign", "best"), ("--assign goes with",)),
    (("--cluster", "0.1", "--min-pts", "3", "--threshold", "0.1"), ("--cluster", "--threshold")),
    (("--cluster", "0.1", "--min-pts", "3", "--nearest-neighbors", "2"), ("--cluster", "--nearest-neighbors")),
    (("--cluster", "0.1", "--min-pts", "3", "--representatives", "0.1"), ("--representatives", "--cluster")),
    (("--cluster", "0.1", "--min-pts", "3", "-U"), ("--cluster", "-U")),
    (("--cluster", "0.1", "--min-pts", "3", "-T"), ("--cluster", "-T")),
    (("--cluster", "0.1", "--min-pts", "3", "--ngpus", "2"), ("--cluster", "one device")),
    (("--cluster", "0.1", "--min-pts", "3", "--mst"), ("--mst", "--cluster")),
    (("--cluster", "0.1", "--min-pts", "3", "--stats", "--sizes"), ("--stats", "--sizes")),
])
def test_refusals(hlls, extra, msgs):
    d, names = hlls
    r = cli("dist", "--presketched", "-S", 10, *extra, "-o", os.devnull, *names[:3], cwd=d, ok=False)
    for m in msgs:
        assert m in r.stderr.decode(), r.stderr.decode()


def test_single_linkage_given_goes_with_min_pts(hlls, tmp_path):
    """--linkage single names the components, which is what the cores are united by: the same bytes with and without it"""
    d, names = hlls
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", "-M", *names[:12], "--cluster", 0.2, "--min-pts", 3, "-o", os.devnull]
    assert cli(*common, "--linkage", "single", cwd=d).stdout == cli(*common, cwd=d).stdout
