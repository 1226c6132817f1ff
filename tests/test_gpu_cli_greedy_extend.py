"""GPU: `dashing-amd dist --representatives` with --assign and --extend: --assign best against the API on the same
sketches, a two-step run (the first inputs with -b, then all inputs with --extend) against the one-step run, and the
refusals."""
import os

import numpy as np
import pytest

import dashing_amd
from test_gpu_cli_greedy import cli, hlls, parse_reps_bin  # noqa: F401  (hlls: the 40 .hll files of that module)

pytestmark = pytest.mark.gpu
D = dashing_amd
CASES = [((), D.JI, (0.5, 0.02, 1.5)), (("-M",), D.MASH_DIST, (0.03, 0.2, -1.0))]


def reps_bin(common, flags, t, extra, tmp_path, cwd, name="reps.bin"):
    rb = tmp_path / name
    cli(*common, *flags, "--representatives", t, *extra, "-b", "-O", rb, "-o", os.devnull, cwd=cwd)
    return rb


def load_regs(d, names):
    import ctypes as C

    host = C.CDLL(os.path.join(os.path.dirname(D.lib_path()), "libdashing_host.so"))
    host.dshh_read_hll.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    regs = np.zeros((len(names), 1 << 10), np.uint8)
    for i, nm in enumerate(names):
        p = C.c_int()
        assert host.dshh_read_hll(str(d / nm).encode(), regs[i].ctypes.data, regs[i].size, C.byref(p)) == 0 and p.value == 10
    return regs


@pytest.mark.parametrize("flags,rt,ts", CASES)
def test_assign_best_equals_the_api(ctx, hlls, tmp_path, flags, rt, ts):
    d, names = hlls
    n = len(names)
    common = ["dist", "--presketched", "-S", 10, "--avoid-sorting", *names]
    ctx.set_sketches(load_regs(d, names))
    differ = 0
    for t in ts:
        for mname in ("first", "best"):
            got, gr = parse_reps_bin(reps_bin(common, flags, t, ("--assign", mname), tmp_path, d).read_bytes(), n)
            want, wr = ctx.greedy_extend(float(np.float32(t)), 0, None, mname, estim=2, result_type=rt, k=31)
            assert np.array_equal(got, want) and gr == wr, (t, mname)
        plain, pr = parse_reps_bin(reps_bin(common, flags, t, (), tmp_path, d).read_bytes(), n)
        first, _ = ctx.greedy_extend(float(np.float32(t)), 0, None, "first", estim=2, result_type=rt, k=31)
        assert np.array_equal(plain, first)  # without --assign: the first representative, as before
        differ += int((got != first).sum())
        # text: the value column is the pair's value under either mode
        out = cli(*common, *flags, "--representatives", t, "--assign", "best", "-o", os.devnull, cwd=d).stdout.decode().split("\n")
        assert out[-1] == "" and len(out) == n + 2 and out[0].startswith("#Representatives\t")
        reps = sorted(set(got.tolist()))
        for x, line in enumerate(out[1:-1]):
            f = line.split("\t")
            assert f[0] == names[x] and int(f[1]) == reps.index(int(got[x])) and f[2] == names[int(got[x])], line
            if got[x] == x:
                assert f[3] == "-"
            else:
                v = ctx.dist_pairs([x], [int(got[x])], result_types=(rt,), estim=2, k=31)[0, 0]
                assert f[3] == "%.6g" % v, line
    print("labels that differ between --assign best and first over the thresholds:", differ)


@pytest.mark.parametrize("flags,rt,ts", CASES)
def test_two_steps_equal_one(hlls, tmp_path, flags, rt, ts):
    d, names = hlls
    n, m = len(names), 25
    for t in ts:
        for mname in ("first", "best"):
            one = reps_bin(["dist", "--presketched", "-S", 10, "--avoid-sorting", *names], flags, t, ("--assign", mname), tmp_path, d, "one.bin").read_bytes()
            old = reps_bin(["dist", "--presketched", "-S", 10, "--avoid-sorting", *names[:m]], flags, t, ("--assign", mname), tmp_path, d, "old.bin")
            assert parse_reps_bin(old.read_bytes(), m)[0].tolist() == parse_reps_bin(one, n)[0][:m].tolist()  # the prefix property
            two = reps_bin(["dist", "--presketched", "-S", 10, "--avoid-sorting", *names], flags, t, ("--assign", mname, "--extend", old), tmp_path, d, "two.bin").read_bytes()
            assert two == one, (t, mname)
            # text keeps its format
            a = cli("dist", "--presketched", "-S", 10, "--avoid-sorting", *names, *flags, "--representatives", t, "--assign", mname, "-o", os.devnull, cwd=d).stdout
            b = cli("dist", "--presketched", "-S", 10, "--avoid-sorting", *names, *flags, "--representatives", t, "--assign", mname, "--extend", old, "-o", os.devnull, cwd=d).stdout
            assert a == b and a.startswith(b"#Representatives\t")
    # --extend alone means --assign first; an old file of all n inputs is copied and counted
    whole = reps_bin(["dist", "--presketched", "-S", 10, "--avoid-sorting", *names], flags, ts[0], (), tmp_path, d, "whole.bin")
    again = reps_bin(["dist", "--presketched", "-S", 10, "--avoid-sorting", *names], flags, ts[0], ("--extend", whole), tmp_path, d, "again.bin")
    assert again.read_bytes() == whole.read_bytes()


def test_refusals(hlls, tmp_path):
    d, names = hlls
    base = ["dist", "--presketched", "-S", 10]
    old = reps_bin([*base, "--avoid-sorting", *names[:10]], (), 0.5, (), tmp_path, d, "old.bin")
    # without --avoid-sorting
    r = cli(*base, "--representatives", 0.5, "--extend", old, "-o", os.devnull, *names, cwd=d, ok=False)
    assert b"--extend" in r.stderr and b"--avoid-sorting" in r.stderr
    # n_old > n
    r = cli(*base, "--avoid-sorting", "--representatives", 0.5, "--extend", old, "-o", os.devnull, *names[:9], cwd=d, ok=False)
    assert b"--extend" in r.stderr and b"10" in r.stderr
    # a file of the wrong length, a file that is none, a missing file
    cut = tmp_path / "cut.bin"
    cut.write_bytes(old.read_bytes()[:-4])
    short = tmp_path / "short.bin"
    short.write_bytes(b"\x01\x02\x03")
    for f in (cut, short, tmp_path / "none.bin"):
        r = cli(*base, "--avoid-sorting", "--representatives", 0.5, "--extend", f, "-o", os.devnull, *names, cwd=d, ok=False)
        assert b"--extend" in r.stderr
    # labels the library refuses: slot 3 points behind itself
    bad = np.frombuffer(old.read_bytes(), np.uint8).copy()
    bad[16 + 4 * 3] = 7
    (tmp_path / "bad.bin").write_bytes(bad.tobytes())
    r = cli(*base, "--avoid-sorting", "--representatives", 0.5, "--extend", tmp_path / "bad.bin", "-o", os.devnull, *names, cwd=d, ok=False)
    assert b"labels_in[3]" in r.stderr
    # --assign and --extend go with --representatives only, and wherever that is refused
    assert b"--assign" in cli(*base, "--assign", "best", "-o", os.devnull, *names[:3], cwd=d, ok=False).stderr
    assert b"--assign" in cli(*base, "--representatives", 0.5, "--assign", "nearest", *names[:3], cwd=d, ok=False).stderr
    assert b"--extend" in cli(*base, "--avoid-sorting", "--extend", old, "-o", os.devnull, *names, cwd=d, ok=False).stderr
    r = cli(*base, "--avoid-sorting", "--representatives", 0.5, "--extend", old, "--cluster", 0.1, "-o", os.devnull, *names, cwd=d, ok=False)
    assert b"--representatives" in r.stderr and b"--cluster" in r.stderr
    r = cli(*base, "--avoid-sorting", "--representatives", 0.5, "--assign", "best", "-U", "-o", os.devnull, *names, cwd=d, ok=False)
    assert b"--representatives" in r.stderr and b"-U" in r.stderr
