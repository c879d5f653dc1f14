"""phaser_ae_test (phaser_amd/ae_test.py, K_binom and K_bh in phaser_amd/csrc/phz_aetest.hip, the host stages in phz_aematrix.cpp).

CPU tests: both kernels under the host emulation -- the product build and one with PHZ_AETEST_GRID=3, where workgroups are reused -- K_binom against
scipy.stats.binomtest on one fixed case list within a tolerance derived from lgamma's error, K_bh bit for bit against
scipy.stats.false_discovery_control; the native parser against a plain Python parse, the native row writer against Python's '%.6g'; the argument
errors; the whole tool on the emulated kernels against the restatement.  GPU tests: the same lists on the product kernels, PHZ_DEVICE against
PHZ_HOST, and the CLI on plain, BGZF and gene_ae input."""
import ctypes as C
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

import ae_test_restatement as R

HIPEMU = os.path.join(REPO, "tests", "hipemu")
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
EMU_DIR = os.path.join(HIPEMU, "_build", "aetest")

# The largest error of K_binom over the fixed list, in units of max(E(n), 2^-46) (ae_test_restatement.binom_error_units), measured against scipy:
F_EMULATED = 1.249      # the emulated kernel (the host's libm lgamma): at k 28, n 79, p0 1/3
F_GPU = 1.169           # the product kernel on an MI355X (the device library's lgamma): at k 49, n 101, p0 1/3
BINOM_F = 4 * max(F_EMULATED, F_GPU)          # math libraries differ by an ulp or so between versions


# ------------------------------------------------------------------------------------------------ the kernels under the emulation
def _emu_lib(grid=None):
    from phaser_amd import _lib
    os.makedirs(EMU_DIR, exist_ok=True)
    tag = "" if grid is None else "_g%d" % grid
    lib = os.path.join(EMU_DIR, "libphz_aetest%s.so" % tag)
    srcs = [os.path.join(CSRC, "phz_api.hip"), os.path.join(CSRC, "phz_aetest.hip"), os.path.join(HIPEMU, "hipemu.cpp")]
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(REPO, "include", "phz.h"), os.path.join(HIPEMU, "hipemu.h")]
    newest = max(os.path.getmtime(p) for p in srcs + hdrs)
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        import fcntl
        with open(os.path.join(EMU_DIR, ".lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            flags = ["-O1", "-std=c++17", "-fPIC", "-I" + os.path.join(HIPEMU, "include"), "-I" + os.path.join(REPO, "include"), "-I" + CSRC]
            defs = [] if grid is None else ["-DPHZ_AETEST_GRID=%d" % grid]
            objs = []
            for src in srcs:
                obj = os.path.join(EMU_DIR, os.path.basename(src) + tag + ".o"); objs.append(obj)
                lang = [] if src.endswith(".cpp") else ["-x", "c++"]
                subprocess.check_call(["g++"] + flags + defs + lang + ["-c", src, "-o", obj])
            subprocess.check_call(["g++", "-shared", "-fPIC"] + objs + ["-o", lib + ".tmp", "-lpthread"])
            os.replace(lib + ".tmp", lib)
    L = C.CDLL(lib)
    for name in ("phz_ctx_create", "phz_ctx_destroy", "phz_last_error", "phz_strerror", "phz_binom_test", "phz_bh_adjust"):
        res, args = _lib.SYMBOLS[name]
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


class EmuCtx:
    """what ae_test needs of a _lib.Context, on the emulated library"""

    def __init__(self, grid=None):
        self.lib = _emu_lib(grid)
        self.h = C.c_void_p()
        assert self.lib.phz_ctx_create(0, C.byref(self.h)) == 0

    def close(self):
        self.lib.phz_ctx_destroy(self.h)


@pytest.fixture(scope="module", params=[None, 3], ids=["grid_default", "grid_3"])
def emu(request):
    from phaser_amd import _lib
    _lib.build()
    ctx = EmuCtx(request.param)
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------ K_binom
@functools.lru_cache(maxsize=None)
def binom_reference():
    """{p0: (a, b, scipy p-values, near-tie mask)} of the fixed list, computed once"""
    out = {}
    for p0, (a, b) in R.binom_cases().items():
        ref = R.scipy_binom(a, b, p0, 0)
        tie = np.array([R.near_tie(int(x), int(x + y), p0) for x, y in zip(a, b)])
        for arr in (a, b, ref, tie):
            arr.setflags(write=False)
        out[p0] = (a, b, ref, tie)
    return out


def test_binom_case_list_covers_the_edges_and_has_few_near_ties():
    ref = binom_reference()
    total = sum(len(v[0]) for v in ref.values()); ties = sum(int(v[3].sum()) for v in ref.values())
    assert 2900 <= total <= 3400 and min(len(v[0]) for v in ref.values()) > 3 * 256
    assert ties <= 0.01 * total, (ties, total)
    for p0, (a, b, p, tie) in ref.items():
        n = a.astype(np.int64) + b
        assert not np.isnan(p).any()
        assert np.any((a == 0) & (n == 200000)) and np.any((b == 0) & (n == 200000)) and np.any(p < 1e-250)          # pmf underflow
        assert np.any(a.astype(np.float64) == p0 * n)                                          # k == p0 * n exactly
    a, b, p, tie = ref[1.0 / 3.0]
    assert p[(a == 0) & (b == 2)][0] == pytest.approx(1.0)                                     # the exact tie pmf(0) = pmf(1) at n = 2
    a, b, p, tie = ref[0.05]
    assert np.any((a == 1) & (b == 0))                                                         # k = n = 1: no far-side index qualifies


def _assert_binom_matches_scipy(lib, handle, what):
    """every p0 of the fixed list at test counts 1, 63, 65, 257 and all; -> the largest error in units of max(E(n), 2^-46)"""
    from phaser_amd import ae_test
    worst = 0.0
    for p0, (a, b, ref, tie) in binom_reference().items():
        got = ae_test.binom_test(lib, handle, a, b, p0, 0)
        for count in (1, 63, 65, 257):
            part = ae_test.binom_test(lib, handle, a[:count], b[:count], p0, 0)
            assert np.array_equal(part.view(np.uint64), got[:count].view(np.uint64)), (what, p0, count)
        assert not np.isnan(got).any() and np.all(got >= 0) and np.all(got <= 1), (what, p0)
        n = a.astype(np.int64) + b
        units = R.binom_error_units(got, ref, n)
        units[tie] = 0.0
        i = int(np.argmax(units))
        print("%s p0 %.4g: F = %.3f at k %d n %d (ours %.17g scipy %.17g)" % (what, p0, units[i], a[i], n[i], got[i], ref[i]))
        worst = max(worst, float(units[i]))
        assert units[i] <= BINOM_F, (what, p0, int(a[i]), int(n[i]), got[i], ref[i], float(units[i]))
    print("%s: largest F over the list %.3f (asserted at %.3f)" % (what, worst, BINOM_F))
    return worst


def test_kbinom_emulated_matches_binomtest(emu):
    _assert_binom_matches_scipy(emu.lib, emu.h, "emulated")


UNTESTED_A = np.array([-1, 3, -1, 0, 3, 7, 4, 8, 0, 2 ** 31 - 1, 5], dtype=np.int32)
UNTESTED_B = np.array([5, -1, -1, 0, 4, 0, 4, 0, 8, -1, 1], dtype=np.int32)


def _assert_untested_cells(lib, handle):
    """min_cov 8: a negative count, n = 0 and n < 8 give NaN (scipy is not called there); n = 8 is tested.  min_cov 0 and -3 test from n = 1."""
    from phaser_amd import ae_test
    got = ae_test.binom_test(lib, handle, UNTESTED_A, UNTESTED_B, 0.5, 8)
    want = R.scipy_binom(UNTESTED_A, UNTESTED_B, 0.5, 8)
    assert np.isnan(want).tolist() == [True, True, True, True, True, True, False, False, False, True, True]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-12, atol=0)
    for mc in (0, 1, -3):
        got = ae_test.binom_test(lib, handle, UNTESTED_A, UNTESTED_B, 0.5, mc)
        assert np.isnan(got).tolist() == [True, True, True, True, False, False, False, False, False, True, False], mc


def test_kbinom_emulated_untested_cells_are_nan(emu):
    _assert_untested_cells(emu.lib, emu.h)


def test_kbinom_argument_errors(emu):
    from phaser_amd import _lib
    a = np.array([5, 2 ** 31 - 1], dtype=np.int32); b = np.array([5, 1], dtype=np.int32); p = np.full(2, -5.0)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    for p0 in (0.0, 1.0, -0.25, 1.5, float("nan")):
        assert emu.lib.phz_binom_test(emu.h, 1, vp(a), vp(b), p0, 8, vp(p), _lib.PHZ_HOST) == _lib.PHZ_E_ARG, p0
    assert b"strictly between 0 and 1" in emu.lib.phz_last_error(emu.h)
    assert emu.lib.phz_binom_test(emu.h, 2, vp(a), vp(b), 0.5, 8, vp(p), _lib.PHZ_HOST) == _lib.PHZ_E_ARG          # a + b = 2^31
    assert b"int32" in emu.lib.phz_last_error(emu.h)
    assert np.all(p == -5.0)
    assert emu.lib.phz_binom_test(emu.h, 1, vp(a), vp(b), 0.5, 8, vp(p), _lib.PHZ_HOST) == _lib.PHZ_OK and p[0] == 1.0 and p[1] == -5.0


# ------------------------------------------------------------------------------------------------ K_bh
def bh_matrices(kernel_p):
    """[(name, p matrix)]: 1, 3 and 65 columns; column sizes 0 (all NaN), 1, 2, 1023, 1024, 1025 and 4097; NaN interleaved, blocks of tied values, p = 1,
    p = 0; the 65-column matrix is drawn from the doubles K_binom produced"""
    rng = np.random.default_rng(17)
    one = rng.uniform(0, 1, (4097, 1))
    one[rng.integers(0, 4097, 300), 0] = one[5, 0]; one[1000:1100, 0] = 1.0; one[2000:2040, 0] = one[7, 0]; one[3, 0] = 0.0
    three = np.full((1100, 3), np.nan)
    for c, m in enumerate((1023, 1024, 1025)):
        rows = np.sort(rng.choice(1100, m, replace=False))
        v = rng.uniform(0, 1, m) ** 3
        v[rng.integers(0, m, m // 5)] = v[0]; v[rng.integers(0, m, 7)] = 1.0
        three[rows, c] = v
    wide = np.full((70, 65), np.nan)
    sizes = [0, 1, 2, 70, 64, 65, 3] + rng.integers(0, 71, 58).tolist()
    for c, m in enumerate(sizes):
        rows = rng.choice(70, m, replace=False)
        wide[rows, c] = rng.choice(kernel_p, m)
    wide[:, 3] = 1.0                                          # a column of p = 1 alone
    return [("4097x1", one), ("1100x3", three), ("70x65", wide), ("1x1", np.array([[0.25]])), ("0x3", np.zeros((0, 3))), ("2x2 untested", np.full((2, 2), np.nan))]


def _assert_bh_bit_equal(lib, handle, kernel_p, what):
    from phaser_amd import ae_test
    for name, pm in bh_matrices(kernel_p):
        want_q, want_nt = R.scipy_bh(pm)
        got_q, got_nt = ae_test.bh_adjust(lib, handle, pm)
        assert np.array_equal(got_nt, want_nt), (what, name, got_nt.tolist(), want_nt.tolist())
        assert np.array_equal(np.isnan(got_q), np.isnan(pm)), (what, name)
        ok = ~np.isnan(pm)
        assert np.array_equal(got_q[ok].view(np.uint64), want_q[ok].view(np.uint64)), (what, name)


def test_kbh_emulated_is_bit_equal_to_false_discovery_control(emu):
    from phaser_amd import ae_test
    a, b, ref, tie = binom_reference()[0.5]
    kernel_p = ae_test.binom_test(emu.lib, emu.h, a, b, 0.5, 0)
    _assert_bh_bit_equal(emu.lib, emu.h, kernel_p, "emulated")


# ------------------------------------------------------------------------------------------------ host stages
MATRIX = ("#contig\tstart\tstop\tname\tS1\tS2\tS3\n"
          "chr1\t100\t200\tG1\t10|2\t\t0|0\r\n"
          "chr1\t300\t400\tG2\t5|x\t7|7\t3|4|5\n"
          "\n"
          "chr1\t500\t600\tG3\t12|30\n"
          "chr2\t10\t20\tG4\t2147483647|0\t2147483647|1\t2147483648|0\t9|9\n"
          "chr2\t30\t40\n"
          "chr2\t50\t60\tG6\t 1|2\t1| 2\t-1|2\n"
          "chr2\t70\t80\tG7\t|4\t4|\t00012|0")


def test_aematrix_parse_equals_a_python_parse():
    from phaser_amd import _lib, ae_test
    _lib.build()
    rng = np.random.default_rng(3)
    big = ["#contig\tstart\tstop\tname\t" + "\t".join("s%d" % i for i in range(7))]
    for r in range(2000):
        cells = ["%d|%d" % (rng.integers(0, 5000), rng.integers(0, 5000)) if rng.random() > 0.1 else rng.choice(["", "0|0", "x", "3|"]) for _ in range(7)]
        big.append("chr%d\t%d\t%d\tgene%d\t" % (r % 3, r, r + 5, r) + "\t".join(cells) + ("\r" if r % 17 == 0 else ""))
    for text in (MATRIX, MATRIX + "\n", "\n".join(big) + "\n", "#contig\tstart\tstop\tname\tS1\n", "#a\tb\n1\t2\n"):
        header, leads, a, b = R.py_parse(text)
        for threads in (1, 5):
            mx = ae_test.Matrix(text.encode(), threads)
            assert mx.header == header and mx.samples == header.split("\t")[4:]
            assert [text.encode()[o:o + n].decode() for o, n in zip(mx.lead_off.tolist(), mx.lead_len.tolist())] == leads
            assert np.array_equal(mx.a, a) and np.array_equal(mx.b, b), (mx.a.tolist(), a.tolist())
    header, leads, a, b = R.py_parse(MATRIX)
    assert a.tolist() == [[10, -1, 0], [-1, 7, -1], [12, -1, -1], [2147483647, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, 12]]
    with pytest.raises(ae_test.FatalError):
        ae_test.Matrix(b"\n\r\n", 1)


def test_aetest_rows_are_byte_equal_to_python_formatting():
    from phaser_amd import _lib, ae_test
    _lib.build()
    rng = np.random.default_rng(4)
    n = 3000
    lines = ["#contig\tstart\tstop\tname\tA\tB\tC"] + ["chr1\t%d\t%d\tg%d\t1|1\t2|2\t3|3" % (i, i + 1, i) for i in range(n)]
    text = ("\n".join(lines) + "\n").encode()
    v = np.exp(rng.uniform(-700, 0, (n, 3)))
    v[rng.random((n, 3)) < 0.2] = np.nan
    v[0] = [0.0, 1.0, 0.05]; v[1] = [1e-5, 9.9999995e-5, 0.000123456789]; v[2] = [5e-324, 1e-300, 0.99999949]; v[3] = [0.1234565, 0.1234575, 1e-4]
    v[4] = [float("inf"), float("-inf"), 123456.5]
    want = lines[0] + "\n" + "".join("chr1\t%d\t%d\tg%d\t" % (i, i + 1, i) + "\t".join("NA" if x != x else "%.6g" % x for x in v[i].tolist()) + "\n" for i in range(n))
    for threads in (1, 7):
        mx = ae_test.Matrix(text, threads)
        assert mx.rows_text(v, threads) == want.encode()
    empty = ae_test.Matrix(b"#contig\tstart\tstop\tname\tA\n", 1)
    assert empty.rows_text(np.zeros((0, 1)), 1) == b"#contig\tstart\tstop\tname\tA\n"


@pytest.mark.parametrize("argv,line", [(["--null", "0"], "FATAL ERROR - --null must lie strictly between 0 and 1"),
                                       (["--null", "1"], "FATAL ERROR - --null must lie strictly between 0 and 1"),
                                       (["--null", "nan"], "FATAL ERROR - --null must lie strictly between 0 and 1"),
                                       (["--fdr", "-0.01"], "FATAL ERROR - --fdr must lie between 0 and 1"),
                                       (["--fdr", "1.5"], "FATAL ERROR - --fdr must lie between 0 and 1")])
@pytest.mark.parametrize("mode", ["--bed", "--gene_ae"])
def test_argument_errors_print_a_line_and_exit_1(tmp_path, capsys, argv, line, mode):
    from phaser_amd import ae_test
    src = os.path.join(str(tmp_path), "in.txt")
    open(src, "w").write(MATRIX)
    assert ae_test.main([mode, src, "--o", os.path.join(str(tmp_path), "out")] + argv) == 1
    assert line in capsys.readouterr().out.split("\n")
    assert sorted(os.listdir(str(tmp_path))) == ["in.txt"]


# ------------------------------------------------------------------------------------------------ the tool against the restatement
SIX_BY_THREE = ("#contig\tstart\tstop\tname\tS1\tS2\tS3\n"
                "chr1\t100\t200\tG1\t100|20\t30|0\t0|0\n"
                "chr1\t300\t400\tG2\t5|4\t0|25\t\n"
                "chr1\t500\t600\tG3\t40|38\t1|2\t300|200\n"
                "chr2\t10\t20\tG4\t7|0\t500|510\t17|3\n"
                "chr2\t30\t40\tG5\t4|4\t60|15\tbad\n"
                "chr3\t5\t50\tG6\t1000|1200\t9|9\t2|30\n")
GENE_AE = ("contig\tstart\tstop\tname\taCount\tbCount\ttotalCount\tlog2_aFC\tn_variants\tvariants\tgw_phased\tbam\n" +
           "".join("chr1\t%d\t%d\tG%d\t%d\t%d\t%d\t0\t1\tv\t1\t%s\n" % (i, i + 9, i, a, b, a + b, bam)
                   for i, (a, b, bam) in enumerate([(100, 20, "x.bam"), (5, 4, "x.bam"), (0, 0, "y.bam"), (40, 38, "x.bam"), (30, 2, "y.bam"), (7, 0, "x.bam"),
                                                    (12, 12, "y.bam"), (3, 30, "y.bam"), (1000, 1200, "x.bam"), (2, 2, "y.bam")])))


def _number_close(got, want, n_max):
    """a printed %.6g number against the restatement's double: the K_binom tolerance at the largest n of the input, widened by the 6-digit rounding"""
    if want != want:
        return got == "NA"
    if got == "NA":
        return False
    g = float(got)
    if want < 1e-250:
        return g < 1e-240
    return abs(g - want) <= want * (BINOM_F * max(R.lgamma_error(n_max), 2.0 ** -46) + 5.1e-6)


def _assert_matrix_text(raw, want, values, n_max):
    lines = raw.decode().split("\n")
    assert lines[-1] == "" and lines[0] == want["header"] and len(lines) == len(want["leads"]) + 2
    for r, l in enumerate(lines[1:-1]):
        f = l.split("\t")
        assert "\t".join(f[:4]) == want["leads"][r] and len(f) == 4 + len(want["samples"])
        for c, cell in enumerate(f[4:]):
            assert _number_close(cell, values[r, c], n_max), (r, c, cell, values[r, c])


def _assert_bed_outputs(out, text, null, min_cov, fdr):
    """out: {"pvalue", "qvalue": matrix bytes, "significant", "summary": str} against the restatement: structure and NA cells exactly, numbers parsed back"""
    want = R.restate_bed(text, null, min_cov, fdr)
    n_max = int((want["a"].astype(np.int64) + want["b"]).max())
    assert not np.any((np.abs(want["q"] - fdr) <= 1e-4 * fdr) & (want["q"] != 1.0))          # no cell whose significance hangs on the last digits (a clipped q is 1 exactly)
    _assert_matrix_text(out["pvalue"], want, want["p"], n_max); _assert_matrix_text(out["qvalue"], want, want["q"], n_max)
    sig = out["significant"].split("\n")
    assert sig[0] == "gene\tsample\taCount\tbCount\tlog2_aFC\tpvalue\tqvalue" and sig[-1] == "" and len(sig) == len(want["significant"]) + 2
    for l, w in zip(sig[1:-1], want["significant"]):
        f = l.split("\t")
        assert f[:5] == [w[0], w[1], str(w[2]), str(w[3]), "%.6g" % w[4]], (l, w)
        assert _number_close(f[5], w[5], n_max) and _number_close(f[6], w[6], n_max), (l, w)
    summ = out["summary"].split("\n")
    assert summ[0] == "sample\ttested\tsignificant\tmin_pvalue" and summ[-1] == "" and len(summ) == len(want["summary"]) + 2
    for l, w in zip(summ[1:-1], want["summary"]):
        f = l.split("\t")
        assert f[:3] == [w[0], str(w[1]), str(w[2])] and _number_close(f[3], w[3], n_max), (l, w)
    return want


def _assert_gene_ae_output(body, text, null, min_cov):
    head, lines, p, q = R.restate_gene_ae(text, null, min_cov)
    got = body.split("\n")
    assert got[0] == "\t".join(head + ["pvalue", "qvalue"]) and got[-1] == "" and len(got) == len(lines) + 2
    for l, w, pv, qv in zip(got[1:-1], lines, p, q):
        f = l.split("\t")
        assert "\t".join(f[:-2]) == w and _number_close(f[-2], pv, 2200) and _number_close(f[-1], qv, 2200), (l, pv, qv)


@pytest.mark.parametrize("opt", [dict(), dict(null=0.52, min_cov=0, fdr=0.2), dict(null=1.0 / 3.0, min_cov=30, fdr=1.0), dict(fdr=0.0)])
def test_ae_test_on_emulated_kernels_matches_restatement(emu, opt):
    from phaser_amd import ae_test
    kw = dict(null=0.5, min_cov=8, fdr=0.05); kw.update(opt)
    out = ae_test.ae_test(SIX_BY_THREE, ctx=emu, threads=2, **kw)
    want = _assert_bed_outputs(out, SIX_BY_THREE, kw["null"], kw["min_cov"], kw["fdr"])
    if not opt:
        assert [w[:4] for w in want["significant"]] == [("G1", "S1", 100, 20), ("G1", "S2", 30, 0), ("G2", "S2", 0, 25), ("G3", "S3", 300, 200),
                                                        ("G4", "S3", 17, 3), ("G5", "S2", 60, 15), ("G6", "S1", 1000, 1200), ("G6", "S3", 2, 30)]
        assert "G1\tS2\t30\t0\tinf\t" in out["significant"] and "G2\tS2\t0\t25\t-inf\t" in out["significant"]
    assert ae_test.ae_test(SIX_BY_THREE, ctx=emu, threads=1, **kw) == out
    body = ae_test.ae_test_gene_ae(GENE_AE, kw["null"], kw["min_cov"], kw["fdr"], ctx=emu)
    _assert_gene_ae_output(body, GENE_AE, kw["null"], kw["min_cov"])


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_kbinom_gpu_matches_binomtest(gpu_ctx):
    _assert_binom_matches_scipy(gpu_ctx.lib, gpu_ctx.h, "gpu")
    from phaser_amd import _lib
    assert gpu_ctx.timing(_lib.PHZ_T_BINOM)[2] > 0 and gpu_ctx.timing(_lib.PHZ_T_BINOM)[0] > 0


@pytest.mark.gpu
def test_kbinom_gpu_untested_cells_are_nan(gpu_ctx):
    _assert_untested_cells(gpu_ctx.lib, gpu_ctx.h)


@pytest.mark.gpu
def test_kbh_gpu_is_bit_equal_to_false_discovery_control(gpu_ctx):
    from phaser_amd import ae_test
    a, b, ref, tie = binom_reference()[0.5]
    kernel_p = ae_test.binom_test(gpu_ctx.lib, gpu_ctx.h, a, b, 0.5, 0)
    _assert_bh_bit_equal(gpu_ctx.lib, gpu_ctx.h, kernel_p, "gpu")


@pytest.mark.gpu
def test_kbh_gpu_device_space_gives_the_bits_of_host_space(gpu_ctx):
    import torch
    from phaser_amd import _lib, ae_test
    a, b, ref, tie = binom_reference()[0.5]
    dev = torch.device("cuda", gpu_ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    # K_binom in PHZ_DEVICE space first: its doubles feed the matrices
    ta = torch.from_numpy(np.array(a)).to(dev); tb = torch.from_numpy(np.array(b)).to(dev); tp = torch.full((len(a),), -5.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    gpu_ctx.check(gpu_ctx.lib.phz_binom_test(gpu_ctx.h, len(a), p(ta), p(tb), 0.5, 0, p(tp), _lib.PHZ_DEVICE))
    kernel_p = ae_test.binom_test(gpu_ctx.lib, gpu_ctx.h, a, b, 0.5, 0)
    assert np.array_equal(tp.cpu().numpy().view(np.uint64), kernel_p.view(np.uint64))
    for name, pm in bh_matrices(kernel_p):
        host_q, host_nt = ae_test.bh_adjust(gpu_ctx.lib, gpu_ctx.h, pm)
        tpm = torch.from_numpy(pm).to(dev)
        tq = torch.full(pm.shape, -5.0, dtype=torch.float64, device=dev); tn = torch.full((pm.shape[1],), -5, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        gpu_ctx.check(gpu_ctx.lib.phz_bh_adjust(gpu_ctx.h, pm.shape[0], pm.shape[1], p(tpm), p(tq), p(tn), _lib.PHZ_DEVICE))
        assert np.array_equal(tn.cpu().numpy(), host_nt), name
        assert np.array_equal(tq.cpu().numpy().view(np.uint64), host_q.view(np.uint64)), name


def _read_outputs(prefix):
    out = {k: gzip.open("%s.%s.bed.gz" % (prefix, k), "rb").read() for k in ("pvalue", "qvalue")}
    out["significant"] = open(prefix + ".significant.txt").read(); out["summary"] = open(prefix + ".summary.txt").read()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["bgzf", "plain"])
def test_cli_gpu_bed_mode_matches_restatement(tmp_path, form, capsys):
    from phaser_amd import ae_test, vcfout
    tmp = str(tmp_path)
    if form == "bgzf":
        src = os.path.join(tmp, "m.bed.gz")
        vcfout.write_bgzf(src, SIX_BY_THREE, 2)
    else:
        src = os.path.join(tmp, "m.bed")
        open(src, "w").write(SIX_BY_THREE)
    runs = []
    for k in (0, 1):
        prefix = os.path.join(tmp, "run%d" % k, "out")
        os.makedirs(os.path.dirname(prefix))
        assert ae_test.main(["--bed", src, "--o", prefix, "--t", str(1 + k)]) == 0
        names = sorted(os.listdir(os.path.dirname(prefix)))
        assert names == ["out.pvalue.bed.gz", "out.pvalue.bed.gz.tbi", "out.qvalue.bed.gz", "out.qvalue.bed.gz.tbi", "out.significant.txt", "out.summary.txt"]
        runs.append({n: open(os.path.join(os.path.dirname(prefix), n), "rb").read() for n in names})
    assert runs[0] == runs[1]                                 # a second run (with another --t) writes identical bytes
    assert "WARNING" not in capsys.readouterr().out
    want = _assert_bed_outputs(_read_outputs(os.path.join(tmp, "run0", "out")), SIX_BY_THREE, 0.5, 8, 0.05)
    assert len(want["significant"]) == 8
    # other options, and a matrix that is not position-sorted: the warning line, no index
    lines = SIX_BY_THREE.split("\n")
    unsorted = "\n".join([lines[0], lines[3], lines[1]] + lines[4:])
    src2 = os.path.join(tmp, "u.bed"); open(src2, "w").write(unsorted)
    prefix = os.path.join(tmp, "u", "out"); os.makedirs(os.path.dirname(prefix))
    assert ae_test.main(["--bed", src2, "--o", prefix, "--null", "0.52", "--min_cov", "0", "--fdr", "0.2"]) == 0
    assert not os.path.exists(prefix + ".pvalue.bed.gz.tbi") and "is not position-sorted, no tabix index written" in capsys.readouterr().out
    _assert_bed_outputs(_read_outputs(prefix), unsorted, 0.52, 0, 0.2)


@pytest.mark.gpu
def test_cli_gpu_gene_ae_mode_matches_restatement(tmp_path):
    from phaser_amd import ae_test
    src = os.path.join(str(tmp_path), "s.gene_ae.txt")
    open(src, "w").write(GENE_AE)
    bodies = []
    for k in (0, 1):
        prefix = os.path.join(str(tmp_path), "out%d" % k)
        assert ae_test.main(["--gene_ae", src, "--o", prefix, "--min_cov", "4"]) == 0
        bodies.append(open(prefix + ".txt").read())
    assert bodies[0] == bodies[1]
    _assert_gene_ae_output(bodies[0], GENE_AE, 0.5, 4)
