"""The overdispersed path of phaser_ae_test (phaser_amd/ae_betabinom.py, --overdispersion; K_bbfit and K_bbtest in phaser_amd/csrc/phz_aebb.hip).

CPU tests: both kernels under the host emulation in three builds -- the product macros, PHZ_AETEST_GRID=3 (workgroups are reused) and PHZ_BB_WAVE_N=32 (almost
every case takes the wave tier) -- K_bbtest against scipy.stats.betabinom on one fixed case list within a tolerance derived from lgamma's error, K_bbfit
against the restated search and a bounded Brent, judged in scipy's likelihood; equal bits across builds and runs; the argument errors; the tool on the emulated
kernels against the restatement.  GPU tests: the same lists on the product kernels, PHZ_DEVICE against PHZ_HOST, the timing slots, the CLI."""
import ctypes as C
import functools
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

import ae_betabinom_restatement as R
import ae_test_restatement as R0

HIPEMU = os.path.join(REPO, "tests", "hipemu")
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
EMU_DIR = os.path.join(HIPEMU, "_build", "aebb")
BUILDS = {"product": [], "grid_3": ["-DPHZ_AETEST_GRID=3"], "wave_32": ["-DPHZ_BB_WAVE_N=32"]}

# The largest error of K_bbtest over the fixed list, in units of max(E(N), 2^-46), N = n + (1 - rho) / rho (ae_betabinom_restatement.bb_error_units),
# measured against scipy:
F_EMULATED = 2.097    # the emulated kernels (the host's libm lgamma), the largest of the three builds: at k 1, n 232, p0 1/3, rho 0.25 (wave tier build: 2.080)
F_GPU = 2.341         # the product kernels on an MI355X (the device library's lgamma; PHZ_BB_WAVE_N 8192, and the same figure at 2048): at k 31, n 537, p0 0.05, rho 0.03
BB_F = 4 * max(F_EMULATED, F_GPU)          # math libraries differ by an ulp or so between versions

# K_bbfit over ae_betabinom_restatement.fit_matrices, measured (emulated, MI355X; K_bbfit has no tiers, PHZ_BB_WAVE_N does not enter):
#   margin 1   max(LL_scipy(rho_brent), LL_scipy(rho_grid_restated)) - LL_scipy(rho_ours)
#   margin 2   |loglik_ours - LL_scipy(rho_ours)|
#   margin 3   |ln rho_ours - ln rho_grid_restated|, in steps of the last round of the search; never asserted below one step
# All three are largest in the columns of binomial counts, where the likelihood is flat next to RHO_MIN and alpha, beta reach 5e5 (|LL| about 3,000 there).
M1_EMULATED, M1_GPU = 3.9e-6, 1.11e-6
M2_EMULATED, M2_GPU = 2.89e-6, 1.24e-6
M3_EMULATED, M3_GPU = 122.0, 427.0
FIT_M1 = 4 * max(M1_EMULATED, M1_GPU)
FIT_M2 = 4 * max(M2_EMULATED, M2_GPU)
FIT_M3_STEPS = max(4 * max(M3_EMULATED, M3_GPU), 1.0)


# ------------------------------------------------------------------------------------------------ the kernels under the emulation
def _emu_lib(tag):
    from phaser_amd import _lib
    os.makedirs(EMU_DIR, exist_ok=True)
    lib = os.path.join(EMU_DIR, "libphz_aebb_%s.so" % tag)
    srcs = [os.path.join(CSRC, "phz_api.hip"), os.path.join(CSRC, "phz_aetest.hip"), os.path.join(CSRC, "phz_aebb.hip"), os.path.join(HIPEMU, "hipemu.cpp")]
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(REPO, "include", "phz.h"), os.path.join(HIPEMU, "hipemu.h")]
    newest = max(os.path.getmtime(p) for p in srcs + hdrs)
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        import fcntl
        with open(os.path.join(EMU_DIR, ".lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            flags = ["-O1", "-std=c++17", "-fPIC", "-I" + os.path.join(HIPEMU, "include"), "-I" + os.path.join(REPO, "include"), "-I" + CSRC]
            objs = []
            for src in srcs:
                obj = os.path.join(EMU_DIR, "%s_%s.o" % (os.path.basename(src), tag)); objs.append(obj)
                lang = [] if src.endswith(".cpp") else ["-x", "c++"]
                subprocess.check_call(["g++"] + flags + BUILDS[tag] + lang + ["-c", src, "-o", obj])
            subprocess.check_call(["g++", "-shared", "-fPIC"] + objs + ["-o", lib + ".tmp", "-lpthread"])
            os.replace(lib + ".tmp", lib)
    L = C.CDLL(lib)
    for name in ("phz_ctx_create", "phz_ctx_destroy", "phz_last_error", "phz_strerror", "phz_binom_test", "phz_bh_adjust", "phz_betabinom_fit", "phz_betabinom_test"):
        res, args = _lib.SYMBOLS[name]
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


class EmuCtx:
    """what ae_test needs of a _lib.Context, on an emulated library"""

    def __init__(self, tag):
        self.lib = _emu_lib(tag)
        self.h = C.c_void_p()
        assert self.lib.phz_ctx_create(0, C.byref(self.h)) == 0

    def close(self):
        self.lib.phz_ctx_destroy(self.h)


@pytest.fixture(scope="module")
def emus():
    from phaser_amd import _lib
    _lib.build()
    ctxs = {tag: EmuCtx(tag) for tag in BUILDS}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope="module", params=list(BUILDS))
def emu(request, emus):
    return emus[request.param]


# ------------------------------------------------------------------------------------------------ K_bbtest
@functools.lru_cache(maxsize=None)
def bb_reference():
    """{p0: (a, b [rows, 4], rho [4], scipy p-values, near-tie mask)} of the fixed list (every row under every rho column), computed once"""
    out = {}
    for p0, (a, b) in R.bb_cases().items():
        rho = np.array(R.rho_columns(p0))
        a2 = np.ascontiguousarray(np.repeat(a[:, None], 4, axis=1)); b2 = np.ascontiguousarray(np.repeat(b[:, None], 4, axis=1))
        ref, tie = R.scipy_bb(a2, b2, p0, rho, 0)
        for arr in (a2, b2, rho, ref, tie):
            arr.setflags(write=False)
        out[p0] = (a2, b2, rho, ref, tie)
    return out


def test_bb_case_list_covers_the_edges_and_leaves_few_cases_out():
    ref = bb_reference()
    total = sum(v[0].size for v in ref.values()); ties = sum(int(v[4].sum()) for v in ref.values())
    print("cases %d, left out as near ties %d" % (total, ties))
    assert min(v[0].size for v in ref.values()) > 3 * 256
    assert ties <= 0.01 * total, (ties, total)
    for p0, (a, b, rho, p, tie) in ref.items():
        n = a.astype(np.int64) + b
        assert not np.isnan(p).any()
        assert np.any(p < 1e-250)                                                              # pmf underflow
        assert np.any((a == 0) & (n == 200000)) and np.any((b == 0) & (n == 200000)) and np.any(n == 1)
    a, b, rho, p, tie = ref[0.5]
    assert rho[3] == 1.0 / 3.0 and np.all(p[:, 3] >= 1 - 1e-9)                                 # the uniform column


def _assert_bb_matches_scipy(lib, handle, what):
    """every p0 of the fixed list, whole and in prefixes of 1, 63, 65, 257 cells; -> the largest error in units of max(E(N), 2^-46)"""
    from phaser_amd import ae_betabinom as bb
    worst = 0.0
    for p0, (a, b, rho, ref, tie) in bb_reference().items():
        got = bb.betabinom_test(lib, handle, a, b, p0, rho, 0)
        for count in (1, 63, 65, 257):
            for c in range(4):
                part = bb.betabinom_test(lib, handle, a[:count, c:c + 1], b[:count, c:c + 1], p0, rho[c:c + 1], 0)
                assert np.array_equal(part[:, 0].view(np.uint64), np.ascontiguousarray(got[:count, c]).view(np.uint64)), (what, p0, count, c)
        assert not np.isnan(got).any() and np.all(got >= 0) and np.all(got <= 1), (what, p0)
        n = a.astype(np.int64) + b
        units = R.bb_error_units(got, ref, n, rho[None, :])
        units[tie] = 0.0
        r, c = np.unravel_index(int(np.argmax(units)), units.shape)
        print("%s p0 %.4g: F = %.3f at k %d n %d rho %.6g (ours %.17g scipy %.17g)" % (what, p0, units[r, c], a[r, c], n[r, c], rho[c], got[r, c], ref[r, c]))
        worst = max(worst, float(units[r, c]))
        assert units[r, c] <= BB_F, (what, p0, int(a[r, c]), int(n[r, c]), float(rho[c]), got[r, c], ref[r, c], float(units[r, c]))
    print("%s: largest F over the list %.3f (asserted at %.3f)" % (what, worst, BB_F))
    return worst


def test_kbbtest_emulated_matches_scipy(emu):
    _assert_bb_matches_scipy(emu.lib, emu.h, "emulated")


UNTESTED_A = np.array([-1, 3, -1, 0, 3, 7, 4, 8, 0, 2 ** 31 - 1, 5], dtype=np.int32)
UNTESTED_B = np.array([5, -1, -1, 0, 4, 0, 4, 0, 8, -1, 1], dtype=np.int32)


def _assert_untested_cells(lib, handle):
    """min_cov 8: a negative count, n = 0 and n < 8 give NaN, n = 8 is tested; min_cov 0 and -3 test from n = 1; a NaN rho leaves its column NaN"""
    from phaser_amd import ae_betabinom as bb
    a = np.stack([UNTESTED_A, UNTESTED_A], axis=1); b = np.stack([UNTESTED_B, UNTESTED_B], axis=1)
    rho = np.array([0.02, float("nan")])
    got = bb.betabinom_test(lib, handle, a, b, 0.5, rho, 8)
    want, _ = R.scipy_bb(a, b, 0.5, rho, 8)
    assert np.isnan(want[:, 0]).tolist() == [True, True, True, True, True, True, False, False, False, True, True] and np.isnan(want[:, 1]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(R.bb_error_units(got[ok], want[ok], (a.astype(np.int64) + b)[ok], 0.02) <= BB_F)          # the cells of the NaN rho column are not among them
    for mc in (0, 1, -3):
        got = bb.betabinom_test(lib, handle, a, b, 0.5, rho, mc)
        assert np.isnan(got[:, 0]).tolist() == [True, True, True, True, False, False, False, False, False, True, False], mc
        assert np.isnan(got[:, 1]).all()


def test_kbbtest_emulated_untested_cells_and_nan_rho(emu):
    _assert_untested_cells(emu.lib, emu.h)


# ------------------------------------------------------------------------------------------------ K_bbfit
@functools.lru_cache(maxsize=None)
def fit_reference():
    """{p0: (a, b, tested cells per column, [(k, n, rho_grid, rho_brent, the better of their scipy LL) per column])}, computed once"""
    out = {}
    for p0, (a, b, sizes) in R.fit_matrices().items():
        cols = []
        for c in range(a.shape[1]):
            k, n = R.tested_cells(a[:, c], b[:, c], R.FIT_MIN_COV)
            assert len(k) == sizes[c]
            if len(k) == 0:
                cols.append((k, n, float("nan"), float("nan"), float("nan")))
                continue
            rg, _, step = R.fit_grid(k, n, p0)
            assert step <= R.last_step(p0) * (1 + 1e-9)          # smaller only where a bracket was clipped at its end
            rb = R.fit_brent(k, n, p0)
            cols.append((k, n, rg, rb, float(max(R.scipy_ll(k, n, p0, [rg, rb])))))
        for arr in (a, b, sizes):
            arr.setflags(write=False)
        out[p0] = (a, b, sizes, cols)
    return out


def _assert_fit(lib, handle, what):
    """-> {p0: (rho, loglik, n_used)}; the three margins printed and asserted"""
    from phaser_amd import ae_betabinom as bb
    res = {}
    m1 = m2 = m3 = 0.0
    for p0, (a, b, sizes, cols) in fit_reference().items():
        rho, ll, used = bb.betabinom_fit(lib, handle, a, b, p0, R.FIT_MIN_COV)
        res[p0] = (rho, ll, used)
        assert np.array_equal(used, sizes), (what, p0, used.tolist())
        for c, (k, n, rg, rb, best) in enumerate(cols):
            if len(k) == 0:
                assert np.isnan(rho[c]) and np.isnan(ll[c]), (what, p0, c)
                continue
            assert R.RHO_MIN <= rho[c] <= R.rho_max(p0), (what, p0, c, rho[c])
            ours = float(R.scipy_ll(k, n, p0, rho[c])[0])
            d1 = best - ours; d2 = abs(ll[c] - ours); d3 = abs(math.log(rho[c]) - math.log(rg)) / R.last_step(p0)
            if d1 > m1 or d2 > m2 or d3 > m3:
                print("%s p0 %.4g column %d (%d cells): rho %.9g grid %.9g brent %.9g, LL %.12g: margin1 %.3g margin2 %.3g margin3 %.3g steps"
                      % (what, p0, c, len(k), rho[c], rg, rb, ours, d1, d2, d3))
            m1, m2, m3 = max(m1, d1), max(m2, d2), max(m3, d3)
            assert d1 <= FIT_M1 and d2 <= FIT_M2 and d3 <= FIT_M3_STEPS, (what, p0, c, d1, d2, d3)
    print("%s: margin1 %.3g (asserted at %.3g), margin2 %.3g (%.3g), margin3 %.3g steps (%.3g)" % (what, m1, FIT_M1, m2, FIT_M2, m3, FIT_M3_STEPS))
    return res


def _bits(res):
    return {p0: tuple(np.ascontiguousarray(x).view(np.uint64).tolist() for x in v[:2]) + (v[2].tolist(),) for p0, v in res.items()}


def test_kbbfit_emulated_quality_and_equal_bits_across_builds_and_runs(emus):
    bits = {tag: _bits(_assert_fit(ctx.lib, ctx.h, "emulated " + tag)) for tag, ctx in emus.items()}
    assert bits["product"] == bits["grid_3"] == bits["wave_32"]
    assert _bits(_assert_fit(emus["product"].lib, emus["product"].h, "emulated product, second run")) == bits["product"]


# ------------------------------------------------------------------------------------------------ argument errors
def _assert_argument_errors(lib, handle):
    from phaser_amd import _lib
    vp = lambda x: C.c_void_p(x.ctypes.data)
    a = np.array([5, 2 ** 31 - 1], dtype=np.int32); b = np.array([5, 1], dtype=np.int32); fine = np.array([5, 5], dtype=np.int32)
    p = np.full(2, -5.0); rho = np.array([0.02, 0.02]); ro = np.full(2, -5.0); lo = np.full(2, -5.0); no = np.full(2, -5, dtype=np.int64)
    fit = lambda rows, cols, p0: lib.phz_betabinom_fit(handle, rows, cols, vp(a), vp(b), p0, 8, vp(ro), vp(lo), vp(no), _lib.PHZ_HOST)
    test = lambda rows, cols, p0, r: lib.phz_betabinom_test(handle, rows, cols, vp(a), vp(b), p0, vp(r), 8, vp(p), _lib.PHZ_HOST)
    for p0 in (0.0, 1.0, -0.25, 1.5, float("nan")):
        assert fit(1, 1, p0) == _lib.PHZ_E_ARG and b"phz_betabinom_fit: p0 must lie strictly between 0 and 1" in lib.phz_last_error(handle), p0
        assert test(1, 1, p0, rho) == _lib.PHZ_E_ARG and b"phz_betabinom_test: p0 must lie strictly between 0 and 1" in lib.phz_last_error(handle), p0
    for rows, cols in ((2, 1), (1, 2)):                                                         # a + b = 2^31
        assert fit(rows, cols, 0.5) == _lib.PHZ_E_ARG and b"phz_betabinom_fit: a + b does not fit in int32" in lib.phz_last_error(handle)
        assert test(rows, cols, 0.5, rho) == _lib.PHZ_E_ARG and b"phz_betabinom_test: a + b does not fit in int32" in lib.phz_last_error(handle)
    for rows, cols in ((2 ** 31, 1), (2 ** 16, 2 ** 15), (1, 2 ** 31)):                         # checked before a cell is read
        assert fit(rows, cols, 0.5) == _lib.PHZ_E_ARG and b"phz_betabinom_fit: more than 2^31 - 1 cells" in lib.phz_last_error(handle)
        assert test(rows, cols, 0.5, rho) == _lib.PHZ_E_ARG and b"phz_betabinom_test: more than 2^31 - 1 cells" in lib.phz_last_error(handle)
    for p0, bad in ((0.5, 0.9e-6), (0.5, 0.3334), (0.5, 0.0), (0.5, -0.1), (0.5, float("inf")), (0.05, 0.048), (0.95, 0.048)):
        assert lib.phz_betabinom_test(handle, 1, 2, vp(fine), vp(fine), p0, vp(np.array([0.02, bad])), 8, vp(p), _lib.PHZ_HOST) == _lib.PHZ_E_ARG, (p0, bad)
        assert b"phz_betabinom_test: rho must lie in" in lib.phz_last_error(handle), (p0, bad)
    assert np.all(p == -5.0) and np.all(ro == -5.0) and np.all(lo == -5.0) and np.all(no == -5)
    # the bounds themselves, and NaN, are arguments like any other
    assert test(1, 1, 0.5, np.array([1e-6])) == _lib.PHZ_OK and test(1, 1, 0.5, np.array([1.0 / 3.0])) == _lib.PHZ_OK and p[0] == 1.0 and p[1] == -5.0
    assert test(1, 1, 0.5, np.array([float("nan")])) == _lib.PHZ_OK and np.isnan(p[0])
    assert fit(1, 1, 0.5) == _lib.PHZ_OK and no[0] == 1 and no[1] == -5 and R.RHO_MIN <= ro[0] <= 1.0 / 3.0


def test_argument_errors_of_both_entry_points(emus):
    _assert_argument_errors(emus["product"].lib, emus["product"].h)


# ------------------------------------------------------------------------------------------------ the tool against the restatement
EIGHT_BY_FOUR = ("#contig\tstart\tstop\tname\tS1\tS2\tS3\tS4\n"
                 "chr1\t100\t200\tG1\t100|20\t30|0\t0|0\t\n"
                 "chr1\t300\t400\tG2\t5|4\t0|25\t\t1|2\n"
                 "chr1\t500\t600\tG3\t40|38\t1|2\t300|200\t\n"
                 "chr2\t10\t20\tG4\t7|0\t500|510\t17|3\t3|3\n"
                 "chr2\t30\t40\tG5\t4|4\t60|15\tbad\t\n"
                 "chr3\t5\t50\tG6\t1000|1200\t9|9\t2|30\t0|0\n"
                 "chr3\t60\t70\tG7\t80|120\t45|44\t21|20\t\n"
                 "chr3\t80\t90\tG8\t250|260\t130|90\t64|70\t2|1\n")
GENE_AE = ("contig\tstart\tstop\tname\taCount\tbCount\ttotalCount\tlog2_aFC\tn_variants\tvariants\tgw_phased\tbam\n" +
           "".join("chr1\t%d\t%d\tG%d\t%d\t%d\t%d\t0\t1\tv\t1\t%s\n" % (i, i + 9, i, a, b, a + b, bam)
                   for i, (a, b, bam) in enumerate([(100, 20, "x.bam"), (5, 4, "x.bam"), (0, 0, "y.bam"), (40, 38, "x.bam"), (30, 2, "y.bam"), (7, 0, "x.bam"),
                                                    (12, 12, "y.bam"), (3, 30, "y.bam"), (1000, 1200, "x.bam"), (2, 2, "y.bam"), (1, 1, "z.bam"),
                                                    (250, 260, "x.bam"), (55, 70, "y.bam"), (90, 60, "y.bam")])))


def seventy_by_five():
    """a seeded 70 x 5 matrix: beta-binomial counts with a rho per sample, empty and low cells strewn in"""
    rng = np.random.default_rng(31)
    lines = ["#contig\tstart\tstop\tname\t" + "\t".join("T%d" % j for j in range(5))]
    for r in range(70):
        cells = []
        for j, rho in enumerate((0.002, 0.01, 0.03, 0.08, 0.2)):
            n = int(round(math.exp(rng.uniform(math.log(4), math.log(3000)))))
            al, be = R.ab(0.5, rho)
            k = int(rng.binomial(n, rng.beta(al, be)))
            cells.append("" if rng.random() < 0.1 else "%d|%d" % (k, n - k))
        lines.append("chr%d\t%d\t%d\tgene%d\t" % (1 + r // 40, 100 * (r % 40), 100 * (r % 40) + 50, r) + "\t".join(cells))
    return "\n".join(lines) + "\n"


def _number_close(got, want, N_max, extra=0.0):
    """a printed %.6g number against the restatement's double: the K_bbtest tolerance at the largest lgamma argument of the input, widened by the 6-digit rounding"""
    if want != want:
        return got == "NA"
    if got == "NA":
        return False
    g = float(got)
    if want < 1e-250:
        return g < 1e-240
    return abs(g - want) <= want * (BB_F * max(R.lgamma_error(N_max), 2.0 ** -46) + 5.1e-6 + extra)


def _rho_close(got, want_grid, null):
    """a printed rho against the restated search: margin 3, widened by the 6-digit rounding"""
    if want_grid != want_grid:
        return got == "NA"
    return got != "NA" and abs(math.log(float(got)) - math.log(want_grid)) <= FIT_M3_STEPS * R.last_step(null) + 5.1e-6


def _assert_matrix_text(raw, want, values, N_max):
    lines = raw.decode().split("\n")
    assert lines[-1] == "" and lines[0] == want["header"] and len(lines) == len(want["leads"]) + 2
    for r, l in enumerate(lines[1:-1]):
        f = l.split("\t")
        assert "\t".join(f[:4]) == want["leads"][r] and len(f) == 4 + len(want["samples"])
        for c, cell in enumerate(f[4:]):
            assert _number_close(cell, values[r, c], N_max), (r, c, cell, values[r, c])


def _sample_rhos(ctx, a, b, null, min_cov, overdispersion):
    """the rho of every sample that the tool works with: a given number, or for "auto" the bits of phz_betabinom_fit on the same arrays (held to the restated
    search here; the restatement then tests at exactly these rho, so that its p-values are held to the tolerance of K_bbtest alone) -> (rho, restated rho)"""
    from phaser_amd import ae_betabinom as bb
    if overdispersion != "auto":
        return np.full(a.shape[1], float(overdispersion)), np.full(a.shape[1], float(overdispersion))
    rho, _, used = bb.betabinom_fit(ctx.lib, ctx.h, a, b, null, min_cov)
    grid = np.array([R.fit_grid(*R.tested_cells(a[:, c], b[:, c], min_cov), null)[0] for c in range(a.shape[1])])
    assert np.array_equal(np.isnan(rho), np.isnan(grid)) and np.array_equal(np.isnan(rho), used == 0)
    ok = ~np.isnan(rho)
    assert np.all(np.abs(np.log(rho[ok]) - np.log(grid[ok])) <= FIT_M3_STEPS * R.last_step(null)), (rho, grid)
    return rho, grid


def _assert_bed_outputs(out, text, null, min_cov, fdr, rho, rho_grid):
    """out: {"pvalue", "qvalue": matrix bytes, "significant", "summary": str} against the restatement: structure and NA cells exactly, numbers parsed back"""
    want = R.restate_bed(text, null, min_cov, fdr, np.where(np.isnan(rho), 0.02, rho))
    N_max = float(np.max(R.largest_argument((want["a"].astype(np.int64) + want["b"]).max(), np.nanmin(rho))))
    assert not np.any((np.abs(want["q"] - fdr) <= 1e-4 * fdr) & (want["q"] != 1.0))          # no cell whose significance hangs on the last digits
    _assert_matrix_text(out["pvalue"], want, want["p"], N_max); _assert_matrix_text(out["qvalue"], want, want["q"], N_max)
    sig = out["significant"].split("\n")
    assert sig[0] == "gene\tsample\taCount\tbCount\tlog2_aFC\tpvalue\tqvalue" and sig[-1] == "" and len(sig) == len(want["significant"]) + 2
    for l, w in zip(sig[1:-1], want["significant"]):
        f = l.split("\t")
        assert f[:5] == [w[0], w[1], str(w[2]), str(w[3]), "%.6g" % w[4]], (l, w)
        assert _number_close(f[5], w[5], N_max) and _number_close(f[6], w[6], N_max), (l, w)
    summ = out["summary"].split("\n")
    assert summ[0] == "sample\ttested\tsignificant\tmin_pvalue\trho" and summ[-1] == "" and len(summ) == len(want["summary"]) + 2
    for c, (l, w) in enumerate(zip(summ[1:-1], want["summary"])):
        f = l.split("\t")
        assert len(f) == 5 and f[:3] == [w[0], str(w[1]), str(w[2])] and _number_close(f[3], w[3], N_max), (l, w)
        assert _rho_close(f[4], rho_grid[c] if w[1] else float("nan"), null), (l, rho_grid[c])
    return want


def _assert_gene_ae_output(body, text, null, min_cov, rho, rho_grid):
    head, lines, p, q, rl = R.restate_gene_ae(text, null, min_cov, np.where(np.isnan(rho), 0.02, rho))
    _, _, a, b, bams, col = R.gene_ae_columns(text)
    N_max = float(np.max(R.largest_argument((a + b).max(), np.nanmin(rho))))
    got = body.split("\n")
    assert got[0] == "\t".join(head + ["pvalue", "qvalue", "rho"]) and got[-1] == "" and len(got) == len(lines) + 2
    for l, w, pv, qv, rv, j in zip(got[1:-1], lines, p, q, rl, col):
        f = l.split("\t")
        assert "\t".join(f[:-3]) == w and _number_close(f[-3], pv, N_max) and _number_close(f[-2], qv, N_max), (l, pv, qv)
        assert _rho_close(f[-1], rho_grid[j] if rv == rv else float("nan"), null), (l, rv)


def _gene_ae_matrix(text):
    """the [rank within its bam, bam] matrices of the table, -1 where no line falls"""
    _, _, a, b, bams, col = R.gene_ae_columns(text)
    rank = np.array([int(np.sum(col[:i] == col[i])) for i in range(len(col))], dtype=np.int64)
    am = np.full((int(rank.max()) + 1, len(bams)), -1, dtype=np.int32); bm = am.copy()
    am[rank, col] = a; bm[rank, col] = b
    return am, bm


@pytest.mark.parametrize("opt", [dict(overdispersion="auto"), dict(overdispersion=0.02), dict(overdispersion="auto", null=0.45, min_cov=0, fdr=0.3)])
def test_ae_test_on_emulated_kernels_matches_restatement(emus, opt):
    from phaser_amd import ae_betabinom as bb
    emu = emus["product"]
    kw = dict(null=0.5, min_cov=8, fdr=0.05); kw.update(opt)
    _, _, a, b = R0.py_parse(EIGHT_BY_FOUR)
    rho, grid = _sample_rhos(emu, a, b, kw["null"], kw["min_cov"], kw["overdispersion"])
    out = bb.ae_test(EIGHT_BY_FOUR, ctx=emu, threads=2, **kw)
    want = _assert_bed_outputs(out, EIGHT_BY_FOUR, kw["null"], kw["min_cov"], kw["fdr"], rho, grid)
    assert [w[1] for w in want["summary"]][3] == (0 if kw["min_cov"] == 8 else 3)             # S4 has no gene at min_cov 8: rho NA
    assert bb.ae_test(EIGHT_BY_FOUR, ctx=emu, threads=1, **kw) == out                    # a second call returns equal bytes
    am, bm = _gene_ae_matrix(GENE_AE)
    rho, grid = _sample_rhos(emu, am, bm, kw["null"], kw["min_cov"], kw["overdispersion"])
    body = bb.ae_test_gene_ae(GENE_AE, kw["null"], kw["min_cov"], kw["fdr"], ctx=emu, overdispersion=kw["overdispersion"])
    _assert_gene_ae_output(body, GENE_AE, kw["null"], kw["min_cov"], rho, grid)
    assert bb.ae_test_gene_ae(GENE_AE, kw["null"], kw["min_cov"], kw["fdr"], ctx=emu, overdispersion=kw["overdispersion"]) == body


def test_overdispersion_zero_is_the_binomial_path(emus):
    from phaser_amd import ae_betabinom as bb, ae_test
    emu = emus["product"]
    for zero in (0, 0.0, "0"):
        assert bb.ae_test(EIGHT_BY_FOUR, ctx=emu, overdispersion=zero) == ae_test.ae_test(EIGHT_BY_FOUR, ctx=emu)
        assert bb.ae_test_gene_ae(GENE_AE, ctx=emu, overdispersion=zero) == ae_test.ae_test_gene_ae(GENE_AE, ctx=emu)
    assert bb.ae_test(EIGHT_BY_FOUR, ctx=emu) == ae_test.ae_test(EIGHT_BY_FOUR, ctx=emu)
    assert bb.ae_test(EIGHT_BY_FOUR, ctx=emu)["summary"].split("\n")[0] == "sample\ttested\tsignificant\tmin_pvalue"
    assert bb.ae_test(EIGHT_BY_FOUR, ctx=emu, overdispersion=0.02)["pvalue"] != ae_test.ae_test(EIGHT_BY_FOUR, ctx=emu)["pvalue"]
    # the command line: without the option, and with 0, phaser_amd.ae_test's own main runs on the same arguments without the option
    calls = []
    real = ae_test.main
    ae_test.main = lambda argv=None: calls.append(list(argv)) or 0
    try:
        assert bb.main(["--bed", "m.bed", "--o", "out", "--t", "2", "--null", "0.3333333333333333"]) == 0
        assert bb.main(["--gene_ae", "t.txt", "--overdispersion", "0", "--o", "out", "--fdr", "1e-3", "--min_cov", "0"]) == 0
        assert bb.main(["--bed", "m.bed", "--o", "out", "--null", "1.5", "--overdispersion", "auto"]) == 0          # --null is that tool's error to report
    finally:
        ae_test.main = real
    assert calls == [["--bed", "m.bed", "--o", "out", "--null", "0.3333333333333333", "--min_cov", "8", "--fdr", "0.05", "--t", "2"],
                     ["--gene_ae", "t.txt", "--o", "out", "--null", "0.5", "--min_cov", "0", "--fdr", "0.001", "--t", "1"],
                     ["--bed", "m.bed", "--o", "out", "--null", "1.5", "--min_cov", "8", "--fdr", "0.05", "--t", "1"]]
    assert all(float(c[5]) == v for c, v in zip(calls, (1.0 / 3.0, 0.5, 1.5)))


@pytest.mark.parametrize("argv,top", [(["--overdispersion", "0.5"], "0.333333"), (["--overdispersion", "1e-7"], "0.333333"), (["--overdispersion", "-0.1"], "0.333333"),
                                      (["--overdispersion", "nan"], "0.333333"), (["--overdispersion", "lots"], "0.333333"),
                                      (["--overdispersion", "0.05", "--null", "0.05"], "0.047619"), (["--overdispersion", "0.2", "--null", "0.8"], "0.166667")])
@pytest.mark.parametrize("mode", ["--bed", "--gene_ae"])
def test_bad_overdispersion_prints_a_line_and_exits_1(tmp_path, capsys, argv, top, mode):
    from phaser_amd import ae_betabinom as bb
    src = os.path.join(str(tmp_path), "in.txt")
    open(src, "w").write(EIGHT_BY_FOUR if mode == "--bed" else GENE_AE)
    assert bb.main([mode, src, "--o", os.path.join(str(tmp_path), "out")] + argv) == 1
    lines = [l for l in capsys.readouterr().out.split("\n") if l.startswith("FATAL ERROR - ")]
    assert len(lines) == 1 and lines[0].startswith("FATAL ERROR - --overdispersion must be 0, auto or a number in [1e-06, %s]" % top), lines
    assert sorted(os.listdir(str(tmp_path))) == ["in.txt"]


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_kbbtest_gpu_matches_scipy(gpu_ctx):
    from phaser_amd import _lib
    gpu_ctx.reset_timing()
    _assert_bb_matches_scipy(gpu_ctx.lib, gpu_ctx.h, "gpu")
    assert gpu_ctx.timing(_lib.PHZ_T_BBTEST)[2] > 0 and gpu_ctx.timing(_lib.PHZ_T_BBTEST)[0] > 0


@pytest.mark.gpu
def test_kbbtest_gpu_untested_cells_and_nan_rho(gpu_ctx):
    _assert_untested_cells(gpu_ctx.lib, gpu_ctx.h)


@pytest.mark.gpu
def test_kbbfit_gpu_quality_and_equal_bits_across_spaces_and_runs(gpu_ctx):
    import torch
    from phaser_amd import _lib
    gpu_ctx.reset_timing()
    first = _assert_fit(gpu_ctx.lib, gpu_ctx.h, "gpu")
    assert gpu_ctx.timing(_lib.PHZ_T_BBFIT)[2] > 0 and gpu_ctx.timing(_lib.PHZ_T_BBFIT)[0] > 0
    assert _bits(_assert_fit(gpu_ctx.lib, gpu_ctx.h, "gpu, second run")) == _bits(first)
    dev = torch.device("cuda", gpu_ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    for p0, (a, b, sizes, cols) in fit_reference().items():
        ta = torch.from_numpy(np.array(a)).to(dev); tb = torch.from_numpy(np.array(b)).to(dev)
        tr = torch.full((a.shape[1],), -5.0, dtype=torch.float64, device=dev); tl = tr.clone(); tn = torch.full((a.shape[1],), -5, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        gpu_ctx.check(gpu_ctx.lib.phz_betabinom_fit(gpu_ctx.h, a.shape[0], a.shape[1], p(ta), p(tb), p0, R.FIT_MIN_COV, p(tr), p(tl), p(tn), _lib.PHZ_DEVICE))
        rho, ll, used = first[p0]
        assert np.array_equal(tr.cpu().numpy().view(np.uint64), rho.view(np.uint64)) and np.array_equal(tl.cpu().numpy().view(np.uint64), ll.view(np.uint64))
        assert np.array_equal(tn.cpu().numpy(), used)


@pytest.mark.gpu
def test_kbbtest_gpu_device_space_gives_the_bits_of_host_space(gpu_ctx):
    import torch
    from phaser_amd import _lib, ae_betabinom as bb
    dev = torch.device("cuda", gpu_ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    for p0, (a, b, rho, ref, tie) in bb_reference().items():
        host = bb.betabinom_test(gpu_ctx.lib, gpu_ctx.h, a, b, p0, rho, 0)
        ta = torch.from_numpy(np.array(a)).to(dev); tb = torch.from_numpy(np.array(b)).to(dev); tr = torch.from_numpy(np.array(rho)).to(dev)
        tp = torch.full(a.shape, -5.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        gpu_ctx.check(gpu_ctx.lib.phz_betabinom_test(gpu_ctx.h, a.shape[0], a.shape[1], p(ta), p(tb), p0, p(tr), 0, p(tp), _lib.PHZ_DEVICE))
        assert np.array_equal(tp.cpu().numpy().view(np.uint64), host.view(np.uint64)), p0


@pytest.mark.gpu
def test_gpu_argument_errors_of_both_entry_points(gpu_ctx):
    _assert_argument_errors(gpu_ctx.lib, gpu_ctx.h)


def _read_outputs(prefix):
    out = {k: gzip.open("%s.%s.bed.gz" % (prefix, k), "rb").read() for k in ("pvalue", "qvalue")}
    out["significant"] = open(prefix + ".significant.txt").read(); out["summary"] = open(prefix + ".summary.txt").read()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form,which", [("bgzf", "8x4"), ("plain", "70x5")])
def test_cli_gpu_bed_mode_matches_restatement(tmp_path, gpu_ctx, form, which, capsys):
    from phaser_amd import ae_betabinom as bb, vcfout
    tmp = str(tmp_path)
    text = EIGHT_BY_FOUR if which == "8x4" else seventy_by_five()
    if form == "bgzf":
        src = os.path.join(tmp, "m.bed.gz")
        vcfout.write_bgzf(src, text, 2)
    else:
        src = os.path.join(tmp, "m.bed")
        open(src, "w").write(text)
    runs = []
    for k in (0, 1):
        prefix = os.path.join(tmp, "run%d" % k, "out")
        os.makedirs(os.path.dirname(prefix))
        assert bb.main(["--bed", src, "--o", prefix, "--t", str(1 + k), "--overdispersion", "auto"]) == 0
        names = sorted(os.listdir(os.path.dirname(prefix)))
        assert names == ["out.pvalue.bed.gz", "out.pvalue.bed.gz.tbi", "out.qvalue.bed.gz", "out.qvalue.bed.gz.tbi", "out.significant.txt", "out.summary.txt"]
        runs.append({n: open(os.path.join(os.path.dirname(prefix), n), "rb").read() for n in names})
    assert runs[0] == runs[1]                                 # a second run (with another --t) writes identical files
    assert "K_bbfit" in capsys.readouterr().out
    _, _, a, b = R0.py_parse(text)
    rho, grid = _sample_rhos(gpu_ctx, a, b, 0.5, 8, "auto")
    _assert_bed_outputs(_read_outputs(os.path.join(tmp, "run0", "out")), text, 0.5, 8, 0.05, rho, grid)


@pytest.mark.gpu
def test_cli_gpu_gene_ae_mode_matches_restatement(tmp_path, gpu_ctx):
    from phaser_amd import ae_betabinom as bb
    src = os.path.join(str(tmp_path), "s.gene_ae.txt")
    open(src, "w").write(GENE_AE)
    bodies = []
    for k in (0, 1):
        prefix = os.path.join(str(tmp_path), "out%d" % k)
        assert bb.main(["--gene_ae", src, "--o", prefix, "--min_cov", "4", "--overdispersion", "auto"]) == 0
        bodies.append(open(prefix + ".txt").read())
    assert bodies[0] == bodies[1]
    am, bm = _gene_ae_matrix(GENE_AE)
    rho, grid = _sample_rhos(gpu_ctx, am, bm, 0.5, 4, "auto")
    _assert_gene_ae_output(bodies[0], GENE_AE, 0.5, 4, rho, grid)
