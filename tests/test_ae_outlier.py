"""phaser_ae_outlier (phaser_amd/ae_outlier.py; K_blnfit and K_blntest in phaser_amd/csrc/phz_aebln.hip).

CPU tests: both kernels under the host emulation in two builds -- the product macros and PHZ_AETEST_GRID=3 (workgroups are reused) -- K_blntest against the
piecewise scipy.integrate.quad restatement (ae_outlier_restatement.py) on one fixed case list, K_blnfit against the restated search and a bounded Brent, judged
in the restated likelihood; equal bits across builds and runs; the argument errors; the tool on the emulated kernels against the restatement.  GPU tests: the
same lists on the product kernels, PHZ_DEVICE against PHZ_HOST, the timing slots, the CLI."""
import ctypes as C
import functools
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

import ae_outlier_restatement as R
import ae_test_restatement as R0

HIPEMU = os.path.join(REPO, "tests", "hipemu")
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
EMU_DIR = os.path.join(HIPEMU, "_build", "aebln")
BUILDS = {"product": [], "grid_3": ["-DPHZ_AETEST_GRID=3"]}

# The largest error of K_blntest over the fixed list (3,080 cells), in units of T(n, s) = E(n) + 2^-36 max(s, 1)^11 (ae_outlier_restatement.tolerance), measured
# against the quad restatement (PHZ_BLN_Q 32, PHZ_BLN_SUM_N 64):
F_EMULATED = 0.891    # the emulated kernels (the host's libm), both builds alike: at k 0, n 47, p0 1/3, s 2 (p0 0.5: 0.492 at k 50000, n 200000, s 1)
F_GPU = 0.891         # the product kernels on an MI355X (the device library's lgamma, exp, log1p and erfc): at the same case (p0 0.5: 0.490 at k 99313, n 200000, s 1)
BLN_F = 4 * max(F_EMULATED, F_GPU)          # math libraries differ by an ulp or so between versions
# The one condition that %.6g sets: the worst relative error over the list is at most half a unit of the sixth printed digit.  Measured: 2.66e-8, emulated and
# on the MI355X alike, at k 0, n 47, p0 1/3, s 2: the sum tier at the top of the domain, where the 32-node rule is weakest (p0 0.5: 1.2e-8 at k 0, n 50, s 2).
WORST_RELATIVE = 5e-7

# K_blnfit over ae_outlier_restatement.fit_matrices, measured (emulated, MI355X):
#   margin 1   max(LL(s_brent), LL(s_grid_restated)) - LL(s_ours), LL the restated likelihood
#   margin 2   |loglik_ours - LL(s_ours)|, and |loglik_min_ours - LL(S_MIN)|
#   margin 3   |ln s_ours - ln s_grid_restated|, in steps of the last round of the search (3.86e-6 in ln s); never asserted below one step
# Margin 1 is largest at p0 1/3 in the row of 1,025 cells at true s 1.5 (|LL| about 5,200); margin 2 in loglik_min of the row of 1,025 cells of binomial counts
# at p0 0.5 (|LL| about 3,500); margin 3 is one step in that same row, where two neighbouring candidates differ by less than the restated likelihood's own
# error, and below 1e-9 of a step everywhere else.
M1_EMULATED, M1_GPU = 1.65e-9, 1.65e-9
M2_EMULATED, M2_GPU = 1.27e-9, 1.27e-9
M3_EMULATED, M3_GPU = 1.0, 1.0
FIT_M1 = 4 * max(M1_EMULATED, M1_GPU)
FIT_M2 = 4 * max(M2_EMULATED, M2_GPU)
FIT_M3_STEPS = max(4 * max(M3_EMULATED, M3_GPU), 1.0)


# ------------------------------------------------------------------------------------------------ the kernels under the emulation
def _emu_lib(tag):
    from phaser_amd import _lib
    os.makedirs(EMU_DIR, exist_ok=True)
    lib = os.path.join(EMU_DIR, "libphz_aebln_%s.so" % tag)
    srcs = [os.path.join(CSRC, "phz_api.hip"), os.path.join(CSRC, "phz_aetest.hip"), os.path.join(CSRC, "phz_aebln.hip"), os.path.join(HIPEMU, "hipemu.cpp")]
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
    for name in ("phz_ctx_create", "phz_ctx_destroy", "phz_last_error", "phz_strerror", "phz_bh_adjust", "phz_bln_fit", "phz_bln_test"):
        res, args = _lib.SYMBOLS[name]
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


class EmuCtx:
    """what ae_outlier needs of a _lib.Context, on an emulated library"""

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


# ------------------------------------------------------------------------------------------------ the restatement itself
@functools.lru_cache(maxsize=None)
def bln_reference():
    """{p0: (a, b [5, columns], s [5], restated p-values, quad's relative error estimates)} of the fixed list (every column under every s), computed once"""
    out = {}
    for p0, (a, b) in R.bln_cases().items():
        s = np.array(R.S_VALUES)
        a2 = np.ascontiguousarray(np.repeat(a[None, :], len(s), axis=0)); b2 = np.ascontiguousarray(np.repeat(b[None, :], len(s), axis=0))
        ref, err = R.quad_bln(a2, b2, p0, s, 0)
        for arr in (a2, b2, s, ref, err):
            arr.setflags(write=False)
        out[p0] = (a2, b2, s, ref, err)
    return out


def test_case_list_covers_the_edges_and_leaves_few_cases_out():
    ref = bln_reference()
    total = sum(v[0].size for v in ref.values()); out = sum(int((v[4] > 1e-10).sum()) for v in ref.values())
    print("cases %d, left out for quad's own error estimate %d" % (total, out))
    assert out <= 0.01 * total, (out, total)
    for p0, (a, b, s, p, err) in ref.items():
        n = a.astype(np.int64) + b
        assert a.shape[1] > 257 and np.isfinite(p).all() and np.all(p >= 0) and np.all(p <= 1)
        assert np.any(p < 1e-250)                                                              # a tail that underflows
        assert np.any((a == 0) & (n == 200000)) and np.any((b == 0) & (n == 200000)) and np.any(n == 1)
        for big in R.BIG_N:
            assert np.any(n == big)
        assert np.all(n[:, -1] == 200000) and np.all(n[:, :257] < 200000)                      # the slow columns come last, beyond the prefixes


def test_restated_tails_of_small_n_are_the_sums_of_the_restated_pmf():
    worst = 0.0
    for p0 in R.P0S:
        for s in R.S_VALUES:
            for n in range(1, 13):
                pmf = np.array([R.pmf_quad(k, n, p0, s)[0] for k in range(n + 1)])
                assert abs(pmf.sum() - 1.0) < 1e-12
                for k in range(n + 1):
                    lo, up, _, _ = R.tails_quad(k, n, p0, s)
                    for got, want in ((lo, pmf[:k + 1].sum()), (up, pmf[k:].sum())):
                        worst = max(worst, abs(got - want) / want)
    print("tails by quad against sums of the quad pmf, n <= 12: largest relative difference %.3g" % worst)
    assert worst < 1e-11


def test_fast_binom_cdf_is_binom_cdf_on_arguments_of_the_list():
    """the restatement integrates scipy.stats.binom.cdf through the ufunc it wraps (100 us a call otherwise): equal bits on the list's arguments"""
    from scipy import special, stats
    for p0, (a, b) in R.bln_cases().items():
        n = a.astype(np.int64) + b
        pick = (b > 0)
        k = a[pick].astype(np.float64); nn = n[pick].astype(np.float64)
        for d in (-8.0, -3.0, -1.0, 0.0, 1.0, 3.0, 8.0):
            pm = (k + 1) / (nn + 1)
            p = special.expit(np.log(pm / (1 - pm)) + d / np.sqrt((nn + 1) * pm * (1 - pm)))
            assert np.array_equal(stats.binom.cdf(a[pick], n[pick], p), R.binom_cdf(k, nn, p))


def test_restated_likelihood_of_the_fit_is_the_quad_pmf():
    """the Gauss-Legendre panels that restate the fit's likelihood against the quad pmf, every third case of the list under every s"""
    worst = 0.0
    for p0, (a, b) in R.bln_cases().items():
        n = a.astype(np.int64) + b
        pan = R.log_pmf_panels(a, n, p0, R.S_VALUES)
        for i, s in enumerate(R.S_VALUES):
            for j in range(0, len(a), 3):
                lq, e = R.log_pmf_quad(int(a[j]), int(n[j]), p0, s)
                assert e < 1e-10
                worst = max(worst, abs(pan[i, j] - lq) / max(1.0, float(R.lgamma_error(n[j])) * 2 ** 36))
    print("panels against quad, log pmf: largest difference %.3g in units of max(1, E(n) 2^36)" % worst)
    assert worst < 2e-11


# ------------------------------------------------------------------------------------------------ K_blntest
def _assert_bln_matches_restatement(lib, handle, what):
    """every p0 of the fixed list, whole and in prefixes of 1, 63, 65, 257 cells; -> (the largest error in units of T(n, s), the largest relative error)"""
    from phaser_amd import ae_outlier as ao
    worst = worst_rel = 0.0
    for p0, (a, b, s, ref, err) in bln_reference().items():
        got = ao.bln_test(lib, handle, a, b, p0, s, 0)
        for count in (1, 63, 65, 257):
            for r in range(len(s)):
                part = ao.bln_test(lib, handle, a[r:r + 1, :count], b[r:r + 1, :count], p0, s[r:r + 1], 0)
                assert np.array_equal(part[0].view(np.uint64), np.ascontiguousarray(got[r, :count]).view(np.uint64)), (what, p0, count, r)
        assert not np.isnan(got).any() and np.all(got >= 0) and np.all(got <= 1), (what, p0)
        n = a.astype(np.int64) + b
        units = R.error_units(got, ref, n, s[:, None]); rel = R.relative_error(got, ref)
        units[err > 1e-10] = 0.0; rel[err > 1e-10] = 0.0
        r, c = np.unravel_index(int(np.argmax(units)), units.shape)
        print("%s p0 %.4g: F = %.3f at k %d n %d s %g (ours %.17g restated %.17g)" % (what, p0, units[r, c], a[r, c], n[r, c], s[r], got[r, c], ref[r, c]))
        r2, c2 = np.unravel_index(int(np.argmax(rel)), rel.shape)
        print("%s p0 %.4g: largest relative error %.3g at k %d n %d s %g" % (what, p0, rel[r2, c2], a[r2, c2], n[r2, c2], s[r2]))
        worst = max(worst, float(units[r, c])); worst_rel = max(worst_rel, float(rel[r2, c2]))
        assert units[r, c] <= BLN_F, (what, p0, int(a[r, c]), int(n[r, c]), float(s[r]), got[r, c], ref[r, c], float(units[r, c]))
        assert rel[r2, c2] <= WORST_RELATIVE, (what, p0, int(a[r2, c2]), int(n[r2, c2]), float(s[r2]), float(rel[r2, c2]))
    print("%s: largest F over the list %.3f (asserted at %.3f), largest relative error %.3g (asserted at %.3g)" % (what, worst, BLN_F, worst_rel, WORST_RELATIVE))
    return worst, worst_rel


def test_kblntest_emulated_matches_restatement(emu):
    _assert_bln_matches_restatement(emu.lib, emu.h, "emulated")


def test_kblntest_emulated_builds_give_equal_bits(emus):
    from phaser_amd import ae_outlier as ao
    for p0, (a, b, s, ref, err) in bln_reference().items():
        got = [ao.bln_test(ctx.lib, ctx.h, a, b, p0, s, 0) for ctx in emus.values()]
        assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64)), p0


UNTESTED_A = np.array([-1, 3, -1, 0, 3, 7, 4, 8, 0, 2 ** 31 - 1, 5], dtype=np.int32)
UNTESTED_B = np.array([5, -1, -1, 0, 4, 0, 4, 0, 8, -1, 1], dtype=np.int32)


def _assert_untested_cells(lib, handle):
    """min_cov 8: a negative count, n = 0 and n < 8 give NaN, n = 8 is tested; min_cov 0 and -3 test from n = 1; a NaN s leaves its row NaN"""
    from phaser_amd import ae_outlier as ao
    a = np.stack([UNTESTED_A, UNTESTED_A]); b = np.stack([UNTESTED_B, UNTESTED_B])
    s = np.array([0.3, float("nan")])
    got = ao.bln_test(lib, handle, a, b, 0.5, s, 8)
    want, _ = R.quad_bln(a, b, 0.5, s, 8)
    assert np.isnan(want[0]).tolist() == [True, True, True, True, True, True, False, False, False, True, True] and np.isnan(want[1]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(R.error_units(got[ok], want[ok], (a.astype(np.int64) + b)[ok], 0.3) <= BLN_F)
    for mc in (0, 1, -3):
        got = ao.bln_test(lib, handle, a, b, 0.5, s, mc)
        assert np.isnan(got[0]).tolist() == [True, True, True, True, False, False, False, False, False, True, False], mc
        assert np.isnan(got[1]).all()


def test_kblntest_emulated_untested_cells_and_nan_s(emu):
    _assert_untested_cells(emu.lib, emu.h)


# ------------------------------------------------------------------------------------------------ K_blnfit
@functools.lru_cache(maxsize=None)
def fit_reference():
    """{p0: (a, b, tested cells per row, [(k, n, s_grid, s_brent, the better of their restated LL, restated LL(S_MIN)) per row])}, computed once"""
    out = {}
    for p0, (a, b, sizes) in R.fit_matrices().items():
        rows = []
        for r in range(a.shape[0]):
            k, n = R.tested_cells(a[r], b[r], R.FIT_MIN_COV)
            assert len(k) == sizes[r]
            if len(k) < R.FIT_MIN_SAMPLES:
                rows.append((k, n, float("nan"), float("nan"), float("nan"), float("nan")))
                continue
            sg, _, ll_min, step = R.fit_grid(k, n, p0)
            assert step <= R.last_step() * (1 + 1e-9)          # smaller only where a bracket was clipped at its end
            sb = R.fit_brent(k, n, p0)
            rows.append((k, n, sg, sb, float(max(R.restated_ll(k, n, p0, [sg, sb]))), ll_min))
        for arr in (a, b, sizes):
            arr.setflags(write=False)
        out[p0] = (a, b, sizes, rows)
    return out


def test_fit_matrices_hold_the_designed_rows():
    for p0, (a, b, sizes) in R.fit_matrices().items():
        assert a.shape == (28, 1100) and sorted(set(sizes.tolist())) == [0, 1, R.FIT_MIN_SAMPLES - 1, R.FIT_MIN_SAMPLES, 64, 65, 1025]
        assert np.any(a == -1) and np.any((a >= 0) & (a.astype(np.int64) + b < R.FIT_MIN_COV))


def _assert_fit(lib, handle, what):
    """-> {p0: (s, loglik, loglik_min, n_used)}; the three margins printed and asserted"""
    from phaser_amd import ae_outlier as ao
    res = {}
    m1 = m2 = m3 = 0.0
    for p0, (a, b, sizes, rows) in fit_reference().items():
        s, ll, ll_min, used = ao.bln_fit(lib, handle, a, b, p0, R.FIT_MIN_COV, R.FIT_MIN_SAMPLES)
        res[p0] = (s, ll, ll_min, used)
        assert np.array_equal(used, sizes), (what, p0, used.tolist())
        for r, (k, n, sg, sb, best, want_min) in enumerate(rows):
            if len(k) < R.FIT_MIN_SAMPLES:
                assert np.isnan(s[r]) and np.isnan(ll[r]) and np.isnan(ll_min[r]), (what, p0, r)
                continue
            assert R.S_MIN <= s[r] <= R.S_MAX, (what, p0, r, s[r])
            ours = float(R.restated_ll(k, n, p0, s[r])[0])
            d1 = best - ours; d2 = max(abs(ll[r] - ours), abs(ll_min[r] - want_min)); d3 = abs(math.log(s[r]) - math.log(sg)) / R.last_step()
            if d1 > m1 or d2 > m2 or d3 > m3:
                print("%s p0 %.4g row %d (%d cells): s %.9g grid %.9g brent %.9g, LL %.12g: margin1 %.3g margin2 %.3g margin3 %.3g steps"
                      % (what, p0, r, len(k), s[r], sg, sb, ours, d1, d2, d3))
            m1, m2, m3 = max(m1, d1), max(m2, d2), max(m3, d3)
            assert d1 <= FIT_M1 and d2 <= FIT_M2 and d3 <= FIT_M3_STEPS, (what, p0, r, d1, d2, d3)
    print("%s: margin1 %.3g (asserted at %.3g), margin2 %.3g (%.3g), margin3 %.3g steps (%.3g)" % (what, m1, FIT_M1, m2, FIT_M2, m3, FIT_M3_STEPS))
    return res


def _bits(res):
    return {p0: tuple(np.ascontiguousarray(x).view(np.uint64).tolist() for x in v[:3]) + (v[3].tolist(),) for p0, v in res.items()}


def test_kblnfit_emulated_quality_and_equal_bits_across_builds_and_runs(emus):
    bits = {tag: _bits(_assert_fit(ctx.lib, ctx.h, "emulated " + tag)) for tag, ctx in emus.items()}
    assert bits["product"] == bits["grid_3"]
    assert _bits(_assert_fit(emus["product"].lib, emus["product"].h, "emulated product, second run")) == bits["product"]


# ------------------------------------------------------------------------------------------------ argument errors
def _assert_argument_errors(lib, handle):
    from phaser_amd import _lib
    vp = lambda x: C.c_void_p(x.ctypes.data)
    a = np.array([5, 2 ** 31 - 1], dtype=np.int32); b = np.array([5, 1], dtype=np.int32); fine = np.array([5, 5], dtype=np.int32)
    p = np.full(2, -5.0); s = np.array([0.3, 0.3]); so = np.full(2, -5.0); lo = np.full(2, -5.0); mo = np.full(2, -5.0); no = np.full(2, -5, dtype=np.int64)
    fit = lambda rows, cols, p0, ms=1: lib.phz_bln_fit(handle, rows, cols, vp(a), vp(b), p0, 8, ms, vp(so), vp(lo), vp(mo), vp(no), _lib.PHZ_HOST)
    test = lambda rows, cols, p0, sv: lib.phz_bln_test(handle, rows, cols, vp(a), vp(b), p0, vp(sv), 8, vp(p), _lib.PHZ_HOST)
    for p0 in (0.0, 1.0, -0.25, 1.5, float("nan")):
        assert fit(1, 1, p0) == _lib.PHZ_E_ARG and b"phz_bln_fit: p0 must lie strictly between 0 and 1" in lib.phz_last_error(handle), p0
        assert test(1, 1, p0, s) == _lib.PHZ_E_ARG and b"phz_bln_test: p0 must lie strictly between 0 and 1" in lib.phz_last_error(handle), p0
    for rows, cols in ((2, 1), (1, 2)):                                                         # a + b = 2^31
        assert fit(rows, cols, 0.5) == _lib.PHZ_E_ARG and b"phz_bln_fit: a + b does not fit in int32" in lib.phz_last_error(handle)
        assert test(rows, cols, 0.5, s) == _lib.PHZ_E_ARG and b"phz_bln_test: a + b does not fit in int32" in lib.phz_last_error(handle)
    for rows, cols in ((2 ** 31, 1), (2 ** 16, 2 ** 15), (1, 2 ** 31)):                         # checked before a cell is read
        assert fit(rows, cols, 0.5) == _lib.PHZ_E_ARG and b"phz_bln_fit: more than 2^31 - 1 cells" in lib.phz_last_error(handle)
        assert test(rows, cols, 0.5, s) == _lib.PHZ_E_ARG and b"phz_bln_test: more than 2^31 - 1 cells" in lib.phz_last_error(handle)
    for ms in (0, -1):
        assert fit(1, 1, 0.5, ms) == _lib.PHZ_E_ARG and b"phz_bln_fit: min_samples must be at least 1" in lib.phz_last_error(handle), ms
    for bad in (0.9e-3, 2.0001, 0.0, -0.1, float("inf")):
        assert lib.phz_bln_test(handle, 2, 1, vp(fine), vp(fine), 0.5, vp(np.array([0.3, bad])), 8, vp(p), _lib.PHZ_HOST) == _lib.PHZ_E_ARG, bad
        assert b"phz_bln_test: s must lie in [1e-3, 2]" in lib.phz_last_error(handle), bad
    assert np.all(p == -5.0) and np.all(so == -5.0) and np.all(lo == -5.0) and np.all(mo == -5.0) and np.all(no == -5)
    # the bounds themselves, and NaN, are arguments like any other
    assert test(1, 1, 0.5, np.array([1e-3])) == _lib.PHZ_OK and test(1, 1, 0.5, np.array([2.0])) == _lib.PHZ_OK and p[0] == 1.0 and p[1] == -5.0
    assert test(1, 1, 0.5, np.array([float("nan")])) == _lib.PHZ_OK and np.isnan(p[0])
    assert fit(1, 1, 0.5) == _lib.PHZ_OK and no[0] == 1 and no[1] == -5 and R.S_MIN <= so[0] <= R.S_MAX and so[1] == -5.0
    assert fit(1, 1, 0.5, 2) == _lib.PHZ_OK and no[0] == 1 and np.isnan(so[0]) and np.isnan(lo[0]) and np.isnan(mo[0])


def test_argument_errors_of_both_entry_points(emus):
    _assert_argument_errors(emus["product"].lib, emus["product"].h)


# ------------------------------------------------------------------------------------------------ the tool against the restatement
TOOL_MIN_SAMPLES = 10


def population_matrix(sort=True):
    """a seeded 14 genes x 16 samples matrix: counts from the model at a per-gene s, a few planted outliers, empty and low cells strewn in; gene 3 keeps
    fewer than TOOL_MIN_SAMPLES tested cells, gene 7 none.  sort=False: the rows in an order that is not position-sorted"""
    rng = np.random.default_rng(47)
    lines = []
    for r in range(14):
        s = (0.02, 0.1, 0.3, 0.6, 1.0)[r % 5]
        cells = []
        for j in range(16):
            n = int(round(math.exp(rng.uniform(math.log(10), math.log(2000)))))
            k = int(rng.binomial(n, 1.0 / (1.0 + math.exp(-rng.normal(0.0, s)))))
            if (r, j) in ((0, 2), (5, 11), (9, 0)):
                k = n // 25
            empty = rng.random() < 0.08 or (r == 3 and j >= 6) or r == 7
            low = rng.random() < 0.05
            cells.append("" if empty else ("%d|%d" % (k % 4, 3) if low else "%d|%d" % (k, n - k)))
        lines.append("chr%d\t%d\t%d\tgene%d\t" % (1 + r // 8, 100 * (r % 8), 100 * (r % 8) + 50, r) + "\t".join(cells))
    if not sort:
        lines = lines[5:] + lines[:5]
    return "#contig\tstart\tstop\tname\t" + "\t".join("P%d" % j for j in range(16)) + "\n" + "\n".join(lines) + "\n"


def _number_close(got, want, T_max):
    """a printed %.6g number against the restatement's double: the K_blntest tolerance at the largest T(n, s) of the input, widened by the 6-digit rounding"""
    if want != want:
        return got == "NA"
    if got == "NA":
        return False
    g = float(got)
    if want < 1e-250:
        return g < 1e-240
    return abs(g - want) <= want * (BLN_F * T_max + 5.1e-6)


def _sigma_close(got, want_grid):
    """a printed sigma against the restated search: margin 3, widened by the 6-digit rounding"""
    if want_grid != want_grid:
        return got == "NA"
    return got != "NA" and abs(math.log(float(got)) - math.log(want_grid)) <= FIT_M3_STEPS * R.last_step() + 5.1e-6


def _loglik_close(got, want):
    """a printed log likelihood against the restated one at the same s: margin 2, widened by the 6-digit rounding"""
    if want != want:
        return got == "NA"
    return got != "NA" and abs(float(got) - want) <= FIT_M2 + 5.1e-6 * abs(want)


def _assert_matrix_text(raw, want, values, T_max):
    lines = raw.decode().split("\n")
    assert lines[-1] == "" and lines[0] == want["header"] and len(lines) == len(want["leads"]) + 2
    for r, l in enumerate(lines[1:-1]):
        f = l.split("\t")
        assert "\t".join(f[:4]) == want["leads"][r] and len(f) == 4 + len(want["samples"])
        for c, cell in enumerate(f[4:]):
            assert _number_close(cell, values[r, c], T_max), (r, c, cell, values[r, c])


def _gene_sigmas(ctx, a, b, null, min_cov, min_samples, sigma):
    """the s of every gene that the tool works with: a given number, or for "auto" the bits of phz_bln_fit on the same arrays (held to the restated search
    here; the restatement then tests at exactly these s, so that its p-values are held to the tolerance of K_blntest alone) -> (s, restated s)"""
    from phaser_amd import ae_outlier as ao
    if sigma != "auto":
        return np.full(a.shape[0], float(sigma)), np.full(a.shape[0], float(sigma))
    s, _, _, used = ao.bln_fit(ctx.lib, ctx.h, a, b, null, min_cov, min_samples)
    grid = np.array([R.fit_grid(*R.tested_cells(a[r], b[r], min_cov), null)[0] if used[r] >= min_samples else float("nan") for r in range(a.shape[0])])
    assert np.array_equal(np.isnan(s), np.isnan(grid)) and np.array_equal(np.isnan(s), used < min_samples)
    ok = ~np.isnan(s)
    assert np.all(np.abs(np.log(s[ok]) - np.log(grid[ok])) <= FIT_M3_STEPS * R.last_step()), (s, grid)
    return s, grid


def _assert_outputs(out, text, null, min_cov, min_samples, fdr, sigma, s, s_grid):
    """out: {"gene_var", "outliers", "summary": str, "pvalue", "qvalue": matrix bytes} against the restatement: structure and NA cells exactly, numbers parsed back"""
    want = R.restate_bed(text, null, min_cov, min_samples if sigma == "auto" else 0, fdr, s)
    n = want["a"].astype(np.int64) + want["b"]
    T_max = float(np.max(R.tolerance(n.max(), np.nanmax(s))))
    assert not np.any((np.abs(want["q"] - fdr) <= 1e-4 * fdr) & (want["q"] != 1.0))          # no cell whose significance hangs on the last digits
    _assert_matrix_text(out["pvalue"], want, want["p"], T_max); _assert_matrix_text(out["qvalue"], want, want["q"], T_max)
    gv = out["gene_var"].split("\n")
    assert gv[0] == "#contig\tstart\tstop\tname\tn_used\tsigma\tloglik\tloglik_min" and gv[-1] == "" and len(gv) == len(want["leads"]) + 2
    for r, l in enumerate(gv[1:-1]):
        f = l.split("\t")
        assert "\t".join(f[:4]) == want["leads"][r] and len(f) == 8 and f[4] == str(want["n_used"][r]), l
        if sigma == "auto":
            assert _sigma_close(f[5], s_grid[r]) and _loglik_close(f[6], want["loglik"][r]) and _loglik_close(f[7], want["loglik_min"][r]), (l, s_grid[r], want["loglik"][r])
        else:
            assert f[5:] == ["%.6g" % float(sigma), "NA", "NA"], l
    rows = out["outliers"].split("\n")
    assert rows[0] == "gene\tsample\taCount\tbCount\tsigma\tpvalue\tqvalue" and rows[-1] == "" and len(rows) == len(want["outliers"]) + 2
    for l, w in zip(rows[1:-1], want["outliers"]):
        f = l.split("\t")
        assert f[:5] == [w[0], w[1], str(w[2]), str(w[3]), "%.6g" % w[4]], (l, w)
        assert _number_close(f[5], w[5], T_max) and _number_close(f[6], w[6], T_max), (l, w)
    summ = out["summary"].split("\n")
    assert summ[0] == "sample\ttested\tsignificant\tmin_pvalue" and summ[-1] == "" and len(summ) == len(want["summary"]) + 2
    for l, w in zip(summ[1:-1], want["summary"]):
        f = l.split("\t")
        assert len(f) == 4 and f[:3] == [w[0], str(w[1]), str(w[2])] and _number_close(f[3], w[3], T_max), (l, w)
    return want


@pytest.mark.parametrize("opt", [dict(sigma="auto"), dict(sigma=0.3), dict(sigma="auto", null=0.45, min_cov=0, min_samples=12, fdr=0.3)])
def test_ae_outlier_on_emulated_kernels_matches_restatement(emus, opt):
    from phaser_amd import ae_outlier as ao
    emu = emus["product"]
    kw = dict(null=0.5, min_cov=8, min_samples=TOOL_MIN_SAMPLES, fdr=0.05); kw.update(opt)
    text = population_matrix()
    _, _, a, b = R0.py_parse(text)
    s, grid = _gene_sigmas(emu, a, b, kw["null"], kw["min_cov"], kw["min_samples"], kw["sigma"])
    out = ao.ae_outlier(text, ctx=emu, threads=2, **kw)
    want = _assert_outputs(out, text, kw["null"], kw["min_cov"], kw["min_samples"], kw["fdr"], kw["sigma"], s, grid)
    assert want["n_used"][7] == 0 and 0 < want["n_used"][3] < kw["min_samples"] and len(want["outliers"]) >= 2
    if kw["sigma"] == "auto":
        assert np.isnan(want["p"][3]).all() and np.isnan(s[3]) and np.isnan(s[7])             # a gene that is not fitted is not tested
    else:
        assert not np.isnan(want["p"][3]).all()                                               # a given sigma tests every gene
    assert ao.ae_outlier(text, ctx=emu, threads=1, **kw) == out                               # a second call returns equal bytes


OUTPUT_NAMES = ["out.gene_var.txt", "out.outliers.txt", "out.pvalue.bed.gz", "out.pvalue.bed.gz.tbi", "out.qvalue.bed.gz", "out.qvalue.bed.gz.tbi", "out.summary.txt"]


def _read_outputs(prefix):
    out = {k: gzip.open("%s.%s.bed.gz" % (prefix, k), "rb").read() for k in ("pvalue", "qvalue")}
    for k in ("gene_var", "outliers", "summary"):
        out[k] = open("%s.%s.txt" % (prefix, k)).read()
    return out


def _assert_cli(tmp, ctx, form, sort, sigma, capsys):
    """the command line twice (with another --t) on a plain or BGZF matrix: the files, equal bytes, the numbers against the restatement"""
    from phaser_amd import ae_outlier as ao, vcfout
    text = population_matrix(sort)
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
        assert ao.main(["--bed", src, "--o", prefix, "--t", str(1 + k), "--sigma", str(sigma)]) == 0
        names = sorted(os.listdir(os.path.dirname(prefix)))
        assert names == (OUTPUT_NAMES if sort else [x for x in OUTPUT_NAMES if not x.endswith(".tbi")])
        runs.append({x: open(os.path.join(os.path.dirname(prefix), x), "rb").read() for x in names})
    assert runs[0] == runs[1]                                 # a second run (with another --t) writes identical files
    printed = capsys.readouterr().out
    assert "K_blnfit" in printed and ("not position-sorted" in printed) == (not sort)
    _, _, a, b = R0.py_parse(text)
    s, grid = _gene_sigmas(ctx, a, b, 0.5, 8, TOOL_MIN_SAMPLES, sigma)
    _assert_outputs(_read_outputs(os.path.join(tmp, "run0", "out")), text, 0.5, 8, TOOL_MIN_SAMPLES, 0.05, sigma, s, grid)


CLI_CASES = [("bgzf", True, "auto"), ("plain", False, "auto"), ("plain", True, 0.3)]


@pytest.mark.parametrize("form,sort,sigma", CLI_CASES)
def test_cli_on_emulated_kernels_matches_restatement(tmp_path, emus, monkeypatch, capsys, form, sort, sigma):
    from phaser_amd import _lib
    monkeypatch.setattr(_lib, "Context", lambda device=0: emus["product"])          # the command line makes its own context: here the emulated one
    _assert_cli(str(tmp_path), emus["product"], form, sort, sigma, capsys)


@pytest.mark.parametrize("argv", [["--sigma", "2.5"], ["--sigma", "1e-4"], ["--sigma", "-0.1"], ["--sigma", "nan"], ["--sigma", "lots"], ["--sigma", "0"]])
def test_bad_sigma_prints_a_line_and_exits_1(tmp_path, capsys, argv):
    from phaser_amd import ae_outlier as ao
    src = os.path.join(str(tmp_path), "in.txt")
    open(src, "w").write(population_matrix())
    assert ao.main(["--bed", src, "--o", os.path.join(str(tmp_path), "out")] + argv) == 1
    lines = [l for l in capsys.readouterr().out.split("\n") if l.startswith("FATAL ERROR - ")]
    assert lines == ["FATAL ERROR - --sigma must be auto or a number in [0.001, 2]"], lines
    assert sorted(os.listdir(str(tmp_path))) == ["in.txt"]


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_kblntest_gpu_matches_restatement(gpu_ctx):
    from phaser_amd import _lib
    gpu_ctx.reset_timing()
    _assert_bln_matches_restatement(gpu_ctx.lib, gpu_ctx.h, "gpu")
    assert gpu_ctx.timing(_lib.PHZ_T_BLNTEST)[2] > 0 and gpu_ctx.timing(_lib.PHZ_T_BLNTEST)[0] > 0


@pytest.mark.gpu
def test_kblntest_gpu_untested_cells_and_nan_s(gpu_ctx):
    _assert_untested_cells(gpu_ctx.lib, gpu_ctx.h)


@pytest.mark.gpu
def test_kblnfit_gpu_quality_and_equal_bits_across_spaces_and_runs(gpu_ctx):
    import torch
    from phaser_amd import _lib
    gpu_ctx.reset_timing()
    first = _assert_fit(gpu_ctx.lib, gpu_ctx.h, "gpu")
    assert gpu_ctx.timing(_lib.PHZ_T_BLNFIT)[2] > 0 and gpu_ctx.timing(_lib.PHZ_T_BLNFIT)[0] > 0
    assert _bits(_assert_fit(gpu_ctx.lib, gpu_ctx.h, "gpu, second run")) == _bits(first)
    dev = torch.device("cuda", gpu_ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    for p0, (a, b, sizes, rows) in fit_reference().items():
        ta = torch.from_numpy(np.array(a)).to(dev); tb = torch.from_numpy(np.array(b)).to(dev)
        ts = torch.full((a.shape[0],), -5.0, dtype=torch.float64, device=dev); tl = ts.clone(); tm = ts.clone()
        tn = torch.full((a.shape[0],), -5, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        gpu_ctx.check(gpu_ctx.lib.phz_bln_fit(gpu_ctx.h, a.shape[0], a.shape[1], p(ta), p(tb), p0, R.FIT_MIN_COV, R.FIT_MIN_SAMPLES, p(ts), p(tl), p(tm), p(tn),
                                              _lib.PHZ_DEVICE))
        s, ll, ll_min, used = first[p0]
        for t, h in ((ts, s), (tl, ll), (tm, ll_min)):
            assert np.array_equal(t.cpu().numpy().view(np.uint64), h.view(np.uint64)), p0
        assert np.array_equal(tn.cpu().numpy(), used)


@pytest.mark.gpu
def test_kblntest_gpu_device_space_gives_the_bits_of_host_space(gpu_ctx):
    import torch
    from phaser_amd import _lib, ae_outlier as ao
    dev = torch.device("cuda", gpu_ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    for p0, (a, b, s, ref, err) in bln_reference().items():
        host = ao.bln_test(gpu_ctx.lib, gpu_ctx.h, a, b, p0, s, 0)
        ta = torch.from_numpy(np.array(a)).to(dev); tb = torch.from_numpy(np.array(b)).to(dev); ts = torch.from_numpy(np.array(s)).to(dev)
        tp = torch.full(a.shape, -5.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        gpu_ctx.check(gpu_ctx.lib.phz_bln_test(gpu_ctx.h, a.shape[0], a.shape[1], p(ta), p(tb), p0, p(ts), 0, p(tp), _lib.PHZ_DEVICE))
        assert np.array_equal(tp.cpu().numpy().view(np.uint64), host.view(np.uint64)), p0


@pytest.mark.gpu
def test_gpu_argument_errors_of_both_entry_points(gpu_ctx):
    _assert_argument_errors(gpu_ctx.lib, gpu_ctx.h)


@pytest.mark.gpu
@pytest.mark.parametrize("form,sort,sigma", CLI_CASES)
def test_cli_gpu_matches_restatement(tmp_path, gpu_ctx, capsys, form, sort, sigma):
    _assert_cli(str(tmp_path), gpu_ctx, form, sort, sigma, capsys)
