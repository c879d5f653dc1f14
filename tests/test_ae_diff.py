"""phaser_ae_diff (phaser_amd/ae_diff.py; K_fisher and K_cmh in phaser_amd/csrc/phz_aediff.hip).

CPU tests: both kernels under the host emulation in three builds -- the product macros, PHZ_AETEST_GRID=3 (workgroups are reused) and PHZ_FISHER_WAVE_N=16
(almost every case takes the wave tier) -- K_fisher against the exact rule (ae_diff_restatement) on one fixed case list within a tolerance in units of lgamma's
error, K_cmh against sums taken in fractions; the cells that are not tested; the argument errors; the whole tool on the emulated kernels against a plain
Python restatement, byte for byte.  GPU tests: the same lists on the product kernels, PHZ_DEVICE against PHZ_HOST, two runs, the CLI as a child process."""
import ctypes as C
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import ae_diff_restatement as R

HIPEMU = os.path.join(REPO, "tests", "hipemu")
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
EMU_DIR = os.path.join(HIPEMU, "_build", "aediff")
BUILDS = {"product": [], "grid_3": ["-DPHZ_AETEST_GRID=3"], "wave_16": ["-DPHZ_FISHER_WAVE_N=16"]}

# The largest error of K_fisher over the fixed list, in units of max(E(N), 2^-46) (ae_diff_restatement.fisher_error_units), measured against the exact rule:
F_EMULATED = 2.113    # the emulated kernels (the host's libm lgamma): at [[277, 723], [209, 792]], the lane tier (wave tier build: 2.097, the same table)
F_GPU = 2.344         # the product kernels on an MI355X (the device library's lgamma; the same figure with PHZ_FISHER_WAVE_N at 8192 and with the wave tier off, the default): at [[836, 164], [1756, 244]]
FISHER_F = 4 * max(F_EMULATED, F_GPU)          # math libraries differ by an ulp or so between versions

# The largest error of K_cmh's p-value over the shapes below against scipy.stats.chi2.sf, in units of (1 + stat) stat_tol + 2^-52
# (ae_diff_restatement.cmh_pvalue_units):
C_EMULATED = 6.500    # the emulated kernel: at stat 2.0249, one stratum [[157, 47], [250, 102]]; chi2.sf itself is 2.6e-14 off there against 40-digit arithmetic, erfc(sqrt(stat / 2)) 5e-17
C_GPU = 6.456         # the product kernel on an MI355X: the same gene
CMH_F = 4 * max(C_EMULATED, C_GPU)

CMH_SAMPLES = (1, 2, 63, 64, 65, 257)
CMH_GENES = (1, 3, 70)


# ------------------------------------------------------------------------------------------------ the kernels under the emulation
def _emu_lib(tag):
    from phaser_amd import _lib
    os.makedirs(EMU_DIR, exist_ok=True)
    lib = os.path.join(EMU_DIR, "libphz_aediff_%s.so" % tag)
    srcs = [os.path.join(CSRC, "phz_api.hip"), os.path.join(CSRC, "phz_aetest.hip"), os.path.join(CSRC, "phz_aediff.hip"), os.path.join(HIPEMU, "hipemu.cpp")]
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
    for name in ("phz_ctx_create", "phz_ctx_destroy", "phz_last_error", "phz_strerror", "phz_bh_adjust", "phz_fisher_test", "phz_cmh_test"):
        res, args = _lib.SYMBOLS[name]
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


class EmuCtx:
    """what ae_diff needs of a _lib.Context, on an emulated library"""

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


# ------------------------------------------------------------------------------------------------ K_fisher
@functools.lru_cache(maxsize=None)
def fisher_list():
    """(a1, b1, a2, b2, exact p-values, near-tie mask) of the fixed list, computed once"""
    a1, b1, a2, b2 = R.fisher_cases()
    ref, near = R.fisher_reference(a1, b1, a2, b2, 0)
    for arr in (a1, b1, a2, b2, ref, near):
        arr.setflags(write=False)
    return a1, b1, a2, b2, ref, near


def test_fisher_case_list_covers_the_corners_and_has_few_near_ties():
    from phaser_amd import _lib
    a1, b1, a2, b2, ref, near = fisher_list()
    N = a1.astype(np.int64) + b1 + a2 + b2
    print("cases %d, near ties %d" % (len(a1), int(near.sum())))
    assert 2900 <= len(a1) <= 3400
    assert near.sum() <= 0.01 * len(a1), (int(near.sum()), len(a1))
    assert not np.isnan(ref).any() and np.all(ref >= 0) and np.all(ref <= 1)
    for n in R.N1S:
        at = (a1.astype(np.int64) + b1) == n
        assert np.any(at & (a1 == 0) & (b2 == 0) & (a2 == n)) and np.any(at & (b1 == 0) & (a2 == 0) & (b2 == n))          # the extreme tables
        assert np.all(ref[at & (b1 == 0) & (b2 == 0)] == 1.0) and np.any(at & (b1 == 0) & (b2 == 0))                       # m = N: one point
        assert np.all(ref[at & (a1 == 0) & (a2 == 0)] == 1.0) and np.any(at & (a1 == 0) & (a2 == 0))                       # m = 0: one point
        h = n // 2
        assert ref[at & (a1 == h) & (a2 == h) & (b2 == n - h)][0] == pytest.approx(1.0, abs=1e-12)                          # balanced
        i = np.nonzero(at & (a1 == n // 3) & (a2 == h) & (b2 == n - h))[0][0]; j = np.nonzero(at & (a1 == h) & (a2 == n // 3) & (b2 == n - n // 3))[0][0]
        assert ref[i] == pytest.approx(ref[j], rel=1e-14)                                                                                       # a table and its mirror
    assert np.any(ref[N == 400000] < 1e-250)                                                                                # pmf(k) underflows
    wave_n = int(_lib.PHZ_FISHER_WAVE_N)
    assert np.any(N <= 16) and np.any(N > 16) and np.any(N <= wave_n) and (wave_n >= 2 ** 31 - 1 or np.any(N > wave_n))     # both sides of either threshold


def test_fisher_restatement_agrees_with_scipy():
    a1, b1, a2, b2, ref, near = fisher_list()
    sp = R.scipy_fisher(a1, b1, a2, b2)
    ok = ~near
    big = ok & (ref >= 1e-250)
    rel = np.abs(sp[big] - ref[big]) / ref[big]
    i = int(np.argmax(rel))
    print("largest relative difference to scipy.stats.fisher_exact %.3g at %s" % (rel[i], [int(x[big][i]) for x in (a1, b1, a2, b2)]))
    assert rel[i] <= 1e-9
    assert np.all(sp[ok & (ref < 1e-250)] < 1e-240)          # below that scipy's own tails underflow


def _fisher_units(lib, handle, what):
    """-> (largest error in units of max(E(N), 2^-46) over the non-near-tie cases, its case); prefixes of 1, 63, 65 and 257 cells give the bits of the full call"""
    from phaser_amd import ae_diff
    a1, b1, a2, b2, ref, near = fisher_list()
    col = lambda x, n=None: np.array(x[:n]).reshape(-1, 1)
    got = ae_diff.fisher_test(lib, handle, col(a1), col(b1), col(a2), col(b2), 0)[:, 0]
    for count in (1, 63, 65, 257):
        part = ae_diff.fisher_test(lib, handle, col(a1, count), col(b1, count), col(a2, count), col(b2, count), 0)[:, 0]
        assert np.array_equal(part.view(np.uint64), got[:count].view(np.uint64)), (what, count)
    wide = ae_diff.fisher_test(lib, handle, *(np.array(x[:3000]).reshape(40, 75) for x in (a1, b1, a2, b2)), 0)          # the matrix shape does not enter
    assert np.array_equal(wide.reshape(-1).view(np.uint64), got[:3000].view(np.uint64)), what
    assert not np.isnan(got).any() and np.all(got >= 0) and np.all(got <= 1), what
    N = a1.astype(np.int64) + b1 + a2 + b2
    units = R.fisher_error_units(got, ref, N)
    units[near] = 0.0
    i = int(np.argmax(units))
    case = [int(x[i]) for x in (a1, b1, a2, b2)]
    print("%s: F = %.3f at %s (ours %.17g exact %.17g)" % (what, units[i], case, got[i], ref[i]))
    return float(units[i]), case, got


def _assert_fisher_matches_the_rule(lib, handle, what):
    worst, case, got = _fisher_units(lib, handle, what)
    assert worst <= FISHER_F, (what, case, worst)
    return got


def test_kfisher_emulated_matches_the_exact_rule(emu):
    _assert_fisher_matches_the_rule(emu.lib, emu.h, "emulated")


UNTESTED = np.array([[-1, 5, 5, 5], [5, -1, 5, 5], [5, 5, -1, 5], [5, 5, 5, -1], [3, 4, 5, 5], [5, 5, 3, 4], [4, 4, 4, 4], [0, 0, 5, 5], [5, 5, 0, 0], [1, 0, 0, 1], [0, 1, 8, 0],
                     [-1, -1, -1, -1], [2 ** 31 - 1, 2 ** 31 - 1, -1, 0]], dtype=np.int32)


def _assert_untested_cells(lib, handle):
    """min_cov 8: a negative count anywhere, n1 < 8 alone, n2 < 8 alone give NaN; n1 = n2 = 8 is tested.  min_cov 0, 1 and -3 test from n1, n2 >= 1."""
    from phaser_amd import ae_diff
    cols = [np.ascontiguousarray(UNTESTED[:, j]).reshape(-1, 1) for j in range(4)]
    got = ae_diff.fisher_test(lib, handle, *cols, 8)[:, 0]
    want, _ = R.fisher_reference(*[c[:, 0] for c in cols], 8)
    assert np.isnan(want).tolist() == [True, True, True, True, True, True, False, True, True, True, True, True, True]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and got[6] == pytest.approx(want[6], rel=1e-12)
    for mc in (0, 1, -3):
        got = ae_diff.fisher_test(lib, handle, *cols, mc)[:, 0]
        want, _ = R.fisher_reference(*[c[:, 0] for c in cols], mc)
        assert np.isnan(got).tolist() == [True, True, True, True, False, False, False, True, True, False, False, True, True], mc
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(got), ~ok) and np.allclose(got[ok], want[ok], rtol=1e-12, atol=0)


def test_kfisher_emulated_untested_cells_are_nan(emu):
    _assert_untested_cells(emu.lib, emu.h)


def test_argument_errors_leave_the_outputs_untouched(emu):
    from phaser_amd import _lib
    vp = lambda x: C.c_void_p(x.ctypes.data)
    a1 = np.array([5, 2 ** 30], dtype=np.int32); b1 = np.array([5, 2 ** 30 - 1], dtype=np.int32); a2 = np.array([5, 1], dtype=np.int32); b2 = np.array([5, 0], dtype=np.int32)
    p = np.full(2, -5.0); stat = np.full(2, -5.0); lor = np.full(2, -5.0); ns = np.full(2, -5, dtype=np.int32)
    fisher = lambda rows, cols: emu.lib.phz_fisher_test(emu.h, rows, cols, vp(a1), vp(b1), vp(a2), vp(b2), 8, vp(p), _lib.PHZ_HOST)
    cmh = lambda rows, cols: emu.lib.phz_cmh_test(emu.h, rows, cols, vp(a1), vp(b1), vp(a2), vp(b2), 8, 1, 1, vp(stat), vp(p), vp(lor), vp(ns), _lib.PHZ_HOST)
    for call in (fisher, cmh):
        assert call(2, 1) == _lib.PHZ_E_ARG and b"int32" in emu.lib.phz_last_error(emu.h)              # N = 2^31 in the second cell
        assert call(1, 2) == _lib.PHZ_E_ARG and b"int32" in emu.lib.phz_last_error(emu.h)
        assert call(2 ** 31, 1) == _lib.PHZ_E_ARG and b"2^31 - 1 cells" in emu.lib.phz_last_error(emu.h)
        assert call(2 ** 16, 2 ** 15) == _lib.PHZ_E_ARG and b"2^31 - 1 cells" in emu.lib.phz_last_error(emu.h)
        assert call(-1, 1) == _lib.PHZ_E_ARG
        assert np.all(p == -5.0) and np.all(stat == -5.0) and np.all(lor == -5.0) and np.all(ns == -5)
    assert emu.lib.phz_fisher_test(emu.h, 1, 1, vp(a1), vp(b1), vp(a2), vp(b2), 8, vp(p), 7) == _lib.PHZ_E_ARG and np.all(p == -5.0)
    assert fisher(1, 1) == _lib.PHZ_OK and p[0] == 1.0 and p[1] == -5.0
    assert cmh(1, 1) == _lib.PHZ_OK and ns[0] == 1 and ns[1] == -5 and stat[1] == -5.0


# ------------------------------------------------------------------------------------------------ K_cmh
@functools.lru_cache(maxsize=None)
def cmh_shapes():
    """[(genes, samples, the four matrices, reference)] at min_cov 8, min_samples 1, correct 1, computed once"""
    out = []
    for cols in CMH_SAMPLES:
        for rows in CMH_GENES:
            m = R.cmh_matrices(rows, cols, 5)
            for x in m:
                x.setflags(write=False)
            out.append((rows, cols, m, R.cmh_reference(*m, 8, 1, 1)))
    return out


def _close(got, want, tol_rel=None, tol_abs=None):
    """element by element: NaN where NaN, an infinity where that infinity, else within the tolerance"""
    got = np.asarray(got); want = np.asarray(want)
    fin = np.isfinite(want)
    if not (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])):
        return False
    bound = tol_rel[fin] * np.abs(want[fin]) if tol_rel is not None else tol_abs[fin]
    return bool(np.all(np.abs(got[fin] - want[fin]) <= bound))


def _cmh_units(lib, handle, what):
    """every shape against the restatement (n_strata exactly, stat and log2_or within the propagated bounds) -> the largest p-value error in its units"""
    from phaser_amd import ae_diff
    worst, where = 0.0, None
    for rows, cols, m, ref in cmh_shapes():
        stat, p, lor, ns = ae_diff.cmh_test(lib, handle, *m, 8, 1, 1)
        again = ae_diff.cmh_test(lib, handle, *m, 8, 1, 1)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip((stat, p, lor, ns), again)), (what, rows, cols)
        assert np.array_equal(ns, ref["n_strata"]), (what, rows, cols, ns.tolist(), ref["n_strata"].tolist())
        assert _close(stat, ref["stat"], tol_rel=ref["stat_tol"]), (what, rows, cols, stat.tolist(), ref["stat"].tolist())
        assert _close(lor, ref["log2_or"], tol_abs=ref["lor_tol"]), (what, rows, cols, lor.tolist(), ref["log2_or"].tolist())
        assert np.array_equal(np.isnan(p), np.isnan(ref["pvalue"]))
        ok = ~np.isnan(p)
        if ok.any():
            units = R.cmh_pvalue_units(p[ok], ref["pvalue"][ok], ref["stat"][ok], ref["stat_tol"][ok])
            i = int(np.argmax(units))
            if units[i] > worst:
                worst, where = float(units[i]), (rows, cols, int(np.nonzero(ok)[0][i]))
    print("%s: largest p-value error of K_cmh %.3f units at (genes, samples, gene) %s" % (what, worst, where))
    return worst, where


def test_kcmh_emulated_matches_the_fractions(emu):
    worst, where = _cmh_units(emu.lib, emu.h, "emulated")
    assert any(np.isfinite(ref["stat"]).any() for _, _, _, ref in cmh_shapes()) and worst <= CMH_F, (worst, where)


def _cmh_corner_matrices():
    """[8 genes, 4 samples]; -1 = empty.  Gene 0: V = 0 (every stratum has b1 = b2 = 0); 1: no cell with n1 >= 1 and n2 >= 1, so none with N >= 2, at any min_cov; 2: one stratum; 3: |D| < 0.5;
    4: S = 0; 5: R = 0; 6: R = S = 0; 7: the only tested sample is the last column"""
    e = (-1, -1, -1, -1)
    rows = [[(9, 0, 12, 0), (8, 0, 8, 0), e, (20, 0, 11, 0)],
            [(1, 0, -1, 0), (0, 1, 0, 0), (0, 0, 1, 0), e],
            [(20, 10, 10, 20), e, e, e],
            [(10, 10, 10, 11), (11, 10, 11, 10), e, e],
            [(10, 0, 4, 9), (7, 3, 0, 12), e, e],
            [(0, 9, 4, 9), (0, 12, 8, 3), e, e],
            [(0, 9, 0, 9), (10, 0, 8, 0), e, e],
            [e, (3, 3, 30, 30), (2, 2, 2, 2), (30, 10, 12, 28)]]
    t = np.array(rows, dtype=np.int32)
    return tuple(np.ascontiguousarray(t[:, :, j]) for j in range(4))


def _assert_cmh_corners(lib, handle):
    from phaser_amd import ae_diff
    m = _cmh_corner_matrices()
    for min_cov, min_samples, correct in ((8, 2, 1), (8, 1, 1), (8, 2, 0), (0, 1, 1), (8, 0, 1), (8, 3, 0)):
        ref = R.cmh_reference(*m, min_cov, min_samples, correct)
        stat, p, lor, ns = ae_diff.cmh_test(lib, handle, *m, min_cov, min_samples, correct)
        key = (min_cov, min_samples, correct)
        assert np.array_equal(ns, ref["n_strata"]), key
        assert _close(stat, ref["stat"], tol_rel=ref["stat_tol"]), (key, stat.tolist(), ref["stat"].tolist())
        assert _close(lor, ref["log2_or"], tol_abs=ref["lor_tol"]), (key, lor.tolist(), ref["log2_or"].tolist())
        assert _close(p, ref["pvalue"], tol_rel=np.full(len(p), 1e-12)), (key, p.tolist(), ref["pvalue"].tolist())
    stat, p, lor, ns = ae_diff.cmh_test(lib, handle, *m, 8, 2, 1)
    assert ns.tolist() == [3, 0, 1, 2, 2, 2, 2, 1]
    assert np.isnan(stat[0]) and np.isnan(p[0]) and ns[0] == 3                        # V = 0
    assert np.isnan(stat[2]) and np.isnan(stat[7])                                    # one stratum < min_samples 2
    assert stat[3] == pytest.approx(R.cmh_reference(*m, 8, 2, 0)["stat"][3], rel=1e-13)          # |D| < 0.5: no correction although correct = 1
    assert lor[4] == float("inf") and lor[5] == float("-inf") and np.isnan(lor[6]) and np.isnan(lor[0])
    assert np.isfinite(ae_diff.cmh_test(lib, handle, *m, 8, 1, 1)[0][7])              # the last column alone
    s0 = ae_diff.cmh_test(lib, handle, *m, 8, 2, 0)[0]; s1 = stat
    assert s0[4] > s1[4] > 0                                                          # correct = 0 leaves the 0.5 out
    assert ae_diff.cmh_test(lib, handle, *m, 0, 1, 1)[3][1] == 0                      # min_cov 0 still asks for n1, n2 >= 1: a stratum has N >= 2


def test_kcmh_emulated_corners(emu):
    _assert_cmh_corners(emu.lib, emu.h)


# ------------------------------------------------------------------------------------------------ the tool against the restatement
def _tool_texts():
    """two 7-gene x 6-sample matrices.  The second lists its genes in another order and ends its lines in \\r\\n; G7 and sample T6 are in the first alone, G8 and
    T7 in the second alone; each has a malformed cell and an empty one"""
    rng = np.random.default_rng(29)
    genes = ["G%d" % i for i in range(1, 8)]; s1 = ["T1", "T2", "T3", "T4", "T5", "T6"]; s2 = ["T3", "T7", "T1", "T2", "T5", "T4"]
    ratio = {"G1": (0.5, 0.5), "G2": (0.7, 0.3), "G3": (0.5, 0.62), "G4": (0.2, 0.2), "G5": (0.9, 0.5), "G6": (0.5, 0.45), "G7": (0.5, 0.5), "G8": (0.4, 0.6)}

    def cell(g, cond):
        n = int(rng.integers(3, 400))
        a = int(rng.binomial(n, ratio[g][cond]))
        return "%d|%d" % (a, n - a)
    l1 = ["\t".join(["#contig", "start", "stop", "name"] + s1)]
    for i, g in enumerate(genes):
        l1.append("\t".join(["chr1", str(100 * i + 10), str(100 * i + 60), g] + [cell(g, 0) for _ in s1]))
    f = l1[2].split("\t"); f[5] = "7|x"; l1[2] = "\t".join(f)
    f = l1[4].split("\t"); f[6] = ""; l1[4] = "\t".join(f)
    l2 = ["\t".join(["#contig", "start", "stop", "name"] + s2)]
    for i, g in enumerate(["G4", "G8", "G1", "G6", "G2", "G5", "G3"]):
        l2.append("\t".join(["chr1", str(100 * i + 10), str(100 * i + 60), g] + [cell(g, 1) for _ in s2]))
    f = l2[3].split("\t"); f[8] = "bad"; l2[3] = "\t".join(f)
    f = l2[5].split("\t"); f[4] = "0|0"; l2[5] = "\t".join(f)
    return "\n".join(l1) + "\n", "\r\n".join(l2) + "\r\n"


TOOL_OPTS = [dict(), dict(min_cov=0, min_samples=1, correct=0, fdr=0.2), dict(min_cov=40, min_samples=4, fdr=1.0), dict(fdr=0.0)]
TOOL_FILES = ("pvalue", "qvalue", "delta", "cells", "genes", "summary")


@pytest.mark.parametrize("opt", TOOL_OPTS)
def test_ae_diff_on_emulated_kernels_equals_the_restatement(emu, opt):
    from phaser_amd import ae_diff
    t1, t2 = _tool_texts()
    kw = dict(min_cov=8, min_samples=2, correct=1, fdr=0.05); kw.update(opt)
    stats = {}
    out = ae_diff.ae_diff(t1, t2, ctx=emu, threads=2, stats=stats, **kw)
    want = R.restate_tool(t1, t2, **kw)
    for k in TOOL_FILES:
        assert out[k] == want[k], (k, out[k], want[k])
    assert (stats["dropped_genes"], stats["dropped_samples"]) == want["dropped"] == (1, 1) and (stats["genes"], stats["samples"]) == (6, 5)
    if not opt:
        assert out["cells"].count("\n") > 3 and "\nG2\t" in out["genes"] and out["pvalue"].count(b"NA") >= 2
        assert out["pvalue"].split(b"\n")[0] == b"#contig\tstart\tstop\tname\tT1\tT2\tT3\tT4\tT5"
    assert ae_diff.ae_diff(t1, t2, ctx=emu, threads=1, **kw) == out


def test_ae_diff_refuses_duplicate_names_and_an_empty_intersection(emus):
    from phaser_amd import ae_diff
    emu = emus["product"]
    t1, t2 = _tool_texts()
    for bad in (t1.replace("\tG3\t", "\tG2\t"), t1.replace("\tT4\t", "\tT2\t")):
        with pytest.raises(ae_diff.FatalError, match="occurs twice in --bed1"):
            ae_diff.ae_diff(bad, t2, ctx=emu)
        with pytest.raises(ae_diff.FatalError, match="occurs twice in --bed2"):
            ae_diff.ae_diff(t2, bad, ctx=emu)
        with pytest.raises(R.Fatal):
            R.restate_tool(bad, t2)
    other_genes = t2.replace("\tG", "\tH")
    with pytest.raises(ae_diff.FatalError, match="no gene in common"):
        ae_diff.ae_diff(t1, other_genes, ctx=emu)
    other_samples = t2.replace("T", "U")
    with pytest.raises(ae_diff.FatalError, match="no sample in common"):
        ae_diff.ae_diff(t1, other_samples, ctx=emu)
    with pytest.raises(R.Fatal):
        R.restate_tool(t1, other_genes)


def test_cli_prints_a_fatal_error_and_exits_1(tmp_path, capsys):
    from phaser_amd import ae_diff
    t1, t2 = _tool_texts()
    p1 = os.path.join(str(tmp_path), "a.bed"); p2 = os.path.join(str(tmp_path), "b.bed")
    open(p1, "w").write(t1); open(p2, "w", newline="").write(t2)
    assert ae_diff.main(["--bed1", p1, "--bed2", p2, "--o", os.path.join(str(tmp_path), "out"), "--fdr", "1.5"]) == 1
    assert "FATAL ERROR - --fdr must lie between 0 and 1" in capsys.readouterr().out.split("\n")
    assert sorted(os.listdir(str(tmp_path))) == ["a.bed", "b.bed"]


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_kfisher_gpu_matches_the_exact_rule_in_both_spaces_and_twice(gpu_ctx):
    import torch
    from phaser_amd import _lib
    got = _assert_fisher_matches_the_rule(gpu_ctx.lib, gpu_ctx.h, "gpu")
    assert gpu_ctx.timing(_lib.PHZ_T_FISHER)[2] > 0 and gpu_ctx.timing(_lib.PHZ_T_FISHER)[0] > 0
    again = _fisher_units(gpu_ctx.lib, gpu_ctx.h, "gpu, second run")[2]
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
    a1, b1, a2, b2, ref, near = fisher_list()
    dev = torch.device("cuda", gpu_ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    t = [torch.from_numpy(np.array(x)).to(dev) for x in (a1, b1, a2, b2)]
    tp = torch.full((len(a1),), -5.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    gpu_ctx.check(gpu_ctx.lib.phz_fisher_test(gpu_ctx.h, len(a1), 1, p(t[0]), p(t[1]), p(t[2]), p(t[3]), 0, p(tp), _lib.PHZ_DEVICE))
    assert np.array_equal(tp.cpu().numpy().view(np.uint64), got.view(np.uint64))


@pytest.mark.gpu
def test_kfisher_gpu_untested_cells_are_nan(gpu_ctx):
    _assert_untested_cells(gpu_ctx.lib, gpu_ctx.h)


@pytest.mark.gpu
def test_kcmh_gpu_matches_the_fractions_in_both_spaces(gpu_ctx):
    import torch
    from phaser_amd import _lib, ae_diff
    worst, where = _cmh_units(gpu_ctx.lib, gpu_ctx.h, "gpu")          # two runs are compared in there
    assert worst <= CMH_F, (worst, where)
    assert gpu_ctx.timing(_lib.PHZ_T_CMH)[2] > 0
    _assert_cmh_corners(gpu_ctx.lib, gpu_ctx.h)
    dev = torch.device("cuda", gpu_ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    for rows, cols, m, ref in cmh_shapes():
        host = ae_diff.cmh_test(gpu_ctx.lib, gpu_ctx.h, *m, 8, 1, 1)
        t = [torch.from_numpy(np.array(x)).to(dev) for x in m]
        o = [torch.full((rows,), -5.0, dtype=torch.float64, device=dev) for _ in range(3)] + [torch.full((rows,), -5, dtype=torch.int32, device=dev)]
        torch.cuda.synchronize(dev)
        gpu_ctx.check(gpu_ctx.lib.phz_cmh_test(gpu_ctx.h, rows, cols, p(t[0]), p(t[1]), p(t[2]), p(t[3]), 8, 1, 1, p(o[0]), p(o[1]), p(o[2]), p(o[3]), _lib.PHZ_DEVICE))
        for x, y in zip(host, o):
            assert np.array_equal(x.view(np.uint8), y.cpu().numpy().view(np.uint8)), (rows, cols)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "gzip", "bgzf"])
def test_cli_gpu_as_a_child_process_equals_the_restatement(tmp_path, form):
    from phaser_amd import vcfout
    tmp = str(tmp_path)
    t1, t2 = _tool_texts()
    paths = []
    for k, text in enumerate((t1, t2)):
        if form == "plain":
            path = os.path.join(tmp, "c%d.bed" % k); open(path, "w", newline="").write(text)
        elif form == "gzip":
            path = os.path.join(tmp, "c%d.bed.gz" % k); gzip.open(path, "wb").write(text.encode())
        else:
            path = os.path.join(tmp, "c%d.bed.gz" % k); vcfout.write_bgzf(path, text, 2)
        paths.append(path)
    runs = []
    for k in (0, 1):
        d = os.path.join(tmp, "run%d" % k); os.makedirs(d)
        done = subprocess.run([sys.executable, "-m", "phaser_amd.ae_diff", "--bed1", paths[0], "--bed2", paths[1], "--o", os.path.join(d, "out"), "--t", str(1 + k)],
                              cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert done.returncode == 0, done.stdout.decode()
        assert b"1 gene(s) and 1 sample(s) of --bed1 are not in --bed2" in done.stdout and b"K_fisher" in done.stdout and b"WARNING" not in done.stdout
        runs.append({x: open(os.path.join(d, x), "rb").read() for x in sorted(os.listdir(d))})
    assert runs[0] == runs[1]                                 # a second run (with another --t) writes identical bytes
    assert sorted(runs[0]) == sorted(["out.%s.bed.gz" % k for k in ("pvalue", "qvalue", "delta")] + ["out.%s.bed.gz.tbi" % k for k in ("pvalue", "qvalue", "delta")] +
                                     ["out.%s.txt" % k for k in ("cells", "genes", "summary")])
    want = R.restate_tool(t1, t2)
    for k in ("pvalue", "qvalue", "delta"):
        assert gzip.decompress(runs[0]["out.%s.bed.gz" % k]) == want[k], k
    for k in ("cells", "genes", "summary"):
        assert runs[0]["out.%s.txt" % k].decode() == want[k], k
    if form == "plain":          # a --bed1 that is not position-sorted: the warning line, no index
        lines = t1.split("\n")
        src = os.path.join(tmp, "u.bed"); open(src, "w").write("\n".join([lines[0], lines[3], lines[1], lines[2]] + lines[4:]))
        d = os.path.join(tmp, "u"); os.makedirs(d)
        done = subprocess.run([sys.executable, "-m", "phaser_amd.ae_diff", "--bed1", src, "--bed2", paths[1], "--o", os.path.join(d, "out")],
                              cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert done.returncode == 0 and b"is not position-sorted, no tabix index written" in done.stdout
        assert not any(x.endswith(".tbi") for x in os.listdir(d))
