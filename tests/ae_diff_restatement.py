"""A restatement of phaser_ae_diff (phaser_amd/ae_diff.py), the yardstick of tests/test_ae_diff.py.  Fisher's exact test by its rule in exact integers
(N <= 4096) or in 50-digit mpmath arithmetic (above), the Cochran-Mantel-Haenszel sums in fractions.Fraction and scipy.stats.chi2.sf, Benjamini-Hochberg
through scipy, a plain Python parse and alignment of the two matrices.  Also the fixed case lists of the kernel tests and the tolerances they are held to.
Nothing here calls the code under test."""
import math
from fractions import Fraction

import numpy as np

import ae_test_restatement as R0

N1S = [1, 2, 3, 8, 9, 20, 63, 64, 65, 100, 257, 1000, 200000]
EXACT_MAX_N = 4096
TOL_NUM, TOL_DEN = 10 ** 7 + 1, 10 ** 7          # the rule's 1 + 1e-7, as a ratio of integers


# ------------------------------------------------------------------------------------------------ K_fisher: reference
def _support(a1, b1, a2, b2):
    n1, n2, m = a1 + b1, a2 + b2, a1 + a2
    return n1, n2, m, max(0, m - n2), min(n1, m)


def fisher_exact_int(a1, b1, a2, b2):
    """-> (p, near_tie) in integers: w_i = C(n1, i) C(n2, m - i), the set {i: w_i 10^7 <= w_k (10^7 + 1)}, p = sum over the set / C(N, m).  The first
    weight comes from math.comb, the others by the recurrence in exact integer division (checked against math.comb at the last index)."""
    n1, n2, m, lo, hi = _support(a1, b1, a2, b2)
    w = [math.comb(n1, lo) * math.comb(n2, m - lo)]
    for x in range(lo, hi):
        num = w[-1] * (n1 - x) * (m - x); den = (x + 1) * (n2 - m + x + 1)
        assert num % den == 0
        w.append(num // den)
    assert w[-1] == math.comb(n1, hi) * math.comb(n2, m - hi)
    wk = w[a1 - lo]
    inside = sum(x for x in w if x * TOL_DEN <= wk * TOL_NUM)
    total = math.comb(n1 + n2, m)
    assert sum(w) == total
    # near tie: some w_i != w_k with w_i / w_k within 1e-6 of 1 or of 1 + 1e-7
    near = any(x != wk and (abs(x - wk) * 10 ** 6 <= wk or abs(x * TOL_DEN - wk * TOL_NUM) * 10 ** 6 <= wk * TOL_DEN) for x in w)
    return float(Fraction(min(inside, total), total)), near


def fisher_mp(a1, b1, a2, b2):
    """-> (p, near_tie) at 50 digits.  The pmf is unimodal (mode floor((n1+1)(m+1)/(N+2))): the set of the rule is a lower and an upper run of the support, each
    found by bisection of the 50-digit log pmf on its side of the mode and summed outward by the ratio recurrence until a term is below 1e-60 of the sum."""
    import mpmath
    n1, n2, m, lo, hi = _support(a1, b1, a2, b2)
    N = n1 + n2
    with mpmath.workdps(50):
        lg = lambda v: mpmath.loggamma(v + 1)
        base = lg(n1) + lg(n2) + lg(m) + lg(N - m) - lg(N)
        lp = lambda x: base - lg(x) - lg(n1 - x) - lg(m - x) - lg(n2 - m + x)
        k = a1
        lk = lp(k)
        thr = lk + mpmath.log(mpmath.mpf(TOL_NUM) / TOL_DEN)
        mode = min(hi, max(lo, (n1 + 1) * (m + 1) // (N + 2)))
        # jl: the largest i in [lo, mode] with lp <= thr (lo - 1: none); jr: the smallest i in [mode, hi] with lp <= thr (hi + 1: none)
        if lp(lo) <= thr:
            a, b = lo, mode
            while a < b:
                mid = (a + b + 1) // 2
                if lp(mid) <= thr: a = mid
                else: b = mid - 1
            jl = a
        else:
            jl = lo - 1
        if lp(hi) <= thr:
            a, b = mode, hi
            while a < b:
                mid = (a + b) // 2
                if lp(mid) <= thr: b = mid
                else: a = mid + 1
            jr = a
        else:
            jr = hi + 1
        near = False
        for i in (jl, jl + 1, jr - 1, jr):
            if lo <= i <= hi and i != k:
                ratio = mpmath.exp(lp(i) - lk)
                if ratio != 1 and (abs(ratio - 1) <= mpmath.mpf("1e-6") or abs(ratio - mpmath.mpf(TOL_NUM) / TOL_DEN) <= mpmath.mpf("1e-6")):
                    # an exact tie (the mirror of a symmetric pmf) differs from 1 by the 50-digit rounding alone
                    if abs(ratio - 1) > mpmath.mpf("1e-38"):
                        near = True
        if jl >= jr:
            return 1.0, near
        total = mpmath.mpf(0)
        if jl >= lo:
            term = mpmath.exp(lp(jl) - lk); s = term; x = jl
            while x > lo and term > mpmath.mpf("1e-60") * s:
                term = term * x * (n2 - m + x) / ((n1 - x + 1) * (m - x + 1)); x -= 1; s += term
            total += s
        if jr <= hi:
            term = mpmath.exp(lp(jr) - lk); s = term; x = jr
            while x < hi and term > mpmath.mpf("1e-60") * s:
                term = term * (n1 - x) * (m - x) / ((x + 1) * (n2 - m + x + 1)); x += 1; s += term
            total += s
        p = total * mpmath.exp(lk)          # the sums are relative to pmf(k): no underflow before the last step
        return float(min(p, mpmath.mpf(1))), near


def fisher_reference(a1, b1, a2, b2, min_cov=0):
    """-> (p-values with NaN where the cell is not tested, near-tie mask), any shape"""
    a1 = np.asarray(a1, dtype=np.int64); b1 = np.asarray(b1, dtype=np.int64); a2 = np.asarray(a2, dtype=np.int64); b2 = np.asarray(b2, dtype=np.int64)
    p = np.full(a1.shape, np.nan); near = np.zeros(a1.shape, dtype=bool)
    memo = {}
    for idx in np.ndindex(a1.shape):
        t = (int(a1[idx]), int(b1[idx]), int(a2[idx]), int(b2[idx]))
        if min(t) < 0 or t[0] + t[1] < max(min_cov, 1) or t[2] + t[3] < max(min_cov, 1):
            continue
        if t not in memo:
            memo[t] = fisher_exact_int(*t) if sum(t) <= EXACT_MAX_N else fisher_mp(*t)
        p[idx], near[idx] = memo[t]
    return p, near


def scipy_fisher(a1, b1, a2, b2):
    from scipy.stats import fisher_exact
    return np.array([fisher_exact([[int(w), int(x)], [int(y), int(z)]])[1] for w, x, y, z in zip(a1, b1, a2, b2)])


# ------------------------------------------------------------------------------------------------ K_fisher: the fixed list, the tolerance
def fisher_cases():
    """-> (a1, b1, a2, b2) int32, about 3,000 tables: for every n1 of N1S the corners, then n2 from {n1, n1 / 2, n1 + 1, 2 n1} and random values with a1 and
    a2 drawn binomially around a common ratio (a2's shifted by up to a few standard deviations).  Fewer random tables at n1 = 200000, where the reference
    is the 50-digit one."""
    rng = np.random.default_rng(23)
    rows = []
    for n in N1S:
        h = n // 2
        rows += [(0, n, n, 0), (n, 0, 0, n), (n, 0, n, 0), (0, n, 0, n),           # the two extreme tables, the one-point supports m = N and m = 0
                 (h, n - h, h, n - h),                                                # balanced
                 (n // 3, n - n // 3, h, n - h), (h, n - h, n // 3, n - n // 3),      # a table and its mirror: an exact tie across the mode
                 (n // 3, n - n // 3, n - n // 3, n // 3)]                            # 2 m == N
        count = 60 if n == 200000 else 245
        fixed = [n, max(1, h), n + 1, 2 * n]
        for j in range(count):
            n2 = fixed[j % 4] if j < count // 2 else int(round(math.exp(rng.uniform(0.0, math.log(4.0 * n)))))
            n2 = max(1, n2)
            ratio = rng.uniform(0.03, 0.97)
            a1 = int(rng.binomial(n, ratio))
            sd = math.sqrt(max(ratio * (1 - ratio) / n + ratio * (1 - ratio) / n2, 1e-12))
            r2 = min(1.0, max(0.0, ratio + rng.uniform(-5, 5) * sd))
            a2 = int(rng.binomial(n2, r2))
            rows.append((a1, n - a1, a2, n2 - a2))
    t = np.array(rows, dtype=np.int32)
    return tuple(np.ascontiguousarray(t[:, j]) for j in range(4))


def lgamma_error(N):
    """E(N): the growth of the error of a log pmf taken through lgamma (lgamma(N + 1) is about N ln N, known to an ulp of that)"""
    return 2.0 ** -52 * (N + 1) * math.log(N + 2)


def fisher_error_units(ours, ref, N):
    """|ours - ref| / ref in units of max(E(N), 2^-46), per case; where the reference is below 1e-250 (0 included: the pmf underflows): 0 when ours < 1e-240,
    inf otherwise"""
    ours = np.asarray(ours, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64); N = np.asarray(N, dtype=np.float64)
    unit = np.maximum(2.0 ** -52 * (N + 1) * np.log(N + 2), 2.0 ** -46)
    tiny = ref < 1e-250
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.abs(ours - ref) / ref / unit
    return np.where(tiny, np.where(ours < 1e-240, 0.0, np.inf), f)


# ------------------------------------------------------------------------------------------------ K_cmh
def cmh_reference(a1, b1, a2, b2, min_cov=8, min_samples=2, correct=1):
    """per row of the [rows, columns] matrices -> dict of arrays: n_strata, stat, pvalue, log2_or, and the relative bounds stat_tol and (absolute) lor_tol that
    follow from n_strata * 2^-52 on each of the four sums (D's against the sum of its terms' magnitudes), the roundings of the last operations added:
      stat = e^2 / V, e = |D| - Y:   2 (eps sum|d| + 2^-53 |D|) / e  +  eps  +  3 * 2^-53          (e's subtraction, the square, the division)
      log2(R / S):                  (2 eps + 2^-52) / ln 2  +  2^-51 |log2(R / S)|                 (the division and an ulp of the logarithm, here and in the kernel)"""
    from scipy.stats import chi2
    a1 = np.asarray(a1, dtype=np.int64); b1 = np.asarray(b1, dtype=np.int64); a2 = np.asarray(a2, dtype=np.int64); b2 = np.asarray(b2, dtype=np.int64)
    rows = a1.shape[0]
    out = {"n_strata": np.zeros(rows, dtype=np.int32), "stat": np.full(rows, np.nan), "pvalue": np.full(rows, np.nan), "log2_or": np.full(rows, np.nan),
           "stat_tol": np.zeros(rows), "lor_tol": np.zeros(rows)}
    least = max(min_cov, 1)
    for r in range(rows):
        D = V = Rs = Ss = absD = Fraction(0)
        k = 0
        for c in range(a1.shape[1]):
            w, x, y, z = int(a1[r, c]), int(b1[r, c]), int(a2[r, c]), int(b2[r, c])
            if min(w, x, y, z) < 0 or w + x < least or y + z < least or w + x + y + z < 2:
                continue
            n1, n2, m, N = w + x, y + z, w + y, w + x + y + z
            d = Fraction(w * N - n1 * m, N)
            D += d; absD += abs(d); V += Fraction(n1 * n2 * m * (N - m), N * N * (N - 1)); Rs += Fraction(w * z, N); Ss += Fraction(x * y, N)
            k += 1
        out["n_strata"][r] = k
        eps = k * 2.0 ** -52
        if k >= max(min_samples, 1) and V != 0:
            Y = Fraction(1, 2) if correct and abs(D) >= Fraction(1, 2) else Fraction(0)
            e = abs(D) - Y
            stat = float(e * e / V)
            out["stat"][r] = stat; out["pvalue"][r] = chi2.sf(stat, 1)
            out["stat_tol"][r] = (2 * (eps * float(absD) + 2.0 ** -53 * float(abs(D))) / float(e) if e else 0.0) + eps + 3 * 2.0 ** -53
        if Ss == 0:
            out["log2_or"][r] = float("nan") if Rs == 0 else float("inf")
        elif Rs == 0:
            out["log2_or"][r] = float("-inf")
        else:
            lor = math.log2(float(Rs / Ss))          # the fraction is rounded once, then the logarithm: this reference's own 2^-53 / ln 2 + an ulp are in the bound
            out["log2_or"][r] = lor
            out["lor_tol"][r] = (2 * eps + 2.0 ** -52) / math.log(2) + 2.0 ** -51 * abs(lor)
    return out


def cmh_matrices(rows, cols, seed):
    """four [rows, cols] int32 matrices: counts around a per-gene ratio with a per-gene shift between the conditions, a tenth of the cells empty (-1) and a tenth
    below a coverage of 8"""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    n1 = rng.integers(8, 400, (rows, cols)); n2 = rng.integers(8, 400, (rows, cols))
    low = rng.random((rows, cols)) < 0.1
    n1[low] = rng.integers(0, 8, int(low.sum()))
    ratio = rng.uniform(0.2, 0.8, (rows, 1)); shift = rng.uniform(-0.15, 0.15, (rows, 1))
    a1 = rng.binomial(n1, ratio); a2 = rng.binomial(n2, np.clip(ratio + shift, 0.01, 0.99))
    b1 = n1 - a1; b2 = n2 - a2
    gone = rng.random((rows, cols)) < 0.1
    for m in (a1, b1):
        m[gone] = -1
    return tuple(np.ascontiguousarray(m, dtype=np.int32) for m in (a1, b1, a2, b2))


def cmh_pvalue_units(ours, ref, stat, stat_tol):
    """|ours - ref| / ref in units of (1 + stat) stat_tol + 2^-52: d ln p / d ln stat of the chi-square tail with one degree of freedom stays below
    (1 + stat) / 2 ... (1 + stat), and erfc itself is good to an ulp or so.  Reference below 1e-290: 0 when ours is below 1e-280."""
    unit = (1.0 + stat) * stat_tol + 2.0 ** -52
    tiny = ref < 1e-290
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.abs(ours - ref) / ref / unit
    return np.where(tiny, np.where(ours < 1e-280, 0.0, np.inf), f)


# ------------------------------------------------------------------------------------------------ the tool
class Fatal(Exception):
    pass


def _fmt(x):
    return "NA" if x != x else "%.6g" % x


def restate_tool(text1, text2, min_cov=8, min_samples=2, correct=1, fdr=0.05):
    """-> {"pvalue", "qvalue", "delta": matrix text (bytes), "cells", "genes", "summary": str, "dropped": (genes, samples)}: what phaser_ae_diff writes
    (the three matrices before compression)"""
    h1, leads1, a1, b1 = R0.py_parse(text1)
    h2, leads2, a2, b2 = R0.py_parse(text2)
    s1, s2 = h1.split("\t")[4:], h2.split("\t")[4:]
    g1 = [(l.split("\t") + ["", "", "", ""])[3] for l in leads1]; g2 = [(l.split("\t") + ["", "", "", ""])[3] for l in leads2]
    for names in (g1, g2, s1, s2):
        named = [n for n in names if n != ""]          # a row without a fourth column has no name: it matches nothing
        if len(set(named)) != len(named):
            raise Fatal("duplicate")
    rows = [i for i, g in enumerate(g1) if g != "" and g in set(g2)]; cols = [j for j, s in enumerate(s1) if s != "" and s in set(s2)]
    if not rows or not cols:
        raise Fatal("empty")
    r2 = [g2.index(g1[i]) for i in rows]; c2 = [s2.index(s1[j]) for j in cols]
    A1, B1 = a1[np.ix_(rows, cols)], b1[np.ix_(rows, cols)]
    A2, B2 = a2[np.ix_(r2, c2)], b2[np.ix_(r2, c2)]
    p, _ = fisher_reference(A1, B1, A2, B2, min_cov)
    q, nt = R0.scipy_bh(p)
    cm = cmh_reference(A1, B1, A2, B2, min_cov, min_samples, correct)
    gq, gnt = R0.scipy_bh(cm["pvalue"].reshape(-1, 1))
    samples = [s1[j] for j in cols]; genes = [g1[i] for i in rows]
    delta = np.full(p.shape, np.nan)
    for r in range(p.shape[0]):
        for c in range(p.shape[1]):
            if p[r, c] == p[r, c]:
                delta[r, c] = math.log2((A1[r, c] + .5) * (B2[r, c] + .5) / ((B1[r, c] + .5) * (A2[r, c] + .5)))
    header = "\t".join(h1.split("\t")[:4] + samples)

    def matrix(v):
        return (header + "\n" + "".join(leads1[i] + "\t" + "\t".join(_fmt(x) for x in v[k].tolist()) + "\n" for k, i in enumerate(rows))).encode()
    cells = ["gene\tsample\ta1\tb1\ta2\tb2\tdelta_log2_aFC\tpvalue\tqvalue\n"]
    for r in range(p.shape[0]):
        for c in range(p.shape[1]):
            if q[r, c] <= fdr:
                cells.append("%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n" % (genes[r], samples[c], A1[r, c], B1[r, c], A2[r, c], B2[r, c], _fmt(delta[r, c]), _fmt(p[r, c]), _fmt(q[r, c])))
    gl = ["gene\tn_strata\tlog2_or\tcmh_stat\tpvalue\tqvalue\n"]
    for r, g in enumerate(genes):
        gl.append("%s\t%d\t%s\t%s\t%s\t%s\n" % (g, cm["n_strata"][r], _fmt(cm["log2_or"][r]), _fmt(cm["stat"][r]), _fmt(cm["pvalue"][r]), _fmt(gq[r, 0])))
    summ = ["sample\ttested\tsignificant\tmin_pvalue\n"]
    for c, s in enumerate(samples):
        col = p[:, c][~np.isnan(p[:, c])]
        summ.append("%s\t%d\t%d\t%s\n" % (s, nt[c], int(np.sum(q[:, c] <= fdr)), _fmt(col.min() if len(col) else float("nan"))))
    gp = cm["pvalue"][~np.isnan(cm["pvalue"])]
    summ.append("#cmh_genes\t%d\t%d\t%s\n" % (gnt[0], int(np.sum(gq[:, 0] <= fdr)), _fmt(gp.min() if len(gp) else float("nan"))))
    return {"pvalue": matrix(p), "qvalue": matrix(q), "delta": matrix(delta), "cells": "".join(cells), "genes": "".join(gl), "summary": "".join(summ),
            "dropped": (len(g1) - len(rows), len(s1) - len(cols))}
