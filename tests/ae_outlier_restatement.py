"""A scipy-backed restatement of phaser_ae_outlier (K_blnfit and K_blntest, phaser_amd/csrc/phz_aebln.hip), the yardstick of tests/test_ae_outlier.py.

The model: x ~ N(mu0, s^2), mu0 = logit(p0), k | x ~ Binomial(n, expit(x)).
  pmf     scipy.integrate.quad (epsrel 1e-13) of C(n, k) expit(x)^k (1 - expit(x))^(n-k) N(x; mu0, s), piecewise: the pieces are cut at the integrand's mode
          +- {2, 6, 20, 60} of its Laplace widths.  The integrand is taken relative to its value at the mode, so that nothing underflows inside quad.
  tails   P(X <= k) = quad of BinCDF(k; n, expit(x)) N(x; mu0, s) over mu0 +- 39 s, cut at the mode of g (the density of logit Beta(k + 1, n - k)) +- {3, 10, 40} w,
          w = 1 / sqrt((n + 1) pm (1 - pm)), pm = (k + 1) / (n + 1), and at mu0 and mu0 +- 8 s.  BinCDF is scipy.stats.binom.cdf, reached through the ufunc
          that it wraps where scipy exposes it (binom_cdf below): the wrapper costs 100 us a call and quad calls it a thousand times per tail;
          test_ae_outlier.py holds the two to equal bits on arguments of the list.  scipy.special.bdtr will not do: at n = 200,000 it is 7e-10 off.
          P(X >= k) is the lower tail of (n - k, -mu0).  A single quad over a wide interval is wrong here (at n = 200,000 it misses a peak 0.005 wide):
          piecewise throughout.
  p       min(1, 2 min(lower, upper))
Each value comes with quad's own error estimate, summed over the pieces.
The fit is restated with a likelihood that must be cheap (a row of 1,025 cells is evaluated 300 times): the same piecewise integral by fixed Gauss-Legendre
panels of 24 nodes between the same cuts, vectorised; test_ae_outlier.py holds it to the quad pmf on the case list.  Nothing here calls the code under test."""
import functools
import math

import numpy as np
from scipy import integrate, optimize, special

import ae_test_restatement as R0

try:
    from scipy.special._ufuncs import _binom_cdf as binom_cdf          # what scipy.stats.binom.cdf evaluates, without its argument checks
except ImportError:                                                    # another scipy: the wrapper itself, slower
    from scipy import stats

    def binom_cdf(k, n, p):
        return stats.binom.cdf(k, n, p)

P0S = [0.5, 1.0 / 3.0]
S_VALUES = [1e-3, 0.03, 0.3, 1.0, 2.0]
BIG_N = [63, 64, 65, 1000, 4999, 200000]
SD_OFFSETS = [0, -1, 1, -3, 3, -8, 8]
S_MIN, S_MAX = 1e-3, 2.0
G, ROUNDS = 64, 4
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def logit(p):
    return math.log(p) - math.log1p(-p)


def sd_bln(n, p0, s):
    v = n * p0 * (1 - p0)
    return math.sqrt(v + (v * s) ** 2)


# ------------------------------------------------------------------------------------------------ the case list
def bln_cases():
    """{p0: (a, b)}, one entry per column; every column is tested under each s of S_VALUES (a row per s).  n = 1..12 with every k; a seeded block of n
    log-uniform in [13, 5000] with k within 6 sd of the mean (the s of the sd drawn per case); n in BIG_N with k at 0, at n and at the mean plus 0, +-1, +-3,
    +-8 sd for each s, sd = sqrt(n p0 q0 + (n p0 q0 s)^2).  The n = 200000 columns come last."""
    rng = np.random.default_rng(41)
    out = {}
    for p0 in P0S:
        ks, ns = [], []
        for n in range(1, 13):
            for k in range(n + 1):
                ks.append(k); ns.append(n)
        for _ in range(110):
            n = int(round(math.exp(rng.uniform(math.log(13), math.log(5000)))))
            s = S_VALUES[int(rng.integers(0, len(S_VALUES)))]
            k = int(round(n * p0 + rng.uniform(-6, 6) * sd_bln(n, p0, s)))
            ks.append(min(n, max(0, k))); ns.append(n)
        for n in BIG_N:
            seen = set()
            for k in [0, n] + [int(round(n * p0 + d * sd_bln(n, p0, s))) for s in S_VALUES for d in SD_OFFSETS]:
                k = min(n, max(0, k))
                if k not in seen:
                    seen.add(k); ks.append(k); ns.append(n)
        k = np.array(ks, dtype=np.int64); n = np.array(ns, dtype=np.int64)
        out[p0] = (k.astype(np.int32), (n - k).astype(np.int32))
    return out


# ------------------------------------------------------------------------------------------------ pmf
def _mode(k, n, mu0, s):
    """mode and Laplace width of k log expit + (n - k) log(1 - expit) - (x - mu0)^2 / 2 s^2"""
    d1 = lambda x: k - n * special.expit(x) - (x - mu0) / (s * s)
    xm = optimize.brentq(d1, -800.0, 800.0, xtol=1e-14, rtol=8.9e-16)
    p = special.expit(xm)
    return xm, 1.0 / math.sqrt(n * p * (1.0 - p) + 1.0 / (s * s))


def _log_integrand(x, k, n, mu0, s):
    return k * special.log_expit(x) + (n - k) * special.log_expit(-x) - 0.5 * ((x - mu0) / s) ** 2 - math.log(s) - LOG_SQRT_2PI


def _lchoose(k, n):
    return special.gammaln(n + 1.0) - special.gammaln(k + 1.0) - special.gammaln(n - k + 1.0)


@functools.lru_cache(maxsize=None)
def log_pmf_quad(k, n, p0, s):
    """-> (log pmf, quad's relative error estimate)"""
    mu0 = logit(p0)
    xm, wl = _mode(k, n, mu0, s)
    h0 = float(_log_integrand(xm, k, n, mu0, s))
    cuts = [xm + d * wl for d in (-60, -20, -6, -2, 2, 6, 20, 60)]
    f = lambda x: math.exp(float(_log_integrand(x, k, n, mu0, s)) - h0)
    total = err = 0.0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        v, e = integrate.quad(f, lo, hi, epsabs=0.0, epsrel=1e-13, limit=200)
        total += v; err += e
    return float(_lchoose(k, n)) + h0 + math.log(total), err / total


def pmf_quad(k, n, p0, s):
    lp, e = log_pmf_quad(int(k), int(n), float(p0), float(s))
    return math.exp(lp), e


# ------------------------------------------------------------------------------------------------ tails
def _norm_pdf(x, mu0, s):
    return math.exp(-0.5 * ((x - mu0) / s) ** 2) / (s * math.sqrt(2.0 * math.pi))


def _lower_quad(k, n, mu0, s):
    """P(X <= k) -> (value, absolute error estimate)"""
    if k >= n:
        return 1.0, 0.0
    pm = (k + 1.0) / (n + 1.0)
    gm = math.log(pm) - math.log1p(-pm); w = 1.0 / math.sqrt((n + 1.0) * pm * (1.0 - pm))
    lo, hi = mu0 - 39.0 * s, mu0 + 39.0 * s
    cuts = sorted({min(hi, max(lo, c)) for c in [lo, hi, mu0, mu0 - 8 * s, mu0 + 8 * s] + [gm + d * w for d in (-40, -10, -3, 3, 10, 40)]})
    f = lambda x: float(binom_cdf(float(k), float(n), float(special.expit(x)))) * _norm_pdf(x, mu0, s)
    total = err = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        v, e = integrate.quad(f, a, b, epsabs=0.0, epsrel=1e-13, limit=200)
        total += v; err += e
    return total, err


@functools.lru_cache(maxsize=None)
def tails_quad(k, n, p0, s):
    """-> (lower, upper, relative error estimate of lower, of upper); where a value underflows to 0 there is nothing to estimate (0): such a case is judged by
    the rule for references below 1e-250"""
    import warnings
    mu0 = logit(p0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", integrate.IntegrationWarning)          # quad's complaints show in its error estimate, which the caller reads
        lo, elo = _lower_quad(k, n, mu0, s)
        up, eup = _lower_quad(n - k, n, -mu0, s)
    return lo, up, (elo / lo if lo > 0 else 0.0), (eup / up if up > 0 else 0.0)


def p_quad(k, n, p0, s):
    """-> (p-value, quad's relative error estimate of the tail that decides it)"""
    lo, up, elo, eup = tails_quad(int(k), int(n), float(p0), float(s))
    t, e = (lo, elo) if lo <= up else (up, eup)
    return min(1.0, 2.0 * t), e


def quad_bln(a, b, p0, s, min_cov):
    """the reference of phz_bln_test: a, b [rows, columns], s per row -> (p-values with NaN where not tested or s is NaN, quad's relative error estimates)"""
    a = np.asarray(a, dtype=np.int64); b = np.asarray(b, dtype=np.int64)
    out = np.full(a.shape, np.nan); err = np.zeros(a.shape)
    for r, c in np.ndindex(a.shape):
        x, y = int(a[r, c]), int(b[r, c])
        if x < 0 or y < 0 or x + y < max(min_cov, 1) or s[r] != s[r]:
            continue
        out[r, c], err[r, c] = p_quad(x, x + y, p0, float(s[r]))
    return out, err


# ------------------------------------------------------------------------------------------------ the tolerance
Q_FLOOR = 2.0 ** -36


def lgamma_error(n):
    """E(n) of K_binom: the growth of the error of log C(n, k) taken through lgamma"""
    n = np.asarray(n, dtype=np.float64)
    return 2.0 ** -52 * (n + 1) * np.log(n + 2)


def tolerance(n, s):
    """T(n, s) = E(n) + 2^-36 max(s, 1)^11.
    E(n) is the lgamma part.  The second term is the truncation error of a 32-node Gauss-Hermite rule laid over the mode: the rule is exact for a Gaussian
    integrand, and the integrand departs from one as s grows (the logistic factors are no longer narrow against the normal factor).  The issue's numpy
    measurement of that rule against quad -- not of this code -- gives 1.4e-11 up to s = 1, 4e-10 at s = 1.5, 2.6e-8 at s = 2: a power law through the ends
    has exponent log2(2.6e-8 / 1.4e-11) = 10.9.  2^-36 = 1.46e-11 also covers quad's own admitted error (cases above 1e-10 are left out)."""
    s = np.asarray(s, dtype=np.float64)
    return lgamma_error(n) + Q_FLOOR * np.maximum(s, 1.0) ** 11


def error_units(ours, ref, n, s):
    """|ours - ref| / ref in units of T(n, s); where the reference is below 1e-250: 0 when ours < 1e-240, inf otherwise"""
    ours = np.asarray(ours, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    tiny = ref < 1e-250
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.abs(ours - ref) / ref / tolerance(n, s)
    return np.where(tiny, np.where(ours < 1e-240, 0.0, np.inf), f)


def relative_error(ours, ref):
    """|ours - ref| / ref, 0 where the reference is below 1e-250"""
    ours = np.asarray(ours, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref < 1e-250, 0.0, np.abs(ours - ref) / ref)


# ------------------------------------------------------------------------------------------------ the fit
_GL_X, _GL_W = np.polynomial.legendre.leggauss(24)
_CUTS = np.array([-60.0, -20.0, -6.0, -2.0, 2.0, 6.0, 20.0, 60.0])


def log_pmf_panels(k, n, p0, s):
    """log pmf of arrays k, n (cells) at an array s (candidates) -> [candidates, cells]: Gauss-Legendre panels of 24 nodes between the cuts of log_pmf_quad"""
    k = np.asarray(k, dtype=np.float64)[None, :]; n = np.asarray(n, dtype=np.float64)[None, :]
    s = np.atleast_1d(np.asarray(s, dtype=np.float64))[:, None]
    mu0 = logit(p0); is2 = 1.0 / (s * s)
    # the mode by bisection of the decreasing derivative between mu0 and logit of the binomial's own mode (clipped), then Newton
    lo = np.full(np.broadcast_shapes(k.shape, s.shape), -800.0); hi = -lo
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        up = k - n * special.expit(mid) - (mid - mu0) * is2 > 0
        lo = np.where(up, mid, lo); hi = np.where(up, hi, mid)
    xm = 0.5 * (lo + hi)
    p = special.expit(xm)
    wl = 1.0 / np.sqrt(n * p * (1.0 - p) + is2)
    h = lambda x: k * special.log_expit(x) + (n - k) * special.log_expit(-x) - 0.5 * (x - mu0) ** 2 * is2 - np.log(s) - LOG_SQRT_2PI
    h0 = h(xm)
    total = np.zeros(xm.shape)
    for a, b in zip(_CUTS[:-1], _CUTS[1:]):
        half = 0.5 * (b - a) * wl; mid = xm + 0.5 * (a + b) * wl
        for x, w in zip(_GL_X, _GL_W):
            total += w * half * np.exp(h(mid + half * x) - h0)
    return _lchoose(k, n) + h0 + np.log(total)


def tested_cells(a, b, min_cov):
    """-> (k, n) of the tested cells of one row"""
    a = np.asarray(a, dtype=np.int64); b = np.asarray(b, dtype=np.int64)
    ok = (a >= 0) & (b >= 0) & (a + b >= max(min_cov, 1))
    return a[ok], (a + b)[ok]


def restated_ll(k, n, p0, s):
    """the summed restated log pmf at each s of an array -> array"""
    return log_pmf_panels(k, n, p0, s).sum(axis=1)


def fit_grid(k, n, p0):
    """the search of phz_bln_fit restated: -> (s, LL, LL(S_MIN), the step of the last round in ln s)"""
    lo, hi = math.log(S_MIN), math.log(S_MAX)
    ll_min = None
    for _ in range(ROUNDS):
        x = np.linspace(lo, hi, G)
        ll = restated_ll(k, n, p0, np.clip(np.exp(x), S_MIN, S_MAX))
        if ll_min is None:
            ll_min = float(ll[0])
        j = int(np.argmax(ll))                          # the first of the largest
        step = (hi - lo) / (G - 1)
        lo, hi = x[max(j - 1, 0)], x[min(j + 1, G - 1)]
    return float(np.clip(math.exp(x[j]), S_MIN, S_MAX)), float(ll[j]), ll_min, step


def fit_brent(k, n, p0):
    """a bounded Brent in ln s (xatol 1e-10) -> s"""
    res = optimize.minimize_scalar(lambda x: -float(restated_ll(k, n, p0, math.exp(x))[0]), bounds=(math.log(S_MIN), math.log(S_MAX)), method="bounded",
                                   options={"xatol": 1e-10})
    return float(np.clip(math.exp(res.x), S_MIN, S_MAX))


def last_step():
    """the step of the last round in ln s where no bracket was clipped at its end: each round keeps two steps of the one before"""
    return (math.log(S_MAX) - math.log(S_MIN)) / (G - 1) * (2.0 / (G - 1)) ** (ROUNDS - 1)


FIT_MIN_COV = 8
FIT_MIN_SAMPLES = 10
FIT_SIZES = [0, 1, FIT_MIN_SAMPLES - 1, FIT_MIN_SAMPLES, 64, 65, 1025]
FIT_TRUE_S = [None, 0.1, 0.5, 1.5]          # None: binomial counts (the fit lands at or next to S_MIN)
FIT_COLS = 1100


def fit_matrices():
    """{p0: (a, b, tested cells per row)}: 28 rows x FIT_COLS, a row per (tested cells in FIT_SIZES, true s); the tested cells at seeded columns with n
    log-uniform in [8, 5000], the other cells alternately a -1 count and n < FIT_MIN_COV"""
    rng = np.random.default_rng(43)
    out = {}
    for p0 in P0S:
        rows_a, rows_b, sizes = [], [], []
        for m in FIT_SIZES:
            for s in FIT_TRUE_S:
                a = np.empty(FIT_COLS, dtype=np.int64); b = np.empty(FIT_COLS, dtype=np.int64)
                flip = np.arange(FIT_COLS) % 2 == 0
                a[flip] = -1; b[flip] = rng.integers(0, 5000, int(flip.sum()))
                a[~flip] = rng.integers(0, 4, int((~flip).sum())); b[~flip] = rng.integers(0, 4, int((~flip).sum()))          # n <= 6 < FIT_MIN_COV
                cols = np.sort(rng.choice(FIT_COLS, m, replace=False))
                n = np.round(np.exp(rng.uniform(math.log(8), math.log(5000), m))).astype(np.int64)
                if s is None:
                    k = rng.binomial(n, p0)
                else:
                    k = rng.binomial(n, special.expit(rng.normal(logit(p0), s, m)))
                a[cols] = k; b[cols] = n - k
                rows_a.append(a); rows_b.append(b); sizes.append(m)
        out[p0] = (np.stack(rows_a).astype(np.int32), np.stack(rows_b).astype(np.int32), np.array(sizes, dtype=np.int64))
    return out


# ------------------------------------------------------------------------------------------------ the tool
def restate_bed(text, null, min_cov, min_samples, fdr, s):
    """phaser_ae_outlier on the text of a matrix with the restated p-values at `s` (one per gene: the caller's, a fitted one is not refitted here; NaN: the
    gene is not tested) -> dict: header, leads, samples, a, b, p, q, n_used per gene, loglik and loglik_min per gene (restated, NaN where s is NaN),
    outliers [(gene, sample, a, b, s, p, q)] in row then column order, summary [(sample, tested, significant, smallest p or NaN)]"""
    header, leads, a, b = R0.py_parse(text)
    samples = header.split("\t")[4:]
    s = np.asarray(s, dtype=np.float64)
    p, _ = quad_bln(a, b, null, s, min_cov)
    q, nt = R0.scipy_bh(p)
    n_used, ll, ll_min = [], [], []
    for r in range(a.shape[0]):
        k, n = tested_cells(a[r], b[r], min_cov)
        n_used.append(len(k))
        fitted = s[r] == s[r] and len(k) >= min_samples
        ll.append(float(restated_ll(k, n, null, s[r])[0]) if fitted else float("nan"))
        ll_min.append(float(restated_ll(k, n, null, S_MIN)[0]) if fitted else float("nan"))
    out = []
    for r in range(p.shape[0]):
        for c in range(p.shape[1]):
            if q[r, c] <= fdr:
                out.append((leads[r].split("\t")[3], samples[c], int(a[r, c]), int(b[r, c]), float(s[r]), p[r, c], q[r, c]))
    summary = []
    for c, name in enumerate(samples):
        col = p[:, c][~np.isnan(p[:, c])]
        summary.append((name, int(nt[c]), int(np.sum(q[:, c] <= fdr)), float(col.min()) if len(col) else float("nan")))
    return {"header": header, "leads": leads, "samples": samples, "a": a, "b": b, "p": p, "q": q, "n_used": n_used, "loglik": ll, "loglik_min": ll_min,
            "outliers": out, "summary": summary}
