"""A scipy-backed restatement of the overdispersed path of phaser_ae_test (K_bbfit and K_bbtest, phaser_amd/csrc/phz_aebb.hip), the yardstick of
tests/test_ae_betabinom.py: scipy.stats.betabinom.pmf over the full support with the two-sided rule applied literally, the 64 x 4 search of the fit restated
with scipy.stats.betabinom.logpmf sums, a bounded Brent beside it, and the tool on top of ae_test_restatement's parse and BH.  Also the fixed case lists and
the tolerance.  Nothing here calls the code under test."""
import functools
import math

import numpy as np

import ae_test_restatement as R0

P0S = [0.5, 0.52, 1.0 / 3.0, 0.05]
BIG_N = [63, 64, 65, 1000, 4999, 200000]
SD_OFFSETS = [0, -1, 1, -3, 3, -8, 8]
RHO_MIN = 1e-6
RERR = 1 + 1e-7
G, ROUNDS = 64, 4


def rho_max(p0):
    m = min(p0, 1.0 - p0)
    return m / (1.0 + m)


def rho_columns(p0):
    return [RHO_MIN, 1e-3, 0.03, rho_max(p0)]


def ab(p0, rho):
    s = (1.0 - rho) / rho
    return p0 * s, (1.0 - p0) * s


def sd_bb(n, p0, rho):
    return math.sqrt(n * p0 * (1 - p0) * (1 + (n - 1) * rho))


# ------------------------------------------------------------------------------------------------ K_bbtest: cases, reference, tolerance
def bb_cases():
    """{p0: (a, b)}, one entry per row; every row is tested under each of the four rho_columns(p0).  n = 1..12 with every k; n in BIG_N with k at 0, at n and
    at the mean plus 0, +-1, +-3, +-8 sd_bb(rho) for each of the four rho; a seeded block of n log-uniform in [13, 5000] with k within 6 sd_bb of the mean (the rho
    of the sd drawn per row).  The n = 200000 rows, the slow ones, come last: the prefixes that the tests repeat stop short of them.  About 300 rows, 1,190 cells per p0."""
    rng = np.random.default_rng(23)
    out = {}
    for p0 in P0S:
        ks, ns = [], []
        for n in range(1, 13):
            for k in range(n + 1):
                ks.append(k); ns.append(n)
        for _ in range(100):
            n = int(round(math.exp(rng.uniform(math.log(13), math.log(5000)))))
            rho = rho_columns(p0)[int(rng.integers(0, 4))]
            k = int(round(n * p0 + rng.uniform(-6, 6) * sd_bb(n, p0, rho)))
            ks.append(min(n, max(0, k))); ns.append(n)
        for n in BIG_N:
            seen = set()
            for k in [0, n] + [int(round(n * p0 + d * sd_bb(n, p0, rho))) for rho in rho_columns(p0) for d in SD_OFFSETS]:
                k = min(n, max(0, k))
                if k not in seen:
                    seen.add(k); ks.append(k); ns.append(n)
        k = np.array(ks, dtype=np.int64); n = np.array(ns, dtype=np.int64)
        out[p0] = (k.astype(np.int32), (n - k).astype(np.int32))
    return out


@functools.lru_cache(maxsize=64)
def _pmf(n, p0, rho):
    from scipy.stats import betabinom
    al, be = ab(p0, rho)
    pmf = betabinom.pmf(np.arange(n + 1), n, al, be)
    pmf.setflags(write=False)
    return pmf


def scipy_bb_one(k, n, p0, rho):
    """-> (P, near tie): P = min(1, sum of pmf(i) over all i in [0, n] with pmf(i) <= pmf(k) (1 + 1e-7)); near tie: scipy's own pmf puts some index within a relative
    1e-9 of that bound, so that the decision on the index is scipy's rounding, not a rule"""
    pmf = _pmf(n, p0, rho)
    thr = pmf[k] * RERR
    P = min(1.0, float(pmf[pmf <= thr].sum()))
    tie = bool(thr > 0.0 and np.any(np.abs(pmf - thr) <= 1e-9 * thr))
    return P, tie


def scipy_bb(a, b, p0, rho, min_cov):
    """the reference of phz_betabinom_test: a, b [rows, columns], rho per column -> (p-values with NaN where not tested or rho is NaN, near-tie mask)"""
    a = np.asarray(a, dtype=np.int64); b = np.asarray(b, dtype=np.int64)
    out = np.full(a.shape, np.nan); tie = np.zeros(a.shape, dtype=bool)
    order = sorted(np.ndindex(a.shape), key=lambda rc: (rc[1], int(a[rc] + b[rc])))          # cells that share (n, rho) follow each other: the pmf is cached
    memo = {}
    for r, c in order:
        x, y = int(a[r, c]), int(b[r, c])
        if x < 0 or y < 0 or x + y < max(min_cov, 1) or rho[c] != rho[c]:
            continue
        key = (x, y, float(rho[c]))
        if key not in memo:
            memo[key] = scipy_bb_one(x, x + y, p0, float(rho[c]))
        out[r, c], tie[r, c] = memo[key]
    return out, tie


def lgamma_error(N):
    """E(N): the growth of the error of a log pmf taken through lgamma, N its largest argument"""
    return 2.0 ** -52 * (N + 1) * math.log(N + 2)


def largest_argument(n, rho):
    return np.asarray(n, dtype=np.float64) + (1.0 - rho) / rho


def bb_error_units(ours, ref, n, rho):
    """|ours - ref| / ref in units of max(E(N), 2^-46), N = n + (1 - rho) / rho; where the reference is below 1e-250: 0 when ours < 1e-240, inf otherwise"""
    ours = np.asarray(ours, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    N = largest_argument(n, rho)
    unit = np.maximum(2.0 ** -52 * (N + 1) * np.log(N + 2), 2.0 ** -46)
    tiny = ref < 1e-250
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.abs(ours - ref) / ref / unit
    return np.where(tiny, np.where(ours < 1e-240, 0.0, np.inf), f)


# ------------------------------------------------------------------------------------------------ K_bbfit
FIT_SIZES = [0, 1, 30, 1000, 1025]
FIT_ROWS = 1300
FIT_MIN_COV = 8


def fit_true_rhos(p0):
    """None: binomial counts (the fit lands at or next to RHO_MIN)"""
    return [None, 0.003, 0.03, 0.2 if p0 == 0.5 else 0.04]


def fit_matrices():
    """{p0: (a, b, tested cells per column)}: FIT_ROWS x 20, a column per (tested cells in FIT_SIZES, true rho); the tested cells at seeded rows with n
    log-uniform in [8, 5000], the other cells alternately a -1 count and n < FIT_MIN_COV"""
    rng = np.random.default_rng(29)
    out = {}
    for p0 in (0.5, 0.05):
        cols_a, cols_b, sizes = [], [], []
        for m in FIT_SIZES:
            for rho in fit_true_rhos(p0):
                a = np.empty(FIT_ROWS, dtype=np.int64); b = np.empty(FIT_ROWS, dtype=np.int64)
                flip = np.arange(FIT_ROWS) % 2 == 0
                a[flip] = -1; b[flip] = rng.integers(0, 5000, int(flip.sum()))
                a[~flip] = rng.integers(0, 4, int((~flip).sum())); b[~flip] = rng.integers(0, 4, int((~flip).sum()))          # n <= 6 < FIT_MIN_COV
                rows = np.sort(rng.choice(FIT_ROWS, m, replace=False))
                n = np.round(np.exp(rng.uniform(math.log(8), math.log(5000), m))).astype(np.int64)
                if rho is None:
                    k = rng.binomial(n, p0)
                else:
                    al, be = ab(p0, rho)
                    k = rng.binomial(n, rng.beta(al, be, m))
                a[rows] = k; b[rows] = n - k
                cols_a.append(a); cols_b.append(b); sizes.append(m)
        out[p0] = (np.stack(cols_a, axis=1).astype(np.int32), np.stack(cols_b, axis=1).astype(np.int32), np.array(sizes, dtype=np.int64))
    return out


def tested_cells(a, b, min_cov):
    """-> (k, n) of the tested cells of one column"""
    a = np.asarray(a, dtype=np.int64); b = np.asarray(b, dtype=np.int64)
    ok = (a >= 0) & (b >= 0) & (a + b >= max(min_cov, 1))
    return a[ok], (a + b)[ok]


def scipy_ll(k, n, p0, rho):
    """the summed scipy log pmf at each rho of an array -> array"""
    from scipy.stats import betabinom
    rho = np.atleast_1d(np.asarray(rho, dtype=np.float64))
    s = (1.0 - rho) / rho
    return betabinom.logpmf(k[None, :], n[None, :], (p0 * s)[:, None], ((1.0 - p0) * s)[:, None]).sum(axis=1)


def fit_grid(k, n, p0):
    """the search of phz_betabinom_fit restated: -> (rho, LL, the step of the last round in ln rho); NaN, NaN, NaN without cells"""
    if len(k) == 0:
        return float("nan"), float("nan"), float("nan")
    lo, hi = math.log(RHO_MIN), math.log(rho_max(p0))
    for _ in range(ROUNDS):
        x = np.linspace(lo, hi, G)
        ll = scipy_ll(k, n, p0, np.clip(np.exp(x), RHO_MIN, rho_max(p0)))
        j = int(np.argmax(ll))                          # the first of the largest
        step = (hi - lo) / (G - 1)
        lo, hi = x[max(j - 1, 0)], x[min(j + 1, G - 1)]
    return float(np.clip(math.exp(x[j]), RHO_MIN, rho_max(p0))), float(ll[j]), step


def fit_brent(k, n, p0):
    """a bounded Brent in ln rho (xatol 1e-10) -> rho"""
    from scipy.optimize import minimize_scalar
    res = minimize_scalar(lambda x: -float(scipy_ll(k, n, p0, math.exp(x))[0]), bounds=(math.log(RHO_MIN), math.log(rho_max(p0))), method="bounded",
                          options={"xatol": 1e-10})
    return float(np.clip(math.exp(res.x), RHO_MIN, rho_max(p0)))


def last_step(p0):
    """the step of the last round in ln rho where no bracket was clipped at its end: each round keeps two steps of the one before"""
    return (math.log(rho_max(p0)) - math.log(RHO_MIN)) / (G - 1) * (2.0 / (G - 1)) ** (ROUNDS - 1)


# ------------------------------------------------------------------------------------------------ the tool
def restate_bed(text, null, min_cov, fdr, rho):
    """ae_test_restatement.restate_bed with the p-values of the beta-binomial test at `rho` (one per sample: the caller's, a fitted one is not refitted here);
    "rho" in the result: per sample, NaN where the sample has no tested gene"""
    header, leads, a, b = R0.py_parse(text)
    samples = header.split("\t")[4:]
    rho = np.asarray(rho, dtype=np.float64)
    p, _ = scipy_bb(a, b, null, rho, min_cov)
    q, nt = R0.scipy_bh(p)
    sig = []
    for r in range(p.shape[0]):
        for c in range(p.shape[1]):
            if q[r, c] <= fdr:
                sig.append((leads[r].split("\t")[3], samples[c], int(a[r, c]), int(b[r, c]), R0.log2_afc(int(a[r, c]), int(b[r, c])), p[r, c], q[r, c]))
    summary = []
    for c, s in enumerate(samples):
        col = p[:, c][~np.isnan(p[:, c])]
        summary.append((s, int(nt[c]), int(np.sum(q[:, c] <= fdr)), float(col.min()) if len(col) else float("nan"), float(rho[c]) if nt[c] else float("nan")))
    return {"header": header, "leads": leads, "samples": samples, "a": a, "b": b, "p": p, "q": q, "significant": sig, "summary": summary}


def gene_ae_columns(text):
    """-> (header fields, data lines, a, b, `bam` values in order of first appearance, column of every line)"""
    lines = [l for l in (l.rstrip("\r") for l in text.split("\n")) if l]
    head = lines[0].split("\t")
    ia, ib, ibam = head.index("aCount"), head.index("bCount"), head.index("bam")
    rows = [l.split("\t") for l in lines[1:]]
    a = np.array([int(r[ia]) for r in rows], dtype=np.int64); b = np.array([int(r[ib]) for r in rows], dtype=np.int64)
    bams = []
    for r in rows:
        if r[ibam] not in bams:
            bams.append(r[ibam])
    col = np.array([bams.index(r[ibam]) for r in rows], dtype=np.int64)
    return head, lines[1:], a, b, bams, col


def restate_gene_ae(text, null, min_cov, rho):
    """-> (header fields, data lines, p, q, rho per line): `rho` per `bam` value in order of first appearance; BH per `bam` value"""
    head, lines, a, b, bams, col = gene_ae_columns(text)
    p = np.full(len(lines), np.nan); q = np.full(len(lines), np.nan); rl = np.full(len(lines), np.nan)
    for j in range(len(bams)):
        pick = col == j
        pj, _ = scipy_bb(a[pick].reshape(-1, 1), b[pick].reshape(-1, 1), null, np.array([rho[j]]), min_cov)
        qj, nt = R0.scipy_bh(pj)
        p[pick] = pj[:, 0]; q[pick] = qj[:, 0]
        rl[pick] = rho[j] if nt[0] else np.nan
    return head, lines, p, q, rl
