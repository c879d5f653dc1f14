"""A scipy-backed restatement of phaser_ae_test (phaser_amd/ae_test.py), the yardstick of tests/test_ae_test.py: scipy.stats.binomtest per cell,
scipy.stats.false_discovery_control(method="bh") per sample, a plain Python parse of the matrix.  Also the fixed case list of the K_binom tests and
the tolerance they are held to.  Nothing here calls the code under test."""
import math
import re

import numpy as np

P0S = [0.5, 0.52, 1.0 / 3.0, 0.05]
BIG_N = [63, 64, 65, 1000, 4999, 200000]
SD_OFFSETS = [0, -1, 1, -3, 3, -8, 8]
RERR = 1 + 1e-7


# ------------------------------------------------------------------------------------------------ K_binom: cases, reference, tolerance
def binom_cases():
    """{p0: (a, b)} -- the fixed list: n = 1..12 with every k; n in BIG_N with k at the mean, at +-1, +-3, +-8 standard deviations, at 0 and n; and a
    seeded block of n log-uniform in [13, 5000] with k within 6 standard deviations of the mean.  About 3,150 cases in all, more than 768 per p0: more than three workgroups of 256."""
    rng = np.random.default_rng(11)
    out = {}
    for p0 in P0S:
        ks, ns = [], []
        for n in range(1, 13):
            for k in range(n + 1):
                ks.append(k); ns.append(n)
        for n in BIG_N:
            sd = math.sqrt(n * p0 * (1 - p0))
            seen = set()
            for k in [0, n] + [int(round(n * p0 + d * sd)) for d in SD_OFFSETS]:
                k = min(n, max(0, k))
                if k not in seen:
                    seen.add(k); ks.append(k); ns.append(n)
        for _ in range(650):
            n = int(round(math.exp(rng.uniform(math.log(13), math.log(5000)))))
            sd = math.sqrt(n * p0 * (1 - p0))
            k = int(round(n * p0 + rng.uniform(-6, 6) * sd))
            ks.append(min(n, max(0, k))); ns.append(n)
        k = np.array(ks, dtype=np.int64); n = np.array(ns, dtype=np.int64)
        out[p0] = (k.astype(np.int32), (n - k).astype(np.int32))
    return out


def scipy_binom(a, b, p0, min_cov):
    """binomtest(a, a + b, p0).pvalue of every tested cell, NaN elsewhere (scipy is not called there)"""
    from scipy.stats import binomtest
    a = np.asarray(a, dtype=np.int64); b = np.asarray(b, dtype=np.int64)
    out = np.full(a.shape, np.nan)
    memo = {}
    for idx in np.ndindex(a.shape):
        x, y = int(a[idx]), int(b[idx])
        if x < 0 or y < 0 or x + y < max(min_cov, 1):
            continue
        if (x, y) not in memo:
            memo[(x, y)] = binomtest(x, x + y, p0, alternative="two-sided").pvalue
        out[idx] = memo[(x, y)]
    return out


def near_tie(k, n, p0):
    """scipy's own pmf puts some far-side index within a relative 1e-9 of pmf(k) * (1 + 1e-7): the decision on that index is scipy's rounding, not a rule"""
    from scipy.stats import binom
    mean = p0 * n
    if k == mean:
        return False
    far = np.arange(math.ceil(mean), n + 1) if k < mean else np.arange(0, math.floor(mean) + 1)
    thr = binom.pmf(k, n, p0) * RERR
    if thr == 0.0:
        return False
    return bool(np.any(np.abs(binom.pmf(far, n, p0) - thr) <= 1e-9 * thr))


def lgamma_error(n):
    """E(n): the growth of the error of a log pmf taken through lgamma"""
    return 2.0 ** -52 * (n + 1) * math.log(n + 2)


def binom_error_units(ours, ref, n):
    """|ours - ref| / ref in units of max(E(n), 2^-46), per case; where scipy returns less than 1e-250 its own tails underflow: 0 when ours < 1e-240,
    inf otherwise"""
    ours = np.asarray(ours, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64); n = np.asarray(n, dtype=np.float64)
    unit = np.maximum(2.0 ** -52 * (n + 1) * np.log(n + 2), 2.0 ** -46)
    tiny = ref < 1e-250
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.abs(ours - ref) / ref / unit
    return np.where(tiny, np.where(ours < 1e-240, 0.0, np.inf), f)


# ------------------------------------------------------------------------------------------------ K_bh
def scipy_bh(pm):
    """false_discovery_control(method="bh") of the non-NaN cells of every column -> (q matrix with NaN kept, tested cells per column)"""
    from scipy.stats import false_discovery_control
    pm = np.asarray(pm, dtype=np.float64)
    q = np.full(pm.shape, np.nan); nt = np.zeros(pm.shape[1], dtype=np.int64)
    for c in range(pm.shape[1]):
        ok = ~np.isnan(pm[:, c])
        nt[c] = int(ok.sum())
        if nt[c]:
            q[ok, c] = false_discovery_control(pm[ok, c], method="bh")
    return q, nt


# ------------------------------------------------------------------------------------------------ the tool
_CELL = re.compile(r"([0-9]+)\|([0-9]+)")


def py_parse(text):
    """-> (header line, [leading four columns of every row], a, b) with a = b = -1 for an empty or malformed cell"""
    lines = [l for l in (l.rstrip("\r") for l in text.split("\n")) if l]
    ncol = max(0, len(lines[0].split("\t")) - 4)
    leads, a, b = [], [], []
    for l in lines[1:]:
        f = l.split("\t")
        leads.append("\t".join(f[:4]))
        m = [_CELL.fullmatch(f[4 + j]) if 4 + j < len(f) else None for j in range(ncol)]
        ok = [x is not None and int(x.group(1)) + int(x.group(2)) < 2 ** 31 for x in m]
        a.append([int(x.group(1)) if k else -1 for x, k in zip(m, ok)]); b.append([int(x.group(2)) if k else -1 for x, k in zip(m, ok)])
    return lines[0], leads, np.array(a, dtype=np.int32).reshape(len(leads), ncol), np.array(b, dtype=np.int32).reshape(len(leads), ncol)


def log2_afc(a, b):
    if b == 0:
        return float("inf")
    return float("-inf") if a == 0 else math.log(float(a) / float(b), 2)


def restate_bed(text, null=0.5, min_cov=8, fdr=0.05):
    """-> dict: header, leads, samples, p, q (matrices), significant [(gene, sample, a, b, log2_aFC, p, q)] in row then column order,
    summary [(sample, tested, significant, smallest p or NaN)]"""
    header, leads, a, b = py_parse(text)
    samples = header.split("\t")[4:]
    p = scipy_binom(a, b, null, min_cov)
    q, nt = scipy_bh(p)
    sig = []
    for r in range(p.shape[0]):
        for c in range(p.shape[1]):
            if q[r, c] <= fdr:
                sig.append((leads[r].split("\t")[3], samples[c], int(a[r, c]), int(b[r, c]), log2_afc(int(a[r, c]), int(b[r, c])), p[r, c], q[r, c]))
    summary = []
    for c, s in enumerate(samples):
        col = p[:, c][~np.isnan(p[:, c])]
        summary.append((s, int(nt[c]), int(np.sum(q[:, c] <= fdr)), float(col.min()) if len(col) else float("nan")))
    return {"header": header, "leads": leads, "samples": samples, "a": a, "b": b, "p": p, "q": q, "significant": sig, "summary": summary}


def restate_gene_ae(text, null=0.5, min_cov=8):
    """-> (header fields, data lines, p per line, q per line): BH per `bam` value"""
    lines = [l for l in (l.rstrip("\r") for l in text.split("\n")) if l]
    head = lines[0].split("\t")
    ia, ib, ibam = head.index("aCount"), head.index("bCount"), head.index("bam")
    rows = [l.split("\t") for l in lines[1:]]
    a = np.array([int(r[ia]) for r in rows], dtype=np.int64); b = np.array([int(r[ib]) for r in rows], dtype=np.int64)
    p = scipy_binom(a, b, null, min_cov)
    q = np.full(len(rows), np.nan)
    for name in {r[ibam] for r in rows}:
        pick = np.array([r[ibam] == name for r in rows])
        qq, _ = scipy_bh(p[pick].reshape(-1, 1))
        q[pick] = qq[:, 0]
    return head, lines[1:], p, q
