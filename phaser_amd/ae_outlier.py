"""phaser_ae_outlier: per-gene population variance of the allelic ratio and the samples that are outliers against it (the ANEVA / ANEVA-DOT step that
users of a phaser_expr_matrix population matrix take next; no counterpart in the reference).

    python -m phaser_amd.ae_outlier --bed matrix.bed.gz --o out [--null 0.5 --min_cov 8 --min_samples 10 --fdr 0.05 --sigma auto|S --t 1]

phaser_amd.ae_test and ae_betabinom ask of each aCount|bCount cell whether the gene is imbalanced in that sample, against a null with technical noise per
sample.  Here the question is asked per gene across samples.  The model is a logit-normal mixture of binomials centred at --null: x ~ N(logit(null), s^2),
aCount | x ~ Binomial(aCount + bCount, sigma(x)), with no technical overdispersion term and 1e-3 <= s <= 2.  A cell is tested when both counts are there and
aCount + bCount >= max(min_cov, 1).
  --sigma auto   the default: one s per gene, fitted from its tested cells (phz_bln_fit, K_blnfit: a fixed 64-candidate, 4-round search in ln s); a gene with
                 fewer than --min_samples tested cells is not fitted and none of its cells is tested
  --sigma S      no fit: every gene is tested at S; outside [1e-3, 2] one FATAL ERROR line, exit status 1, no file
The cells are tested by phz_bln_test (K_blntest): p = min(1, 2 min(P(X <= a), P(X >= a))) under the gene's s.  BH per sample (phz_bh_adjust), the matrix
parser, the row writer, the formatting, BGZF and tabix are those of phaser_amd.ae_test.  Outputs:
  <o>.gene_var.txt     per gene the four leading columns, n_used (tested cells), sigma, loglik (at sigma), loglik_min (at s = 1e-3, the binomial-like
                       likelihood to compare against); NA where not fitted
  <o>.pvalue.bed.gz, <o>.qvalue.bed.gz   the matrices (BGZF, tabix index when position-sorted)
  <o>.outliers.txt     one row per cell with q <= --fdr, row then column order: gene, sample, aCount, bCount, sigma, pvalue, qvalue
  <o>.summary.txt      per sample: tested genes, significant genes, smallest p
There is no CPU path: without a GPU the run raises.  Two runs on the same input write identical bytes.
"""
from __future__ import annotations

import argparse
import sys
import time
from typing import Optional

import numpy as np

from . import _lib
from . import ae_test as base
from .ae_test import Matrix, _check, _check_options, _fmt, _vp, bh_adjust
from .cis_var import FatalError

OUTLIERS_HEADER = ["gene", "sample", "aCount", "bCount", "sigma", "pvalue", "qvalue"]
GENE_VAR_COLUMNS = ["n_used", "sigma", "loglik", "loglik_min"]


def bln_fit(lib, handle, a, b, null: float = 0.5, min_cov: int = 8, min_samples: int = 10):
    """phz_bln_fit on [genes, samples] matrices -> (s, loglik, loglik at s = 1e-3, tested cells) per row; NaN, NaN, NaN for a row with fewer than min_samples tested cells"""
    a = np.ascontiguousarray(a, dtype=np.int32); b = np.ascontiguousarray(b, dtype=np.int32)
    assert a.ndim == 2 and a.shape == b.shape
    R = a.shape[0]
    s = np.empty(R, dtype=np.float64); ll = np.empty(R, dtype=np.float64); ll_min = np.empty(R, dtype=np.float64); used = np.zeros(R, dtype=np.int64)
    _check(lib, handle, lib.phz_bln_fit(handle, R, a.shape[1], _vp(a), _vp(b), float(null), int(min_cov), int(min_samples), _vp(s), _vp(ll), _vp(ll_min), _vp(used),
                                        _lib.PHZ_HOST))
    return s, ll, ll_min, used


def bln_test(lib, handle, a, b, null, s, min_cov: int = 8) -> np.ndarray:
    """phz_bln_test on [genes, samples] matrices with one s per row -> p-values in the shape of `a` (NaN where not tested, and in a row whose s is NaN)"""
    a = np.ascontiguousarray(a, dtype=np.int32); b = np.ascontiguousarray(b, dtype=np.int32)
    assert a.ndim == 2 and a.shape == b.shape
    s = np.ascontiguousarray(s, dtype=np.float64)
    assert s.shape == (a.shape[0],)
    p = np.empty(a.shape, dtype=np.float64)
    _check(lib, handle, lib.phz_bln_test(handle, a.shape[0], a.shape[1], _vp(a), _vp(b), float(null), _vp(s), int(min_cov), _vp(p), _lib.PHZ_HOST))
    return p


def _sigma(value):
    """"auto" | S, as given to --sigma or to ae_outlier() -> "auto" or a float inside the domain"""
    if isinstance(value, str) and value.strip().lower() == "auto":
        return "auto"
    try:
        s = float(value)
    except (TypeError, ValueError):
        s = float("nan")
    if not (_lib.PHZ_BLN_S_MIN <= s <= _lib.PHZ_BLN_S_MAX):
        raise FatalError("FATAL ERROR - --sigma must be auto or a number in [%g, %g]" % (_lib.PHZ_BLN_S_MIN, _lib.PHZ_BLN_S_MAX))
    return s


def _check_min_samples(min_samples: int):
    if min_samples < 1:
        raise FatalError("FATAL ERROR - --min_samples must be at least 1")


def _gene_var(mx, used, s, ll, ll_min) -> str:
    out = ["\t".join(mx.header.split("\t")[:4] + GENE_VAR_COLUMNS) + "\n"]
    t = mx.text
    for o, n, u, sv, l1, l0 in zip(mx.lead_off.tolist(), mx.lead_len.tolist(), used.tolist(), s.tolist(), ll.tolist(), ll_min.tolist()):
        out.append("%s\t%d\t%s\t%s\t%s\n" % (t[o:o + n].decode(), u, _fmt(sv), _fmt(l1), _fmt(l0)))
    return "".join(out)


def ae_outlier(bed_text, null: float = 0.5, min_cov: int = 8, min_samples: int = 10, fdr: float = 0.05, sigma="auto", threads: int = 1, ctx=None,
               stats: Optional[dict] = None) -> dict:
    """The tool on the text of a matrix -> {"gene_var": str, "pvalue": bytes, "qvalue": bytes, "outliers": str, "summary": str} (the two matrices before
    compression).  ctx: anything with .lib and .h (a _lib.Context; made here when None, which raises without a GPU)."""
    _check_options(null, fdr)
    _check_min_samples(min_samples)
    mode = _sigma(sigma)
    if ctx is None:
        ctx = _lib.Context(0)                          # raises without a GPU: there is no CPU path
    text = bed_text.encode() if isinstance(bed_text, str) else bytes(bed_text)
    t0 = time.perf_counter()
    mx = Matrix(text, threads)
    t1 = time.perf_counter()
    if mode == "auto":
        s, ll, ll_min, used = bln_fit(ctx.lib, ctx.h, mx.a, mx.b, null, min_cov, min_samples)
    else:
        s = np.full(mx.a.shape[0], mode, dtype=np.float64); ll = np.full(mx.a.shape[0], np.nan); ll_min = ll
        used = ((mx.a >= 0) & (mx.b >= 0) & (mx.a.astype(np.int64) + mx.b >= max(min_cov, 1))).sum(axis=1)
    t2 = time.perf_counter()
    pvalue = bln_test(ctx.lib, ctx.h, mx.a, mx.b, null, s, min_cov)
    t3 = time.perf_counter()
    qvalue, n_tested = bh_adjust(ctx.lib, ctx.h, pvalue)
    t4 = time.perf_counter()
    out = {"gene_var": _gene_var(mx, used, s, ll, ll_min), "pvalue": mx.rows_text(pvalue, threads), "qvalue": mx.rows_text(qvalue, threads)}
    t5 = time.perf_counter()
    with np.errstate(invalid="ignore"):
        rr, cc = np.nonzero(qvalue <= fdr)             # row order, then column order
    names = mx.names()
    rows = ["\t".join(OUTLIERS_HEADER) + "\n"]
    for r, c, a, b, p, q in zip(rr.tolist(), cc.tolist(), mx.a[rr, cc].tolist(), mx.b[rr, cc].tolist(), pvalue[rr, cc].tolist(), qvalue[rr, cc].tolist()):
        rows.append("%s\t%s\t%d\t%d\t%s\t%s\t%s\n" % (names[r], mx.samples[c], a, b, _fmt(float(s[r])), _fmt(p), _fmt(q)))
    out["outliers"] = "".join(rows)
    out["summary"] = base._summary(mx.samples, pvalue, qvalue, n_tested, fdr)
    if stats is not None:
        with np.errstate(invalid="ignore"):
            fitted = int((s == s).sum()) if mode == "auto" else 0
        stats.update({"genes": int(mx.a.shape[0]), "samples": len(mx.samples), "fitted": fitted, "tested": int(n_tested.sum()), "significant": int(len(rr)),
                      "seconds": {"parse": round(t1 - t0, 3), "fit": round(t2 - t1, 3), "test": round(t3 - t2, 3), "bh": round(t4 - t3, 3),
                                  "matrix_text": round(t5 - t4, 3), "lists": round(time.perf_counter() - t5, 3)}})
        if hasattr(ctx, "timing"):
            stats["k_blnfit_ms"] = ctx.timing(_lib.PHZ_T_BLNFIT)[0] if mode == "auto" else 0.0
            stats["k_blntest_ms"] = ctx.timing(_lib.PHZ_T_BLNTEST)[0]; stats["k_bh_ms"] = ctx.timing(_lib.PHZ_T_BH)[0]
    return out


def _banner():
    print(""); print("##################################################")
    print("        Welcome to phaser_ae_outlier (phaser_amd, MI355X)")
    print("##################################################"); print("")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bed", type=str, required=True)
    ap.add_argument("--o", type=str, required=True)
    ap.add_argument("--null", type=float, default=0.5); ap.add_argument("--min_cov", type=int, default=8)
    ap.add_argument("--min_samples", type=int, default=10)
    ap.add_argument("--fdr", type=float, default=0.05); ap.add_argument("--t", type=int, default=1)
    ap.add_argument("--sigma", type=str, default="auto", help="auto: one s fitted per gene; S: that s for every gene, no fit")
    args = ap.parse_args(argv)
    _banner()
    stats: dict = {}
    try:
        _check_options(args.null, args.fdr)
        _check_min_samples(args.min_samples)
        mode = _sigma(args.sigma)
        print("#1 Loading expression matrix...")
        with open(args.bed, "rb") as f:
            raw = f.read()
        if ".gz" in args.bed:                              # plain gzip and BGZF alike, as cis_var.read_text
            import gzip
            raw = gzip.decompress(raw)
        print("#2 Fitting the population variance and testing for outliers...")
        out = ae_outlier(raw, args.null, args.min_cov, args.min_samples, args.fdr, mode, threads=args.t, stats=stats)
    except FatalError as e:
        print(str(e))
        return 1
    from . import vcfout
    print("#3 Saving gene variances, p-value and q-value matrices...")
    with open(args.o + ".gene_var.txt", "w") as f:
        f.write(out["gene_var"])
    for kind in ("pvalue", "qvalue"):
        path = "%s.%s.bed.gz" % (args.o, kind)
        vcfout.write_bgzf(path, out[kind], args.t)
        if not vcfout.tabix_index(path, "bed", args.t):
            print("WARNING - %s is not position-sorted, no tabix index written (tabix refuses such files too)" % path)
    with open(args.o + ".outliers.txt", "w") as f:
        f.write(out["outliers"])
    with open(args.o + ".summary.txt", "w") as f:
        f.write(out["summary"])
    print("     %d genes x %d samples: %d genes fitted, %d cells tested, %d with q <= %g" % (stats["genes"], stats["samples"], stats["fitted"], stats["tested"],
                                                                                           stats["significant"], args.fdr))
    print("     seconds %s; K_blnfit %.3f ms, K_blntest %.3f ms, K_bh %.3f ms" % (stats["seconds"], stats.get("k_blnfit_ms", float("nan")),
                                                                                 stats.get("k_blntest_ms", float("nan")), stats.get("k_bh_ms", float("nan"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
