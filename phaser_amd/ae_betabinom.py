"""phaser_ae_test with an overdispersed null: phaser_amd.ae_test plus --overdispersion {0 | auto | RHO}.

    python -m phaser_amd.ae_betabinom --bed matrix.bed.gz --o out --overdispersion auto [--null 0.5 --min_cov 8 --fdr 0.05 --t 1]
    python -m phaser_amd.ae_betabinom --gene_ae sample.gene_ae.txt --o out --overdispersion 0.02 [...]

Haplotypic read counts are overdispersed against a binomial (library preparation, mapping bias, PCR duplicates), so the binomial test of
phaser_amd.ae_test turns anti-conservative as coverage grows.  Here the null is a beta-binomial with the same mean and overdispersion rho
(variance n p0 (1 - p0)(1 + (n - 1) rho)):
  auto   one rho per sample, fitted from all of its tested genes (phz_betabinom_fit, K_bbfit: a fixed 64-candidate, 4-round search in ln rho);
         in --gene_ae mode a sample is a `bam` value
  RHO    that rho for every sample; outside [1e-6, m / (1 + m)], m = min(null, 1 - null), one FATAL ERROR line, exit status 1, no file
  0      the default: phaser_amd.ae_test itself runs -- identical bytes, no new call
The cells are tested by phz_betabinom_test (K_bbtest) in place of phz_binom_test; BH (phz_bh_adjust), the p / q matrices, significant.txt, BGZF and tabix
are those of phaser_amd.ae_test, whose parser, row writer and formatting this module calls.  With the option on, summary.txt gains a fifth column `rho`
(%.6g, NA for a sample with no tested gene), the gene_ae table a `rho` column after qvalue, and the stats line names the K_bbfit and K_bbtest device times.
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
from .ae_test import Matrix, _check, _check_options, _fmt, _vp, bh_adjust, log2_afc
from .cis_var import FatalError, read_text


def betabinom_fit(lib, handle, a, b, null: float = 0.5, min_cov: int = 8):
    """phz_betabinom_fit on [rows, columns] matrices -> (rho, loglik, tested cells) per column; NaN, NaN, 0 for a column without a tested cell"""
    a = np.ascontiguousarray(a, dtype=np.int32); b = np.ascontiguousarray(b, dtype=np.int32)
    assert a.ndim == 2 and a.shape == b.shape
    rho = np.empty(a.shape[1], dtype=np.float64); ll = np.empty(a.shape[1], dtype=np.float64); used = np.zeros(a.shape[1], dtype=np.int64)
    _check(lib, handle, lib.phz_betabinom_fit(handle, a.shape[0], a.shape[1], _vp(a), _vp(b), float(null), int(min_cov), _vp(rho), _vp(ll), _vp(used), _lib.PHZ_HOST))
    return rho, ll, used


def betabinom_test(lib, handle, a, b, null, rho, min_cov: int = 8) -> np.ndarray:
    """phz_betabinom_test on [rows, columns] matrices with one rho per column -> p-values in the shape of `a` (NaN where not tested, and in a column whose rho is NaN)"""
    a = np.ascontiguousarray(a, dtype=np.int32); b = np.ascontiguousarray(b, dtype=np.int32)
    assert a.ndim == 2 and a.shape == b.shape
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    assert rho.shape == (a.shape[1],)
    p = np.empty(a.shape, dtype=np.float64)
    _check(lib, handle, lib.phz_betabinom_test(handle, a.shape[0], a.shape[1], _vp(a), _vp(b), float(null), _vp(rho), int(min_cov), _vp(p), _lib.PHZ_HOST))
    return p


def rho_max(null: float) -> float:
    """the largest overdispersion at which alpha, beta >= 1 (the pmf stays unimodal): m / (1 + m), m = min(null, 1 - null)"""
    m = min(null, 1.0 - null)
    return m / (1.0 + m)


def _overdispersion(value, null: float):
    """0 | "auto" | RHO, as given to --overdispersion or to ae_test() -> None (the binomial path), "auto" or a float inside the domain"""
    if isinstance(value, str) and value.strip().lower() == "auto":
        return "auto"
    try:
        rho = float(value)
    except (TypeError, ValueError):
        rho = float("nan")
    if rho == 0.0:
        return None
    if not (_lib.PHZ_BB_RHO_MIN <= rho <= rho_max(null)):
        raise FatalError("FATAL ERROR - --overdispersion must be 0, auto or a number in [%g, %.6g] (the upper bound is m / (1 + m), m = min(null, 1 - null))"
                         % (_lib.PHZ_BB_RHO_MIN, rho_max(null)))
    return rho


def _betabinom_pvalues(ctx, a, b, null, min_cov, mode):
    """mode "auto": one fitted rho per column; a float: that rho everywhere -> (p-values, rho per column with NaN where the column has no tested cell)"""
    if mode == "auto":
        rho, _, used = betabinom_fit(ctx.lib, ctx.h, a, b, null, min_cov)
    else:
        rho = np.full(a.shape[1], mode, dtype=np.float64)
    p = betabinom_test(ctx.lib, ctx.h, a, b, null, rho, min_cov)
    if mode != "auto":
        rho = np.where(np.isnan(p).all(axis=0), np.nan, rho)
    return p, rho


def _summary(samples, pvalue, qvalue, n_tested, fdr, rho):
    out = ["\t".join(base.SUMMARY_HEADER + ["rho"]) + "\n"]
    sig = (qvalue <= fdr).sum(axis=0) if qvalue.size else np.zeros(len(samples), dtype=np.int64)
    for j, s in enumerate(samples):
        smallest = np.nanmin(pvalue[:, j]) if n_tested[j] else float("nan")
        out.append("%s\t%d\t%d\t%s\t%s\n" % (s, int(n_tested[j]), int(sig[j]), _fmt(smallest), _fmt(float(rho[j]))))
    return "".join(out)


def _record_times(ctx, stats, mode):
    if hasattr(ctx, "timing"):
        stats["k_bbfit_ms"] = ctx.timing(_lib.PHZ_T_BBFIT)[0] if mode == "auto" else 0.0
        stats["k_bbtest_ms"] = ctx.timing(_lib.PHZ_T_BBTEST)[0]; stats["k_bh_ms"] = ctx.timing(_lib.PHZ_T_BH)[0]


def ae_test(bed_text, null: float = 0.5, min_cov: int = 8, fdr: float = 0.05, threads: int = 1, ctx=None, stats: Optional[dict] = None,
            overdispersion=0) -> dict:
    """phaser_amd.ae_test.ae_test with overdispersion: 0 (that function itself), "auto" (beta-binomial null, one fitted rho per sample) or a rho for every
    sample -> {"pvalue": bytes, "qvalue": bytes, "significant": str, "summary": str}, the summary with a rho column when the option is on"""
    _check_options(null, fdr)
    mode = _overdispersion(overdispersion, null)
    if mode is None:
        return base.ae_test(bed_text, null, min_cov, fdr, threads, ctx, stats)
    if ctx is None:
        ctx = _lib.Context(0)                          # raises without a GPU: there is no CPU path
    text = bed_text.encode() if isinstance(bed_text, str) else bytes(bed_text)
    t0 = time.perf_counter()
    mx = Matrix(text, threads)
    t1 = time.perf_counter()
    pvalue, rho = _betabinom_pvalues(ctx, mx.a, mx.b, null, min_cov, mode)
    t2 = time.perf_counter()
    qvalue, n_tested = bh_adjust(ctx.lib, ctx.h, pvalue)
    t3 = time.perf_counter()
    out = {"pvalue": mx.rows_text(pvalue, threads), "qvalue": mx.rows_text(qvalue, threads)}
    t4 = time.perf_counter()
    with np.errstate(invalid="ignore"):
        rr, cc = np.nonzero(qvalue <= fdr)             # row order, then column order
    names = mx.names()
    sig = ["\t".join(base.SIGNIFICANT_HEADER) + "\n"]
    for r, c, a, b, p, q in zip(rr.tolist(), cc.tolist(), mx.a[rr, cc].tolist(), mx.b[rr, cc].tolist(), pvalue[rr, cc].tolist(), qvalue[rr, cc].tolist()):
        sig.append("%s\t%s\t%d\t%d\t%s\t%s\t%s\n" % (names[r], mx.samples[c], a, b, _fmt(log2_afc(a, b)), _fmt(p), _fmt(q)))
    out["significant"] = "".join(sig)
    out["summary"] = _summary(mx.samples, pvalue, qvalue, n_tested, fdr, rho)
    if stats is not None:
        stats.update({"genes": int(mx.a.shape[0]), "samples": len(mx.samples), "tested": int(n_tested.sum()), "significant": int(len(rr)),
                      "seconds": {"parse": round(t1 - t0, 3), "betabinom": round(t2 - t1, 3), "bh": round(t3 - t2, 3), "matrix_text": round(t4 - t3, 3),
                                  "lists": round(time.perf_counter() - t4, 3)}})
        _record_times(ctx, stats, mode)
    return out


def ae_test_gene_ae(table_text: str, null: float = 0.5, min_cov: int = 8, fdr: float = 0.05, ctx=None, stats: Optional[dict] = None, overdispersion=0) -> str:
    """phaser_amd.ae_test.ae_test_gene_ae with overdispersion (see ae_test): a sample is a `bam` value, a rho column follows qvalue when the option is on"""
    _check_options(null, fdr)
    mode = _overdispersion(overdispersion, null)
    if mode is None:
        return base.ae_test_gene_ae(table_text, null, min_cov, fdr, ctx, stats)
    if ctx is None:
        ctx = _lib.Context(0)
    lines = [l.rstrip("\r") for l in table_text.split("\n")]
    lines = [l for l in lines if l]
    if not lines:
        raise FatalError("FATAL ERROR - the gene_ae table is empty")
    head = lines[0].split("\t")
    for k in ("aCount", "bCount", "bam"):
        if k not in head:
            raise FatalError("FATAL ERROR - the gene_ae table has no %s column" % k)
    ia, ib, ibam = head.index("aCount"), head.index("bCount"), head.index("bam")
    rows = [l.split("\t") for l in lines[1:]]
    n = len(rows)
    a = np.full(n, -1, dtype=np.int32); b = np.full(n, -1, dtype=np.int32)
    col = np.zeros(n, dtype=np.int64); rank = np.zeros(n, dtype=np.int64)
    bams: dict = {}
    seen = []
    for i, r in enumerate(rows):
        try:
            x, y = int(r[ia]), int(r[ib])
            if 0 <= x and 0 <= y and x + y < 2 ** 31:
                a[i], b[i] = x, y
        except (ValueError, IndexError):
            pass
        name = r[ibam] if ibam < len(r) else ""
        j = bams.setdefault(name, len(bams))
        if j == len(seen):
            seen.append(0)
        col[i] = j; rank[i] = seen[j]; seen[j] += 1
    # one column per `bam` value, rows in the order of the table; the cells no row fills are untested
    shape = (max(seen) if seen else 0, len(bams))
    am = np.full(shape, -1, dtype=np.int32); bm = np.full(shape, -1, dtype=np.int32)
    am[rank, col] = a; bm[rank, col] = b
    pm, rho = _betabinom_pvalues(ctx, am, bm, null, min_cov, mode)
    qm, _ = bh_adjust(ctx.lib, ctx.h, pm)
    p = pm[rank, col] if n else np.zeros(0)
    q = qm[rank, col] if n else np.zeros(0)
    out = ["\t".join(head + ["pvalue", "qvalue", "rho"]) + "\n"]
    for l, pv, qv, j in zip(lines[1:], p.tolist(), q.tolist(), col.tolist()):
        out.append("%s\t%s\t%s\t%s\n" % (l, _fmt(pv), _fmt(qv), _fmt(float(rho[j]))))
    if stats is not None:
        with np.errstate(invalid="ignore"):
            stats.update({"rows": n, "samples": len(bams), "tested": int((~np.isnan(p)).sum()), "significant": int((q <= fdr).sum())})
        _record_times(ctx, stats, mode)
    return "".join(out)


def _banner():
    print(""); print("##################################################")
    print("        Welcome to phaser_ae_test (phaser_amd, MI355X)")
    print("##################################################"); print("")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--bed", type=str); src.add_argument("--gene_ae", type=str)
    ap.add_argument("--o", type=str, required=True)
    ap.add_argument("--null", type=float, default=0.5); ap.add_argument("--min_cov", type=int, default=8)
    ap.add_argument("--fdr", type=float, default=0.05); ap.add_argument("--t", type=int, default=1)
    ap.add_argument("--overdispersion", type=str, default="0", help="0: binomial null; auto: beta-binomial null, one rho fitted per sample; RHO: that rho for every sample")
    args = ap.parse_args(argv)
    # the same command line without this module's option, for phaser_amd.ae_test's own main (repr of a float reads back as the same float)
    plain = (["--bed", args.bed] if args.bed is not None else ["--gene_ae", args.gene_ae]) + \
            ["--o", args.o, "--null", repr(args.null), "--min_cov", str(args.min_cov), "--fdr", repr(args.fdr), "--t", str(args.t)]
    try:
        _check_options(args.null, args.fdr)
    except FatalError:
        return base.main(plain)                            # its line, its status
    try:
        mode = _overdispersion(args.overdispersion, args.null)
    except FatalError as e:
        _banner()
        print(str(e))
        return 1
    if mode is None:
        return base.main(plain)                            # the binomial path: that tool itself
    _banner()
    stats: dict = {}
    try:
        if args.gene_ae:
            print("#1 Loading gene_ae table...")
            table = read_text(args.gene_ae)
            print("#2 Testing allelic imbalance...")
            body = ae_test_gene_ae(table, args.null, args.min_cov, args.fdr, stats=stats, overdispersion=mode)
            with open(args.o + ".txt", "w") as f:
                f.write(body)
            print("     %d rows of %d sample(s): %d tested, %d with q <= %g" % (stats["rows"], stats["samples"], stats["tested"], stats["significant"], args.fdr))
            print("     K_bbfit %.3f ms, K_bbtest %.3f ms" % (stats.get("k_bbfit_ms", float("nan")), stats.get("k_bbtest_ms", float("nan"))))
            return 0
        print("#1 Loading expression matrix...")
        with open(args.bed, "rb") as f:
            raw = f.read()
        if ".gz" in args.bed:                              # plain gzip and BGZF alike, as cis_var.read_text
            import gzip
            raw = gzip.decompress(raw)
        print("#2 Testing allelic imbalance...")
        out = ae_test(raw, args.null, args.min_cov, args.fdr, threads=args.t, stats=stats, overdispersion=mode)
    except FatalError as e:
        print(str(e))
        return 1
    from . import vcfout
    print("#3 Saving p-value and q-value matrices...")
    for kind in ("pvalue", "qvalue"):
        path = "%s.%s.bed.gz" % (args.o, kind)
        vcfout.write_bgzf(path, out[kind], args.t)
        if not vcfout.tabix_index(path, "bed", args.t):
            print("WARNING - %s is not position-sorted, no tabix index written (tabix refuses such files too)" % path)
    with open(args.o + ".significant.txt", "w") as f:
        f.write(out["significant"])
    with open(args.o + ".summary.txt", "w") as f:
        f.write(out["summary"])
    print("     %d genes x %d samples: %d cells tested, %d with q <= %g" % (stats["genes"], stats["samples"], stats["tested"], stats["significant"], args.fdr))
    print("     seconds %s; K_bbfit %.3f ms, K_bbtest %.3f ms, K_bh %.3f ms" % (stats["seconds"], stats.get("k_bbfit_ms", float("nan")),
                                                                               stats.get("k_bbtest_ms", float("nan")), stats.get("k_bh_ms", float("nan"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
