"""phaser_ae_diff: allelic imbalance compared between two conditions of the same individuals -- two tissues, treated against untreated, two time points
(no counterpart in the reference: what its users do next in R, fisher.test per cell and mantelhaen.test per gene).

    python -m phaser_amd.ae_diff --bed1 cond1.bed.gz --bed2 cond2.bed.gz --o out [--min_cov 8 --min_samples 2 --correct 1 --fdr 0.05 --t N]

Both inputs are aCount|bCount matrices as phaser_expr_matrix writes them (plain, gzip or BGZF).  Genes are matched by column 4, samples by header name; the
intersection is used, in the row and column order of --bed1.  Every cell [[a1, b1], [a2, b2]] with a1 + b1 and a2 + b2 both >= max(min_cov, 1) gets Fisher's
exact two-sided test and every sample Benjamini-Hochberg q-values; every gene gets the Cochran-Mantel-Haenszel test over its samples (the strata), with the
Mantel-Haenszel common odds ratio, and the genes' p-values get q-values as one column.  Pipeline:
  phz_aematrix_parse (libphz.so, host threads)   either matrix text -> row-major a / b arrays, the byte range of every row's four leading columns
  numpy                                          the aligned int32 matrices
  phz_fisher_test    (HIP, K_fisher)             one lane per cell (one wave per cell above PHZ_FISHER_WAVE_N in a build that sets it)
  phz_bh_adjust      (HIP, K_bh)                 per sample
  phz_cmh_test       (HIP, K_cmh)                one wave per gene
  phz_bh_adjust      (HIP, K_bh)                 the genes' p-values, one column
  phz_aetest_rows    (libphz.so, host threads)   the p-value, q-value and delta matrices as text (%.6g, NA where not tested)
Writes <o>.pvalue.bed.gz, <o>.qvalue.bed.gz and <o>.delta.bed.gz (BGZF, tabix index when position-sorted; delta = log2((a1 + .5)(b2 + .5) / ((b1 + .5)(a2 + .5)))
per tested cell), <o>.cells.txt (one row per cell with q <= --fdr, row then column order), <o>.genes.txt (one row per gene) and <o>.summary.txt (per sample:
tested cells, significant cells, smallest p; a last line for the gene test).
There is no CPU path: without a GPU the run raises.  Two runs on the same input write identical bytes.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
import time
from typing import Optional

import numpy as np

from . import _lib
from .ae_test import FatalError, Matrix, _check, _fmt, _vp, bh_adjust

CELLS_HEADER = ["gene", "sample", "a1", "b1", "a2", "b2", "delta_log2_aFC", "pvalue", "qvalue"]
GENES_HEADER = ["gene", "n_strata", "log2_or", "cmh_stat", "pvalue", "qvalue"]
SUMMARY_HEADER = ["sample", "tested", "significant", "min_pvalue"]
GENE_TEST_ROW = "#cmh_genes"          # the summary's last line: the gene test


def _matrices(*ms):
    out = [np.ascontiguousarray(m, dtype=np.int32) for m in ms]
    assert all(m.ndim == 2 and m.shape == out[0].shape for m in out)
    return out


def fisher_test(lib, handle, a1, b1, a2, b2, min_cov: int = 8) -> np.ndarray:
    """phz_fisher_test on [rows, columns] matrices -> p-values in their shape (NaN where not tested)"""
    a1, b1, a2, b2 = _matrices(a1, b1, a2, b2)
    p = np.empty(a1.shape, dtype=np.float64)
    _check(lib, handle, lib.phz_fisher_test(handle, a1.shape[0], a1.shape[1], _vp(a1), _vp(b1), _vp(a2), _vp(b2), int(min_cov), _vp(p), _lib.PHZ_HOST))
    return p


def cmh_test(lib, handle, a1, b1, a2, b2, min_cov: int = 8, min_samples: int = 2, correct: int = 1):
    """phz_cmh_test on [rows, columns] matrices -> (stat, pvalue, log2_or, n_strata), one value per row"""
    a1, b1, a2, b2 = _matrices(a1, b1, a2, b2)
    rows = a1.shape[0]
    stat = np.empty(rows, dtype=np.float64); p = np.empty(rows, dtype=np.float64); lor = np.empty(rows, dtype=np.float64); ns = np.empty(rows, dtype=np.int32)
    _check(lib, handle, lib.phz_cmh_test(handle, rows, a1.shape[1], _vp(a1), _vp(b1), _vp(a2), _vp(b2), int(min_cov), int(min_samples), int(correct), _vp(stat), _vp(p),
                                         _vp(lor), _vp(ns), _lib.PHZ_HOST))
    return stat, p, lor, ns


def _unique_index(names, what, which):
    index = {}
    for i, n in enumerate(names):
        if n == "":                                    # a row without a fourth column: it has no name to match
            continue
        if n in index:
            raise FatalError("FATAL ERROR - %s %s occurs twice in %s" % (what, n, which))
        index[n] = i
    return index


def align(m1: Matrix, m2: Matrix):
    """-> (rows of m1, rows of m2, columns of m1, columns of m2, names of the kept genes) of the genes and samples both have, in m1's order"""
    g1, g2 = m1.names(), m2.names()
    _unique_index(g1, "gene", "--bed1"); _unique_index(m1.samples, "sample", "--bed1")
    gi = _unique_index(g2, "gene", "--bed2"); si = _unique_index(m2.samples, "sample", "--bed2")
    rows = [i for i, g in enumerate(g1) if g in gi]; cols = [j for j, s in enumerate(m1.samples) if s in si]
    if not rows:
        raise FatalError("FATAL ERROR - --bed1 and --bed2 have no gene in common")
    if not cols:
        raise FatalError("FATAL ERROR - --bed1 and --bed2 have no sample in common")
    return (np.array(rows, dtype=np.int64), np.array([gi[g1[i]] for i in rows], dtype=np.int64),
            np.array(cols, dtype=np.int64), np.array([si[m1.samples[j]] for j in cols], dtype=np.int64), [g1[i] for i in rows])


def _submatrix(m: Matrix, rows, cols, a) -> Matrix:
    """the rows and columns of m that are kept, as a Matrix over the same text: what rows_text needs"""
    sub = Matrix.__new__(Matrix)
    sub.text = m.text
    sub.a = a; sub.b = a
    sub.lead_off = np.ascontiguousarray(m.lead_off[rows]); sub.lead_len = np.ascontiguousarray(m.lead_len[rows])
    sub.samples = [m.samples[j] for j in cols.tolist()]
    sub.header = "\t".join(m.header.split("\t")[:4] + sub.samples)
    return sub


def _check_options(fdr: float):
    if not (0.0 <= fdr <= 1.0):
        raise FatalError("FATAL ERROR - --fdr must lie between 0 and 1")


def ae_diff(bed1_text, bed2_text, min_cov: int = 8, min_samples: int = 2, correct: int = 1, fdr: float = 0.05, threads: int = 1, ctx=None,
            stats: Optional[dict] = None) -> dict:
    """The tool on the texts of the two matrices -> {"pvalue", "qvalue", "delta": bytes (the matrices before compression), "cells", "genes", "summary": str}.
    ctx: anything with .lib and .h (a _lib.Context; made here when None, which raises without a GPU)."""
    _check_options(fdr)
    if ctx is None:
        ctx = _lib.Context(0)                          # raises without a GPU: there is no CPU path
    t0 = time.perf_counter()
    m1 = Matrix(bed1_text.encode() if isinstance(bed1_text, str) else bytes(bed1_text), threads)
    m2 = Matrix(bed2_text.encode() if isinstance(bed2_text, str) else bytes(bed2_text), threads)
    t1 = time.perf_counter()
    r1, r2, c1, c2, genes = align(m1, m2)
    a1 = np.ascontiguousarray(m1.a[np.ix_(r1, c1)]); b1 = np.ascontiguousarray(m1.b[np.ix_(r1, c1)])
    a2 = np.ascontiguousarray(m2.a[np.ix_(r2, c2)]); b2 = np.ascontiguousarray(m2.b[np.ix_(r2, c2)])
    mx = _submatrix(m1, r1, c1, a1)
    t2 = time.perf_counter()
    pvalue = fisher_test(ctx.lib, ctx.h, a1, b1, a2, b2, min_cov)
    t3 = time.perf_counter()
    qvalue, n_tested = bh_adjust(ctx.lib, ctx.h, pvalue)
    t4 = time.perf_counter()
    stat, gene_p, log2_or, n_strata = cmh_test(ctx.lib, ctx.h, a1, b1, a2, b2, min_cov, min_samples, correct)
    gene_q, gene_tested = bh_adjust(ctx.lib, ctx.h, gene_p.reshape(-1, 1))
    gene_q = gene_q[:, 0]
    t5 = time.perf_counter()
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.log2((a1 + .5) * (b2 + .5) / ((b1 + .5) * (a2 + .5)))
    delta[np.isnan(pvalue)] = np.nan
    out = {"pvalue": mx.rows_text(pvalue, threads), "qvalue": mx.rows_text(qvalue, threads), "delta": mx.rows_text(delta, threads)}
    t6 = time.perf_counter()
    with np.errstate(invalid="ignore"):
        rr, cc = np.nonzero(qvalue <= fdr)             # row order, then column order
    cells = ["\t".join(CELLS_HEADER) + "\n"]
    for r, c, w, x, y, z, d, p, q in zip(rr.tolist(), cc.tolist(), a1[rr, cc].tolist(), b1[rr, cc].tolist(), a2[rr, cc].tolist(), b2[rr, cc].tolist(),
                                         delta[rr, cc].tolist(), pvalue[rr, cc].tolist(), qvalue[rr, cc].tolist()):
        cells.append("%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n" % (genes[r], mx.samples[c], w, x, y, z, _fmt(d), _fmt(p), _fmt(q)))
    out["cells"] = "".join(cells)
    rows = ["\t".join(GENES_HEADER) + "\n"]
    for g, k, lor, s, p, q in zip(genes, n_strata.tolist(), log2_or.tolist(), stat.tolist(), gene_p.tolist(), gene_q.tolist()):
        rows.append("%s\t%d\t%s\t%s\t%s\t%s\n" % (g, k, _fmt(lor), _fmt(s), _fmt(p), _fmt(q)))
    out["genes"] = "".join(rows)
    summ = ["\t".join(SUMMARY_HEADER) + "\n"]
    with np.errstate(invalid="ignore"):
        sig = (qvalue <= fdr).sum(axis=0); gene_sig = int((gene_q <= fdr).sum())
    for j, s in enumerate(mx.samples):
        summ.append("%s\t%d\t%d\t%s\n" % (s, int(n_tested[j]), int(sig[j]), _fmt(np.nanmin(pvalue[:, j]) if n_tested[j] else float("nan"))))
    summ.append("%s\t%d\t%d\t%s\n" % (GENE_TEST_ROW, int(gene_tested[0]), gene_sig, _fmt(np.nanmin(gene_p) if gene_tested[0] else float("nan"))))
    out["summary"] = "".join(summ)
    if stats is not None:
        stats.update({"genes": len(genes), "samples": len(mx.samples), "dropped_genes": int(m1.a.shape[0] - len(genes)), "dropped_samples": int(len(m1.samples) - len(mx.samples)),
                      "tested": int(n_tested.sum()), "significant": int(len(rr)), "genes_tested": int(gene_tested[0]), "genes_significant": gene_sig,
                      "seconds": {"parse": round(t1 - t0, 3), "align": round(t2 - t1, 3), "fisher": round(t3 - t2, 3), "bh": round(t4 - t3, 3), "cmh_bh": round(t5 - t4, 3),
                                  "matrix_text": round(t6 - t5, 3), "lists": round(time.perf_counter() - t6, 3)}})
        if hasattr(ctx, "timing"):
            stats["k_fisher_ms"] = ctx.timing(_lib.PHZ_T_FISHER)[0]; stats["k_cmh_ms"] = ctx.timing(_lib.PHZ_T_CMH)[0]; stats["k_bh_ms"] = ctx.timing(_lib.PHZ_T_BH)[1]
    return out


def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":                             # plain gzip and BGZF alike
        import gzip
        raw = gzip.decompress(raw)
    return raw


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bed1", type=str, required=True); ap.add_argument("--bed2", type=str, required=True); ap.add_argument("--o", type=str, required=True)
    ap.add_argument("--min_cov", type=int, default=8); ap.add_argument("--min_samples", type=int, default=2); ap.add_argument("--correct", type=int, default=1)
    ap.add_argument("--fdr", type=float, default=0.05); ap.add_argument("--t", type=int, default=1)
    args = ap.parse_args(argv)
    print(""); print("##################################################")
    print("        Welcome to phaser_ae_diff (phaser_amd, MI355X)")
    print("##################################################"); print("")
    stats: dict = {}
    try:
        _check_options(args.fdr)
        print("#1 Loading expression matrices...")
        raw1, raw2 = _read(args.bed1), _read(args.bed2)
        print("#2 Testing differential allelic imbalance...")
        out = ae_diff(raw1, raw2, args.min_cov, args.min_samples, args.correct, args.fdr, threads=args.t, stats=stats)
    except FatalError as e:
        print(str(e))
        return 1
    from . import vcfout
    print("     %d gene(s) and %d sample(s) of --bed1 are not in --bed2: dropped" % (stats["dropped_genes"], stats["dropped_samples"]))
    print("#3 Saving p-value, q-value and delta matrices...")
    for kind in ("pvalue", "qvalue", "delta"):
        path = "%s.%s.bed.gz" % (args.o, kind)
        vcfout.write_bgzf(path, out[kind], args.t)
        if not vcfout.tabix_index(path, "bed", args.t):
            print("WARNING - %s is not position-sorted, no tabix index written (tabix refuses such files too)" % path)
    for kind in ("cells", "genes", "summary"):
        with open("%s.%s.txt" % (args.o, kind), "w") as f:
            f.write(out[kind])
    print("     %d genes x %d samples: %d cells tested, %d with q <= %g; %d genes tested, %d with q <= %g" %
          (stats["genes"], stats["samples"], stats["tested"], stats["significant"], args.fdr, stats["genes_tested"], stats["genes_significant"], args.fdr))
    print("     seconds %s; K_fisher %.3f ms, K_cmh %.3f ms, K_bh %.3f ms" % (stats["seconds"], stats.get("k_fisher_ms", float("nan")), stats.get("k_cmh_ms", float("nan")),
                                                                             stats.get("k_bh_ms", float("nan"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
