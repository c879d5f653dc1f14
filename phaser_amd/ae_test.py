"""phaser_ae_test: allelic-imbalance test of the aCount|bCount cells that phaser_gene_ae and phaser_expr_matrix write (no counterpart in the
reference: the step its users take next, in R or pandas, one scalar test per cell).

    python -m phaser_amd.ae_test --bed matrix.bed.gz --o out [--null 0.5 --min_cov 8 --fdr 0.05 --t 1]
    python -m phaser_amd.ae_test --gene_ae sample.gene_ae.txt --o out [...]

Every cell with aCount + bCount >= max(min_cov, 1) gets the exact two-sided binomial test of aCount out of aCount + bCount against --null
(scipy.stats.binomtest's rule), then the p-values of a sample get Benjamini-Hochberg q-values (scipy.stats.false_discovery_control).  Pipeline:
  phz_aematrix_parse (libphz.so, host threads)   matrix text -> row-major a / b arrays, the byte range of every row's four leading columns
  phz_binom_test     (HIP, K_binom)              one lane per cell
  phz_bh_adjust      (HIP, K_bh)                 per sample: compaction, two radix sorts, one workgroup walking the column from the top rank down
  phz_aetest_rows    (libphz.so, host threads)   the p-value and q-value matrices as text (%.6g, NA where not tested)
--bed writes <o>.pvalue.bed.gz and <o>.qvalue.bed.gz (BGZF, tabix index when position-sorted), <o>.significant.txt (one row per cell with q <= --fdr,
row then column order) and <o>.summary.txt (per sample: tested genes, significant genes, smallest p).  --gene_ae takes the table of one phaser_gene_ae
run: every `bam` value is one sample, the output <o>.txt is the table with pvalue and qvalue columns appended.
There is no CPU path: without a GPU the run raises.  Two runs on the same input write identical bytes.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import sys
import time
from typing import Optional

import numpy as np

from . import _lib
from .cis_var import FatalError, read_text

SIGNIFICANT_HEADER = ["gene", "sample", "aCount", "bCount", "log2_aFC", "pvalue", "qvalue"]
SUMMARY_HEADER = ["sample", "tested", "significant", "min_pvalue"]


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _check(lib, handle, st):
    if st != _lib.PHZ_OK:
        raise _lib.PhzError(st, (lib.phz_last_error(handle) or b"").decode() or lib.phz_strerror(st).decode())


def binom_test(lib, handle, a, b, null: float = 0.5, min_cov: int = 8) -> np.ndarray:
    """phz_binom_test -> p-values in the shape of `a` (NaN where not tested)"""
    a = np.ascontiguousarray(a, dtype=np.int32); b = np.ascontiguousarray(b, dtype=np.int32)
    p = np.empty(a.shape, dtype=np.float64)
    _check(lib, handle, lib.phz_binom_test(handle, a.size, _vp(a), _vp(b), float(null), int(min_cov), _vp(p), _lib.PHZ_HOST))
    return p


def bh_adjust(lib, handle, pvalue):
    """phz_bh_adjust on a [rows, columns] matrix -> (q-values, tested cells per column)"""
    p = np.ascontiguousarray(pvalue, dtype=np.float64)
    assert p.ndim == 2
    q = np.empty_like(p); nt = np.zeros(p.shape[1], dtype=np.int64)
    _check(lib, handle, lib.phz_bh_adjust(handle, p.shape[0], p.shape[1], _vp(p), _vp(q), _vp(nt), _lib.PHZ_HOST))
    return q, nt


class Matrix:
    """phz_aematrix_parse: header fields, a / b [rows, samples], the byte ranges of the rows' leading columns in `text`"""

    def __init__(self, text: bytes, threads: int = 1):
        lib = _lib.load()
        self.text = text
        buf = C.cast(C.c_char_p(text), C.c_void_p)
        nr, nc, hl = C.c_int64(), C.c_int64(), C.c_int64()
        st = lib.phz_aematrix_parse(buf, len(text), int(threads), C.byref(nr), C.byref(nc), C.byref(hl), None, None, None, None)
        if st != _lib.PHZ_OK:
            raise FatalError("FATAL ERROR - the expression matrix has no header line")
        R, S = nr.value, nc.value
        self.a = np.empty((R, S), dtype=np.int32); self.b = np.empty((R, S), dtype=np.int32)
        self.lead_off = np.empty(R, dtype=np.int64); self.lead_len = np.empty(R, dtype=np.int32)
        st = lib.phz_aematrix_parse(buf, len(text), int(threads), C.byref(nr), C.byref(nc), C.byref(hl), _vp(self.a), _vp(self.b), _vp(self.lead_off),
                                    _vp(self.lead_len))
        if st != _lib.PHZ_OK:
            raise _lib.PhzError(st, "phz_aematrix_parse failed")
        first = len(text) - len(text.lstrip(b"\r\n"))            # the header is the first non-empty line
        self.header = text[first:first + hl.value].decode()
        self.samples = self.header.split("\t")[4:]

    def names(self):
        """column 4 of every row"""
        t = self.text
        return [t[o:o + n].decode().split("\t")[3] if t[o:o + n].count(b"\t") >= 3 else "" for o, n in zip(self.lead_off.tolist(), self.lead_len.tolist())]

    def rows_text(self, values: np.ndarray, threads: int = 1) -> bytes:
        """phz_aetest_rows: header + one row per gene with `values` as %.6g / NA"""
        lib = _lib.load()
        v = np.ascontiguousarray(values, dtype=np.float64)
        assert v.shape == self.a.shape
        out = C.c_void_p(); n = C.c_int64()
        st = lib.phz_aetest_rows(C.cast(C.c_char_p(self.text), C.c_void_p), _vp(self.lead_off), _vp(self.lead_len), v.shape[0], v.shape[1], _vp(v), int(threads),
                                 C.byref(out), C.byref(n))
        if st != _lib.PHZ_OK:
            raise _lib.PhzError(st, "phz_aetest_rows failed")
        try:
            return self.header.encode() + b"\n" + C.string_at(out, n.value)
        finally:
            lib.phz_buf_free(out)


def log2_afc(a: int, b: int) -> float:
    """log2(a / b) with phaser_gene_ae's conventions: b = 0 -> inf, a = 0 -> -inf"""
    ratio = float("inf") if b == 0 else float(a) / float(b)
    return float("-inf") if ratio == 0 else math.log(ratio, 2)


def _fmt(x) -> str:
    return "NA" if x != x else "%.6g" % x


def _check_options(null: float, fdr: float):
    if not (0.0 < null < 1.0):
        raise FatalError("FATAL ERROR - --null must lie strictly between 0 and 1")
    if not (0.0 <= fdr <= 1.0):
        raise FatalError("FATAL ERROR - --fdr must lie between 0 and 1")


def _summary(samples, pvalue, qvalue, n_tested, fdr):
    out = ["\t".join(SUMMARY_HEADER) + "\n"]
    sig = (qvalue <= fdr).sum(axis=0) if qvalue.size else np.zeros(len(samples), dtype=np.int64)
    for j, s in enumerate(samples):
        col = pvalue[:, j]
        smallest = np.nanmin(col) if n_tested[j] else float("nan")
        out.append("%s\t%d\t%d\t%s\n" % (s, int(n_tested[j]), int(sig[j]), _fmt(smallest)))
    return "".join(out)


def ae_test(bed_text, null: float = 0.5, min_cov: int = 8, fdr: float = 0.05, threads: int = 1, ctx=None, stats: Optional[dict] = None) -> dict:
    """The --bed mode on the text of a matrix -> {"pvalue": bytes, "qvalue": bytes, "significant": str, "summary": str} (the two matrices before
    compression).  ctx: anything with .lib and .h (a _lib.Context; made here when None, which raises without a GPU)."""
    _check_options(null, fdr)
    if ctx is None:
        ctx = _lib.Context(0)                          # raises without a GPU: there is no CPU path
    text = bed_text.encode() if isinstance(bed_text, str) else bytes(bed_text)
    t0 = time.perf_counter()
    mx = Matrix(text, threads)
    t1 = time.perf_counter()
    pvalue = binom_test(ctx.lib, ctx.h, mx.a, mx.b, null, min_cov)
    t2 = time.perf_counter()
    qvalue, n_tested = bh_adjust(ctx.lib, ctx.h, pvalue)
    t3 = time.perf_counter()
    out = {"pvalue": mx.rows_text(pvalue, threads), "qvalue": mx.rows_text(qvalue, threads)}
    t4 = time.perf_counter()
    with np.errstate(invalid="ignore"):
        rr, cc = np.nonzero(qvalue <= fdr)             # row order, then column order
    names = mx.names()
    sig = ["\t".join(SIGNIFICANT_HEADER) + "\n"]
    for r, c, a, b, p, q in zip(rr.tolist(), cc.tolist(), mx.a[rr, cc].tolist(), mx.b[rr, cc].tolist(), pvalue[rr, cc].tolist(), qvalue[rr, cc].tolist()):
        sig.append("%s\t%s\t%d\t%d\t%s\t%s\t%s\n" % (names[r], mx.samples[c], a, b, _fmt(log2_afc(a, b)), _fmt(p), _fmt(q)))
    out["significant"] = "".join(sig)
    out["summary"] = _summary(mx.samples, pvalue, qvalue, n_tested, fdr)
    if stats is not None:
        stats.update({"genes": int(mx.a.shape[0]), "samples": len(mx.samples), "tested": int(n_tested.sum()), "significant": int(len(rr)),
                      "seconds": {"parse": round(t1 - t0, 3), "binom": round(t2 - t1, 3), "bh": round(t3 - t2, 3), "matrix_text": round(t4 - t3, 3),
                                  "lists": round(time.perf_counter() - t4, 3)}})
        if hasattr(ctx, "timing"):
            stats["k_binom_ms"] = ctx.timing(_lib.PHZ_T_BINOM)[0]; stats["k_bh_ms"] = ctx.timing(_lib.PHZ_T_BH)[0]
    return out


def ae_test_gene_ae(table_text: str, null: float = 0.5, min_cov: int = 8, fdr: float = 0.05, ctx=None, stats: Optional[dict] = None) -> str:
    """The --gene_ae mode: the table of one phaser_gene_ae run -> the same table with pvalue and qvalue columns (BH per `bam` value)."""
    _check_options(null, fdr)
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
    p = binom_test(ctx.lib, ctx.h, a, b, null, min_cov)
    pm = np.full((max(seen) if seen else 0, len(bams)), np.nan)
    pm[rank, col] = p
    qm, _ = bh_adjust(ctx.lib, ctx.h, pm)
    q = qm[rank, col] if n else np.zeros(0)
    out = ["\t".join(head + ["pvalue", "qvalue"]) + "\n"]
    for l, pv, qv in zip(lines[1:], p.tolist(), q.tolist()):
        out.append("%s\t%s\t%s\n" % (l, _fmt(pv), _fmt(qv)))
    if stats is not None:
        with np.errstate(invalid="ignore"):
            stats.update({"rows": n, "samples": len(bams), "tested": int((~np.isnan(p)).sum()), "significant": int((q <= fdr).sum())})
    return "".join(out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--bed", type=str); src.add_argument("--gene_ae", type=str)
    ap.add_argument("--o", type=str, required=True)
    ap.add_argument("--null", type=float, default=0.5); ap.add_argument("--min_cov", type=int, default=8)
    ap.add_argument("--fdr", type=float, default=0.05); ap.add_argument("--t", type=int, default=1)
    args = ap.parse_args(argv)
    print(""); print("##################################################")
    print("        Welcome to phaser_ae_test (phaser_amd, MI355X)")
    print("##################################################"); print("")
    stats: dict = {}
    try:
        _check_options(args.null, args.fdr)
        if args.gene_ae:
            print("#1 Loading gene_ae table...")
            table = read_text(args.gene_ae)
            print("#2 Testing allelic imbalance...")
            body = ae_test_gene_ae(table, args.null, args.min_cov, args.fdr, stats=stats)
            with open(args.o + ".txt", "w") as f:
                f.write(body)
            print("     %d rows of %d sample(s): %d tested, %d with q <= %g" % (stats["rows"], stats["samples"], stats["tested"], stats["significant"], args.fdr))
            return 0
        print("#1 Loading expression matrix...")
        with open(args.bed, "rb") as f:
            raw = f.read()
        if ".gz" in args.bed:                              # plain gzip and BGZF alike, as cis_var.read_text
            import gzip
            raw = gzip.decompress(raw)
        print("#2 Testing allelic imbalance...")
        out = ae_test(raw, args.null, args.min_cov, args.fdr, threads=args.t, stats=stats)
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
    print("     seconds %s; K_binom %.3f ms, K_bh %.3f ms" % (stats["seconds"], stats.get("k_binom_ms", float("nan")), stats.get("k_bh_ms", float("nan"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
