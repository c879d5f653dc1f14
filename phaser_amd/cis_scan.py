"""phaser_cis_scan: ASE-based cis mapping on the gw-phased population matrix (no counterpart in the reference, whose phaser_cis_var only measures pairs the user
already knows).  For each gene, every VCF variant within --window of it is tested for "the gene's |aFC| is larger in the variant's heterozygotes than in its
homozygotes" (the rank-sum test that is cis_var's het_hom_pvalue), the best variant is reported, and a permutation p-value accounts for having looked at all of them.

    python -m phaser_amd.cis_scan --bed M.gw_phased.bed.gz --vcf POP.vcf.gz --map map.txt --o OUT
                                  [--window 100000 --min_cov 8 --pc 1 --min_het 5 --min_hom 5 --perm 1000 --seed 0 --chr C --fdr 0.05 --output_pairs 0 --t N]

Samples, coverage and aFC follow phaser_amd.cis_var: map-file order, a sample is covered for a gene when its cell parses and a + b >= --min_cov,
aFC = log2((a + pc) / (b + pc)); --pc 0 with a zero count is a FATAL ERROR.  A gene's variants are the VCF records of its contig with
start + 1 - window <= POS <= stop + window; the class of (variant, sample) is cis_var's (het, hom or skipped; unphased and missing genotypes are skipped).
Pipeline:
  matrix                 (native)   phz_aematrix_parse, as phaser_amd.ae_test
  classes of the windows (native)   phz_vcf_region_classes: the gene windows merged per contig, read through the .tbi index when there is one
  orders and tie runs    (numpy)    per gene the covered samples by ascending |aFC|
  scan                   (HIP)      phz_cis_scan (K_cisscan), one call per contig: n_het, n_hom and the rank-sum count of every pair, the best variant of every
                                    gene, and in how many of --perm permutations of the gene's samples the best statistic is reached
  z, p, q, output        (numpy)    cis_var.ranksums_p's expressions on the integers; BH over the genes through phz_bh_adjust
There is no CPU path: without a GPU the run raises.  Two runs on the same input write identical bytes; --seed changes only the permutation columns.  Outputs:
  <o>.genes.txt        one row per gene (GENES_HEADER); NA where the gene has no testable pair, and in the permutation columns with --perm 0
  <o>.significant.txt  the rows with q <= --fdr
  <o>.summary.txt      counts
  <o>.pairs.txt.gz     with --output_pairs 1: every testable pair (PAIRS_HEADER)
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
from .ae_test import Matrix, _check, _vp, bh_adjust
from .cis_var import FatalError, read_map

GENES_HEADER = ["gene", "contig", "start", "stop", "n_covered", "n_tested", "var_id", "var_pos", "var_het_n", "var_hom_n", "z", "het_hom_pvalue", "var_het_afc",
                "perm_exceed", "perm_p", "q"]
PAIRS_HEADER = ["gene", "var_id", "var_pos", "n_het", "n_hom", "z", "het_hom_pvalue"]


def _fmt(x) -> str:
    return "NA" if x != x else repr(float(x))


def check_options(window, min_cov, pc, min_het, min_hom, perm, fdr):
    if window < 0:
        raise FatalError("FATAL ERROR - --window must not be negative")
    if min_het < 1 or min_hom < 1:
        raise FatalError("FATAL ERROR - --min_het and --min_hom must be at least 1")
    if perm < 0 or perm > 2 ** 31 - 2:
        raise FatalError("FATAL ERROR - --perm must lie between 0 and 2^31 - 2")
    if pc < 0 or min_cov < 0:
        raise FatalError("FATAL ERROR - --pc and --min_cov must not be negative")
    if not (0.0 <= fdr <= 1.0):
        raise FatalError("FATAL ERROR - --fdr must lie between 0 and 1")


# ---------------------------------------------------------------------------------------------------------------- VCF
def region_classes(path: str, regions, samples, threads: int = 1, use_index: bool = True):
    """phz_vcf_region_classes: every record inside a region (contig, lo, hi; 1-based, inclusive), once, in file order
    -> ([(CHROM, POS, ID, REF, ALT, gt_index)], codes uint8 [records, samples] = class | alt-on-haplotype-2 << 2, contigs of the VCF)"""
    lib = _lib.load()
    cb = [str(c).encode() for c, _, _ in regions]; sb = [x.encode() for x in samples]
    carr = (C.c_char_p * max(1, len(cb)))(*cb); sarr = (C.c_char_p * max(1, len(sb)))(*sb)
    lo = np.ascontiguousarray([r[1] for r in regions] or [0], dtype=np.int64); hi = np.ascontiguousarray([r[2] for r in regions] or [0], dtype=np.int64)
    optr = C.c_void_p(); olen = C.c_int64(0); cptr = C.c_void_p(); clen = C.c_int64(0)
    st = lib.phz_vcf_region_classes(path.encode(), len(cb), carr, _vp(lo), _vp(hi), len(sb), sarr, int(bool(use_index)), max(1, int(threads)),
                                    C.byref(optr), C.byref(olen), C.byref(cptr), C.byref(clen))
    if st != _lib.PHZ_OK:
        raise _lib.PhzError(st, "phz_vcf_region_classes(%s) failed" % path)
    try:
        text = C.string_at(optr, olen.value); ctext = C.string_at(cptr, clen.value).decode()
    finally:
        lib.phz_buf_free(optr); lib.phz_buf_free(cptr)
    recs = []; rows = []
    for line in text.split(b"\n"):
        if line:
            f = line.split(b"\t")
            recs.append((f[0].decode(), int(f[1]), f[2].decode(), f[3].decode(), f[4].decode(), int(f[5])))
            rows.append(f[6])
    S = len(samples)
    codes = (np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), S) - 48) if rows and S else np.zeros((len(rows), S), dtype=np.uint8)
    return recs, codes, set(ctext.split("\n")) - {""}


def merge_windows(contigs, lo, hi):
    """gene windows -> [(contig, lo, hi)] merged per contig, contigs in order of first appearance"""
    per = {}
    for c, a, b in zip(contigs, lo, hi):
        per.setdefault(c, []).append((max(int(a), 1), int(b)))
    out = []
    for c, iv in per.items():
        iv.sort()
        cur = None
        for a, b in iv:
            if b < a:
                continue
            if cur is not None and a <= cur[1] + 1:
                cur[1] = max(cur[1], b)
            else:
                if cur is not None:
                    out.append((c, cur[0], cur[1]))
                cur = [a, b]
        if cur is not None:
            out.append((c, cur[0], cur[1]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the scan
class ScanInput:
    """The arrays of phz_cisscan_in for the genes of one call.  covered: bool [genes, samples]; absafc: |aFC| [genes, samples] (read where covered)."""

    def __init__(self, cls, covered, absafc, v_lo, v_hi, subseq, min_het, min_hom, n_perm, seed):
        self.cls = np.ascontiguousarray(cls, dtype=np.uint8)
        G, S = covered.shape
        assert self.cls.ndim == 2 and (self.cls.shape[1] == S or self.cls.shape[0] == 0)
        gi, si = np.nonzero(covered)                                    # row-major: ascending sample index inside a gene
        n = np.bincount(gi, minlength=G).astype(np.int64)
        self.g_off = np.zeros(G + 1, dtype=np.int64); np.cumsum(n, out=self.g_off[1:])
        vals = absafc[gi, si]
        o = np.lexsort((vals, gi))                                      # by gene, then |aFC| (stable)
        sv = vals[o]
        local = np.arange(len(gi), dtype=np.int64) - self.g_off[:-1][gi]
        newrun = np.ones(len(gi), dtype=bool)
        if len(gi) > 1:
            newrun[1:] = (sv[1:] != sv[:-1]) | (gi[1:] != gi[:-1])
        starts = np.nonzero(newrun)[0]
        run = np.cumsum(newrun) - 1
        ends = np.r_[starts[1:], len(gi)] - 1
        self.covered = si.astype(np.uint16)
        self.order = si[o].astype(np.uint16)
        self.run_first = (local[starts[run]] if len(gi) else local).astype(np.uint16)
        self.run_last = (local[ends[run]] if len(gi) else local).astype(np.uint16)
        self.v_lo = np.ascontiguousarray(v_lo, dtype=np.int64); self.v_hi = np.ascontiguousarray(v_hi, dtype=np.int64)
        self.subseq = np.ascontiguousarray(subseq, dtype=np.uint64)
        self.n_samples = S
        self.min_het, self.min_hom, self.n_perm, self.seed = int(min_het), int(min_hom), int(n_perm), int(seed)
        self.pair_off = np.zeros(G + 1, dtype=np.int64); np.cumsum(self.v_hi - self.v_lo, out=self.pair_off[1:])

    @property
    def n_genes(self):
        return len(self.g_off) - 1

    def struct(self):
        s = _lib.phz_cisscan_in()
        vp = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
        s.n_genes = self.n_genes; s.n_vars = self.cls.shape[0]; s.n_samples = self.n_samples
        s.cls = vp(self.cls); s.g_off = vp(self.g_off); s.covered = vp(self.covered); s.order = vp(self.order)
        s.run_first = vp(self.run_first); s.run_last = vp(self.run_last); s.v_lo = vp(self.v_lo); s.v_hi = vp(self.v_hi); s.subseq = vp(self.subseq)
        s.min_het = self.min_het; s.min_hom = self.min_hom; s.n_perm = self.n_perm; s.seed = self.seed & (2 ** 64 - 1)
        return s


def cis_scan_call(lib, handle, si: ScanInput):
    """phz_cis_scan -> (n_het, n_hom int32 [pairs], u2 int64 [pairs], best_v, exceed int32 [genes])"""
    P = int(si.pair_off[-1]); G = si.n_genes
    n_het = np.zeros(P, dtype=np.int32); n_hom = np.zeros(P, dtype=np.int32); u2 = np.zeros(P, dtype=np.int64)
    best_v = np.full(G, -1, dtype=np.int32); exceed = np.zeros(G, dtype=np.int32)
    s = si.struct()
    _check(lib, handle, lib.phz_cis_scan(handle, C.byref(s), _vp(n_het), _vp(n_hom), _vp(u2), _vp(best_v), _vp(exceed), _lib.PHZ_HOST))
    return n_het, n_hom, u2, best_v, exceed


def ranksum_z_p(u2, n1, n2):
    """z and p of the rank-sum test from the integers, in the expressions of cis_var.ranksums_p"""
    from scipy.special import ndtr
    n1 = np.asarray(n1, dtype=np.int64); n2 = np.asarray(n2, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = ((np.asarray(u2, dtype=np.int64) - n1 * n2) / 2.0) / np.sqrt(n1 * n2 * (n1 + n2 + 1) / 12.0)
        p = 2 * ndtr(-np.abs(z))
    return z, p


def _afc_matrix(a, b, pc):
    """math.log((a + pc) / (b + pc), 2) of every cell with both counts (bit-exact with cis_var); NaN elsewhere and where a count + pc is 0"""
    out = np.full(a.shape, np.nan)
    ok = (a >= 0) & (b >= 0)
    if ok.any():
        key = ((a[ok].astype(np.int64) + pc) << 32) | (b[ok].astype(np.int64) + pc)
        uq, inv = np.unique(key, return_inverse=True)
        vals = np.empty(len(uq))
        for i, k in enumerate(uq.tolist()):
            x, y = float(k >> 32), float(k & 0xFFFFFFFF)
            vals[i] = math.log(x / y, 2) if x > 0 and y > 0 else math.nan
        out[ok] = vals[inv]
    return out


def cis_scan(bed_text, vcf_path: str, map_text: str, window: int = 100000, min_cov: int = 8, pc: int = 1, min_het: int = 5, min_hom: int = 5, perm: int = 1000,
             seed: int = 0, chrom: str = "", fdr: float = 0.05, output_pairs: int = 0, threads: int = 1, ctx=None, stats: Optional[dict] = None,
             use_index: bool = True) -> dict:
    """The tool on the text of a matrix -> {"genes": str, "significant": str, "summary": str, "pairs": str or None}.
    ctx: anything with .lib and .h (a _lib.Context; made here when None, which raises without a GPU)."""
    check_options(window, min_cov, pc, min_het, min_hom, perm, fdr)
    if ctx is None:
        ctx = _lib.Context(0)                          # raises without a GPU: there is no CPU path
    text = bed_text.encode() if isinstance(bed_text, str) else bytes(bed_text)
    t0 = time.perf_counter()
    smap = read_map(map_text)
    S = len(smap)
    if S == 0:
        raise FatalError("FATAL ERROR - the sample map holds no sample")
    if S > _lib.PHZ_CISSCAN_MAX_S:
        raise FatalError("FATAL ERROR - the map holds %d samples; at most %d are supported" % (S, _lib.PHZ_CISSCAN_MAX_S))
    mx = Matrix(text, threads)
    head = mx.header.split("\t")
    col_of = {}
    for j, h in enumerate(head):
        col_of.setdefault(h, j)
    mcol = np.array([col_of.get(b, -1) - 4 for _, b in smap], dtype=np.int64)
    lead = [text[o:o + n].decode().split("\t") for o, n in zip(mx.lead_off.tolist(), mx.lead_len.tolist())]
    rows = [r for r, f in enumerate(lead) if len(f) >= 4 and (chrom == "" or f[0] == chrom)]
    try:
        g_start = np.array([int(lead[r][1]) for r in rows], dtype=np.int64); g_stop = np.array([int(lead[r][2]) for r in rows], dtype=np.int64)
    except ValueError:
        raise FatalError("FATAL ERROR - a matrix row has a start or stop that is not a number")
    g_contig = [lead[r][0] for r in rows]; g_name = [lead[r][3] for r in rows]
    G = len(rows)
    rsel = np.asarray(rows, dtype=np.int64)
    have = mcol >= 0
    a = np.full((G, S), -1, dtype=np.int32); b = np.full((G, S), -1, dtype=np.int32)
    if G and have.any():
        a[:, have] = mx.a[np.ix_(rsel, mcol[have])]; b[:, have] = mx.b[np.ix_(rsel, mcol[have])]
    covered = (a >= 0) & (b >= 0) & (a.astype(np.int64) + b >= min_cov)
    afc = _afc_matrix(a, b, pc)
    bad = covered & np.isnan(afc)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise FatalError("FATAL ERROR - a haplotype count of 0 with --pc %d: log(%r / %r) is undefined" % (pc, float(a[r, c] + pc), float(b[r, c] + pc)))
    absafc = np.abs(afc)
    t1 = time.perf_counter()
    # ---- the variants of the windows
    w_lo = g_start + 1 - window; w_hi = g_stop + window
    recs, codes, vcf_contigs = region_classes(vcf_path, merge_windows(g_contig, w_lo, w_hi), [s for s, _ in smap], threads, use_index)
    by_contig = {}
    for i, rec in enumerate(recs):
        by_contig.setdefault(rec[0], []).append(i)
    t2 = time.perf_counter()
    # ---- one call per contig
    n_cov = covered.sum(axis=1)
    n_tested = np.zeros(G, dtype=np.int64)
    best = np.full(G, -1, dtype=np.int64)              # record index of the best variant
    b_het = np.zeros(G, dtype=np.int64); b_hom = np.zeros(G, dtype=np.int64); b_u2 = np.zeros(G, dtype=np.int64)
    exceed = np.zeros(G, dtype=np.int64)
    pair_rows = []
    k_ms = 0.0; n_pairs = 0
    contig_genes = {}
    for g, c in enumerate(g_contig):
        contig_genes.setdefault(c, []).append(g)
    for c, gl in contig_genes.items():
        gs = np.asarray(gl, dtype=np.int64)
        ridx = np.asarray(by_contig.get(c, []), dtype=np.int64)
        pos = np.array([recs[i][1] for i in ridx.tolist()], dtype=np.int64)
        if len(pos) > 1 and np.any(pos[1:] < pos[:-1]):
            raise FatalError("FATAL ERROR - the VCF records of contig %s are not sorted by position" % c)
        v_lo = np.searchsorted(pos, w_lo[gs], side="left"); v_hi = np.searchsorted(pos, w_hi[gs], side="right")
        v_hi = np.maximum(v_hi, v_lo)
        si = ScanInput(codes[ridx] & 3 if len(ridx) else np.zeros((0, S), np.uint8), covered[gs], absafc[gs], v_lo, v_hi, rsel[gs].astype(np.uint64), min_het, min_hom,
                       perm, seed)
        nh, nm, u2, bv, ex = cis_scan_call(ctx.lib, ctx.h, si)
        if hasattr(ctx, "timing"):
            k_ms += ctx.timing(_lib.PHZ_T_CISSCAN)[0]
        n_pairs += len(nh)
        testable = (nh >= min_het) & (nm >= min_hom)
        pg = np.repeat(np.arange(len(gs)), si.v_hi - si.v_lo)
        n_tested[gs] = np.bincount(pg[testable], minlength=len(gs))
        ok = bv >= 0
        k = si.pair_off[:-1][ok] + (bv[ok] - si.v_lo[ok])
        best[gs[ok]] = ridx[bv[ok]]; b_het[gs[ok]] = nh[k]; b_hom[gs[ok]] = nm[k]; b_u2[gs[ok]] = u2[k]
        exceed[gs] = ex
        if output_pairs:
            kk = np.nonzero(testable)[0]
            pv = si.v_lo[pg[kk]] + (kk - si.pair_off[:-1][pg[kk]])
            pair_rows.append((gs[pg[kk]], ridx[pv], nh[kk].astype(np.int64), nm[kk].astype(np.int64), u2[kk]))
    t3 = time.perf_counter()
    # ---- statistics of the best pairs
    has = best >= 0
    z, p = ranksum_z_p(b_u2, b_het, b_hom)
    het_afc = np.full(G, np.nan)
    for g in np.nonzero(has)[0].tolist():
        code = codes[best[g]]
        het = covered[g] & ((code & 3) == 1)
        v = afc[g, het]
        v = np.sort(np.where((code[het] >> 2) == 1, np.negative(v), v), kind="stable")          # cis_var's median: the middle one or two of the stable order
        het_afc[g] = v[len(v) // 2] if len(v) % 2 else (v[len(v) // 2 - 1] + v[len(v) // 2]) / 2.0
    perm_p = np.full(G, np.nan)
    if perm > 0:
        perm_p[has] = (1.0 + exceed[has]) / (perm + 1.0)
    q = np.full(G, np.nan)
    if G and perm > 0:
        q = bh_adjust(ctx.lib, ctx.h, perm_p.reshape(G, 1))[0].reshape(G)
    t4 = time.perf_counter()

    def var_id(i):
        c, ps, vid, ref, alt, _ = recs[i]
        return "%s_%d_%s_%s" % (c, ps, ref, alt) if vid == "." else vid

    lines = ["\t".join(GENES_HEADER) + "\n"]; sig = ["\t".join(GENES_HEADER) + "\n"]
    for g in range(G):
        f = [g_name[g], g_contig[g], str(int(g_start[g])), str(int(g_stop[g])), str(int(n_cov[g])), str(int(n_tested[g]))]
        if has[g]:
            f += [var_id(int(best[g])), str(recs[int(best[g])][1]), str(int(b_het[g])), str(int(b_hom[g])), _fmt(z[g]), _fmt(p[g]), _fmt(het_afc[g])]
        else:
            f += ["NA"] * 7
        f += [str(int(exceed[g])), _fmt(perm_p[g]), _fmt(q[g])] if (has[g] and perm > 0) else ["NA"] * 3
        row = "\t".join(f) + "\n"
        lines.append(row)
        if q[g] <= fdr:
            sig.append(row)
    out = {"genes": "".join(lines), "significant": "".join(sig), "pairs": None}
    if output_pairs:
        pl = ["\t".join(PAIRS_HEADER) + "\n"]
        for gg, rr, nh, nm, u2 in pair_rows:
            zz, pp = ranksum_z_p(u2, nh, nm)
            for g, r, x, y, zv, pv in zip(gg.tolist(), rr.tolist(), nh.tolist(), nm.tolist(), zz.tolist(), pp.tolist()):
                pl.append("%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (g_name[g], var_id(r), recs[r][1], x, y, _fmt(zv), _fmt(pv)))
        out["pairs"] = "".join(pl)
    missing = sorted({c for c in g_contig if c not in vcf_contigs})
    out["summary"] = "".join("%s\t%s\n" % kv for kv in (
        ("genes", G), ("samples", S), ("variants", len(recs)), ("pairs", n_pairs), ("testable_pairs", int(n_tested.sum())), ("genes_tested", int(has.sum())),
        ("permutations", perm), ("seed", seed), ("fdr", repr(float(fdr))), ("significant", len(sig) - 1), ("contigs_absent_from_vcf", ",".join(missing) or "-")))
    if stats is not None:
        stats.update({"genes": G, "samples": S, "variants": len(recs), "pairs": n_pairs, "genes_tested": int(has.sum()), "significant": len(sig) - 1,
                      "k_cisscan_ms": k_ms,
                      "seconds": {"matrix": round(t1 - t0, 3), "vcf": round(t2 - t1, 3), "scan": round(t3 - t2, 3), "statistics": round(t4 - t3, 3),
                                  "format": round(time.perf_counter() - t4, 3)}})
    return out


def _banner():
    print(""); print("##################################################")
    print("        Welcome to phaser_cis_scan (phaser_amd, MI355X)")
    print("##################################################"); print("")


class _Parser(argparse.ArgumentParser):
    def error(self, message):                          # one line, status 1
        print("FATAL ERROR - %s" % message)
        sys.exit(1)


def main(argv=None) -> int:
    ap = _Parser()
    ap.add_argument("--bed", type=str, required=True); ap.add_argument("--vcf", type=str, required=True)
    ap.add_argument("--map", type=str, required=True); ap.add_argument("--o", type=str, required=True)
    ap.add_argument("--window", type=int, default=100000); ap.add_argument("--min_cov", type=int, default=8); ap.add_argument("--pc", type=int, default=1)
    ap.add_argument("--min_het", type=int, default=5); ap.add_argument("--min_hom", type=int, default=5)
    ap.add_argument("--perm", type=int, default=1000); ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--chr", type=str, default=""); ap.add_argument("--fdr", type=float, default=0.05)
    ap.add_argument("--output_pairs", type=int, default=0); ap.add_argument("--t", type=int, default=1)
    args = ap.parse_args(argv)
    stats: dict = {}
    try:
        check_options(args.window, args.min_cov, args.pc, args.min_het, args.min_hom, args.perm, args.fdr)
        _banner()
        print("#1 Loading sample map and expression matrix...")
        with open(args.map) as f:
            map_text = f.read()
        with open(args.bed, "rb") as f:
            raw = f.read()
        if ".gz" in args.bed:                              # plain gzip and BGZF alike, as cis_var.read_text
            import gzip
            raw = gzip.decompress(raw)
        print("#2 Scanning the cis windows (%d permutations, seed %d)..." % (args.perm, args.seed))
        out = cis_scan(raw, args.vcf, map_text, args.window, args.min_cov, args.pc, args.min_het, args.min_hom, args.perm, args.seed, args.chr, args.fdr,
                       args.output_pairs, threads=args.t, stats=stats)
    except FatalError as e:
        print(str(e))
        return 1
    print("#3 Saving results...")
    for kind in ("genes", "significant", "summary"):
        with open("%s.%s.txt" % (args.o, kind), "w") as f:
            f.write(out[kind])
    if out["pairs"] is not None:
        from . import vcfout
        vcfout.write_bgzf(args.o + ".pairs.txt.gz", out["pairs"].encode(), args.t)
    print("     %d genes x %d samples, %d variants, %d pairs: %d genes tested, %d with q <= %g" % (stats["genes"], stats["samples"], stats["variants"], stats["pairs"],
                                                                                               stats["genes_tested"], stats["significant"], args.fdr))
    print("     seconds %s; K_cisscan %.3f ms" % (stats["seconds"], stats["k_cisscan_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
