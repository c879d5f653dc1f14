"""phaser_pop/phaser_cis_var.py on the GPU: per eQTL (variant, gene) pair, the allelic fold change (aFC) of the gene's phased
expression in the variant's heterozygotes and homozygotes, with 95 % bootstrap CIs.

Same command line (`--bed --vcf --pairs --map --o [--pc --min_cov --chr --bs --ignore_v --t]`) plus `--seed`, same 28 output
columns.  Pipeline:
  sample map, pairs, expression matrix   (Python)     map / pairs TSV, the wanted rows of the gene x sample matrix (:45-90)
  VCF lookup                             (native)     phz_bgzf_read, then every record at a pair's (contig, position) (:276-284)
  per-sample aFCs                        (numpy)      GT classes, min_cov, log((a+pc)/(b+pc), 2) (:137-159)
  bootstrap                              (HIP, K_boot) every replicate median and the CI order statistics of every group (:166-171)
  point estimates, rank-sum p, output    (numpy)      numpy.median, ranksums, DataFrame.to_csv text (:161-178, :93-101)
There is no CPU path: without a GPU `_lib.Context(0)` raises.  `_bootstrap=` replaces the K_boot launch in the CPU tests.

Deliberate differences from the reference (each pinned by a test in tests/test_cis_var.py):
  * resamples: the reference draws from an unseeded numpy.random, so its CI and p columns change on every run; here replicate b of a
    group draws from a Philox4x32-10 stream keyed by --seed (the stream contract is in phaser_amd/csrc/phz_cisvar.hip): the same
    estimator, one deterministic realisation, independent of --t.
  * the signed and the |aFC| set of a group share their resamples (the reference draws them independently; every column is a
    marginal, so no distribution changes).
  * sample order is map-file order (the reference iterates a Python 2 dict).
  * several matching records of one pair are reported in VCF record order (the reference sorts them with pandas' unstable sort).
  * inputs the reference crashes on: an empty matrix cell of a mapped sample -> the sample is skipped; a gene twice in the matrix
    -> FATAL ERROR (status 1); a pair's contig absent from the VCF -> no row, counted in the log; --pc 0 with a zero count -> FATAL
    ERROR (status 1); a GT whose only "1" is part of an allele such as 0|10 -> the sample is skipped.
  * --ignore_v 1 strips the pairs' gene ids but the matrix filter compares the versioned column 4 (the reference strips column 2,
    :79): reproduced, not repaired.
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import math
import sys
import time
from typing import Callable, Dict, List, Optional

import numpy as np

from . import _lib

COLUMNS = ["gene", "var_id", "var_chr", "var_pos", "var_het_n", "var_hom_n", "het_hom_pvalue", "var_het_afc_lower", "var_het_afc",
           "var_het_afc_upper", "var_het_pval", "var_het_abs_afc_lower", "var_het_abs_afc", "var_het_abs_afc_upper", "var_hom_afc_lower",
           "var_hom_afc", "var_hom_afc_upper", "var_hom_abs_afc_lower", "var_hom_abs_afc", "var_hom_abs_afc_upper", "var_het_afcs",
           "var_hom_afcs", "var_het_ref_counts", "var_het_alt_counts", "var_hom_hap1_counts", "var_hom_hap2_counts", "var_het_sample_ids",
           "var_hom_sample_ids"]
NO_DATA = "     ERROR: no phASER data read from input... check that chromsome naming is correct."


class FatalError(Exception):
    pass


# ---------------------------------------------------------------------------------------------------------------- inputs
def _tsv(text: str):
    lines = [l for l in text.split("\n") if l.strip("\r")]
    head = lines[0].rstrip("\r").split("\t") if lines else []
    return head, [l.rstrip("\r").split("\t") for l in lines[1:]]


def read_map(text: str):
    """-> [(vcf_sample, bed_sample)] in map-file order (a dict: a repeated vcf_sample keeps its first place and its last value)."""
    head, rows = _tsv(text)
    iv, ib = head.index("vcf_sample"), head.index("bed_sample")
    d: Dict[str, str] = {}
    for r in rows:
        d[r[iv]] = r[ib]
    return list(d.items())


def read_pairs(text: str, ignore_v: int = 0, chrom: str = ""):
    """-> list of dicts with xindex = 0-based data-row number (kept through the --chr filter)."""
    head, rows = _tsv(text)
    col = {k: head.index(k) for k in ("gene_id", "var_id", "var_contig", "var_pos", "var_ref", "var_alt")}
    out = []
    for i, r in enumerate(rows):
        r = r + [""] * (len(head) - len(r))
        p = {k: r[j] for k, j in col.items()}
        p["xindex"] = i
        if ignore_v == 1:
            p["gene_id"] = p["gene_id"].split(".")[0]
        if chrom != "" and p["var_contig"] != chrom:
            continue
        p["var_pos"] = int(float(p["var_pos"]))
        out.append(p)
    return out


def read_text(path: str) -> str:
    if ".gz" in path:                                  # the reference's test (:66): gzip.open reads plain gzip and BGZF alike
        with gzip.open(path, "rt") as f:
            return f.read()
    with open(path) as f:
        return f.read()


def read_matrix(text: str, genes: set, ignore_v: int = 0, chrom: str = ""):
    """The matrix rows the pairs need (:62-90): header + rows whose column 4 is a wanted gene (versioned column, see the module
    docstring), restricted to contig `chrom` when given (`tabix -h bed chr:`).  -> (sample columns, {gene key: [row fields]})"""
    header = None
    rows: Dict[str, list] = {}
    dup = set()
    for line in text.split("\n"):
        line = line.rstrip()
        if not line:
            continue
        c = line.split("\t")
        if line.startswith("#"):
            if header is None:
                header = c
                continue
        elif chrom != "" and c[0] != chrom:
            continue
        if header is None:
            header = c
            continue
        if len(c) > 3 and c[3] in genes:
            key = c[3].split(".")[0] if ignore_v == 1 else c[3]
            if key in rows:
                dup.add(key)
            rows[key] = c
    return (header or []), rows, dup


def _cell_counts(cells: List[str]):
    """'a|b' cells -> (a, b) float64 arrays; NaN where the cell is empty or not two numbers."""
    a = np.full(len(cells), np.nan); b = np.full(len(cells), np.nan)
    arr = np.array(cells, dtype=str) if cells else np.zeros(0, dtype=str)
    if not len(arr):
        return a, b
    parts = np.char.partition(arr, "|")
    ok = (parts[:, 1] == "|") & (parts[:, 0] != "") & (parts[:, 2] != "") & (np.char.find(parts[:, 2], "|") < 0)
    if ok.any():
        a[ok] = parts[ok, 0].astype(np.float64); b[ok] = parts[ok, 2].astype(np.float64)
    return a, b


# ---------------------------------------------------------------------------------------------------------------- VCF lookup
def vcf_records(path: str, wanted: list, samples: List[str], threads: int = 1, use_index: bool = True):
    """Every record with (CHROM, POS) in `wanted` (what tabix fetch(chr, pos-1, pos) + the POS filter return, :276-284), in file
    order, through phz_vcf_lookup: with <path>.tbi only the index's chunks of those positions are inflated, otherwise the whole file.
    -> ({(chrom, pos): [[CHROM, POS, ID, REF, ALT, gt_index, GT of each sample...]]}, contigs of the VCF); a sample the VCF or the
    record lacks has GT "\x01", gt_index is -1 when FORMAT has no GT"""
    lib = _lib.load()
    keys = list(wanted)
    cb = [c.encode() for c, _ in keys]; sb = [x.encode() for x in samples]
    carr = (C.c_char_p * max(1, len(cb)))(*cb); sarr = (C.c_char_p * max(1, len(sb)))(*sb)
    parr = np.ascontiguousarray([p for _, p in keys] or [0], dtype=np.int64)
    optr = C.c_void_p(); olen = C.c_int64(0); cptr = C.c_void_p(); clen = C.c_int64(0)
    st = lib.phz_vcf_lookup(path.encode(), len(keys), carr, C.c_void_p(parr.ctypes.data), len(sb), sarr, int(bool(use_index)), max(1, int(threads)),
                            C.byref(optr), C.byref(olen), C.byref(cptr), C.byref(clen))
    if st != _lib.PHZ_OK:
        raise _lib.PhzError(st, "phz_vcf_lookup(%s) failed" % path)
    try:
        text = C.string_at(optr, olen.value).decode(); ctext = C.string_at(cptr, clen.value).decode()
    finally:
        lib.phz_buf_free(optr); lib.phz_buf_free(cptr)
    out: Dict[tuple, list] = {}
    for line in text.split("\n"):
        if line:
            f = line.split("\t")
            out.setdefault(keys[int(f[0])], []).append(f[1:])
    return out, set(ctext.split("\n")) - {""}


def _classify(gt: str):
    """GT text -> (class, alt_index): 0 skip, 1 het, 2 hom, with the reference's substring tests (:146-159)."""
    if "|" not in gt:
        return 0, 0
    if "0" in gt and "1" in gt:
        f = gt.split("|")
        if "1" not in f:
            return 0, 0                               # e.g. 0|10: the reference's .index("1") raises
        ai = f.index("1")
        return (1, ai) if ai <= 1 else (0, 0)
    if gt.count("0") == 2 or gt.count("1") == 2:
        return 2, 0
    return 0, 0


class _GtClasses(dict):
    """GT text -> code = phased | class << 1 | alt_index << 3, computed once per distinct GT"""

    def __missing__(self, gt):
        c, ai = _classify(gt)
        v = self[gt] = int("|" in gt) | (c << 1) | (ai << 3)
        return v


# ---------------------------------------------------------------------------------------------------------------- statistics
def quantile_positions(bs: int, q: float):
    """numpy.percentile(reps, q) with the default 'linear' method reads sorted positions (prev, next) and lerps with gamma
    (numpy/lib/_function_base_impl.py: _quantile, _get_indexes, _get_gamma): -> (prev, next, gamma)"""
    vi = np.asanyarray((bs - 1) * np.true_divide(q, 100))
    prev = np.floor(vi)
    if vi >= bs - 1:
        prev = np.float64(-1)
        return bs - 1, bs - 1, np.asanyarray(vi - prev)
    return int(prev), int(prev) + 1, np.asanyarray(vi - prev)


def lerp(a, b, t):
    """numpy's _lerp: a + (b - a) * t, or b - (b - a) * (1 - t) where t >= 0.5"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    d = np.subtract(b, a)
    r = np.add(a, d * t)
    return np.where(t >= 0.5, np.subtract(b, d * (1 - t)), r)


def ranksums_p(x_vals, x_row, y_vals, y_row, n_rows):
    """scipy.stats.ranksums(x, y).pvalue for every row at once: average ranks of the pooled values, z of the x rank sum,
    2 * ndtr(-|z|); NaN where a side is empty."""
    from scipy.special import ndtr
    v = np.concatenate([x_vals, y_vals]).astype(np.float64)
    row = np.concatenate([x_row, y_row]).astype(np.int64)
    isx = np.concatenate([np.ones(len(x_vals), bool), np.zeros(len(y_vals), bool)])
    n1 = np.bincount(x_row, minlength=n_rows).astype(np.int64); n2 = np.bincount(y_row, minlength=n_rows).astype(np.int64)
    out = np.full(n_rows, np.nan)
    if not len(v):
        return out
    o = np.lexsort((v, row))
    vs, rs = v[o], row[o]
    start = np.searchsorted(rs, np.arange(n_rows), side="left")
    pos = np.arange(len(v)) - start[rs] + 1                          # 1-based position inside the row
    newrun = np.r_[True, (vs[1:] != vs[:-1]) | (rs[1:] != rs[:-1])]
    run = np.cumsum(newrun) - 1
    first = pos[newrun]
    run_len = np.bincount(run)
    last = first + run_len - 1
    rank = 0.5 * (first + last).astype(np.float64)
    r = np.empty(len(v)); r[o] = rank[run]
    s = np.bincount(row[isx], weights=r[isx], minlength=n_rows)
    ok = (n1 > 0) & (n2 > 0)
    expected = n1 * (n1 + n2 + 1) / 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (s - expected) / np.sqrt(n1 * n2 * (n1 + n2 + 1) / 12.0)
        p = 2 * ndtr(-np.abs(z))
    out[ok] = p[ok]
    return out


class BootInput:
    """Groups in the layout of phz_boot_in: values in list order, per-sample ranks, the sorted sets."""

    def __init__(self, values: np.ndarray, off: np.ndarray, subseq: np.ndarray, seed: int, bs: int):
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        self.subseq = np.ascontiguousarray(subseq, dtype=np.uint64)
        self.seed = int(seed); self.bs = int(bs)
        ng = len(self.off) - 1
        sizes = np.diff(self.off)
        self.max_n = int(sizes.max()) if ng else 0
        if self.max_n > 65535:
            raise FatalError("FATAL ERROR - a group holds %d samples; at most 65535 are supported" % self.max_n)
        grp = np.repeat(np.arange(ng), sizes)
        local = np.arange(len(self.values)) - self.off[:-1][grp]
        self.rank = np.zeros(len(self.values), dtype=np.uint32)
        self.sorted_s = np.empty(len(self.values)); self.sorted_a = np.empty(len(self.values))
        for which, dst in ((0, self.sorted_s), (1, self.sorted_a)):
            v = self.values if which == 0 else np.abs(self.values)
            o = np.lexsort((v, grp))                                  # by group, then value
            dst[:] = v[o]
            r = np.empty(len(v), dtype=np.uint32); r[o] = local.astype(np.uint32)      # sorted position i holds rank i - off[group]
            self.rank |= r << np.uint32(16 * which)
        self.k = [0, 0, 0, 0]
        lo_p, lo_n, self.gamma_lo = quantile_positions(self.bs, 2.5)
        hi_p, hi_n, self.gamma_hi = quantile_positions(self.bs, 97.5)
        self.k = [lo_p, lo_n, hi_p, hi_n]

    @property
    def n_groups(self):
        return len(self.off) - 1

    def struct(self):
        s = _lib.phz_boot_in()
        vp = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None
        s.n_groups = self.n_groups; s.off = vp(self.off); s.subseq = vp(self.subseq); s.rank = vp(self.rank)
        s.sorted_s = vp(self.sorted_s); s.sorted_a = vp(self.sorted_a); s.max_n = self.max_n; s.bs = self.bs
        for i in range(4):
            s.k[i] = int(self.k[i])
        s.seed = self.seed
        return s


def bootstrap_gpu(lib, handle, bi: BootInput, want_replicates: bool = False):
    """phz_bootstrap_medians -> (order_stats [G, 2, 4], sign_counts [G, 2, 2], replicates [G, 2, bs] or None)"""
    G = bi.n_groups
    os_ = np.zeros((G, 2, 4)); sc = np.zeros((G, 2, 2), dtype=np.int64)
    reps = np.zeros((G, 2, bi.bs)) if want_replicates else None
    if G == 0:
        return os_, sc, reps
    s = bi.struct()
    st = lib.phz_bootstrap_medians(handle, C.byref(s), C.c_void_p(os_.ctypes.data), C.c_void_p(sc.ctypes.data),
                                   C.c_void_p(reps.ctypes.data) if reps is not None else None, _lib.PHZ_HOST)
    if st != _lib.PHZ_OK:
        raise _lib.PhzError(st, (lib.phz_last_error(handle) or b"").decode())
    return os_, sc, reps


def _median_sorted(sorted_vals, off):
    """numpy.median of every group from its sorted values (the mean of the middle one or two)"""
    n = np.diff(off)
    out = np.full(len(n), np.nan)
    ok = n > 0
    i1 = off[:-1] + (n - 1) // 2; i2 = off[:-1] + n // 2
    a = sorted_vals[np.where(ok, i1, 0)] if len(sorted_vals) else np.zeros(len(n))
    b = sorted_vals[np.where(ok, i2, 0)] if len(sorted_vals) else np.zeros(len(n))
    odd = (n % 2) == 1
    out[ok & odd] = a[ok & odd]
    out[ok & ~odd] = ((a + b) / 2.0)[ok & ~odd]
    return out


# ---------------------------------------------------------------------------------------------------------------- run
def _fmt_float(x) -> str:
    return "" if x != x else repr(float(x))


def cis_var(bed_text: str, vcf_path: str, pairs_text: str, map_text: str, pc: int = 1, min_cov: int = 8, chrom: str = "",
            bs: int = 10000, ignore_v: int = 0, threads: int = 1, seed: int = 0, log: Optional[Callable[[str], None]] = None,
            stats: Optional[dict] = None, ctx: Optional[_lib.Context] = None, _bootstrap=None) -> Optional[str]:
    """-> output text, or None when no matrix row was read (the reference prints NO_DATA and writes nothing).
    _bootstrap: test hook replacing the K_boot launch, called as _bootstrap(BootInput) -> (order_stats, sign_counts)."""
    log = log or (lambda s: None)
    if bs < 1:
        raise FatalError("FATAL ERROR - --bs must be at least 1")
    if ctx is None and _bootstrap is None:
        ctx = _lib.Context(0)                          # raises without a GPU: there is no CPU path
    t0 = time.perf_counter()
    smap = read_map(map_text)
    pairs = read_pairs(pairs_text, ignore_v, chrom)
    genes = {p["gene_id"] for p in pairs}
    header, mrows, dup = read_matrix(bed_text, genes, ignore_v, chrom)
    if not mrows:
        log(NO_DATA)
        return None
    log("#4 Measuring allelic expression...")
    t1 = time.perf_counter()
    bed_col = {}
    for j, h in enumerate(header):
        bed_col.setdefault(h, j)
    # mapped samples in map order; their matrix column (or -1)
    vcf_names = [s for s, _ in smap]
    mcol = np.array([bed_col.get(b, -1) for _, b in smap], dtype=np.int64)
    S = len(smap)
    # ---- VCF records of the pairs whose gene has a matrix row
    live = [p for p in pairs if p["gene_id"] in mrows]
    for p in live:
        if p["gene_id"] in dup:
            raise FatalError("FATAL ERROR - gene %s appears more than once in the expression matrix" % p["gene_id"])
    recs, contigs = vcf_records(vcf_path, sorted({(p["var_contig"], p["var_pos"]) for p in live}), vcf_names, threads)
    missing_contig = sum(1 for p in live if p["var_contig"] not in contigs)
    if missing_contig:
        log("     %d pair(s) name a contig that the VCF does not hold: no row" % missing_contig)
    t2 = time.perf_counter()
    # ---- per (pair, record): the het and hom sample lists
    gene_counts: Dict[str, tuple] = {}
    classes = _GtClasses()
    classes["\x01"] = 0                                # a sample the VCF or the record lacks
    rows = []             # (pair, gene row name)
    grp_idx: List[np.ndarray] = []          # per row: [het sample indices, hom sample indices] in map order
    alt_of: List[np.ndarray] = []
    pending_afc = []
    for p in live:
        rl = recs.get((p["var_contig"], p["var_pos"]), [])
        mr = mrows[p["gene_id"]]
        if p["gene_id"] not in gene_counts:
            cells = [(mr[j] if 0 <= j < len(mr) else "") for j in mcol.tolist()]
            a, b = _cell_counts(cells)
            a[mcol < 0] = np.nan; b[mcol < 0] = np.nan
            gene_counts[p["gene_id"]] = (a, b)
        a, b = gene_counts[p["gene_id"]]
        for ordinal, rec in enumerate(rl):
            ref_ok = p["var_ref"] != "" and p["var_alt"] != "" and rec[3] == p["var_ref"] and rec[4] == p["var_alt"]
            if not (ref_ok or rec[2] == p["var_id"]):
                continue
            if rec[5] == "-1":
                raise FatalError("FATAL ERROR - VCF record %s:%s has no GT field" % (rec[0], rec[1]))
            gts = rec[6:]
            code = np.fromiter(map(classes.__getitem__, gts), dtype=np.int8, count=S) if S else np.zeros(0, np.int8)
            present = ~np.isnan(a)
            phased = present & ((code & 1) == 1)
            cls = (code >> 1) & 3; alt = code >> 3
            covered = phased & (a + b >= min_cov)
            pending_afc.append(covered)
            het = np.nonzero(covered & (cls == 1))[0]; hom = np.nonzero(covered & (cls == 2))[0]
            rows.append((p, mr[3] if len(mr) > 3 else "", ordinal, p["gene_id"]))
            grp_idx.append((het, hom)); alt_of.append(alt)
    t3 = time.perf_counter()
    # ---- aFCs: math.log((a+pc)/(b+pc), 2) of every distinct count pair (bit-exact with CPython's math.log), once per gene
    afc_tab: Dict[tuple, float] = {}
    gene_afc: Dict[str, np.ndarray] = {}
    for gkey, (a, b) in gene_counts.items():
        ok = ~np.isnan(a)
        v = np.full(len(a), np.nan)
        if ok.any():
            num = a[ok] + pc; den = b[ok] + pc
            uq, inv = np.unique(np.stack([num, den], axis=1), axis=0, return_inverse=True)
            vals = np.empty(len(uq))
            for i, (x, y) in enumerate(uq.tolist()):
                if (x, y) not in afc_tab:
                    afc_tab[(x, y)] = math.log(x / y, 2) if x > 0 and y > 0 else math.nan
                vals[i] = afc_tab[(x, y)]
            v[ok] = vals[np.asarray(inv).reshape(-1)]
        gene_afc[gkey] = v
    for (p, name, ordinal, gkey), cov in zip(rows, pending_afc):
        bad = cov & np.isnan(gene_afc[gkey])
        if bad.any():
            a, b = gene_counts[gkey]
            i = int(np.nonzero(bad)[0][0])
            raise FatalError("FATAL ERROR - a haplotype count of 0 with --pc %d: log(%r / %r) is undefined" % (pc, float(a[i] + pc), float(b[i] + pc)))
    R = len(rows)
    het_vals = []; hom_vals = []; het_off = [0]; hom_off = [0]
    row_lists = []
    for r, ((p, name, ordinal, gkey), (het, hom), alt) in enumerate(zip(rows, grp_idx, alt_of)):
        a, b = gene_counts[gkey]
        av = gene_afc[gkey]
        hv = av[het]
        hv = np.where(alt[het] == 1, np.negative(hv), hv).tolist()
        mv = av[hom].tolist()
        het_vals.extend(hv); hom_vals.extend(mv)
        het_off.append(len(het_vals)); hom_off.append(len(hom_vals))
        ai = alt[het].astype(np.int64)
        cnt = np.stack([a[het], b[het]], axis=1) if len(het) else np.zeros((0, 2))
        ref_c = cnt[np.arange(len(het)), 1 - ai].astype(np.int64) if len(het) else np.zeros(0, np.int64)
        alt_c = cnt[np.arange(len(het)), ai].astype(np.int64) if len(het) else np.zeros(0, np.int64)
        row_lists.append((",".join(map(str, hv)), ",".join(map(str, mv)), ",".join(map(str, ref_c.tolist())), ",".join(map(str, alt_c.tolist())),
                          ",".join(map(str, a[hom].astype(np.int64).tolist())), ",".join(map(str, b[hom].astype(np.int64).tolist())),
                          ",".join(vcf_names[i] for i in het.tolist()), ",".join(vcf_names[i] for i in hom.tolist())))
    het_off = np.asarray(het_off, dtype=np.int64); hom_off = np.asarray(hom_off, dtype=np.int64)
    # ---- groups: row r -> group 2r (het), 2r + 1 (hom)
    values = np.empty(len(het_vals) + len(hom_vals))
    sizes = np.empty(2 * R, dtype=np.int64)
    sizes[0::2] = np.diff(het_off); sizes[1::2] = np.diff(hom_off)
    off = np.zeros(2 * R + 1, dtype=np.int64); np.cumsum(sizes, out=off[1:])
    hv_a = np.asarray(het_vals, dtype=np.float64); mv_a = np.asarray(hom_vals, dtype=np.float64)
    gsrc = np.repeat(np.arange(2 * R), sizes)
    if len(values):
        pos_in = np.arange(len(values)) - off[:-1][gsrc]
        is_het = (gsrc % 2) == 0
        values[is_het] = hv_a[het_off[:-1][gsrc[is_het] // 2] + pos_in[is_het]]
        values[~is_het] = mv_a[hom_off[:-1][gsrc[~is_het] // 2] + pos_in[~is_het]]
    subseq = np.array([(p["xindex"] << 16) + ordinal * 2 + h for (p, _, ordinal, _) in rows for h in (0, 1)], dtype=np.uint64)
    # only non-empty groups go to the kernel
    nz = np.nonzero(sizes > 0)[0]
    sel_off = np.zeros(len(nz) + 1, dtype=np.int64); np.cumsum(sizes[nz], out=sel_off[1:])
    sel_vals = np.concatenate([values[off[g]:off[g + 1]] for g in nz]) if len(nz) else np.zeros(0)
    bi = BootInput(sel_vals, sel_off, subseq[nz] if len(nz) else np.zeros(0, np.uint64), seed, bs)
    t4 = time.perf_counter()
    if _bootstrap is not None:
        os_nz, sc_nz = _bootstrap(bi)[:2]
    else:
        os_nz, sc_nz, _ = bootstrap_gpu(ctx.lib, ctx.h, bi)
        if stats is not None:
            stats["k_boot_ms"] = ctx.timing(_lib.PHZ_T_BOOT)[0]
    t5 = time.perf_counter()
    order_stats = np.full((2 * R, 2, 4), np.nan); signs = np.zeros((2 * R, 2, 2), dtype=np.int64)
    order_stats[nz] = os_nz; signs[nz] = sc_nz
    lo = lerp(order_stats[:, :, 0], order_stats[:, :, 1], bi.gamma_lo)
    hi = lerp(order_stats[:, :, 2], order_stats[:, :, 3], bi.gamma_hi)
    point = np.full((2 * R, 2), np.nan)
    point[nz, 0] = _median_sorted(bi.sorted_s, bi.off); point[nz, 1] = _median_sorted(bi.sorted_a, bi.off)
    with np.errstate(invalid="ignore"):
        pval = np.minimum(signs[:, 0, 0], signs[:, 0, 1]).astype(np.float64) / float(bs) * 2
    pval[sizes == 0] = np.nan
    het_rows = np.repeat(np.arange(R), np.diff(het_off)); hom_rows = np.repeat(np.arange(R), np.diff(hom_off))
    rs_p = ranksums_p(np.abs(hv_a), het_rows, np.abs(mv_a), hom_rows, R)
    out = ["\t".join(COLUMNS) + "\n"]
    for r, (p, name, ordinal, gkey) in enumerate(rows):
        h, m = 2 * r, 2 * r + 1
        f = [name, p["var_id"], p["var_contig"], str(p["var_pos"]), str(int(sizes[h])), str(int(sizes[m])), _fmt_float(rs_p[r]),
             _fmt_float(lo[h, 0]), _fmt_float(point[h, 0]), _fmt_float(hi[h, 0]), _fmt_float(pval[h]),
             _fmt_float(lo[h, 1]), _fmt_float(point[h, 1]), _fmt_float(hi[h, 1]),
             _fmt_float(lo[m, 0]), _fmt_float(point[m, 0]), _fmt_float(hi[m, 0]),
             _fmt_float(lo[m, 1]), _fmt_float(point[m, 1]), _fmt_float(hi[m, 1])] + list(row_lists[r])
        out.append("\t".join(f) + "\n")
    if stats is not None:
        stats.update({"rows": R, "groups": int(len(nz)), "draws": int(sizes.sum()) * bs, "samples": S,
                      "seconds": {"inputs": round(t1 - t0, 3), "vcf": round(t2 - t1, 3), "samples": round(t3 - t2, 3), "groups": round(t4 - t3, 3),
                                  "bootstrap": round(t5 - t4, 3), "format": round(time.perf_counter() - t5, 3)}})
    return "".join(out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bed", type=str, required=True); ap.add_argument("--vcf", type=str, required=True)
    ap.add_argument("--pairs", type=str, required=True); ap.add_argument("--map", type=str, required=True)
    ap.add_argument("--o", type=str, required=True)
    ap.add_argument("--pc", default=1, type=int); ap.add_argument("--min_cov", type=int, default=8)
    ap.add_argument("--chr", type=str, default=""); ap.add_argument("--bs", type=int, default=10000)
    ap.add_argument("--ignore_v", type=int, default=0); ap.add_argument("--t", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    print(""); print("##################################################")
    print("          Welcome to phASER-POP v0.1.0 (phaser_amd, MI355X)")
    print("##################################################"); print("")
    print("     bootstrap seed %d" % args.seed)
    print("#1 Loading sample map...")
    map_text = open(args.map).read()
    print("#2 Loading variant gene pairs...")
    pairs_text = open(args.pairs).read()
    print("#3 Loading phASER BED...")
    if args.chr != "":
        print("     subsetting chr %s from input BED..." % args.chr)
    bed_text = read_text(args.bed)
    try:
        body = cis_var(bed_text, args.vcf, pairs_text, map_text, pc=args.pc, min_cov=args.min_cov, chrom=args.chr, bs=args.bs,
                       ignore_v=args.ignore_v, threads=args.t, seed=args.seed, log=print)
    except FatalError as e:
        print(str(e))
        return 1
    if body is None:
        return 0
    with open(args.o, "w") as f:
        f.write(body)
    return 0


if __name__ == "__main__":
    sys.exit(main())
