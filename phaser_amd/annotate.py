"""phaser_annotate/phaser_annotate.py on the GPU: for every gene, the pairs of a sample's annotated variant alleles with their cis / trans
configuration from the genome-wide phase (GT) and from the read-backed phase (PG + PI), i.e. the compound heterozygotes of a phased sample.

Same command line (`--geno_vcf --sample --cadd_file --o [--af_vcf --af_field --threads]`), same 16 output columns.  Pipeline:
  genotype VCF                      (Python)      the GW set from GT, the PG set from PG + PI (:56-114)
  CADD rows, allele frequencies     (native)      phz_tabix_lines: the index's chunks of the wanted positions, the wanted columns (:283-332, :249-281)
  per-gene entry lists              (Python)      a variant once per matching CADD row, annotation masks, list flags (:124-174)
  pair loops                        (HIP, K_annot) every ordered pair of a gene's entries, both passes, every allele combination (:344-403, :225-247, :426)
  rows                              (native)      phz_annot_rows: threaded text from the fixed-width records (:405-456)
There is no CPU path: without a GPU `_lib.Context(0)` raises.  `_interactions=` replaces the K_annot launch in the CPU tests.

Reproduced, not repaired: a variant that is eligible by GT keeps its GT alleles and block 0 in the read-backed table as well (:144-147); only a variant
that is eligible by PG alone carries its PG alleles and float(PI) block.

Deliberate differences from the reference (each pinned by a test in tests/test_annotate.py):
  * gene order is first appearance: the genes in the order the GW variants' gene lists name them, then the PG ones (the reference iterates a Python set).
  * a genotype that does not reduce to exactly two single-digit alleles (a haploid call, an allele index of 10 or more) is skipped and counted in a log
    line (the reference splits the genotype into characters and then raises IndexError, or pairs the wrong digits).
  * no `NA` gene among the annotations is no error (the reference's set.remove raises).
  * a missing --o or an unknown sample print the reference's message and give status 1 (the same, stated because nothing else is written then).
  * an AF list shorter than the alt index (or not a number) gives `.`.
  * `.gz` inputs are read as text (the reference opens them in binary mode, which fails under Python 3).
  * a contig that the CADD table or the AF VCF does not hold gives no annotation / AF 0 (pysam raises).
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import sys
import time
from typing import Callable, Dict, List, Optional

import numpy as np

from . import _lib

COLUMNS = ["ensg", "name", "variant_a", "rsid_a", "allele_a", "af_a", "cadd_phred_a", "cadd_effect_a", "variant_b", "rsid_b", "allele_b", "af_b",
           "cadd_phred_b", "cadd_effect_b", "configuration", "read_backed"]
CADD_COLS = [0, 1, 4, 10, 92, 95, -1]          # Chrom, Pos, Alt, Consequence, GeneID, GeneName, PHRED (vfields[1], [4], [10], [92], [95], [-1], :307-331)
AF_COLS = [1, 4, 7]                            # POS, ALT, INFO
REC_DTYPE = np.dtype([("gene", "<i4"), ("entry_a", "<i4"), ("entry_b", "<i4"), ("bits", "<u4")])
NO_OUTPUT = "Error: please specify an output directory."
NO_SAMPLE = "Error sample not found in VCF."


class FatalError(Exception):
    pass


def read_text(path: str) -> str:
    if "gz" in path:                               # the reference's test (:35)
        with gzip.open(path, "rt") as f:
            return f.read()
    with open(path) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------- genotype VCF
def _info_dict(text: str) -> Dict[str, str]:
    out = {}
    for item in text.split(";"):
        if "=" in item:
            p = item.split("=")
            out[p[0]] = p[1]
    return out


def _two_alleles(gt: str, allow_slash: bool):
    """A genotype field -> (eligible, alleles): `eligible` by the reference's tests (:84-89, :99-106), `alleles` the two allele indices or None
    when the text does not reduce to exactly two single digits."""
    chars = list(gt)
    if "." in chars or chars.count("0") == 2 or (not allow_slash and "/" in chars):
        return False, None
    rest = list(chars)
    if allow_slash and "/" in rest:
        rest.remove("/")
    if "|" in rest:
        rest.remove("|")
    if not ("|" in chars or len(set(rest)) == 1):
        return False, None
    if len(rest) != 2 or not all(c in "0123456789" for c in rest):
        return True, None
    return True, (int(rest[0]), int(rest[1]))


def parse_genotypes(vcf_text: str, sample: str, log: Callable[[str], None]):
    """-> (gw, pg, rsid_of): gw / pg = [(unique_id, info fields, (allele, allele), block)] in file order; raises FatalError(NO_SAMPLE)"""
    gw, pg, rsid_of = [], [], {}
    col = 0
    skipped = 0
    for line in vcf_text.split("\n"):
        if line[0:4] == "#CHR":
            c = line.split("\t")
            if sample not in c:
                raise FatalError(NO_SAMPLE)
            col = c.index(sample)
        elif line and line[0:1] != "#":
            c = line.split("\t")
            uid = "_".join([c[0], c[1], c[3], c[4]])
            rsid_of[uid] = c[2]
            fmt = c[8].split(":"); cell = c[col].split(":")
            if len(fmt) != len(cell):
                log("Column info error %s" % uid)
                continue
            info = None
            if "GT" in fmt:
                ok, al = _two_alleles(cell[fmt.index("GT")], True)
                if ok and al is None:
                    skipped += 1
                elif ok:
                    info = _info_dict(c[7])
                    gw.append((uid, info, al, 0.0))
            if "PG" in fmt and "PI" in fmt:
                ok, al = _two_alleles(cell[fmt.index("PG")], False)
                if ok and al is None:
                    skipped += 1
                elif ok:
                    try:
                        block = float(cell[fmt.index("PI")])
                    except ValueError:
                        skipped += 1
                        continue
                    pg.append((uid, info if info is not None else _info_dict(c[7]), al, block))
    if skipped:
        log("     %d genotype(s) that are not two single-digit alleles were skipped" % skipped)
    return gw, pg, rsid_of


# ---------------------------------------------------------------------------------------------------------------- native lookup
def tabix_lines(path: str, wanted: list, cols: List[int], threads: int = 1, use_index: bool = True):
    """Every line of a bgzipped table whose (column 1, column 2) is a (contig, 1-based position) of `wanted`, in file order, reduced to the 0-based
    columns `cols` (-1 = the last) -> ({(contig, pos): [[column text...]]}, contigs of the file)"""
    lib = _lib.load()
    keys = list(wanted)
    cb = [c.encode() for c, _ in keys]
    carr = (C.c_char_p * max(1, len(cb)))(*cb)
    parr = np.ascontiguousarray([p for _, p in keys] or [0], dtype=np.int64)
    colarr = np.ascontiguousarray(cols, dtype=np.int32)
    optr = C.c_void_p(); olen = C.c_int64(0); cptr = C.c_void_p(); clen = C.c_int64(0)
    st = lib.phz_tabix_lines(path.encode(), len(keys), carr, C.c_void_p(parr.ctypes.data), len(colarr), C.c_void_p(colarr.ctypes.data),
                             int(bool(use_index)), max(1, int(threads)), C.byref(optr), C.byref(olen), C.byref(cptr), C.byref(clen))
    if st != _lib.PHZ_OK:
        raise _lib.PhzError(st, "phz_tabix_lines(%s) failed" % path)
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


def _chrom_pos(uid: str):
    f = uid.split("_")
    return f[0], int(f[1])


# ---------------------------------------------------------------------------------------------------------------- kernel input
class AnnotInput:
    """The arrays of phz_annot_in (include/phz.h) plus what the rows need: genes[g], uids[v], and per entry its variant."""

    def __init__(self, genes, uids, entry_off, n_gw, entry_var, entry_mask, entry_flags, gw_allele, pg_allele, gw_block, pg_block):
        self.genes = list(genes); self.uids = list(uids)
        self.entry_off = np.ascontiguousarray(entry_off, dtype=np.int64)
        self.n_gw = np.ascontiguousarray(n_gw, dtype=np.int32)
        self.entry_var = np.ascontiguousarray(entry_var, dtype=np.int32)
        self.entry_mask = np.ascontiguousarray(entry_mask, dtype=np.uint16)
        self.entry_flags = np.ascontiguousarray(entry_flags, dtype=np.uint8)
        self.gw_allele = np.ascontiguousarray(gw_allele, dtype=np.uint8).reshape(-1)
        self.pg_allele = np.ascontiguousarray(pg_allele, dtype=np.uint8).reshape(-1)
        self.gw_block = np.ascontiguousarray(gw_block, dtype=np.int32)
        self.pg_block = np.ascontiguousarray(pg_block, dtype=np.int32)

    @property
    def n_pairs(self):
        n = self.n_gw.astype(np.int64); m = np.diff(self.entry_off) - n
        return int((n * n + m * m).sum())

    def struct(self):
        s = _lib.phz_annot_in()
        vp = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None
        s.n_genes = len(self.genes); s.n_entries = len(self.entry_var); s.n_vars = len(self.uids)
        s.entry_off = vp(self.entry_off); s.n_gw = vp(self.n_gw); s.entry_var = vp(self.entry_var); s.entry_mask = vp(self.entry_mask)
        s.entry_flags = vp(self.entry_flags); s.gw_allele = vp(self.gw_allele); s.pg_allele = vp(self.pg_allele)
        s.gw_block = vp(self.gw_block); s.pg_block = vp(self.pg_block)
        return s


def annot_pairs(lib, handle, ai: AnnotInput, batch_rows: int = 0, stats: Optional[dict] = None) -> np.ndarray:
    """phz_annot_pairs (count call, then fill call) -> records (REC_DTYPE) in the reference's row order"""
    s = ai.struct()
    n_rows = C.c_int64(0); n_pairs = C.c_int64(0); n_batches = C.c_int32(0)

    def call(ptr, cap):
        st = lib.phz_annot_pairs(handle, C.byref(s), int(batch_rows), ptr, cap, C.byref(n_rows), C.byref(n_pairs), C.byref(n_batches))
        if st != _lib.PHZ_OK:
            raise _lib.PhzError(st, (lib.phz_last_error(handle) or b"").decode())
    call(None, 0)
    rec = np.zeros(n_rows.value, dtype=REC_DTYPE)
    if n_rows.value:
        call(C.c_void_p(rec.ctypes.data), len(rec))
    if stats is not None:
        stats.update({"pairs": n_pairs.value, "rows": n_rows.value, "batches": n_batches.value})
    return rec


def build_input(gw, pg, cadd: Dict[tuple, list], af_field: Optional[str]):
    """Steps 2 of the reference (:116-174) on looked-up CADD rows.  gw / pg from parse_genotypes; cadd = {(contig, pos): [CADD_COLS fields]};
    af_field = the INFO key to take allele frequencies from, None with --af_vcf.
    -> (AnnotInput, ann): ann[v] = {(gene, alt_index): [phred, effect, gene name, alt base, af or None]}"""
    var_of: Dict[str, int] = {}
    uids: List[str] = []
    ann: List[dict] = []
    genes_of: List[list] = []
    gw_info: Dict[int, tuple] = {}
    pg_info: Dict[int, tuple] = {}
    gene_idx: Dict[str, int] = {}
    gw_list: List[list] = []
    pg_list: List[list] = []
    blocks: Dict[float, int] = {0.0: 0}

    def retrieve(uid, info):                       # get_variant_cadd (:283-332)
        chrom, pos = _chrom_pos(uid)
        alts = uid.split("_")[3].split(",")
        out = {}; gl = []
        for f in cadd.get((chrom, pos), ()):
            alt = f[2]
            if alt in alts:
                ai = alts.index(alt) + 1
                gl.append(f[4])
                af = None
                if af_field is not None and af_field in info:
                    try:
                        af = float(info[af_field].split(",")[ai - 1])
                    except (ValueError, IndexError):
                        af = None
                out[(f[4], ai)] = [f[6], f[3], f[5], alt, af]
        return out, gl

    def variant(uid):
        v = var_of.get(uid)
        if v is None:
            v = var_of[uid] = len(uids)
            uids.append(uid); ann.append({}); genes_of.append([])
        return v

    def add(lists, gene, v):
        g = gene_idx.get(gene)
        if g is None:
            g = gene_idx[gene] = len(gene_idx)
            gw_list.append([]); pg_list.append([])
        lists[g].append(v)

    for uid, info, al, _ in gw:
        v = variant(uid)
        ann[v], genes_of[v] = retrieve(uid, info)
        gw_info[v] = (al, 0)
        for gene in genes_of[v]:
            add(gw_list, gene, v)
    later = []
    for uid, info, al, block in pg:
        v = var_of.get(uid)
        if v is not None and v in gw_info:         # keeps its GW info (:144-147)
            pg_info[v] = gw_info[v]
            for gene in genes_of[v]:
                add(pg_list, gene, v)
        else:
            later.append((uid, info, al, block))
    for uid, info, al, block in later:
        v = variant(uid)
        ann[v], genes_of[v] = retrieve(uid, info)
        pg_info[v] = (al, blocks.setdefault(block, len(blocks)))
        for gene in genes_of[v]:
            add(pg_list, gene, v)
    # ---- arrays; the pseudo-gene NA is never reported (:210)
    genes = [g for g in gene_idx if g != "NA"]
    nv = len(uids)
    gw_allele = np.zeros((nv, 2), np.uint8); pg_allele = np.zeros((nv, 2), np.uint8)
    gw_block = np.zeros(nv, np.int32); pg_block = np.zeros(nv, np.int32)
    for v, (al, b) in gw_info.items():
        gw_allele[v] = al; gw_block[v] = b
    for v, (al, b) in pg_info.items():
        pg_allele[v] = al; pg_block[v] = b
    entry_off = [0]; n_gw = []; e_var = []; e_mask = []; e_flags = []
    for gene in genes:
        g = gene_idx[gene]
        in_gw = set(gw_list[g]); in_pg = set(pg_list[g])
        seen = set()
        for which, lst in ((0, gw_list[g]), (1, pg_list[g])):
            for v in lst:
                mask = 0
                for (gn, ai) in ann[v]:
                    if gn == gene and ai < 16:
                        mask |= 1 << ai
                fl = _lib.PHZ_ANNOT_BOTH if v in (in_pg if which == 0 else in_gw) else 0
                if which == 1 and v not in seen:
                    seen.add(v); fl |= _lib.PHZ_ANNOT_FIRST
                e_var.append(v); e_mask.append(mask); e_flags.append(fl)
        n_gw.append(len(gw_list[g]))
        entry_off.append(len(e_var))
    return AnnotInput(genes, uids, entry_off, n_gw, e_var, e_mask, e_flags, gw_allele, pg_allele, gw_block, pg_block), ann


def lookup_af(af_rows: Dict[tuple, list], af_field: str, wanted):
    """get_variant_af (:249-281) on looked-up rows [POS, ALT, INFO]: the AF of the alt base in the FIRST record at the position, the integer 0 when
    the position, the field or the base is absent -> {(contig, pos, alt): text}"""
    out = {}
    for chrom, pos, alt in wanted:
        text = "0"
        rows = af_rows.get((chrom, pos), ())
        if rows:
            alts = rows[0][1].split(",")
            val = _info_dict(rows[0][2]).get(af_field)
            afs = val.split(",") if val not in (None, "") else []
            if afs and alt in alts and alts.index(alt) < len(afs):
                try:
                    text = repr(float(afs[alts.index(alt)]))
                except ValueError:
                    text = "None"                  # the VCF parser's value of "."
        out[(chrom, pos, alt)] = text
    return out


def format_rows(ai: AnnotInput, ann, rec: np.ndarray, rsid_of: Dict[str, str], af_text: Optional[dict], threads: int = 1) -> bytes:
    """build_interaction_result (:405-456): the text of the records.  af_text = lookup_af's table with --af_vcf, else None.  What a row says about
    one side depends on (entry, allele) only: that text is made here once per annotated (entry, allele), phz_annot_rows assembles the rows."""
    egene = np.repeat(np.arange(len(ai.genes)), np.diff(ai.entry_off)).tolist()
    evar = ai.entry_var.tolist()
    slot_of = np.full(len(evar) * 16, -1, dtype=np.int32)
    heads: List[str] = []; sides: List[str] = []
    for e, (g, v) in enumerate(zip(egene, evar)):
        gene = ai.genes[g]; uid = ai.uids[v]
        for (gn, k), (phred, effect, name, alt, af) in ann[v].items():
            if gn != gene or k >= 16:
                continue
            if af_text is not None:
                chrom, pos = _chrom_pos(uid)
                allele, aftxt = alt, af_text[(chrom, pos, alt)]
            else:
                allele, aftxt = str(k), ("." if af is None else repr(af))
            slot_of[e * 16 + k] = len(heads)
            heads.append(gene + "\t" + name)
            sides.append("\t".join([uid, rsid_of[uid], allele, aftxt, phred, effect]))
    header = ("\t".join(COLUMNS) + "\n").encode()
    if not len(rec):
        return header

    def pool(items):
        raw = [x.encode() for x in items]
        off = np.zeros(len(raw) + 1, dtype=np.int64); np.cumsum([len(x) for x in raw], out=off[1:])
        return b"".join(raw), off
    hb, ho = pool(heads); sb, so = pool(sides)
    rec = np.ascontiguousarray(rec, dtype=REC_DTYPE)
    lib = _lib.load()
    optr = C.c_void_p(); olen = C.c_int64(0)
    st = lib.phz_annot_rows(C.c_void_p(rec.ctypes.data), len(rec), len(evar), C.c_void_p(slot_of.ctypes.data), len(heads), hb, C.c_void_p(ho.ctypes.data),
                            sb, C.c_void_p(so.ctypes.data), max(1, int(threads)), C.byref(optr), C.byref(olen))
    if st != _lib.PHZ_OK:
        raise _lib.PhzError(st, "phz_annot_rows: a record names an (entry, allele) without an annotation")
    try:
        return header + C.string_at(optr, olen.value)
    finally:
        lib.phz_buf_free(optr)


# ---------------------------------------------------------------------------------------------------------------- run
def annotate(geno_vcf: str, sample: str, cadd_file: str, af_vcf: Optional[str] = None, af_field: str = "AF", threads: int = 1,
             batch_rows: int = 0, log: Optional[Callable[[str], None]] = None, stats: Optional[dict] = None, ctx: Optional[_lib.Context] = None,
             _interactions=None, as_bytes: bool = False):
    """-> the output text (bytes with as_bytes).  _interactions: test hook replacing the K_annot launch, called as _interactions(AnnotInput) -> records (REC_DTYPE)."""
    log = log or (lambda s: None)
    if ctx is None and _interactions is None:
        ctx = _lib.Context(0)                          # raises without a GPU: there is no CPU path
    t0 = time.perf_counter()
    log("1. Reading VCF...")
    gw, pg, rsid_of = parse_genotypes(read_text(geno_vcf), sample, log)
    t1 = time.perf_counter()
    log("2. Retrieving CADD info for all phased variants...")
    keys = sorted({_chrom_pos(x[0]) for x in gw} | {_chrom_pos(x[0]) for x in pg})
    cadd, cadd_contigs = tabix_lines(cadd_file, keys, CADD_COLS, threads) if keys else ({}, set())
    ai, ann = build_input(gw, pg, cadd, None if af_vcf is not None else af_field)
    t2 = time.perf_counter()
    log("3. Retrieving variant allele frequencies...")
    af_text = None
    if af_vcf is not None:
        wanted = sorted({_chrom_pos(ai.uids[v]) + (f[3],) for v in range(len(ai.uids)) for f in ann[v].values()})
        af_rows, _ = tabix_lines(af_vcf, sorted({w[:2] for w in wanted}), AF_COLS, threads) if wanted else ({}, set())
        af_text = lookup_af(af_rows, af_field, wanted)
    t3 = time.perf_counter()
    log("4. Identifying cases of compound heterozygosity...")
    if _interactions is not None:
        rec = _interactions(ai)
    else:
        rec = annot_pairs(ctx.lib, ctx.h, ai, batch_rows, stats)
        if stats is not None:
            stats["k_annot_ms"] = ctx.timing(_lib.PHZ_T_ANNOT)[0]
    t4 = time.perf_counter()
    text = format_rows(ai, ann, rec, rsid_of, af_text, threads)
    if stats is not None:
        stats.setdefault("pairs", ai.n_pairs); stats.setdefault("rows", len(rec))
        stats.update({"genes": len(ai.genes), "variants": len(ai.uids), "entries": len(ai.entry_var),
                      "seconds": {"vcf": round(t1 - t0, 3), "cadd": round(t2 - t1, 3), "af": round(t3 - t2, 3), "pairs": round(t4 - t3, 3),
                                  "format": round(time.perf_counter() - t4, 3)}})
    return text if as_bytes else text.decode()


def main(argv=None, _interactions=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--geno_vcf", help="VCF containing phased genotype.")
    ap.add_argument("--sample", help="Name of sample to use in VCF file.")
    ap.add_argument("--af_vcf", help="VCF to retrieve allele frequencies from. Must be indexed with tabix. If left blank will attempt to retrieve from genotype vcf.")
    ap.add_argument("--af_field", default="AF", help="Allele frequency field in af_vcf to use ('AF' by default).")
    ap.add_argument("--cadd_file", help="The path to the CADD 'whole_genome_SNVs.tsv.gz' file.")
    ap.add_argument("--o", help="Output file")
    ap.add_argument("--threads", type=int, default=1, help="Number of threads to use.")
    args = ap.parse_args(argv)
    print(""); print("##################################################")
    print("          Welcome to phASER Annotate (phaser_amd, MI355X)")
    print("##################################################"); print("")
    if args.o is None:
        print(NO_OUTPUT)
        return 1
    stats: dict = {}
    try:
        text = annotate(args.geno_vcf, args.sample, args.cadd_file, af_vcf=args.af_vcf, af_field=args.af_field, threads=args.threads, log=print, stats=stats,
                        _interactions=_interactions, as_bytes=True)
    except FatalError as e:
        print(str(e))
        return 1
    with open(args.o, "wb") as f:
        f.write(text)
    print("     %d genes, %d variants, %d ordered pairs -> %d rows in %d batch(es); K_annot %.3f ms" %
          (stats["genes"], stats["variants"], stats["pairs"], stats["rows"], stats.get("batches", 0), stats.get("k_annot_ms", 0.0)))
    print("     seconds: " + ", ".join("%s %.3f" % kv for kv in stats["seconds"].items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
