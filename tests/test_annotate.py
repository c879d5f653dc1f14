"""phaser_annotate on the GPU (phaser_amd/annotate.py, K_annot in phaser_amd/csrc/phz_annot.hip, phz_tabix_lines).

The reference needs pysam and PyVCF, so no golden comes from it.  Two anchors instead: tests/annotate_restatement.py restates its four steps over plain
dicts, and one tiny case whose expected rows are written out below, derived by reading phaser_annotate/phaser_annotate.py, pins that restatement."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import annotate_restatement as R
from conftest import REPO

HIPEMU = os.path.join(REPO, "tests", "hipemu")
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
EMU_DIR = os.path.join(HIPEMU, "_build", "annot")
SAMPLE = "S1"
N_CADD = 100            # columns of a synthetic CADD row (a few rows are shorter: "last column" is not a fixed index)


# ------------------------------------------------------------------------------------------------ worlds: a genotype VCF, a CADD table, an AF VCF
def cadd_row(contig, pos, ref, alt, effect, gene, name, phred, width=N_CADD):
    f = ["c%d" % i for i in range(width)]
    f[0], f[1], f[2], f[3], f[4], f[10], f[92], f[95], f[-1] = contig, str(pos), ref, "NA", alt, effect, gene, name, phred
    return f


class World:
    def __init__(self):
        self.vcf = ["##fileformat=VCFv4.2", "#" + "\t".join(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT", "S0", SAMPLE])]
        self.cadd = []
        self.af = ["##fileformat=VCFv4.2", "#" + "\t".join(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"])]

    def var(self, contig, pos, ref, alt, gt, pg=None, pi=None, info=".", rsid=None):
        fmt, cell, other = ("GT", gt, "0|0") if pg is None else ("GT:PG:PI", "%s:%s:%s" % (gt, pg, pi), "0|0:.:.")
        self.vcf.append("\t".join([contig, str(pos), rsid or "rs%d" % pos, ref, alt, ".", "PASS", info, fmt, other, cell]))

    def note(self, contig, pos, ref, alt, gene, effect="MISSENSE", phred=None, name=None, width=N_CADD):
        self.cadd.append(cadd_row(contig, pos, ref, alt, effect, gene, name or gene.replace("ENSG", "NAME"), phred or "%d.%d" % (pos % 37, pos % 10), width))

    def freq(self, contig, pos, ref, alt, info):
        self.af.append("\t".join([contig, str(pos), ".", ref, alt, ".", "PASS", info]))

    @property
    def vcf_text(self):
        return "\n".join(self.vcf) + "\n"

    @property
    def cadd_text(self):
        return "## CADD synthetic\n#Chrom\tPos\tRef\tAnc\tAlt\n" + "".join("\t".join(r) + "\n" for r in self.cadd)

    def cadd_rows(self):
        out = {}
        for r in self.cadd:
            out.setdefault((r[0], int(r[1])), []).append(r)
        return out

    def af_rows(self):
        out = {}
        for line in self.af[2:]:
            c = line.split("\t")
            out.setdefault((c[0], int(c[1])), []).append((c[4], c[7]))
        return out

    def write(self, tmp, tbi=True, gz_vcf=False):
        from phaser_amd import vcfout
        paths = {"vcf": os.path.join(tmp, "geno.vcf.gz" if gz_vcf else "geno.vcf"), "cadd": os.path.join(tmp, "cadd.tsv.gz"), "af": os.path.join(tmp, "af.vcf.gz")}
        if gz_vcf:
            with gzip.open(paths["vcf"], "wt") as f:
                f.write(self.vcf_text)
        else:
            open(paths["vcf"], "w").write(self.vcf_text)
        assert vcfout.write_bgzf(paths["cadd"], self.cadd_text, 2, index="vcf" if tbi else None)
        assert vcfout.write_bgzf(paths["af"], "\n".join(self.af) + "\n", 2, index="vcf" if tbi else None)
        assert os.path.exists(paths["cadd"] + ".tbi") == tbi
        return paths


def literal_world():
    """two genes, six variants (the hand-derived case)"""
    w = World()
    w.var("1", 100, "A", "G", "0|1", "0|1", "1", "AF=0.1", "rs1");     w.note("1", 100, "A", "G", "ENSG01", "MISSENSE", "10.1", "G1")
    w.var("1", 200, "C", "T", "1|0", "1|0", "1", "AF=0.2", "rs2");     w.note("1", 200, "C", "T", "ENSG01", "STOP_GAINED", "20.2", "G1")
    w.var("1", 300, "G", "A", "0/1", "0|1", "1", "AF=0.3", "rs3");     w.note("1", 300, "G", "A", "ENSG01", "SYNONYMOUS", "5.5", "G1")
    w.var("1", 400, "T", "C,G", "1|2", "1|2", "2", "AF=0.4,0.04", "rs4")
    w.note("1", 400, "T", "C", "ENSG02", "MISSENSE", "7.7", "G2");     w.note("1", 400, "T", "G", "ENSG02", "SPLICE_SITE", "8.8", "G2")
    w.var("1", 500, "A", "T", "1|1", "1|1", "2", "AF=0.5", "rs5");     w.note("1", 500, "A", "T", "ENSG02", "MISSENSE", "9.9", "G2")
    w.var("1", 600, "C", "A", "0/1", "0|1", "1", "DP=5", ".");         w.note("1", 600, "C", "A", "ENSG01", "INTRONIC", "3.3", "G1")
    w.freq("1", 100, "A", "G", "AF=0.11"); w.freq("1", 200, "C", "T", "AC=3;AF=0.22"); w.freq("1", 400, "T", "G,C", "AF=0.044,0.44")
    w.freq("1", 500, "A", "C", "AF=0.55"); w.freq("1", 600, "C", "A", "AF=0.66"); w.freq("1", 600, "C", "A", "AF=0.99")
    return w


# Derived from the reference's text.  ENSG01: GW list [100, 200], PG list [100, 200, then the PG-only 300, 600].  First pass: (100, 200) has alleles
# [0,1] x [1,0] in block 0 -> only (1, 1) with indices (1, 0): trans; both are in the PG list with their GW info (:144-147), so read_backed 1; (200, 100)
# likewise.  Second pass: (100, 200) / (200, 100) are in outputted_configs; 100 / 200 (block 0) never meet 300 / 600 (block 1.0); (300, 600): [0,1] x [0,1]
# -> (1, 1) at indices (1, 1): cis; (600, 300) likewise.  ENSG02: 400 has two CADD rows for the gene (alts C and G), so it is listed twice (:320):
# GW [400, 400, 500] = PG.  (400, 500): [1,2] x [1,1] -> all four combinations, once per listing of 400; then (500, 400): [1,1] x [1,2], twice as well.
# The second pass puts out nothing: every pair is in outputted_configs.
_A = {100: ("1_100_A_G", "rs1", "G", "0.1", "0.11", "10.1", "MISSENSE"), 200: ("1_200_C_T", "rs2", "T", "0.2", "0.22", "20.2", "STOP_GAINED"),
      300: ("1_300_G_A", "rs3", "A", "0.3", "0", "5.5", "SYNONYMOUS"), 600: ("1_600_C_A", ".", "A", ".", "0.66", "3.3", "INTRONIC"),
      500: ("1_500_A_T", "rs5", "T", "0.5", "0", "9.9", "MISSENSE"),
      (400, 1): ("1_400_T_C,G", "rs4", "C", "0.4", "0.44", "7.7", "MISSENSE"), (400, 2): ("1_400_T_C,G", "rs4", "G", "0.04", "0.044", "8.8", "SPLICE_SITE")}
_FWD = [("ENSG02", "G2", (400, 1), 1, 500, 1, "cis", 1), ("ENSG02", "G2", (400, 1), 1, 500, 1, "trans", 1),
        ("ENSG02", "G2", (400, 2), 2, 500, 1, "trans", 1), ("ENSG02", "G2", (400, 2), 2, 500, 1, "cis", 1)]
_REV = [("ENSG02", "G2", 500, 1, (400, 1), 1, "cis", 1), ("ENSG02", "G2", 500, 1, (400, 2), 2, "trans", 1),
        ("ENSG02", "G2", 500, 1, (400, 1), 1, "trans", 1), ("ENSG02", "G2", 500, 1, (400, 2), 2, "cis", 1)]
_LITERAL = [("ENSG01", "G1", 100, 1, 200, 1, "trans", 1), ("ENSG01", "G1", 200, 1, 100, 1, "trans", 1),
            ("ENSG01", "G1", 300, 1, 600, 1, "cis", 1), ("ENSG01", "G1", 600, 1, 300, 1, "cis", 1)] + _FWD + _FWD + _REV + _REV


def literal_text(af_vcf):
    lines = ["\t".join(R.HEADER)]
    for gene, name, a, ia, b, ib, cfg, rb in _LITERAL:
        ua, ra, basea, afa, afva, pa, ea = _A[a]; ub, rb_, baseb, afb, afvb, pb, eb = _A[b]
        lines.append("\t".join([gene, name, ua, ra, basea if af_vcf else str(ia), afva if af_vcf else afa, pa, ea,
                                ub, rb_, baseb if af_vcf else str(ib), afvb if af_vcf else afb, pb, eb, cfg, str(rb)]))
    return "\n".join(lines) + "\n"


GTS = ["0|1", "1|0", "1|1", "1/1", "1|2"]


def small_world():
    """The smallest inputs at which K_annot can go wrong, built by hand (the list is in the issue of this feature and in DESIGN.md)."""
    w = World()
    # a gene with one entry; a variant that only the pseudo-gene NA annotates; a variant in NA and in a real gene
    w.var("1", 1000, "A", "G", "0|1", info="AF=0.25"); w.note("1", 1000, "A", "G", "ENSG_ONE")
    w.var("1", 1010, "A", "G", "0|1"); w.note("1", 1010, "A", "G", "NA")
    # two entries, GW only (no PG field at all)
    w.var("1", 1100, "A", "G", "0|1", info="AF=0.5,0.1"); w.note("1", 1100, "A", "G", "NA"); w.note("1", 1100, "A", "G", "ENSG_TWO")
    w.var("1", 1110, "C", "T", "1|0", info="DP=3;AF=0.125"); w.note("1", 1110, "C", "T", "ENSG_TWO", width=98)
    # PG entries only: equal PI, a different PI, a PG-only variant with two CADD rows (no duplicate pair in the second pass)
    w.var("1", 1200, "A", "G", "0/1", "0|1", "5"); w.note("1", 1200, "A", "G", "ENSG_PG")
    w.var("1", 1210, "A", "G", "0/1", "1|0", "5"); w.note("1", 1210, "A", "G", "ENSG_PG", "SYNONYMOUS"); w.note("1", 1210, "A", "G", "ENSG_PG", "MISSENSE", "31.5")
    w.var("1", 1220, "A", "G", "0/1", "0|1", "6"); w.note("1", 1220, "A", "G", "ENSG_PG")
    w.var("1", 1230, "A", "C,G", "0/1", "1|2", "5.0"); w.note("1", 1230, "A", "C", "ENSG_PG"); w.note("1", 1230, "A", "G", "ENSG_PG")
    # 40 GW entries of 34 variants over the five genotypes: a 1|2 with a row per alt is listed twice, one variant has two rows for one alt (a duplicate
    # entry), one 1|2 has no row for its second alt
    k = 0
    for i in range(39):
        pos = 2000 + 10 * i
        gt = GTS[i % 5]
        alt = "C,G" if gt == "1|2" else "G"
        if i % 4 == 0:
            w.var("1", pos, "A", alt, gt)                                                      # GW only
        elif i % 4 == 1:
            w.var("1", pos, "A", alt, gt, gt.replace("/", "|"), str(1 + i % 3))               # both sets, same alleles
        elif i % 4 == 2:
            w.var("1", pos, "A", alt, gt, {"0|1": "1|0", "1|0": "0|1"}.get(gt, "1|1"), "2")    # both sets, PG alleles differ: the GW info wins
        else:
            w.var("1", pos, "A", alt, "0/1", "0|1" if i % 8 == 3 else "1|0", str(1 + i % 2))   # unphased in GT, phased in PG: PG only
        w.note("1", pos, "A", alt.split(",")[0], "ENSG_BIG"); k += i % 4 != 3
        if gt == "1|2" and i != 9:
            w.note("1", pos, "A", "G", "ENSG_BIG"); k += i % 4 != 3                            # (listed twice); i == 9: only alt 1 annotated (rows dropped through the mask)
        if i == 5:
            w.note("1", pos, "A", "G", "ENSG_BIG", "SPLICE_SITE", "40"); k += 1                # the same key again: the last row wins, the variant is listed twice
        if i >= 36:
            w.note("1", pos, "A", alt.split(",")[0], "ENSG_NEXT")                              # the neighbouring gene overlaps the big one
    assert k == 36
    for i in range(4):                                                                         # four more GW entries -> 40
        pos = 2400 + 10 * i
        w.var("1", pos, "A", "G", GTS[i % 4], GTS[i % 4].replace("/", "|") if i % 2 else None, "1" if i % 2 else None)
        w.note("1", pos, "A", "G", "ENSG_BIG")
    w.var("1", 2600, "A", "G", "1|0", "1|0", "3"); w.note("1", 2600, "A", "G", "ENSG_NEXT")
    w.var("2", 50, "A", "G", "1|1"); w.note("2", 50, "A", "G", "ENSG_NEXT"); w.note("2", 50, "A", "T", "ENSG_NEXT")
    w.var("2", 60, "A", "G", "1"); w.note("2", 60, "A", "G", "ENSG_NEXT")                      # haploid: skipped
    w.var("2", 70, "A", "G", "1|10", "1|10", "3"); w.note("2", 70, "A", "G", "ENSG_NEXT")      # allele index 10: skipped (twice)
    for pos, alt, info in ((1000, "G", "AF=0.5"), (1100, "T,G", "AF=0.2,0.3"), (2000, "G", "AC=1"), (2050, "G", "AF=0.75"), (2090, "G,C", "AF=0.1,0.9")):
        w.freq("1", pos, "A", alt, info)
    w.freq("2", 50, "A", "G", "AF=1.0")
    return w


# ------------------------------------------------------------------------------------------------ K_annot under the emulation
def _emu_lib(tile=None):
    from phaser_amd import _lib
    os.makedirs(EMU_DIR, exist_ok=True)
    tag = "" if tile is None else "_t%d" % tile
    lib = os.path.join(EMU_DIR, "libphz_annot%s.so" % tag)
    srcs = [os.path.join(CSRC, "phz_api.hip"), os.path.join(CSRC, "phz_annot.hip"), os.path.join(HIPEMU, "hipemu.cpp")]
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(REPO, "include", "phz.h"), os.path.join(HIPEMU, "hipemu.h")]
    newest = max(os.path.getmtime(p) for p in srcs + hdrs)
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        import fcntl
        with open(os.path.join(EMU_DIR, ".lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            flags = ["-O1", "-std=c++17", "-fPIC", "-I" + os.path.join(HIPEMU, "include"), "-I" + os.path.join(REPO, "include"), "-I" + CSRC]
            defs = [] if tile is None else ["-DPHZ_ANNOT_TILE=%d" % tile, "-DPHZ_ANNOT_GRID=37"]          # small tiles, several launches per pass
            objs = []
            for src in srcs:
                obj = os.path.join(EMU_DIR, os.path.basename(src) + tag + ".o"); objs.append(obj)
                lang = [] if src.endswith(".cpp") else ["-x", "c++"]
                subprocess.check_call(["g++"] + flags + defs + lang + ["-c", src, "-o", obj])
            subprocess.check_call(["g++", "-shared", "-fPIC"] + objs + ["-o", lib + ".tmp", "-lpthread"])
            os.replace(lib + ".tmp", lib)
    L = C.CDLL(lib)
    for name in ("phz_ctx_create", "phz_ctx_destroy", "phz_last_error", "phz_annot_pairs", "phz_get_timing"):
        res, args = _lib.SYMBOLS[name]
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


class Emu:
    def __init__(self, tile=None):
        self.tile = tile
        self.lib = _emu_lib(tile)
        self.h = C.c_void_p()
        assert self.lib.phz_ctx_create(0, C.byref(self.h)) == 0

    def __call__(self, ai, batch_rows=0, stats=None):
        from phaser_amd import annotate
        return annotate.annot_pairs(self.lib, self.h, ai, batch_rows, stats)

    def close(self):
        self.lib.phz_ctx_destroy(self.h)


@pytest.fixture(scope="module", params=[None, 8], ids=["tile256", "tile8"])
def emu(request):
    e = Emu(request.param)
    yield e
    e.close()


def record_tuples(ai, rec):
    """kernel records -> the tuples of annotate_restatement.record_tuples"""
    out = []
    for g, a, b, bits in rec.tolist():
        out.append((ai.genes[g], ai.uids[ai.entry_var[a]], ai.uids[ai.entry_var[b]], bits & 15, (bits >> 4) & 15, "trans" if bits >> 8 & 1 else "cis",
                    ((bits >> 10) & 3) - 1))
    return out


def product_input(w, af_field="AF"):
    from phaser_amd import annotate
    gw, pg, rsid = annotate.parse_genotypes(w.vcf_text, SAMPLE, lambda s: None)
    cadd = {k: [[r[c] for c in annotate.CADD_COLS] for r in rows] for k, rows in w.cadd_rows().items()}
    return annotate.build_input(gw, pg, cadd, af_field)


def with_empty_gene(ai, at):
    """the same input with a gene of no entries put in front of gene `at`"""
    from phaser_amd import annotate
    off = ai.entry_off.tolist(); n_gw = ai.n_gw.tolist()
    return annotate.AnnotInput(ai.genes[:at] + ["ENSG_EMPTY"] + ai.genes[at:], ai.uids, off[:at + 1] + off[at:], n_gw[:at] + [0] + n_gw[at:], ai.entry_var,
                               ai.entry_mask, ai.entry_flags, ai.gw_allele, ai.pg_allele, ai.gw_block, ai.pg_block)


def tables_to_input(T):
    """restatement tables -> AnnotInput, written apart from the product's build_input (the random sets and the conflicting-phase case start from tables)"""
    from phaser_amd import _lib, annotate
    uids = list(dict.fromkeys(list(T["gw_info"]) + list(T["pg_info"])))
    vi = {u: i for i, u in enumerate(uids)}
    blocks = {}
    gwa = np.zeros((len(uids), 2), np.uint8); pga = np.zeros((len(uids), 2), np.uint8)
    gwb = np.zeros(len(uids), np.int32); pgb = np.zeros(len(uids), np.int32)
    for tab, al, bl in ((T["gw_info"], gwa, gwb), (T["pg_info"], pga, pgb)):
        for u, rec in tab.items():
            al[vi[u]] = rec[0]; bl[vi[u]] = blocks.setdefault(float(rec[3]), len(blocks))
    genes = [g for g in T["gene_order"] if g != "NA"]
    off = [0]; n_gw = []; ev = []; em = []; ef = []
    for g in genes:
        gl, pl = T["gw_genes"].get(g, []), T["pg_genes"].get(g, [])
        for u in gl:
            notes = T["gw_info"][u][1]
            ev.append(vi[u]); em.append(sum(1 << k for k in range(1, 16) if "%s:%d" % (g, k) in notes)); ef.append(_lib.PHZ_ANNOT_BOTH if u in pl else 0)
        seen = set()
        for u in pl:
            notes = T["pg_info"][u][1]
            ev.append(vi[u]); em.append(sum(1 << k for k in range(1, 16) if "%s:%d" % (g, k) in notes))
            ef.append((_lib.PHZ_ANNOT_BOTH if u in gl else 0) | (0 if u in seen else _lib.PHZ_ANNOT_FIRST)); seen.add(u)
        n_gw.append(len(gl)); off.append(len(ev))
    return annotate.AnnotInput(genes, uids, off, n_gw, ev, em, ef, gwa, pga, gwb, pgb)


def random_tables(seed, n_genes=200, max_n=60, conflicts=True):
    rng = np.random.default_rng(seed)
    T = {"gw_info": {}, "pg_info": {}, "gw_genes": {}, "pg_genes": {}, "gene_order": [], "rsid": {}, "af": None}
    pos = 0
    prev = []
    for g in range(n_genes):
        gene = "ENSG%04d" % g
        T["gene_order"].append(gene)
        n, m = int(rng.integers(0, max_n + 1)), int(rng.integers(0, max_n + 1))
        if g % 17 == 0:
            n = 0
        if g % 19 == 0:
            m = 0
        pool = list(prev[:3])
        for _ in range(max(2, (n + m) // 2)):
            pos += 7
            pool.append("1_%d_A_C,G" % pos)
        for u in pool:
            keys = [k for k in (1, 2) if rng.random() < 0.8]
            kind = int(rng.integers(0, 3))              # 0 GW only, 1 both, 2 PG only
            if u not in T["gw_info"] and u not in T["pg_info"]:
                al = [int(x) for x in rng.integers(0, 3, 2)]
                if al == [0, 0]:
                    al = [0, 1]
                if kind < 2:
                    T["gw_info"][u] = [al, {}, [], 0.0]
                if kind == 1:
                    T["pg_info"][u] = T["gw_info"][u]
                    if conflicts and rng.random() < 0.3:          # beyond what files can produce: the read-backed record of a shared variant differs
                        T["pg_info"][u] = [[al[1], al[0]] if rng.random() < 0.7 else al, T["gw_info"][u][1], [], float(rng.integers(0, 2))]
                if kind == 2:
                    T["pg_info"][u] = [al, {}, [], float(rng.integers(1, 4))]
            for tab in ("gw_info", "pg_info"):
                if u in T[tab]:
                    for k in keys:
                        T[tab][u][1]["%s:%d" % (gene, k)] = ["1.5", "EFFECT", gene, "N" + gene, "1", int(u.split("_")[1]), None, "CG"[k - 1]]
        gwp = [u for u in pool if u in T["gw_info"]]; pgp = [u for u in pool if u in T["pg_info"]]
        if gwp and n:
            T["gw_genes"][gene] = [gwp[int(i)] for i in rng.integers(0, len(gwp), n)]
        if pgp and m:
            T["pg_genes"][gene] = [pgp[int(i)] for i in rng.integers(0, len(pgp), m)]
        prev = pool[-3:]
    return T


_RANDOM = {}


def random_case():
    """computed once, shared by the GPU tests, never changed"""
    if not _RANDOM:
        T = random_tables(11)
        _RANDOM.update(T=T, ai=tables_to_input(T), want=R.record_tuples(R.all_rows(T)))
    return _RANDOM["T"], _RANDOM["ai"], _RANDOM["want"]


# ------------------------------------------------------------------------------------------------ CPU: the anchors
@pytest.mark.parametrize("af_vcf", [False, True])
def test_restatement_matches_the_hand_derived_case(af_vcf):
    w = literal_world()
    T = R.build_tables(w.vcf_text, SAMPLE, w.cadd_rows(), w.af_rows() if af_vcf else None)
    assert R.text_of(R.all_rows(T)) == literal_text(af_vcf)


def test_small_world_holds_the_shapes_it_promises():
    w = small_world()
    T = R.build_tables(w.vcf_text, SAMPLE, w.cadd_rows())
    size = lambda g: (len(T["gw_genes"].get(g, [])), len(T["pg_genes"].get(g, [])))
    assert size("ENSG_ONE") == (1, 0) and size("ENSG_TWO") == (2, 0) and size("ENSG_PG")[0] == 0 and size("ENSG_PG")[1] == 6
    assert size("ENSG_BIG")[0] == 40 and size("ENSG_BIG")[1] > 10
    order = [g for g in T["gene_order"] if g != "NA"]
    assert order.index("ENSG_NEXT") == order.index("ENSG_BIG") + 1 and "NA" in T["gene_order"] and T["skipped"] == 3
    big = T["gw_genes"]["ENSG_BIG"]
    assert len(set(big)) == 34 and len(T["pg_genes"]["ENSG_PG"]) == len(set(T["pg_genes"]["ENSG_PG"])) + 2
    rows = R.all_rows(T)
    assert {r[15] for r in rows} == {"0", "1"} and {r[14] for r in rows} == {"cis", "trans"} and len(rows) > 1500
    assert any(r[4] == 2 for r in rows) and not any(r[2].startswith("1_2090_") and r[4] == 2 for r in rows)      # the mask drops alt 2 of the 1|2 at 2090


# ------------------------------------------------------------------------------------------------ CPU: K_annot emulated
def test_kannot_emulated_small_shapes_match_restatement(emu):
    w = small_world()
    want = R.record_tuples(R.all_rows(R.build_tables(w.vcf_text, SAMPLE, w.cadd_rows())))
    ai, _ = product_input(w)
    stats = {}
    assert record_tuples(ai, emu(ai, stats=stats)) == want
    assert stats["pairs"] == ai.n_pairs and stats["rows"] == len(want) and stats["batches"] == 1
    for at in (0, 2, len(ai.genes)) if emu.tile is None else (2,):          # a gene of no entries: first, between two genes, last
        ai0 = with_empty_gene(ai, at)
        assert record_tuples(ai0, emu(ai0)) == want


def test_kannot_emulated_literal_case(emu):
    w = literal_world()
    ai, _ = product_input(w)
    assert record_tuples(ai, emu(ai)) == R.record_tuples(R.all_rows(R.build_tables(w.vcf_text, SAMPLE, w.cadd_rows())))


def test_kannot_emulated_conflicting_read_backed_phase(emu):
    """The -1 branch (:374-384) cannot come from files (a shared variant keeps its GW info) but the kernel keeps it: tables whose read-backed record of
    a shared variant differs.  The conflicting pair puts out its GW rows with -1 and then its PG rows with 1."""
    T = random_tables(3, n_genes=12, max_n=14)
    want = R.record_tuples(R.all_rows(T))
    assert {t[6] for t in want} == {-1, 0, 1}
    ai = tables_to_input(T)
    assert record_tuples(ai, emu(ai)) == want


def test_kannot_emulated_batches_and_capacity(emu):
    from phaser_amd import _lib
    w = small_world()
    ai, _ = product_input(w)
    whole = emu(ai)
    per_gene = np.bincount(whole["gene"], minlength=len(ai.genes))
    stats = {}
    got = emu(ai, batch_rows=int(per_gene.max()), stats=stats)          # the big gene fills a batch of its own
    assert np.array_equal(got, whole) and stats["batches"] >= 3
    with pytest.raises(_lib.PhzError) as e:
        emu(ai, batch_rows=int(per_gene.max()) - 1)
    assert e.value.status == _lib.PHZ_E_CAPACITY and "gene %d alone" % int(per_gene.argmax()) in str(e.value)
    assert np.array_equal(emu(ai), whole)                                # the context is usable after the refusal


def test_kannot_refuses_indices_out_of_range(emu):
    from phaser_amd import _lib, annotate
    ai, _ = product_input(literal_world())
    bad = annotate.AnnotInput(ai.genes, ai.uids, ai.entry_off, ai.n_gw, np.where(np.arange(len(ai.entry_var)) == 3, len(ai.uids), ai.entry_var), ai.entry_mask,
                              ai.entry_flags, ai.gw_allele, ai.pg_allele, ai.gw_block, ai.pg_block)
    with pytest.raises(_lib.PhzError) as e:
        emu(bad)
    assert e.value.status == _lib.PHZ_E_ARG
    bad = annotate.AnnotInput(ai.genes, ai.uids, ai.entry_off, ai.n_gw + 9, ai.entry_var, ai.entry_mask, ai.entry_flags, ai.gw_allele, ai.pg_allele,
                              ai.gw_block, ai.pg_block)
    with pytest.raises(_lib.PhzError):
        emu(bad)


# ------------------------------------------------------------------------------------------------ CPU: the CLI's host stages with the launch replaced
@pytest.mark.parametrize("af_vcf", [False, True])
@pytest.mark.parametrize("tbi", [True, False])
def test_annotate_host_stages_match_restatement(tmp_path, emu, af_vcf, tbi):
    from phaser_amd import _lib, annotate
    _lib.build()
    for w in (literal_world(), small_world()):
        p = w.write(str(tmp_path), tbi=tbi)
        T = R.build_tables(w.vcf_text, SAMPLE, w.cadd_rows(), w.af_rows() if af_vcf else None)
        stats = {}
        got = annotate.annotate(p["vcf"], SAMPLE, p["cadd"], af_vcf=p["af"] if af_vcf else None, threads=2, stats=stats, _interactions=emu)
        assert got == R.text_of(R.all_rows(T))
        assert stats["pairs"] == R.pair_count(T) and set(stats["seconds"]) == {"vcf", "cadd", "af", "pairs", "format"}
    assert annotate.annotate(p["vcf"], SAMPLE, p["cadd"], _interactions=emu).count("\n") > 1500


def test_annotate_literal_case_from_files(tmp_path, emu):
    from phaser_amd import _lib, annotate
    _lib.build()
    p = literal_world().write(str(tmp_path))
    assert annotate.annotate(p["vcf"], SAMPLE, p["cadd"], _interactions=emu) == literal_text(False)
    assert annotate.annotate(p["vcf"], SAMPLE, p["cadd"], af_vcf=p["af"], _interactions=emu) == literal_text(True)


# ------------------------------------------------------------------------------------------------ CPU: the lookup export
@pytest.mark.parametrize("tbi", [True, False])
def test_tabix_lines_equals_a_plain_line_scan(tmp_path, tbi):
    from phaser_amd import _lib, annotate, vcfout
    _lib.build()
    rng = np.random.default_rng(3)
    lines = ["## header", "#Chrom\tPos"]
    keys = []
    for contig in ("1", "2", "X"):
        pos = np.cumsum(rng.integers(1, 4000, 2500))
        for k, p in enumerate(pos.tolist()):
            for alt in "CGT"[:1 + k % 3]:                                 # one to three lines per position
                width = 100 if k % 11 else 8 + k % 5
                lines.append("\t".join([contig, str(p)] + ["%s%d_%d" % (alt, k, j) for j in range(2, width)]))
            keys.append((contig, p))
    text = "\n".join(lines) + "\n"
    path = os.path.join(str(tmp_path), "t.tsv.gz")
    assert vcfout.write_bgzf(path, text, 3, index="vcf" if tbi else None)
    q = sorted(set([keys[int(i)] for i in rng.integers(0, len(keys), 300)] + [(c, p + 1) for c, p in keys[:40:3]] + [("7", 100), ("1", 0), ("X", 10 ** 9)]))
    cols = [0, 1, 4, 10, 92, 95, -1]
    got, contigs = annotate.tabix_lines(path, q, cols, threads=3)
    want = {}
    for line in text.split("\n"):
        if line and not line.startswith("#"):
            f = line.split("\t")
            if (f[0], int(f[1])) in set(q):
                want.setdefault((f[0], int(f[1])), []).append([(f[c] if c < len(f) else "") if c >= 0 else f[-1] for c in cols])
    assert got == want and len(got) > 250 and ("7", 100) not in got
    assert contigs == {"1", "2", "X"}
    assert annotate.tabix_lines(path, q, [-1, 1], threads=1, use_index=False)[0] == {k: [[r[6], r[1]] for r in v] for k, v in want.items()}
    assert annotate.tabix_lines(path, [("9", 5)], [0])[0] == {}
    with pytest.raises(_lib.PhzError):
        annotate.tabix_lines(path, q, [])


# ------------------------------------------------------------------------------------------------ CPU: the deliberate differences
def test_gene_order_is_first_appearance_gw_lists_first(tmp_path, emu):
    from phaser_amd import _lib, annotate
    _lib.build()
    w = World()
    w.var("1", 100, "A", "G", "0/1", "0|1", "1"); w.note("1", 100, "A", "G", "ENSG_Z_PG")           # read-backed only: named after every GW gene
    w.var("1", 110, "A", "G", "0/1", "1|0", "1"); w.note("1", 110, "A", "G", "ENSG_Z_PG")
    w.var("1", 200, "A", "G", "0|1"); w.note("1", 200, "A", "G", "ENSG_B"); w.note("1", 200, "A", "G", "ENSG_A")
    w.var("1", 210, "A", "G", "1|0"); w.note("1", 210, "A", "G", "ENSG_A"); w.note("1", 210, "A", "G", "ENSG_B")
    p = w.write(str(tmp_path))
    got = annotate.annotate(p["vcf"], SAMPLE, p["cadd"], _interactions=emu)
    assert list(dict.fromkeys(l.split("\t")[0] for l in got.split("\n")[1:-1])) == ["ENSG_B", "ENSG_A", "ENSG_Z_PG"]


def test_genotypes_that_are_not_two_digits_are_skipped_and_counted(tmp_path, emu):
    from phaser_amd import _lib, annotate
    _lib.build()
    w = literal_world()
    base = annotate.annotate(w.write(str(tmp_path))["vcf"], SAMPLE, os.path.join(str(tmp_path), "cadd.tsv.gz"), _interactions=emu)
    w.var("1", 700, "A", "G", "1"); w.note("1", 700, "A", "G", "ENSG01")
    w.var("1", 710, "A", "G", "1|10", "10|1", "1"); w.note("1", 710, "A", "G", "ENSG01")
    w.var("1", 720, "A", "G", "0/1", "1|1|1", "1"); w.note("1", 720, "A", "G", "ENSG01")
    w.var("1", 730, "A", "G", "0/1"); w.note("1", 730, "A", "G", "ENSG01")                          # not eligible at all: not counted
    p = w.write(str(tmp_path))
    logs = []
    assert annotate.annotate(p["vcf"], SAMPLE, p["cadd"], log=logs.append, _interactions=emu) == base
    assert [l for l in logs if "skipped" in l] == ["     4 genotype(s) that are not two single-digit alleles were skipped"]


def test_no_na_gene_is_no_error_and_an_na_gene_is_never_reported(tmp_path, emu):
    from phaser_amd import _lib, annotate
    _lib.build()
    w = literal_world()
    assert "NA" not in {r[92] for r in w.cadd}
    base = annotate.annotate(w.write(str(tmp_path))["vcf"], SAMPLE, os.path.join(str(tmp_path), "cadd.tsv.gz"), _interactions=emu)
    assert base == literal_text(False)
    w.note("1", 100, "A", "G", "NA"); w.note("1", 200, "C", "T", "NA")
    w.cadd.sort(key=lambda r: int(r[1]))
    p = w.write(str(tmp_path))
    assert annotate.annotate(p["vcf"], SAMPLE, p["cadd"], _interactions=emu) == base


def test_missing_output_and_unknown_sample_give_the_reference_message_and_status_1(tmp_path, emu, capsys):
    from phaser_amd import _lib, annotate
    _lib.build()
    p = literal_world().write(str(tmp_path))
    assert annotate.main(["--geno_vcf", p["vcf"], "--sample", SAMPLE, "--cadd_file", p["cadd"]]) == 1
    assert "Error: please specify an output directory." in capsys.readouterr().out
    out = os.path.join(str(tmp_path), "o.txt")
    assert annotate.main(["--geno_vcf", p["vcf"], "--sample", "nobody", "--cadd_file", p["cadd"], "--o", out], _interactions=emu) == 1
    assert "Error sample not found in VCF." in capsys.readouterr().out and not os.path.exists(out)
    assert annotate.main(["--geno_vcf", p["vcf"], "--sample", SAMPLE, "--cadd_file", p["cadd"], "--o", out], _interactions=emu) == 0
    assert open(out).read() == literal_text(False)
    banner = capsys.readouterr().out
    assert "1. Reading VCF..." in banner and "4. Identifying cases of compound heterozygosity..." in banner and "20 rows" in banner


def test_af_list_shorter_than_the_alt_index_gives_a_dot(tmp_path, emu):
    from phaser_amd import _lib, annotate
    _lib.build()
    w = literal_world()
    w.vcf = [l.replace("AF=0.4,0.04", "AF=0.4") for l in w.vcf]
    p = w.write(str(tmp_path))
    got = annotate.annotate(p["vcf"], SAMPLE, p["cadd"], _interactions=emu)
    assert got == literal_text(False).replace("\t2\t0.04\t", "\t2\t.\t") and got != literal_text(False)


def test_gz_genotype_vcf_is_read_as_text(tmp_path, emu):
    from phaser_amd import _lib, annotate
    _lib.build()
    p = literal_world().write(str(tmp_path), gz_vcf=True)
    assert p["vcf"].endswith(".gz") and annotate.annotate(p["vcf"], SAMPLE, p["cadd"], _interactions=emu) == literal_text(False)


def test_contig_absent_from_the_tables_gives_no_annotation_and_af_zero(tmp_path, emu):
    from phaser_amd import _lib, annotate
    _lib.build()
    w = literal_world()
    w.var("9", 5, "A", "G", "0|1")
    w.af = [l for l in w.af if not l.startswith("1\t100\t")]
    p = w.write(str(tmp_path))
    assert annotate.annotate(p["vcf"], SAMPLE, p["cadd"], _interactions=emu) == literal_text(False)
    assert annotate.annotate(p["vcf"], SAMPLE, p["cadd"], af_vcf=p["af"], _interactions=emu) == literal_text(True).replace("\t0.11\t", "\t0\t")


def test_product_path_needs_a_gpu(tmp_path):
    import torch
    from phaser_amd import _lib, annotate
    _lib.build()
    if torch.cuda.is_available():
        return
    p = literal_world().write(str(tmp_path))
    with pytest.raises(_lib.PhzError):
        annotate.annotate(p["vcf"], SAMPLE, p["cadd"])


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    from phaser_amd import _lib, annotate
    ctx = _lib.Context(0)
    yield lambda ai, batch_rows=0, stats=None: annotate.annot_pairs(ctx.lib, ctx.h, ai, batch_rows, stats)
    ctx.close()


@pytest.mark.gpu
def test_kannot_gpu_small_shapes_match_restatement(gpu):
    for w in (small_world(), literal_world()):
        want = R.record_tuples(R.all_rows(R.build_tables(w.vcf_text, SAMPLE, w.cadd_rows())))
        ai, _ = product_input(w)
        assert record_tuples(ai, gpu(ai)) == want
        for at in (0, 2, len(ai.genes)):
            ai0 = with_empty_gene(ai, at)
            assert record_tuples(ai0, gpu(ai0)) == want
    T = random_tables(3, n_genes=12, max_n=14)
    ai = tables_to_input(T)
    assert record_tuples(ai, gpu(ai)) == R.record_tuples(R.all_rows(T))


@pytest.mark.gpu
def test_kannot_gpu_random_genes_match_restatement(gpu):
    T, ai, want = random_case()
    stats = {}
    got = gpu(ai, stats=stats)
    assert stats["pairs"] == R.pair_count(T) and stats["batches"] == 1 and len(want) > 50000
    assert record_tuples(ai, got) == want


@pytest.mark.gpu
def test_kannot_gpu_batches_equal_one_launch(gpu):
    from phaser_amd import _lib
    T, ai, want = random_case()
    whole = gpu(ai)
    per_gene = np.bincount(whole["gene"], minlength=len(ai.genes))
    for cap in (int(per_gene.max()), len(whole) // 3 + int(per_gene.max())):
        stats = {}
        got = gpu(ai, batch_rows=cap, stats=stats)
        assert stats["batches"] >= 3 and np.array_equal(got, whole)
    assert record_tuples(ai, whole) == want
    with pytest.raises(_lib.PhzError) as e:
        gpu(ai, batch_rows=int(per_gene.max()) - 1)
    assert e.value.status == _lib.PHZ_E_CAPACITY


_BIG = {}


def big_case():
    """500 genes: more than 4,096 tiles of 256 pairs, so the scan of a whole batch's tile counts runs over more than one chunk.  Computed once, never changed"""
    if not _BIG:
        T = random_tables(13, n_genes=500)
        _BIG.update(T=T, ai=tables_to_input(T), want=R.record_tuples(R.all_rows(T)))
    return _BIG["T"], _BIG["ai"], _BIG["want"]


@pytest.mark.gpu
def test_kannot_gpu_one_batch_of_more_than_one_scan_chunk(gpu):
    T, ai, want = big_case()
    stats = {}
    got = gpu(ai, stats=stats)
    assert stats["pairs"] == R.pair_count(T) and stats["pairs"] > 4096 * 256 and stats["batches"] == 1
    assert record_tuples(ai, got) == want


@pytest.mark.gpu
def test_kannot_gpu_batches_that_start_at_any_tile(gpu):
    """every batch but the first hands the scan `tile_count + t0`: a base pointer that is 16-byte aligned or not as t0 falls"""
    T, ai, want = big_case()
    import collections
    largest = max(collections.Counter(t[0] for t in want).values())          # rows of the largest gene: the smallest capacity the entry accepts
    for cap in (largest, len(want) // 3 + largest):
        stats = {}
        got = gpu(ai, batch_rows=cap, stats=stats)
        assert stats["batches"] >= 3
        assert record_tuples(ai, got) == want


@pytest.mark.gpu
def test_kannot_gpu_second_smaller_call_on_one_context(gpu):
    T, ai, want = random_case()
    assert record_tuples(ai, gpu(ai)) == want
    w = small_world()
    small, _ = product_input(w)
    small_want = R.record_tuples(R.all_rows(R.build_tables(w.vcf_text, SAMPLE, w.cadd_rows())))
    assert record_tuples(small, gpu(small)) == small_want            # stale tile counts / bases / records of the larger call must not show
    lit, _ = product_input(literal_world())
    assert len(gpu(lit)) == 20
    assert record_tuples(ai, gpu(ai, batch_rows=len(want) // 2)) == want


@pytest.mark.gpu
@pytest.mark.parametrize("af_vcf", [False, True])
def test_annotate_gpu_cli_from_files(tmp_path, capsys, af_vcf):
    from phaser_amd import annotate
    w = small_world()
    p = w.write(str(tmp_path))
    T = R.build_tables(w.vcf_text, SAMPLE, w.cadd_rows(), w.af_rows() if af_vcf else None)
    outs = []
    for k in range(2):
        o = os.path.join(str(tmp_path), "out%d.txt" % k)
        argv = ["--geno_vcf", p["vcf"], "--sample", SAMPLE, "--cadd_file", p["cadd"], "--o", o, "--threads", "2"] + (["--af_vcf", p["af"]] if af_vcf else [])
        assert annotate.main(argv) == 0
        outs.append(open(o, "rb").read())
    assert outs[0] == outs[1] == R.text_of(R.all_rows(T)).encode()
    assert "K_annot" in capsys.readouterr().out
