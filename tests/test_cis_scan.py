"""phaser_cis_scan (phaser_amd/cis_scan.py; K_cisscan in phaser_amd/csrc/phz_cisscan.hip; phz_vcf_region_classes in phz_vcflookup.cpp).

Every kernel comparison is equality of integers against the plain-Python restatement (cis_scan_restatement.py: U2 by counting pairs, T as Fractions, the
Philox stream and the replicate orders restated).  CPU tests: the kernels under the host emulation in two builds -- the product macros and PHZ_CISSCAN_GRID=3
(every kernel strides over its work) -- on one designed call; the uniformity of the restated stream; a planted gene; the VCF reader against a plain-Python
reader; the tool on the emulated kernels against the restated pipeline and against cis_var; the errors.  GPU tests: the designed call, PHZ_DEVICE against
PHZ_HOST, the timing slot, one gene at n = S = 4096, the refusal of S = 4097, the command line as a child process."""
import ctypes as C
import functools
import gzip
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import cis_scan_restatement as R

HIPEMU = os.path.join(REPO, "tests", "hipemu")
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
EMU_DIR = os.path.join(HIPEMU, "_build", "cisscan")
BUILDS = {"product": [], "grid_3": ["-DPHZ_CISSCAN_GRID=3"]}
DESIGN_SEED = 5
COMBOS = [(mh, mm, P) for (mh, mm) in ((1, 1), (5, 5)) for P in (0, 1, R.DESIGN_P)]


# ------------------------------------------------------------------------------------------------ the kernels under the emulation
def _emu_lib(tag):
    from phaser_amd import _lib
    os.makedirs(EMU_DIR, exist_ok=True)
    lib = os.path.join(EMU_DIR, "libphz_cisscan_%s.so" % tag)
    srcs = [os.path.join(CSRC, "phz_api.hip"), os.path.join(CSRC, "phz_aetest.hip"), os.path.join(CSRC, "phz_cisscan.hip"), os.path.join(HIPEMU, "hipemu.cpp")]
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(REPO, "include", "phz.h"), os.path.join(HIPEMU, "hipemu.h")]
    newest = max(os.path.getmtime(p) for p in srcs + hdrs)
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        import fcntl
        with open(os.path.join(EMU_DIR, ".lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            flags = ["-O1", "-std=c++17", "-fPIC", "-I" + os.path.join(HIPEMU, "include"), "-I" + os.path.join(REPO, "include"), "-I" + CSRC]
            objs = []
            for src in srcs:
                obj = os.path.join(EMU_DIR, "%s_%s.o" % (os.path.basename(src), tag)); objs.append(obj)
                lang = [] if src.endswith(".cpp") else ["-x", "c++"]
                subprocess.check_call(["g++"] + flags + BUILDS[tag] + lang + ["-c", src, "-o", obj])
            subprocess.check_call(["g++", "-shared", "-fPIC"] + objs + ["-o", lib + ".tmp", "-lpthread"])
            os.replace(lib + ".tmp", lib)
    L = C.CDLL(lib)
    for name in ("phz_ctx_create", "phz_ctx_destroy", "phz_last_error", "phz_strerror", "phz_bh_adjust", "phz_cis_scan"):
        res, args = _lib.SYMBOLS[name]
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


class EmuCtx:
    """what cis_scan needs of a _lib.Context, on an emulated library"""

    def __init__(self, tag):
        self.lib = _emu_lib(tag)
        self.h = C.c_void_p()
        assert self.lib.phz_ctx_create(0, C.byref(self.h)) == 0

    def close(self):
        self.lib.phz_ctx_destroy(self.h)


@pytest.fixture(scope="module")
def emus():
    from phaser_amd import _lib
    _lib.build()
    ctxs = {tag: EmuCtx(tag) for tag in BUILDS}
    yield ctxs
    for c in ctxs.values():
        c.close()


# ------------------------------------------------------------------------------------------------ 1. the designed call
def _scan_input(cls, genes, S, min_het, min_hom, P, seed):
    """a restatement-style gene list -> cis_scan.ScanInput"""
    from phaser_amd import cis_scan as cs
    G = len(genes)
    covered = np.zeros((G, S), dtype=bool); val = np.zeros((G, S))
    for g, ge in enumerate(genes):
        for s in ge["covered"]:
            covered[g, s] = True; val[g, s] = ge["value"][s]
    return cs.ScanInput(np.array(cls, dtype=np.uint8).reshape(len(cls), S), covered, val, [ge["v_lo"] for ge in genes], [ge["v_hi"] for ge in genes],
                        [ge["subseq"] for ge in genes], min_het, min_hom, P, seed)


def _restated_outputs(genes, ref, min_het, min_hom, P):
    """-> the five output arrays of phz_cis_scan from the restated counts"""
    nh = np.array([x for r in ref for x in r[0]], dtype=np.int32); nm = np.array([x for r in ref for x in r[1]], dtype=np.int32)
    u2 = np.array([x for r in ref for x in r[2]], dtype=np.int64)
    best, exceed = [], []
    for ge, r in zip(genes, ref):
        b, e = R.best_and_exceed(r[0], r[1], r[2], r[3], min_het, min_hom, P)
        best.append(-1 if b < 0 else ge["v_lo"] + b); exceed.append(e)
    return nh, nm, u2, np.array(best, dtype=np.int32), np.array(exceed, dtype=np.int32)


def _assert_designed_call(lib, handle, what, combos=COMBOS):
    """-> {combo: output arrays}, each equal to the restatement"""
    from phaser_amd import cis_scan as cs
    d = R.designed_call(); ref = R.designed_reference(DESIGN_SEED)
    got = {}
    for mh, mm, P in combos:
        si = _scan_input(d["cls"], d["genes"], R.DESIGN_S, mh, mm, P, DESIGN_SEED)
        out = cs.cis_scan_call(lib, handle, si)
        want = _restated_outputs(d["genes"], ref, mh, mm, P)
        for name, o, w in zip(("n_het", "n_hom", "u2", "best_v", "exceed"), out, want):
            assert o.dtype == w.dtype and np.array_equal(o, w), (what, mh, mm, P, name, np.nonzero(o != w)[0][:8] if o.shape == w.shape else (o.shape, w.shape))
        got[(mh, mm, P)] = out
    return got


def test_designed_call_holds_what_it_is_meant_to():
    d = R.designed_call(); ref = R.designed_reference(DESIGN_SEED)
    genes, cls = d["genes"], d["cls"]
    assert [len(g["covered"]) for g in genes[:11]] == [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 130] and len(cls) == R.DESIGN_V
    sv = sorted(genes[11]["value"].values())
    assert len(set(sv[60:71])) == 1 and sv[59] < sv[60] and sv[70] < sv[71]                     # one run spans positions 60-70
    assert len(set(genes[12]["value"].values())) == 1 and len(set(genes[13]["value"].values())) == 90
    assert genes[14]["v_lo"] == genes[14]["v_hi"] and genes[15]["v_hi"] - genes[15]["v_lo"] == 1
    assert any(len(set(g["value"].values())) < len(g["value"]) for g in genes[4:11])            # tie runs exist
    _, _, _, best, exceed = _restated_outputs(genes, ref, 1, 1, R.DESIGN_P)
    assert best[16] == -1 and exceed[16] == 0 and best[0] == -1 and best[14] == -1              # no testable pair
    assert best[17] == 10 and cls[10] == cls[14] and (genes[17]["v_lo"], genes[17]["v_hi"]) == (8, 16)      # two variants with equal T: the first wins
    r = ref[17]
    assert R.t_stat(r[2][2], r[0][2], r[1][2]) == R.t_stat(r[2][6], r[0][6], r[1][6])
    b5 = _restated_outputs(genes, ref, 5, 5, R.DESIGN_P)[3]
    assert np.any(best != b5) and np.any(exceed > 0) and np.any((exceed < R.DESIGN_P) & (best >= 0))


def test_designed_call_emulated_matches_restatement_in_both_builds_and_two_runs(emus):
    first = _assert_designed_call(emus["product"].lib, emus["product"].h, "emulated product")
    for tag, what in (("grid_3", "emulated grid_3"), ("product", "emulated product, second run")):
        again = _assert_designed_call(emus[tag].lib, emus[tag].h, what)
        for k in first:
            assert all(np.array_equal(x, y) for x, y in zip(first[k], again[k])), (what, k)


# ------------------------------------------------------------------------------------------------ 2. the restated stream
def test_restated_stream_orders_are_uniform():
    """n = 4, 24,000 replicates of one gene at seed 0: each of the 24 orders occurs 1000 +- 155 times (five standard deviations of Binomial(24000, 1/24))"""
    counts = {}
    for b in range(24000):
        o = tuple(R.replicate_order(b, 4, 0, 0))
        counts[o] = counts.get(o, 0) + 1
    assert len(counts) == 24 and set(counts) == set(itertools.permutations(range(4)))
    print("orders: min %d max %d" % (min(counts.values()), max(counts.values())))
    assert all(abs(c - 1000) <= 155 for c in counts.values()), counts


def test_restated_philox_is_the_published_one():
    """known-answer vectors of Philox4x32-10 (Random123's kat_vectors)"""
    assert R.philox4x32_10(0, 0, 0) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert R.philox4x32_10(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)


# ------------------------------------------------------------------------------------------------ 3. a planted gene
def test_planted_gene_is_found_and_never_reached(emus):
    import random
    from phaser_amd import cis_scan as cs
    rnd = random.Random(3)
    S, V, planted = 60, 12, 7
    cls = [[rnd.choice((1, 2)) for _ in range(S)] for _ in range(V)]
    value = {s: (2.0 + rnd.random() if cls[planted][s] == 1 else 0.5 * rnd.random()) for s in range(S)}
    genes = [{"covered": list(range(S)), "value": value, "v_lo": 0, "v_hi": V, "subseq": 0}]
    for tag in BUILDS:
        nh, nm, u2, best, exceed = cs.cis_scan_call(emus[tag].lib, emus[tag].h, _scan_input(cls, genes, S, 5, 5, 99, 0))
        assert best[0] == planted and exceed[0] == 0, (tag, best, exceed)
        assert u2[planted] == 2 * int(nh[planted]) * int(nm[planted])


# ------------------------------------------------------------------------------------------------ 4. phz_vcf_region_classes
GTS = ["0|1", "1|0", "0/1", "1|1", "0|0", ".|.", "0|2", "1|2", "0|10", "1|10", "2|1", "."]
VCF_SAMPLES = ["s%02d" % i for i in range(len(GTS))]


def _class_vcf_text():
    lines = ["##fileformat=VCFv4.2", "##contig=<ID=chr1>", "##contig=<ID=chr2>", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(VCF_SAMPLES)]
    k = 0
    for chrom, positions in (("chr1", list(range(100, 40000, 1700)) + [40000, 40000]), ("chr2", [5, 16384, 16385, 70000, 900000])):
        for pos in positions:
            rot = GTS[k % len(GTS):] + GTS[:k % len(GTS)]
            if k % 7 == 3:
                lines.append("%s\t%d\t.\tA\tG\t.\tPASS\t.\tDP\t%s" % (chrom, pos, "\t".join("9" for _ in rot)))                     # no GT in FORMAT
            elif k % 5 == 1:
                lines.append("%s\t%d\trs%d\tC\tT\t.\tPASS\t.\tDP:GT:GQ\t%s" % (chrom, pos, k, "\t".join("7:%s:30" % g for g in rot)))
            else:
                lines.append("%s\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t%s" % (chrom, pos, "\t".join(rot)))
            k += 1
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def class_vcf(tmp_path_factory):
    from phaser_amd import vcfout
    d = tmp_path_factory.mktemp("classvcf")
    text = _class_vcf_text()
    indexed = os.path.join(str(d), "with.vcf.gz"); bare = os.path.join(str(d), "bare.vcf.gz")
    assert vcfout.write_bgzf(indexed, text, 1, index="vcf")
    vcfout.write_bgzf(bare, text, 1)
    assert os.path.exists(indexed + ".tbi") and not os.path.exists(bare + ".tbi")
    return text, indexed, bare


def test_class_codes_are_cis_vars_for_every_gt():
    from phaser_amd.cis_var import _classify
    want = {"0|1": (1, 1), "1|0": (1, 0), "0/1": (0, 0), "1|1": (2, 0), "0|0": (2, 0), ".|.": (0, 0), "0|2": (0, 0), "1|2": (0, 0), "0|10": (0, 0), "1|10": (1, 0),
            "2|1": (0, 0), ".": (0, 0)}
    for gt in GTS:
        c, ai = _classify(gt) if "|" in gt else (0, 0)
        assert R.classify(gt) == (c, ai if c == 1 else 0) == want[gt], gt


REGION_CASES = {
    "one": [("chr1", 1, 10000)],
    "overlapping": [("chr1", 1000, 9000), ("chr1", 5000, 20000), ("chr1", 5100, 5200), ("chr2", 16385, 70000), ("chr2", 1, 16385)],
    "no_records": [("chr1", 101, 1799), ("chr2", 6, 16383)],
    "absent_contig": [("chrZ", 1, 100000), ("chr1", 39000, 41000)],
    "everything": [("chr1", -500, 2 ** 40), ("chr2", 1, 2 ** 31)],
    "none": [],
    "empty_interval": [("chr1", 500, 400)],
}


@pytest.mark.parametrize("case", list(REGION_CASES))
def test_region_classes_indexed_scan_and_plain_python_agree(class_vcf, case):
    from phaser_amd import cis_scan as cs
    text, indexed, bare = class_vcf
    regions = REGION_CASES[case]
    samples = VCF_SAMPLES[::-1] + ["absent_from_the_file", VCF_SAMPLES[0]]
    want = R.region_records(text, regions, samples)
    outs = [cs.region_classes(indexed, regions, samples, threads=t, use_index=u) for t, u in ((1, True), (3, True), (1, False))] + \
           [cs.region_classes(bare, regions, samples, threads=2, use_index=True)]
    for recs, codes, contigs in outs:
        assert [r[:5] for r in recs] == [w[:5] for w in want] and contigs == {"chr1", "chr2"}
        assert codes.shape == (len(want), len(samples)) and codes.dtype == np.uint8
        assert codes.tolist() == [w[5] for w in want]
    if case == "everything":
        recs, codes, _ = outs[0]
        assert len(recs) == text.count("\nchr") and any(r[5] == -1 for r in recs) and any(r[5] == 1 for r in recs)
        assert sorted(set(codes.reshape(-1).tolist())) == [0, 1, 2, 5] and not codes[:, len(VCF_SAMPLES)].any()
        assert all(not codes[i].any() for i, r in enumerate(recs) if r[5] == -1)
    if case in ("no_records", "none", "empty_interval"):
        assert want == []
    if case == "overlapping":
        assert len({(r[0], r[1], r[2]) for r in outs[0][0]}) == len(outs[0][0]) > 8


# ------------------------------------------------------------------------------------------------ 5. the tool
TOOL_S = 40
TOOL_OPTS = dict(window=3000, min_cov=8, pc=1, min_het=4, min_hom=4, perm=19, seed=0, fdr=0.3)


@functools.lru_cache(maxsize=None)
def tool_texts():
    """-> (matrix text, VCF text, map text): 9 genes on two contigs, 40 mapped samples of which one is absent from the matrix and one from the VCF"""
    import random
    rnd = random.Random(11)
    vs = ["v%02d" % i for i in range(TOOL_S)]; bs = ["b%02d" % i for i in range(TOOL_S)]
    map_text = "vcf_sample\tbed_sample\n" + "".join("%s\t%s\n" % (v, b) for v, b in zip(vs, bs))
    vcf_cols = [v for v in vs if v != "v05"] + ["extra"]
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(vcf_cols)]
    variants = {}
    k = 0
    for chrom in ("chr1", "chr2"):
        for pos in sorted(rnd.sample(range(1000, 30000), 36)):
            gts = [rnd.choice(("0|1", "1|0", "0|0", "1|1", "1|1", "0|0", "0/1", ".|.")) for _ in vcf_cols]
            variants[(chrom, pos)] = dict(zip(vcf_cols, gts))
            lines.append("%s\t%d\t%s\tA\tG\t.\tPASS\t.\tGT:DP\t%s" % (chrom, pos, "." if k % 3 else "rs%d" % k, "\t".join(g + ":9" for g in gts)))
            k += 1
    bed_cols = [b for b in bs if b != "b11"] + ["unmapped"]
    rows = ["#contig\tstart\tstop\tname\t" + "\t".join(bed_cols)]
    planted = [(c, p) for (c, p) in variants if 8000 < p < 12000]
    for g in range(9):
        chrom = "chr1" if g < 5 else "chr2"
        start = 2000 + 6000 * (g % 5); stop = start + 2500
        cells = []
        plant = next(((c, p) for (c, p) in planted if c == chrom and start - 2000 < p < stop + 2000), None) if g in (1, 6) else None
        for b in bed_cols:
            v = "v" + b[1:]
            if g == 8:
                cells.append("%d|%d" % (rnd.randrange(0, 3), rnd.randrange(0, 3)))      # too few covered samples: no testable pair
                continue
            if rnd.random() < 0.08:
                cells.append(rnd.choice(("", "3|", "0|0")))
                continue
            tot = rnd.randrange(10, 400)
            big = plant is not None and variants[plant].get(v) in ("0|1", "1|0")
            frac = (0.85 if variants[plant].get(v) == "1|0" else 0.15) if big else rnd.choice((0.45, 0.5, 0.5, 0.55))
            a = int(tot * frac)
            cells.append("%d|%d" % (a, tot - a))
        rows.append("%s\t%d\t%d\tgene%d.1\t%s" % (chrom, start, stop, g, "\t".join(cells)))
    return "\n".join(rows) + "\n", "\n".join(lines) + "\n", map_text


@pytest.fixture(scope="module")
def tool_files(tmp_path_factory):
    from phaser_amd import vcfout
    d = str(tmp_path_factory.mktemp("cistool"))
    bed, vcf, mp = tool_texts()
    paths = {"bed_plain": os.path.join(d, "m.bed"), "bed_gzip": os.path.join(d, "m.gzip.bed.gz"), "bed_bgzf": os.path.join(d, "m.bgzf.bed.gz"),
             "vcf": os.path.join(d, "pop.vcf.gz"), "vcf_noindex": os.path.join(d, "noindex.vcf.gz"), "map": os.path.join(d, "map.txt")}
    open(paths["bed_plain"], "w").write(bed); open(paths["map"], "w").write(mp)
    with gzip.GzipFile(paths["bed_gzip"], "wb", mtime=0) as f:
        f.write(bed.encode())
    vcfout.write_bgzf(paths["bed_bgzf"], bed, 1)
    assert vcfout.write_bgzf(paths["vcf"], vcf, 1, index="vcf")
    vcfout.write_bgzf(paths["vcf_noindex"], vcf, 1)
    return paths


@functools.lru_cache(maxsize=None)
def tool_restated(chrom="", perm=TOOL_OPTS["perm"], seed=0):
    bed, vcf, mp = tool_texts()
    kw = dict(TOOL_OPTS); kw.update(chrom=chrom, perm=perm, seed=seed)
    return R.restate_tool(bed, vcf, mp, **kw)


def _assert_tool_outputs(out, chrom="", perm=TOOL_OPTS["perm"], seed=0, pairs=False):
    from phaser_amd import cis_scan as cs
    rows, perm_ps, want_pairs = tool_restated(chrom, perm, seed)
    got = [l.split("\t") for l in out["genes"].split("\n")[1:] if l]
    assert out["genes"].split("\n")[0].split("\t") == cs.GENES_HEADER
    assert [g[:15] for g in got] == rows
    q = R.bh(perm_ps)
    sig = []
    for g, qq in zip(got, q):
        if qq is None:
            assert g[15] == "NA"
        else:
            assert abs(float(g[15]) - qq) <= 1e-12 * qq, (g, qq)
            if float(g[15]) <= TOOL_OPTS["fdr"]:
                sig.append("\t".join(g))
    assert out["significant"].split("\n")[1:-1] == sig
    if pairs:
        assert [l.split("\t") for l in out["pairs"].split("\n")[1:] if l] == want_pairs and out["pairs"].split("\n")[0].split("\t") == cs.PAIRS_HEADER
    else:
        assert out["pairs"] is None
    return got, sig


def test_tool_on_emulated_kernels_matches_restated_pipeline(emus, tool_files):
    from phaser_amd import cis_scan as cs
    emu = emus["product"]
    bed, vcf, mp = tool_texts()
    out = cs.cis_scan(bed, tool_files["vcf"], mp, ctx=emu, output_pairs=1, threads=2, **TOOL_OPTS)
    got, sig = _assert_tool_outputs(out, pairs=True)
    assert len(got) == 9 and got[8][5] == "0" and got[8][6:] == ["NA"] * 10                    # a gene without a testable pair
    assert 1 <= len(sig) < sum(1 for g in got if g[15] != "NA")                                # planted genes are found, others are not
    assert any(g[6].startswith("rs") for g in got) and any(g[6].startswith("chr") for g in got)
    assert cs.cis_scan(bed, tool_files["vcf"], mp, ctx=emu, output_pairs=1, threads=1, **TOOL_OPTS) == out          # a second run: equal bytes
    assert cs.cis_scan(bed, tool_files["vcf_noindex"], mp, ctx=emus["grid_3"], output_pairs=1, **TOOL_OPTS) == out  # no .tbi, the other build
    assert cs.cis_scan(bed, tool_files["vcf"], mp, ctx=emu, output_pairs=1, use_index=False, **TOOL_OPTS) == out
    # --chr
    one = cs.cis_scan(bed, tool_files["vcf"], mp, ctx=emu, chrom="chr2", **TOOL_OPTS)
    g2, _ = _assert_tool_outputs(one, chrom="chr2")
    assert [g[:15] for g in g2] == [g[:15] for g in got if g[1] == "chr2"] and len(g2) == 4   # subseq is the row number of the whole matrix
    # --perm 0
    kw = dict(TOOL_OPTS); kw["perm"] = 0
    p0 = cs.cis_scan(bed, tool_files["vcf"], mp, ctx=emu, **kw)
    g0, s0 = _assert_tool_outputs(p0, perm=0)
    assert all(g[13:] == ["NA"] * 3 for g in g0) and s0 == [] and [g[:13] for g in g0] == [g[:13] for g in got]
    # another seed changes the permutation columns alone
    kw = dict(TOOL_OPTS); kw["seed"] = 77
    other = cs.cis_scan(bed, tool_files["vcf"], mp, ctx=emu, output_pairs=1, **kw)
    go, _ = _assert_tool_outputs(other, seed=77, pairs=True)
    assert [g[:13] for g in go] == [g[:13] for g in got] and other["pairs"] == out["pairs"] and [g[13] for g in go] != [g[13] for g in got]


def test_best_pairs_agree_with_cis_var(emus, tool_files):
    """the best pairs of genes.txt as a --pairs file of phaser_amd.cis_var: the same strings in the columns both tools have"""
    from phaser_amd import cis_scan as cs, cis_var as cv
    bed, vcf, mp = tool_texts()
    out = cs.cis_scan(bed, tool_files["vcf"], mp, ctx=emus["product"], **TOOL_OPTS)
    got = [l.split("\t") for l in out["genes"].split("\n")[1:] if l and l.split("\t")[6] != "NA"]
    recs = {("%s_%d_%s_%s" % (r[0], r[1], r[3], r[4]) if r[2] == "." else r[2]): r for r in R.vcf_records(vcf)[1]}
    pairs = "gene_id\tvar_id\tvar_contig\tvar_pos\tvar_ref\tvar_alt\n" + "".join(
        "%s\t%s\t%s\t%d\t%s\t%s\n" % (g[0], g[6], recs[g[6]][0], recs[g[6]][1], recs[g[6]][3], recs[g[6]][4]) for g in got)
    hook = lambda bi: (np.zeros((bi.n_groups, 2, 4)), np.zeros((bi.n_groups, 2, 2), dtype=np.int64))
    body = cv.cis_var(bed, tool_files["vcf"], pairs, mp, pc=TOOL_OPTS["pc"], min_cov=TOOL_OPTS["min_cov"], bs=10, _bootstrap=hook)
    rows = [dict(zip(cv.COLUMNS, l.split("\t"))) for l in body.split("\n")[1:] if l]
    assert len(rows) == len(got) >= 6
    for g, r in zip(got, rows):
        assert (r["gene"], r["var_het_n"], r["var_hom_n"], r["het_hom_pvalue"], r["var_het_afc"]) == (g[0], g[8], g[9], g[11], g[12]), (g, r)


@pytest.mark.parametrize("bed,vcf", [("bed_plain", "vcf"), ("bed_gzip", "vcf_noindex"), ("bed_bgzf", "vcf")])
def test_cli_on_emulated_kernels(tmp_path, emus, tool_files, monkeypatch, capsys, bed, vcf):
    from phaser_amd import _lib, cis_scan as cs
    monkeypatch.setattr(_lib, "Context", lambda device=0: emus["product"])          # the command line makes its own context: here the emulated one
    runs = []
    for k in (0, 1):
        d = os.path.join(str(tmp_path), "run%d" % k); os.makedirs(d)
        argv = ["--bed", tool_files[bed], "--vcf", tool_files[vcf], "--map", tool_files["map"], "--o", os.path.join(d, "out"), "--t", str(1 + k), "--output_pairs", "1"]
        for key, v in TOOL_OPTS.items():
            argv += ["--" + key, str(v)]
        assert cs.main(argv) == 0
        assert sorted(os.listdir(d)) == ["out.genes.txt", "out.pairs.txt.gz", "out.significant.txt", "out.summary.txt"]
        runs.append({x: open(os.path.join(d, x), "rb").read() for x in os.listdir(d)})
    assert runs[0] == runs[1]
    out = {k: runs[0]["out.%s.txt" % k].decode() for k in ("genes", "significant", "summary")}
    out["pairs"] = gzip.decompress(runs[0]["out.pairs.txt.gz"]).decode()
    _assert_tool_outputs(out, pairs=True)
    assert "genes\t9\n" in out["summary"] and "samples\t40\n" in out["summary"]


def test_pc_0_with_a_zero_count_is_fatal(emus, tool_files):
    from phaser_amd import cis_scan as cs
    from phaser_amd.cis_var import FatalError
    bed, vcf, mp = tool_texts()
    zero = bed.split("\n")
    f = zero[2].split("\t"); f[6] = "12|0"; zero[2] = "\t".join(f)
    kw = dict(TOOL_OPTS); kw["pc"] = 0
    with pytest.raises(FatalError, match="a haplotype count of 0 with --pc 0"):
        cs.cis_scan("\n".join(zero), tool_files["vcf"], mp, ctx=emus["product"], **kw)


@pytest.mark.parametrize("n,what", [(0, "holds no sample"), (4097, "at most 4096 are supported")])
def test_a_map_without_samples_or_with_too_many_is_fatal(n, what):
    from phaser_amd import cis_scan as cs
    from phaser_amd.cis_var import FatalError
    mp = "vcf_sample\tbed_sample\n" + "".join("v%d\tb%d\n" % (i, i) for i in range(n))
    with pytest.raises(FatalError, match=what):
        cs.cis_scan(tool_texts()[0], "never_opened.vcf.gz", mp, ctx=object(), **TOOL_OPTS)


@pytest.mark.parametrize("argv,line", [(["--min_het", "0"], "FATAL ERROR - --min_het and --min_hom must be at least 1"),
                                       (["--min_hom", "-2"], "FATAL ERROR - --min_het and --min_hom must be at least 1"),
                                       (["--perm", "-1"], "FATAL ERROR - --perm must lie between 0 and 2^31 - 2"),
                                       (["--window", "-5"], "FATAL ERROR - --window must not be negative"),
                                       (["--fdr", "1.5"], "FATAL ERROR - --fdr must lie between 0 and 1"),
                                       (["--pc", "-1"], "FATAL ERROR - --pc and --min_cov must not be negative"),
                                       (["--perm", "many"], "FATAL ERROR - argument --perm: invalid int value: 'many'")])
def test_bad_options_print_one_line_and_exit_1(tmp_path, tool_files, capsys, argv, line):
    from phaser_amd import cis_scan as cs
    base = ["--bed", tool_files["bed_plain"], "--vcf", tool_files["vcf"], "--map", tool_files["map"], "--o", os.path.join(str(tmp_path), "out")]
    try:
        status = cs.main(base + argv)
    except SystemExit as e:
        status = e.code
    assert status == 1
    assert [l for l in capsys.readouterr().out.split("\n") if l] == [line]
    assert os.listdir(str(tmp_path)) == []


def _assert_argument_errors(lib, handle):
    from phaser_amd import _lib, cis_scan as cs
    d = R.designed_call()
    genes = d["genes"][3:8]

    def call(change, status=_lib.PHZ_E_ARG, S=R.DESIGN_S, cls=d["cls"]):
        si = _scan_input(cls, genes, S, 1, 1, 2, 0)
        change(si)
        s = si.struct()
        P = int(si.pair_off[-1])
        outs = [np.full(P, -7, np.int32), np.full(P, -7, np.int32), np.full(P, -7, np.int64), np.full(len(genes), -7, np.int32), np.full(len(genes), -7, np.int32)]
        st = lib.phz_cis_scan(handle, C.byref(s), *[C.c_void_p(o.ctypes.data) for o in outs], _lib.PHZ_HOST)
        assert st == status, (st, status)
        if status != _lib.PHZ_OK:
            assert (lib.phz_last_error(handle) or b"").startswith(b"phz_cis_scan: ")
            assert all((o == -7).all() for o in outs)                    # the outputs are untouched

    call(lambda si: None, _lib.PHZ_OK)

    def set_(name, idx, v):
        def f(si):
            getattr(si, name)[idx] = v
        return f
    call(set_("g_off", 2, 1))                                            # offsets not ascending
    call(set_("order", 5, R.DESIGN_S))                                   # a sample index >= S
    call(set_("covered", 0, 60000))
    call(lambda si: si.cls.__setitem__((3, 4), 3))                       # a class above 2
    call(set_("v_hi", 1, R.DESIGN_V + 1)); call(set_("v_lo", 1, -1)); call(set_("v_lo", 0, R.DESIGN_V + 1))      # a variant range outside [0, V]
    call(set_("run_last", 4, 0)); call(set_("run_first", 10, 11)); call(set_("run_last", 66, 200))     # run bounds that are not runs
    call(lambda si: setattr(si, "n_perm", -1)); call(lambda si: setattr(si, "min_het", 0)); call(lambda si: setattr(si, "min_hom", 0))
    big = np.zeros((1, _lib.PHZ_CISSCAN_MAX_S + 1), dtype=np.uint8)
    si = cs.ScanInput(big, np.ones((1, big.shape[1]), bool), np.zeros((1, big.shape[1])), [0], [1], [0], 1, 1, 0, 0)
    s = si.struct()
    o = [np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.int32)]
    assert lib.phz_cis_scan(handle, C.byref(s), *[C.c_void_p(x.ctypes.data) for x in o], _lib.PHZ_HOST) == _lib.PHZ_E_UNSUPPORTED      # S = 4097
    # more than 2^31 - 1 pairs: two genes that each claim 2^30 + 1 variants of a table nobody has to allocate (the check comes before any read of cls)
    si = _scan_input(d["cls"], genes[:2], R.DESIGN_S, 1, 1, 0, 0)
    s = si.struct(); s.n_vars = 2 ** 30 + 1
    si.v_lo[:] = 0; si.v_hi[:] = 2 ** 30 + 1
    assert lib.phz_cis_scan(handle, C.byref(s), None, None, None, C.c_void_p(o[3].ctypes.data), C.c_void_p(o[4].ctypes.data), _lib.PHZ_HOST) == _lib.PHZ_E_ARG
    assert b"2^31 - 1 pairs" in lib.phz_last_error(handle)


def test_argument_errors_of_the_abi_emulated(emus):
    _assert_argument_errors(emus["product"].lib, emus["product"].h)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_designed_call_gpu_matches_restatement_host_and_device_space(gpu_ctx):
    import torch
    from phaser_amd import _lib
    gpu_ctx.reset_timing()
    host = _assert_designed_call(gpu_ctx.lib, gpu_ctx.h, "gpu")
    last, total, launches = gpu_ctx.timing(_lib.PHZ_T_CISSCAN)
    assert launches == len(COMBOS) and last > 0 and total > 0                                 # the timing slot
    dev = torch.device("cuda", gpu_ctx.device)
    d = R.designed_call()
    for (mh, mm, P), want in host.items():
        si = _scan_input(d["cls"], d["genes"], R.DESIGN_S, mh, mm, P, DESIGN_SEED)
        s = si.struct()
        keep = {}
        for name in ("cls", "g_off", "covered", "order", "run_first", "run_last", "v_lo", "v_hi", "subseq"):
            keep[name] = torch.from_numpy(np.ascontiguousarray(getattr(si, name)).view(np.uint8).reshape(-1).copy()).to(dev)
            setattr(s, name, keep[name].data_ptr())
        outs = [torch.full((w.nbytes,), 0xA5, dtype=torch.uint8, device=dev) for w in want]
        torch.cuda.synchronize(dev)
        gpu_ctx.check(gpu_ctx.lib.phz_cis_scan(gpu_ctx.h, C.byref(s), *[C.c_void_p(t.data_ptr()) for t in outs], _lib.PHZ_DEVICE))
        for t, w in zip(outs, want):
            assert np.array_equal(t.cpu().numpy().view(w.dtype), w), (mh, mm, P)


@pytest.mark.gpu
def test_one_gene_at_the_largest_sample_count_gpu(gpu_ctx):
    """n = S = 4096, 3 variants, P = 2; the variants are sparse on one side so that the restated pair count stays small"""
    import random
    from phaser_amd import _lib, cis_scan as cs
    rnd = random.Random(4096)
    S = _lib.PHZ_CISSCAN_MAX_S
    cls = [[1 if s % 137 == 5 else 2 for s in range(S)], [2 if s % 131 == 7 else 1 for s in range(S)], [rnd.choice((0,) * 12 + (1, 2)) for _ in range(S)]]
    value = {s: rnd.choice(R.LEVELS) + (0.001 * rnd.randrange(50) if s % 3 else 0.0) for s in range(S)}
    genes = [{"covered": list(range(S)), "value": value, "v_lo": 0, "v_hi": 3, "subseq": 9}]
    ref = [R.scan_gene(cls, genes[0]["covered"], value, 9, 2, 1)]
    got = cs.cis_scan_call(gpu_ctx.lib, gpu_ctx.h, _scan_input(cls, genes, S, 5, 5, 2, 1))
    want = _restated_outputs(genes, ref, 5, 5, 2)
    assert want[3][0] >= 0 and min(want[0].min(), want[1].min()) >= 5
    for name, o, w in zip(("n_het", "n_hom", "u2", "best_v", "exceed"), got, want):
        assert np.array_equal(o, w), (name, o, w)


@pytest.mark.gpu
def test_argument_errors_and_the_refusal_of_4097_samples_gpu(gpu_ctx):
    _assert_argument_errors(gpu_ctx.lib, gpu_ctx.h)


@pytest.mark.gpu
def test_cli_as_a_child_process_gpu(tmp_path, tool_files):
    runs = []
    for k in (0, 1):
        d = os.path.join(str(tmp_path), "run%d" % k); os.makedirs(d)
        argv = [sys.executable, "-m", "phaser_amd.cis_scan", "--bed", tool_files["bed_bgzf"], "--vcf", tool_files["vcf"], "--map", tool_files["map"],
                "--o", os.path.join(d, "out"), "--output_pairs", "1", "--t", str(1 + k)]
        for key, v in TOOL_OPTS.items():
            argv += ["--" + key, str(v)]
        done = subprocess.run(argv, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert done.returncode == 0, done.stdout.decode()
        assert b"K_cisscan" in done.stdout
        runs.append({x: open(os.path.join(d, x), "rb").read() for x in sorted(os.listdir(d))})
    assert runs[0] == runs[1] and sorted(runs[0]) == ["out.genes.txt", "out.pairs.txt.gz", "out.significant.txt", "out.summary.txt"]
    out = {k: runs[0]["out.%s.txt" % k].decode() for k in ("genes", "significant", "summary")}
    out["pairs"] = gzip.decompress(runs[0]["out.pairs.txt.gz"]).decode()
    _assert_tool_outputs(out, pairs=True)
