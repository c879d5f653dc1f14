"""phaser_sample_match (phaser_amd/sample_match.py; K_match in phaser_amd/csrc/phz_match.hip; phz_vcf_site_genotypes in phz_vcflookup.cpp).

CPU tests: K_match under the host emulation in three builds -- the product macros, PHZ_MATCH_GRID=3 (workgroups are reused) and PHZ_MATCH_TILE=5 (many tile
boundaries) -- bit for bit against the restatement (sample_match_restatement: Fraction terms, one add per entry) over the shape list; a sample alone and a
prefix of the donors alone; the argument errors and the skipped entries of the PHZ_DEVICE space; the VCF reader against a Python restatement on a designed
VCF; the whole tool on the emulated kernels against a plain Python restatement, byte for byte; detection of planted swaps on a seeded synthetic.
GPU tests: the shape list on the product kernels in both spaces, two runs, the CLI as a child process."""
import ctypes as C
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import sample_match_restatement as R

HIPEMU = os.path.join(REPO, "tests", "hipemu")
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
EMU_DIR = os.path.join(HIPEMU, "_build", "match")
BUILDS = {"product": [], "grid_3": ["-DPHZ_MATCH_GRID=3"], "tile_5": ["-DPHZ_MATCH_TILE=5"]}
TILE_OF = {"product": 256, "grid_3": 256, "tile_5": 5}
CAP, HET = 30, 100
LOG_REF, LOG_ALT = R.log_tables(0.01)


# ------------------------------------------------------------------------------------------------ the kernels under the emulation
def _emu_lib(tag):
    from phaser_amd import _lib
    os.makedirs(EMU_DIR, exist_ok=True)
    lib = os.path.join(EMU_DIR, "libphz_match_%s.so" % tag)
    srcs = [os.path.join(CSRC, "phz_api.hip"), os.path.join(CSRC, "phz_match.hip"), os.path.join(HIPEMU, "hipemu.cpp")]
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
    for name in ("phz_ctx_create", "phz_ctx_destroy", "phz_last_error", "phz_strerror", "phz_sample_match"):
        res, args = _lib.SYMBOLS[name]
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


class EmuCtx:
    """what sample_match needs of a _lib.Context, on an emulated library"""

    def __init__(self, tag):
        self.tag = tag
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


@pytest.fixture(scope="module", params=list(BUILDS))
def emu(request, emus):
    return emus[request.param]


def raw_call(lib, handle, geno, e_off, e_site, e_ref, e_alt, space=0, cap=CAP, het=HET, n_sites=None, n_samples=None, n_donors=None, ptr=None, out=None):
    """phz_sample_match on numpy arrays (ptr: how an array becomes a pointer) -> (status, loglik, n_called, n_match)"""
    from phaser_amd import _lib
    ptr = ptr or (lambda x: x.ctypes.data)
    arg = _lib.phz_match_in()
    arg.n_sites = geno.shape[0] if n_sites is None else n_sites
    arg.n_samples = len(e_off) - 1 if n_samples is None else n_samples
    arg.n_donors = geno.shape[1] if n_donors is None else n_donors
    arg.geno, arg.e_off, arg.e_site, arg.e_ref, arg.e_alt = (ptr(x) for x in (geno, e_off, e_site, e_ref, e_alt))
    arg.log_ref = (C.c_double * 3)(*LOG_REF); arg.log_alt = (C.c_double * 3)(*LOG_ALT)
    arg.cap, arg.het_permille = cap, het
    S, D = max(int(arg.n_samples), 0), max(int(arg.n_donors), 1)
    ll, nc, nm = out or (np.full((S, D), -5.0), np.full((S, D), -5, dtype=np.int32), np.full((S, D), -5, dtype=np.int32))
    st = lib.phz_sample_match(handle, C.byref(arg), C.c_void_p(ptr(ll)), C.c_void_p(ptr(nc)), C.c_void_p(ptr(nm)), space)
    return st, ll, nc, nm


@functools.lru_cache(maxsize=None)
def shape_reference(n_donors, entries, cap=CAP):
    """(inputs, restatement's outputs) of one shape, computed once and left unchanged"""
    case = R.shape_case(n_donors, list(entries))
    ref = R.match_reference(*case, LOG_REF, LOG_ALT, cap, HET)
    for x in case + ref:
        x.setflags(write=False)
    return case, ref


def shape_list(tile):
    return [(d, tuple(layout)) for d in R.DONOR_COUNTS for n in R.entry_counts(tile) for layout in R.sample_layouts(n)]


def same_bits(got, want):
    return (np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]))


def _assert_shapes_match_the_restatement(call, tile, what):
    """call(case) -> (loglik, n_called, n_match)"""
    shapes = shape_list(tile)
    assert len(shapes) == 11 * 7 * 3
    worst = 0
    for d, entries in shapes:
        case, ref = shape_reference(d, entries)
        got = call(case)
        assert same_bits(got, ref), (what, d, entries)
        worst = max(worst, int(ref[1].max()) if ref[1].size else 0)
    assert worst >= 600                                               # three codes of four are calls: of a thousand entries about 750 enter a donor's sum


def test_designed_counts_cover_the_contract():
    c = R.DESIGNED_COUNTS
    assert R.capped(1, 59, 30) == (1, 29) and (1 * 30 + 30) // 60 == 1                 # the rounding half
    assert R.capped(31, 0, 30) == (30, 0) and R.capped(30, 0, 30) == (30, 0) and R.capped(5, 3, 30) == (5, 3) and R.capped(1000, 1, 0) == (1000, 1)
    assert R.capped(R.I32, R.I32, 30) == (15, 15) and R.I32 * 30 + R.I32 > 2 ** 32     # a product beyond 32 bits
    assert R.observed(1, 9, 100) == 2 and R.observed(1, 10, 100) == 3 and R.observed(10, 1, 100) == 1 and R.observed(7, 7, 100) == 2
    assert R.observed(999, 9001, 100) == 3 and R.observed(1000, 9000, 100) == 2
    for want in ((1, 59), (0, 8), (8, 0), (R.I32, R.I32), (1, 9), (1, 10), (7, 7), (30, 0), (31, 0), (5, 3)):
        assert want in c
    case, ref = shape_reference(17, (1000,))
    assert (ref[1][:, 3] == 0).all() and (ref[0][:, 3] == 0).all() and ref[1][:, 0].max() > 0          # the all-no-call donor
    assert (case[0][11] == 0).all() and 11 in case[1 + 1].tolist()                                        # the all-no-call site is an entry
    t = R.entry_terms(3, 2, 0, LOG_REF, LOG_ALT)
    assert t[1] == 5 * LOG_REF[1] and t[0] < 0 and abs(t[0] - (3 * LOG_REF[0] + 2 * LOG_ALT[0])) < 1e-12


def test_kmatch_emulated_equals_the_restatement_bit_for_bit(emu):
    call = lambda case: raw_call(emu.lib, emu.h, *case)[1:]
    _assert_shapes_match_the_restatement(call, TILE_OF[emu.tag], emu.tag)
    for cap in (0, 1, 7):                                                              # cap 0: no cap at all
        case, ref = shape_reference(65, (2 * TILE_OF[emu.tag] + 3, 0, 40), cap)
        assert same_bits(raw_call(emu.lib, emu.h, *case, cap=cap)[1:], ref), cap


def _assert_independence(call):
    """a sample alone gives the bits it gives among others; the first 17 of 600 donors alone give the bits of their columns"""
    case, ref = shape_reference(600, (2, 1000, 5, 0, 1000, 1, 0))
    geno, e_off, e_site, e_ref, e_alt = case
    full = call(case)
    assert same_bits(full, ref)
    for s in (1, 3, 4, 6):
        lo, hi = int(e_off[s]), int(e_off[s + 1])
        alone = call((geno, np.array([0, hi - lo], dtype=np.int64), np.array(e_site[lo:hi]), np.array(e_ref[lo:hi]), np.array(e_alt[lo:hi])))
        assert same_bits(alone, tuple(x[s:s + 1] for x in full)), s
    few = call((np.ascontiguousarray(geno[:, :17]), e_off, e_site, e_ref, e_alt))
    assert same_bits(few, tuple(np.ascontiguousarray(x[:, :17]) for x in full))


def test_kmatch_emulated_sample_alone_and_donor_prefix(emu):
    _assert_independence(lambda case: raw_call(emu.lib, emu.h, *case)[1:])


def test_kmatch_argument_errors_and_skipped_entries(emu):
    from phaser_amd import _lib
    case, ref = shape_reference(17, (7, 0, 9))
    geno, e_off, e_site, e_ref, e_alt = (np.array(x) for x in case)
    untouched = lambda r: bool(np.all(r[1] == -5.0) and np.all(r[2] == -5) and np.all(r[3] == -5))
    bad_entries = []
    for k, (arr, value) in enumerate(((e_site, -1), (e_site, geno.shape[0]), (e_ref, -1), (e_alt, -2))):
        changed = [np.array(x) for x in (e_site, e_ref, e_alt)]
        changed[(0, 0, 1, 2)[k]][5 + k] = value                        # entries 5 to 8 (entry 4 is at the site without a call)
        bad_entries.append(changed)
    zero = [np.array(x) for x in (e_site, e_ref, e_alt)]; zero[1][12] = 0; zero[2][12] = 0          # total == 0
    bad_entries.append(zero)
    for changed in bad_entries:
        r = raw_call(emu.lib, emu.h, geno, e_off, *changed)
        assert r[0] == _lib.PHZ_E_ARG and b"entry" in emu.lib.phz_last_error(emu.h) and untouched(r)
        # the same arrays in the PHZ_DEVICE space: the entry is skipped
        r = raw_call(emu.lib, emu.h, geno, e_off, *changed, space=_lib.PHZ_DEVICE)
        assert r[0] == _lib.PHZ_OK and same_bits(r[1:], R.match_reference(geno, e_off, *changed, LOG_REF, LOG_ALT, CAP, HET))
        assert not same_bits(r[1:], ref)
    for off in ([1, 7, 16], [0, 9, 7], [0, -1, 16]):
        r = raw_call(emu.lib, emu.h, geno, np.array([off[0], off[1], off[1], off[2]], dtype=np.int64), e_site, e_ref, e_alt)
        assert r[0] == _lib.PHZ_E_ARG and b"e_off" in emu.lib.phz_last_error(emu.h) and untouched(r)
    for kw, text in ((dict(n_donors=0), b"n_donors"), (dict(n_donors=-3), b"n_donors"), (dict(het=0), b"het_permille"), (dict(het=501), b"het_permille"),
                     (dict(cap=-1), b"cap")):
        for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
            r = raw_call(emu.lib, emu.h, geno, e_off, e_site, e_ref, e_alt, space=space, **kw)
            assert r[0] == _lib.PHZ_E_ARG and text in emu.lib.phz_last_error(emu.h) and untouched(r), kw
    assert raw_call(emu.lib, emu.h, geno, e_off, e_site, e_ref, e_alt, space=7)[0] == _lib.PHZ_E_ARG
    assert raw_call(emu.lib, emu.h, geno, e_off, e_site, e_ref, e_alt, n_samples=-1)[0] == _lib.PHZ_E_ARG
    for het in (1, 500):
        r = raw_call(emu.lib, emu.h, geno, e_off, e_site, e_ref, e_alt, het=het)
        assert r[0] == _lib.PHZ_OK and same_bits(r[1:], R.match_reference(geno, e_off, e_site, e_ref, e_alt, LOG_REF, LOG_ALT, CAP, het))
    # zero samples, zero entries, zero sites
    r = raw_call(emu.lib, emu.h, geno, np.zeros(1, dtype=np.int64), e_site[:0], e_ref[:0], e_alt[:0])
    assert r[0] == _lib.PHZ_OK
    r = raw_call(emu.lib, emu.h, geno, np.zeros(4, dtype=np.int64), e_site[:0], e_ref[:0], e_alt[:0])
    assert r[0] == _lib.PHZ_OK and np.all(r[1].view(np.uint64) == 0) and np.all(r[2] == 0) and np.all(r[3] == 0)
    r = raw_call(emu.lib, emu.h, geno[:0], np.zeros(3, dtype=np.int64), e_site[:0], e_ref[:0], e_alt[:0])
    assert r[0] == _lib.PHZ_OK and r[1].shape == (2, 17) and np.all(r[1].view(np.uint64) == 0) and np.all(r[2] == 0)
    r = raw_call(emu.lib, emu.h, geno[:0], e_off, e_site, e_ref, e_alt, space=_lib.PHZ_DEVICE)                   # every entry is out of range
    assert r[0] == _lib.PHZ_OK and np.all(r[1].view(np.uint64) == 0) and np.all(r[2] == 0)
    assert raw_call(emu.lib, emu.h, geno[:0], e_off, e_site, e_ref, e_alt)[0] == _lib.PHZ_E_ARG


def test_match_call_wrapper(emus):
    from phaser_amd import sample_match
    emu = emus["product"]
    case, ref = shape_reference(65, (300, 0, 40))
    assert same_bits(sample_match.match_call(emu.lib, emu.h, *case, 0.01, CAP, HET), ref)
    assert sample_match.log_tables(0.01) == (LOG_REF, LOG_ALT)


# ------------------------------------------------------------------------------------------------ phz_vcf_site_genotypes
def designed_vcf():
    """-> (text, positions asked for).  Samples A B C D; D is asked for twice over and E is not in the header."""
    head = ["##fileformat=VCFv4.2", "##contig=<ID=1>", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT", "A", "B", "C", "D"])]
    rec = lambda c, p, i, r, a, fmt, *gt: "\t".join([c, str(p), i, r, a, ".", "PASS", "."] + ([fmt] if fmt is not None else []) + list(gt))
    lines = head + [
        rec("1", 100, "v1", "A", "G", "GT", "0/0", "0|1", "1|0", "1/1"),
        rec("1", 150, "skip", "A", "G", "GT", "1/1", "1/1", "1/1", "1/1"),                     # not asked for
        rec("1", 200, "v2", "C", "T", "GT", "./.", ".", "0", "1/2"),
        rec("1", 300, "v3", "G", "A", "GT", "0/2", "1", "1|1", ".|."),
        rec("1", 400, "v4", "T", "C", "GT:DP:GQ", "0/1:12:40", "1/1:3", "0|0", "1|0:9:9"),     # further subfields
        rec("1", 500, "v5", "T", "C", "DP:GT", "12:0/1", "3:1/1", "7", "4:0|0"),               # GT not first; C has fewer subfields than FORMAT
        rec("1", 600, "v6", "A", "C", "DP", "12", "3", "7", "4"),                              # FORMAT without GT
        rec("1", 700, "v7m", "A", "C,T", "GT", "0/1", "1/2", "2/2", "0/0"),                    # multi-allelic, then the biallelic record of the key
        rec("1", 700, "v7", "A", "C", "GT", "0/1", "1/1", "0/0", "0/1"),
        rec("1", 800, "v8", "G", "T", "GT", "1/1", "0/0", "0/1", "1/1"),                       # a duplicate record
        rec("1", 800, "v8", "G", "T", "GT", "0/0", "0/0", "0/0", "0/0"),
        rec("1", 900, "v9", "G", "T", "GT", "0/1/1", "0/", "/1", "00/1"),
        rec("1", 1000, "v10", "G", "T", "GT", "0/1"),                                          # a record that lacks sample columns
        rec("1", 70000, "far", "G", "T", "GT", "1|1", "0|0", "0|1", "1|0"),                    # another 16 kb window of the index
        rec("2", 100, "w1", "A", "G", "GT", "1|1", "1|0", "0|1", "0|0"),
        rec("2", 5000, "w2", "A", "G", "GT", "0|0", "0|0", "1|1", "1|1"),
    ]
    positions = [("1", 100), ("1", 200), ("1", 300), ("1", 400), ("1", 500), ("1", 600), ("1", 700), ("1", 800), ("1", 900), ("1", 1000), ("1", 70000), ("1", 123),
                 ("2", 100), ("2", 5000), ("7", 100), ("2", 100)]
    return "\n".join(lines) + "\n", positions


def test_vcf_site_genotypes_against_the_restatement(tmp_path):
    from phaser_amd import _lib, sample_match, vcfout
    _lib.build()
    text, positions = designed_vcf()
    indexed = os.path.join(str(tmp_path), "i.vcf.gz"); bare = os.path.join(str(tmp_path), "b.vcf.gz")
    assert vcfout.write_bgzf(indexed, text, 1, index="vcf")
    vcfout.write_bgzf(bare, text, 1)
    assert os.path.exists(indexed + ".tbi") and not os.path.exists(bare + ".tbi")
    samples = ["A", "B", "C", "D", "E", "D"]
    want = R.site_genotypes_reference(text, positions, samples)
    rows = [l.split("\t") for l in want.split("\n") if l]
    by_id = {r[3]: r[7] for r in rows if r[3] != "v8"}
    assert by_id["v1"] == "122303" and by_id["v2"] == "000000" and by_id["v3"] == "003000" and by_id["v4"] == "231202" and by_id["v5"] == "230101"
    assert by_id["v6"] == "000000" and by_id["v7m"] == "200101" and by_id["v7"] == "231202" and by_id["v9"] == "000000" and by_id["v10"] == "200000"
    assert [r[7] for r in rows if r[3] == "v8"] == ["312303", "111101"] and "skip" not in by_id and len(rows) == 15
    assert [r[6] for r in rows if r[3] in ("v5", "v6")] == ["1", "-1"]
    for path in (indexed, bare):
        for threads in (1, 3):
            recs, codes, contigs = sample_match.site_genotypes(path, positions, samples, threads, use_index=True)
            got = "".join("\t".join([str(r[0]), r[1], str(r[2]), r[3], r[4], r[5], str(r[6]), "".join(str(int(c)) for c in codes[i])]) + "\n" for i, r in enumerate(recs))
            assert got == want, (path, threads)
            assert contigs == {"1", "2"}
    recs, codes, _ = sample_match.site_genotypes(indexed, positions, samples, 1, use_index=False)
    assert len(recs) == 15 and codes.shape == (15, 6)
    # the first record with the key's alleles gives the key's genotypes; a multi-allelic record never matches
    keys = [("1", 100, "A", "G"), ("1", 700, "A", "C"), ("1", 700, "A", "T"), ("1", 800, "G", "T"), ("1", 123, "A", "C"), ("7", 100, "A", "C"), ("2", 100, "A", "G"),
            ("2", 5000, "A", "C")]
    kept, geno = sample_match.panel_genotypes(indexed, keys, ["A", "B", "C", "D"], 2)
    assert kept == [("1", 100, "A", "G"), ("1", 700, "A", "C"), ("1", 800, "G", "T"), ("2", 100, "A", "G")]
    assert geno.tolist() == [[1, 2, 2, 3], [2, 3, 1, 2], [3, 1, 2, 3], [3, 2, 2, 1]]
    assert sample_match.vcf_donors(indexed) == ["A", "B", "C", "D"]


# ------------------------------------------------------------------------------------------------ the tool against the restatement
DONORS = ["D1", "D2", "D3", "D4", "D5", "D6"]


@functools.lru_cache(maxsize=None)
def tool_world():
    """6 donors (D5 and D6 carry identical genotypes), 8 samples, 125 sites on chr1 and chr2.
    S1 D1's reads, claimed D1; S2 D3's reads claimed D2 (the swap); S3 D4 / D4; S4 D1's reads without a map line; S5 ten lines of D2; S6 D5 / D5 (D6 is its
    twin); S7 a header alone; S8 D3 / D3."""
    rng = np.random.default_rng(77)
    sites = [("chr1", 500 + 90 * j, "ACGT"[j % 4], "CATG"[j % 4]) for j in range(80)] + [("chr2", 300 + 55 * j, "ACGT"[j % 4], "TGCA"[(j + 1) % 4]) for j in range(45)]
    sites[7] = ("chr1", sites[7][1], "AT", "A")                                                     # a deletion: the key is REF and ALT as written
    geno = rng.choice(np.array([1, 2, 3]), size=(len(sites), 6), p=[0.4, 0.4, 0.2])
    geno[:, 5] = geno[:, 4]
    gt = {1: "0|0", 2: "0|1", 3: "1|1"}
    lines = ["##fileformat=VCFv4.2", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + DONORS)]
    absent = {5, 33, 90}                                                                             # keys the VCF lacks
    for j, (c, p, r, a) in enumerate(sites):
        if j in absent:
            continue
        cells = [gt[int(g)] + ":%d" % (10 + j % 7) for g in geno[j]]
        if j == 12:
            cells[1] = "./.:0"; cells[2] = ".:0"
        if j == 20:                                                                                  # a multi-allelic record in front of the key's own
            lines.append("\t".join([c, str(p), "m%d" % j, r, a + ",N", ".", "PASS", ".", "GT:DP"] + ["1/2:5"] * 6))
        if j == 40:                                                                                  # the key's alleles differ from every record's
            lines.append("\t".join([c, str(p), "x%d" % j, r, "N", ".", "PASS", ".", "GT:DP"] + cells))
            continue
        lines.append("\t".join([c, str(p), "v%d" % j, r, a, ".", "PASS", ".", "GT:DP"] + cells))
    vcf = "\n".join(lines) + "\n"
    one = "\n".join(["\t".join(l.split("\t")[:10]) if not l.startswith("##") else l for l in lines]) + "\n"          # the VCF of D1 alone
    p_alt = {1: 0.01, 2: 0.5, 3: 0.99}
    header = "contig\tposition\tvariantID\trefAllele\taltAllele\trefCount\taltCount\ttotalCount"

    def counts(donor, n=None, low_every=9):
        rows = []
        for j, (c, p, r, a) in enumerate(sites[:n]):
            total = int(rng.integers(8, 45)) if j % low_every else int(rng.integers(1, 8))           # some lines below --min_cov
            alt = int(rng.binomial(total, p_alt[int(geno[j, donor])]))
            rows.append("%s\t%d\tv%d\t%s\t%s\t%d\t%d\t%d" % (c, p, j, r, a, total - alt, alt, total))
        return rows
    s1 = counts(0)
    s1.insert(4, s1[2].replace("\t", "\t", 1))                                                       # a duplicate line: the first counts
    dup = s1[10].split("\t"); dup[5] = "40"; dup[6] = "0"; s1.insert(30, "\t".join(dup))            # a duplicate with other counts
    s1.insert(6, "chr1\tnot_a_number\tvX\tA\tC\t9\t9\t18"); s1.insert(50, "chr1\t77\tvY\tA\tC\t9"); s1.insert(60, "chr1\t78\tvZ\tA\tC\t-3\t9\t6")
    s3 = counts(3)
    s3.insert(9, "chr2\t99\tvQ\t\tC\t9\t9\t18"); s3.insert(3, "chr1\t88\tvW\tA\tC\t4294967296\t1\t4294967297")
    s4 = [header.replace("contig\tposition", "position\tcontig")] + ["\t".join([f.split("\t")[1], f.split("\t")[0]] + f.split("\t")[2:]) for f in counts(0)]   # columns by name
    texts = {"S1": "\n".join([header] + s1) + "\n", "S2": "\n".join([header] + counts(2)) + "\n", "S3": "\r\n".join([header] + s3) + "\r\n", "S4": "\n".join(s4) + "\n",
             "S5": "\n".join([header] + counts(1, 10, 99)) + "\n", "S6": "\n".join([header] + counts(4)) + "\n", "S7": header + "\n", "S8": "\n".join([header] + counts(2)) + "\n"}
    samples = [(s, texts[s]) for s in sorted(texts)]
    map_text = "vcf_sample\tbed_sample\textra\n" + "".join("%s\t%s\tx\n" % (d, s) for d, s in (("D1", "S1"), ("D2", "S2"), ("D4", "S3"), ("D6", "S5"), ("D5", "S6"), ("D3", "S8"),
                                                                                                ("D9", "S7")))
    return {"vcf": vcf, "vcf_one": one, "samples": samples, "map": map_text}


@pytest.fixture(scope="module")
def tool_files(tmp_path_factory):
    """the world as files: counts files plain and gzipped (S2, S5, S7 gzipped), the VCFs bgzipped and indexed, the map, a list file in another order"""
    from phaser_amd import _lib, vcfout
    _lib.build()
    w = tool_world()
    d = str(tmp_path_factory.mktemp("sample_match"))
    cdir = os.path.join(d, "counts"); os.makedirs(cdir)
    paths = {}
    for s, text in w["samples"]:
        if s in ("S2", "S5", "S7"):
            paths[s] = os.path.join(cdir, s + ".allelic_counts.txt.gz")
            with gzip.open(paths[s], "wb") as f:
                f.write(text.encode())
        else:
            paths[s] = os.path.join(cdir, s + ".allelic_counts.txt")
            with open(paths[s], "w", newline="") as f:
                f.write(text)
    open(os.path.join(cdir, "notes.txt"), "w").write("not a counts file\n")
    vcf = os.path.join(d, "pop.vcf.gz"); one = os.path.join(d, "one.vcf.gz")
    assert vcfout.write_bgzf(vcf, w["vcf"], 1, index="vcf") and vcfout.write_bgzf(one, w["vcf_one"], 1, index="vcf")
    mp = os.path.join(d, "map.txt"); open(mp, "w").write(w["map"])
    order = ["S8", "S1", "S7", "S2", "S6", "S3", "S5", "S4"]
    lst = os.path.join(d, "list.txt"); open(lst, "w").write("".join("%s\t%s\n" % (s, paths[s]) for s in order))
    return {"dir": d, "counts": cdir, "paths": paths, "vcf": vcf, "vcf_one": one, "map": mp, "list": lst, "order": order}


TOOL_OPTS = [dict(), dict(cap=0), dict(max_sites=70, min_sites=20), dict(output_matrix=1), dict(chrom="chr2", min_sites=20), dict(min_cov=1, error=0.05, het_permille=250, min_lod=3.0)]
TOOL_FILES = ("matches", "map", "summary", "loglik", "concordance")


def _verdicts(matches_text):
    rows = [l.split("\t") for l in matches_text.split("\n")[1:] if l]
    return {r[0]: (r[-1], r[7]) for r in rows}


@pytest.mark.parametrize("opt", TOOL_OPTS)
def test_tool_on_emulated_kernels_equals_the_restatement(emu, tool_files, opt):
    from phaser_amd import sample_match
    w = tool_world()
    stats = {}
    files = sample_match.list_counts_dir(tool_files["counts"])
    assert [s for s, _ in files] == [s for s, _ in w["samples"]]
    out = sample_match.sample_match([(s, p, None) for s, p in files], tool_files["vcf"], w["map"], ctx=emu, threads=3, stats=stats, **opt)
    want = R.restate_tool(w["samples"], w["vcf"], w["map"], **opt)
    for k in TOOL_FILES:
        assert out[k] == want[k], (k, out[k], want[k])
    v = _verdicts(out["matches"])
    if not opt or opt == dict(cap=0) or "output_matrix" in opt:
        assert v == {"S1": ("MATCH", "D1"), "S2": ("MISMATCH", "D3"), "S3": ("MATCH", "D4"), "S4": ("UNCLAIMED", "D1"), "S5": ("LOW_SITES", "D2"), "S6": ("AMBIGUOUS", "D5"),
                     "S7": ("NO_SITES", "NA"), "S8": ("MATCH", "D3")}
        assert out["map"] == "vcf_sample\tbed_sample\nD1\tS1\nD3\tS2\nD4\tS3\nD3\tS8\n"
        # sites 0, 9, ..., 117 are below --min_cov in every sample but S5, which covers site 9: 125 - 14 + 1 keys; of the VCF's four gaps site 90 is one of those
        assert "union_keys\t112\n" in out["summary"] and "keys_not_in_vcf\t3\n" in out["summary"] and "malformed_lines\t5\n" in out["summary"]
        assert "shared_best\tD1\t2\tS1,S4\n" in out["summary"] and "shared_best\tD3\t2\tS2,S8\n" in out["summary"]
    if "max_sites" in opt:
        assert "union_keys\t112\npanel_keys\t56\n" in out["summary"] and v["S2"] == ("MISMATCH", "D3")
    if "chrom" in opt:
        assert "union_keys\t40\n" in out["summary"] and v["S2"] == ("MISMATCH", "D3")
    if "output_matrix" in opt:
        assert out["loglik"].split("\n")[0] == "sample\t" + "\t".join(DONORS) and out["loglik"].count("\n") == 9 and "\tNA" in out["loglik"]
    else:
        assert out["loglik"] is None and out["concordance"] is None
    # the same from texts, in one thread, without the index
    again = sample_match.sample_match([(s, None, t) for s, t in w["samples"]], tool_files["vcf"], w["map"], ctx=emu, threads=1, use_index=False, **opt)
    assert again == out


def test_tool_counts_list_no_map_single_donor_and_the_written_map(emus, tool_files):
    from phaser_amd import cis_var, sample_match
    emu = emus["product"]
    w = tool_world()
    by_name = dict(w["samples"])
    files = sample_match.read_counts_list(open(tool_files["list"]).read())
    assert [s for s, _ in files] == tool_files["order"]
    listed = [(s, by_name[s]) for s in tool_files["order"]]
    out = sample_match.sample_match([(s, p, None) for s, p in files], tool_files["vcf"], w["map"], ctx=emu)
    want = R.restate_tool(listed, w["vcf"], w["map"])
    assert all(out[k] == want[k] for k in TOOL_FILES)
    assert out["matches"].split("\n")[1].startswith("S8\t") and "shared_best\tD3\t2\tS8,S2\n" in out["summary"]          # file order
    assert cis_var.read_map(out["map"]) == [("D3", "S2"), ("D1", "S1"), ("D4", "S3")]                                     # read_map keeps a donor's last sample
    # without --map the claimed donor is the donor of the sample's name
    renamed = [("D3" if s == "S2" else ("D2" if s == "S8" else s), t) for s, t in w["samples"]]
    out = sample_match.sample_match([(s, None, t) for s, t in renamed], tool_files["vcf"], None, ctx=emu)
    want = R.restate_tool(renamed, w["vcf"], None)
    assert all(out[k] == want[k] for k in TOOL_FILES)
    v = _verdicts(out["matches"])
    assert v["D3"] == ("MATCH", "D3") and v["D2"] == ("MISMATCH", "D3") and v["S1"] == ("UNCLAIMED", "D1")
    # a VCF of one donor
    out = sample_match.sample_match([(s, None, t) for s, t in w["samples"]], tool_files["vcf_one"], w["map"], ctx=emu)
    want = R.restate_tool(w["samples"], w["vcf_one"], w["map"])
    assert all(out[k] == want[k] for k in TOOL_FILES)
    v = _verdicts(out["matches"])
    assert v["S1"] == ("SINGLE_DONOR", "D1") and v["S2"] == ("SINGLE_DONOR", "D1") and v["S5"] == ("LOW_SITES", "D1") and v["S7"] == ("NO_SITES", "NA")
    assert out["map"] == "vcf_sample\tbed_sample\n"
    # a sample named twice
    with pytest.raises(sample_match.FatalError, match="occurs twice in --counts_list"):
        sample_match.read_counts_list("S1\ta\nS2\tb\nS1\tc\n")
    with pytest.raises(sample_match.FatalError, match="named twice"):
        sample_match.sample_match([("S1", None, by_name["S1"]), ("S1", None, by_name["S2"])], tool_files["vcf"], None, ctx=emu)
    with pytest.raises(sample_match.FatalError, match="lacks one of the columns"):
        sample_match.sample_match([("S1", None, by_name["S1"].replace("refCount", "rc"))], tool_files["vcf"], None, ctx=emu)


# ------------------------------------------------------------------------------------------------ detection
DETECT_SEED = 2024


@functools.lru_cache(maxsize=None)
def detection_world():
    vcf, samples, map_text, truth, swapped = R.synthetic_population(40, 40, 3000, DETECT_SEED, 8, 60, 0.01, 3)
    want = R.restate_tool(samples, vcf, map_text)
    return vcf, samples, map_text, truth, swapped, want


def _assert_detection(verdicts, truth, swapped):
    assert len(swapped) == 3 and len(verdicts) == 40
    for s, (verdict, best) in verdicts.items():
        assert best == truth[s], s
        assert verdict == ("MISMATCH" if s in swapped else "MATCH"), s


def test_detection_of_planted_swaps(emus, tmp_path):
    from phaser_amd import sample_match, vcfout
    vcf, samples, map_text, truth, swapped, want = detection_world()
    _assert_detection(want["verdicts"], truth, swapped)                                # the restatement alone
    path = os.path.join(str(tmp_path), "pop.vcf.gz")
    assert vcfout.write_bgzf(path, vcf, 2, index="vcf")
    out = sample_match.sample_match([(s, None, t) for s, t in samples], path, map_text, ctx=emus["product"], threads=4)
    _assert_detection(_verdicts(out["matches"]), truth, swapped)
    assert all(out[k] == want[k] for k in ("matches", "map", "summary"))


# ------------------------------------------------------------------------------------------------ options, no GPU
def test_option_checks_raise_fatal_errors(tmp_path, capsys):
    from phaser_amd import sample_match
    ok = dict(min_cov=8, cap=30, error=0.01, het_permille=100, max_sites=50000, min_sites=50, min_lod=10.0)
    sample_match.check_options(**ok)
    sample_match.check_options(**dict(ok, cap=0, max_sites=0, min_lod=0.0, het_permille=500, min_cov=1, min_sites=1, error=0.49))
    for bad, text in ((dict(error=0.0), "--error"), (dict(error=0.5), "--error"), (dict(error=float("nan")), "--error"), (dict(het_permille=0), "--het_permille"),
                      (dict(het_permille=501), "--het_permille"), (dict(cap=-1), "--cap"), (dict(min_cov=0), "--min_cov"), (dict(max_sites=-1), "--max_sites"),
                      (dict(min_sites=0), "--min_sites"), (dict(min_lod=-0.5), "--min_lod"), (dict(min_lod=float("nan")), "--min_lod")):
        with pytest.raises(sample_match.FatalError, match="FATAL ERROR - .*" + text):
            sample_match.check_options(**dict(ok, **bad))
        with pytest.raises(R.Fatal):
            R.restate_tool([], "", None, **dict(ok, **bad))
    tmp = str(tmp_path)
    assert sample_match.main(["--counts_dir", tmp, "--vcf", "x.vcf.gz", "--o", os.path.join(tmp, "out"), "--error", "0.7"]) == 1
    assert "FATAL ERROR - --error must lie strictly between 0 and 0.5" in capsys.readouterr().out.split("\n")
    assert sample_match.main(["--vcf", "x.vcf.gz", "--o", os.path.join(tmp, "out")]) == 1
    assert "FATAL ERROR - exactly one of --counts_dir and --counts_list must be given" in capsys.readouterr().out.split("\n")
    assert sample_match.main(["--counts_dir", tmp, "--counts_list", "l", "--vcf", "x.vcf.gz", "--o", os.path.join(tmp, "out")]) == 1
    assert os.listdir(tmp) == []


def test_without_a_gpu_the_tool_raises(tool_files):
    import torch
    from phaser_amd import _lib, sample_match
    _lib.build()
    if torch.cuda.is_available():
        return
    w = tool_world()
    with pytest.raises(_lib.PhzError):
        sample_match.sample_match([(s, None, t) for s, t in w["samples"]], tool_files["vcf"], w["map"])
    with pytest.raises(_lib.PhzError):
        sample_match.main(["--counts_dir", tool_files["counts"], "--vcf", tool_files["vcf"], "--o", os.path.join(tool_files["dir"], "nogpu")])
    assert not any(x.startswith("nogpu") for x in os.listdir(tool_files["dir"]))


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def _device_call(gpu_ctx):
    """-> call(case) that runs phz_sample_match on torch tensors in the PHZ_DEVICE space"""
    import torch
    from phaser_amd import _lib
    dev = torch.device("cuda", gpu_ctx.device)

    def call(case):
        t = [torch.from_numpy(np.array(x)).to(dev) for x in case]
        S, D = len(case[1]) - 1, case[0].shape[1]
        o = [torch.full((S, D), -5.0, dtype=torch.float64, device=dev), torch.full((S, D), -5, dtype=torch.int32, device=dev), torch.full((S, D), -5, dtype=torch.int32, device=dev)]
        torch.cuda.synchronize(dev)
        arg = _lib.phz_match_in()
        arg.n_sites, arg.n_samples, arg.n_donors = case[0].shape[0], S, D
        arg.geno, arg.e_off, arg.e_site, arg.e_ref, arg.e_alt = (x.data_ptr() for x in t)
        arg.log_ref = (C.c_double * 3)(*LOG_REF); arg.log_alt = (C.c_double * 3)(*LOG_ALT)
        arg.cap, arg.het_permille = CAP, HET
        gpu_ctx.check(gpu_ctx.lib.phz_sample_match(gpu_ctx.h, C.byref(arg), C.c_void_p(o[0].data_ptr()), C.c_void_p(o[1].data_ptr()), C.c_void_p(o[2].data_ptr()), _lib.PHZ_DEVICE))
        return tuple(x.cpu().numpy() for x in o)
    return call


@pytest.mark.gpu
def test_kmatch_gpu_equals_the_restatement_in_both_spaces_and_twice(gpu_ctx):
    from phaser_amd import _lib
    host = lambda case: raw_call(gpu_ctx.lib, gpu_ctx.h, *case)[1:]
    _assert_shapes_match_the_restatement(host, 256, "gpu, host arrays")
    last, total, launches = gpu_ctx.timing(_lib.PHZ_T_MATCH)
    assert launches >= 11 * 7 * 3 and last > 0 and total > 0
    _assert_shapes_match_the_restatement(_device_call(gpu_ctx), 256, "gpu, device arrays")
    case, ref = shape_reference(600, (2, 1000, 5, 0, 1000, 1, 0))
    a = host(case); b = host(case)
    assert same_bits(a, b) and same_bits(a, ref)                                       # two runs give identical bits
    for cap in (0, 1, 7):
        case, ref = shape_reference(65, (2 * 256 + 3, 0, 40), cap)
        assert same_bits(raw_call(gpu_ctx.lib, gpu_ctx.h, *case, cap=cap)[1:], ref), cap


@pytest.mark.gpu
def test_kmatch_gpu_sample_alone_and_donor_prefix(gpu_ctx):
    _assert_independence(lambda case: raw_call(gpu_ctx.lib, gpu_ctx.h, *case)[1:])
    _assert_independence(_device_call(gpu_ctx))


@pytest.mark.gpu
def test_kmatch_gpu_skips_bad_entries_of_device_arrays(gpu_ctx):
    case, ref = shape_reference(17, (7, 0, 9))
    geno, e_off, e_site, e_ref, e_alt = (np.array(x) for x in case)
    e_site[3] = -1; e_site[4] = geno.shape[0]; e_ref[5] = -1; e_alt[6] = -2; e_ref[12] = 0; e_alt[12] = 0
    got = _device_call(gpu_ctx)((geno, e_off, e_site, e_ref, e_alt))
    assert same_bits(got, R.match_reference(geno, e_off, e_site, e_ref, e_alt, LOG_REF, LOG_ALT, CAP, HET)) and not same_bits(got, ref)


def _run_cli(args, out_dir):
    done = subprocess.run([sys.executable, "-m", "phaser_amd.sample_match"] + args + ["--o", os.path.join(out_dir, "out")], cwd=REPO, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0, done.stdout.decode()
    assert b"K_match" in done.stdout
    return {x: open(os.path.join(out_dir, x), "rb").read() for x in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_cli_gpu_as_a_child_process_equals_the_restatement(tool_files, tmp_path):
    w = tool_world()
    runs = []
    for k in (0, 1):
        d = os.path.join(str(tmp_path), "run%d" % k); os.makedirs(d)
        runs.append(_run_cli(["--counts_dir", tool_files["counts"], "--vcf", tool_files["vcf"], "--map", tool_files["map"], "--output_matrix", "1", "--t", str(1 + 2 * k)], d))
    assert runs[0] == runs[1]                                                          # a second run (with another --t) writes identical bytes
    assert sorted(runs[0]) == ["out.concordance.txt.gz", "out.loglik.txt.gz", "out.map.txt", "out.matches.txt", "out.summary.txt"]
    want = R.restate_tool(w["samples"], w["vcf"], w["map"], output_matrix=1)
    for k in ("matches", "map", "summary"):
        assert runs[0]["out.%s.txt" % k].decode() == want[k], k
    for k in ("loglik", "concordance"):
        assert gzip.decompress(runs[0]["out.%s.txt.gz" % k]).decode() == want[k], k
    d = os.path.join(str(tmp_path), "list"); os.makedirs(d)
    got = _run_cli(["--counts_list", tool_files["list"], "--vcf", tool_files["vcf"], "--map", tool_files["map"], "--cap", "0", "--chr", "chr2", "--min_sites", "20"], d)
    by_name = dict(w["samples"])
    want = R.restate_tool([(s, by_name[s]) for s in tool_files["order"]], w["vcf"], w["map"], cap=0, chrom="chr2", min_sites=20)
    assert sorted(got) == ["out.map.txt", "out.matches.txt", "out.summary.txt"]
    for k in ("matches", "map", "summary"):
        assert got["out.%s.txt" % k].decode() == want[k], k


@pytest.mark.gpu
def test_cli_gpu_detects_the_planted_swaps(tmp_path):
    from phaser_amd import vcfout
    vcf, samples, map_text, truth, swapped, want = detection_world()
    tmp = str(tmp_path)
    cdir = os.path.join(tmp, "counts"); os.makedirs(cdir)
    for s, text in samples:
        open(os.path.join(cdir, s + ".allelic_counts.txt"), "w").write(text)
    path = os.path.join(tmp, "pop.vcf.gz")
    assert vcfout.write_bgzf(path, vcf, 2, index="vcf")
    open(os.path.join(tmp, "map.txt"), "w").write(map_text)
    d = os.path.join(tmp, "run"); os.makedirs(d)
    got = _run_cli(["--counts_dir", cdir, "--vcf", path, "--map", os.path.join(tmp, "map.txt"), "--t", "4"], d)
    _assert_detection(_verdicts(got["out.matches.txt"].decode()), truth, swapped)
    for k in ("matches", "map", "summary"):
        assert got["out.%s.txt" % k].decode() == want[k], k
