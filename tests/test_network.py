"""--output_network (phaser/phaser.py:1127-1157, generate_hap_network_all :1928-1949) without a GPU: the text layer of phaser_amd/network.py against the two
files the reference wrote (tests/golden/network, tools/make_golden.py fx_network), the numpy restatement links_from_edges on hand-made pair tables, the kernels of
phz_variant_links under the host-side HIP emulation against that restatement and against brute-force set intersections over the tally's read lists, every refusal
of the entry, and Engine.network on the fixtures' tallies through both row stages.  The real kernels: tests/test_gpu_network.py."""
import ctypes as C
import gzip
import json
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import GOLD, REPO, gz_text
from helpers import EmuContext, emu_library, stub_emu_stages, stub_gpu_stages
from test_emu_tally import run_tally

NET = os.path.join(GOLD, "network")
CASES = json.load(open(os.path.join(NET, "cases.json")))["cases"]
WITH_FILES = [k for k, v in CASES.items() if v["files"]]
WITHOUT_FILES = [k for k, v in CASES.items() if not v["files"]]


def golden(name, which):
    with gzip.open(os.path.join(NET, "%s.%s.txt.gz" % (name, which)), "rb") as f:
        return f.read()


def reference_block(name):
    """The block of a case as the reference's other files show it: (unique ids in block order, allele strings 2 v + k in allele-index order, allele index on
    haplotype A) from the fixture's haplotypic_counts row that lists the variant and the variant table of its VCF."""
    from phaser_amd import vcf
    case = CASES[name]
    d = os.path.join(GOLD, case["fixture"])
    row = next(f for f in (l.split("\t") for l in gz_text(os.path.join(d, "out.haplotypic_counts.txt.gz")).split("\n")[1:] if l)
               if case["variant"] in f[3].split(",") and int(f[4]) > 1)
    ids = row[3].split(","); hap_a_text = row[7].split(",")
    vs = vcf.load_variants(open(os.path.join(d, "in.vcf")).read(), include_indels=case["options"].get("include_indels", 0))
    cv = vs.chroms[row[0]]
    at = {u: i for i, u in enumerate(cv.uid)}
    alleles = [cv.alleles[at[u]][k] for u in ids for k in (0, 1)]
    hap_a = [cv.alleles[at[u]].index(a) for u, a in zip(ids, hap_a_text)]
    return ids, alleles, hap_a


def records_of(links_bytes, ids, alleles):
    from phaser_amd.network import LINK_DTYPE
    rows = [l.split("\t") for l in links_bytes.decode().split("\n")[1:] if l]
    at = {u: i for i, u in enumerate(ids)}
    rec = np.zeros(len(rows), dtype=LINK_DTYPE)
    for r, (a, b, n, inferred) in enumerate(rows):
        (ua, xa), (ub, xb) = a.split(":"), b.split(":")
        i, j = at[ua], at[ub]
        rec[r] = (i, j, int(n), alleles[2 * i:2 * i + 2].index(xa), alleles[2 * j:2 * j + 2].index(xb), int(inferred), 0)
    return rec


# ------------------------------------------------------------------------------------------------ text layer against the reference's files
@pytest.mark.parametrize("name", WITH_FILES)
def test_text_layer_regenerates_the_reference_files(name):
    from phaser_amd import network
    ids, alleles, hap_a = reference_block(name)
    want_links = golden(name, "links"); want_nodes = golden(name, "nodes")
    rec = records_of(want_links, ids, alleles)
    assert len(rec) > 20 and np.all(rec["i"] < rec["j"])
    assert network.links_text(rec, ids, alleles) == want_links
    assert network.nodes_text(rec, ids, alleles, hap_a, hash_order=True) == want_nodes                      # the reference's set(nodes) order, byte for byte
    canon = network.nodes_text(rec, ids, alleles, hap_a).decode().split("\n")
    assert sorted(canon) == sorted(want_nodes.decode().split("\n")) and canon[0] == "id\tindex\tassigned_hap"
    first = []
    for l in want_links.decode().split("\n")[1:]:
        for node in l.split("\t")[:2] if l else ():
            if node not in first:
                first.append(node)
    assert [l.split("\t")[0] for l in canon[1:] if l] == first                                              # canonical tier: first appearance in the links rows
    if name == "indel_block":
        assert any(len(a) > 1 for a in alleles) and b":GATA\t" in want_links                                 # multi-base allele strings


def test_text_of_no_rows():
    from phaser_amd import network
    empty = np.zeros(0, dtype=network.LINK_DTYPE)
    assert network.links_text(empty, ["a", "b"], ["A", "C", "G", "T"]) == b"variantA\tvariantB\tconnections\tinferred\n"
    assert network.nodes_text(empty, ["a", "b"], ["A", "C", "G", "T"], [0, 1], hash_order=True) == b"id\tindex\tassigned_hap\n"


# ------------------------------------------------------------------------------------------------ the numpy restatement on hand-made pair tables
def _cells(rr=0, ra=0, ar=0, aa=0, other=0):
    return [rr, ra, other, ar, aa, other, other, other, other]


def test_links_from_edges_on_hand_made_tables():
    from phaser_amd.network import links_from_edges
    ea = np.array([2, 2, 2, 5, 5, 7], np.int32); eb = np.array([5, 7, 9, 7, 8, 9], np.int32)
    cells = np.array([_cells(rr=4, aa=3), _cells(ra=2), _cells(rr=9), _cells(other=6), _cells(ar=1), _cells(rr=1, ra=2, ar=3, aa=4)], np.int32)
    tup = lambda r: [tuple(int(x) for x in t)[:6] for t in r.tolist()]
    # 9 and 8 are outside the set: (2, 9), (5, 8), (7, 9) are dropped; (5, 7) has only "other" cells: no row
    got = links_from_edges(ea, eb, cells, [2, 5, 7])
    assert tup(got) == [(0, 1, 4, 0, 0, 0), (0, 1, 4, 1, 1, 1), (0, 1, 3, 1, 1, 0), (0, 1, 3, 0, 0, 1),          # edge (2, 5): cells rr, aa, each direct then inferred
                        (0, 2, 2, 0, 1, 0), (0, 2, 2, 1, 0, 1)]                                                  # edge (2, 7): cell ra
    # x then y inside a pair, direct before inferred
    got = links_from_edges(ea, eb, cells, [7, 9])
    assert tup(got) == [(0, 1, 1, 0, 0, 0), (0, 1, 1, 1, 1, 1), (0, 1, 2, 0, 1, 0), (0, 1, 2, 1, 0, 1), (0, 1, 3, 1, 0, 0), (0, 1, 3, 0, 1, 1), (0, 1, 4, 1, 1, 0), (0, 1, 4, 0, 0, 1)]
    # one non-zero cell: exactly its direct and its inferred row
    assert tup(links_from_edges(ea, eb, cells, [5, 8])) == [(0, 1, 1, 1, 0, 0), (0, 1, 1, 0, 1, 1)]
    # all four cells zero, an unpaired set, sets of 0 / 1 / 2 variants
    assert len(links_from_edges(ea, eb, cells, [5, 7])) == 0 and len(links_from_edges(ea, eb, cells, [3, 4])) == 0
    assert len(links_from_edges(ea, eb, cells, [])) == 0 and len(links_from_edges(ea, eb, cells, [2])) == 0 and len(links_from_edges(ea, eb, cells, [2, 9])) == 2
    assert len(links_from_edges(ea[:0], eb[:0], cells[:0], [2, 5])) == 0


# ------------------------------------------------------------------------------------------------ the kernels under emulation
def variant_links(ctx, vars, space=None, device_rows=False):
    """phz_variant_links the way a caller uses it: count with rows_cap = 0, then fill with the exact count.  (Under the emulation device memory is host memory: the
    PHZ_DEVICE form gets the same numpy arrays.)"""
    from phaser_amd import _lib
    from phaser_amd.network import LINK_DTYPE
    space = _lib.PHZ_HOST if space is None else space
    vars = np.ascontiguousarray(vars, dtype=np.int32)
    vp = C.c_void_p(vars.ctypes.data) if len(vars) else None
    n = C.c_int64(-1)
    st = ctx.lib.phz_variant_links(ctx.h, vp, len(vars), None, 0, C.byref(n), space)
    if st == 0:
        assert n.value == 0
        return np.zeros(0, dtype=LINK_DTYPE)
    assert st == _lib.PHZ_E_CAPACITY and n.value > 0, (st, ctx.lib.phz_last_error(ctx.h))
    assert b"rows_cap" in ctx.lib.phz_last_error(ctx.h)
    need = int(n.value)
    if need > 2:                                                # one row short: still refused, nothing written
        short = np.full(need - 1, 0x55, dtype=np.uint8).repeat(16).view(LINK_DTYPE)
        n2 = C.c_int64(-1)
        assert ctx.lib.phz_variant_links(ctx.h, vp, len(vars), C.c_void_p(short.ctypes.data), need - 1, C.byref(n2), space) == _lib.PHZ_E_CAPACITY and n2.value == need
        assert np.all(short.view(np.uint8) == 0x55)
    rows = np.full((need + 1) * 16, 0xA5, dtype=np.uint8)
    n3 = C.c_int64(-1)
    ctx.check(ctx.lib.phz_variant_links(ctx.h, vp, len(vars), C.c_void_p(rows.ctypes.data), need, C.byref(n3), space))
    assert n3.value == need and np.all(rows[need * 16:] == 0xA5)          # nothing behind the last row
    return rows[:need * 16].view(LINK_DTYPE).copy()


@pytest.fixture(scope="module", params=["pipe_two", "pipe_noisy_b"])
def tallied(request):
    """K_tally under emulation on a fixture's call lines, its results fetched once: (ctx with the tally resident, fetched arrays, chromosome bases, saved)"""
    saved = pickle.load(gzip.open(os.path.join(GOLD, "tally", request.param + ".pkl.gz"), "rb"))
    chroms = list(saved["tally"])
    nb = 1 + max(b for c in chroms for b, _, _ in saved["tally"][c]["bam_offsets"])
    ctx = EmuContext(emu_library())
    got, sz = run_tally(ctx, saved, chroms, nb)
    bases = np.cumsum([0] + [saved["tally"][c]["nv"] for c in chroms])
    for k in got:
        got[k].setflags(write=False)
    return ctx, got, bases, nb, request.param


def _same(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and a.tobytes() == b.tobytes()


def test_kernel_equals_the_restatement_on_fixture_tallies(tallied):
    from phaser_amd import _lib
    from phaser_amd.network import links_from_edges
    ctx, T, bases, nb, case = tallied
    NV = int(bases[-1])
    rng = np.random.default_rng(12)
    sets = {"every variant": np.arange(NV), "from the first variant": np.arange(0, min(NV, 40)), "up to the last variant": np.arange(max(0, NV - 37), NV),
            "first and last only": np.array([0, NV - 1]), "every third": np.arange(1, NV, 3)}
    for ci in range(len(bases) - 1):
        lo, hi = int(bases[ci]), int(bases[ci + 1])
        sets["inside chromosome %d" % ci] = np.sort(rng.choice(np.arange(lo, hi), size=min(hi - lo, 25), replace=False))
        sets["a run of chromosome %d" % ci] = np.arange(lo + (hi - lo) // 3, lo + (hi - lo) // 3 + 17)
    total = 0
    for what, vars in sets.items():
        want = links_from_edges(T["ea"], T["eb"], T["cells"], vars)
        for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
            got = variant_links(ctx, vars, space)
            assert _same(got, want), (case, what, space, len(got), len(want))
        total += len(want)
    assert total > 1000
    assert len(links_from_edges(T["ea"], T["eb"], T["cells"], sets["every variant"])) > 500


def test_counts_equal_set_intersections_of_the_read_lists(tallied):
    """What the feature rests on: cell (x, y) of a pair of the resident table = |read_set[v][x] & read_set[o][y]|, the deduplicated QNAME sets over ALL BAMs that
    generate_hap_network_all intersects (phaser.py:1928-1949, built at :1318-1322) -- recomputed here with Python sets from the tally's read lists alone."""
    ctx, T, bases, nb, case = tallied
    NV = int(bases[-1])
    rs = T["rl_start"].astype(np.int64); rq = T["rl_qid"]
    sets = [[set(), set()] for _ in range(NV)]
    for v in range(NV):
        for k in range(2):
            for b in range(nb):
                e = (2 * v + k) * nb + b
                sets[v][k].update(rq[rs[e]:rs[e + 1]].tolist())                     # union over the BAMs
    want = {}
    for ci in range(len(bases) - 1):                                               # QNAME ids are per chromosome: nothing pairs across chromosomes
        for v in range(int(bases[ci]), int(bases[ci + 1])):
            if not (sets[v][0] or sets[v][1]):
                continue
            for o in range(v + 1, int(bases[ci + 1])):
                for x in range(2):
                    for y in range(2):
                        n = len(sets[v][x] & sets[o][y])
                        if n:
                            want[(v, o, x, y)] = n
    rec = variant_links(ctx, np.arange(NV))
    direct = rec[rec["inferred"] == 0]
    got = {(int(r["i"]), int(r["j"]), int(r["allele_i"]), int(r["allele_j"])): int(r["count"]) for r in direct}
    assert got == want and len(want) > 200
    inferred = rec[rec["inferred"] == 1]
    assert np.array_equal(inferred["count"], direct["count"]) and np.array_equal(inferred["allele_i"], 1 - direct["allele_i"]) and np.array_equal(inferred["allele_j"], 1 - direct["allele_j"])
    if nb > 1:                                                                     # some read set really is a union over BAMs
        assert any(len(set(rq[rs[(2 * v) * nb]:rs[(2 * v) * nb + 1]].tolist())) < len(sets[v][0]) for v in range(NV))


def test_refusals_leave_the_ctx_usable(tallied):
    from phaser_amd import _lib
    from phaser_amd.network import links_from_edges
    _, T, bases, nb, case = tallied
    NV = int(bases[-1])
    lib = emu_library()
    ctx = EmuContext(lib)
    n = C.c_int64(-1)
    good = np.arange(NV, dtype=np.int32)

    def refused(vars, space, needle):
        v = np.ascontiguousarray(vars, dtype=np.int32)
        n.value = -1
        assert lib.phz_variant_links(ctx.h, C.c_void_p(v.ctypes.data), len(v), None, 0, C.byref(n), space) == _lib.PHZ_E_ARG
        assert needle in lib.phz_last_error(ctx.h), lib.phz_last_error(ctx.h)
        assert n.value == 0

    def works():
        assert _same(variant_links(ctx, good), links_from_edges(T["ea"], T["eb"], T["cells"], good))

    # ---- no resident tally
    refused(good[:5], _lib.PHZ_HOST, b"no resident tally")
    # ---- a tally adopted without its pair cells (what tests/helpers.py stub_emu_stages imports)
    vp = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    keep = {k: np.ascontiguousarray(T[k]) for k in T}
    rl_list = np.repeat(np.arange(NV * 2 * nb, dtype=np.uint32), np.diff(keep["rl_start"].astype(np.int64))).astype(np.uint32)
    sz = _lib.phz_tally_sizes(len(keep["line_cls"]), 0, len(keep["ea"]), len(keep["rl_qid"]), 0, 0, 0, 0)

    def adopt(with_cells):
        out = _lib.phz_tally_out(vp(keep["var_count"]), vp(keep["var_first"]), vp(keep["var_distinct"]), vp(keep["var_rank"]), None, vp(keep["ea"]), vp(keep["eb"]),
                                 vp(keep["cells"]) if with_cells else None, vp(keep["linked"]), vp(keep["cto"]), vp(keep["rl_start"]), vp(keep["rl_qid"]), vp(keep["stats"]))
        ctx.check(lib.phz_tally_import(ctx.h, NV, nb, C.byref(sz), C.byref(out), vp(rl_list), _lib.PHZ_HOST))
    adopt(False)
    refused(good[:5], _lib.PHZ_HOST, b"edge_cells")
    adopt(True)
    works()                                                                           # ... and an import WITH the cells serves the links
    # ---- sets that are not strictly ascending inside [0, nv), host and device arguments
    for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
        for bad in ([3, 3, 5], [5, 4], [0, 1, NV], [-1, 2], [2, 7, 6, 9]):
            refused(bad, space, b"strictly ascending")
            works()
        refused([NV + 3], space, b"strictly ascending")                               # a one-variant set is still checked
    # ---- fewer than two variants: no row, no error
    for vars in ([], [0], [NV - 1]):
        assert len(variant_links(ctx, vars)) == 0
    assert len(variant_links(ctx, [4], _lib.PHZ_DEVICE)) == 0
    works()
    gen = C.c_uint64(0)
    ctx.check(lib.phz_tally_generation(ctx.h, C.byref(gen)))
    assert gen.value == 2


# ------------------------------------------------------------------------------------------------ Engine.network on the fixtures' tallies (both row stages)
def engine_on_fixture(name, device_rows, **extra):
    from phaser_amd import vcf
    from phaser_amd.engine import Config, Engine
    from phaser_amd.network import links_from_edges
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    from phasing_oracle import bam_display_names          # naming helper only
    case = CASES[name]
    d = os.path.join(GOLD, case["fixture"])
    opts = dict(case["options"]); inc = opts.pop("include_indels", 0)
    vs = vcf.load_variants(open(os.path.join(d, "in.vcf")).read(), include_indels=inc)
    saved = pickle.load(gzip.open(os.path.join(GOLD, "tally", case["fixture"] + ".pkl.gz"), "rb"))

    class _M:
        ctx = EmuContext(emu_library()) if device_rows else type("ctx", (), {"lib": None})
        device = None
    eng = Engine(vs, bam_display_names([b + ".bam" for b in case["bams"]]), Config(include_indels=inc, device_rows=device_rows, **opts, **extra), mapper=_M())
    eng.n_qid.update(saved["n_qid"]); eng.qnames.update(saved["qnames"])
    (stub_emu_stages if device_rows else stub_gpu_stages)(eng, saved)
    eng.finish()
    assert eng.rows_path == ("device" if device_rows else "host")
    cells = np.concatenate([saved["tally"][c]["cells"].reshape(-1, 9) for c in eng.chrom_list])
    return eng, (lambda vars: links_from_edges(eng.G["ea"], eng.G["eb"], cells, vars))


@pytest.mark.parametrize("device_rows", [True, False], ids=["device_rows", "host_rows"])
@pytest.mark.parametrize("name", WITH_FILES)
def test_engine_network_gives_the_reference_files(name, device_rows):
    """The block comes from the row stage (phz_rowsdev_fetch_blocks under emulation / the host twin), the records from the fixture's pair cells through the
    _links hook: the links file is the reference's byte for byte, the nodes file row for row and, in the reference's set order, byte for byte."""
    from phaser_amd import _lib, network
    eng, hook = engine_on_fixture(name, device_rows)
    net = eng.network(CASES[name]["variant"], _links=hook)
    assert net is not None and net["links"] == golden(name, "links")
    assert sorted(net["nodes"].split(b"\n")) == sorted(golden(name, "nodes").split(b"\n"))
    chrom, vars, hap = network.block_of(eng, CASES[name]["variant"])
    ids, alleles = network.block_strings(eng, chrom, vars)
    assert network.nodes_text(net["records"], ids, alleles, hap, hash_order=True) == golden(name, "nodes")
    assert [u.decode() for u in ids] == reference_block(name)[0]                     # the FINAL block (pipe_noisy_b: a piece phase_v3 cut out of a component)
    if name == "two_chr22":
        assert eng.G["var_base"][chrom] > 0 and vars[0] >= eng.G["var_base"][chrom]   # second chromosome: a non-zero base in the joint variant space
    if device_rows:
        # without the hook the launch is asked for -- and refuses, with the reason: this stub adopted the tally without its pair cells
        with pytest.raises(_lib.PhzError, match="edge_cells"):
            eng.network(CASES[name]["variant"])
        assert eng.network(CASES[name]["variant"], _links=hook)["links"] == net["links"]


@pytest.mark.parametrize("device_rows", [True, False], ids=["device_rows", "host_rows"])
def test_engine_network_of_a_variant_in_no_block(device_rows):
    eng, hook = engine_on_fixture(WITHOUT_FILES[0], device_rows)
    for name in WITHOUT_FILES:                                                       # a singleton, an id the VCF does not hold
        assert eng.network(CASES[name]["variant"], _links=hook) is None
    assert eng.network("chr22_333178", _links=hook) is None and eng.network("", _links=hook) is None      # a prefix of an id is no id


def test_network_needs_the_block_arrays():
    from phaser_amd import _lib
    eng, hook = engine_on_fixture(WITH_FILES[0], False, want_vcf=False)
    with pytest.raises(_lib.PhzError, match="want_vcf"):
        eng.network(CASES[WITH_FILES[0]]["variant"], _links=hook)
