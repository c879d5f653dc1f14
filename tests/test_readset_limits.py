"""The read-set kernels of the row stage (phaser_amd/csrc/phz_rowsdev.hip: k_seg_small, k_seg_big<MODE, SLOTS, THREADS, HUGE>, the two pool-growth loops of
phz_rowsdev_run and phz_hap_counts) on the designed inputs of tests/readset_inputs.py, under the host-side emulation and on the product build on an MI355X, against
tests/readset_restatement.py.  There is no tolerance anywhere: counts, label texts and QNAME lists are compared as text.

Three tiers.  The restatement (numpy.unique, sets; definitions from oracle/phasing_oracle.py) is pinned first, with no kernel involved: it must reproduce the read-set
columns of every haplotypic_counts.txt / haplotypes.txt the reference wrote under tests/golden, from the read lists of tests/golden/tally.  The
test_*_designs_hold_what_they_promise tests then check, still without a kernel, that every design holds the segments its name promises (entry counts on both sides of
every threshold, in every mode; pieces of length zero; tables whose ids all hash into the last 16 slots) and print one line per design.  Only then the kernels: K_tally,
the device row stage without and with --output_read_ids, the host row stage, phz_hap_counts -- emulated (product thresholds, every row by a wave, pools that start at
64 KB) and on the GPU, every case twice on one context and all cases in one sequence on one context.  PHZ_C_SEG_POOL_REDOS must move exactly where the mirrored pool
arithmetic says a pool overflows."""
import ctypes as C
import functools
import gzip
import os
import pickle
import sys

import numpy as np
import pytest

import readset_inputs as ri
import readset_restatement as rr
from conftest import GOLD, REPO, gz_text
from helpers import OUTPUTS, EmuContext, canonical, emu_library, genome_from_saved, stub_emu_stages, stub_gpu_stages
from test_emu_tally import run_tally


# ------------------------------------------------------------------------------------------------ shared: variant names, block tables
def variant_names(vs, chrom_list, unique_ids=0):
    """per variant of the joint space {"uid", "name", "chrom", "pos", "alleles"}, and the lookup (contig, name or uid) -> variant"""
    table = []; index = {}
    for c in chrom_list:
        cv = vs.chroms[c]
        for i in range(len(cv)):
            index[(c, cv.uid[i])] = len(table); index[(c, cv.rsid[i])] = len(table)
            table.append({"uid": cv.uid[i], "name": cv.uid[i] if unique_ids else cv.rsid[i], "chrom": c, "pos": int(cv.pos[i]), "alleles": cv.alleles[i]})
    return table, index


def restated_columns(rl_start, rl_qid, nb, table, index, hap_text, bam_names, qnames=None, blacklist=frozenset(), excluded=(), unphased_vars=1, sorted_ids=False):
    """the block table a haplotypes.txt states (its non-read-set columns) -> the restatement on the read lists -> (restatement, counts rows, haplotypes rows)"""
    blocks = rr.blocks_of_file(hap_text, lambda contig, x: index[(contig, x)], lambda v: table[v]["alleles"])
    black = frozenset(v for v, t in enumerate(table) if "%s_%d" % (t["chrom"], t["pos"]) in blacklist)
    r = rr.restate(rl_start, rl_qid, nb, blocks, black, excluded)
    qname_of = None if qnames is None else (lambda v, q: qnames[table[v]["chrom"]][q])
    ase, hap = rr.expected_columns(r, table, bam_names, qname_of, unphased_vars, sorted_ids)
    return r, ase, hap


# ------------------------------------------------------------------------------------------------ tier 1: the restatement against the reference's files
def _fixture_cases():
    from test_host_stages import _cases
    return _cases()


@pytest.mark.parametrize("case,gold,load,cfg", _fixture_cases(), ids=[c[0] for c in _fixture_cases()])
def test_restatement_reproduces_the_reference_files(case, gold, load, cfg, c1_inputs):
    """no kernel runs here: the read-set columns of the files the reference wrote, from the read lists of the tally fixture and the block table the file itself states"""
    from test_emu_rowsdev import _inputs
    from phaser_amd import vcf
    d, vcf_text, bams = _inputs(case, gold, c1_inputs)
    load = dict(load); inc = load.pop("include_indels", 0)
    vs = vcf.load_variants(vcf_text, include_indels=inc, **load)
    saved = pickle.load(gzip.open(os.path.join(GOLD, "tally", case + ".pkl.gz"), "rb"))
    chroms = [c for c in vs.chroms if c in saved["tally"]]
    assert sorted(chroms) == sorted(saved["tally"]) and all(saved["tally"][c]["nv"] == len(vs.chroms[c]) for c in chroms)
    G = genome_from_saved(saved, chroms, len(bams))
    table, index = variant_names(vs, chroms, cfg.get("unique_ids", 0))
    want_ase, want_hap = rr.file_columns(canonical("haplotypic_counts", gz_text(os.path.join(d, "out.haplotypic_counts.txt.gz"))),
                                         gz_text(os.path.join(d, "out.haplotypes.txt.gz")))
    r, ase, hap = restated_columns(G["rl_start"], G["rl_qid"], len(bams), table, index, gz_text(os.path.join(d, "out.haplotypes.txt.gz")), bams,
                                   saved["qnames"] if cfg.get("output_read_ids") else None, cfg.get("haplo_blacklist", frozenset()),
                                   cfg.get("haplo_count_bam_exclude", ()), cfg.get("unphased_vars", 1), sorted_ids=True)
    assert hap == want_hap and len(hap) > 0
    assert sorted(ase) == sorted(want_ase)
    for key in ase:
        assert ase[key] == want_ase[key], key
    if case == "opts_read_ids":
        assert all(len(v) == 6 for v in ase.values())
    if case == "opts_blacklist":
        assert r["black"] and any(v in r["black"] for m, _ in r["blocks"] for v in m)
    if case == "opts_bam_exclude":
        assert r["excluded"] == (1,) and not any(b == bams[1] for _, b in ase)


# ------------------------------------------------------------------------------------------------ tier 2: the designs, no kernel
DESIGNS = {d.name: d for d in ri.all_designs()}


def segs(d, mode, cls=None):
    """(M, np) of the segments of a mode (and class) by the restatement on the declared block table"""
    return [(s[1], s[2]) for s in d.declared()["segments"][mode] if cls is None or s[3] == cls]


def row(d):
    t = rr.class_table(d.declared())
    print("%-20s lines %6d  " % (d.name, d.n_lines) + "  ".join("mode %d: %s" % (m, " ".join("%s %d" % (c, t[m][c]) for c in rr.CLASSES if t[m][c])) for m in (0, 1, 2)))
    assert d.name == "pool_growth_product" or d.n_lines <= 37000
    return t


def test_size_class_designs_hold_what_they_promise():
    d = ri.size_classes()
    row(d)
    assert ri.BOUNDARY_SIZES == (0, 1, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 6001) and d.n_bams == 2
    for mode in (0, 1, 2):
        have = {M for M, _ in segs(d, mode)}
        assert set(ri.BOUNDARY_SIZES) <= have, (mode, sorted(set(ri.BOUNDARY_SIZES) - have))
    r = d.declared()
    for k, S in enumerate(ri.BOUNDARY_SIZES):
        big, small = r["mode0"][(k, 0, 0)], r["mode0"][(k, 1, 0)]
        assert big["M"] == S and 0 < small["M"] <= 200                      # the small haplotype next to the big one
        if S >= 8:
            assert big["count"] < S                                         # QNAMEs repeat inside the segment ...
            lst = big["entries"][:len(big["piece_labels"][0])]
            assert len(set(lst.tolist())) < len(lst)                        # ... and inside one list
        both = set(r["mode0"][(k, 1, 0)]["entries"].tolist()) & set(r["mode0"][(k, 1, 1)]["entries"].tolist())
        assert both and r["mode1"][(k, 1)]["count"] < r["mode0"][(k, 1, 0)]["count"] + r["mode0"][(k, 1, 1)]["count"]      # mode 1 is a union over the BAMs
    assert r["mode0"][(11, 0, 0)]["count"] > 1000 and int(r["mode0"][(11, 0, 0)]["labels"].max()) >= 1000                  # labels of four digits
    assert max(s["count"] for s in r["mode0"].values()) < 100000
    assert not rr.pool_overflows(r, (0, 1, 2), rr.SEG_POOL_BYTES) and not rr.pool_overflows(r, (2,), rr.HAP_POOL_BYTES)
    assert rr.pool_overflows(r, (0,), 65536) and rr.pool_overflows(r, (2,), 65536)                                         # pool_growth_emulated: the same design on 64 KB pools
    assert not rr.pool_overflows(r, (0, 1, 2), rr.grown_pool_bytes(rr.grown_pool_bytes(65536)))                            # ... and fit after two growths (three are allowed)


def test_one_qname_designs_hold_what_they_promise():
    d = ri.one_qname()
    row(d)
    r = d.declared()
    for k, S in enumerate((257, 2049)):
        s = r["mode0"][(k, 0, 0)]
        assert s["M"] == S and s["count"] == 1 and not s["labels"].any() and s["flags"].tolist() == [True] + [False] * (S - 1)
    assert sorted(c for _, _, _, c in r["segments"][0] if c not in ("thread", "empty")) == ["workgroup_lds", "workgroup_pool"]
    assert {"wave", "workgroup_lds"} <= {c for _, _, _, c in r["segments"][2]}                                             # the lists of 129 and 1,025 entries


def test_huge_block_designs_hold_what_they_promise():
    d = ri.huge_block()
    row(d)
    r = d.declared()
    n0 = rr.STAT_N + 1
    assert [len(m) for m, _ in d.blocks] == [n0, rr.STAT_N] and d.n_bams == 3
    seg = {k: (s["M"], s["np"]) for k, s in r["mode0"].items()}
    assert seg[(0, 0, 0)][0] > rr.SEG_LDS and seg[(0, 1, 0)][0] > rr.SEG_LDS and seg[(0, 0, 0)][1] == n0                   # pieces and table in the pool
    assert rr.SEG_SMALL < seg[(0, 0, 1)][0] <= rr.SEG_MID and 0 < seg[(0, 1, 1)][0] <= rr.SEG_SMALL                       # pieces in the pool, table in LDS; one thread, 513 pieces
    assert seg[(0, 0, 2)][0] == 0 and seg[(0, 1, 2)][0] == 0                                                               # BAM 2: no read in the block, no row
    assert rr.SEG_MID < seg[(1, 0, 0)][0] <= rr.SEG_LDS and seg[(1, 0, 0)][1] == rr.STAT_N                                 # exactly STAT_N pieces: not huge
    cls = {k: c for k, _, _, c in r["segments"][0]}
    assert (cls[(0, 0, 0)], cls[(0, 0, 1)], cls[(0, 1, 1)], cls[(1, 0, 0)]) == ("huge_pool", "huge_lds", "thread", "workgroup_lds")
    assert {c for _, _, _, c in r["segments"][1]} == {"huge_pool", "workgroup_lds"}
    assert not rr.pool_overflows(r, (0, 1, 2), rr.SEG_POOL_BYTES)


def test_blacklist_designs_hold_what_they_promise():
    d = ri.blacklisted_pieces()
    row(d)
    r = d.declared()
    assert d.black == {0, 3, 4, 7, 8, 9, 11} and [m for m, _ in d.blocks] == [list(range(8)), list(range(8, 12))]
    cls = {k: c for k, _, _, c in r["segments"][0]}
    assert (cls[(0, 0, 0)], cls[(0, 1, 0)], cls[(1, 0, 0)], cls[(1, 1, 0)]) == ("wave", "workgroup_lds", "wave", "thread")
    assert len(r["mode0"][(0, 0, 0)]["piece_labels"]) == 4 and len(r["mode0"][(1, 0, 0)]["piece_labels"]) == 1
    assert r["mode1"][(0, 0)]["M"] > r["mode0"][(0, 0, 0)]["M"] + r["mode0"][(0, 0, 1)]["M"]                               # mode 1 counts the blacklisted members too
    rs, rq = d.read_lists()
    assert all(rs[(v * 2 + k) * 2 + 1] > rs[(v * 2 + k) * 2] for v in d.black for k in (0, 1))                             # ... whose lists are not empty


def test_pool_growth_designs_hold_what_they_promise():
    assert rr.smallest_overflowing_segment(rr.SEG_POOL_BYTES) == 2 ** 19 + 1 and rr.smallest_overflowing_segment(rr.HAP_POOL_BYTES) == 2 ** 17 + 1
    assert 3 * rr.table_slots(2 ** 19) <= rr.pool_capacity_words(rr.SEG_POOL_BYTES) and 3 * rr.table_slots(2 ** 17) <= rr.pool_capacity_words(rr.HAP_POOL_BYTES)
    d = ri.pool_growth_product()
    row(d)
    r = d.declared()
    s = r["mode0"][(0, 0, 0)]
    assert s["M"] == d.big_entries == 2 ** 19 + 2 and s["count"] == ri.POOL_DISTINCT > 100000 and 520000 < d.n_lines < 530000
    assert rr.pool_overflows(r, (0,), rr.SEG_POOL_BYTES) and rr.pool_overflows(r, (1,), rr.SEG_POOL_BYTES)
    assert not rr.pool_overflows(r, (0, 1, 2), rr.grown_pool_bytes(rr.SEG_POOL_BYTES))                                     # one growth is enough
    assert max(s2["M"] for k, s2 in r["mode0"].items() if k[0] == 1) <= rr.SEG_SMALL                                       # a small second block follows
    p = ri.direct_pool_list()
    assert p["big_entries"] == 2 ** 17 + 1 == len(p["lists"][p["named"]["pool"]])


def test_direct_list_designs_hold_what_they_promise():
    d = ri.direct_lists()
    sizes = {n: len(d["lists"][k]) for n, k in d["named"].items()}
    print("direct_lists         lists %d entries %d: %s" % (len(d["lists"]), sum(sizes.values()), " ".join("%s=%d" % x for x in sizes.items())))
    assert [sizes["size_%d" % S] for S in ri.BOUNDARY_SIZES[1:]] == list(ri.BOUNDARY_SIZES[1:])
    for (nd, ne), cap, cls in zip(ri.COLLIDING, (512, 4096, 8192), ("wave", "workgroup_lds", "workgroup_pool")):
        e = d["lists"][d["named"]["colliding_%d" % nd]]
        assert len(e) == ne and len(set(e.tolist())) == nd and rr.table_slots(ne) == cap and rr.size_class(ne, 1) == cls
        slots = ri.mixer(e) & np.uint64(cap - 1)
        assert int(slots.min()) >= cap - 16 and nd > 16                                                                    # every id starts in the last 16 slots: probing wraps
    assert ri.BIG_QID in d["lists"][d["named"]["largest_id"]].tolist()
    for S in (257, 2049):
        assert set(d["lists"][d["named"]["one_qname_%d" % S]].tolist()) == {12345}
    rs, rq, rl = ri.csr_of(d)
    assert rs[1] == 0 and rs[-1] == rs[-2] and len(rq) == rs[-1] < 37000


def test_design_order_puts_a_small_design_after_the_heavy_ones():
    order = [d.name for d in ri.designs()]
    assert order[order.index("huge_block") + 1] == "one_qname" and order.count("size_classes") == 2 and len(DESIGNS) == 4


# ------------------------------------------------------------------------------------------------ tier 3: the kernels
def redos_of(ctx):
    from phaser_amd import _lib
    return ctx.counter(_lib.PHZ_C_SEG_POOL_REDOS)


@functools.lru_cache(maxsize=None)
def oracle_files(name, read_ids):
    """the five files of oracle/phasing_oracle.py on the design's call lines, one call text per BAM: computed once, read-only"""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import phasing_oracle as po
    d = DESIGNS[name]
    R = d.saved["tally"][ri.CHROM]
    gt = {v: ("0|1" if v % 3 else "1|0") for v in range(d.nv)}
    ph = po.Phaser(d.bam_names, as_q_cutoff=0, output_read_ids=read_ids, haplo_blacklist=d.blacklist)
    for b, base, n in R["bam_offsets"]:
        sl = slice(base, base + n)
        ph.add_bam(["".join("q%d\t%s_%d_A_G\trs%d\t%s\t0\t%s\tNone\n" % (q, ri.CHROM, ri.position(v), v, "AG"[k], gt[v])
                            for v, q, k in zip(R["line_var"][sl].tolist(), R["line_qid"][sl].tolist(), R["line_cls"][sl].tolist()))])
    return ph.finish()


def tally_of(ctx, d):
    """K_tally on the design's call lines -> the `saved` form with its results (what the row stages start from); the read lists it hands out are those of the design"""
    got, sz = run_tally(ctx, d.saved, d.chrom_list, d.n_bams)
    rs, rq = d.read_lists()
    assert np.array_equal(got["rl_start"].astype(np.int64), rs) and np.array_equal(got["rl_qid"].astype(np.int64), rq), d.name
    R = dict(d.saved["tally"][ri.CHROM])
    R.update({k: got[k] for k in ("var_count", "var_first", "var_distinct", "var_rank", "ea", "eb", "cells", "linked")})
    return {"tally": {ri.CHROM: R}, "n_qid": d.saved["n_qid"], "qnames": d.saved["qnames"]}


def engine_pass(ctx, d, vs, saved, device_rows, read_ids):
    from phaser_amd.engine import Config, Engine

    class _M:
        device = None
    m = _M(); m.ctx = ctx
    eng = Engine(vs, d.bam_names, Config(device_rows=device_rows, output_read_ids=read_ids, haplo_blacklist=d.blacklist), mapper=m)
    eng.n_qid.update(saved["n_qid"]); eng.qnames.update(saved["qnames"])
    (stub_emu_stages if device_rows else stub_gpu_stages)(eng, saved)
    out = eng.finish()
    assert eng.rows_path == ("device" if device_rows else "host"), getattr(eng, "rows_fallback", "")
    return out, eng


def hap_counts(ctx, nseg, device):
    """phz_hap_counts on the context's resident tally into a host array or into device memory"""
    from phaser_amd import _lib
    if not device:
        got = np.full(nseg, -1, dtype=np.int32)
        ctx.check(ctx.lib.phz_hap_counts(ctx.h, C.c_void_p(got.ctypes.data), nseg, _lib.PHZ_HOST))
        return got
    if isinstance(ctx, EmuContext):                        # (the emulation's device memory is host memory)
        got = np.full(nseg, -1, dtype=np.int32)
        ctx.check(ctx.lib.phz_hap_counts(ctx.h, C.c_void_p(got.ctypes.data), nseg, _lib.PHZ_DEVICE))
        return got
    import torch
    t = torch.full((nseg,), -1, dtype=torch.int32, device="cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.phz_hap_counts(ctx.h, C.c_void_p(t.data_ptr()), nseg, _lib.PHZ_DEVICE))
    return t.cpu().numpy()


def check_hap_counts(ctx, want, overflows, where):
    for device in (False, True):
        before = redos_of(ctx)
        got = hap_counts(ctx, len(want), device)
        assert np.array_equal(got, want), (where, device, np.flatnonzero(got != want)[:5], got[got != want][:5], want[got != want][:5])
        delta = redos_of(ctx) - before
        assert (delta >= 1) if overflows else (delta == 0), (where, "phz_hap_counts", delta)          # (its pool is freed with every call)


def check_design(ctx, d, pool_bytes=(rr.SEG_POOL_BYTES, rr.HAP_POOL_BYTES), reps=2, oracle=True, ids=(0, 1)):
    """K_tally, then per --output_read_ids setting `reps` device passes over ONE variant set (one handle: the pool a first pass grew is kept), phz_hap_counts on the
    resident tally, the host row stage, the oracle.  -> the counter deltas of the device passes"""
    from phaser_amd import vcf
    saved = tally_of(ctx, d)
    vs = vcf.load_variants(d.vcf_text)
    table, index = variant_names(vs, d.chrom_list)
    rs, rq = d.read_lists()
    deltas = []; grown = False
    for read_ids in ids:
        first = None
        for rep in range(reps):
            where = "%s (read ids %d, pass %d)" % (d.name, read_ids, rep)
            before = redos_of(ctx)
            out, eng = engine_pass(ctx, d, vs, saved, True, read_ids)
            delta = redos_of(ctx) - before
            deltas.append(delta)
            r, ase, hap = restated_columns(rs, rq, d.n_bams, table, index, out["haplotypes"], d.bam_names, d.saved["qnames"] if read_ids else None, d.blacklist)
            # the blocks the design is built to give formed, whichever haplotype the phasing calls A
            assert sorted(m for m, _ in r["blocks"]) == sorted(m for m, _ in d.blocks), where
            assert all(a == b or [x ^ 1 for x in a] == b for (_, a), (_, b) in zip(sorted(r["blocks"]), sorted(d.blocks))), where
            got_ase, got_hap = rr.file_columns(out["haplotypic_counts"], out["haplotypes"])
            assert got_hap == hap, where
            assert sorted(got_ase) == sorted(ase), where
            for key in ase:
                assert got_ase[key] == ase[key], (where, key, [i for i, (x, y) in enumerate(zip(got_ase[key], ase[key])) if x != y])
            modes = (0, 1, 2)                                # two BAMs or more: the union over the BAMs and the per-list counts are their own passes
            assert d.n_bams > 1 and int(eng.stats["rowsdev_n_big_segments"]) == rr.big_segments(r, modes), (where, eng.stats["rowsdev_n_big_segments"], rr.big_segments(r, modes))
            overflows = rr.pool_overflows(r, modes, pool_bytes[0])
            assert (delta >= 1) if (overflows and not grown) else (delta == 0), (where, delta, overflows, grown)
            grown = grown or overflows
            if rep == 0:                                     # (the resident tally is the same in every pass)
                check_hap_counts(ctx, r["mode2"], rr.pool_overflows(r, (2,), pool_bytes[1]), where)
            if first is None:
                first = out
            for name in OUTPUTS:
                assert out[name] == first[name], (where, name)
        host, _ = engine_pass(ctx, d, vs, saved, False, read_ids)
        for name in OUTPUTS:
            assert first[name] == host[name], (d.name, read_ids, name)
        if oracle:
            want = oracle_files(d.name, read_ids)
            for name in OUTPUTS:
                assert canonical(name, first[name]) == canonical(name, want[name]), (d.name, read_ids, name)
    return deltas


def check_sequence(ctx, pool_bytes=(rr.SEG_POOL_BYTES, rr.HAP_POOL_BYTES)):
    for d in ri.designs():
        check_design(ctx, d, pool_bytes, reps=1, ids=(1,))


def import_lists(ctx, d):
    from phaser_amd import _lib
    rs, rq, rl = ri.csr_of(d)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    sz = _lib.phz_tally_sizes(0, 0, 0, len(rq), 0, 0, 0, 0)
    out = _lib.phz_tally_out(None, None, None, None, None, None, None, None, None, None, vp(rs), vp(rq), None)
    ctx.check(ctx.lib.phz_tally_import(ctx.h, d["nv"], d["nb"], C.byref(sz), C.byref(out), vp(rl), _lib.PHZ_HOST))
    return rr.restate(rs, rq, d["nb"], [])


def check_direct(ctx, d, hap_pool_bytes=rr.HAP_POOL_BYTES, reps=2):
    """hand-built read lists adopted as the resident tally, phz_hap_counts (mode 2 alone) against the restatement"""
    r = import_lists(ctx, d)
    for name, (v, k, b) in d["named"].items():
        e = (v * 2 + k) * d["nb"] + b
        assert r["mode2"][e] == len(set(d["lists"][(v, k, b)].tolist())), name
    for rep in range(reps):
        check_hap_counts(ctx, r["mode2"], rr.pool_overflows(r, (2,), hap_pool_bytes), "direct lists, call %d" % rep)
    return r


EMU_VARIANTS = {"product_thresholds": {}, "rows_by_wave": {"row_wave_min": 0}, "pools_of_64_kb": {"seg_pool": 65536}}
# every design twice, without and with the QNAME columns, at the product's thresholds; the two other builds where they matter, with the QNAME columns (the longer rows):
# every block row formatted by a wave on the designs whose blocks the product formats by a thread, the 64 KB pools on the designs with a table or piece arrays in the pool
EMU_RUNS = [(n, "product_thresholds") for n in sorted(DESIGNS)] + [(n, "rows_by_wave") for n in ("blacklisted_pieces", "one_qname", "size_classes")] + \
           [(n, "pools_of_64_kb") for n in ("huge_block", "one_qname", "size_classes")]


def _pools(variant):
    return (65536, 65536) if "seg_pool" in EMU_VARIANTS[variant] else (rr.SEG_POOL_BYTES, rr.HAP_POOL_BYTES)


@pytest.mark.parametrize("name,variant", EMU_RUNS, ids=["%s-%s" % x for x in EMU_RUNS])
def test_emulated_kernels_match_the_restatement(name, variant):
    """(pools_of_64_kb on size_classes is the design pool_growth_emulated: the redo counter moves on the first pass over the variant set and not again)"""
    ctx = EmuContext(emu_library(**EMU_VARIANTS[variant]))
    if variant == "product_thresholds":
        assert not any(check_design(ctx, DESIGNS[name]))
    elif variant == "rows_by_wave":
        assert not any(check_design(ctx, DESIGNS[name], reps=1, ids=(1,)))
    else:
        deltas = check_design(ctx, DESIGNS[name], _pools(variant), ids=(1,))
        print("%s on 64 KB pools: PHZ_C_SEG_POOL_REDOS deltas of the two row-stage passes %s" % (name, deltas))
        assert deltas[0] >= 1 and deltas[1] == 0, deltas


@pytest.mark.parametrize("variant", ["product_thresholds", "pools_of_64_kb"])
def test_emulated_kernels_leave_the_context_clean_over_all_designs(variant):
    check_sequence(EmuContext(emu_library(**EMU_VARIANTS[variant])), _pools(variant))


@pytest.mark.parametrize("variant", ["product_thresholds", "pools_of_64_kb"])
def test_emulated_hap_counts_on_hand_built_lists(variant):
    ctx = EmuContext(emu_library(**EMU_VARIANTS[variant]))
    r = check_direct(ctx, ri.direct_lists(), _pools(variant)[1])
    assert rr.pool_overflows(r, (2,), 65536) and not rr.pool_overflows(r, (2,), rr.HAP_POOL_BYTES)
    check_direct(ctx, {"nv": 2, "nb": 1, "lists": {(0, 1, 0): np.asarray([4, 4, 9])}, "named": {}}, _pools(variant)[1])          # a small table right after


@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DESIGNS))
def test_product_kernels_match_the_restatement(gpu_ctx, name):
    assert not any(check_design(gpu_ctx, DESIGNS[name]))                      # the product's pools hold every one of these designs: no redo


@pytest.mark.gpu
def test_product_kernels_leave_the_context_clean_over_all_designs(gpu_ctx):
    check_sequence(gpu_ctx)


@pytest.mark.gpu
def test_product_hap_counts_on_hand_built_lists(gpu_ctx):
    check_direct(gpu_ctx, ri.direct_lists())
    check_direct(gpu_ctx, {"nv": 2, "nb": 1, "lists": {(0, 1, 0): np.asarray([4, 4, 9])}, "named": {}})


@pytest.mark.gpu
def test_product_pools_grow_once_and_the_row_stage_keeps_what_it_grew():
    """pool_growth_product: a segment of 2^19 + 2 entries overflows the row stage's 12 MB pool (the stage is redone with a larger one, which the handle of the variant
    set keeps: the second pass does not redo), a list of 2^17 + 1 entries the 4 MB pool of phz_hap_counts (freed with every call: every call redoes).  The small design
    afterwards shows the context clean.  Counter deltas seen on an MI355X: row stage 1 then 0; phz_hap_counts 1 on each of the four calls."""
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    try:
        d = ri.pool_growth_product()
        deltas = check_design(ctx, d, oracle=False, ids=(0,))
        print("pool_growth_product: PHZ_C_SEG_POOL_REDOS deltas of the two row-stage passes", deltas)
        assert deltas[0] >= 1 and deltas[1] == 0, deltas
        p = ri.direct_pool_list()
        before = redos_of(ctx)
        r = check_direct(ctx, p)
        print("direct_pool_list: PHZ_C_SEG_POOL_REDOS delta of four phz_hap_counts calls", redos_of(ctx) - before)
        assert r["mode2"][(1 * 2 + 0) * 1 + 0] == 70001 and redos_of(ctx) - before >= 4
        check_design(ctx, ri.one_qname(), reps=1)
    finally:
        ctx.close()
