"""The text writers of the row stage (phaser_amd/csrc/phz_rowsdev.hip: the sinks SCount / SWrite / WCount / WWrite, k_mem_rec, the row functions RowConn ... RowCfg,
k_row_len / k_row_write / k_row_wave_len / k_row_wave_write, the closed-form allele_config offsets k_cfg_chunks / k_cfg_prefix / k_cfg_prefix_wave / k_cfg_write) on the
designed inputs of tests/rowtext_inputs.py, under the host-side emulation and on the product build on an MI355X.  There is no tolerance anywhere: text is compared as text.

Three tiers.  The test_*_design_holds_what_it_promises tests run no kernel: from the design and from the five files oracle/phasing_oracle.py writes on its call lines
they check that the blocks, member kinds, string lengths, digit counts, blacklisted rounds and staged / unstaged workgroups the design's name promises are there, and print
one line per design.  Then the kernels, emulated (product thresholds; every block row by a wave on the designs with blocks a thread formats; blocks beyond the gwStat table
on block_sizes) and on the GPU (every design twice on one context, all designs in one sequence on one context): per design and option set the device rows must equal the
host rows (phz_rows.cpp) byte for byte in all five files, both must equal the oracle under canonical(), and allele_config.txt must equal, in exact row order, the
restatement restated_config() below -- for every block row of the produced haplotypes.txt, for i, for j != i, one row."""
import functools
import os
import sys

import numpy as np
import pytest

import rowtext_inputs as xi
from conftest import REPO
from helpers import OUTPUTS, EmuContext, canonical, emu_library, stub_emu_stages, stub_gpu_stages
from test_emu_tally import run_tally

DESIGNS = {d.name: d for d in xi.all_designs()}
TALLY_KEYS = ("var_count", "var_first", "var_distinct", "var_rank", "ea", "eb", "cells", "linked")


# ------------------------------------------------------------------------------------------------ shared: the oracle's files, the restatement of allele_config
@functools.lru_cache(maxsize=None)
def oracle_files(name, option):
    """the five files of oracle/phasing_oracle.py on the design's call lines under its option set `option`: computed once, read-only"""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import phasing_oracle as po
    d = DESIGNS[name]
    ph = po.Phaser(d.bam_names, as_q_cutoff=0, haplo_blacklist=d.blacklist, **d.options[option])
    for b in range(d.n_bams):
        ph.add_bam(d.call_texts(b))
    return ph.finish()


def rows_of(text):
    return text.split("\n")[1:-1]


def name_index(d):
    """(contig, uid or rsid) -> Variant"""
    return {(c, n): v for c in d.chrom_list for v in d.vars[c] for n in (v.uid, v.rsid)}


def hap_blocks(d, hap_text):
    """the block rows of a haplotypes.txt -> [(members as Variants, alleles of haplotype A, alleles of haplotype B)] in file order"""
    idx = name_index(d)
    out = []
    for line in rows_of(hap_text):
        f = line.split("\t")
        if int(f[4]) >= 2:
            a, b = (h.split(",") for h in f[6].split("|"))
            out.append(([idx[(f[0], x)] for x in f[5].split(",")], a, b))
    return out


def restated_config(d, hap_text):
    rows = ["variant_a\trsid_a\tvariant_b\trsid_b\tconfiguration\n"]
    for vs, a, b in hap_blocks(d, hap_text):
        for i, vi in enumerate(vs):
            for j, vj in enumerate(vs):
                if j != i:
                    rows.append("%s\t%s\t%s\t%s\t%s\n" % (vi.uid, vi.rsid, vj.uid, vj.rsid, "trans" if (vi.ref == a[i]) == (vj.ref == b[j]) else "cis"))
    return "".join(rows)


# ------------------------------------------------------------------------------------------------ tier 1: the designs, no kernel
def promised_blocks(d):
    """the oracle forms the blocks the design declares; -> its block rows, and the table line of the design"""
    blocks = hap_blocks(d, oracle_files(d.name, 0)["haplotypes"])
    assert sorted(tuple(v.uid for v in vs) for vs, _, _ in blocks) == d.block_uids()
    ids = [v.id for c in d.chrom_list for v in d.vars[c] if v.id != "."]
    assert len(ids) == len(set(ids)) and all(v.ref not in v.alt.split(",") for c in d.chrom_list for v in d.vars[c])
    sizes = [len(m) for _, m in d.blocks]
    thread = [n for n in sizes if n <= xi.ROW_WAVE_MIN]; wave = [n for n in sizes if n > xi.ROW_WAVE_MIN]
    print("%-17s lines %5d  variants %5d  blocks %3d: by a thread %s, by a wave %s  allele_config rows %d  options %s" % (
        d.name, d.n_lines, sum(len(d.vars[c]) for c in d.chrom_list), len(sizes), sorted(set(thread)), sorted(set(wave)), sum(n * (n - 1) for n in sizes), d.options))
    assert d.n_lines <= 8000 and max(sizes) <= 193
    return blocks, thread, wave


def test_genotypes_design_holds_what_it_promises():
    d = xi.genotypes()
    blocks, thread, wave = promised_blocks(d)
    assert set(thread) == {2, 3, 16} and set(wave) == {17, 65}
    assert [n for _, n, _, _ in xi.GENOTYPE_BLOCKS] == [len(vs) for vs, _, _ in blocks]                                # (file order = design order: one chromosome, ascending)
    seen = set()
    for (name, n, kinds, truth), (vs, a, b) in zip(xi.GENOTYPE_BLOCKS, blocks):
        assert [v.kind for v in vs] == list(kinds)
        ra = [v.ref == x for v, x in zip(vs, a)]; rb = [v.ref == x for v, x in zip(vs, b)]
        both_alt = [not x and not y for x, y in zip(ra, rb)]                                                           # the members with B_i == A_i
        assert both_alt == [k in xi.BOTH_ALT for k in kinds] and not any(x and y for x, y in zip(ra, rb))
        if name.startswith("mixed"):
            assert both_alt[0] and both_alt[n // 2] and both_alt[-1] and (n == 2 or not all(both_alt))
            assert n == 2 or set(kinds) == set(xi.KINDS)
        if name.startswith("only_both_alt"):
            assert all(both_alt) and not any(rb)                                                                       # NB = 0
        if name.startswith("no_both_alt"):
            assert not any(both_alt) and any(ra) and any(rb)
        if name.startswith("hap_a_is_ref"):
            assert all(ra) and not any(rb)
        seen |= set(kinds)
    assert seen == set(xi.KINDS) and d.options == [{}, {"unique_ids": 1}]
    singles = [r.split("\t") for r in rows_of(oracle_files(d.name, 0)["haplotypes"]) if r.split("\t")[4] == "1"]
    assert {"0|1", "1|0", "-|-"} <= {f[12] for f in singles} and any("_" in f[5] for f in singles)                     # unphased singletons; ID '.': the uid is the name


def test_block_sizes_design_holds_what_it_promises():
    d = xi.block_sizes()
    blocks, thread, wave = promised_blocks(d)
    assert sorted(thread) == [2, 3, 16] and sorted(wave) == [17, 63, 64, 65, 127, 128, 129, 193] and d.n_bams == 2
    assert d.options == [{}, {"haplo_count_bam_exclude": [0]}]
    ase = [r.split("\t") for r in rows_of(oracle_files(d.name, 0)["haplotypic_counts"]) if r.split("\t")[4] != "1"]
    per_bam = {b: sorted(int(f[4]) for f in ase if f[15] == b) for b in d.bam_names}
    assert per_bam["bam0"] == sorted(xi.BLOCK_SIZES) and per_bam["bam1"] == sorted(set(xi.BLOCK_SIZES) - {3})         # a block without a row of BAM 1
    ase = [r.split("\t") for r in rows_of(oracle_files(d.name, 1)["haplotypic_counts"])]
    assert ase and {f[15] for f in ase} == {"bam1"}


EXPECTED_LIVE = {(129, "first_round"): [0, 64, 1], (129, "middle_round"): [64, 0, 1], (129, "last_partial_round"): [64, 64, 0], (129, "all_but_one"): [0, 1, 0],
                 (129, "exactly_one"): [63, 64, 1], (129, "every_second"): [32, 32, 0],
                 (193, "first_round"): [0, 64, 64, 1], (193, "middle_round"): [64, 0, 64, 1], (193, "last_partial_round"): [64, 64, 64, 0], (193, "all_but_one"): [0, 1, 0, 0],
                 (193, "exactly_one"): [64, 63, 64, 1], (193, "every_second"): [32, 32, 32, 0]}


def test_blacklist_rounds_design_holds_what_it_promises():
    d = xi.blacklist_rounds()
    blocks, thread, wave = promised_blocks(d)
    assert not thread and sorted(set(wave)) == [129, 193] and len(d.patterns) == len(EXPECTED_LIVE) == 12
    for (name, n, black), (c, members) in zip(d.patterns, d.blocks):
        live = [sum(1 for t in range(t0, min(n, t0 + xi.WAVE)) if t not in set(black)) for t0 in range(0, n, xi.WAVE)]
        print("    %3d members, %-18s live members per round of 64 lanes %s" % (n, name, live))
        assert live == EXPECTED_LIVE[(n, name)] and all((c, members[t]) in d.black for t in black)
    ase = [r.split("\t") for r in rows_of(oracle_files(d.name, 0)["haplotypic_counts"])]
    assert sorted((int(f[4]), int(f[6])) for f in ase) == sorted((sum(EXPECTED_LIVE[k]), k[0] - sum(EXPECTED_LIVE[k])) for k in EXPECTED_LIVE)
    assert [o.get("output_read_ids") for o in d.options] == [0, 1]
    assert len(rows_of(oracle_files(d.name, 1)["haplotypic_counts"])[0].split("\t")) == 20


def test_string_lengths_design_holds_what_it_promises():
    d = xi.string_lengths()
    promised_blocks(d)
    vs = d.vars["chrL"]
    ids = {len(v.id) for v in vs}; refs = {len(v.ref) for v in vs}; alts = {len(v.alt) for v in vs}; digits = {len(str(v.pos)) for v in vs}
    uid8 = {len(v.uid) % 8 for v in vs}
    print("    ID lengths %d-%d, REF lengths %d-%d, ALT lengths %d-%d, uid lengths mod 8 %s, position digits %s" % (
        min(ids), max(ids), min(refs), max(refs), min(alts), max(alts), sorted(uid8), sorted(digits)))
    assert set(range(1, 25)) <= ids and set(range(1, 41)) <= refs and set(range(1, 41)) <= alts and uid8 == set(range(8)) and digits == set(range(1, 11))
    assert {1, 9, 10, 99, 100} <= {v.pos for v in vs} and max(v.pos for v in vs) == 2147483000 < 2 ** 31
    hap = [r.split("\t") for r in rows_of(oracle_files(d.name, 0)["haplotypes"])]
    assert any(f[1:3] == ["0", "1"] and f[4] == "1" for f in hap)                                                      # pos - 1 at pos = 1
    assert any(f[1:4] == ["9", "100", "91"] for f in hap)                                                              # a block from position 9 (one digit) to 100 (three)
    for kind in ("2", "1"):                                                                                            # a two-variant block and a singleton per count pair
        counts = {tuple(sorted((int(f[7]), int(f[8])))) + (int(f[9]),) for f in hap if f[4] == kind}
        assert {(9, 10, 19), (99, 100, 199), (999, 1000, 1999)} <= counts, (kind, counts)
    assert any(f[1] == "2147482999" and f[2] == "2147483000" for f in hap)


def kernel_rows(d, files):
    """row lengths per staged text of a one-BAM, one-chromosome design in the row order of the writers (launch_rows), from the oracle's text: the block files in file order,
    the singleton files one row per covered variant in first-appearance order (= the rows of allelic_counts), length 0 for a member of a block"""
    assert d.n_bams == 1 and len(d.chrom_list) == 1
    L = lambda r: len(r) + 1
    uid_of = {v.rsid: v.uid for c in d.chrom_list for v in d.vars[c]}
    keys = [r.split("\t")[2] for r in rows_of(files["allelic_counts"])]
    hap = rows_of(files["haplotypes"]); ase = rows_of(files["haplotypic_counts"])
    hap_blk = [r for r in hap if r.split("\t")[4] != "1"]; hap_one = {uid_of[r.split("\t")[5]]: L(r) for r in hap if r.split("\t")[4] == "1"}
    ase_blk = [r for r in ase if r.split("\t")[4] != "1"]; ase_one = {r.split("\t")[3]: L(r) for r in ase if r.split("\t")[4] == "1"}
    assert [r.split("\t")[3].split(",") for r in ase_blk] == [[uid_of[x] for x in r.split("\t")[5].split(",")] for r in hap_blk]      # one row per block, in block order
    assert set(hap_one) <= set(keys) and set(hap_one) == set(ase_one)
    return {"conn": [L(r) for r in rows_of(files["variant_connections"])], "hap": [L(r) for r in hap_blk], "ase": [L(r) for r in ase_blk],
            "allelic": [L(r) for r in rows_of(files["allelic_counts"])], "single_ase": [ase_one.get(k, 0) for k in keys], "single_hap": [hap_one.get(k, 0) for k in keys],
            "cfg": [L(r) for r in rows_of(files["allele_config"])]}


def test_stage_overflow_design_holds_what_it_promises():
    d = xi.stage_overflow()
    promised_blocks(d)
    rows = kernel_rows(d, oracle_files(d.name, 0))
    assert set(rows) == set(xi.LAUNCH)
    for f, (n_rows, stage) in xi.LAUNCH.items():
        groups = [sum(rows[f][r0:r0 + n_rows]) for r0 in range(0, len(rows[f]), n_rows)]
        groups = [g for g in groups if g]                                                                              # (a workgroup without a byte returns at once)
        staged = [g for g in groups if g + 16 < stage]; unstaged = [g for g in groups if g > stage + 16]              # the kernels add up to 15 bytes of misalignment
        print("    %-10s %3d rows / %5d B per workgroup: %2d workgroups staged (largest %5d B), %2d written directly (smallest %6d B)" % (
            f, n_rows, stage, len(staged), max(staged, default=0), len(unstaged), min(unstaged, default=0)))
        assert staged and unstaged and len(staged) + len(unstaged) == len(groups), f
    alts = [len(v.alt) for v in d.vars["chrO"] if len(v.alt) > 1]
    assert 40 <= min(alts) and max(alts) <= 201 and len(set(alts)) > 100


def test_wide_members_design_holds_what_it_promises():
    d = xi.wide_members()
    blocks, thread, wave = promised_blocks(d)
    assert sorted(thread) == [3, 3, 3] and wave == [17]
    vs = d.vars["chrW"]
    where = {}
    for kind, v in d.wide:
        x = vs[v]
        ctx = next((len(m) for _, m in d.blocks if v in m), 1)
        longest = max(len(x.uid), len(x.rsid), len(x.alleles[0]), len(x.alleles[1]))
        where.setdefault(kind, []).append((ctx, len(x.uid), longest >= xi.WIDE))
    print("    " + "  ".join("%s: %s" % (k, sorted(w)) for k, w in where.items()))
    assert sorted(c for c, _, _ in where["uid_65535"]) == [1, 3, 17] and all(n == 65535 and not wide for _, n, wide in where["uid_65535"])      # uint16 holds it
    assert sorted(c for c, _, _ in where["uid_65536"]) == [1, 3, 17] and all(n == 65536 and wide for _, n, wide in where["uid_65536"])
    assert sorted(c for c, _, _ in where["allele_70000"]) == [1, 3, 17] and all(wide for _, _, wide in where["allele_70000"])
    assert all(len(vs[v].alleles[1]) == 70000 for k, v in d.wide if k == "allele_70000")
    assert any(vs[v].id == "." for k, v in d.wide if k == "uid_65536")


def test_chromosome_gaps_design_holds_what_it_promises():
    d = xi.chromosome_gaps()
    blocks, thread, wave = promised_blocks(d)
    per = {c: (sum(1 for cc, _ in d.blocks if cc == c), len(d.saved["tally"][c]["line_var"]) > 0, len(d.vars[c])) for c in d.chrom_list}
    print("    " + "  ".join("%s: blocks %d covered %s variants %d" % ((c,) + per[c]) for c in d.chrom_list))
    assert [per[c][:2] for c in d.chrom_list] == [(2, True), (0, True), (2, True), (0, False)] and all(per[c][2] for c in d.chrom_list)
    cfg = rows_of(oracle_files(d.name, 0)["allele_config"])
    assert {r.split("_")[0] for r in cfg} == {"1", "chrom3"}


def test_the_mirrored_constants_are_those_of_the_kernels():
    src = open(os.path.join(REPO, "phaser_amd", "csrc", "phz_rowsdev.hip")).read()
    assert "#define PHZ_ROW_WAVE_MIN %d " % xi.ROW_WAVE_MIN in src
    K = lambda b: "%d * 1024" % (b // 1024)
    for text in ("launch_rows_of<RowConn, %d, %s, NO_WAVE>" % (xi.LAUNCH["conn"][0], K(xi.LAUNCH["conn"][1])),
                 "launch_rows_of<RowAllelic, %d, %s, NO_WAVE>" % (xi.LAUNCH["allelic"][0], K(xi.LAUNCH["allelic"][1])),
                 "launch_rows_of<RowSingleAse, %d, %s, NO_WAVE>" % (xi.LAUNCH["single_ase"][0], K(xi.LAUNCH["single_ase"][1])),
                 "launch_rows_of<RowSingleHap, %d, %s, NO_WAVE>" % (xi.LAUNCH["single_hap"][0], K(xi.LAUNCH["single_hap"][1])),
                 "k_cfg_write<%d, %s>" % (xi.LAUNCH["cfg"][0], K(xi.LAUNCH["cfg"][1])),
                 "#define PHZ_HAP_ROWS %d\n" % xi.LAUNCH["hap"][0], "#define PHZ_HAP_STAGE (%s)\n" % K(xi.LAUNCH["hap"][1]),
                 "#define PHZ_ASE_ROWS %d\n" % xi.LAUNCH["ase"][0], "#define PHZ_ASE_STAGE (%s)\n" % K(xi.LAUNCH["ase"][1])):
        assert text in src, text


def test_design_order_puts_small_designs_after_the_heavy_ones():
    order = [d.name for d in xi.all_designs()]
    assert len(order) == len(DESIGNS) == 7 and order.index("blacklist_rounds") < order.index("string_lengths") and order[-1] == "chromosome_gaps"


# ------------------------------------------------------------------------------------------------ tiers 2 and 3: the kernels
def tally_of(ctx, d):
    """K_tally on the design's call lines, one chromosome per call -> the `saved` form with its results (what the row stages start from); a chromosome without a call
    line gets the empty results"""
    if isinstance(ctx, EmuContext):          # the emulated K_tally is most of an emulated run and is the same code in every variant of the row stage: once per design
        if d.name not in _EMU_TALLY:
            _EMU_TALLY[d.name] = _tally_of(EmuContext(emu_library()), d)
        return _EMU_TALLY[d.name]
    return _tally_of(ctx, d)


_EMU_TALLY = {}


def _tally_of(ctx, d):
    out = {"tally": {}, "n_qid": d.saved["n_qid"], "qnames": d.saved["qnames"]}
    for c in d.chrom_list:
        R = dict(d.saved["tally"][c]); nv = R["nv"]
        if len(R["line_var"]):
            got, sz = run_tally(ctx, {"tally": {c: R}, "n_qid": {c: d.saved["n_qid"][c]}}, [c], d.n_bams)
            R.update({k: got[k] for k in TALLY_KEYS})
        else:
            R.update({"var_count": np.zeros(nv * 3, np.int32), "var_first": np.full(nv, -1, np.int64), "var_distinct": np.zeros(nv * 3, np.int32),
                      "var_rank": np.full(nv, 0xFFFFFFFFFFFFFFFF, np.uint64), "ea": np.zeros(0, np.int32), "eb": np.zeros(0, np.int32), "cells": np.zeros(0, np.int32),
                      "linked": np.zeros(0, np.uint8)})
        out["tally"][c] = R
    return out


def engine_pass(ctx, d, vs, saved, device_rows, options):
    from phaser_amd.engine import Config, Engine

    class _M:
        device = None
    m = _M(); m.ctx = ctx
    eng = Engine(vs, d.bam_names, Config(device_rows=device_rows, haplo_blacklist=d.blacklist, include_indels=d.load.get("include_indels", 0), **options), mapper=m)
    eng.n_qid.update(saved["n_qid"]); eng.qnames.update(saved["qnames"])
    (stub_emu_stages if device_rows else stub_gpu_stages)(eng, saved)
    out = eng.finish()
    assert eng.rows_path == ("device" if device_rows else "host"), getattr(eng, "rows_fallback", "")
    return out


def first_difference(a, b):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return "lengths %d / %d, first difference at byte %d: %r / %r" % (len(a), len(b), n, a[max(0, n - 60):n + 40], b[max(0, n - 60):n + 40])


def check_design(ctx, d, reps=1, options=None):
    """K_tally, then per option set `reps` device passes over ONE variant set, the host row stage, the oracle, the restatement of allele_config"""
    from phaser_amd import vcf
    saved = tally_of(ctx, d)
    vs = vcf.load_variants(d.vcf_text, **d.load)
    assert [len(vs.chroms[c]) for c in d.chrom_list] == [len(d.vars[c]) for c in d.chrom_list] and list(vs.chroms) == d.chrom_list
    for oi in (range(len(d.options)) if options is None else options):
        opts = d.options[oi]
        first = None
        for rep in range(reps):
            out = engine_pass(ctx, d, vs, saved, True, opts)
            if first is None:
                first = out
            for name in OUTPUTS:
                assert out[name] == first[name], (d.name, opts, "pass %d" % rep, name, first_difference(out[name], first[name]))
        host = engine_pass(ctx, d, vs, saved, False, opts)
        want = oracle_files(d.name, oi)
        for name in OUTPUTS:
            assert first[name] == host[name], (d.name, opts, name, "device / host", first_difference(first[name], host[name]))
            assert canonical(name, first[name]) == canonical(name, want[name]), (d.name, opts, name, "device / oracle",
                                                                                 first_difference(canonical(name, first[name]), canonical(name, want[name])))
        assert sorted(tuple(v.uid for v in m) for m, _, _ in hap_blocks(d, first["haplotypes"])) == d.block_uids(), (d.name, opts)
        cfg = restated_config(d, first["haplotypes"])
        assert first["allele_config"] == cfg, (d.name, opts, "allele_config / restatement", first_difference(first["allele_config"], cfg))
        assert len(cfg.split("\n")) - 2 == sum(len(m) * (len(m) - 1) for _, m in d.blocks)


def check_sequence(ctx):
    for d in xi.all_designs():
        check_design(ctx, d, options=(len(d.options) - 1,))


EMU_VARIANTS = {"product_thresholds": {}, "rows_by_wave": {"row_wave_min": 0}, "blocks_beyond_tables": {"stat_n": 2}}
EMU_RUNS = [(n, "product_thresholds") for n in DESIGNS] + [(n, "rows_by_wave") for n in xi.THREAD_FORMATTED] + [("block_sizes", "blocks_beyond_tables")]


@pytest.mark.parametrize("name,variant", EMU_RUNS, ids=["%s-%s" % x for x in EMU_RUNS])
def test_emulated_writers_match_host_rows_oracle_and_restatement(name, variant):
    check_design(EmuContext(emu_library(**EMU_VARIANTS[variant])), DESIGNS[name])


@pytest.mark.parametrize("name", ["wide_members"])
def test_wide_member_records_are_marked_on_the_right_side_of_65536(name):
    """the 65,535-byte uid must come out whole through the 16-bit lengths and the 65,536-byte one through the pools: the rows that carry them, by length, in the text
    the emulated writers produced (allele_config: 2 (n - 1) rows per member of a block of n)"""
    d = DESIGNS[name]
    ctx = EmuContext(emu_library())
    from phaser_amd import vcf
    out = engine_pass(ctx, d, vcf.load_variants(d.vcf_text, **d.load), tally_of(ctx, d), True, {})
    vs = d.vars["chrW"]
    for kind, v in d.wide:
        n = next((len(m) for _, m in d.blocks if v in m), 1)
        first = [r for r in rows_of(out["allele_config"]) if r.split("\t")[0] == vs[v].uid]
        second = [r for r in rows_of(out["allele_config"]) if r.split("\t")[2] == vs[v].uid]
        assert len(first) == len(second) == (n - 1 if n > 1 else 0), (kind, n)
        assert sum(1 for r in rows_of(out["allelic_counts"]) if r.split("\t")[2] == vs[v].uid and r.split("\t")[4] == vs[v].alleles[1]) == 1, kind


@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DESIGNS))
def test_product_writers_match_host_rows_oracle_and_restatement(gpu_ctx, name):
    check_design(gpu_ctx, DESIGNS[name], reps=2)


@pytest.mark.gpu
def test_product_writers_leave_the_context_clean_over_all_designs(gpu_ctx):
    check_sequence(gpu_ctx)
