"""The kernels of the row stage between the tally and block phasing and between phasing and the text writers (phaser_amd/csrc/phz_rowsdev.hip: k_pair_keys, k_keep; the
ordering stage order_variants_and_pairs / key_stage with k_iota_rank ... k_block_counts; k_blocks, k_gather_nsub, k_blk_edges, k_blk_stats, k_vcf_blocks) on the designed
call lines of tests/rowstage_inputs.py, under the host-side emulation and on the product build on an MI355X.  Everything is compared as text, integers or bit patterns.

Three tiers, as in tests/test_rowtext_limits.py.  The test_*_design_holds_what_it_promises tests run no kernel: from tests/rowstage_restatement.py and the files
oracle/phasing_oracle.py writes on the design's call lines they check that the p-values, thresholds, colliding home slots, swapped pairs, empty segments, gwStat kinds and
MAF weights the design promises are there (and that restatement and oracle agree), and print one line per design.  Then the kernels, emulated and on the GPU: per design
and option set the device rows equal the host rows (phz_rows.cpp) byte for byte, both equal the oracle under canonical(), log and phased count agree, and the stage's
own results -- the pair-key set, the counters and per-chromosome tables of phz_rowsdev_result, the row order of variant_connections.txt, the block rows of haplotypes.txt
in block order, the per-block arrays behind the phased VCF -- equal the restatement."""
import contextlib
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import rowstage_inputs as xi
import rowstage_restatement as rr
from conftest import REPO
from helpers import OUTPUTS, EmuContext, canonical, emu_library, stub_emu_stages, stub_gpu_stages
from test_rowtext_limits import _tally_of, first_difference

DESIGNS = {d.name: d for d in xi.all_designs()}
PS_EMPTY = 0xFFFFFFFFFFFFFFFF          # an empty slot of the pair-key set (phz_rowsdev.hip)


# ------------------------------------------------------------------------------------------------ shared: the oracle's files, the restatement
@functools.lru_cache(maxsize=None)
def oracle_run(name, option):
    """(the five files, noise, log, phased variants) of oracle/phasing_oracle.py on the design's call lines under its option set `option`: computed once, read-only"""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import phasing_oracle as po
    d = DESIGNS[name]
    ph = po.Phaser(d.bam_names, as_q_cutoff=0, **d.options[option])
    for b in range(d.n_bams):
        ph.add_bam(d.call_texts(b, option))
    return ph.finish(), ph.noise, list(ph.log), ph.phased


@functools.lru_cache(maxsize=None)
def restated(name, option):
    return rr.restate(DESIGNS[name], option)


def rows_of(text):
    return text.split("\n")[1:-1]


def block_rows(hap_text):
    return [r for r in rows_of(hap_text) if int(r.split("\t")[4]) >= 2]


def check_conn_order(d, r, conn_text, who):
    """row order of variant_connections.txt: the first variants in the restated order exactly, the rows of one first variant as a set (the reference walks a set there:
    SURVEY.md 8.1 rule 6)"""
    got = rows_of(conn_text); want = rr.conn_rows(d, r)
    assert [x.split("\t")[0] for x in got] == [x.split("\t")[0] for x in want], (d.name, who)
    assert sorted(got) == sorted(want), (d.name, who)


def check_restatement(d, oi):
    """the restatement against oracle/phasing_oracle.py: noise, pair rows and their order, first-appearance order, components in block order, the statistics of every block
    -> (restatement, block facts of the oracle's haplotypes.txt)"""
    files, noise, log, phased = oracle_run(d.name, oi)
    r = restated(d.name, oi)
    assert r.noise == noise and noise > 0, (d.name, r.noise, noise)
    check_conn_order(d, r, files["variant_connections"], "oracle")
    assert log[-1].strip().startswith("%d variant connections dropped" % sum(p.dropped for p in r.pairs))
    # rule 2: allelic_counts lists the covered variants with a ref / alt read in first-appearance order, BAM by BAM
    has = lambda c, v: any(k < 2 for b in range(d.n_bams) for q, calls in d.reads[c][b] for x, k in calls if x == v)
    want = [d.vars[c][v].uid for b in range(d.n_bams) for c in d.chrom_list for v in r.keys[(b, c)] if has(c, v)]
    assert [x.split("\t")[2] for x in rows_of(files["allelic_counts"])] == want, d.name
    # components in block order: the blocks of the file lie in their components, and the components come in restated order
    facts = rr.block_facts(d, oi, r, files["haplotypes"])
    where = []
    for f in facts:
        k = [i for i, (c, m) in enumerate(r.components) if c == f["chrom"] and set(f["members"]) <= set(m)]
        assert len(k) == 1, (d.name, f["members"])
        where.append(k[0])
    assert where == sorted(where), (d.name, where)
    assert sum(len(f["members"]) for f in facts) == phased
    for f, row in zip(facts, block_rows(files["haplotypes"])):
        assert rr.hap_row_fields(f) == row.split("\t")[10:16], (d.name, oi, row)
    # max_haplo_maf of the block rows of haplotypic_counts.txt (column 14 without read ids), blocks identified by their variants
    by_vars = {",".join(d.vars[f["chrom"]][v].uid for v in f["members"]): f for f in facts}
    seen = 0
    for row in rows_of(files["haplotypic_counts"]):
        x = row.split("\t")
        if x[3] in by_vars:
            assert x[14] == by_vars[x[3]]["maf_text"], (d.name, oi, x[3], x[14]); seen += 1
    assert seen >= len(facts)
    return r, facts


def summary(d, r0):
    print("%-14s lines %4d  variants %3d  BAMs %d  noise %.6f  pairs %2d (tested keys %2d)  components %2d  options %s" % (
        d.name, d.n_lines, d.n_vars, d.n_bams, r0.noise, len(r0.pairs), len(r0.tested), len(r0.components), d.options))
    assert d.n_lines <= 3000 and d.n_vars <= 400
    # every QNAME is one read of one BAM (ids are per chromosome)
    assert all(len({q for q, calls in d.reads[c][b]}) == len(d.reads[c][b]) for c in d.chrom_list for b in range(d.n_bams))
    assert all(not ({q for q, _ in d.reads[c][b]} & {q for q, _ in d.reads[c][b2]}) for c in d.chrom_list for b in range(d.n_bams) for b2 in range(b))


def pair_of(d, r, ab, chrom=None):
    c = chrom or d.chrom_list[0]
    got = [p for p in r.pairs if p.chrom == c and {p.a, p.b} == set(ab)]
    return got[0] if got else None


# ------------------------------------------------------------------------------------------------ tier 1: the designs, no kernel
def test_verdicts_design_holds_what_it_promises():
    d = xi.verdicts()
    m = d.marks
    per = [check_restatement(d, oi) for oi in range(len(d.options))]
    r0 = per[0][0]
    summary(d, r0)
    P = lambda r, name: pair_of(d, r, m[name])
    key = lambda p: (p.sup, p.tot)
    assert [o.get("cc_threshold") for o in d.options[:3]] == [None, 0.0, 1.0]
    # default threshold: p strictly between 0 and 1 on both sides of 0.01
    assert key(P(r0, "kept_8_10")) == (8, 10) and 0.01 < P(r0, "kept_8_10").p < 1 and not P(r0, "kept_8_10").dropped
    assert key(P(r0, "equal_7_10")) == key(P(r0, "with_other")) == xi.EQUAL_KEY and 0 < P(r0, "equal_7_10").p < 0.01 and P(r0, "equal_7_10").dropped
    assert P(r0, "with_other").other == 2 and P(r0, "with_other").cis + P(r0, "with_other").trans == 8
    assert key(P(r0, "dropped_6_10")) == (6, 10) and 0 < P(r0, "dropped_6_10").p < P(r0, "equal_7_10").p and P(r0, "dropped_6_10").dropped
    assert P(r0, "no_conflict").p == 1 and isinstance(P(r0, "no_conflict").p, int) and P(r0, "no_conflict").tot == P(r0, "no_conflict").sup == 3
    t = P(r0, "tie_kept")
    assert t.cis == t.trans == 1 and t.cfg == -1 and t.conc == "." and not t.dropped
    t = P(r0, "tie_dropped")
    assert t.cis == t.trans == 5 and t.cfg == -1 and t.conc == "." and t.dropped
    # no linked pair is without a supporting read: the pair with nothing but other-class overlap is no pair, and its class-2 variant has no ref / alt read
    assert P(r0, "only_other") is None and all(p.sup > 0 for r, _ in per for p in r.pairs)
    # the dropped pair that isolates its two variants, the bridge, the side of the triangle
    comps = lambda r: [tuple(mm) for c, mm in r.components]
    assert not set(m["dropped_6_10"]) & {v for mm in comps(r0) for v in mm}
    br = m["bridge"]; tr = m["triangle"]
    assert pair_of(d, r0, br[1:3]).dropped and key(pair_of(d, r0, br[1:3])) == (6, 10) and tuple(br[:2]) in comps(r0) and tuple(br[2:]) in comps(r0)
    assert pair_of(d, r0, (tr[0], tr[2])).dropped and tuple(tr) in comps(r0)
    # cc_threshold 0.0: nothing dropped, the big tie enters phasing (a component without a block); 1.0: only p = 1 survives
    r1, f1 = per[1]
    assert not any(p.dropped for p in r1.pairs) and tuple(m["tie_dropped"]) in comps(r1) and tuple(br) in comps(r1)
    assert not any(set(f["members"]) & set(m["tie_dropped"]) for f in f1)
    r2 = per[2][0]
    assert all(p.dropped == (p.p != 1) for p in r2.pairs) and sum(not p.dropped for p in r2.pairs) == 5
    # the threshold equal to p(7, 10): kept; the next smaller p of the design is p(6, 10): dropped
    r3 = per[3][0]
    cc = d.options[3]["cc_threshold"]
    ps = sorted({p.p for p in r3.pairs})
    assert cc == P(r3, "equal_7_10").p == xi.p_of(r3.noise, *xi.EQUAL_KEY) and not P(r3, "equal_7_10").dropped and not P(r3, "with_other").dropped
    assert ps[ps.index(cc) - 1] == P(r3, "dropped_6_10").p and P(r3, "dropped_6_10").dropped and ps.index(cc) >= 2
    assert [sum(p.dropped for p in r.pairs) for r, _ in per] == [6, 0, 8, 4]
    print("    p by (supporting, total): %s" % "  ".join("%s %.6g" % (k, v) for k, v in sorted({key(p): p.p for p in r0.pairs}.items())))


@pytest.mark.parametrize("n_keys", [16, 17])
def test_pair_table_design_holds_what_it_promises(n_keys):
    d = xi.pair_table(n_keys)
    r, facts = check_restatement(d, 0)
    summary(d, r)
    assert len(r.tested) == n_keys == len(set(d.marks["keys"])) and set(r.tested) == set(d.marks["keys"]) and len(r.pairs) == n_keys + 1
    homes = [xi.home_slot(s, t, 16) for s, t in r.tested]
    assert homes.count(15) >= 3          # three keys collide on the last slot: at least two probe sequences wrap to slot 0, whatever the order of insertion
    assert xi.ps_hash(0) == 0 and xi.ps_hash(1) == 0x34C2CB2C          # (the low words of MurmurHash3's fmix64(0) = 0 and fmix64(1) = 0xb456bcfc34c2cb2c)
    assert [e.get("PHZ_ROWS_PAIR_SLOTS") for e in d.env] == ["16", "64", None]
    print("    home slots of the %d keys among 16: %s" % (n_keys, sorted(homes)))


def test_ordering_design_holds_what_it_promises():
    d = xi.ordering()
    r, facts = check_restatement(d, 0)
    summary(d, r)
    m = d.marks
    A, M, C_ = d.chrom_list
    assert d.n_bams == 3 and not any(d.reads[M][b] for b in range(3)) and not d.reads[A][0] and d.reads[C_][0]
    assert r.chroms == [C_, A] and r.first_bam == {C_: 0, A: 1}                                   # chrC's blocks come before chrA's
    hi, low = m["hi"], m["low"]
    assert r.rank[C_][0] == hi[2] == max(hi) and min(hi) > max(low)                               # the highest variant of its component is the first key
    comps = [(c, tuple(mm)) for c, mm in r.components]
    assert comps.index((C_, tuple(hi))) < comps.index((C_, tuple(low)))                           # block order is not position order
    assert [f["members"] for f in facts][:2] == [hi, low]
    p = pair_of(d, r, (hi[0], hi[2]), C_)
    assert (p.a, p.b) == (hi[2], hi[0]) and p.a > p.b                                             # the pair the tally holds as (hi0, hi2) is turned round
    assert any(q.a < q.b for q in r.pairs)
    c, v = m["bam2_only_single"]
    assert r.keys[(2, c)] == [v] and all(v not in r.keys[(b, c)] for b in (0, 1))
    assert r.keys[(2, A)] == m["bam2_only_block"]
    for c, v in m["unlinked"]:
        assert any(v in r.keys[(b, c)] for b in range(3)) and v not in r.rank[c]
    for c, v in m["uncovered"]:
        assert not any(v in r.keys[(b, c)] for b in range(3))
    segs = [bool(r.keys[(b, c)]) for b in range(3) for c in d.chrom_list]
    assert segs == [False, False, True, True, False, False, True, False, True]                   # empty segments before, between and after segments with keys
    print("    segments (BAM, chromosome) with keys: %s   rank of chrC: %s" % ("".join("x" if s else "." for s in segs), r.rank[C_]))


def test_block_stats_design_holds_what_it_promises():
    d = xi.block_stats()
    per = [check_restatement(d, oi) for oi in range(len(d.options))]
    summary(d, per[0][0])
    assert d.options == [{}, {"gw_phase_method": 1}, {"max_block_size": 2}]
    m = d.marks
    F = lambda oi, name: next(f for f in per[oi][1] if f["members"] == m[name])
    sym = lambda xs: "".join("-" if x is None else str(x) for x in xs)
    for oi in (0, 1):
        assert F(oi, "all_equal")["kind"] == "int1" and sym(F(oi, "all_equal")["phase"]) == "000"
        assert F(oi, "none_phased")["kind"] == "half" and sym(F(oi, "none_phased")["phase"]) == "---"
    # by the mean
    assert (F(0, "half")["kind"], F(0, "half")["stat"], sym(F(0, "half")["cor"])) == ("mean", 0.5, "01")
    assert (F(0, "two_thirds")["stat"], sym(F(0, "two_thirds")["phase"]), sym(F(0, "two_thirds")["cor"])) == (2 / 3, "011", "111")
    assert (F(0, "one_third")["stat"], sym(F(0, "one_third")["phase"]), sym(F(0, "one_third")["cor"])) == (1 - 1 / 3, "001", "000")
    assert (F(0, "unknown_among_known")["kind"], rr.stat_text(F(0, "unknown_among_known")), sym(F(0, "unknown_among_known")["phase"])) == ("mean", "1.0", "0-0-")
    # by MAF weight: w0 == w1 (the annotated phase stays), w0 > w1 and w1 > w0 against the mean's verdict, no weight at all
    f = F(1, "half")
    assert f["kind"] == "maf" and f["w"][0] == f["w"][1] == 0.25 and f["stat"] == 0.5 and sym(f["cor"]) == "01"
    f = F(1, "two_thirds")
    assert f["kind"] == "maf" and f["w"][0] > f["w"][1] > 0 and sym(f["cor"]) == "000"
    f = F(1, "one_third")
    assert f["kind"] == "maf" and 0 < f["w"][0] < f["w"][1] and sym(f["cor"]) == "111"
    for name in ("no_weight", "no_weight_int_first"):
        f = F(1, name)
        assert f["kind"] == "mean" and f["w"] == [0, 0] and f["stat"] == F(0, name)["stat"] and f["cor"] == F(0, name)["cor"]
    # the member whose maf is printed: the first of two tied ones, also where the tie is between the float 0.0 and the int 0
    vs = d.vars["chrS"]
    assert vs[m["half"][0]].maf == vs[m["half"][1]].maf == 0.25 and F(1, "half")["maxmaf"] == m["half"][0]
    assert (F(1, "no_weight")["maxmaf"], F(1, "no_weight")["maf_text"]) == (m["no_weight"][0], "0.0")
    assert (F(1, "no_weight_int_first")["maxmaf"], F(1, "no_weight_int_first")["maf_text"]) == (m["no_weight_int_first"][0], "0")
    assert F(1, "unknown_among_known")["maxmaf"] == m["unknown_among_known"][1] and vs[m["unknown_among_known"][1]].gt == "0/1"
    # a kept tie pair inside a block is not counted
    r0 = per[0][0]
    t = m["tie_inside"]
    assert pair_of(d, r0, (t[0], t[2])).cfg == -1 and not pair_of(d, r0, (t[0], t[2])).dropped and (F(0, "tie_inside")["sup"], F(0, "tie_inside")["tot"]) == (2, 2)
    # the conflict: no block at the default size, two final blocks under --max_block_size 2 with two kept pairs between them
    s = m["split"]
    assert not any(set(f["members"]) & set(s) for f in per[0][1])
    halves = [f for f in per[2][1] if set(f["members"]) & set(s)]
    assert [f["members"] for f in halves] == [s[:2], s[2:]] and [(f["sup"], f["tot"]) for f in halves] == [(1, 1), (1, 1)]
    inside = [p for p in per[2][0].pairs if {p.a, p.b} <= set(s)]
    assert len(inside) == 4 and not any(p.dropped or p.cfg < 0 for p in inside)
    kinds = {f["kind"] for oi in range(3) for f in per[oi][1]}
    assert kinds == {"int1", "half", "mean", "maf"}
    assert max(len([x for x in f["phase"] if x is not None]) for f in per[0][1] if f["kind"] == "mean") > 2          # beyond a table of two, for the stat_n = 2 variant


def test_the_restated_hash_is_the_one_of_the_kernels():
    src = open(os.path.join(REPO, "phaser_amd", "csrc", "phz_rowsdev.hip")).read()
    assert "k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;" in src
    assert "constexpr unsigned long long PS_EMPTY = ~0ull;" in src
    assert "((unsigned long long)(uint32_t)tot[e] << 32) | (uint32_t)sup[e]" in src


# ------------------------------------------------------------------------------------------------ tiers 2 and 3: the kernels
class Spy:
    """what the row stage's native calls returned during a pass: the pair-key tables of phz_rowsdev_pair_keys with their status, the phz_rowsdev_result of the run"""

    def __init__(self, lib, n_chrom):
        self.lib = lib; self.n_chrom = n_chrom; self.tables = []; self.result = None

    def __enter__(self):
        lib = self.lib
        self.real = (lib.phz_rowsdev_pair_keys, lib.phz_rowsdev_run)

        def pair_keys(ctx_h, th, keys_p):
            st = self.real[0](ctx_h, th, keys_p)
            n = int(lib.phz_rowsdev_pair_slots(th))
            self.tables.append((int(st), n, np.frombuffer(C.string_at(keys_p.value, n * 8), np.uint64).copy()))
            return st

        def run(ctx_h, th, o, pv, off, txt, res):
            st = self.real[1](ctx_h, th, o, pv, off, txt, res)
            R = res._obj
            if st == 0:
                self.result = {k: int(getattr(R, k)) for k in ("n_linked", "dropped", "n_components", "n_blocks", "phased", "n_blk_vars")}
                self.result["chrom_blocks"] = [int(R.chrom_blocks[i]) for i in range(self.n_chrom)]
                self.result["chrom_first_bam"] = [int(R.chrom_first_bam[i]) for i in range(self.n_chrom)]
            return st
        lib.phz_rowsdev_pair_keys = pair_keys; lib.phz_rowsdev_run = run
        return self

    def __exit__(self, *exc):
        self.lib.phz_rowsdev_pair_keys, self.lib.phz_rowsdev_run = self.real


def engine_pass(ctx, d, vs, saved, device_rows, options):
    """-> (the five files, the Engine)"""
    from phaser_amd.engine import Config, Engine

    class _M:
        device = None
    m = _M(); m.ctx = ctx
    eng = Engine(vs, d.bam_names, Config(device_rows=device_rows, **options), mapper=m)
    eng.n_qid.update(saved["n_qid"]); eng.qnames.update(saved["qnames"])
    (stub_emu_stages if device_rows else stub_gpu_stages)(eng, saved)
    out = eng.finish()
    assert eng.rows_path == ("device" if device_rows else "host"), getattr(eng, "rows_fallback", "")
    return out, eng


_EMU_TALLY = {}


def tally_of(ctx, d):
    if isinstance(ctx, EmuContext):          # the emulated K_tally is the same code in every variant of the row stage: once per design
        if d.name not in _EMU_TALLY:
            _EMU_TALLY[d.name] = _tally_of(EmuContext(emu_library()), d)
        return _EMU_TALLY[d.name]
    return _tally_of(ctx, d)


def check_pair_table(ctx, d, r, spy, slots):
    """the last table of the pass holds exactly the distinct tested keys, each reachable by linear probing from its restated home slot; a table started at `slots` slots that
    cannot hold them reports PHZ_E_CAPACITY and is redone once, four times as large"""
    from phaser_amd import _lib
    n_keys = len(r.tested)
    want_status = [_lib.PHZ_OK]; sizes = [slots]
    if slots is not None and n_keys > slots:
        want_status = [_lib.PHZ_E_CAPACITY, _lib.PHZ_OK]; sizes = [slots, 4 * slots]
    assert [t[0] for t in spy.tables] == want_status, (d.name, slots, [t[:2] for t in spy.tables])
    if slots is not None:
        assert [t[1] for t in spy.tables] == sizes
    st, n, keys = spy.tables[-1]
    assert n & (n - 1) == 0 and n >= n_keys
    used = np.empty(n, np.uint32); sup = np.empty(n, np.float64); tot = np.empty(n, np.int64)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    k = int(ctx.lib.phz_pair_slots_used(vp(keys), n, vp(used), vp(sup), vp(tot)))
    assert k == n_keys == int((keys != np.uint64(PS_EMPTY)).sum()), (d.name, k, n_keys)
    got = sorted((int(s), int(t)) for s, t in zip(sup[:k], tot[:k]))
    assert got == r.tested, (d.name, got)
    occupied = keys != np.uint64(PS_EMPTY)
    for slot in np.flatnonzero(occupied).tolist():
        key = int(keys[slot]); s, t = key & 0xFFFFFFFF, key >> 32
        at = xi.home_slot(s, t, n)
        steps = 0
        while at != slot:
            assert occupied[at] and steps < n, (d.name, (s, t), "home", xi.home_slot(s, t, n), "slot", slot)
            at = (at + 1) & (n - 1); steps += 1
    return n


def check_blocks(d, eng, facts, who):
    """the per-block arrays behind the phased VCF (phz_rowsdev_fetch_blocks / the host stage's) against the restatement, in block order"""
    at = 0
    for c, v, first in eng.vcf_blocks:
        assert first == at, (d.name, who)
        o = 0
        for b in range(len(v["size"])):
            f = facts[at]; n = int(v["size"][b])
            assert f["chrom"] == c and v["var"][o:o + n].tolist() == f["members"] and v["hap"][o:o + n].tolist() == f["alleles"], (d.name, who, at)
            cor = [-1 if x is None else x for x in f["cor"]]
            assert v["cor"][2 * o:2 * (o + n)].tolist() == [y for x in cor for y in (x, -1 if x < 0 else 1 - x)], (d.name, who, at)
            assert float(v["stat"][b]).hex() == float(f["stat"]).hex() and int(v["stat_int"][b]) == (f["kind"] == "int1"), (d.name, who, at, float(v["stat"][b]), f["stat"])
            assert int(v["maxmaf"][b]) == f["maxmaf"], (d.name, who, at, int(v["maxmaf"][b]), f["maxmaf"])
            o += n; at += 1
    assert at == len(facts), (d.name, who)


def check_design(ctx, d, reps=1, options=None, slots=None, vcf_modes=True):
    """K_tally once, then per option set `reps` device passes over ONE variant set, the host row stage, the oracle, the restatement -> the device's files per option set"""
    from phaser_amd import vcf, vcfout
    saved = tally_of(ctx, d)
    outs = {}
    for oi in (range(len(d.options)) if options is None else options):
        opts = d.options[oi]
        vs = vcf.load_variants(d.vcf_text, **d.load_kwargs(oi))          # (maf belongs to the variant set: one per option set)
        assert [len(vs.chroms[c]) for c in d.chrom_list] == [len(d.vars[c]) for c in d.chrom_list] and list(vs.chroms) == d.chrom_list
        files, noise, log, phased = oracle_run(d.name, oi)
        r = restated(d.name, oi)
        first = None
        for rep in range(reps):
            with Spy(ctx.lib, len(d.chrom_list)) as spy:
                out, eng = engine_pass(ctx, d, vs, saved, True, opts)
            if first is None:
                first = out
            for name in OUTPUTS:
                assert out[name] == first[name], (d.name, opts, "pass %d" % rep, name, first_difference(out[name], first[name]))
            # ---- the stage's own results against the restatement
            check_pair_table(ctx, d, r, spy, slots if rep == 0 else None)
            R = spy.result
            facts = rr.block_facts(d, oi, r, out["haplotypes"])
            assert R["n_linked"] == len(r.pairs) and R["dropped"] == sum(p.dropped for p in r.pairs), (d.name, opts, R)
            assert R["n_components"] == len(r.components) and R["n_blocks"] == len(facts) and R["phased"] == R["n_blk_vars"] == sum(len(f["members"]) for f in facts) == phased, (d.name, opts, R)
            assert R["chrom_blocks"] == [sum(f["chrom"] == c for f in facts) for c in d.chrom_list], (d.name, opts, R)
            assert R["chrom_first_bam"] == [r.first_bam.get(c, -1) for c in d.chrom_list], (d.name, opts, R)
            check_blocks(d, eng, facts, "device")
        host, heng = engine_pass(ctx, d, vs, saved, False, opts)
        for name in OUTPUTS:
            assert first[name] == host[name], (d.name, opts, name, "device / host", first_difference(first[name], host[name]))
            assert canonical(name, first[name]) == canonical(name, files[name]), (d.name, opts, name, "device / oracle",
                                                                                 first_difference(canonical(name, first[name]), canonical(name, files[name])))
        assert eng.log == heng.log and eng.phased == heng.phased == phased, (d.name, opts)
        assert log[-1] in eng.log and log[-2] in eng.log and eng.noise == noise, (d.name, opts, eng.log, log[-2:])          # (noise level, dropped connections)
        check_conn_order(d, r, first["variant_connections"], "device")
        assert block_rows(first["haplotypes"]) == block_rows(files["haplotypes"]), (d.name, opts, "block rows of haplotypes.txt in block order")
        for f, row in zip(facts, block_rows(first["haplotypes"])):
            assert rr.hap_row_fields(f) == row.split("\t")[10:16], (d.name, opts, row)
        check_blocks(d, heng, facts, "host")
        if vcf_modes:
            # the phased VCF from the device's arrays and from the host's, with --gw_phase_vcf_min_confidence on either side of the designed gwStat 2/3
            for mode, conf in ((1, 0.6), (1, 0.7), (2, 0.6), (2, 0.7)):
                a = vcfout.phased_vcf_text(d.vcf_text, 9, eng, gw_phase_vcf=mode, min_confidence=conf, threads=2)
                b = vcfout.phased_vcf_text(d.vcf_text, 9, heng, gw_phase_vcf=mode, min_confidence=conf, threads=2)
                assert a == b, (d.name, opts, mode, conf)
        outs[oi] = first
    return outs


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_pair_table_sizes(ctx, n_keys, reps=1):
    """the design through a table of 16 slots, of 64 and of the default size: same bytes"""
    d = DESIGNS["pair_table_%d" % n_keys]
    outs = []
    for env in d.env:
        with environment(env):
            slots = int(env["PHZ_ROWS_PAIR_SLOTS"]) if env else None
            outs.append(check_design(ctx, d, reps=reps, slots=slots, vcf_modes=False)[0])
    for o in outs[1:]:
        for name in OUTPUTS:
            assert o[name] == outs[0][name], (d.name, name)


ORDERING_SWITCHES = [{"PHZ_ROWS_SORT64": "1"}, {"PHZ_ROWS_FAKE_LINE_BITS": "31"}, {"PHZ_ROWS_FAKE_LINE_BITS": "32"}, {"PHZ_ROWS_NO_PRESTAGE": "1"}, {"PHZ_ROWS_NO_PREKEYS": "1"}]


def check_sequence(ctx):
    for d in xi.all_designs():
        check_design(ctx, d, options=(len(d.options) - 1,), vcf_modes=False)


@pytest.mark.parametrize("name", ["verdicts", "ordering", "block_stats"])
def test_emulated_stage_matches_host_rows_oracle_and_restatement(name):
    check_design(EmuContext(emu_library()), DESIGNS[name])


@pytest.mark.parametrize("n_keys", [16, 17])
def test_emulated_pair_table_full_and_grown(n_keys):
    """16 keys in 16 slots: PHZ_OK, every slot taken, probe sequences that wrap; 17: PHZ_E_CAPACITY, one growth to 64 slots, the same bytes"""
    check_pair_table_sizes(EmuContext(emu_library()), n_keys)


@pytest.mark.parametrize("env", ORDERING_SWITCHES, ids=["%s_%s" % (list(e)[0][9:].lower(), list(e.values())[0]) for e in ORDERING_SWITCHES])
def test_emulated_ordering_under_the_key_layout_switches(env):
    ctx = EmuContext(emu_library())
    d = DESIGNS["ordering"]
    plain = check_design(ctx, d, vcf_modes=False)[0]
    with environment(env):
        got = check_design(ctx, d, vcf_modes=False)[0]
    for name in OUTPUTS:
        assert got[name] == plain[name], (env, name)


def test_emulated_block_stats_beyond_the_tables():
    """stat_n = 2: every block with more than two phased members sends its gwStat through big_stat (text formatted by the host inside the run)"""
    check_design(EmuContext(emu_library(stat_n=2)), DESIGNS["block_stats"])


@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["verdicts", "ordering", "block_stats"])
def test_product_stage_matches_host_rows_oracle_and_restatement(gpu_ctx, name):
    check_design(gpu_ctx, DESIGNS[name], reps=2)


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys", [16, 17])
def test_product_pair_table_full_and_grown(gpu_ctx, n_keys):
    check_pair_table_sizes(gpu_ctx, n_keys, reps=2)


@pytest.mark.gpu
def test_product_stage_leaves_the_context_clean_over_all_designs(gpu_ctx):
    check_sequence(gpu_ctx)
