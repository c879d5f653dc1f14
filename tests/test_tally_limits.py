"""K_tally (phaser_amd/csrc/phz_tally.hip, entry points phz_tally / phz_tally_fetch) on the designed call lines of tests/tally_inputs.py, under the
host-side emulation and on the product build on an MI355X, against tests/tally_restatement.py: every array phz_tally_fetch returns and every field of
phz_tally_sizes must equal the restatement exactly; there is no tolerance anywhere.

Three tiers.  The restatement (dicts, sets and sorts over the call lines, definitions from oracle/phasing_oracle.py) is pinned first, with no kernel
involved: it must reproduce every array of every fixture under tests/golden/tally, which are tied to the reference through the five output files.  The
test_*_designs_hold_what_they_promise tests, one per family of cases, then check, still without a kernel, that every case is what its name says (sizes,
more than 2^16 distinct pairs, far / dirty / spilled / out-of-bitmap counts that are non-zero where the case is built for them and zero where it is
built to avoid them) and print the table name, lines, nv, QNAMEs, far, dirty, spilled, pairs.  Only then the kernels: emulated at the product tile of
1,024 lines and, where the tile matters, at 256; on the GPU through the product library.  Next to the results, the deltas of the context's work
counters must equal what the mirror of the tiling rules promises (PHZ_C_FAR_LINES, PHZ_C_DIRTY_LISTS, PHZ_C_SPILL_QNAMES, PHZ_C_SPILL_LINES), and
PHZ_C_PAIR_REDOS must move for the redo case on a context whose table has not grown yet and for nothing else.

State that must come back clean (the per-QNAME cursors, the read-list cursors, the dirty bitmap, the pair table after a failed attempt, the enlarged
table the context keeps): every case twice on one context, and all cases in one sequence on one context (tally_inputs.designed_cases: a small case
right after the redo, the far-left and the spill-heavy ones)."""
import functools
import glob
import gzip
import os
import pickle

import numpy as np
import pytest

import tally_inputs as ti
import tally_restatement as tr
from conftest import GOLD
from helpers import EmuContext, emu_library, genome_from_saved
from test_emu_tally import run_tally

FIXTURES = sorted(os.path.basename(f)[:-len(".pkl.gz")] for f in glob.glob(os.path.join(GOLD, "tally", "*.pkl.gz")))
CASES = {c.name: c for c in ti.all_cases()}
TILE_CASES = sorted(n for n, c in CASES.items() if c.tile_matters)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's result of a designed case: computed once, read-only"""
    c = CASES[name]
    return tr.restate(c.saved, c.chrom_list, c.n_bams)


# ------------------------------------------------------------------------------------------------ tier 1: the restatement against the fixtures
def test_every_fixture_is_listed():
    assert len(FIXTURES) >= 18 and "c1" in FIXTURES and "pipe_sparse" in FIXTURES


@pytest.mark.parametrize("case", FIXTURES)
def test_restatement_reproduces_the_gpu_fixture(case):
    """no kernel runs here: what the fixtures hold (written by K_tally on an MI355X, tied to the reference through the five files) from their call lines"""
    saved = pickle.load(gzip.open(os.path.join(GOLD, "tally", case + ".pkl.gz"), "rb"))
    chroms = list(saved["tally"]); nb = tr.n_bams_of(saved, chroms)
    want = genome_from_saved(saved, chroms, nb)
    got = tr.restate(saved, chroms, nb)
    for k in ("var_count", "var_first", "var_distinct", "var_rank", "ea", "eb", "linked", "cto", "stats", "rl_start", "rl_qid"):
        assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), k
    # what genome_from_saved does not expose, from the pickle itself
    assert np.array_equal(got["cells"], np.concatenate([saved["tally"][c]["cells"].reshape(-1, 9) for c in chroms]))
    assert np.array_equal(got["line_cls"], np.concatenate([saved["tally"][c]["line_cls"] for c in chroms]))
    s = got["sizes"]
    assert (s["noise_match"], s["noise_mismatch"]) == want["noise"] and s["n_kept"] == want["n_kept"] and s["n_lines"] == want["n_lines"]
    assert s["n_edges"] == len(want["ea"]) and s["n_read_list"] == len(want["rl_qid"])


# ------------------------------------------------------------------------------------------------ tier 2: the designs, no kernel
def row(c, tile=1024):
    p = c.promise(tile); r = reference(c.name)
    print("%-42s tile %4d lines %6d nv %6d QNAMEs %6d far %5d dirty %4d spilled %5d out-of-bitmap %5d pairs %6d" % (
        c.name, tile, c.n_lines, c.nv, p["qnames"], p["far"], p["dirty"], p["spilled"], p["oob"], r["sizes"]["n_edges"]))
    assert c.n_lines <= 37000                       # no case above the largest input the emulated suite had
    return p, r


def test_moved_designs_hold_what_they_promise():
    """the five inputs test_emu_tally.py had"""
    p, r = row(ti.skewed())
    assert ti.skewed().n_lines == 37000 and p["far"] == 0 and p["dirty"] == 0 and p["oob"] == 0 and p["spilled"] > 1000
    rs = r["rl_start"].astype(np.int64)
    assert np.diff(rs).max() > 4096                 # a read list beyond the LDS sort ... which no far line makes dirty here
    for tile in (1024, 256):
        p, r = row(ti.far_lines(), tile)
        assert p["far"] > 0 and p["dirty"] >= 4 and p["oob"] == 0              # lists (0, ref / alt), (7, ref / alt) and the tile where the window moves on
    assert np.diff(r["rl_start"].astype(np.int64))[:2].sum() > 4096 and ti.far_lines().as16
    for tile in (1024, 256):
        p, r = row(ti.long_groups(), tile)
        assert 20 <= p["spilled"] <= 60          # the 20 spread QNAMEs, and the contiguous groups a tile boundary cuts
    groups = {}
    for v, q, k in zip(*[ti.long_groups().saved["tally"]["chrS"][x].tolist() for x in ("line_var", "line_qid", "line_cls")]):
        if k != 255:
            groups.setdefault(q, set()).add((v, k))
    assert sum(len(g) > 64 for q, g in groups.items() if q < 40) == 40 and sum(len(g) > 64 for q, g in groups.items() if q >= 40) == 20
    p, r = row(ti.scan_over_many_tiles())
    assert 2 * ti.scan_over_many_tiles().nv > 12 * 4096 and p["far"] > 0          # 13 scan tiles of 4,096 read lists
    e, d, l = ti.empty_dropped_live()
    for c in (e, d):
        p, r = row(c)
        assert (p["far"], p["dirty"], p["spilled"], p["qnames"]) == (0, 0, 0, 0) and r["sizes"]["n_kept"] == 0 and r["sizes"]["n_edges"] == 0
    assert e.n_lines == 0 and d.n_lines == 300
    p, r = row(l)
    assert r["sizes"]["n_kept"] == 300 and p["far"] == 0


def test_bitmap_designs_hold_what_they_promise():
    c = ti.qnames_beyond_the_bitmap()
    p, r = row(c)
    assert c.n_lines == 8192 and c.n_bams == 1 and c.saved["n_qid"]["chrQ"] == 40000
    assert p["oob"] > r["sizes"]["n_kept"] // 2                                   # most lines lie outside their tile's bitmap
    assert p["far"] == 0 and p["dirty"] == 0
    tiles_of = p["tiles_of"]
    for q in c.kinds["two_in_one_tile"]:
        assert list(tiles_of[q].values()) == [[2, 2]]
    for q in c.kinds["one_in_each_of_two_tiles"]:
        assert sorted(tiles_of[q].values()) == [[1, 1], [1, 1]]
    for q in c.kinds["in_and_out"]:
        assert sorted(tiles_of[q].values()) == [[1, 0], [1, 1]]
    designed = sum(c.kinds.values(), [])
    assert len(set(designed)) == 3 * ti.N_KIND and p["spilled"] == 3 * ti.N_KIND and p["spill_lines"] == 6 * ti.N_KIND      # every other QNAME has one line
    assert row(c, 256)[0]["spilled"] >= 2 * ti.N_KIND


def test_group_window_designs_hold_what_they_promise():
    c = ti.spilled_groups_beyond_the_group_window()
    for tile in (1024, 256):
        p, r = row(c, tile)
        assert c.nv == 3000 and p["far"] == 0 and p["dirty"] == 0 and p["oob"] == 0
        assert p["spilled"] == 300 and p["spill_lines"] == 1800                   # two workgroups of k_groups, a few hundred lines each
    R = c.saved["tally"]["chrG"]
    own = {}
    for v, q, k in zip(R["line_var"].tolist(), R["line_qid"].tolist(), R["line_cls"].tolist()):
        if q < 300:
            assert k < 2
            own.setdefault(q, []).append(v)
    for q, vs in own.items():
        # whichever item sets the workgroup's window [v - 256, v + 768), the QNAME has ref/alt lines above and / or below it
        assert len(vs) == 6 and all(any(not (b - 256 <= v < b + 768) for v in vs) for b in range(0, 3000))
        assert min(vs) < 150 and max(vs) >= 2850 and max(vs) - min(vs) > 1024
    assert len(own) == 300


def test_redo_designs_hold_what_they_promise():
    c = ti.pair_table_redo()
    p, r = row(c)
    assert c.redo and c.nv <= 16384 and 4 * c.nv <= ti.PAIR_TABLE_MIN             # the table starts at its minimum of 2^16 slots
    assert r["sizes"]["n_edges"] > ti.PAIR_TABLE_MIN                              # more distinct pairs than slots: overflow whatever the hash does
    assert c.n_lines == 6144 and p["far"] == 0 and p["spilled"] == 0
    assert sum(not x.redo for x in CASES.values()) == len(CASES) - 1
    for x in CASES.values():
        if not x.redo:
            assert reference(x.name)["sizes"]["n_edges"] < ti.PAIR_TABLE_MIN // 4, x.name      # ... and no other case fills a quarter of them


def test_tile_start_designs_hold_what_they_promise():
    for tile in (1024, 256):
        c = ti.tile_starts_far_right()
        p, r = row(c, tile)
        R = c.saved["tally"]["chrT"]
        assert 2048 % tile == 0 and R["line_var"][2048] - np.delete(R["line_var"], 2048).max() > 256 and R["line_cls"][2048] == 0
        assert p["far"] == 1 and p["dirty"] == 1
        assert all(w <= 400 for _, _, w in p["wb"])                               # the suffix minimum kept the third tile's window with its other lines
        c = ti.tile_starts_far_left()
        p, r = row(c, tile)
        R = c.saved["tally"]["chrT"]
        assert 3072 % tile == 0 and R["line_var"][3072] == 5 and np.delete(R["line_var"], 3072).min() - 5 > 256
        assert all(w == 0 for _, _, w in p["wb"][:3072 // tile + 1])              # every earlier tile's window pulled down to variant 0
        assert p["far"] >= int((R["line_cls"][:3072] != 255).sum()) > 2800          # every kept line of the earlier tiles is far
        if tile == 1024:                                                          # (the stray line starts the last tile: every kept line but itself, every list but its own)
            assert p["far"] == r["sizes"]["n_kept"] - 1 and p["dirty"] == int((np.diff(r["rl_start"].astype(np.int64)) > 0).sum()) - 1


def test_seam_and_owner_designs_hold_what_they_promise():
    c = ti.chromosome_seams()
    assert [c.saved["tally"][x]["nv"] for x in c.chrom_list] == [300, 10] and c.n_bams == 3
    assert [(b, n > 0) for b, _, n in c.saved["tally"]["chrA"]["bam_offsets"]] == [(0, True), (1, True), (2, False)]      # a shard with zero lines
    assert [b for b, _, n in c.saved["tally"]["chrB"]["bam_offsets"]] == [0, 2]                                           # BAM 1 has no line on chrB
    assert c.saved["tally"]["chrA"]["line_var"].min() == 295 and sorted(set(c.saved["tally"]["chrB"]["line_var"].tolist())) == list(range(10))
    for tile in (1024, 256):
        p, r = row(c, tile)
        assert p["far"] == 0 and p["spilled"] > 700
        assert all(w + ti.TWT > 300 for x, _, w in p["wb"] if x == "chrA") and all(w < 300 for x, _, w in p["wb"] if x == "chrB")      # windows across the seam
    c = ti.two_bams_owner_rule()
    p, r = row(c)
    assert c.n_lines == 4008 and p["far"] == 0
    link = {(a, b): l for a, b, l in zip(r["ea"].tolist(), r["eb"].tolist(), r["linked"].tolist())}
    assert (link[(24, 25)], link[(26, 27)], link[(28, 29)]) == (0, 0, 1) and link[(0, 24)] == 0 and link[(1, 28)] == 0
    assert list(r["var_rank"][24:28]) == [tr.NONE_RANK] * 4 and r["var_rank"][28] != tr.NONE_RANK and r["var_rank"][29] != tr.NONE_RANK
    R = c.saved["tally"]["chrS"]
    seen = {}
    for q, k, b in zip(R["line_qid"].tolist(), R["line_cls"].tolist(), R["line_bam"].tolist()):
        if k != 255:
            seen.setdefault(q, set()).add((b, k < 2))
    for band, (lo, hi) in c.bands.items():
        qs = [seen[q] for q in range(lo, hi) if q in seen]
        want = {"bam0_only": lambda s: {b for b, _ in s} == {0}, "bam1_only": lambda s: {b for b, _ in s} == {1},
                "both": lambda s: (0, True) in s and (1, True) in s, "bam0_and_other_in_bam1": lambda s: (0, True) in s and (1, False) in s and (1, True) not in s}[band]
        assert all((1, True) not in s for s in qs) if band == "bam0_and_other_in_bam1" else True
        assert sum(want(s) for s in qs) >= 50, band


def test_case_names_are_distinct():
    assert len(CASES) == len({id(c) for c in ti.designed_cases()}) == 14
    for name in ("qnames_beyond_the_bitmap", "spilled_groups_beyond_the_group_window", "pair_table_redo", "tile_starts_far_right", "tile_starts_far_left",
                 "chromosome_seams", "two_bams_owner_rule", "skewed", "far_lines", "long_groups", "scan_over_many_tiles"):
        assert name in CASES
    order = [c.name for c in ti.designed_cases()]
    small = ("two_bams_owner_rule", "all_lines_dropped", "live_after_dropped", "empty_shard", "chromosome_seams")
    for heavy in ("pair_table_redo", "tile_starts_far_left", "spilled_groups_beyond_the_group_window", "qnames_beyond_the_bitmap"):
        assert order[order.index(heavy) + 1] in small


# ------------------------------------------------------------------------------------------------ tier 3: the kernels
def counters_of(ctx):
    from phaser_amd import _lib
    return {k: ctx.counter(getattr(_lib, "PHZ_C_" + k)) for k in ("FAR_LINES", "DIRTY_LISTS", "SPILL_QNAMES", "SPILL_LINES", "PAIR_REDOS")}


def run_case(ctx, c, tile):
    """one phz_tally + fetch of case c on ctx: the whole result against the restatement, the counter deltas against the promise.  Whether the pair table of this
    context has grown already (then the redo case must NOT redo) is kept on the context object"""
    p = c.promise(tile); where = "%s (tile %d)" % (c.name, tile)
    before = counters_of(ctx)
    got, sz = run_tally(ctx, c.saved, c.chrom_list, c.n_bams, as16=c.as16)
    delta = {k: v - before[k] for k, v in counters_of(ctx).items()}
    tr.assert_equal(got, sz, reference(c.name), where)
    assert delta["FAR_LINES"] == p["far"], (where, delta, p["far"])
    assert delta["DIRTY_LISTS"] == p["dirty"], (where, delta, p["dirty"])
    assert delta["SPILL_QNAMES"] == p["spilled"], (where, delta, p["spilled"])
    assert delta["SPILL_LINES"] == p["spill_lines"], (where, delta, p["spill_lines"])
    if c.redo and not getattr(ctx, "pair_table_grown", False):
        assert delta["PAIR_REDOS"] >= 1, where
        ctx.pair_table_grown = True
    else:
        assert delta["PAIR_REDOS"] == 0, where
    return delta


def check_twice(ctx, name, tile):
    for rep in range(2):
        run_case(ctx, CASES[name], tile)


def check_sequence(ctx, tile):
    for c in ti.designed_cases():
        run_case(ctx, c, tile)


def check_redo_on_its_own_context(ctx, tile):
    c = ti.pair_table_redo()
    assert run_case(ctx, c, tile)["PAIR_REDOS"] >= 1          # the first call overflows the 2^16 slots and is redone with a larger table ...
    assert run_case(ctx, c, tile)["PAIR_REDOS"] == 0          # ... which the context keeps
    run_case(ctx, ti.two_bams_owner_rule(), tile)


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_kernels_match_the_restatement(name):
    check_twice(EmuContext(emu_library()), name, 1024)


@pytest.mark.parametrize("name", TILE_CASES)
def test_emulated_kernels_match_the_restatement_at_tile_256(name):
    check_twice(EmuContext(emu_library(256)), name, 256)


def test_emulated_kernels_leave_the_context_clean_over_all_cases():
    check_sequence(EmuContext(emu_library()), 1024)


def test_emulated_pair_table_is_redone_once_and_kept():
    check_redo_on_its_own_context(EmuContext(emu_library()), 1024)


@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_product_kernels_match_the_restatement(gpu_ctx, name):
    check_twice(gpu_ctx, name, 1024)


@pytest.mark.gpu
def test_product_kernels_leave_the_context_clean_over_all_cases(gpu_ctx):
    check_sequence(gpu_ctx, 1024)


@pytest.mark.gpu
def test_product_pair_table_is_redone_once_and_kept():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    try:
        check_redo_on_its_own_context(ctx, 1024)
    finally:
        ctx.close()
