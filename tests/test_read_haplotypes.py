"""--output_read_haplotypes without a GPU: the numpy restatement readhap.rows_from_lists on hand-made read lists with known answers, the kernels of
phz_read_haplotypes under the host-side HIP emulation against that restatement (fixture tallies, blocks from the emulated row stage), the file against what the
reference wrote for the same sample (tests/golden/pipe_opts: the read-id lists of --output_read_ids 1, the counts of the other cases), every refusal of the entry.
The real kernels: tests/test_gpu_read_haplotypes.py."""
import ctypes as C
import gzip
import json
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import GOLD, REPO, gz_text
from helpers import EmuContext, emu_library, option_case_kwargs, stub_emu_stages, stub_gpu_stages
from test_emu_tally import run_tally


# ------------------------------------------------------------------------------------------------ helpers (shared with tests/test_gpu_read_haplotypes.py)
def lists_from(entries, nv, nb):
    """{(variant, allele, bam): [qid, ...]} -> (rl_start, rl_qid, rl_list) in the layout phz_tally leaves"""
    n_lists = nv * 2 * nb
    per = [[] for _ in range(n_lists)]
    for (v, k, b), q in entries.items():
        per[(2 * v + k) * nb + b] = list(q)
    rl_start = np.zeros(n_lists + 1, dtype=np.uint32)
    np.cumsum([len(x) for x in per], out=rl_start[1:])
    rl_qid = np.array([q for x in per for q in x], dtype=np.int32)
    rl_list = np.repeat(np.arange(n_lists, dtype=np.uint32), np.diff(rl_start.astype(np.int64))).astype(np.uint32)
    return rl_start, rl_qid, rl_list


def table_of(blocks):
    """[[(variant, allele on A), ...], ...] -> (blk_off, blk_var, blk_hap)"""
    off = np.zeros(len(blocks) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in blocks], out=off[1:])
    return off, np.array([v for b in blocks for v, _ in b], dtype=np.int32), np.array([h for b in blocks for _, h in b], dtype=np.uint8)


def tuples(rec):
    return [tuple(int(x) for x in r) for r in rec.tolist()]


def adopt_lists(ctx, nv, nb, rl_start, rl_qid, rl_list, space=None):
    """the read lists alone as the resident tally of a context (phz_tally_import); None leaves an array out"""
    from phaser_amd import _lib
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    sz = _lib.phz_tally_sizes(0, 0, 0, int(rl_start[-1]) if rl_start is not None else len(rl_list), 0, 0, 0, 0)
    out = _lib.phz_tally_out(None, None, None, None, None, None, None, None, None, None, vp(rl_start), vp(rl_qid), None)
    ctx.check(ctx.lib.phz_tally_import(ctx.h, nv, nb, C.byref(sz), C.byref(out), vp(rl_list), _lib.PHZ_HOST if space is None else space))


def read_haplotypes(ctx, blk_off, blk_var, blk_hap, var_skip=None, bam_skip=None, space=None):
    """phz_read_haplotypes the way a caller uses it: count with rows_cap = 0, one row short (refused, nothing written), then the exact count with a canary behind
    the last row.  (Under the emulation device memory is host memory: the PHZ_DEVICE form gets the same numpy arrays.)"""
    from phaser_amd import _lib
    from phaser_amd.readhap import READHAP_DTYPE
    space = _lib.PHZ_HOST if space is None else space
    arrs = [np.ascontiguousarray(blk_off, np.int64), np.ascontiguousarray(blk_var, np.int32), np.ascontiguousarray(blk_hap, np.uint8),
            None if var_skip is None else np.ascontiguousarray(var_skip, np.uint8), None if bam_skip is None else np.ascontiguousarray(bam_skip, np.uint8)]
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None
    args = (len(arrs[0]) - 1,) + tuple(vp(a) for a in arrs)
    n = C.c_int64(-1)
    st = ctx.lib.phz_read_haplotypes(ctx.h, *args, None, 0, C.byref(n), space)
    if st == 0:
        assert n.value == 0
        return np.zeros(0, dtype=READHAP_DTYPE)
    assert st == _lib.PHZ_E_CAPACITY and n.value > 0, (st, ctx.lib.phz_last_error(ctx.h))
    assert b"rows_cap" in ctx.lib.phz_last_error(ctx.h)
    need = int(n.value)
    if need > 1:
        short = np.full((need - 1) * 20, 0x55, dtype=np.uint8)
        n2 = C.c_int64(-1)
        assert ctx.lib.phz_read_haplotypes(ctx.h, *args, C.c_void_p(short.ctypes.data), need - 1, C.byref(n2), space) == _lib.PHZ_E_CAPACITY and n2.value == need
        assert np.all(short == 0x55)
    rows = np.full((need + 1) * 20, 0xA5, dtype=np.uint8)
    n3 = C.c_int64(-1)
    ctx.check(ctx.lib.phz_read_haplotypes(ctx.h, *args, C.c_void_p(rows.ctypes.data), need, C.byref(n3), space))
    assert n3.value == need and np.all(rows[need * 20:] == 0xA5)          # nothing behind the last row
    return rows[:need * 20].view(READHAP_DTYPE).copy()


def _same(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ the numpy restatement on hand-made lists
def test_rows_from_lists_on_hand_made_lists():
    from phaser_amd.readhap import rows_from_lists
    nv, nb = 6, 2
    entries = {(0, 0, 0): [5, 7, 7],          # template 7: both mates on allele 0 of variant 0 -> counted twice
               (0, 1, 0): [9],
               (1, 0, 0): [5],                # variant 1: haplotype A carries allele 1, so allele 0 is side B -- template 5 sits on both sides: a tie
               (1, 1, 0): [7, 9],             # template 9: one line on each side as well
               (1, 1, 1): [5],                # the same template id in the other BAM is another row
               (2, 0, 0): [1, 2], (2, 1, 1): [2],      # block 1 = {2, 3}
               (3, 0, 0): [1], (3, 1, 0): [3],
               (4, 1, 0): [8],                # block 2 = {4}: a one-variant block
               (5, 0, 0): [6]}                # variant 5: in no block
    rs, rq, _ = lists_from(entries, nv, nb)
    off, var, hap = table_of([[(0, 0), (1, 1)], [(3, 0), (2, 0)], [(4, 1)]])
    got = rows_from_lists(rs, rq, nb, off, var, hap)
    assert tuples(got) == [(0, 0, 5, 1, 1), (0, 0, 7, 3, 0), (0, 0, 9, 1, 1), (0, 1, 5, 1, 0),
                           (1, 0, 1, 2, 0), (1, 0, 2, 1, 0), (1, 0, 3, 0, 1), (1, 1, 2, 0, 1),
                           (2, 0, 8, 1, 0)]
    # a skipped variant leaves the vote, the block keeps its ordinal
    skip = np.zeros(nv, np.uint8); skip[1] = 1
    got = rows_from_lists(rs, rq, nb, off, var, hap, var_skip=skip)
    assert tuples(got)[:3] == [(0, 0, 5, 1, 0), (0, 0, 7, 2, 0), (0, 0, 9, 0, 1)] and (0, 1, 5, 1, 0) not in tuples(got) and len(got) == 8
    # a skipped BAM
    got = rows_from_lists(rs, rq, nb, off, var, hap, bam_skip=np.array([1, 0], np.uint8))
    assert tuples(got) == [(0, 1, 5, 1, 0), (1, 1, 2, 0, 1)]
    # a block whose variants are all skipped gives no row
    skip = np.zeros(nv, np.uint8); skip[[2, 3]] = 1
    got = rows_from_lists(rs, rq, nb, off, var, hap, var_skip=skip)
    assert not np.any(got["block"] == 1) and len(got) == 5
    # no block, no row; lists without entries
    assert len(rows_from_lists(rs, rq, nb, np.zeros(1, np.int64), var[:0], hap[:0])) == 0
    rs0, rq0, _ = lists_from({}, nv, nb)
    assert len(rows_from_lists(rs0, rq0, nb, off, var, hap)) == 0


def test_the_same_local_qid_in_blocks_of_two_chromosomes_gives_two_rows():
    """QNAME ids are chromosome-local: template 4 of the first chromosome (variants 0-1) and template 4 of the second (variants 2-3) are different reads"""
    from phaser_amd.readhap import rows_from_lists
    rs, rq, _ = lists_from({(0, 0, 0): [4], (1, 0, 0): [4], (2, 1, 0): [4], (3, 0, 0): [4]}, 4, 1)
    off, var, hap = table_of([[(0, 0), (1, 0)], [(2, 0), (3, 0)]])
    assert tuples(rows_from_lists(rs, rq, 1, off, var, hap)) == [(0, 0, 4, 2, 0), (1, 0, 4, 1, 1)]


# ------------------------------------------------------------------------------------------------ Engines on fixtures
def _engine(case, vcf_text, bam_files, load, cfg, device_rows, **extra):
    from phaser_amd import vcf
    from phaser_amd.engine import Config, Engine
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    from phasing_oracle import bam_display_names          # naming helper only
    load = dict(load); cfg = dict(cfg)
    inc = load.pop("include_indels", 0); cfg.pop("include_indels", None)
    vs = vcf.load_variants(vcf_text, include_indels=inc, **load)
    saved = pickle.load(gzip.open(os.path.join(GOLD, "tally", case + ".pkl.gz"), "rb"))

    class _M:
        ctx = EmuContext(emu_library()) if device_rows else type("ctx", (), {"lib": None})
        device = None
    eng = Engine(vs, bam_display_names(bam_files), Config(include_indels=inc, device_rows=device_rows, **cfg, **extra), mapper=_M())
    eng.n_qid.update(saved["n_qid"]); eng.qnames.update(saved["qnames"])
    (stub_emu_stages if device_rows else stub_gpu_stages)(eng, saved)
    eng.finish()
    assert eng.rows_path == ("device" if device_rows else "host")
    return eng, saved


def opts_engine(name, device_rows, **extra):
    d0 = os.path.join(GOLD, "pipe_opts")
    meta = json.load(open(os.path.join(d0, "cases.json")))
    load, cfg, baseq, isize = option_case_kwargs(name, meta["cases"][name], meta["blacklist"])
    return _engine("opts_" + name, open(os.path.join(d0, "in.vcf")).read(), ["o1.bam", "o2.bam"], load, cfg, device_rows, **extra)[0]


def restated(eng, table):
    """rows_from_lists on the Engine's own read lists (host arrays of its tally)"""
    from phaser_amd.readhap import rows_from_lists
    return rows_from_lists(eng.G["rl_start"], eng.G["rl_qid"], len(eng.bam_names), table["blk_off"], table["blk_var"], table["blk_hap"], table["var_skip"], table["bam_skip"])


# ------------------------------------------------------------------------------------------------ the kernels under emulation on fixture tallies
@pytest.mark.parametrize("case,bams,cfg", [("pipe_two", ["t1.bam", "t2.bam"], {}), ("pipe_noisy_b", ["n.bam"], None)], ids=["pipe_two", "pipe_noisy_b"])
def test_kernels_equal_the_restatement_on_fixture_tallies(case, bams, cfg):
    """K_tally under emulation on the fixture's call lines leaves the read lists (rl_list included) resident; the block table comes from the emulated row stage of
    an Engine on the same fixture.  Records byte for byte, host and device arguments, with and without the skip arrays."""
    from phaser_amd import _lib
    from phaser_amd.readhap import block_table, rows_from_lists
    d = os.path.join(GOLD, case)
    if cfg is None:
        cfg = {"max_block_size": json.load(open(os.path.join(d, "meta.json")))["max_block_size"]}
    eng, saved = _engine(case, open(os.path.join(d, "in.vcf")).read(), bams, {}, cfg, True)
    table = block_table(eng)
    nb = len(bams)
    ctx = EmuContext(emu_library())
    T, sz = run_tally(ctx, saved, eng.chrom_list, nb)
    NV = eng.G["nv"]
    assert len(T["rl_start"]) == NV * 2 * nb + 1 and table["n_phased"] > 3 and len(table["blk_off"]) - 1 > table["n_phased"]          # blocks and singletons
    rng = np.random.default_rng(4)
    some = (rng.random(NV) < 0.2).astype(np.uint8)
    total = 0
    for var_skip, bam_skip in ((None, None), (some, None), (None, np.eye(1, nb, nb - 1, dtype=np.uint8)[0]), (some, np.eye(1, nb, 0, dtype=np.uint8)[0])):
        want = rows_from_lists(T["rl_start"], T["rl_qid"], nb, table["blk_off"], table["blk_var"], table["blk_hap"], var_skip, bam_skip)
        for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
            got = read_haplotypes(ctx, table["blk_off"], table["blk_var"], table["blk_hap"], var_skip, bam_skip, space)
            assert _same(got, want), (case, space, len(got), len(want))
        total += len(want)
    assert total > 1000
    # the phased blocks alone, and the Engine's own adopted tally through Engine.read_haplotypes
    k = table["n_phased"]; o = table["blk_off"][:k + 1]
    want = rows_from_lists(T["rl_start"], T["rl_qid"], nb, o, table["blk_var"][:o[-1]], table["blk_hap"][:o[-1]])
    assert _same(read_haplotypes(ctx, o, table["blk_var"][:o[-1]], table["blk_hap"][:o[-1]]), want) and np.any((want["a"] > 0) & (want["b"] > 0))
    rh = eng.read_haplotypes()
    assert _same(rh["records"], restated(eng, table)) and rh["text"].count(b"\n") == len(rh["records"]) + 1
    if nb > 1:
        assert eng.G["var_base"][eng.chrom_list[1]] > 0 and len(set(rh["records"]["bam"].tolist())) == 2


# ------------------------------------------------------------------------------------------------ pinned by the reference
def golden_rows(name):
    rows = [l.split("\t") for l in gz_text(os.path.join(GOLD, "pipe_opts", name, "out.haplotypic_counts.txt.gz")).split("\n")[1:] if l]
    return rows


def our_groups(text):
    """the file -> {(contig, start, stop, bam): (set of reads with aCount > 0, set of reads with bCount > 0)}"""
    lines = text.decode().split("\n")
    assert lines[0] == "contig\tstart\tstop\tbam\tread\taCount\tbCount\thaplotype" and lines[-1] == ""
    out = {}
    for l in lines[1:-1]:
        contig, start, stop, bam, read, a, b, h = l.split("\t")
        assert int(a) + int(b) > 0 and h == ("A" if int(a) > int(b) else "B" if int(b) > int(a) else "-")
        g = out.setdefault((contig, start, stop, bam), (set(), set()))
        assert read not in g[0] and read not in g[1]                         # one row per (block, bam, read)
        if int(a) > 0:
            g[0].add(read)
        if int(b) > 0:
            g[1].add(read)
    return out


def check_against_golden(name, text):
    rows = golden_rows(name)
    ours = our_groups(text)
    keys = set()
    with_ids = len(rows[0]) == 20
    bam_col = 17 if with_ids else 15
    both = ids_a = ids_b = 0
    for f in rows:
        key = (f[0], f[1], f[2], f[bam_col])
        assert key not in keys                                               # every golden row is a group of its own
        keys.add(key)
        assert key in ours, key
        a, b = ours[key]
        if with_ids:
            want_a = set(x for x in f[14].split(",") if x); want_b = set(x for x in f[15].split(",") if x)
            assert a == want_a and b == want_b, key
            if int(f[4]) > 1:
                ids_a += len(want_a); ids_b += len(want_b); both += len(want_a & want_b)
        assert len(a) == int(f[9]) and len(b) == int(f[10]), key
    assert set(ours) == keys                                                 # no group the golden lacks
    return rows, ours, (ids_a, ids_b, both)


@pytest.mark.parametrize("device_rows", [True, False], ids=["device_rows", "host_rows"])
@pytest.mark.parametrize("name", ["read_ids", "bam_exclude", "blacklist"])
def test_file_matches_what_the_reference_wrote(name, device_rows):
    """device_rows: blocks from phz_rowsdev_fetch_blocks and records from phz_read_haplotypes, both under emulation on the adopted fixture tally; host_rows: blocks
    from the host twin, records from the restatement through the _launch hook."""
    eng = opts_engine(name, device_rows)
    rh = eng.read_haplotypes() if device_rows else eng.read_haplotypes(_launch=lambda table: restated(eng, table))
    assert _same(rh["records"], restated(eng, rh["blocks"]))
    rows, ours, (ids_a, ids_b, both) = check_against_golden(name, rh["text"])
    if name == "read_ids":
        assert len(rows) == 174 and sum(int(f[4]) > 1 for f in rows) == 47 and len(set(f[0] for f in rows)) == 2 and len(set(f[17] for f in rows)) == 2
        assert (ids_a, ids_b, both) == (646, 608, 8)
    if name == "bam_exclude":
        excluded = [eng.bam_names[b] for b in eng.cfg.haplo_count_bam_exclude]
        assert excluded and not any(k[3] in excluded for k in ours) and rh["blocks"]["bam_skip"].sum() == len(excluded)
    if name == "blacklist":
        assert rh["blocks"]["var_skip"].sum() > 0 and any(int(f[6]) > 0 for f in rows)


def test_read_haplotypes_needs_the_block_arrays():
    from phaser_amd import _lib
    eng = opts_engine("read_ids", False, want_vcf=False)
    with pytest.raises(_lib.PhzError, match="want_vcf") as e:
        eng.read_haplotypes(_launch=lambda table: None)
    assert e.value.status == _lib.PHZ_E_ARG


def test_text_needs_the_qname_table():
    from phaser_amd import _lib
    eng = opts_engine("read_ids", False)
    first = eng.chrom_list[0]
    del eng.qnames[first]
    with pytest.raises(_lib.PhzError, match="QNAME table") as e:
        eng.read_haplotypes(_launch=lambda table: restated(eng, table))
    assert e.value.status == _lib.PHZ_E_ARG


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_ctx_usable():
    from phaser_amd import _lib
    from phaser_amd.readhap import rows_from_lists
    lib = emu_library()
    ctx = EmuContext(lib)
    nv, nb = 40, 2
    rng = np.random.default_rng(8)
    entries = {(v, k, b): rng.integers(0, 30, size=int(rng.integers(0, 6))).tolist() for v in range(nv) for k in range(2) for b in range(nb)}
    rs, rq, rl = lists_from(entries, nv, nb)
    good = table_of([[(v, int(v % 3 == 0)) for v in range(s, s + 4)] for s in range(0, 32, 4)] + [[(36, 1)]])
    n = C.c_int64(-1)
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None

    def refused(table, space, needle, status=_lib.PHZ_E_ARG):
        off, var, hap = (np.ascontiguousarray(x, dt) for x, dt in zip(table, (np.int64, np.int32, np.uint8)))
        n.value = -1
        st = lib.phz_read_haplotypes(ctx.h, len(off) - 1, vp(off), vp(var), vp(hap), None, None, None, 0, C.byref(n), space)
        assert st == status, (st, lib.phz_last_error(ctx.h))
        assert needle in lib.phz_last_error(ctx.h), lib.phz_last_error(ctx.h)
        assert n.value == 0

    def works():
        want = rows_from_lists(rs, rq, nb, *good)
        assert len(want) > 50 and _same(read_haplotypes(ctx, *good), want)

    # ---- no resident tally
    refused(good, _lib.PHZ_HOST, b"no resident tally")
    # ---- a tally adopted without one of its read-list arrays
    for missing in range(3):
        parts = [rs, rq, rl]; parts[missing] = None
        adopt_lists(ctx, nv, nb, *parts)
        refused(good, _lib.PHZ_HOST, b"read lists")
    adopt_lists(ctx, nv, nb, rs, rq, rl)
    works()
    off, var, hap = good
    for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
        # ---- a variant outside [0, nv)
        for bad in (nv, -1, nv + 1000):
            v2 = var.copy(); v2[5] = bad
            refused((off, v2, hap), space, b"outside [0, nv)")
            works()
        # ---- a variant in two blocks, twice in one block
        v2 = var.copy(); v2[9] = var[2]
        refused((off, v2, hap), space, b"in two blocks")
        v2 = var.copy(); v2[1] = var[0]
        refused((off, v2, hap), space, b"in two blocks")
        works()
        # ---- blk_off not ascending
        for o2 in ([0, 4, 3, 12, 16, 20, 24, 28, 32, 33], [-1, 4, 8, 12, 16, 20, 24, 28, 32, 33], [0, 4, 8, 12, 16, 20, 24, 28, 33, 32]):
            refused((np.array(o2, np.int64), var, hap), space, b"blk_off")
            works()
        # ---- blk_hap above 1
        h2 = hap.copy(); h2[7] = 2
        refused((off, var, h2), space, b"blk_hap")
        works()
    # ---- n_blocks == 0: no row, no error; a table of empty blocks
    n.value = -1
    assert lib.phz_read_haplotypes(ctx.h, 0, None, None, None, None, None, None, 0, C.byref(n), _lib.PHZ_HOST) == 0 and n.value == 0
    assert len(read_haplotypes(ctx, np.zeros(4, np.int64), var[:0], hap[:0])) == 0
    # ---- empty blocks between filled ones keep the ordinals of the others
    off3 = np.array([0, 0, 4, 4, 4, 8], np.int64)
    want = rows_from_lists(rs, rq, nb, off3, var[:8], hap[:8])
    assert set(want["block"].tolist()) == {1, 4}
    for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
        assert _same(read_haplotypes(ctx, off3, var[:8], hap[:8], space=space), want)
    # ---- fields that do not fit a 64-bit key: 2^30 blocks need 31 bits beside 33 of (qid, side) and 1 of the BAM.  Decided from n_blocks alone, before a
    #      PHZ_DEVICE table is looked at (no table of that size is built here)
    n.value = -1
    st = lib.phz_read_haplotypes(ctx.h, 1 << 30, vp(off), vp(var), vp(hap), None, None, None, 0, C.byref(n), _lib.PHZ_DEVICE)
    assert st == _lib.PHZ_E_UNSUPPORTED and b"64-bit key" in lib.phz_last_error(ctx.h) and n.value == 0
    works()
    # ---- more read-list entries than the device sort takes: decided from the resident tally's size (adopted in PHZ_DEVICE space: the arrays are not read)
    sz = _lib.phz_tally_sizes(0, 0, 0, 1 << 30, 0, 0, 0, 0)
    out = _lib.phz_tally_out(None, None, None, None, None, None, None, None, None, None, vp(rs), vp(rq), None)
    ctx.check(lib.phz_tally_import(ctx.h, nv, nb, C.byref(sz), C.byref(out), vp(rl), _lib.PHZ_DEVICE))
    refused(good, _lib.PHZ_HOST, b"2^30", status=_lib.PHZ_E_UNSUPPORTED)
    adopt_lists(ctx, nv, nb, rs, rq, rl)
    works()
