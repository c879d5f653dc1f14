"""--output_read_haplotypes on the GPU: the kernels of phz_read_haplotypes on hand-built read lists against their numpy restatement (readhap.rows_from_lists),
Engine.read_haplotypes against what the reference wrote (tests/golden/pipe_opts) and against the restatement on the fetched tally, and the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, gz_text
from helpers import OUTPUTS, option_case_kwargs
from test_gpu_network import cli_inputs          # noqa: F401  (fixture: pipe_one as an unfiltered BAM + gzipped VCF)
from test_gpu_pipeline import compare, run_product
from test_read_haplotypes import check_against_golden, lists_from, table_of, tuples

pytestmark = pytest.mark.gpu

NV, NB = 600, 2
BIG_QID = 2 ** 31 - 1


@pytest.fixture(scope="module")
def mapper():
    from phaser_amd.mapper import Mapper
    return Mapper(0)


# ------------------------------------------------------------------------------------------------ the kernels on hand-built read lists
@pytest.fixture(scope="module")
def read_lists():
    """600 variants, 2 BAMs, ~40,000 entries adopted as the resident tally of a context of its own (phz_tally_import: rl_start, rl_qid, rl_list): more than nine
    4,096-key sort tiles, more than 150 workgroups of 256.  ~80 blocks of 2-40 variants drawn from a shuffled variant list (non-contiguous, interleaved), ~100
    variants in no block, block 7 wholly skipped by var_skip.  Built in:
      block 0 = variants (300, 17), BAM 0: template 0 with 3,000 entries on haplotype A (the smallest key of all: padding), template 1 with 1,096 entries on A and 50
              on B -- its A run ends at index 4,095 of the sorted keys, its B run starts at 4,096 (tile and workgroup boundary);
      block 5: template 77 with 6,000 entries in ONE list: a single run across a sort tile and 23 workgroups;
      the first list (variant 0, allele 0, BAM 0) and the last one (variant 599, allele 1, BAM 1) are empty;
      the last entry of the array (list of variant 599, allele 1, BAM 0) is the only entry of template 2^31 - 1, the largest id."""
    from phaser_amd import _lib
    rng = np.random.default_rng(2024)
    order = rng.permutation(np.arange(1, NV - 1)).tolist()
    for v in (300, 17):
        order.remove(v)
    blocks = [[(300, 1), (17, 0)]]
    at = 0
    while len(blocks) < 80 and at + 40 <= len(order) - 90:
        size = 12 if len(blocks) == 5 else 40 if len(blocks) in (10, 30) else int(rng.integers(2, 9))
        blocks.append([(v, int(rng.integers(0, 2))) for v in order[at:at + size]]); at += size
    blocks[3].append((NV - 1, 1)); blocks[9].append((0, 0))
    off, var, hap = table_of(blocks)
    in_block = np.zeros(NV, bool); in_block[var] = True
    assert 75 <= len(blocks) <= 80 and 80 <= int((~in_block).sum()) <= 200
    entries = {}
    for v in range(NV):
        for k in range(2):
            for b in range(NB):
                entries[(v, k, b)] = rng.integers(0, 2000, size=int(rng.integers(0, 27))).tolist()
    entries[(300, 1, 0)] = [0] * 1800 + [1] * 600; entries[(300, 0, 0)] = [1] * 20
    entries[(17, 0, 0)] = [1] * 496 + [0] * 1200; entries[(17, 1, 0)] = [1] * 30
    v5 = blocks[5][4][0]
    entries[(v5, 1, 1)] = entries[(v5, 1, 1)][:5] + [77] * 6000 + [1999]
    entries[(0, 0, 0)] = []; entries[(NV - 1, 1, 1)] = []
    entries[(NV - 1, 1, 0)] = [3, 3, BIG_QID]
    rs, rq, rl = lists_from(entries, NV, NB)
    assert 9 * 4096 < len(rq) < 46000 and len(rq) > 150 * 256 and rq[-1] == BIG_QID and rs[1] == 0 and rs[-1] == rs[-2]
    var_skip = np.zeros(NV, np.uint8)
    var_skip[[v for v, _ in blocks[7]]] = 1
    var_skip[rng.choice(NV, size=30, replace=False)] = 1
    var_skip[[300, 17, v5, NV - 1]] = 0
    ctx = _lib.Context(0)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    sz = _lib.phz_tally_sizes(0, 0, 0, len(rq), 0, 0, 0, 0)
    out = _lib.phz_tally_out(None, None, None, None, None, None, None, None, None, None, vp(rs), vp(rq), None)
    ctx.check(ctx.lib.phz_tally_import(ctx.h, NV, NB, C.byref(sz), C.byref(out), vp(rl), _lib.PHZ_HOST))
    return ctx, rs, rq, (off, var, hap), var_skip, v5


def gpu_rows(ctx, off, var, hap, var_skip, bam_skip, device):
    """count with rows_cap = 0, then a fill with exactly that capacity and the 0xA5 canary behind the last record"""
    from phaser_amd import _lib
    from phaser_amd.readhap import READHAP_DTYPE
    host = [np.ascontiguousarray(off, np.int64), np.ascontiguousarray(var, np.int32), np.ascontiguousarray(hap, np.uint8),
            None if var_skip is None else np.ascontiguousarray(var_skip, np.uint8), None if bam_skip is None else np.ascontiguousarray(bam_skip, np.uint8)]
    n = C.c_int64(-1)
    if not device:
        args = (len(host[0]) - 1,) + tuple(C.c_void_p(a.ctypes.data) if a is not None and a.size else None for a in host)
        st = ctx.check(ctx.lib.phz_read_haplotypes(ctx.h, *args, None, 0, C.byref(n), _lib.PHZ_HOST), allow=(_lib.PHZ_E_CAPACITY,))
        rows = np.full((int(n.value) + 1) * 20, 0xA5, dtype=np.uint8)
        if st:
            ctx.check(ctx.lib.phz_read_haplotypes(ctx.h, *args, C.c_void_p(rows.ctypes.data), int(n.value), C.byref(n), _lib.PHZ_HOST))
    else:
        dev = [None if a is None else torch.from_numpy(a).cuda() for a in host]
        torch.cuda.synchronize()
        args = (len(host[0]) - 1,) + tuple(C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None for t in dev)
        st = ctx.check(ctx.lib.phz_read_haplotypes(ctx.h, *args, None, 0, C.byref(n), _lib.PHZ_DEVICE), allow=(_lib.PHZ_E_CAPACITY,))
        dr = torch.full(((int(n.value) + 1) * 20,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if st:
            ctx.check(ctx.lib.phz_read_haplotypes(ctx.h, *args, C.c_void_p(dr.data_ptr()), int(n.value), C.byref(n), _lib.PHZ_DEVICE))
        rows = dr.cpu().numpy()
    assert np.all(rows[int(n.value) * 20:] == 0xA5)                  # nothing behind the last record
    return rows[:int(n.value) * 20].view(READHAP_DTYPE).copy()


@pytest.mark.parametrize("device", [False, True], ids=["host_args", "device_args"])
@pytest.mark.parametrize("skip_bam0", [False, True], ids=["all_bams", "bam0_skipped"])
def test_kernels_on_hand_built_read_lists(read_lists, skip_bam0, device):
    from phaser_amd.readhap import rows_from_lists
    ctx, rs, rq, (off, var, hap), var_skip, v5 = read_lists
    bam_skip = np.array([1, 0], np.uint8) if skip_bam0 else None
    want = rows_from_lists(rs, rq, NB, off, var, hap, var_skip, bam_skip)
    got = gpu_rows(ctx, off, var, hap, var_skip, bam_skip, device)
    assert got.tobytes() == want.tobytes(), (len(got), len(want))
    assert len(want) > 5000 and not np.any(want["block"] == 7)
    big = want[(want["block"] == 5) & (want["bam"] == 1) & (want["qid"] == 77)]
    assert len(big) == 1 and int(big["a"][0] + big["b"][0]) >= 6000 and min(int(big["a"][0]), int(big["b"][0])) < 100          # one run of >= 6,000 entries
    if not skip_bam0:
        assert tuples(want[:2]) == [(0, 0, 0, 3000, 0), (0, 0, 1, 1096, 50)]          # sorted keys [3000, 4096) = its A run, [4096, 4146) = its B run
        last = want[(want["block"] == 3) & (want["bam"] == 0) & (want["qid"] == BIG_QID)]
        assert tuples(last) == [(3, 0, BIG_QID, 1, 0)]
        assert int(want["qid"].max()) == BIG_QID
    else:
        assert not np.any(want["bam"] == 0)


@pytest.mark.parametrize("device", [False, True], ids=["host_args", "device_args"])
def test_small_tables(read_lists, device):
    from phaser_amd.readhap import rows_from_lists
    ctx, rs, rq, (off, var, hap), var_skip, v5 = read_lists
    # without the skip arrays; one block of one variant; the phased blocks in another order; n_blocks = 0
    for o, v, h in ((off, var, hap), table_of([[(v5, 1)]]), table_of([[(NV - 1, 0)], [(300, 0), (17, 1)], [(5, 0)]])):
        want = rows_from_lists(rs, rq, NB, o, v, h)
        assert len(want) > 0 and gpu_rows(ctx, o, v, h, None, None, device).tobytes() == want.tobytes()
    assert len(gpu_rows(ctx, np.zeros(1, np.int64), var[:0], hap[:0], None, None, device)) == 0
    n = C.c_int64(-1)
    assert ctx.lib.phz_read_haplotypes(ctx.h, 0, None, None, None, None, None, None, 0, C.byref(n), 0) == 0 and n.value == 0


# ------------------------------------------------------------------------------------------------ through the Engine
def opts_engine(mapper, name, **extra):
    d0 = os.path.join(GOLD, "pipe_opts")
    meta = json.load(open(os.path.join(d0, "cases.json")))
    load, cfg, baseq, isize = option_case_kwargs(name, meta["cases"][name], meta["blacklist"])
    bams = {b + ".bam": {c: gz_text(os.path.join(d0, "%s.%s.sam.gz" % (b, c))) for c in ("chr21", "chr22")} for b in ("o1", "o2")}
    out, eng = run_product(mapper, open(os.path.join(d0, "in.vcf")).read(), bams, "cuda", load_kw=load, isize=isize, **cfg, **extra)
    return eng


@pytest.mark.parametrize("device_rows", [True, False], ids=["device_rows", "host_rows"])
@pytest.mark.parametrize("name", ["read_ids", "bam_exclude", "blacklist"])
def test_engine_file_matches_what_the_reference_wrote(mapper, name, device_rows):
    eng = opts_engine(mapper, name, device_rows=device_rows, want_vcf=True)
    assert eng.rows_path == ("device" if device_rows else "host")
    rh = eng.read_haplotypes()
    rows, ours, (ids_a, ids_b, both) = check_against_golden(name, rh["text"])
    if name == "read_ids":
        assert len(rows) == 174 and (ids_a, ids_b, both) == (646, 608, 8)
    if name == "bam_exclude":
        assert not any(k[3] == eng.bam_names[eng.cfg.haplo_count_bam_exclude[0]] for k in ours)


def two_bam_engine(mapper, **cfg):
    d = os.path.join(GOLD, "pipe_two")
    bams = {b + ".bam": {c: gz_text(os.path.join(d, "%s.%s.sam.gz" % (b, c))) for c in ("chr21", "chr22")} for b in ("t1", "t2")}
    return run_product(mapper, open(os.path.join(d, "in.vcf")).read(), bams, "cuda", want_vcf=True, **cfg)[1]


def test_engine_records_equal_the_restatement_on_the_fetched_tally(mapper):
    """two chromosomes (a non-zero base in the joint variant space), two BAMs that share QNAMEs"""
    from phaser_amd.readhap import rows_from_lists
    eng = two_bam_engine(mapper)
    rh = eng.read_haplotypes()
    t = rh["blocks"]
    eng._fetch_tally()
    want = rows_from_lists(eng.G["rl_start"], eng.G["rl_qid"], 2, t["blk_off"], t["blk_var"], t["blk_hap"], t["var_skip"], t["bam_skip"])
    assert rh["records"].tobytes() == want.tobytes() and len(want) > 1000
    assert eng.G["var_base"][eng.chrom_list[1]] > 0 and set(want["bam"].tolist()) == {0, 1}
    both_bams = set(want["qid"][(want["bam"] == 0) & (t["chrom"][want["block"]] == 0)].tolist()) & set(want["qid"][(want["bam"] == 1) & (t["chrom"][want["block"]] == 0)].tolist())
    assert both_bams                                                             # a template id seen in both BAMs
    assert rh["text"].count(b"\n") == len(want) + 1


def test_read_haplotypes_refuses_a_replaced_tally(mapper):
    from phaser_amd import _lib
    first = two_bam_engine(mapper)
    second = opts_engine(mapper, "read_ids", want_vcf=True)
    with pytest.raises(_lib.PhzError, match="resident tally"):
        first.read_haplotypes()
    check_against_golden("read_ids", second.read_haplotypes()["text"])


# ------------------------------------------------------------------------------------------------ the command line
def run_cli(cli_inputs, tag, *extra):          # noqa: F811
    from phaser_amd import phaser
    tmp, bam, vcfgz = cli_inputs
    prefix = str(tmp / tag)
    rc = phaser.main(["--vcf", vcfgz, "--bam", bam, "--sample", "S1", "--mapq", "255", "--baseq", "10", "--paired_end", "1", "--o", prefix, "--write_vcf", "0", "--threads", "3"]
                     + list(extra))
    return rc, prefix


def test_cli_writes_the_file(cli_inputs, mapper, capsys):          # noqa: F811
    from phaser_amd import bamio, vcf
    from phaser_amd.engine import Config, Engine
    rc, prefix = run_cli(cli_inputs, "with_switch", "--output_read_haplotypes", "1")
    assert rc == 0
    assert "read_haplotypes.txt" in capsys.readouterr().out
    got = open(prefix + ".read_haplotypes.txt", "rb").read()
    compare({name: open(prefix + "." + name + ".txt").read() for name in OUTPUTS}, os.path.join(GOLD, "pipe_one"))
    # the same inputs in process
    tmp, bam, vcfgz = cli_inputs
    vs = vcf.load_variants(open(os.path.join(GOLD, "pipe_one", "in.vcf")).read())
    its = {}
    shards = bamio.shards_from_bam_device(mapper.ctx, bam, its, 255, True, True, 0.0, chroms=set(vs.chroms), device="cuda:0")
    assert shards is not None
    eng = Engine(vs, ["a"], Config(want_vcf=True), mapper=mapper)
    eng.add_shards(0, [(c, shards[c].to("cuda:0"), len(its[c]), its[c].names) for c in vs.chroms if c in shards])
    for c in its:
        eng.n_qid[c] = len(its[c])
    eng.close_bam(0)
    eng.finish()
    rh = eng.read_haplotypes()
    assert len(rh["records"]) > 500 and got == rh["text"]


def test_cli_without_the_switch_writes_no_such_file(cli_inputs):          # noqa: F811
    rc, prefix = run_cli(cli_inputs, "without_switch")
    assert rc == 0 and os.path.exists(prefix + ".haplotypic_counts.txt") and not os.path.exists(prefix + ".read_haplotypes.txt")
