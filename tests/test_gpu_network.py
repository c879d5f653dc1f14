"""--output_network on the GPU (phaser/phaser.py:1127-1157): Engine.network and the command line against the two files the reference wrote
(tests/golden/network), and the kernels of phz_variant_links on a hand-built pair table against their numpy restatement (network.links_from_edges)."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, gz_text
from helpers import OUTPUTS
from test_gpu_pipeline import compare, run_product

pytestmark = pytest.mark.gpu

NET = os.path.join(GOLD, "network")
CASES = json.load(open(os.path.join(NET, "cases.json")))["cases"]


def golden(name, which):
    with gzip.open(os.path.join(NET, "%s.%s.txt.gz" % (name, which)), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def mapper():
    from phaser_amd.mapper import Mapper
    return Mapper(0)


def engine_for(mapper, name, **cfg):
    case = CASES[name]
    d = os.path.join(GOLD, case["fixture"])
    bams = {b + ".bam": {c: gz_text(os.path.join(d, "%s.%s.sam.gz" % (b, c))) for c in case["chroms"]} for b in case["bams"]}
    opts = dict(case["options"]); inc = opts.pop("include_indels", 0)
    out, eng = run_product(mapper, open(os.path.join(d, "in.vcf")).read(), bams, "cuda", include_indels=inc, **opts, **cfg)
    return eng


@pytest.mark.parametrize("py_hash_order", [0, 1], ids=["canonical", "py_hash_order"])
@pytest.mark.parametrize("device_rows", [True, False], ids=["device_rows", "host_rows"])
@pytest.mark.parametrize("name", ["two_chr22", "noisy_b_split", "indel_block"])
def test_engine_network_matches_the_reference(mapper, name, device_rows, py_hash_order):
    """(a) the largest block of the SECOND chromosome of a two-BAM sample (non-zero base in the joint variant space, read sets that are unions over BAMs),
    (b) a block phase_v3 cut out of a larger component, (d) a block with an indel allele: the links file byte for byte, the nodes file row for row in the
    canonical tier and byte for byte with py_hash_order."""
    eng = engine_for(mapper, name, device_rows=device_rows, py_hash_order=py_hash_order)
    assert eng.rows_path == ("device" if device_rows else "host")
    net = eng.network(CASES[name]["variant"])
    assert net is not None
    assert net["links"] == golden(name, "links")
    if py_hash_order:
        assert net["nodes"] == golden(name, "nodes")
    else:
        assert sorted(net["nodes"].split(b"\n")) == sorted(golden(name, "nodes").split(b"\n"))
    if name == "two_chr22":
        assert eng.G["var_base"][net["chrom"]] > 0


def test_engine_network_of_a_variant_in_no_block(mapper):
    """(c) a variant that ends as a singleton, and an id the VCF does not hold: no files, no error"""
    eng = engine_for(mapper, "one_singleton")
    assert eng.network(CASES["one_singleton"]["variant"]) is None
    assert eng.network(CASES["one_unknown"]["variant"]) is None
    assert eng.network(CASES["one_block"]["variant"])["links"] == golden("one_block", "links")          # the same pass still serves a variant that is in a block


def test_network_refuses_a_replaced_tally(mapper):
    """The pair cells are those of the context's LAST tally: an Engine whose pass another pass has replaced says so instead of reading the other sample's cells."""
    from phaser_amd import _lib
    first = engine_for(mapper, "one_block")
    second = engine_for(mapper, "noisy_b_split")
    with pytest.raises(_lib.PhzError, match="resident tally"):
        first.network(CASES["one_block"]["variant"])
    assert second.network(CASES["noisy_b_split"]["variant"])["links"] == golden("noisy_b_split", "links")


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    """fixture pipe_one as an unfiltered BAM + gzipped VCF (as in test_gpu_pipeline.test_cli_from_bam_matches_reference)"""
    from phaser_amd import bamio, synth
    tmp = tmp_path_factory.mktemp("network_cli")
    v, gs, ge, w = synth.make_variants("chr22", 1, 3_000_000, 300, 201, n_genes=20)
    rb = synth.make_reads(v, gs, ge, w, 9000, 202)
    bam = str(tmp / "a.bam")
    bamio.readbatch_to_bam(bam, [rb], [("chr21", 46709983), ("chr22", 50818468)])
    vcfgz = str(tmp / "in.vcf.gz")
    with gzip.open(vcfgz, "wt") as f:
        f.write(open(os.path.join(GOLD, "pipe_one", "in.vcf")).read())
    return tmp, bam, vcfgz


def run_cli(cli_inputs, tag, variant):
    from phaser_amd import phaser
    tmp, bam, vcfgz = cli_inputs
    prefix = str(tmp / tag)
    rc = phaser.main(["--vcf", vcfgz, "--bam", bam, "--sample", "S1", "--mapq", "255", "--baseq", "10", "--paired_end", "1", "--o", prefix, "--write_vcf", "0", "--threads", "3",
                      "--output_network", variant])
    return rc, prefix


def test_cli_output_network_writes_the_reference_files(cli_inputs):
    """`--output_network <id in a block>` (refused with "not supported by this build" before this option existed): both files as the reference wrote them, the
    five files unchanged."""
    rc, prefix = run_cli(cli_inputs, "in_block", CASES["one_block"]["variant"])
    assert rc == 0
    assert open(prefix + ".network.links.txt", "rb").read() == golden("one_block", "links")
    assert sorted(open(prefix + ".network.nodes.txt", "rb").read().split(b"\n")) == sorted(golden("one_block", "nodes").split(b"\n"))
    compare({name: open(prefix + "." + name + ".txt").read() for name in OUTPUTS}, os.path.join(GOLD, "pipe_one"))


def test_cli_output_network_of_an_unknown_id(cli_inputs, capsys):
    rc, prefix = run_cli(cli_inputs, "unknown", CASES["one_unknown"]["variant"])
    assert rc == 0
    assert not os.path.exists(prefix + ".network.links.txt") and not os.path.exists(prefix + ".network.nodes.txt")
    assert "is in no phased block" in capsys.readouterr().out
    compare({name: open(prefix + "." + name + ".txt").read() for name in OUTPUTS}, os.path.join(GOLD, "pipe_one"))


# ------------------------------------------------------------------------------------------------ the kernels on a hand-built pair table
NV = 2000


@pytest.fixture(scope="module")
def pair_table():
    """~3,000 pairs over 2,000 variants, sorted by (a, b), adopted WITH their cells as the resident tally of a context of its own (phz_tally_import): twelve
    workgroups of the count / fill kernels, a scan that crosses them.  Pairs of variants 900-1,099 are left out of every set below (a run of > 256 dropped
    edges in the middle of the range); every fifth pair has no non-zero ref/alt cell; the last pair of the list is (1,998, 1,999)."""
    from phaser_amd import _lib
    rng = np.random.default_rng(77)
    a = rng.integers(0, NV - 2, size=3400); b = a + rng.integers(1, 40, size=3400)
    ok = b < NV - 2
    key = np.unique(a[ok].astype(np.int64) * NV + b[ok])
    ea = np.concatenate([key // NV, [NV - 2]]).astype(np.int32); eb = np.concatenate([key % NV, [NV - 1]]).astype(np.int32)
    ne = len(ea)
    cells = rng.integers(0, 4, size=(ne, 9)).astype(np.int32) * (rng.random((ne, 9)) < 0.6)
    cells[::5, [0, 1, 3, 4]] = 0                                   # pairs that only "other" alleles join: no row
    cells[-1] = [0, 7, 1, 0, 0, 2, 3, 0, 0]
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    assert 2900 < ne < 3500 and int(((ea >= 900) & (ea < 1100)).sum()) > 256
    ctx = _lib.Context(0)
    sz = _lib.phz_tally_sizes(0, 0, ne, 0, 0, 0, 0, 0)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    out = _lib.phz_tally_out(None, None, None, None, None, vp(ea), vp(eb), vp(cells), None, None, None, None, None)
    ctx.check(ctx.lib.phz_tally_import(ctx.h, NV, 1, C.byref(sz), C.byref(out), None, _lib.PHZ_HOST))
    return ctx, ea, eb, cells


def gpu_links(ctx, vars, device):
    from phaser_amd import _lib
    from phaser_amd.network import LINK_DTYPE
    vars = np.ascontiguousarray(vars, dtype=np.int32)
    n = C.c_int64(-1)
    if not device:
        st = ctx.check(ctx.lib.phz_variant_links(ctx.h, C.c_void_p(vars.ctypes.data), len(vars), None, 0, C.byref(n), _lib.PHZ_HOST), allow=(_lib.PHZ_E_CAPACITY,))
        rows = np.full((int(n.value) + 1) * 16, 0xA5, dtype=np.uint8)
        if st:
            ctx.check(ctx.lib.phz_variant_links(ctx.h, C.c_void_p(vars.ctypes.data), len(vars), C.c_void_p(rows.ctypes.data), int(n.value), C.byref(n), _lib.PHZ_HOST))
    else:
        dv = torch.from_numpy(vars).cuda()
        torch.cuda.synchronize()
        st = ctx.check(ctx.lib.phz_variant_links(ctx.h, C.c_void_p(dv.data_ptr()), len(vars), None, 0, C.byref(n), _lib.PHZ_DEVICE), allow=(_lib.PHZ_E_CAPACITY,))
        dr = torch.full(((int(n.value) + 1) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if st:
            ctx.check(ctx.lib.phz_variant_links(ctx.h, C.c_void_p(dv.data_ptr()), len(vars), C.c_void_p(dr.data_ptr()), int(n.value), C.byref(n), _lib.PHZ_DEVICE))
        rows = dr.cpu().numpy()
    assert np.all(rows[int(n.value) * 16:] == 0xA5)                  # nothing behind the last row
    return rows[:int(n.value) * 16].view(LINK_DTYPE).copy()


@pytest.mark.parametrize("device", [False, True], ids=["host_args", "device_args"])
def test_kernels_on_a_hand_built_pair_table(pair_table, device):
    from phaser_amd.network import links_from_edges
    ctx, ea, eb, cells = pair_table
    rng = np.random.default_rng(5)
    middle = np.concatenate([np.arange(600, 900), np.arange(1100, 1500)])                             # 700 members in the middle of the space, 900-1,099 left out
    sets = {"700 in the middle": middle,
            "interleaved": np.sort(rng.choice(np.arange(NV), size=1100, replace=False)),             # members and non-members alternate at random
            "every variant": np.arange(NV),
            "the last pair": np.array([NV - 2, NV - 1]),
            "first and last variant": np.array([0, NV - 1]),
            "a pair nobody joins": np.array([3, 1500])}
    for what, vars in sets.items():
        want = links_from_edges(ea, eb, cells, vars)
        got = gpu_links(ctx, vars, device)
        assert got.tobytes() == want.tobytes(), (what, len(got), len(want))
    assert len(links_from_edges(ea, eb, cells, middle)) > 1000 and len(links_from_edges(ea, eb, cells, sets["every variant"])) > 256 * 8 * 2
    last = links_from_edges(ea, eb, cells, sets["the last pair"])
    assert [tuple(int(x) for x in r)[:6] for r in last.tolist()] == [(0, 1, 7, 0, 1, 0), (0, 1, 7, 1, 0, 1)]
