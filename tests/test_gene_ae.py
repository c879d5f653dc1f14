"""phaser_gene_ae drop-in (phaser_amd/gene_ae.py): native parser + K_genes + host aggregation vs what the reference's script wrote
(tests/golden/gene_ae/*).  The GPU test runs the product path; the CPU test replaces only the kernel launch by a Python
restatement of the same per-item rule, so that parser, pair finding, aggregation and formatting are covered without a GPU.
`_items_on_cpu` is the kernel's own loop restated line by line: a wrong rule in the kernel would be a wrong rule in it, so it checks the
host stages and nothing else.  The independent check of the rule (a set union over the label lists, on designed inputs) lives in
tests/test_gene_counts.py; the `emulated` tests below put the kernel text itself, under the host emulation, behind the real item builder."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLD, REPO
from test_oracle_gene_ae import CASES, case_inputs


def _canon(text):
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import gene_ae_oracle as go
    return go.canonical(text)


def _items_on_cpu(P, it_lo, it_n, it_run, it_pair, it_hap, p_begin, p_end, out):
    """What k_gene_items computes, one label at a time (test-side checker of the host stages)."""
    for lo, n, run, pair, hap in zip(it_lo.tolist(), it_n.tolist(), it_run.tolist(), it_pair.tolist(), it_hap.tolist()):
        pos = P.lab_pos[hap]; prev = P.lab_prev[hap]
        fb, fe = int(p_begin[pair]), int(p_end[pair])
        c = 0
        for p in range(lo, lo + n):
            x = int(pos[p]) - 1
            if x < fb or x > fe:
                continue
            q = int(prev[p]); first = True
            while q >= 0:
                y = int(pos[run + q]) - 1
                if fb <= y <= fe:
                    first = False
                    break
                q = int(prev[run + q])
            c += first
        out[pair, hap] += c


@pytest.mark.parametrize("name", CASES)
def test_gene_ae_host_stages(name):
    from phaser_amd import _lib, gene_ae
    _lib.build()
    hc, bed, kw, want = case_inputs(name)
    got = gene_ae.gene_ae(hc.encode(), bed, threads=3, _pair_counts=_items_on_cpu, **kw)
    assert _canon(got) == _canon(want)


def _items_on_emulation(P, it_lo, it_n, it_run, it_pair, it_hap, p_begin, p_end, out):
    """the items handed to phz_gene_counts of the emulated build of phz_genes.hip (tests/test_gene_counts.py::emu_lib)"""
    import ctypes as C
    from phaser_amd import _lib
    from test_gene_counts import emu_lib
    L = emu_lib()
    vp = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None
    w = _lib.phz_gene_work()
    w.n_items = len(it_lo); w.item_lo = vp(it_lo); w.item_n = vp(it_n); w.item_run = vp(it_run); w.item_pair = vp(it_pair); w.item_hap = vp(it_hap)
    w.n_pairs = len(p_begin); w.pair_begin = vp(p_begin); w.pair_end = vp(p_end)
    w.n_lab_a = P.n_lab[0]; w.n_lab_b = P.n_lab[1]
    w.lab_pos_a = vp(P.lab_pos[0]); w.lab_prev_a = vp(P.lab_prev[0]); w.lab_pos_b = vp(P.lab_pos[1]); w.lab_prev_b = vp(P.lab_prev[1])
    h = C.c_void_p()
    assert L.phz_ctx_create(0, C.byref(h)) == 0
    try:
        assert out.dtype == np.int32 and out.flags.c_contiguous and out.shape == (len(p_begin), 2)
        st = L.phz_gene_counts(h, C.byref(w), C.c_void_p(out.ctypes.data), _lib.PHZ_HOST)
        assert st == 0, L.phz_last_error(h)
    finally:
        L.phz_ctx_destroy(h)


@pytest.mark.parametrize("name", CASES)
def test_gene_ae_host_stages_with_the_emulated_kernel(name):
    from phaser_amd import _lib, gene_ae
    _lib.build()
    hc, bed, kw, want = case_inputs(name)
    got = gene_ae.gene_ae(hc.encode(), bed, threads=3, _pair_counts=_items_on_emulation, **kw)
    assert _canon(got) == _canon(want)


def _big_block(nvar, lo, hi, nreads_a, nreads_b, seed):
    """one row of nvar variants with lo..hi labels each (drawn from nreads_a / nreads_b reads) and four features over it"""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(np.arange(1000, 9000), nvar, replace=False))
    ids = ["chr7_%d_A_G" % p for p in pos]
    def labels(nreads):
        groups = []
        for v in range(nvar):
            k = int(rng.integers(lo, hi))
            groups.append(",".join(map(str, rng.integers(0, nreads, k).tolist())))
        return ";".join(groups)
    a = labels(nreads_a); b = labels(nreads_b)
    head = "contig\tstart\tstop\tvariants\tvariantCount\tvariantsBlacklisted\tvariantCountBlacklisted\thaplotypeA\thaplotypeB\taCount\tbCount\ttotalCount\tblockGWPhase\tgwStat\tmax_haplo_maf\tbam\taReads\tbReads\n"
    row = "\t".join(["chr7", str(pos[0]), str(pos[-1]), ",".join(ids), str(nvar), "", "0", ",".join("A" * nvar), ",".join("G" * nvar), "100", "100", "200",
                     "1|0", "0.95", "0", "big", a, b]) + "\n"
    bed = "chr7\t900\t9100\tall\nchr7\t%d\t%d\tmid\nchr7\t%d\t%d\tedge\nchr7\t100\t200\tnone\n" % (pos[5] - 1, pos[25], pos[10] - 1, pos[30] - 1)
    return head + row, bed


def test_gene_ae_emulated_big_block_matches_oracle():
    """The twin of the GPU big-block test at about 12,000 labels per haplotype: three work items per pair and haplotype at
    ITEM_LABELS = 4096, chains that cross the items, through the emulated kernel, vs the pinned oracle."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import gene_ae_oracle as go
    from phaser_amd import _lib, gene_ae
    _lib.build()
    hc, bed = _big_block(40, 250, 350, 3000, 2000, seed=6)
    seen = []

    def counting(P, it_lo, *rest):
        seen.append((P.n_lab, len(it_lo)))
        _items_on_emulation(P, it_lo, *rest)
    got = gene_ae.gene_ae(hc.encode(), bed, _pair_counts=counting)
    (n_lab, n_items), = seen
    assert all(2 * 4096 < n <= 3 * 4096 for n in n_lab) and n_items == 3 * 2 * 3, (n_lab, n_items)      # "none" does not meet the row: 3 pairs
    assert _canon(got) == _canon(go.gene_ae(hc, bed))


def test_parser_arrays_small():
    from phaser_amd import _lib, gene_ae
    _lib.build()
    text = ("contig\tstart\tstop\tvariants\tvariantCount\tvariantsBlacklisted\tvariantCountBlacklisted\thaplotypeA\thaplotypeB\taCount\tbCount\t"
            "totalCount\tblockGWPhase\tgwStat\tmax_haplo_maf\tbam\taReads\tbReads\n"
            "chr1\t10\t30\tchr1_10_A_C,chr1_20_G_T,chr1_30_T_A\t3\t\t0\tA,G,T\tC,T,A\t3\t2\t5\t0|1\t0.75\t0\tx\t0,1;1,2;\t;0;0,1\n"
            "chr1\t50\t50\tchr1_50_A_C\t1\t\t0\tA\tC\t4\t1\t5\t0/1\t1\t0\tx\t\t\n").encode()
    P = gene_ae.ParsedCounts(text, "_", 2)
    assert P.n_rows == 2 and P.var_pos.tolist() == [10, 20, 30, 50] and P.var_id(1) == "chr1_20_G_T"
    assert P.lab_off[0].tolist() == [0, 4, 4] and P.lab_pos[0].tolist() == [10, 10, 20, 20] and P.lab_prev[0].tolist() == [-1, -1, 1, -1]
    assert P.lab_off[1].tolist() == [0, 3, 3] and P.lab_pos[1].tolist() == [20, 30, 30] and P.lab_prev[1].tolist() == [-1, 0, -1]
    assert P.phase.tolist() == [1, 0] and P.gw_stat.tolist() == [0.75, 1.0] and P.bam_names == ["x"] and P.contig_names == ["chr1"]


def test_wrong_separator_exits():
    from phaser_amd import _lib, gene_ae
    _lib.build()
    hc, bed, kw, want = case_inputs("pipe_one")
    with pytest.raises(SystemExit):
        gene_ae.gene_ae(hc.encode(), bed, id_separator=":", _pair_counts=_items_on_cpu)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gene_ae_gpu_matches_reference(name):
    from phaser_amd import gene_ae
    hc, bed, kw, want = case_inputs(name)
    got = gene_ae.gene_ae(hc.encode(), bed, **kw)
    assert _canon(got) == _canon(want)


@pytest.mark.gpu
def test_gene_ae_gpu_big_block_matches_oracle():
    """A block with far more labels than one work item holds (several items per pair, long prev chains) vs the pinned oracle."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import gene_ae_oracle as go
    from phaser_amd import gene_ae
    rng = np.random.default_rng(5)
    nvar = 40; pos = np.sort(rng.choice(np.arange(1000, 9000), nvar, replace=False))
    ids = ["chr7_%d_A_G" % p for p in pos]
    def labels(nreads):
        groups = []
        for v in range(nvar):
            k = int(rng.integers(500, 1500))
            groups.append(",".join(map(str, rng.integers(0, nreads, k).tolist())))
        return ";".join(groups)
    a = labels(30000); b = labels(20000)
    head = "contig\tstart\tstop\tvariants\tvariantCount\tvariantsBlacklisted\tvariantCountBlacklisted\thaplotypeA\thaplotypeB\taCount\tbCount\ttotalCount\tblockGWPhase\tgwStat\tmax_haplo_maf\tbam\taReads\tbReads\n"
    row = "\t".join(["chr7", str(pos[0]), str(pos[-1]), ",".join(ids), str(nvar), "", "0", ",".join("A" * nvar), ",".join("G" * nvar), "100", "100", "200",
                     "1|0", "0.95", "0", "big", a, b]) + "\n"
    bed = "chr7\t900\t9100\tall\nchr7\t%d\t%d\tmid\nchr7\t%d\t%d\tedge\nchr7\t100\t200\tnone\n" % (pos[5] - 1, pos[25], pos[10] - 1, pos[30] - 1)
    hc = head + row
    got = gene_ae.gene_ae(hc.encode(), bed)
    assert _canon(got) == _canon(go.gene_ae(hc, bed))


def test_null_feature_interval_is_refused_like_intervaltree():
    """intervaltree 3.x refuses `tree[a:b] = x` with a >= b (ValueError "Null Interval objects not allowed"), which ends the
    reference's script at phaser_gene_ae.py:51; product and oracle stop with the same error instead of inventing a result.  The other
    interval rules relied on (tree[a:b] returns the intervals with begin < b and end > a; the per-variant test at :191 is CLOSED at the
    feature end) are pinned by the *_bounds fixtures, generated by the reference's script on features that sit on those edges."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import gene_ae_oracle as go
    from phaser_amd import _lib, gene_ae
    _lib.build()
    hc, bed, kw, want = case_inputs("pipe_one")
    bad = bed + "chr22\t500\t500\tnull\n"
    with pytest.raises(ValueError):
        go.gene_ae(hc, bad)
    with pytest.raises(ValueError):
        gene_ae.gene_ae(hc.encode(), bad, _pair_counts=_items_on_cpu)
