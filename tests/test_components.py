"""The lock-free union-find of phaser_amd/csrc/phz_uf.h (k_uf_init / k_uf_hook / k_uf_flatten) through phz_components, called directly.

Every case compares the labels with one independent CPU reference (helpers.component_labels_cpu: scipy connected_components + the smallest
member of every component) and asserts three properties of the labels on their own: label[v] <= v, label[label] == label, and both
endpoints of every kept edge carry one label.  The edge lists are the ones sequencing reads do NOT produce: one root contended by every
thread, orders that build deep trees before path halving flattens them, a > b edges, self-loops, repeated edges, keep masks that cut a
component, a context reused with a smaller nv.

CPU tests: the kernels under the host emulation (tests/hipemu) at about 2 * 10^4 vertices.  GPU tests: the product kernels at 2^16 and 2^18
vertices; every case prints its PHZ_T_COMPONENTS time (pytest -s).  A shape moves to genome scale (1.5 M vertices, about 3 M edges) once
those times show that it grows in proportion to its size between 2^16 and 2^18: the times have not been measured yet, so none runs there."""
import ctypes as C

import numpy as np
import pytest

from helpers import EmuContext, component_labels_cpu, emu_library


# ------------------------------------------------------------------------------------------------ edge lists
def _chain(lo, hi):
    a = np.arange(lo, hi - 1, dtype=np.int64)
    return a, a + 1


def _cliques(nv, size, max_edges):
    """disjoint cliques of `size` vertices from vertex 0 on, as many as fit into nv and max_edges; the other vertices stay alone"""
    iu, ju = np.triu_indices(size, 1)
    n = max(1, min(nv // size, max_edges // len(iu)))
    base = (np.arange(n, dtype=np.int64) * size)[:, None]
    return (base + iu[None, :]).reshape(-1), (base + ju[None, :]).reshape(-1)


def _random(nv, m, rng):
    return rng.integers(0, nv, m), rng.integers(0, nv, m)


def _two_chains(nv):
    """vertices [0, h) and [h, nv) as two chains, joined by the LAST edge of the list (h - 1, nv - 1)"""
    h = nv // 2
    a1, b1 = _chain(0, h); a2, b2 = _chain(h, nv)
    return np.concatenate([a1, a2, [h - 1]]), np.concatenate([b1, b2, [nv - 1]])


def build(shape, nv, rng, max_edges):
    """(edge_a, edge_b, keep or None) of a named shape on nv >= 4 vertices"""
    keep = None
    if shape == "chain_asc":
        a, b = _chain(0, nv)
    elif shape == "chain_desc":
        a, b = _chain(0, nv); a = a[::-1]; b = b[::-1]
    elif shape == "chain_shuffled":
        a, b = _chain(0, nv); o = rng.permutation(len(a)); a = a[o]; b = b[o]
    elif shape == "chain_swapped":                        # every edge a > b
        b, a = _chain(0, nv)
    elif shape == "star_0":
        b = np.arange(1, nv, dtype=np.int64); a = np.zeros_like(b)
    elif shape == "star_last":                            # centre = the largest index: every hook moves the root
        a = np.arange(0, nv - 1, dtype=np.int64); b = np.full_like(a, nv - 1)
    elif shape == "star_x64":                             # one root, every edge 64 times, the copies of an edge in one wave
        leaves = min(nv - 1, max_edges // 64)
        b = np.repeat(np.arange(1, leaves + 1, dtype=np.int64), 64); a = np.zeros_like(b)
    elif shape == "cliques_64":
        a, b = _cliques(nv, 64, max_edges)
    elif shape == "cliques_256":
        a, b = _cliques(nv, 256, max_edges)
    elif shape == "tree_up":
        a = np.arange(1, nv, dtype=np.int64); b = a // 2
    elif shape == "tree_down":
        b = np.arange(1, nv, dtype=np.int64); a = b // 2
    elif shape == "grid":
        w = int(np.sqrt(nv)); h = nv // w
        idx = np.arange(w * h, dtype=np.int64).reshape(h, w)
        a = np.concatenate([idx[:, :-1].reshape(-1), idx[:-1, :].reshape(-1)]); b = np.concatenate([idx[:, 1:].reshape(-1), idx[1:, :].reshape(-1)])
    elif shape == "random_half":                          # m = nv / 2: a wide spread of component sizes
        a, b = _random(nv, nv // 2, rng)
    elif shape == "random_double":                        # m = 2 nv: one giant component
        a, b = _random(nv, 2 * nv, rng)
    elif shape == "loops_and_repeats":                    # self-loops, one edge 300 times, random edges each repeated a few times
        v = rng.integers(0, nv, nv // 8)
        ra, rb = _random(nv, nv // 8, rng); rep = rng.integers(1, 5, len(ra))
        a = np.concatenate([v, np.full(300, nv - 1), np.repeat(ra, rep)]); b = np.concatenate([v, np.full(300, 1), np.repeat(rb, rep)])
        o = rng.permutation(len(a)); a = a[o]; b = b[o]
    elif shape == "two_chains_bridge":
        a, b = _two_chains(nv)
    elif shape == "two_chains_cut":                       # the mask removes exactly the bridge: two components
        a, b = _two_chains(nv); keep = np.ones(len(a), np.uint8); keep[-1] = 0
    elif shape == "keep_ones":
        a, b = _random(nv, nv, rng); keep = np.ones(len(a), np.uint8)
    elif shape == "keep_zeros":                           # labels must be the identity
        a, b = _random(nv, nv, rng); keep = np.zeros(len(a), np.uint8)
    elif shape == "keep_random":
        a, b = _random(nv, 2 * nv, rng); keep = (rng.random(len(a)) < 0.4).astype(np.uint8)
    else:
        raise KeyError(shape)
    assert len(a) == len(b) and len(a) <= max(max_edges, 2 * nv)
    return np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32), keep


SHAPES = ["chain_asc", "chain_desc", "chain_shuffled", "chain_swapped", "star_0", "star_last", "cliques_64", "tree_up", "tree_down", "grid",
          "random_half", "random_double", "loops_and_repeats", "two_chains_bridge", "two_chains_cut", "keep_ones", "keep_zeros", "keep_random"]
GPU_SHAPES = SHAPES + ["star_x64", "cliques_256"]        # whole waves / whole workgroups CAS on one root


# ------------------------------------------------------------------------------------------------ the call and the checks
def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def components(ctx, nv, ea, eb, keep=None, status=False):
    """phz_components on host arrays -> labels (or the status code)"""
    from phaser_amd import _lib
    lab = np.full(max(nv, 0), -7, dtype=np.int32)
    st = ctx.lib.phz_components(ctx.h, nv, len(ea), _vp(ea), _vp(eb), _vp(keep), _vp(lab), _lib.PHZ_HOST)
    if status:
        return st
    ctx.check(st)
    return lab


def check_labels(lab, nv, ea, eb, keep=None, what=""):
    want = component_labels_cpu(nv, ea, eb, keep)
    assert lab.shape == (nv,) and lab.dtype == np.int32
    k = slice(None) if keep is None else np.nonzero(keep)[0]
    assert np.all(lab <= np.arange(nv)), what                                   # the label is a member no larger than the vertex
    assert np.all(lab >= 0) and np.array_equal(lab[lab], lab), what             # ... and a fixed point
    assert np.array_equal(lab[ea[k]], lab[eb[k]]), what                         # a kept edge never crosses two labels
    bad = np.nonzero(lab != want)[0]
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), lab[bad[:5]].tolist(), want[bad[:5]].tolist())
    return want


def _refusal(ctx, st):
    from phaser_amd import _lib
    assert st == _lib.PHZ_E_ARG
    return (ctx.lib.phz_last_error(ctx.h) or b"").decode()


# ------------------------------------------------------------------------------------------------ CPU: the kernels under the emulation
NV_EMU = 20011
EDGES_EMU = 150_000


@pytest.fixture(scope="module")
def emu():
    return EmuContext(emu_library())


@pytest.mark.parametrize("shape", SHAPES)
def test_components_emulated_matches_scipy(emu, shape):
    rng = np.random.default_rng(SHAPES.index(shape) + 100)
    ea, eb, keep = build(shape, NV_EMU, rng, EDGES_EMU)
    want = check_labels(components(emu, NV_EMU, ea, eb, keep), NV_EMU, ea, eb, keep, shape)
    if shape == "keep_zeros":
        assert np.array_equal(want, np.arange(NV_EMU))
    if shape == "two_chains_cut":
        assert len(np.unique(want)) == 2
    if shape in ("two_chains_bridge", "chain_desc", "star_last", "tree_down"):
        assert not want.any()


@pytest.mark.parametrize("nv", [0, 1, 2, 255, 256, 257])
def test_components_emulated_small_sizes(emu, nv):
    rng = np.random.default_rng(nv)
    none = np.zeros(0, np.int32)
    lab = components(emu, nv, none, none)                                       # n_edges = 0: the identity
    assert np.array_equal(lab, np.arange(nv))
    if nv == 0:
        return
    ea = rng.integers(0, nv, 3 * nv).astype(np.int32); eb = rng.integers(0, nv, 3 * nv).astype(np.int32)
    keep = (rng.random(3 * nv) < 0.3).astype(np.uint8)
    check_labels(components(emu, nv, ea, eb), nv, ea, eb, None, nv)
    check_labels(components(emu, nv, ea, eb, keep), nv, ea, eb, keep, nv)
    a, b = _chain(0, nv)
    a = a[::-1].astype(np.int32); b = b[::-1].astype(np.int32)
    check_labels(components(emu, nv, a, b), nv, a, b, None, nv)


def test_components_emulated_no_edges_is_identity(emu):
    none = np.zeros(0, np.int32)
    assert np.array_equal(components(emu, NV_EMU, none, none), np.arange(NV_EMU))


def _large_small_large(ctx, nv_large, nv_small, max_edges):
    """one context: nv large, then small, then large again -- nothing of an earlier call's parent[] may show"""
    rng = np.random.default_rng(77)
    for i, (nv, shape) in enumerate([(nv_large, "chain_desc"), (nv_small, "random_half"), (nv_large, "random_half"), (nv_small, "keep_zeros"),
                                     (nv_large, "two_chains_cut")]):
        ea, eb, keep = build(shape, nv, rng, max_edges)
        check_labels(components(ctx, nv, ea, eb, keep), nv, ea, eb, keep, (i, nv, shape))


def test_components_emulated_context_reuse_large_small_large():
    _large_small_large(EmuContext(emu_library()), NV_EMU, 300, EDGES_EMU)


def _refusals(ctx):
    from phaser_amd import _lib
    rng = np.random.default_rng(5)
    nv = 1000
    ea, eb, _ = build("random_half", nv, rng, 10 ** 6)
    lab = np.zeros(nv, np.int32)
    call = lambda nv_, ne, a, b, l: ctx.lib.phz_components(ctx.h, nv_, ne, a, b, None, l, _lib.PHZ_HOST)
    assert call(-1, len(ea), _vp(ea), _vp(eb), _vp(lab)) == _lib.PHZ_E_ARG                    # nv < 0
    check_labels(components(ctx, nv, ea, eb), nv, ea, eb)
    assert call(nv, len(ea), _vp(ea), _vp(eb), None) == _lib.PHZ_E_ARG                        # no label array
    check_labels(components(ctx, nv, ea, eb), nv, ea, eb)
    assert "resident" in _refusal(ctx, call(nv, len(ea) + 3, None, None, _vp(lab)))          # no resident edge list of that size
    check_labels(components(ctx, nv, ea, eb), nv, ea, eb)
    assert "NULL" in _refusal(ctx, call(nv, len(ea), _vp(ea), None, _vp(lab)))                # one of the two edge arrays missing
    check_labels(components(ctx, nv, ea, eb), nv, ea, eb)


def test_components_emulated_refusals_leave_the_context_usable():
    _refusals(EmuContext(emu_library()))


def _bad_endpoints(ctx):
    """PHZ_HOST edge arrays with an endpoint outside [0, nv): PHZ_E_ARG before anything is launched, labels untouched, context usable"""
    rng = np.random.default_rng(6)
    nv = 5000
    ea, eb, _ = build("random_double", nv, rng, 10 ** 6)
    for side in (0, 1):
        for bad in (nv, -1, nv + 12345, -2 ** 31, 2 ** 31 - 1):
            for at in (0, len(ea) // 2, len(ea) - 1):
                a = ea.copy(); b = eb.copy()
                (a if side == 0 else b)[at] = bad
                lab = np.full(nv, -7, dtype=np.int32)
                from phaser_amd import _lib
                st = ctx.lib.phz_components(ctx.h, nv, len(a), _vp(a), _vp(b), None, _vp(lab), _lib.PHZ_HOST)
                assert "endpoint" in _refusal(ctx, st), (side, bad, at)
                assert np.all(lab == -7)
    keep = np.ones(len(ea), np.uint8); keep[7] = 0                # an edge that keep[] drops is checked all the same
    a = ea.copy(); a[7] = nv
    assert "endpoint" in _refusal(ctx, components(ctx, nv, a, eb, keep, status=True))
    check_labels(components(ctx, nv, ea, eb), nv, ea, eb)
    # one bad edge among a million good ones
    nv = 40000
    a, b = _random(nv, 1_000_000, rng)
    a = a.astype(np.int32); b = b.astype(np.int32)
    a[rng.integers(0, len(a))] = nv
    assert "endpoint" in _refusal(ctx, components(ctx, nv, a, b, status=True))
    assert "endpoint" in _refusal(ctx, components(ctx, 1, np.ones(1, np.int32), np.zeros(1, np.int32), status=True))
    assert "endpoint" in _refusal(ctx, components(ctx, 0, np.zeros(1, np.int32), np.zeros(1, np.int32), status=True))
    check_labels(components(ctx, 5000, ea, eb), 5000, ea, eb)


def test_components_emulated_bad_endpoint_is_refused():
    _bad_endpoints(EmuContext(emu_library()))


# ------------------------------------------------------------------------------------------------ GPU: the product kernels
EDGES_GPU = 1 << 24

@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    return _lib.Context(0)


def _timed(ctx, nv, ea, eb, keep, what):
    from phaser_amd import _lib
    lab = components(ctx, nv, ea, eb, keep)
    print("PHZ_T_COMPONENTS %-18s nv %8d edges %9d  %9.3f ms" % (what, nv, len(ea), ctx.timing(_lib.PHZ_T_COMPONENTS)[0]))
    return lab


@pytest.mark.gpu
@pytest.mark.parametrize("log2_nv", [16, 18])
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_components_gpu_matches_scipy(gpu_ctx, shape, log2_nv):
    nv = 1 << log2_nv
    rng = np.random.default_rng(GPU_SHAPES.index(shape) + 1000 + log2_nv)
    ea, eb, keep = build(shape, nv, rng, EDGES_GPU)
    check_labels(_timed(gpu_ctx, nv, ea, eb, keep, shape), nv, ea, eb, keep, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [0, 1, 2, 255, 256, 257])
def test_components_gpu_small_sizes(gpu_ctx, nv):
    test_components_emulated_small_sizes(gpu_ctx, nv)


@pytest.mark.gpu
def test_components_gpu_context_reuse_large_small_large():
    from phaser_amd import _lib
    _large_small_large(_lib.Context(0), 1 << 18, 300, EDGES_GPU)


@pytest.mark.gpu
def test_components_gpu_refusals_and_bad_endpoints():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    _refusals(ctx)
    _bad_endpoints(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["chain_desc", "star_last", "cliques_64", "random_double", "loops_and_repeats", "two_chains_cut", "keep_random"])
def test_components_gpu_device_space_equals_host_space(gpu_ctx, shape):
    """edges, keep and labels as device tensors (PHZ_DEVICE): the result of the PHZ_HOST call, and the reference"""
    import torch
    from phaser_amd import _lib
    nv = 1 << 16
    rng = np.random.default_rng(GPU_SHAPES.index(shape) + 3000)
    ea, eb, keep = build(shape, nv, rng, 1 << 21)
    host = components(gpu_ctx, nv, ea, eb, keep)
    dev = torch.device("cuda", gpu_ctx.device)
    ta = torch.from_numpy(ea).to(dev); tb = torch.from_numpy(eb).to(dev)
    tk = torch.from_numpy(keep).to(dev) if keep is not None else None
    tl = torch.full((nv,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    gpu_ctx.check(gpu_ctx.lib.phz_components(gpu_ctx.h, nv, len(ea), C.c_void_p(ta.data_ptr()), C.c_void_p(tb.data_ptr()),
                                     C.c_void_p(tk.data_ptr()) if tk is not None else None, C.c_void_p(tl.data_ptr()), _lib.PHZ_DEVICE))
    got = tl.cpu().numpy()
    assert np.array_equal(got, host)
    check_labels(got, nv, ea, eb, keep, shape)


@pytest.mark.gpu
def test_components_gpu_resident_edge_list():
    """edge_a == edge_b == NULL after a small phz_tally on the same context (the form Engine._component_labels uses): the labels over the
    tally's own edge list, fetched, with every edge, with a random keep[] and with none kept"""
    from phaser_amd import _lib
    from test_emu_tally import run_tally
    ctx = _lib.Context(0)
    rng = np.random.default_rng(31)
    nv = 3000; nq = 4000; n = 20000
    var = np.sort(rng.integers(0, nv, size=n)).astype(np.int32)
    qid = (var // 3 + rng.integers(0, 40, size=n)).astype(np.int32) % nq             # a read touches variants close to each other
    cls = rng.choice([0, 1, 2, 255], size=n, p=[0.45, 0.4, 0.1, 0.05]).astype(np.uint8)
    R = {"nv": nv, "line_var": var, "line_qid": qid, "line_cls": cls, "line_bam": np.zeros(n, np.int32), "bam_offsets": [(0, 0, n)]}
    got, sz = run_tally(ctx, {"tally": {"chrS": R}, "n_qid": {"chrS": nq}}, ["chrS"], 1)
    ea, eb = got["ea"], got["eb"]
    ne = len(ea)
    assert ne == int(sz.n_edges) and ne > 1000
    for keep in (None, (rng.random(ne) < 0.5).astype(np.uint8), np.zeros(ne, np.uint8)):
        lab = np.full(nv, -7, dtype=np.int32)
        ctx.check(ctx.lib.phz_components(ctx.h, nv, ne, None, None, _vp(keep), _vp(lab), _lib.PHZ_HOST))
        check_labels(lab, nv, ea, eb, keep)
    lab = np.zeros(nv, np.int32)
    assert "resident" in _refusal(ctx, ctx.lib.phz_components(ctx.h, nv, ne + 1, None, None, None, _vp(lab), _lib.PHZ_HOST))
    assert "resident" in _refusal(ctx, ctx.lib.phz_components(ctx.h, nv + 1, ne, None, None, None, _vp(lab), _lib.PHZ_HOST))
