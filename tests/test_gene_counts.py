"""K_genes (k_gene_items / phz_gene_counts, phaser_amd/csrc/phz_genes.hip) and phz_hc_parse (phz_genes.cpp) tested directly.

K_genes: the designed inputs of tests/gene_counts_inputs.py -- each aims at one line of the kernel -- against a set union over the label
lists (integer equality, no tolerance).  CPU tests run the kernel text under the host emulation (tests/hipemu), GPU tests the product
library in PHZ_HOST and in PHZ_DEVICE space, twice on one context, with a sentinel behind the declared output.  The entry point's
argument checks and its refusals of host-space indices that would leave the arrays or never end a chain are tested under the emulation
only; the GPU sees only errors that are refused before any HIP call.

phz_hc_parse: the product libphz.so through gene_ae.ParsedCounts against an independent Python parse of the same text (split("\\t"),
split(";"), split(","), drop "", a dictionary for lab_prev) -- label lists, line and field handling, and the chunk merge of the threaded
path on a file large enough for three worker threads.  One chain test goes text -> ParsedCounts -> gene_ae.work_items -> phz_gene_counts
and compares with sets computed from the text alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gene_counts_inputs as gi
from conftest import REPO

HIPEMU = os.path.join(REPO, "tests", "hipemu")
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
EMU_DIR = os.path.join(HIPEMU, "_build", "genes")
SENT = -7


# --------------------------------------------------------------------------------------------------------- libraries and contexts
def emu_lib():
    """phz_api.hip + phz_genes.hip compiled by g++ against the host emulation (tests/test_cis_var.py::_emu_lib is the pattern)"""
    from phaser_amd import _lib
    os.makedirs(EMU_DIR, exist_ok=True)
    lib = os.path.join(EMU_DIR, "libphz_genes.so")
    srcs = [os.path.join(CSRC, "phz_api.hip"), os.path.join(CSRC, "phz_genes.hip"), os.path.join(HIPEMU, "hipemu.cpp")]
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(REPO, "include", "phz.h"), os.path.join(HIPEMU, "hipemu.h")]
    newest = max(os.path.getmtime(p) for p in srcs + hdrs)
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        import fcntl
        with open(os.path.join(EMU_DIR, ".lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
                flags = ["-O1", "-std=c++17", "-fPIC", "-I" + os.path.join(HIPEMU, "include"), "-I" + os.path.join(REPO, "include"), "-I" + CSRC]
                objs = []
                for src in srcs:
                    obj = os.path.join(EMU_DIR, os.path.basename(src) + ".o"); objs.append(obj)
                    lang = [] if src.endswith(".cpp") else ["-x", "c++"]
                    subprocess.check_call(["g++"] + flags + lang + ["-c", src, "-o", obj])
                subprocess.check_call(["g++", "-shared", "-fPIC"] + objs + ["-o", lib + ".tmp", "-lpthread"])
                os.replace(lib + ".tmp", lib)
    L = C.CDLL(lib)
    for name in ("phz_ctx_create", "phz_ctx_destroy", "phz_last_error", "phz_gene_counts"):
        res, args = _lib.SYMBOLS[name]
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


@pytest.fixture(scope="module")
def emu():
    return emu_lib()


@pytest.fixture
def emu_h(emu):
    h = C.c_void_p()
    assert emu.phz_ctx_create(0, C.byref(h)) == 0
    yield h
    emu.phz_ctx_destroy(h)


@pytest.fixture
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def fill_work(enc, dev=None):
    """phz_gene_work over the arrays of an encoded case (host arrays, or device tensors on `dev`) + what keeps them alive"""
    from phaser_amd import _lib
    keep = []

    def ptr(a):
        if not len(a):
            return None
        if dev is None:
            a = np.ascontiguousarray(a); keep.append(a)
            return C.c_void_p(a.ctypes.data)
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev); keep.append(t)
        return C.c_void_p(t.data_ptr())
    w = _lib.phz_gene_work()
    w.n_items = enc.n_items; w.item_lo = ptr(enc.item_lo); w.item_n = ptr(enc.item_n); w.item_run = ptr(enc.item_run)
    w.item_pair = ptr(enc.item_pair); w.item_hap = ptr(enc.item_hap)
    w.n_pairs = enc.n_pairs; w.pair_begin = ptr(enc.pair_begin); w.pair_end = ptr(enc.pair_end)
    w.n_lab_a = len(enc.lab_pos[0]); w.n_lab_b = len(enc.lab_pos[1])
    w.lab_pos_a = ptr(enc.lab_pos[0]); w.lab_prev_a = ptr(enc.lab_prev[0]); w.lab_pos_b = ptr(enc.lab_pos[1]); w.lab_prev_b = ptr(enc.lab_prev[1])
    return w, keep


def call_counts(lib, h, w, n_cells, space, tail=6, dev=None):
    """phz_gene_counts into a buffer of n_cells + tail cells full of SENT -> (status, the n_cells, the tail)"""
    if dev is None:
        out = np.full(n_cells + tail, SENT, dtype=np.int32)
        st = lib.phz_gene_counts(h, C.byref(w) if w is not None else None, C.c_void_p(out.ctypes.data), space)
    else:
        import torch
        t = torch.full((n_cells + tail,), SENT, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        st = lib.phz_gene_counts(h, C.byref(w) if w is not None else None, C.c_void_p(t.data_ptr()), space)
        out = t.cpu().numpy()
    return st, out[:n_cells], out[n_cells:]


def run_counts(lib, h, enc, space, dev=None):
    """one launch of an encoded case -> (status, counts (n_pairs, 2), the cells behind the declared output)"""
    w, keep = fill_work(enc, dev)
    st, got, tail = call_counts(lib, h, w, 2 * enc.n_pairs, space, dev=dev)
    del keep
    return st, got.reshape(-1, 2), tail


def assert_case(lib, h, enc, space, dev=None, what=""):
    st, got, tail = run_counts(lib, h, enc, space, dev)
    assert st == 0, (enc.name, what, lib.phz_last_error(h))
    bad = np.nonzero((got != enc.expected).any(axis=1))[0]
    assert not len(bad), (enc.name, what, "pairs", bad[:8].tolist(), "got", got[bad[:8]].tolist(), "want", enc.expected[bad[:8]].tolist())
    assert (tail == SENT).all(), (enc.name, what, tail.tolist())
    return got


_CASES = {}


def cases(design, emulated):
    """the design's launches, encoded once and shared (the emulated build gets `random` with few one-label items)"""
    key = (design, emulated and design == "random")
    if key not in _CASES:
        built = gi.random(ones_cap=300) if key[1] else gi.DESIGNS[design]()
        _CASES[key] = [(c, gi.encode(c)) for c in built]
    return _CASES[key]


# --------------------------------------------------------------------------------------------------------- the designs themselves
def _inside(case, r, feature):
    return [feature[0] <= p - 1 <= feature[1] for p, _ in case.runs[r][1]]


def test_designs_hold_what_they_promise():
    # bounds
    (c, e), = cases("bounds", True)
    fb, fe = gi.BOUNDS_F
    for r in (0, 1):
        assert sorted(p - 1 for p, _ in c.runs[r][1]) == [fb - 1, fb, fb + 1, fe - 1, fe, fe + 1]
        own = [labels[0] for _, labels in c.runs[r][1]]
        assert len(set(own)) == 6 and all(sum(own[v] in labels for _, labels in c.runs[r][1]) == 1 for v in range(6))
    assert [p for p, _ in c.runs[1][1]] == [p for p, _ in c.runs[0][1]][::-1]
    assert any(a == b for a, b in c.pairs) and (0 < e.expected[[a == b for a, b in c.pairs]]).any()
    assert all((e.expected[k] == 0).all() for k, (a, b) in enumerate(c.pairs) if a > b) and any(a > b for a, b in c.pairs)
    assert any(a <= b and (e.expected[k] == 0).all() for k, (a, b) in enumerate(c.pairs))
    assert any((e.expected[k] == 7).all() for k in range(e.n_pairs))                     # six own labels + "s": everything
    assert e.expected[0].tolist() == [5, 5]
    # walk_on
    (c, e), = cases("walk_on", True)
    ins = _inside(c, 0, gi.WALK_F)
    occ = lambda lab: [ins[v] for v, (_, labels) in enumerate(c.runs[0][1]) if lab in labels]
    assert occ("ioi") == [True, False, True] and occ("oii") == [False, True, True] and occ("ooi") == [False, False, True]
    assert any(labels.count("rep5") == 5 for _, labels in c.runs[0][1])
    long = c.runs[1][1]
    assert len(long) == 64 and all("all" in labels for _, labels in long) and max(gi.encode_run(long)[1]) == 2 * 62
    for v in (0, 31, 63):
        assert (long[v][0] - 1, long[v][0] - 1) in c.pairs
    # any_order
    (c, e), = cases("any_order", True)
    p0 = [p for p, _ in c.runs[0][1]]; p1 = [p for p, _ in c.runs[1][1]]
    assert p0 == sorted(p0, reverse=True) and len(set(p0)) == len(p0)
    assert p1 != sorted(p1) and p1 != sorted(p1, reverse=True) and len(set(p1)) == len(p1) - 1
    assert any(0 < sum(_inside(c, r, f)) < len(c.runs[r][1]) for f in c.pairs for r in (0, 1))
    # slices
    (c, e), *three = cases("slices", True)
    assert e.item_n.tolist() == [3, 3] and (e.item_lo != e.item_run).any() and e.expected[6].tolist() == [3, 0]
    k = int(np.argmax(e.item_lo))
    last = e.lab_prev[0][e.item_lo[k] + 2]                                # "x" in the second item: two steps back, the first one outside
    assert last == 3 and e.lab_pos[0][e.item_run[k] + last] == 50 and e.lab_prev[0][e.item_run[k] + last] == 0
    for c, e in three:
        assert all(8500 <= c.n_labels(r) <= 9500 and len(c.runs[r][1]) == 40 for r in (2, 3))
        assert e.item_lo.tolist() != sorted(e.item_lo.tolist())
        assert (e.item_run[e.item_hap == 0] > 0).all()                                    # hap 0: the run does not start its array
    sizes = [sorted(set(e.item_n.tolist())) for _, e in three]
    assert sizes[0][-1] == 4096 and len(sizes[0]) <= 3 and 0 not in sizes[0]
    assert set(gi.SLICE_SIZES) < set(sizes[1]) and 0 in sizes[2]
    e = three[1][1]
    k = int(np.argmax(e.item_lo - e.item_run))                                            # an item deep inside its run
    prev = e.lab_prev[e.item_hap[k]][e.item_lo[k]:e.item_lo[k] + e.item_n[k]]
    assert (prev >= 0).any() and (prev[prev >= 0] < e.item_lo[k] - e.item_run[k]).any()  # chains leave the slice
    assert all(np.array_equal(three[0][1].expected, e2.expected) for _, e2 in three)
    # wave_tail
    tails = cases("wave_tail", True)
    assert [e.n_items for _, e in tails] == gi.WAVE_TAIL_N
    for c, e in tails:
        slots = list(zip(e.item_pair.tolist(), e.item_hap.tolist()))
        assert len(set(slots)) == len(slots)
        owners = set(e.item_pair.tolist())
        empty = [p for p in range(e.n_pairs) if p not in owners]
        assert empty and (min(empty) < max(owners) or e.n_items < 4)
    # haps
    (c, e), = cases("haps", True)
    assert len(e.lab_pos[0]) != len(e.lab_pos[1]) and e.lab_pos[0].tolist() != e.lab_pos[1].tolist()[:len(e.lab_pos[0])]
    haps_of = lambda p: set(e.item_hap[e.item_pair == p].tolist())
    assert {0} in map(haps_of, range(e.n_pairs)) and {1} in map(haps_of, range(e.n_pairs))
    items = list(zip(e.item_lo.tolist(), e.item_n.tolist(), e.item_run.tolist(), e.item_pair.tolist()))
    twins = [it for it in items if items.count(it) == 2]
    assert twins and e.expected[twins[0][3], 0] != e.expected[twins[0][3], 1]
    lb = [lab for _, labels in c.runs[1][1] for lab in labels]          # haplotype 1's first run read with haplotype 0's positions
    assert c.pairs[3] == (19, 19) and len({lab for lab, p in zip(lb, e.lab_pos[0].tolist()) if p == 20}) != e.expected[3, 1]
    # one_counter
    (c, e), = cases("one_counter", True)
    assert e.n_items == 3000 and set(e.item_n.tolist()) == {1, 2, 3} and len(set(e.item_pair.tolist())) == 1 and len(set(e.item_hap.tolist())) == 1
    # random
    for emulated in (True, False):
        (c, e), = cases("random", emulated)
        assert len(c.runs) == 60 and e.n_pairs == 120 and set(e.item_n.tolist()) - {0} <= set(range(1, 4097))
        assert all(2 <= len(run) <= 11 and all(len(labels) <= 199 for _, labels in run) for _, run in c.runs)
    assert (cases("random", True)[0][1].item_n == 1).sum() <= 300 + 240


def test_reference_is_a_set_union_of_the_variants_inside():
    run = [(10, ["a", "b"]), (20, ["b", "c", "c"]), (30, ["a", "d"])]
    assert gi.expected_counts((9, 9), run) == 2 and gi.expected_counts((9, 19), run) == 3 and gi.expected_counts((19, 29), run) == 4
    assert gi.expected_counts((10, 18), run) == 0 and gi.expected_counts((29, 9), run) == 0 and gi.expected_counts((0, 99), run) == 4
    assert gi.encode_run(run) == ([10, 10, 20, 20, 20, 30, 30], [-1, -1, 1, -1, 3, 0, -1])
    assert gi.cut(10000, [4096] * 8) == [4096, 4096, 1808] and gi.cut(130, gi.SLICE_SIZES) == [1, 63, 64, 2]


# --------------------------------------------------------------------------------------------------------- the emulated kernel
@pytest.mark.parametrize("design", list(gi.DESIGNS))
def test_emulated_kernel_equals_the_set_union(emu, emu_h, design):
    from phaser_amd import _lib
    got = [assert_case(emu, emu_h, e, _lib.PHZ_HOST) for _, e in cases(design, True)]
    if design == "slices":
        assert all(np.array_equal(got[1], g) for g in got[1:])
    if design in ("wave_tail", "haps", "bounds"):                  # caller's memory handed over as it is: the clearing is the entry point's
        for _, e in cases(design, True):
            assert_case(emu, emu_h, e, _lib.PHZ_DEVICE, what="PHZ_DEVICE")


SEQUENCE = [("slices", 2), ("bounds", 0), ("one_counter", 0), ("slices", 3)]


def test_emulated_context_through_changing_sizes(emu, emu_h):
    """staging slots of one context are reused with smaller contents, then with larger ones again"""
    from phaser_amd import _lib
    for design, k in SEQUENCE:
        assert_case(emu, emu_h, cases(design, True)[k][1], _lib.PHZ_HOST, what="sequence")


def _empty(n_pairs):
    c = gi.Case("empty", [], [(0, 10)] * n_pairs, [])
    return gi.encode(c)


def test_no_items_gives_zeros(emu, emu_h):
    from phaser_amd import _lib
    for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
        st, got, tail = run_counts(emu, emu_h, _empty(5), space)
        assert st == 0 and (got == 0).all() and got.shape == (5, 2) and (tail == SENT).all()


def _no_pairs_writes_nothing(lib, h, dev=None):
    from phaser_amd import _lib
    for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
        if dev is not None and space == _lib.PHZ_HOST:
            w, keep = fill_work(_empty(0))
            st, got, tail = call_counts(lib, h, w, 0, space, tail=4)
        else:
            w, keep = fill_work(_empty(0), dev)
            st, got, tail = call_counts(lib, h, w, 0, space, tail=4, dev=dev)
        assert st == 0 and tail.tolist() == [SENT] * 4, (space, tail.tolist())
        assert lib.phz_gene_counts(h, C.byref(w), None, space) == 0


def test_no_pairs_writes_nothing(emu, emu_h):
    _no_pairs_writes_nothing(emu, emu_h)


def _refused_before_any_hip_call(lib, h, dev=None):
    """NULL work, negative counts, NULL pair_counts with pairs: PHZ_E_ARG, a message, the output untouched, the context still good"""
    from phaser_amd import _lib
    enc = cases("haps", True)[0][1]
    for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
        d = dev if space == _lib.PHZ_DEVICE else None
        n = 2 * enc.n_pairs
        st, got, tail = call_counts(lib, h, None, n, space, dev=d)
        assert st == _lib.PHZ_E_ARG and (got == SENT).all() and (tail == SENT).all() and b"NULL" in lib.phz_last_error(h)
        for field in ("n_items", "n_pairs", "n_lab_a", "n_lab_b"):
            w, keep = fill_work(enc, d)
            setattr(w, field, -1)
            st, got, tail = call_counts(lib, h, w, n, space, dev=d)
            assert st == _lib.PHZ_E_ARG and (got == SENT).all() and (tail == SENT).all() and b"negative" in lib.phz_last_error(h), field
        w, keep = fill_work(enc, d)
        assert lib.phz_gene_counts(h, C.byref(w), None, space) == _lib.PHZ_E_ARG and b"NULL" in lib.phz_last_error(h)
        assert lib.phz_gene_counts(None, C.byref(w), None, space) == _lib.PHZ_E_ARG
        assert_case(lib, h, enc, space, d, what="after refusals")


def test_argument_errors(emu, emu_h):
    from phaser_amd import _lib
    _refused_before_any_hip_call(emu, emu_h)
    enc = cases("haps", True)[0][1]
    n = 2 * enc.n_pairs
    for space in (_lib.PHZ_HOST, _lib.PHZ_DEVICE):
        for field in ("item_lo", "item_n", "item_run", "item_pair", "item_hap", "pair_begin", "pair_end", "lab_pos_a", "lab_prev_a", "lab_pos_b", "lab_prev_b"):
            w, keep = fill_work(enc)
            setattr(w, field, None)
            st, got, tail = call_counts(emu, emu_h, w, n, space)
            assert st == _lib.PHZ_E_ARG and (got == SENT).all() and (tail == SENT).all() and b"NULL" in emu.phz_last_error(emu_h), field
        w, keep = fill_work(enc)
        w.n_pairs = 0                                                    # items that can name no pair
        st, got, tail = call_counts(emu, emu_h, w, n, space)
        assert st == _lib.PHZ_E_ARG and (got == SENT).all() and b"pair" in emu.phz_last_error(emu_h)
        st, got, tail = call_counts(emu, emu_h, fill_work(enc)[0], n, 2)
        assert st == _lib.PHZ_E_ARG and (got == SENT).all() and b"space" in emu.phz_last_error(emu_h)


def _refusal_base():
    """A launch that stays harmless if a check is missing: the arrays are longer than the declared counts (4 spare pairs, 8 spare labels
    per haplotype, spare output cells), and the variant at position 999 lies outside every feature, so no chain starts at or reaches its labels
    ("lone" occurs nowhere else).  Items: [0] hap 0 labels 0..4, [1] hap 0 the two labels at 999, [2] hap 1 labels 0..2, [3] hap 1 at 999."""
    a = [(10, ["1", "2"]), (20, ["1", "3", "2"]), (999, ["lone", "lone2"])]
    b = [(10, ["5"]), (20, ["5", "6"]), (999, ["lone", "lone2"])]
    c = gi.Case("refusal", [(0, a), (1, b)], [(0, 100), (9, 9), (19, 19)], [(0, 0, [5, 2]), (2, 1, [3, 2])], seed=3)
    e = gi.encode(c)
    order = np.lexsort((e.item_lo, e.item_hap))
    for k in ("item_lo", "item_n", "item_run", "item_pair", "item_hap"):
        setattr(e, k, getattr(e, k)[order].copy())
    assert e.item_lo.tolist() == [0, 5, 0, 3] and e.item_n.tolist() == [5, 2, 3, 2]
    return e


def _padded_work(e):
    """phz_gene_work with the declared counts of e over arrays that are longer"""
    from phaser_amd import _lib
    pad = lambda a, n, v: np.concatenate([a, np.full(n, v, dtype=a.dtype)])
    arrays = {"pair_begin": pad(e.pair_begin, 4, 5000), "pair_end": pad(e.pair_end, 4, 6000)}
    for h, s in ((0, "a"), (1, "b")):
        arrays["lab_pos_" + s] = pad(e.lab_pos[h], 8, 999); arrays["lab_prev_" + s] = pad(e.lab_prev[h], 8, -1)
    for k in ("item_lo", "item_n", "item_run", "item_pair", "item_hap"):
        arrays[k] = getattr(e, k).copy()
    w = _lib.phz_gene_work()
    for k, a in arrays.items():
        setattr(w, k, C.c_void_p(a.ctypes.data))
    w.n_items = e.n_items; w.n_pairs = e.n_pairs; w.n_lab_a = len(e.lab_pos[0]); w.n_lab_b = len(e.lab_pos[1])
    return w, arrays


# (name, what to spoil in the arrays / the struct, a word of the message)
REFUSALS = [
    ("item_n < 0", lambda w, A: A["item_n"].__setitem__(1, -1), b"item_n"),
    ("item_hap == 2", lambda w, A: (A["item_hap"].__setitem__(1, 2), A["item_n"].__setitem__(1, 0)), b"item_hap"),
    ("item_pair == n_pairs", lambda w, A: A["item_pair"].__setitem__(1, 3), b"item_pair"),
    ("item_pair == -1", lambda w, A: (A["item_pair"].__setitem__(1, -1), A["item_n"].__setitem__(1, 0)), b"item_pair"),
    ("item_run > item_lo", lambda w, A: A["item_run"].__setitem__(1, 6), b"item_run"),
    ("item_run < 0", lambda w, A: A["item_run"].__setitem__(1, -1), b"item_run"),
    ("item_lo + item_n > n_lab_a", lambda w, A: setattr(w, "n_lab_a", 6), b"n_lab"),
    ("item_lo + item_n > n_lab_b", lambda w, A: A["item_n"].__setitem__(3, 3), b"n_lab"),
    ("item_lo > n_lab", lambda w, A: (A["item_lo"].__setitem__(1, 8), A["item_n"].__setitem__(1, 0)), b"n_lab"),
    ("lab_prev points at itself", lambda w, A: A["lab_prev_a"].__setitem__(5, 5), b"lab_prev"),
    ("lab_prev points forwards", lambda w, A: A["lab_prev_b"].__setitem__(3, 4), b"lab_prev"),
    ("lab_prev < -1", lambda w, A: A["lab_prev_a"].__setitem__(6, -2), b"lab_prev"),
    ("lab_prev of a later slice points at its own label", lambda w, A: A["lab_prev_b"].__setitem__(4, 4), b"lab_prev"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_host_space_indices_are_refused(emu, emu_h, k):
    """Every index the kernel would follow out of the arrays, and every lab_prev that could keep a chain from ending, is PHZ_E_ARG with a
    message before anything is staged or launched: the output keeps its sentinel, and the context then serves a good launch."""
    from phaser_amd import _lib
    e = _refusal_base()
    name, spoil, word = REFUSALS[k]
    w, arrays = _padded_work(e)
    st, got, tail = call_counts(emu, emu_h, w, 2 * e.n_pairs, _lib.PHZ_HOST)          # the base itself is good, padding and all
    assert st == 0 and np.array_equal(got.reshape(-1, 2), e.expected) and (tail == SENT).all()
    spoil(w, arrays)
    st, got, tail = call_counts(emu, emu_h, w, 2 * e.n_pairs, _lib.PHZ_HOST)
    assert st == _lib.PHZ_E_ARG, name
    assert (got == SENT).all() and (tail == SENT).all(), name
    assert word in emu.phz_last_error(emu_h), (name, emu.phz_last_error(emu_h))
    assert_case(emu, emu_h, e, _lib.PHZ_HOST, what="after " + name)


def test_prev_limits_that_are_allowed(emu, emu_h):
    """the bound is strict on one side only: lab_prev[p] == p - item_run - 1 (the label just before) and -1 pass"""
    from phaser_amd import _lib
    e = _refusal_base()
    w, arrays = _padded_work(e)
    arrays["lab_prev_a"][6] = 5; arrays["lab_prev_b"][4] = 3
    st, got, tail = call_counts(emu, emu_h, w, 2 * e.n_pairs, _lib.PHZ_HOST)
    assert st == 0 and np.array_equal(got.reshape(-1, 2), e.expected) and (tail == SENT).all()


def test_large_label_arrays_are_checked_by_every_thread(emu, emu_h):
    """From 2^20 declared labels on, the items are shared out among host threads: a broken item is found wherever it lies in the
    item list, the lowest broken item's message is the one reported, and a good launch of that size still counts right."""
    from phaser_amd import _lib
    e = _refusal_base()
    big = (1 << 20) + 5
    n_copies = 61                                                        # of item 1, whose labels lie outside every feature

    def work():
        w, A = _padded_work(e)
        for s in ("a", "b"):
            A["lab_pos_" + s] = np.concatenate([A["lab_pos_" + s], np.full(big, 999, np.int32)])
            A["lab_prev_" + s] = np.concatenate([A["lab_prev_" + s], np.full(big, -1, np.int32)])
        for k in ("item_lo", "item_n", "item_run", "item_pair", "item_hap"):
            A[k] = np.concatenate([A[k], np.repeat(A[k][1:2], n_copies)])
        for k, a in A.items():
            setattr(w, k, C.c_void_p(a.ctypes.data))
        w.n_items = e.n_items + n_copies; w.n_lab_a = len(A["lab_pos_a"]) - 3; w.n_lab_b = len(A["lab_pos_b"]) - 3
        return w, A
    w, A = work()
    st, got, tail = call_counts(emu, emu_h, w, 2 * e.n_pairs, _lib.PHZ_HOST)
    assert st == 0 and np.array_equal(got.reshape(-1, 2), e.expected) and (tail == SENT).all()
    for at in range(4, e.n_items + n_copies, 7):                         # one broken item at a time, all over the list
        w, A = work()
        A["item_pair"][at] = e.n_pairs
        st, got, tail = call_counts(emu, emu_h, w, 2 * e.n_pairs, _lib.PHZ_HOST)
        assert st == _lib.PHZ_E_ARG and (got == SENT).all() and b"item_pair" in emu.phz_last_error(emu_h), at
    w, A = work()
    A["item_n"][60] = -1; A["item_run"][10] = -1
    st, got, tail = call_counts(emu, emu_h, w, 2 * e.n_pairs, _lib.PHZ_HOST)
    assert st == _lib.PHZ_E_ARG and (got == SENT).all() and b"item_run" in emu.phz_last_error(emu_h)


# --------------------------------------------------------------------------------------------------------- the product kernel
@pytest.mark.gpu
@pytest.mark.parametrize("design", list(gi.DESIGNS))
def test_gpu_kernel_equals_the_set_union_in_both_spaces_twice(gpu_ctx, design):
    import torch
    from phaser_amd import _lib
    dev = torch.device("cuda", gpu_ctx.device)
    got = []
    for _, e in cases(design, False):
        for turn in (1, 2):
            got.append(assert_case(gpu_ctx.lib, gpu_ctx.h, e, _lib.PHZ_HOST, what="PHZ_HOST, run %d" % turn))
            got.append(assert_case(gpu_ctx.lib, gpu_ctx.h, e, _lib.PHZ_DEVICE, dev, what="PHZ_DEVICE, run %d" % turn))
    if design == "slices":
        assert all(np.array_equal(got[4], g) for g in got[4:])           # the three cuts, four launches each


@pytest.mark.gpu
def test_gpu_context_through_changing_sizes(gpu_ctx):
    from phaser_amd import _lib
    for design, k in SEQUENCE:
        assert_case(gpu_ctx.lib, gpu_ctx.h, cases(design, False)[k][1], _lib.PHZ_HOST, what="sequence")


@pytest.mark.gpu
def test_gpu_no_pairs_writes_nothing(gpu_ctx):
    import torch
    from phaser_amd import _lib
    dev = torch.device("cuda", gpu_ctx.device)
    _no_pairs_writes_nothing(gpu_ctx.lib, gpu_ctx.h, dev)
    st, got, tail = run_counts(gpu_ctx.lib, gpu_ctx.h, _empty(5), _lib.PHZ_DEVICE, dev)
    assert st == 0 and (got == 0).all() and (tail == SENT).all()


@pytest.mark.gpu
def test_gpu_argument_errors_refused_before_any_hip_call(gpu_ctx):
    import torch
    _refused_before_any_hip_call(gpu_ctx.lib, gpu_ctx.h, torch.device("cuda", gpu_ctx.device))


# --------------------------------------------------------------------------------------------------------- phz_hc_parse
COLS = ["contig", "start", "stop", "variants", "variantCount", "variantsBlacklisted", "variantCountBlacklisted", "haplotypeA", "haplotypeB", "aCount", "bCount",
        "totalCount", "blockGWPhase", "gwStat", "max_haplo_maf", "bam", "aReads", "bReads"]


def hc_text(rows, cols=COLS, eol="\n", last_eol=True):
    """rows: dicts of column -> text; missing columns are empty"""
    lines = ["\t".join(cols)] + ["\t".join(r.get(c, "") for c in cols) for r in rows]
    return (eol.join(lines) + (eol if last_eol else "")).encode()


def row(ids, a_reads, b_reads, contig="chr1", bam="x", a="3", b="2", phase="0|1", gw="0.75", maf="0.1", sep="_"):
    pos = [int(i.split(sep)[1]) for i in ids]
    return {"contig": contig, "start": str(min(pos)), "stop": str(max(pos)), "variants": ",".join(ids), "variantCount": str(len(ids)), "variantCountBlacklisted": "0",
            "aCount": a, "bCount": b, "totalCount": str(int(float(a)) + int(float(b))), "blockGWPhase": phase, "gwStat": gw, "max_haplo_maf": maf, "bam": bam,
            "aReads": a_reads, "bReads": b_reads}


def ids_at(positions, contig="chr1", sep="_"):
    return [sep.join([contig, str(p), "A", "G"]) for p in positions]


def py_parse(text, sep="_"):
    """The same text read with str.split only; a dictionary per (row, haplotype) gives lab_prev.  Keys are ParsedCounts' attributes."""
    lines = text.decode().split("\n")
    header = lines[0][:-1] if lines[0].endswith("\r") else lines[0]
    col = {n: i for i, n in enumerate(header.split("\t"))}
    num = lambda s: int(float(s)) if "." in s else int(s)
    R = {k: [] for k in ("contig", "start", "stop", "a_count", "b_count", "total", "bam", "phase", "gw_stat", "maf", "var_pos", "var_id_off", "var_id_len")}
    R["var_off"] = [0]; R["lab_off"] = [[0], [0]]; R["lab_pos"] = [[], []]; R["lab_prev"] = [[], []]
    R["contig_names"] = []; R["bam_names"] = []; R["var_ids"] = []
    R["has_maf"] = "max_haplo_maf" in col

    def number_of(name, names):
        if name not in names:
            names.append(name)
        return names.index(name)
    at = len(lines[0]) + 1
    for line in lines[1:]:
        here = at; at += len(line) + 1
        if line.endswith("\r"):
            line = line[:-1]
        if not line:
            continue
        f = line.split("\t")
        f += [""] * (len(col) - len(f))
        R["contig"].append(number_of(f[col["contig"]], R["contig_names"])); R["bam"].append(number_of(f[col["bam"]], R["bam_names"]))
        for k, c in (("start", "start"), ("stop", "stop"), ("a_count", "aCount"), ("b_count", "bCount"), ("total", "totalCount")):
            R[k].append(num(f[col[c]]))
        R["phase"].append({"0/1": 0, "0|1": 1, "1|0": 2}.get(f[col["blockGWPhase"]], 3))
        R["gw_stat"].append(float(f[col["gwStat"]])); R["maf"].append(float(f[col["max_haplo_maf"]]) if R["has_maf"] else 0.0)
        o = here + sum(len(x) + 1 for x in f[:col["variants"]])
        ids = f[col["variants"]].split(",")
        pos = []
        for i in ids:
            pos.append(int(i.split(sep)[1])); R["var_id_off"].append(o); R["var_id_len"].append(len(i)); R["var_ids"].append(i)
            o += len(i) + 1
        R["var_pos"] += pos; R["var_off"].append(R["var_off"][-1] + len(ids))
        for hap, c in ((0, "aReads"), (1, "bReads")):
            last = {}; n = 0
            if len(ids) > 1:
                for v, group in enumerate(f[col[c]].split(";")):
                    for lab in group.split(","):
                        if lab == "":
                            continue
                        R["lab_prev"][hap].append(last.get(lab, -1)); last[lab] = n; n += 1
                        R["lab_pos"][hap].append(pos[v])                 # IndexError: more groups than variants
            R["lab_off"][hap].append(R["lab_off"][hap][-1] + n)
    return R


def assert_parsed(P, want, what=""):
    for k in ("contig", "start", "stop", "a_count", "b_count", "total", "bam", "phase", "gw_stat", "maf", "var_pos", "var_id_off", "var_id_len", "var_off"):
        assert getattr(P, k).tolist() == want[k], (what, k)
    for hap in (0, 1):
        for k in ("lab_off", "lab_pos", "lab_prev"):
            assert getattr(P, k)[hap].tolist() == want[k][hap], (what, k, hap)
        assert P.n_lab[hap] == len(want["lab_pos"][hap])
    assert P.contig_names == want["contig_names"] and P.bam_names == want["bam_names"], what
    assert P.has_maf == want["has_maf"] and P.n_rows == len(want["start"]) and P.n_vars == len(want["var_pos"]), what


def parsed(text, sep="_", threads=1):
    from phaser_amd import gene_ae
    return gene_ae.ParsedCounts(text, sep, threads)


@pytest.fixture
def built():
    """the CPU tests of the parser make sure libphz.so is up to date with its sources"""
    from phaser_amd import _lib
    _lib.build()


def raw_status(text, sep="_", threads=1):
    """phz_hc_parse's own status and message"""
    from phaser_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    st = lib.phz_hc_parse(C.cast(C.c_char_p(text), C.c_void_p), len(text), sep.encode(), threads, C.byref(h))
    msg = (lib.phz_hc_error(h) or b"").decode()
    lib.phz_hc_free(h)
    return st, msg


def test_parser_label_lists(built):
    three = ids_at([10, 20, 30])
    rows = [
        row(three, ",,1,,2,;;3,", ",4;5,,;"),                            # blank labels, an empty group, trailing ',' and ';'
        row(three, "01,1,001;1,01;1", "7;07;7"),                         # text, not numbers
        row(three, "1234567890,1234567891;1234567890;9999999999,1234567891", "4294967296;4294967296,0;0"),
        row(three, "5,5,6,5;6,6;5", "8,8,8;;8"),                         # repeats inside one variant
        row(three, "5;5;5", "5;5;5"),                                    # the same text again: a's, b's and the next row's chains all start anew
        row(three, "1,2", "3;4"),                                        # fewer groups than variants
        row(ids_at([50]), "1,2,3;4", "9,9"),                             # single variant: label text is not read
        row(ids_at([60, 70]), "", ""),
    ]
    text = hc_text(rows)
    want = py_parse(text)
    P = parsed(text)
    assert_parsed(P, want)
    # and spelled out, so that a mistake shared by the two parsers does not pass
    assert P.lab_off[0].tolist() == [0, 3, 9, 14, 21, 24, 26, 26, 26] and P.lab_off[1].tolist() == [0, 2, 5, 9, 13, 16, 18, 18, 18]
    assert P.lab_pos[0][:3].tolist() == [10, 10, 30] and P.lab_prev[0][:3].tolist() == [-1, -1, -1]
    assert P.lab_pos[1][:2].tolist() == [10, 20]
    assert P.lab_prev[0][3:9].tolist() == [-1, -1, -1, 1, 0, 3]          # "01" "1" "001" | "1" "01" | "1"
    assert P.lab_prev[1][2:5].tolist() == [-1, -1, 0]                    # "7" | "07" | "7"
    assert P.lab_prev[0][9:14].tolist() == [-1, -1, 0, -1, 1] and P.lab_prev[1][5:9].tolist() == [-1, 0, -1, 2]
    assert P.lab_prev[0][14:21].tolist() == [-1, 0, -1, 1, 2, 4, 3] and P.lab_prev[1][9:13].tolist() == [-1, 0, 1, 2]
    assert P.lab_prev[0][21:24].tolist() == [-1, 0, 1] and P.lab_prev[1][13:16].tolist() == [-1, 0, 1]
    assert P.lab_pos[0][24:26].tolist() == [10, 10] and P.lab_pos[1][16:18].tolist() == [10, 20]


def test_parser_refuses_more_groups_than_variants(built):
    from phaser_amd import _lib
    text = hc_text([row(ids_at([10, 20]), "1;2;3", "1;2")])
    st, msg = raw_status(text)
    assert st == _lib.PHZ_E_ARG and "more read-label groups than variants" in msg
    with pytest.raises(IndexError):
        py_parse(text)
    with pytest.raises(_lib.PhzError):
        parsed(text)
    assert raw_status(hc_text([row(ids_at([10, 20]), "1;2;", "1;2;;,")]))[0] == 0      # blank groups beyond the variants hold no label


def test_parser_lines_and_fields(built):
    from phaser_amd import _lib
    base = [row(ids_at([10, 20]), "1;1,2", "3;4", contig="chr2", bam="s1", a="3.0", b="2", phase="1|0", gw="0.5"),
            row(ids_at([30]), "", "", bam="s2", phase="0/1", gw="1"),
            row(ids_at([40, 50, 60]), "1;;1", ";2;2", bam="s1", phase="x", gw="nan", maf="0.25")]
    plain = hc_text(base)
    want = py_parse(plain)
    assert want["a_count"] == [3, 3, 3] and want["phase"] == [2, 0, 3] and want["contig_names"] == ["chr2", "chr1"] and want["bam_names"] == ["s1", "s2"]
    P = parsed(plain)
    assert P.gw_stat.tolist()[:2] == [0.5, 1.0] and np.isnan(P.gw_stat[2]) and P.maf.tolist() == [0.1, 0.1, 0.25]
    want["gw_stat"][2] = P.gw_stat[2] = 0.0                              # NaN is not equal to itself
    assert_parsed(P, want, "plain")
    assert [P.var_id(i) for i in range(P.n_vars)] == want["var_ids"] == ids_at([10, 20, 30, 40, 50, 60])

    def same_but(text, what):
        w = py_parse(text); Q = parsed(text)
        w["gw_stat"][2] = Q.gw_stat[2] = 0.0
        assert_parsed(Q, w, what)
        for k in ("contig", "start", "stop", "a_count", "phase", "bam", "var_pos", "var_off", "contig_names", "bam_names", "lab_off", "lab_pos", "lab_prev"):
            assert w[k] == want[k], (what, k)
        assert [Q.var_id(i) for i in range(Q.n_vars)] == w["var_ids"]
        return Q
    same_but(hc_text(base, eol="\r\n"), "CRLF")
    same_but(hc_text(base, last_eol=False), "no newline at the end")
    same_but(hc_text(base, eol="\r\n", last_eol=False), "CRLF, no newline at the end")
    same_but(plain.replace(b"\nchr1", b"\n\n\nchr1") + b"\n\n", "empty lines")
    same_but(hc_text(base, cols=COLS[::-1]), "columns reversed")
    same_but(hc_text(base, cols=COLS[9:] + ["extra"] + COLS[:9]), "columns rotated, one unknown")
    Q = same_but(hc_text(base, cols=[c for c in COLS if c != "max_haplo_maf"]), "no maf column")
    assert Q.has_maf is False and Q.maf.tolist() == [0.0, 0.0, 0.0]
    # a separator of two characters
    two = [dict(r, variants=r["variants"].replace("_", "::")) for r in base]
    text = hc_text(two)
    w = py_parse(text, "::"); Q = parsed(text, "::")
    w["gw_stat"][2] = Q.gw_stat[2] = 0.0
    assert_parsed(Q, w, "two-character separator")
    assert w["var_pos"] == [10, 20, 30, 40, 50, 60] and Q.var_id(1) == "chr1::20::A::G"
    # no bam column: results of phASER before 1.0.0
    st, msg = raw_status(hc_text(base, cols=[c for c in COLS if c != "bam"]))
    assert st == _lib.PHZ_E_UNSUPPORTED and msg == "ERROR - this version of phaser_gene_ae is only compatible with results from phASER v1.0.0+"


N_BIG = 9001


def _big_file():
    """9,001 rows (so 3 worker threads, 12 chunks) whose contig and BAM names first appear all over the file, later stretches meeting
    them in another order than the file does"""
    rng = np.random.default_rng(21)
    contigs = ["chr%d" % c for c in (7, 3, 11, 1, 19, 5, 2, 13)]; bams = ["s%d" % b for b in (4, 2, 9, 1, 6, 3)]
    rows = []
    for i in range(N_BIG):
        stage = i * 12 // N_BIG                                         # names come into use stage by stage, the newest ones first within a stage
        c_pool = contigs[:2 + stage // 2][::-1] if stage % 2 else contigs[:2 + stage // 2]
        b_pool = bams[:1 + stage // 2][::-1]
        contig = c_pool[0] if i % 750 == 1 else c_pool[int(rng.integers(0, len(c_pool)))]
        bam = b_pool[0] if i % 750 == 2 else b_pool[int(rng.integers(0, len(b_pool)))]
        nv = int(rng.integers(1, 5))
        pos = np.sort(rng.choice(np.arange(1, 5000), nv, replace=False)) + 10 * i
        labs = lambda: ";".join(",".join(map(str, rng.integers(0, 6, int(rng.integers(0, 5))).tolist())) for _ in range(nv))
        rows.append(row(ids_at(pos.tolist(), contig), labs(), labs(), contig=contig, bam=bam, a=str(int(rng.integers(0, 50))), b=str(int(rng.integers(0, 50))),
                        phase=["0/1", "0|1", "1|0"][i % 3], gw="%.3f" % rng.random(), maf="%.2f" % (rng.random() / 2)))
    return hc_text(rows)


def test_parser_threads_merge_chunks_in_file_order(built):
    text = _big_file()
    want = py_parse(text)
    assert len(want["start"]) == N_BIG and len(want["contig_names"]) == 7 and len(want["bam_names"]) == 6
    # the stretch after the middle meets names in another order than the file: chunk-local numbers cannot be file numbers
    first_seen = lambda xs: list(dict.fromkeys(xs))
    late_c = first_seen(want["contig"][N_BIG // 2:]); late_b = first_seen(want["bam"][N_BIG // 2:])
    assert late_c != sorted(late_c) and late_b != sorted(late_b)
    assert first_seen(want["contig"]) == list(range(7)) and first_seen(want["bam"]) == list(range(6))          # first-appearance order
    for threads in (1, 2, 3, 16):
        assert_parsed(parsed(text, threads=threads), want, "threads=%d" % threads)


# --------------------------------------------------------------------------------------------------------- parser -> kernel
def _chain_input():
    """three rows: the walk_on patterns, the chain of 63, and a row of 5,000 labels per haplotype (two work items each)"""
    (c, _), = cases("walk_on", True)
    rng = np.random.default_rng(22)
    reads = lambda run: ";".join(",".join(labels) for _, labels in run)
    rows = []
    for _, run in c.runs:
        other = [(p, labels[::-1] + ["b%d" % p]) for p, labels in run]
        rows.append(row(ids_at([p for p, _ in run]), reads(run), reads(other)))
    pos = list(range(5000, 5020))
    rows.append(row(ids_at(pos), *[";".join(",".join(map(str, rng.integers(0, 400, 250).tolist())) for _ in pos) for _ in (0, 1)]))
    feats = [(0, f) for f in c.pairs[:4]] + [(1, f) for f in c.pairs[4:]] + [(2, (4999, 5018)), (2, (5009, 5009)), (2, (5015, 9000)), (2, (0, 10))]
    return hc_text(rows), feats


def _chain(lib, h, space, dev=None):
    from phaser_amd import gene_ae
    text, feats = _chain_input()
    P = parsed(text, threads=2)
    rows = np.asarray([r for r, _ in feats], dtype=np.int64)
    e = gi.Encoded()
    e.name = "chain"
    e.item_lo, e.item_n, e.item_run, e.item_pair, e.item_hap = gene_ae.work_items(P.lab_off, rows, np.arange(len(feats), dtype=np.int64))
    e.n_items = len(e.item_lo); e.n_pairs = len(feats)
    assert sorted(e.item_n[e.item_pair == 8].tolist()) == [904, 904, 4096, 4096]
    e.pair_begin = np.asarray([f[0] for _, f in feats], dtype=np.int32); e.pair_end = np.asarray([f[1] for _, f in feats], dtype=np.int32)
    e.lab_pos = P.lab_pos; e.lab_prev = P.lab_prev
    # the sets, from the text alone
    lines = text.decode().split("\n")[1:]
    e.expected = np.zeros((len(feats), 2), dtype=np.int32)
    for k, (r, (fb, fe)) in enumerate(feats):
        f = lines[r].split("\t")
        pos = [int(i.split("_")[1]) for i in f[COLS.index("variants")].split(",")]
        for hap, c in ((0, "aReads"), (1, "bReads")):
            groups = f[COLS.index(c)].split(";")
            e.expected[k, hap] = len(set().union(*[groups[v].split(",") for v in range(len(pos)) if fb <= pos[v] - 1 <= fe]) - {""})
    assert e.expected[0].tolist() == [8, 12] and e.expected[4].tolist() == [2, 3]
    assert_case(lib, h, e, space, dev, what="text to counts")


def test_text_to_counts_emulated(built, emu, emu_h):
    from phaser_amd import _lib
    _chain(emu, emu_h, _lib.PHZ_HOST)


@pytest.mark.gpu
def test_text_to_counts_gpu(gpu_ctx):
    from phaser_amd import _lib
    _chain(gpu_ctx.lib, gpu_ctx.h, _lib.PHZ_HOST)
