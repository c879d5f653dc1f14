"""The device exclusive scan on its own, against numpy.cumsum in uint64 with a leading 0, compared exactly over all n + 1 outputs: gscan_excl of
phaser_amd/csrc/phz_scan.h as its dispatch chooses (impl 1: the one-launch decoupled look-back for 32-bit sums of fewer than 4 Mi elements, three launches
otherwise) and forced onto the three launches (impl 2), through phz_selftest_scan.  impl 0 was an older three-launch u32 scan that phz_scan.h no longer holds (what is left of it is private to
phz_bamdev.hip and tested through the BAM entry points); the entry refuses the number.  Every call also returns the element behind out[n], which the entry fills with 0xA5 bytes and no scan may touch.

Emulated part (CPU suite): every size class of the chunk / tile / row arithmetic, every instantiated type pair, the LabelWidth transform, skewed base
pointers, in-place use, one context through scans of very different sizes, the epoch reset, and more than 1,024 chunks (the second trip of the loops of
k_gs_partials, about 8 s per case here, so it stayed in the CPU suite).  The emulation runs workgroups one after the other in ticket order:
a tile's nearest predecessor always holds a prefix of the current epoch, so the look-back never waits, never takes a second round of 64 words, never
meets a stale word, and a misaligned 16-byte access does not trap.  Those are what the GPU part is for.

GPU part (-m gpu): 64 tiles and one either side, the dispatch boundary at 4 Mi, 1,025 chunks, repetitions on one context with different values every
time (a stale status word taken for a current one then gives a wrong sum, not the same one), real alignment with skewed pointers, widening, in-place,
the epoch reset."""
import ctypes as C
import functools

import numpy as np
import pytest

from phaser_amd import _lib

U32, U64 = np.uint32, np.uint64
TILE = 4096                                # GS_CHUNK
BOUNDARY = 4 << 20                         # u32 sums: look-back below, three launches from here on
MANY_CHUNKS = 1025 * TILE + 5              # more than 1,024 chunk sums: the one-block scan of the sums loops and carries
OVER_64_TILES = 65 * TILE + 7
GUARD = {4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}
EPOCH_NEAR_RESET = (1 << 30) - 4

# (impl, input type, sum type, transform): every instantiation the library has
U32_ALL = [(1, U32, U32, 0), (2, U32, U32, 0)]
COMBOS = U32_ALL + [(1, U64, U64, 0), (2, U64, U64, 0), (1, U32, U64, 0), (2, U32, U64, 0), (1, U32, U32, 1), (2, U32, U32, 1)]


def combo_id(c):
    return "impl%d-%s-%s%s" % (c[0], np.dtype(c[1]).name, np.dtype(c[2]).name, "-labelwidth" if c[3] else "")


def label_width(x):
    """LabelWidth of phz_rowsdev.hip: decimal digits + 1"""
    return np.fromiter((len(str(v)) + 1 for v in x.tolist()), dtype=U64, count=len(x))


def reference(x, transform=0):
    ref = np.zeros(len(x) + 1, dtype=U64)
    np.cumsum(label_width(x) if transform else x.astype(U64), dtype=U64, out=ref[1:])
    return ref


def device_scan(ctx, impl, x, out_dtype, transform=0, in_skew=0, out_skew=0, in_place=0, epoch_preset=-1):
    """-> status, n + 2 values: the sums and the guard element behind them"""
    x = np.ascontiguousarray(x)
    out = np.zeros(len(x) + 2, dtype=out_dtype)
    st = ctx.lib.phz_selftest_scan(ctx.h, impl, x.dtype.itemsize, out.dtype.itemsize, transform, C.c_void_p(x.ctypes.data), len(x), in_skew, out_skew, in_place,
                                   epoch_preset, C.c_void_p(out.ctypes.data))
    return st, out


def check(ctx, impl, x, out_dtype, transform=0, ref=None, tag=None, **kw):
    n = len(x)
    ref = reference(x, transform) if ref is None else ref
    # wrap-around is not a behaviour any caller uses: the inputs of these tests stay below it
    assert int(ref[n]) < (1 << 32 if out_dtype == U32 else 1 << 63)
    st, got = device_scan(ctx, impl, x, out_dtype, transform, **kw)
    ctx.check(st)
    what = (tag, "impl", impl, "n", n, kw)
    assert int(got[n + 1]) == GUARD[np.dtype(out_dtype).itemsize], ("wrote behind out[n]",) + what
    bad = np.nonzero(got[:n + 1].astype(U64) != ref)[0]
    assert bad.size == 0, ("first of %d wrong sums at" % bad.size, int(bad[0]), "got", int(got[bad[0]]), "want", int(ref[bad[0]])) + what


def make_inputs(n, in_dtype, out_dtype, transform, rng):
    """name -> n values.  u32 sums: totals below 2^32, one of them in [2^31, 2^32); 64-bit sums: totals above 2^32 (from two values on), below 2^63"""
    d = {"zeros": np.zeros(n, dtype=in_dtype), "ones": np.ones(n, dtype=in_dtype), "bytes": rng.integers(0, 256, n).astype(in_dtype)}
    if transform:
        # the widths change at the powers of ten: both sides of each, and values of every length in between
        edges = np.array([0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 10 ** 6, 10 ** 7 - 1, 10 ** 7, 10 ** 8 - 1, 10 ** 8, 10 ** 9 - 1, 10 ** 9,
                          (1 << 32) - 1], dtype=U64)
        any_len = rng.integers(0, 1 << 32, n, dtype=U64) >> rng.integers(0, 32, n).astype(U64)
        d["digits"] = np.where(rng.random(n) < 0.5, edges[rng.integers(0, len(edges), n)], any_len).astype(in_dtype)
        return d
    hit = rng.random(n) < 1.0 / 50
    k = int(hit.sum())
    sparse = np.zeros(n, dtype=U64)
    if in_dtype == U64:
        sparse[hit] = rng.integers(1 << 33, 1 << 40, k, dtype=U64)
    elif out_dtype == U64:
        sparse[hit] = rng.integers(1 << 31, 1 << 32, k, dtype=U64)
    elif k:
        top = ((1 << 32) - 1) // k
        sparse[hit] = rng.integers(top // 2, top + 1, k, dtype=U64)
    d["sparse"] = sparse.astype(in_dtype)
    if out_dtype == U32:
        if n:
            d["total_in_2^31..2^32"] = np.full(n, (3 << 30) // n, dtype=in_dtype)
    elif in_dtype == U32:
        d["total_above_2^32"] = rng.integers((1 << 32) - 65536, 1 << 32, n, dtype=U64).astype(in_dtype)
    else:
        d["values_above_2^32"] = rng.integers(1 << 32, 1 << 40, n, dtype=U64)
    return d


# ================================================================================================== emulation (CPU suite)
SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 20001, OVER_64_TILES]


def emu_ctx():
    from helpers import EmuContext, emu_library
    return EmuContext(emu_library())


@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_emu_scan_equals_cumsum_at_every_size_class(combo):
    impl, ti, to, tr = combo
    ctx = emu_ctx()
    rng = np.random.default_rng(101)
    for n in SIZES:
        for name, x in make_inputs(n, ti, to, tr, rng).items():
            # (the emulation's time: the 1,024 fibers of the one-block pass cost 35 ms a call whatever n is, and the 65 tiles half a second a call)
            if (name in ("zeros", "ones") and n not in (0, 1, 5, 257, 1025, 4097, 20001)) or (n > 20001 and name == "sparse"):
                continue
            check(ctx, impl, x, to, tr, tag=name)


@pytest.mark.parametrize("combo", U32_ALL + [(1, U32, U64, 0), (1, U32, U32, 1)], ids=combo_id)
def test_emu_scan_with_skewed_base_pointers(combo):
    """in_skew / out_skew elements behind an aligned address: the scalar path of gs_load_rows / gs_store_rows gives the same sums (alignment itself is
    only real on the GPU)"""
    impl, ti, to, tr = combo
    ctx = emu_ctx()
    rng = np.random.default_rng(102)
    for n in (5, 4097, 8193):
        x = make_inputs(n, ti, to, tr, rng)["digits" if tr else "bytes"]
        ref = reference(x, tr)
        for in_skew in range(4):
            for out_skew in range(4):
                check(ctx, impl, x, to, tr, ref=ref, in_skew=in_skew, out_skew=out_skew)


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("dtype", [U32, U64], ids=["uint32", "uint64"])
def test_emu_scan_in_place(impl, dtype):
    """in == out, as radix_sort_pairs calls it"""
    ctx = emu_ctx()
    rng = np.random.default_rng(103)
    for n in (0, 1, 3, 4, 5, 1024, 4096, 4097, 8193, 20001):
        for name, x in make_inputs(n, dtype, dtype, 0, rng).items():
            if name in ("zeros", "ones"):
                continue
            for skew in (0, 1):
                check(ctx, impl, x, dtype, tag=name, in_place=1, in_skew=skew, out_skew=skew)


def status_word_sequence(fresh_ctx):
    """One context through look-back scans of very different sizes (the status words of a larger scan lie beyond the tiles of a smaller one; growth of the
    status array clears it and restarts epoch and tickets), then a fresh context across the epoch reset.  Different values in every scan."""
    ctx = fresh_ctx()
    rng = np.random.default_rng(104)
    for step, n in enumerate((9000, 300000, 1, 9000, 4097, 300000)):
        check(ctx, 1, rng.integers(0, 256, n).astype(U32), U32, tag=("sequence step", step))
    ctx = fresh_ctx()
    for step in range(4):          # epochs 2^30 - 3, 2^30 - 2, then the reset: 1, 2
        check(ctx, 1, rng.integers(0, 256, 9000).astype(U32), U32, tag=("epoch step", step), epoch_preset=EPOCH_NEAR_RESET if step == 0 else -1)


def test_emu_status_words_over_a_sequence_of_scans_and_the_epoch_reset():
    status_word_sequence(emu_ctx)


@pytest.mark.parametrize("impl", [2])
def test_emu_scan_of_more_than_1024_chunks(impl):
    """the one-block scan of the chunk sums takes a second trip, carrying the first one's total"""
    x = np.random.default_rng(105).integers(0, 256, MANY_CHUNKS).astype(U32)
    check(emu_ctx(), impl, x, U32)


def test_emu_scan_refuses_what_is_not_instantiated():
    ctx = emu_ctx()
    x32 = np.ones(8, dtype=U32); x64 = np.ones(8, dtype=U64)
    assert device_scan(ctx, 0, x32, U32)[0] == _lib.PHZ_E_ARG            # impl 0 (the older scan) is gone, whatever the types
    assert device_scan(ctx, 0, x64, U64)[0] == _lib.PHZ_E_ARG
    assert device_scan(ctx, 0, x32, U64)[0] == _lib.PHZ_E_ARG
    assert device_scan(ctx, 1, x64, U64, transform=1)[0] == _lib.PHZ_E_ARG      # LabelWidth: u32 -> u32 only
    assert device_scan(ctx, 2, x32, U64, transform=1)[0] == _lib.PHZ_E_ARG
    assert device_scan(ctx, 0, x32, U32, transform=1)[0] == _lib.PHZ_E_ARG
    assert device_scan(ctx, 1, x32, U64, in_place=1)[0] == _lib.PHZ_E_ARG       # in place: one width
    assert device_scan(ctx, 1, x64, U32)[0] == _lib.PHZ_E_ARG                   # no narrowing scan
    assert device_scan(ctx, 3, x32, U32)[0] == _lib.PHZ_E_ARG
    assert device_scan(ctx, 1, x32, U32, in_skew=4)[0] == _lib.PHZ_E_ARG
    check(ctx, 1, x32, U32)                                                     # and the ctx is still usable


# ================================================================================================== MI355X
@pytest.fixture(scope="module")
def ctx():
    from phaser_amd.mapper import Mapper
    return Mapper(0).ctx


def fresh_gpu_ctx():
    from phaser_amd.mapper import Mapper
    return Mapper(0).ctx


@functools.lru_cache(maxsize=None)
def gpu_case(n, kind, transform=0):
    """(values, reference) computed once and shared by the tests, read-only"""
    rng = np.random.default_rng(n % 100003 + 7)
    if kind == "bytes":
        x = rng.integers(0, 256, n).astype(U32)
    elif kind == "total_in_2^31..2^32":
        x = np.full(n, (3 << 30) // n, dtype=U32)
    elif kind == "total_above_2^32":
        x = rng.integers((1 << 32) - 65536, 1 << 32, n, dtype=U64).astype(U32)
    elif kind == "values_above_2^32":
        x = rng.integers(1 << 32, 1 << 40, n, dtype=U64)
    else:
        x = make_inputs(n, U32, U32, 1, rng)["digits"]
    ref = reference(x, transform)
    x.setflags(write=False); ref.setflags(write=False)
    return x, ref


GPU_SIZES = [1, 4097, 64 * TILE - 1, 64 * TILE, 64 * TILE + 1, 1_000_003, BOUNDARY - 1, BOUNDARY, BOUNDARY + 1, MANY_CHUNKS]


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [1, 2])
def test_gpu_scan_equals_cumsum(ctx, impl):
    """64 tiles and one either side (the look-back's second round of 64 words needs more than 64 tiles in flight), the dispatch boundary of impl 1, and
    more than 1,024 chunks"""
    for n in GPU_SIZES:
        for kind in ("bytes", "total_in_2^31..2^32"):
            x, ref = gpu_case(n, kind)
            check(ctx, impl, x, U32, ref=ref, tag=kind)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1_000_003, BOUNDARY - 1])
def test_gpu_lookback_repeated_on_one_context(ctx, n):
    """hundreds of tiles really run at once; five scans of other values each, with a scan of one element in between: a status word of an earlier scan read
    as a current one gives that scan's sum, which is not this one's"""
    base, _ = gpu_case(n, "bytes")
    one = np.array([7], dtype=U32)
    for rep in range(5):
        x = np.roll(base, 977 * rep + 1)
        check(ctx, 1, x, U32, tag=("repetition", rep))
        check(ctx, 1, one, U32, tag=("scan of 1 after repetition", rep))


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [1, 2])
def test_gpu_scan_widening_and_transform(ctx, impl):
    for n in (5000, 1_000_003):
        x, ref = gpu_case(n, "total_above_2^32")
        assert int(ref[n]) > 1 << 32
        check(ctx, impl, x, U64, ref=ref, tag="u32->u64")
    x, ref = gpu_case(1_000_003, "values_above_2^32")
    check(ctx, impl, x, U64, ref=ref, tag="u64->u64")
    x, ref = gpu_case(1_000_003, "digits", 1)
    check(ctx, impl, x, U32, transform=1, ref=ref, tag="labelwidth")


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [1, 2])
def test_gpu_scan_with_skewed_base_pointers(ctx, impl):
    """base + k, as K_annot passes `tile_count + t0`: the 16-byte accesses must be taken only where the address is aligned"""
    for n in (4097, 1_000_003):
        x, ref = gpu_case(n, "bytes")
        for in_skew in range(4):
            for out_skew in range(4):
                check(ctx, impl, x, U32, ref=ref, in_skew=in_skew, out_skew=out_skew)


@pytest.mark.gpu
def test_gpu_scan_in_place(ctx):
    x, ref = gpu_case(1_000_003, "bytes")
    check(ctx, 1, x, U32, ref=ref, in_place=1)
    x, ref = gpu_case(BOUNDARY, "bytes")
    check(ctx, 2, x, U32, ref=ref, in_place=1)


@pytest.mark.gpu
def test_gpu_status_words_over_a_sequence_of_scans_and_the_epoch_reset():
    status_word_sequence(fresh_gpu_ctx)
