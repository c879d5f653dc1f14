"""The two staging forms of a mapper step -- the 4-byte word (phz_stagepack.h: no shard wants the text planes, at most 256 records per tile, every table at
most 2^20 entries) and the 8-byte record with its side planes -- against the C oracle and against each other.  Which form a submission took is read from
the context's PHZ_C_MAP_NARROW counter.
  * the mixed batch of tests/test_gpu_mapper_step.py (shards of 1, 255, 256, 257 and 513 records between dead ones): narrow by default, wide with
    PHZ_MAP_WIDE_STAGE=1, the two call lists equal;
  * the same with staging slots of 8 calls (most tiles take a stretch of the overflow area), and that file's 1,173-tile batch with slots of 8, where the
    first attempt outgrows the overflow area and the submission is redone once -- in both forms;
  * 256-thread workgroups (512 records per tile: the record number does not fit the word): wide;
  * one shard of the batch asks for the text planes, the others do not: wide, and that shard's planes are right;
  * a table of exactly 2^20 entries with a call on variant 2^20 - 1: narrow; one of 2^20 + 1 entries with a call on variant 2^20: wide;
  * a tile of spliced records over a dense table, whose candidates overflow the tile's LDS buffer: the in-lane fallback stages its calls itself, in both forms."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import oracle_map_readbatch
from test_gpu_mapper_step import mixed, many_tiles, _check      # noqa: F401  (the fixtures and the checker of the mixed-batch tests)

pytestmark = pytest.mark.gpu

BASEQ = 10
L = 76
KNOBS = ("PHZ_MAP_BLOCK", "PHZ_MAP_RPT", "PHZ_MAP_ONE_PLANE", "PHZ_MAP_TWO_PLANES", "PHZ_MAP_DBG", "PHZ_MAP_SLOT_CAP", "PHZ_MAP_MERGE_CHUNKS", "PHZ_MAP_WIDE_STAGE")


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _narrow_count(m):
    from phaser_amd import _lib
    return m.ctx.counter(_lib.PHZ_C_MAP_NARROW)


def _run(shards, env, monkeypatch, want_narrow, aux=False, reps=1):
    """one Mapper per run (the slot size is fixed at a context's first submission); -> the calls of the last submission, on the host"""
    from phaser_amd.mapper import Mapper
    _env(monkeypatch, env)
    m = Mapper(0)
    dev = [s["host"].to("cuda") for s in shards]
    for _ in range(reps):
        before = _narrow_count(m)
        calls = m.map_batch(dev, [s["vpos"] for s in shards], BASEQ, aux=aux)
        assert (_narrow_count(m) > before) == want_narrow
        _check(shards, calls, aux)
    return [c.cpu() for c in calls]


def _same(a, b):
    for x, y in zip(a, b):
        assert x.n == y.n
        assert torch.equal(x.read_idx, y.read_idx) and torch.equal(x.var_idx, y.var_idx) and torch.equal(x.code, y.code)


@pytest.mark.parametrize("slots", [{}, {"PHZ_MAP_SLOT_CAP": "8"}], ids=["default_slots", "slots_of_8"])
def test_mixed_batch_narrow_and_wide(mixed, monkeypatch, slots):
    narrow = _run(mixed, dict(slots), monkeypatch, True)
    wide = _run(mixed, dict(slots, PHZ_MAP_WIDE_STAGE="1"), monkeypatch, False)
    _same(narrow, wide)


@pytest.mark.parametrize("form", [{}, {"PHZ_MAP_WIDE_STAGE": "1"}], ids=["narrow", "wide"])
def test_overflow_area_redo(many_tiles, monkeypatch, form):
    """slots of 8 calls over 1,173 tiles: the first submission is redone with a larger overflow area, the second finds it in place"""
    _run(many_tiles, dict(form, PHZ_MAP_SLOT_CAP="8"), monkeypatch, not form, reps=2)


def test_block256_takes_the_wide_form(mixed, monkeypatch):
    _run(mixed, {"PHZ_MAP_BLOCK": "256"}, monkeypatch, False)


def test_text_planes_keep_the_wide_form(mixed, monkeypatch):
    _run(mixed, {}, monkeypatch, False, aux=True)


def test_one_shard_with_text_planes(mixed, monkeypatch):
    """phz_map_reads_batch with the two text planes for ONE shard of the batch: the submission takes the wide form and the planes of that shard are right"""
    from phaser_amd import _lib
    from phaser_amd.mapper import Mapper, Calls, _ptr
    _env(monkeypatch, {})
    m = Mapper(0)
    live = [k for k, s in enumerate(mixed) if s["want"] is not None and (s["want"][2] == 4).any()]
    assert live, "the mixed batch has a shard with a text call"
    pick = max(live, key=lambda k: int((mixed[k]["want"][2] == 4).sum()))
    n = len(mixed)
    dev = [s["host"].to("cuda") for s in mixed]
    R = (_lib.phz_reads * n)(); V = (_lib.phz_variants * n)(); O = (_lib.phz_calls * n)(); N = (C.c_int64 * n)()
    keep, bufs = [], []
    for i, (sh, s) in enumerate(zip(dev, mixed)):
        vp = s["vpos"].to("cuda").to(torch.int32).contiguous(); keep.append(vp)
        R[i] = _lib.phz_reads(sh.n, int(sh.cigar.numel()), int(sh.seq2.numel()), _ptr(sh.pos), _ptr(sh.cigar_off), _ptr(sh.cigar), _ptr(sh.seq_off), _ptr(sh.seq2),
                              _ptr(sh.qual), None)
        V[i] = _lib.phz_variants(int(vp.numel()), _ptr(vp), None)
        cap = 2 * sh.n + 4096
        b = [torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.uint8, device="cuda")]
        b += [torch.full((cap,), -1, dtype=torch.int32, device="cuda"), torch.full((cap,), -1, dtype=torch.int32, device="cuda")] if i == pick else [None, None]
        bufs.append(b)
        O[i] = _lib.phz_calls(cap, *[_ptr(t) for t in b])
    torch.cuda.synchronize()
    before = _narrow_count(m)
    m.ctx.check(m.ctx.lib.phz_map_reads_batch(m.ctx.h, n, R, V, BASEQ, O, N))
    assert _narrow_count(m) == before
    calls = [Calls(*[None if t is None else t[:int(N[i])] for t in bufs[i]]) for i in range(n)]
    _check([mixed[pick]], [calls[pick]], True)
    rest = [i for i in range(n) if i != pick]
    _check([mixed[i] for i in rest], [calls[i] for i in rest], False)


def _single_run_records(rng, pos):
    from phaser_amd import synth
    n = len(pos)
    z = torch.zeros(n, dtype=torch.int32)
    return synth.ReadBatch("chr1", L, torch.from_numpy(pos.astype(np.int32)), z, torch.full((n,), 255, dtype=torch.uint8), z, z, torch.arange(n, dtype=torch.int32),
                           torch.arange(n + 1, dtype=torch.int64), torch.full((n,), (L << 4) | 0, dtype=torch.int64),
                           torch.from_numpy(rng.integers(0, 4, (n, L)).astype(np.uint8)), torch.from_numpy(rng.integers(20, 41, (n, L)).astype(np.uint8)))


@pytest.mark.parametrize("extra,want_narrow", [(0, True), (1, False)], ids=["2^20_entries", "2^20+1_entries"])
def test_table_at_the_variant_field_limit(oracle_build, monkeypatch, extra, want_narrow):
    """300 records (two tiles) over the last entries of a table with a het SNP every 20 bp: the last entry of the table gets calls"""
    from phaser_amd import soa
    rng = np.random.default_rng(1720 + extra)
    nv = (1 << 20) + extra
    vpos = (1_000 + 20 * np.arange(nv)).astype(np.int32)
    last = int(vpos[-1])
    pos = np.sort(rng.integers(last - 400, last + 30, 300))
    rb = _single_run_records(rng, pos)
    want = oracle_map_readbatch(oracle_build, rb, vpos, BASEQ, with_text=False)
    assert int(want[1].max()) == nv - 1 and (want[1] == nv - 1).sum() > 20 and len(want[0]) > 300
    shards = [{"rb": rb, "host": soa.pack_readbatch(rb), "vpos": torch.from_numpy(vpos), "want": want}]
    _run(shards, {}, monkeypatch, want_narrow)


@pytest.mark.parametrize("form", [{}, {"PHZ_MAP_WIDE_STAGE": "1"}], ids=["narrow", "wide"])
def test_candidate_buffer_overflow_fallback(oracle_build, monkeypatch, form):
    """600 spliced records (30M 200N 46M) within 600 bp over a het SNP every 9 bp: some 8 candidates per record, far beyond the 192 a tile's LDS buffer holds,
    so every full tile counts and stages its multi-op records in-lane (walk_read<1> / <2>)"""
    from phaser_amd import soa, synth
    rng = np.random.default_rng(1731)
    n = 600
    pos = np.sort(rng.integers(10_000, 10_600, n))
    z = torch.zeros(n, dtype=torch.int32)
    cig = np.tile(np.array([(30 << 4) | 0, (200 << 4) | 3, (46 << 4) | 0], dtype=np.int64), n)
    rb = synth.ReadBatch("chr1", L, torch.from_numpy(pos.astype(np.int32)), z, torch.full((n,), 255, dtype=torch.uint8), z, z, torch.arange(n, dtype=torch.int32),
                         3 * torch.arange(n + 1, dtype=torch.int64), torch.from_numpy(cig),
                         torch.from_numpy(rng.integers(0, 4, (n, L)).astype(np.uint8)), torch.from_numpy(rng.integers(2, 41, (n, L)).astype(np.uint8)))
    vpos = (9_900 + 9 * np.arange(140)).astype(np.int32)
    want = oracle_map_readbatch(oracle_build, rb, vpos, BASEQ, with_text=False)
    per_tile = np.bincount(want[0] // 256, minlength=3)
    assert per_tile[0] > 192 * 4 and per_tile[1] > 192 * 4
    shards = [{"rb": rb, "host": soa.pack_readbatch(rb), "vpos": torch.from_numpy(vpos), "want": want}]
    _run(shards, dict(form), monkeypatch, not form)
