"""The pre-pass of a mapper step (k_tile_window) takes the two words that END a tile -- the position of its last record, the CIGAR offset behind it -- from
the neighbouring lane, whose tile starts there, and loads them itself only where no such lane exists.  One submission, against the C oracle:
  * adjacent shards of 1, 63, 64, 65, 256 and 257 tiles of 256 records (the largest: 65,792 records), so that the lane behind a shard's last tile holds
    another shard's first tile, and the tile counts straddle the 64 lanes of a wave and the 256 threads of a pre-pass workgroup -- every shard with its own
    positions and its own het-SNP table, so a word taken from the wrong shard shows in the calls;
  * a shard whose last tile holds one record, full last tiles, and a last tile one record short;
  * a shard in which a tile boundary coincides with a jump of more than MAP_COVER (65,536) bp with more than 512 table entries inside the jump: the tile
    before the jump must fetch its own last position (the guard), or its window would be sized for the far side of the jump;
  * dead shards (no records / no table) between live ones: they own no tiles, so their neighbours' tiles are adjacent in the grid;
  * a third of the records are spliced (M N M), so a tile's CIGAR word count -- the difference of the two offsets -- is not its record count.
Call lists and per-shard counts must equal the oracle's."""
import numpy as np
import pytest
import torch

from helpers import oracle_map_readbatch

pytestmark = pytest.mark.gpu

BASEQ = 10
TR = 256
L = 76
KNOBS = ("PHZ_MAP_BLOCK", "PHZ_MAP_RPT", "PHZ_MAP_ONE_PLANE", "PHZ_MAP_TWO_PLANES", "PHZ_MAP_DBG", "PHZ_MAP_SLOT_CAP", "PHZ_MAP_MERGE_CHUNKS", "PHZ_MAP_WIDE_STAGE")


def _records(rng, pos):
    """synth.ReadBatch of 76-base records at the sorted positions `pos`: two thirds one aligned run, one third a M b N (76 - a) M"""
    from phaser_amd import synth
    n = len(pos)
    spliced = rng.random(n) < 1 / 3
    a = rng.integers(10, L - 10, n)
    intron = rng.integers(50, 400, n)
    nops = np.where(spliced, 3, 1)
    coff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nops, out=coff[1:])
    cig = np.zeros(int(coff[-1]), dtype=np.int64)
    first = coff[:-1]
    cig[first] = np.where(spliced, (a << 4) | 0, (L << 4) | 0)
    cig[first[spliced] + 1] = (intron[spliced] << 4) | 3
    cig[first[spliced] + 2] = ((L - a[spliced]) << 4) | 0
    z = torch.zeros(n, dtype=torch.int32)
    return synth.ReadBatch("chr1", L, torch.from_numpy(pos.astype(np.int32)), z, torch.full((n,), 255, dtype=torch.uint8), z, z, torch.arange(n, dtype=torch.int32),
                           torch.from_numpy(coff), torch.from_numpy(cig), torch.from_numpy(rng.integers(0, 4, (n, L)).astype(np.uint8)),
                           torch.from_numpy(rng.integers(2, 41, (n, L)).astype(np.uint8)))


@pytest.fixture(scope="module")
def batch(oracle_build):
    """-> list of {"host", "vpos", "want", "tiles"}; dead shards have want = None"""
    from phaser_amd import soa
    rng = np.random.default_rng(1701)
    shards = []

    def add(pos, vpos):
        vpos = np.ascontiguousarray(vpos, dtype=np.int32)
        if pos is None or len(vpos) == 0:
            rb = None if pos is None else _records(rng, pos)
            shards.append({"host": soa.pack_readbatch(rb) if rb is not None else soa.pack_sam([]), "vpos": torch.from_numpy(vpos), "want": None, "tiles": 0})
            return
        rb = _records(rng, pos)
        shards.append({"host": soa.pack_readbatch(rb), "vpos": torch.from_numpy(vpos), "tiles": (len(pos) + TR - 1) // TR,
                       "want": oracle_map_readbatch(oracle_build, rb, vpos, BASEQ, with_text=False)})

    def plain(n, origin):                  # n records over 10 n bp from `origin`, het SNPs on a jittered 220-bp grid around them: some 80 calls per tile
        pos = np.sort(rng.integers(origin, origin + 10 * n + 100, n))
        grid = np.arange(origin - 1000, origin + 10 * n + 1500, 220)
        return pos, grid + rng.integers(0, 100, len(grid))

    sizes = [(1, 77), (63, 62 * TR + 1), (64, 64 * TR), (65, 64 * TR + 255), (256, 256 * TR), (257, 257 * TR)]
    assert sizes[-1][1] == 65_792
    for k, (tiles, n) in enumerate(sizes):
        add(*plain(n, 20_000 + 3_000_000 * k + 977 * k))
        assert shards[-1]["tiles"] == tiles
        if k == 1:
            add(None, np.arange(100, 1100, 7))                                   # dead: no records
        if k == 3:
            add(np.sort(rng.integers(5_000, 9_000, 300)), np.zeros(0))          # dead: no table
    # the guard: records 0 .. 255 (the first tile exactly) within 2,000 bp, the other two tiles 200,000 bp further on; 900 table entries inside the jump,
    # more than 65,536 bp beyond the first tile's last record and before the second tile's first, and entries under both groups of records
    near = np.sort(rng.integers(50_000, 52_000, TR))
    far = np.sort(rng.integers(252_000, 257_000, TR + 100))
    inside = 125_000 + 100 * np.arange(900)
    vpos = np.concatenate([50_000 + 40 * np.arange(60), inside, 251_900 + 45 * np.arange(120)])
    assert inside.min() > near.max() + 65_536 + 8 and inside.max() < far.min() and far.min() - near.min() > 65_536 and len(inside) > 512
    add(np.concatenate([near, far]), vpos)
    assert shards[-1]["tiles"] == 3
    live = [s for s in shards if s["want"] is not None]
    assert len(live) == 7 and len(shards) == 9
    assert all(len(s["want"][0]) > 0 for s in live)
    w = live[-1]["want"]
    assert (w[0] < TR).any() and (w[0] >= TR).any() and not np.isin(w[1], np.arange(60, 960)).any()        # calls on both sides of the jump, none inside it
    return shards


def _check(shards, calls):
    for k, (s, c) in enumerate(zip(shards, calls)):
        c = c.cpu()
        if s["want"] is None:
            assert c.n == 0, k
            continue
        o_r, o_v, o_c, _ = s["want"]
        assert c.n == len(o_r), (k, c.n, len(o_r))
        assert np.array_equal(c.read_idx.numpy(), o_r) and np.array_equal(c.var_idx.numpy(), o_v) and np.array_equal(c.code.numpy(), o_c), k


@pytest.mark.parametrize("env", [{}, {"PHZ_MAP_WIDE_STAGE": "1"}], ids=["default", "wide_stage"])
def test_adjacent_shards_vs_oracle(batch, monkeypatch, env):
    from phaser_amd.mapper import Mapper
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = Mapper(0)
    dev = [s["host"].to("cuda") for s in batch]
    _check(batch, m.map_batch(dev, [s["vpos"] for s in batch], BASEQ, aux=False))


def test_shard_order_reversed(batch, monkeypatch):
    """the same shards in reverse order: other shards meet at the wave and workgroup boundaries of the pre-pass"""
    from phaser_amd.mapper import Mapper
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    m = Mapper(0)
    sub = batch[::-1]
    _check(sub, m.map_batch([s["host"].to("cuda") for s in sub], [s["vpos"] for s in sub], BASEQ, aux=False))
