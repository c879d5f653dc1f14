"""The kernels around k_map in one phz_map_reads_batch step -- the pre-pass's window search (k_tile_window), the totals kernel that also writes the
words the host reads (k_chunk_base; k_shard_totals behind it for very large submissions) and k_compact -- against the C oracle:
  * a mixed batch: shards of 1, 255, 256, 257 and 513 records between dead shards, het-SNP tables of 1, 2, 8, 9, 10, 80, 81, 82 and 730 entries, a shard whose records all lie before the first SNP, one whose records all lie behind the last, one whose table ends
    fewer than 8 entries behind the window start of its last tile; with and without the text planes, with 256-thread workgroups, with the one-byte plane and
    with the profiling instantiation;
  * a submission of more than 1,024 tiles (two chunks of the tile scan) over three shards whose boundaries fall inside a chunk: per-shard counts and lists;
  * the same with staging slots of 8 calls: the tiles ask for more than the overflow area's first size, so the cursor the host reads through the same
    words makes it redo the submission once with a larger area -- on both totals paths (a cursor word not written, or stale, fails the lists);
  * two submissions in a row on one ctx with different shard sets."""
import numpy as np
import pytest
import torch

from helpers import oracle_map_readbatch

pytestmark = pytest.mark.gpu

BASEQ = 10
KNOBS = ("PHZ_MAP_BLOCK", "PHZ_MAP_RPT", "PHZ_MAP_ONE_PLANE", "PHZ_MAP_TWO_PLANES", "PHZ_MAP_DBG", "PHZ_MAP_SLOT_CAP", "PHZ_MAP_MERGE_CHUNKS")


def _clean_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _take(rb, lo, n):
    keep = torch.zeros(len(rb), dtype=torch.bool)
    keep[lo:lo + n] = True
    return rb.select(keep)


@pytest.fixture(scope="module")
def mixed(oracle_build):
    """-> list of {"rb", "host", "vpos", "want"}; dead shards have want = None"""
    from phaser_amd import soa, synth
    v, gs, ge, w = synth.make_variants("chr1", 1, 5_000_000, 3000, 811, n_genes=40)
    rb = synth.make_reads(v, gs, ge, w, 5000, 812, n_rate=0.002)
    rb = rb.select(synth.samtools_keep(rb, 255))
    rb = rb.select(rb.pos > 5000)
    assert len(rb) > 6000
    vp = v.pos.numpy().astype(np.int32)
    pos = rb.pos.numpy()
    sizes = [1, 255, 256, 257, 513]
    shards = []

    def add(recs, table):
        table = np.ascontiguousarray(table, dtype=np.int32)
        host = soa.pack_readbatch(recs) if recs is not None else soa.pack_sam([])
        live = recs is not None and len(table) > 0
        shards.append({"rb": recs, "host": host, "vpos": torch.from_numpy(table),
                       "want": oracle_map_readbatch(oracle_build, recs, table, BASEQ) if live else None})

    def table_at(p0, k):                    # k consecutive entries of the table, starting just below position p0 where the table allows
        i0 = max(0, min(int(np.searchsorted(vp, p0)) - 1, len(vp) - k))
        return vp[i0:i0 + k]
    for t, k in enumerate([1, 2, 8, 9, 10, 80, 81, 82, 730]):
        n = sizes[t % len(sizes)]
        lo = 400 * t
        add(_take(rb, lo, n), table_at(pos[lo], k))
        if t == 2:
            add(None, vp[:10])                                          # dead: no records
        if t == 5:
            add(_take(rb, 100, 300), vp[:0])                            # dead: no variants
    lo = 4000
    recs = _take(rb, lo, 513)
    add(recs, int(recs.pos.max()) + 100_000 + 37 * np.arange(9))        # every record before the first SNP
    add(_take(rb, lo + 600, 257), 1 + 3 * np.arange(81))                # every record behind the last SNP (positions start above 5,000)
    add(None, vp[:0])                                                   # dead: neither
    recs = _take(rb, lo + 1000, 513)                                    # the table ends 3 entries behind the window start of the last tile (records 512 ..)
    w0 = int(np.searchsorted(vp, int(recs.pos[512])))
    assert 100 < w0 < len(vp) - 3
    add(recs, vp[:w0 + 3])
    live = [s for s in shards if s["want"] is not None]
    assert len(live) == 12 and len(shards) == 15
    assert sum(len(s["want"][0]) > 0 for s in live) >= 8 and len(live[9]["want"][0]) == 0 and len(live[10]["want"][0]) == 0
    return shards


def _check(shards, calls, aux):
    from phaser_amd.read_variant_map import _allele_text
    lut = "ACGTN"
    for k, (s, c) in enumerate(zip(shards, calls)):
        c = c.cpu()
        if s["want"] is None:
            assert c.n == 0, k
            continue
        o_r, o_v, o_c, o_t = s["want"]
        assert c.n == len(o_r), k
        assert np.array_equal(c.read_idx.numpy(), o_r) and np.array_equal(c.var_idx.numpy(), o_v) and np.array_equal(c.code.numpy(), o_c), k
        if not aux:
            assert c.aux0 is None and c.aux1 is None
            continue
        a0 = c.aux0.numpy().view(np.uint32); a1 = c.aux1.numpy().view(np.uint32)
        rb = s["rb"]
        for j in np.nonzero(o_c == 4)[0].tolist():
            r = int(o_r[j])
            seq = "".join(lut[x] for x in rb.seq[r].tolist()); qual = "".join(chr(33 + q) for q in rb.qual[r].tolist())
            assert _allele_text(4, int(a0[j]), int(a1[j]), seq, qual, BASEQ) == o_t[j], (k, j)


@pytest.mark.parametrize("env,aux", [({}, True), ({}, False), ({"PHZ_MAP_BLOCK": "256"}, True), ({"PHZ_MAP_ONE_PLANE": "1"}, False), ({"PHZ_MAP_DBG": "4096"}, True)],
                         ids=["text_planes", "lean", "block256", "one_plane", "profiling"])
def test_mixed_batch_vs_oracle(mixed, monkeypatch, env, aux):
    from phaser_amd import soa
    from phaser_amd.mapper import Mapper
    _clean_env(monkeypatch, env)
    dev = [s["host"].to("cuda") for s in mixed]
    if "PHZ_MAP_ONE_PLANE" in env:
        assert all(soa.bq_plane(d) is not None for d, s in zip(dev, mixed) if s["rb"] is not None)
    m = Mapper(0)
    _check(mixed, m.map_batch(dev, [s["vpos"] for s in mixed], BASEQ, aux=aux), aux)


def test_changed_shard_sets_on_one_ctx(mixed, monkeypatch):
    """the second submission has other shards, fewer of them and another tile count: nothing of the first (table, totals, host words) may show in it"""
    from phaser_amd.mapper import Mapper
    _clean_env(monkeypatch, {})
    m = Mapper(0)
    dev = [s["host"].to("cuda") for s in mixed]
    for pick in (list(range(len(mixed))), [14, 3, 9, 0], [1], list(range(len(mixed) - 1, -1, -1))):
        sub = [mixed[i] for i in pick]
        _check(sub, m.map_batch([dev[i] for i in pick], [s["vpos"] for s in sub], BASEQ, aux=False), False)


@pytest.fixture(scope="module")
def many_tiles(oracle_build):
    """three shards of 150,000 / 130,000 / 20,100 single-run records: 586 + 508 + 79 tiles of 256 records, so the second shard crosses the boundary between
    the two 1,024-tile chunks and the third starts inside the second chunk"""
    from phaser_amd import soa, synth
    rng = np.random.default_rng(821)
    L = 76
    out = []
    for n, span in ((150_000, 1_500_000), (130_000, 1_300_000), (20_100, 200_000)):
        pos = np.sort(rng.integers(10_000, 10_000 + span, n)).astype(np.int32)
        grid = np.arange(9_000, 11_000 + span, 220)                      # het SNPs on a jittered grid: about 70 calls in every tile, never 128
        vpos = (grid + rng.integers(0, 100, len(grid))).astype(np.int32)
        z = torch.zeros(n, dtype=torch.int32)
        rb = synth.ReadBatch("chr1", L, torch.from_numpy(pos), z, torch.full((n,), 255, dtype=torch.uint8), z, z, torch.arange(n, dtype=torch.int32),
                             torch.arange(n + 1, dtype=torch.int64), torch.full((n,), (L << 4) | 0, dtype=torch.int64),
                             torch.from_numpy(rng.integers(0, 4, (n, L)).astype(np.uint8)), torch.from_numpy(rng.integers(2, 41, (n, L)).astype(np.uint8)))
        out.append({"rb": rb, "host": soa.pack_readbatch(rb), "vpos": torch.from_numpy(vpos), "want": oracle_map_readbatch(oracle_build, rb, vpos, BASEQ, with_text=False)})
    tiles = [(len(s["rb"]) + 255) // 256 for s in out]
    assert sum(tiles) > 1024 and tiles[0] < 1024 < tiles[0] + tiles[1] and (tiles[0] + tiles[1]) % 1024 != 0
    per_tile = np.concatenate([np.bincount(s["want"][0] // 256, minlength=t) for s, t in zip(out, tiles)])
    assert per_tile.max() < 128                                        # no tile fills the default slot (half a tile's records) ...
    # ... but with slots of 8 calls the tiles above 8 ask for more than the overflow area's first size (its floor of 65,536 slots: a quarter of
    # 1,173 x 8 slots is less), so the first attempt ends with the cursor beyond the area and the submission is redone with a larger one
    assert per_tile[per_tile > 8].sum() > 65_536 + 4_096
    return out


@pytest.mark.parametrize("env", [{}, {"PHZ_MAP_SLOT_CAP": "8"}, {"PHZ_MAP_MERGE_CHUNKS": "1"}, {"PHZ_MAP_MERGE_CHUNKS": "1", "PHZ_MAP_SLOT_CAP": "8"}],
                         ids=["default_slots", "slots_of_8", "separate_totals_launch", "separate_totals_launch_slots_of_8"])
def test_many_tiles_three_shards(many_tiles, monkeypatch, env):
    """PHZ_MAP_MERGE_CHUNKS=1: the per-shard totals and the host's words come from k_shard_totals, the path of a submission beyond a million tiles"""
    from phaser_amd.mapper import Mapper
    _clean_env(monkeypatch, env)
    m = Mapper(0)                                           # its own context: the slot size is fixed at a context's first submission
    dev = [s["host"].to("cuda") for s in many_tiles]
    for rep in range(2):                                    # slots of 8: the first submission is redone with a larger overflow area, the second finds it in place
        _check(many_tiles, m.map_batch(dev, [s["vpos"] for s in many_tiles], BASEQ, aux=False), False)
