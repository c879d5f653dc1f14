"""K_map's lean walker (walk_lean<D>, phz_leanwalk.h) on designed tiles, against the C oracle.

One shard of "islands" 200,000 bp apart (a tile's window covers 65,536 bp past its last record, so the windows of two islands never overlap), each
island exactly one 256-record tile.  Every kind of tile is laid down twice: once with a staged window of at most 64 entries and once -- 150 more het
SNPs inside the window, under no record -- with 129..512 entries, so that both depth classes of the walk run on the same records.  The kinds:
  ragged     multi-op records of 2..9 ops interleaved, so the lanes of one wave end on different trips; het SNPs under the last run of a 9-op record
             and under the first run of a 2-op one;
  uniform    256 records aM bN cM: two rounds of the record loop, every lane the same trip count (and 768 CIGAR words: the last records are declined
             by the 640 words staged);
  long       more than 64 records of more than 3 ops (the back list spills past one wave), one of them with more than 32 candidates;
  poison     every cause the oracle's front end accepts -- a third insertion, an insertion directly after I / S / H / P or after a zero-length op, a
             run beyond the staged window -- twice each, between clean records over the same het SNPs: a lean candidate wrongly kept or dropped shows
             in the call list;
  inskeys    a het SNP on the last base before an I in the first segment; after an N the key lands seg_start bases further on, in a later run; two
             insertions carried in a later segment; two insertions of a later segment colliding on one key (through a zero-length op: the later wins);
  cigwords   256 records of 5 ops: 1,280 CIGAR words against the 640 staged, the second half of the tile is declined by the walker.
Separate shards of 1, 63, 65 and 129 ragged records end on a partial tile.  The batch runs through the default instantiation, the 256-thread one, the
one-byte-plane one, the profiling one, and -- without the text planes -- the 4-byte and the 8-byte staging form."""
import numpy as np
import pytest
import torch

from helpers import oracle_map_readbatch

pytestmark = pytest.mark.gpu

L = 76
TILE = 256
SPACING = 200_000
FIELD = 100             # an island's het SNPs start this far behind its first record, one every STEP bases
STEP = 12
FILLER = 30_000         # the 150 SNPs that only lengthen the window: inside it, under no record
OP = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}
BASEQ = 10
KNOBS = ("PHZ_MAP_BLOCK", "PHZ_MAP_RPT", "PHZ_MAP_ONE_PLANE", "PHZ_MAP_TWO_PLANES", "PHZ_MAP_DBG", "PHZ_MAP_SLOT_CAP", "PHZ_MAP_MERGE_CHUNKS", "PHZ_MAP_WIDE_STAGE")
NO_CALL = [("M", 10), ("N", 5), ("M", 66)]          # at the island's start it ends before the first het SNP


def read_len(ops):
    return sum(n for o, n in ops if o in "MIS=X")


def split(rng, total, parts, least):
    """total as `parts` integers of at least `least`"""
    cut = np.sort(rng.integers(0, total - parts * least + 1, parts - 1))
    return (np.diff(np.concatenate([[0], cut, [total - parts * least]])) + least).tolist()


def ragged_ops(rng, k):
    """k ops, 2..9: runs separated by N / D / I (at most two I), led by a soft clip when k is even"""
    ops = [("S", 3)] if k % 2 == 0 else []
    n_sep = (k - len(ops) - 1) // 2
    seps, n_ins = [], 0
    for _ in range(n_sep):
        kind = "NNDI"[int(rng.integers(0, 4))]
        if kind == "I" and n_ins == 2: kind = "N"
        n_ins += kind == "I"
        seps.append((kind, int(rng.integers(20, 121)) if kind == "N" else int(rng.integers(1, 4)) if kind == "D" else int(rng.integers(1, 3))))
    runs = split(rng, L - read_len(ops) - sum(n for o, n in seps if o == "I"), n_sep + 1, 4)
    for i, r in enumerate(runs):
        ops.append(("M=X"[int(rng.integers(0, 3))] if rng.integers(0, 5) == 0 else "M", r))
        if i < n_sep: ops.append(seps[i])
    assert len(ops) == k and read_len(ops) == L
    return ops


def spliced(rng):
    a = int(rng.integers(10, L - 10))
    return [("M", a), ("N", int(rng.integers(20, 201))), ("M", L - a)]


def runs_of(pos, ops):
    """[(first, end)] reference spans of the record's M / = / X runs"""
    g = pos; out = []
    for o, n in ops:
        if o in "M=X": out.append((g, g + n))
        if o in "M=XDN": g += n
    return out


def field(k):
    return [FIELD + STEP * i for i in range(k)]


def kind_ragged(rng, n=TILE):
    snps = field(40)
    recs = [(i, NO_CALL, None) for i in range(min(4, n))]
    while len(recs) < n:
        recs.append((int(rng.integers(0, 560)), ragged_ops(rng, 2 + len(recs) % 8), "ragged"))
    return recs, snps


def kind_uniform(rng):
    recs = [(i, NO_CALL, None) for i in range(4)]
    while len(recs) < TILE:
        recs.append((int(rng.integers(0, 560)), spliced(rng), "uniform"))
    return recs, field(40)


def kind_long(rng):
    # 39 het SNPs two bases apart under one 5-op record (its 37 candidates pass the 32 ordinals of a record), ten more further on
    dense = [300 + 2 * i for i in range(39)]
    snps = dense + [FIELD + STEP * i for i in range(10)]
    recs = [(i, NO_CALL, None) for i in range(4)]
    recs.append((300, [("M", 20), ("D", 1), ("M", 20), ("D", 1), ("M", 36)], "long_many"))
    for _ in range(100):
        recs.append((int(rng.integers(0, 330)), ragged_ops(rng, 5 + 2 * int(rng.integers(0, 3))), "long"))
    while len(recs) < TILE:
        recs.append((int(rng.integers(0, 330)), [("M", L)], None))
    return recs, snps


POISON = {
    "third_insertion": [("M", 10), ("I", 1), ("M", 10), ("I", 1), ("M", 10), ("I", 1), ("M", 43)],
    "ins_after_I": [("M", 30), ("I", 1), ("I", 1), ("M", 44)],
    "ins_after_S": [("S", 3), ("I", 2), ("M", 71)],
    "ins_after_H": [("H", 2), ("I", 2), ("M", 74)],
    "ins_after_P": [("M", 30), ("P", 2), ("I", 2), ("M", 44)],
    "ins_after_empty": [("M", 30), ("D", 0), ("I", 2), ("M", 44)],
    "beyond_cover": [("M", 30), ("N", 70_000), ("M", 46)],
}


def kind_poison(rng):
    f = field(40)
    snps = list(f)
    recs = [(i, NO_CALL, None) for i in range(4)]
    for i, (cause, ops) in enumerate(POISON.items()):
        for rep in range(2):
            p = f[3 + 5 * i + 2 * rep] - 3          # a het SNP under the fourth base of the first run
            recs.append((p, ops, cause))
            recs.append((p, spliced(rng), "clean"))
            recs.append((p - 1, [("S", 5), ("M", L - 5)], "clean"))
            if cause == "beyond_cover": snps.append(p + 30 + 70_000 + 5 + rep)          # under the run beyond the window
    while len(recs) < TILE:
        recs.append((int(rng.integers(0, 560)), ragged_ops(rng, 3) if rng.integers(0, 2) else [("M", L)], "clean"))
    return recs, snps


def kind_inskeys(rng):
    f = field(40)
    recs = [(i, NO_CALL, None) for i in range(4)]
    for rep in range(3):
        s = f[5 + 9 * rep]
        a = 20 + rep
        recs.append((s - a + 1, [("M", a), ("I", 2), ("M", L - 2 - a)], "ins_first_segment"))              # the SNP under the last base before the I
        # 5M 10N 10M 2I 59M: the I sits at reference offset 25 of a segment that starts at 15: its key is offset 24 + 15 = 39, inside the last run
        recs.append((f[8 + 9 * rep] - 39, [("M", 5), ("N", 10), ("M", 10), ("I", 2), ("M", 59)], "ins_later_segment"))
        # two carried insertions, keys 39 and 39 + STEP: both under het SNPs of the field
        recs.append((f[6 + 9 * rep] - 39, [("M", 5), ("N", 10), ("M", 10), ("I", 1), ("M", STEP), ("I", 2), ("M", 58 - STEP)], "ins_two_carried"))
        # the two insertions of a later segment on ONE key (a zero-length run between them): the later one is the text
        recs.append((f[7 + 9 * rep] - 39, [("M", 5), ("N", 10), ("M", 10), ("I", 1), ("M", 0), ("I", 2), ("M", 58)], "ins_collide"))
    while len(recs) < TILE:
        recs.append((int(rng.integers(0, 560)), ragged_ops(rng, 3 + 2 * int(rng.integers(0, 2))) if rng.integers(0, 3) else [("M", L)], "clean"))
    return recs, f


def kind_cigwords(rng):
    recs = [(i, NO_CALL, None) for i in range(4)]
    while len(recs) < TILE:
        recs.append((int(rng.integers(0, 560)), ragged_ops(rng, 5), "cigwords"))
    return recs, field(40)


KINDS = [("ragged", kind_ragged), ("uniform", kind_uniform), ("long", kind_long), ("poison", kind_poison), ("inskeys", kind_inskeys), ("cigwords", kind_cigwords)]


def make_shard(oracle_build, rng, islands):
    """islands: [(base, records [(relative pos, ops, tag)], relative het SNPs)] -> the shard, its table, the oracle's calls, the records' tags"""
    from phaser_amd import soa, synth
    recs, snps = [], []
    for base, r, s in islands:
        recs += sorted([(base + p, ops, tag) for p, ops, tag in r], key=lambda x: x[0])
        snps += [base + x for x in s]
    n = len(recs)
    vpos = np.array(sorted(set(snps)), dtype=np.int32)
    pos = np.array([p for p, _, _ in recs], dtype=np.int64)
    assert (np.diff(pos) >= 0).all() and all(read_len(ops) == L for _, ops, _ in recs)
    words = [(ln << 4) | OP[o] for _, ops, _ in recs for o, ln in ops]
    coff = np.zeros(n + 1, np.int64); coff[1:] = np.cumsum([len(ops) for _, ops, _ in recs])
    z = torch.zeros(n, dtype=torch.int32)
    # base qualities on both sides of BASEQ; the records a precondition names keep every base above it, so that their designed calls are calls
    qual = rng.integers(2, 41, (n, L)).astype(np.uint8)
    named = np.array([t in POISON or (t or "").startswith("ins_") for _, _, t in recs])
    qual[named] = rng.integers(20, 41, (int(named.sum()), L)).astype(np.uint8)
    rb = synth.ReadBatch("chr1", L, torch.from_numpy(pos.astype(np.int32)), z, torch.full((n,), 255, dtype=torch.uint8), z, z, torch.arange(n, dtype=torch.int32),
                         torch.from_numpy(coff), torch.tensor(words, dtype=torch.int64),
                         torch.from_numpy(rng.integers(0, 4, (n, L)).astype(np.uint8)), torch.from_numpy(qual))
    want = oracle_map_readbatch(oracle_build, rb, vpos, BASEQ)
    return {"rb": rb, "host": soa.pack_readbatch(rb), "vpos": torch.from_numpy(vpos), "want": want, "recs": recs, "pos": pos, "coff": coff}


@pytest.fixture(scope="module")
def lean_batch(oracle_build):
    """The shards and the oracle's calls, computed once on the CPU; the preconditions are checked here, before any GPU work."""
    rng = np.random.default_rng(2121)
    islands, want_class = [], []
    for _, make in KINDS:
        r, s = make(rng)
        assert len(r) == TILE
        for big in (False, True):
            islands.append((1_000_000 + SPACING * len(islands), r, s + ([FILLER + 10 * i for i in range(150)] if big else [])))
            want_class.append(big)
    main = make_shard(oracle_build, rng, islands)
    n = len(main["recs"])
    assert n == TILE * len(islands)
    pos, vp = main["pos"], main["vpos"].numpy().astype(np.int64)
    o_r, o_v, o_c, o_t = main["want"]
    # the staged window length of every tile, as the pre-pass computes it, falls in the intended depth class
    first = pos[::TILE]; last = pos[TILE - 1::TILE]
    wl = np.searchsorted(vp, last + 65536) - np.searchsorted(vp, first) + 8
    for w, big in zip(wl.tolist(), want_class):
        assert (129 <= w <= 512) if big else w <= 64, (w, big)
    assert (first[1:] - last[:-1] > 65536 + 80_000).all()
    # every tile has records with and without a call
    per_rec = np.bincount(o_r, minlength=n)
    per_tile = per_rec.reshape(len(islands), TILE)
    assert (per_tile > 0).any(axis=1).all() and (per_tile == 0).any(axis=1).all()
    # every category produced an oracle call, in both depth classes
    tags = np.array([t or "" for _, _, t in main["recs"]])
    tile_of = np.arange(n) // TILE
    for big in (False, True):
        sel = np.array(want_class)[tile_of] == big
        for t in sorted(set(tags.tolist()) - {""}):
            assert per_rec[(tags == t) & sel].sum() > 0, (t, big)
    for cause in POISON:
        assert (tags == cause).sum() == 4 and (per_rec[tags == cause] > 0).all(), cause
    for r in np.nonzero(tags == "long_many")[0].tolist():          # more than 32 het SNPs under the runs of that record
        assert sum(int(((vp >= a) & (vp < b)).sum()) for a, b in runs_of(main["recs"][r][0], main["recs"][r][1])) > 32
    assert (tags == "long").sum() == 2 * 100                       # per tile: more than 64 records of more than 3 ops
    assert (o_c == 4).sum() > 20                                                       # inserted text next to a het SNP did occur
    text_of = {(int(r), int(v)): t for r, v, t in zip(o_r, o_v, o_t)}
    for t in ("ins_first_segment", "ins_later_segment", "ins_two_carried", "ins_collide"):
        for r in np.nonzero(tags == t)[0].tolist():
            assert max(len(x) for (rr, _), x in text_of.items() if rr == r) > 1, (t, r)      # the call with inserted text is there
    # ragged: a het SNP under the last run of a 9-op record and under the first run of a 2-op one
    called = set(zip(o_r.tolist(), vp[o_v].tolist()))
    def run_called(r, which):
        p, ops, _ = main["recs"][r]
        a, b = runs_of(p, ops)[which]
        return any((r, x) in called for x in range(a, b))
    rag = np.nonzero(tags == "ragged")[0].tolist()
    assert any(len(main["recs"][r][1]) == 9 and run_called(r, -1) for r in rag) and any(len(main["recs"][r][1]) == 2 and run_called(r, 0) for r in rag)
    # uniform / cigwords: the tile's CIGAR words pass the 640 staged
    for name in ("uniform", "cigwords"):
        k = [i for i, (nm, _) in enumerate(KINDS) if nm == name][0] * 2
        assert main["coff"][(k + 1) * TILE] - main["coff"][k * TILE] > 640
    shards = [main]
    for m in (1, 63, 65, 129):          # partial last tiles
        r, s = kind_ragged(rng, m)
        shards.append(make_shard(oracle_build, rng, [(5_000_000, r, s)]))
        assert len(shards[-1]["recs"]) == m
    assert all(len(s["want"][0]) > 0 for s in shards[2:])
    return shards


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check(shards, calls, aux):
    from phaser_amd.read_variant_map import _allele_text
    lut = "ACGTN"
    for s, c in zip(shards, calls):
        c = c.cpu()
        o_r, o_v, o_c, o_t = s["want"]
        assert c.n == len(o_r)
        assert np.array_equal(c.read_idx.numpy(), o_r) and np.array_equal(c.var_idx.numpy(), o_v) and np.array_equal(c.code.numpy(), o_c)
        if not aux:
            continue
        a0 = c.aux0.numpy().view(np.uint32); a1 = c.aux1.numpy().view(np.uint32)
        rb = s["rb"]
        for k in np.nonzero(o_c >= 4)[0].tolist():          # the inserted-text word of a composite call, through the mapper's own text rule
            r = int(o_r[k])
            seq = "".join(lut[x] for x in rb.seq[r].tolist()); qual = "".join(chr(33 + q) for q in rb.qual[r].tolist())
            assert _allele_text(int(o_c[k]), int(a0[k]), int(a1[k]), seq, qual, BASEQ) == o_t[k]


@pytest.mark.parametrize("env", [{}, {"PHZ_MAP_BLOCK": "256"}, {"PHZ_MAP_ONE_PLANE": "1"}, {"PHZ_MAP_DBG": "4096"}],
                         ids=["default", "block256", "one_plane", "profiling"])
def test_lean_tiles_vs_oracle(lean_batch, monkeypatch, env):
    from phaser_amd.mapper import Mapper
    _env(monkeypatch, env)
    dev = [s["host"].to("cuda") for s in lean_batch]
    calls = Mapper(0).map_batch(dev, [s["vpos"] for s in lean_batch], BASEQ)
    _check(lean_batch, calls, True)


@pytest.mark.parametrize("env,want_narrow", [({}, True), ({"PHZ_MAP_WIDE_STAGE": "1"}, False)], ids=["narrow", "wide"])
def test_lean_tiles_without_text_planes(lean_batch, monkeypatch, env, want_narrow):
    """what the headline step submits (prepare_batch(..., aux=False)): the 4-byte staging word, and the 8-byte record when asked for"""
    from phaser_amd import _lib
    from phaser_amd.mapper import Mapper
    _env(monkeypatch, env)
    m = Mapper(0)
    dev = [s["host"].to("cuda") for s in lean_batch]
    before = m.ctx.counter(_lib.PHZ_C_MAP_NARROW)
    calls = m.map_batch(dev, [s["vpos"] for s in lean_batch], BASEQ, aux=False)
    assert (m.ctx.counter(_lib.PHZ_C_MAP_NARROW) > before) == want_narrow
    _check(lean_batch, calls, False)
