"""K_map at the smallest shapes where a tile's staging loads (one bounds-checked descriptor per slice: phz_stageload.h), its cigar_off end word taken from
the pre-pass, and its flush into the tile's slot or a stretch of the overflow area can go wrong, through phz_map_reads_batch against the C oracle.  Every
batch runs in four forms: the 4-byte staging word (default), the 8-byte record (PHZ_MAP_WIDE_STAGE=1), the one-byte plane (PHZ_MAP_ONE_PLANE=1) and the
text planes (aux).
  * partial tiles: shards of 1, 2, 255, 256, 257 and 513 records, each ending in a spliced record with a het SNP under its last run; three shards of such
    sizes around one of 0 records;
  * the window against the end of the table: tables of 1, 7, 8, 9 and 130 entries that end 1 .. 8 entries before the staged window does, and the same tables
    with every record behind the last entry (window start == table size); windows of 127, 128, 129, 511 and 512 entries whose last 8 are padding, and a
    truncated one (more than 512 entries in reach);
  * CIGAR words per tile: 256 (all single-op), 383, 384, 385 (where the three unrolled rounds end), 639, 640, 641 (the LDS cap and one beyond), and a record
    of 799 words; the first and the last record of every such tile have a het SNP under them, and the last record of a tile is a spliced one;
  * the flush: single-run records over 1, 2 and 8 het SNPs with the first, a middle and the last base masked by the base-quality limit; tiles of exactly
    slot_cap - 1, slot_cap and slot_cap + 1 calls (slots of 8), each followed by an ordinary tile; single-run and spliced records alternating in one tile;
  * the lists of PHZ_MAP_MERGE_CHUNKS=1 and of the default equal each other."""
import numpy as np
import pytest
import torch

from helpers import oracle_map_readbatch

pytestmark = pytest.mark.gpu

BASEQ = 10
TILE = 256
COVER = 65536
SLACK = 8
OP = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4}
KNOBS = ("PHZ_MAP_BLOCK", "PHZ_MAP_RPT", "PHZ_MAP_ONE_PLANE", "PHZ_MAP_TWO_PLANES", "PHZ_MAP_DBG", "PHZ_MAP_SLOT_CAP", "PHZ_MAP_MERGE_CHUNKS", "PHZ_MAP_WIDE_STAGE")
FORMS = {"narrow": ({}, False), "wide": ({"PHZ_MAP_WIDE_STAGE": "1"}, False), "one_plane": ({"PHZ_MAP_ONE_PLANE": "1"}, False), "text_planes": ({}, True)}
form = pytest.mark.parametrize("form", list(FORMS))


def read_offset(ops, pos, p):
    """offset in the read of the base aligned to reference position p (None: no aligned base)"""
    g = pos; r = 0
    for o, n in ops:
        if o == "M":
            if g <= p < g + n: return r + (p - g)
            g += n; r += n
        elif o in "IS": r += n
        else: g += n
    return None


def make_shard(oracle_build, recs, snps, rng, L=76, qual=None):
    """recs: [(pos, [(op, len), ...])] sorted by position, every read L bases; snps: het-SNP positions; qual: [n, L] phred (default: 2 .. 40 at random)
    -> {"recs", "rb", "host", "vpos", "want"} with the oracle's calls (computed once, on the CPU)"""
    from phaser_amd import soa, synth
    n = len(recs)
    assert all(sum(k for o, k in ops if o in "MIS") == L and all(k > 0 for _, k in ops) for _, ops in recs)
    pos = np.array([p for p, _ in recs], dtype=np.int64)
    assert (np.diff(pos) >= 0).all()
    words = [(k << 4) | OP[o] for _, ops in recs for o, k in ops]
    coff = np.zeros(n + 1, np.int64); coff[1:] = np.cumsum([len(ops) for _, ops in recs])
    z = torch.zeros(n, dtype=torch.int32)
    if qual is None:
        qual = rng.integers(2, 41, (n, L))
    rb = synth.ReadBatch("chr1", L, torch.from_numpy(pos.astype(np.int32)), z, torch.full((n,), 255, dtype=torch.uint8), z, z, torch.arange(n, dtype=torch.int32),
                         torch.from_numpy(coff), torch.tensor(words, dtype=torch.int64),
                         torch.from_numpy(rng.integers(0, 4, (n, L)).astype(np.uint8)), torch.from_numpy(np.asarray(qual).astype(np.uint8)))
    vpos = np.array(sorted(set(int(x) for x in snps)), dtype=np.int32)
    assert len(vpos) == len(snps)
    return {"recs": recs, "rb": rb, "host": soa.pack_readbatch(rb), "vpos": torch.from_numpy(vpos), "want": oracle_map_readbatch(oracle_build, rb, vpos, BASEQ)}


def dead_shard():
    from phaser_amd import soa
    return {"recs": [], "rb": None, "host": soa.pack_sam([]), "vpos": torch.from_numpy(np.arange(10, 20, dtype=np.int32)), "want": None}


def window_of(shard, tile):
    """(window start, staged length before truncation) of a tile, as the pre-pass computes them"""
    pos = shard["rb"].pos.numpy(); vp = shard["vpos"].numpy()
    first = int(pos[tile * TILE]); last = int(pos[min(len(pos), (tile + 1) * TILE) - 1])
    lo = int(np.searchsorted(vp, first)); lo2 = int(np.searchsorted(vp, last + COVER))
    return lo, lo2 - lo + SLACK


def run(shards, monkeypatch, form_name, extra=None):
    """one Mapper per run (a context fixes its slot size at its first submission) -> the calls of every shard, on the host"""
    from phaser_amd import soa
    from phaser_amd.mapper import Mapper
    env, aux = FORMS[form_name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env, **(extra or {})).items():
        monkeypatch.setenv(k, v)
    dev = [s["host"].to("cuda") for s in shards]
    if "PHZ_MAP_ONE_PLANE" in env:
        assert all(soa.bq_plane(d) is not None for d, s in zip(dev, shards) if s["rb"] is not None)
    return [c.cpu() for c in Mapper(0).map_batch(dev, [s["vpos"] for s in shards], BASEQ, aux=aux)], aux


def check(shards, calls, aux):
    """exact equality with the oracle: counts, (read, variant, code) and -- with the text planes -- the read offset of a plain call and the text of a composite one"""
    from phaser_amd.read_variant_map import _allele_text
    lut = "ACGTN"
    for k, (s, c) in enumerate(zip(shards, calls)):
        if s["want"] is None:
            assert c.n == 0, k
            continue
        o_r, o_v, o_c, o_t = s["want"]
        assert c.n == len(o_r), (k, c.n, len(o_r))
        assert np.array_equal(c.read_idx.numpy(), o_r) and np.array_equal(c.var_idx.numpy(), o_v) and np.array_equal(c.code.numpy(), o_c), k
        if not aux:
            continue
        a0 = c.aux0.numpy().view(np.uint32); a1 = c.aux1.numpy().view(np.uint32)
        recs = s["recs"]; vp = s["vpos"].numpy(); rb = s["rb"]
        plain = o_c < 4
        want0 = np.array([read_offset(recs[r][1], recs[r][0], int(vp[v])) if p else 0 for r, v, p in zip(o_r.tolist(), o_v.tolist(), plain.tolist())], dtype=np.int64)
        assert np.array_equal(a0[plain].astype(np.int64), want0[plain]) and not a1[plain].any(), k
        for j in np.nonzero(~plain)[0].tolist():
            r = int(o_r[j])
            seq = "".join(lut[x] for x in rb.seq[r].tolist()); qual = "".join(chr(33 + q) for q in rb.qual[r].tolist())
            assert _allele_text(int(o_c[j]), int(a0[j]), int(a1[j]), seq, qual, BASEQ) == o_t[j], (k, j)


def same_lists(a, b):
    for x, y in zip(a, b):
        assert x.n == y.n and torch.equal(x.read_idx, y.read_idx) and torch.equal(x.var_idx, y.var_idx) and torch.equal(x.code, y.code)


def spliced(rng, L=76):
    a = int(rng.integers(10, L - 30))
    return [("M", a), ("N", int(rng.integers(20, 300))), ("M", L - a)]


def mixed_record(rng, i, L=76):
    kind = i % 5
    if kind in (0, 1): return [("M", L)]
    if kind == 2: return spliced(rng, L)
    if kind == 3: return [("S", 5), ("M", L - 5)]
    a = int(rng.integers(5, L - 10))
    return [("M", a), ("I", 2), ("M", L - 2 - a)] if i % 2 else [("M", a), ("D", 3), ("M", L - a)]


# ---------------------------------------------------------------------------------------------------------------- partial tiles
def partial_shard(oracle_build, rng, n, base):
    """n records 7 bp apart over a het SNP every 11 bp; the last record is 30M 100N 46M with a het SNP under its last run"""
    recs = [(base + 7 * i, mixed_record(rng, i)) for i in range(n - 1)]
    last = base + 7 * (n - 1)
    recs.append((last, [("M", 30), ("N", 100), ("M", 46)]))
    snps = list(range(base - 40, last + 400, 11))
    s = make_shard(oracle_build, recs, snps, rng, qual=rng.integers(20, 41, (n, 76)))
    o_r, o_v, o_c, _ = s["want"]
    under_last_run = [int(s["vpos"][v]) >= last + 130 for r, v in zip(o_r.tolist(), o_v.tolist()) if r == n - 1]
    assert any(under_last_run), "the last record has a call in its last run"
    return s


@pytest.fixture(scope="module")
def partial(oracle_build):
    rng = np.random.default_rng(2201)
    return {n: partial_shard(oracle_build, rng, n, 10_000 + 1_000 * k) for k, n in enumerate([1, 2, 255, 256, 257, 513])}


@form
def test_partial_tiles(partial, monkeypatch, form):
    shards = list(partial.values())
    calls, aux = run(shards, monkeypatch, form)
    check(shards, calls, aux)
    three = [partial[257], dead_shard(), partial[1], partial[513]]       # sizes mixed around a shard of no records
    calls, aux = run(three, monkeypatch, form)
    check(three, calls, aux)
    for s in (partial[2], partial[256]):                                 # and each alone: its last tile is the submission's last
        calls, aux = run([s], monkeypatch, form)
        check([s], calls, aux)


# ------------------------------------------------------------------------------------------- the window against the table's end
@pytest.fixture(scope="module")
def table_ends(oracle_build):
    """one single-tile shard per (table size, entries the staged window runs past the table): 40 records at 50_000 .. over `near` entries 9 bp apart, then
    `far` entries beyond the window's reach (first record + COVER and more): the window is near + 8 long and the table has near + far entries from its start"""
    rng = np.random.default_rng(2202)
    shards, past = [], []
    for nv in (1, 7, 8, 9, 130):
        for over in range(1, SLACK + 1):
            far = SLACK - over
            near = nv - far
            if near < 0:
                continue
            recs = [(50_000 + 3 * i, mixed_record(rng, i)) for i in range(40)]
            snps = [50_010 + 9 * i for i in range(near)] + [50_000 + 40 * 3 + COVER + 1_000 + 13 * i for i in range(far)]
            s = make_shard(oracle_build, recs, snps, rng)
            w0, wlen = window_of(s, 0)
            assert w0 == 0 and w0 + wlen - nv == over and len(s["vpos"]) == nv
            shards.append(s); past.append(over)
        # every record behind the last entry: the window starts at the table's end
        recs = [(900_000 + 3 * i, mixed_record(rng, i)) for i in range(40)]
        s = make_shard(oracle_build, recs, [1_000 + 9 * i for i in range(nv)], rng)
        assert window_of(s, 0) == (nv, SLACK) and len(s["want"][0]) == 0
        shards.append(s)
    assert sorted(set(past)) == list(range(1, SLACK + 1)) and sum(len(s["want"][0]) > 0 for s in shards) >= 20
    return shards


@form
def test_window_runs_past_the_table(table_ends, monkeypatch, form):
    calls, aux = run(table_ends, monkeypatch, form)
    check(table_ends, calls, aux)


@pytest.fixture(scope="module")
def padded_windows(oracle_build):
    """one full tile per window length over a table that ends with the tile's last reachable entry: the window's last 8 entries are padding; 520 entries in
    reach give the truncated window (512 staged, the LDS walkers off)"""
    rng = np.random.default_rng(2203)
    shards = []
    for wlen in (127, 128, 129, 511, 512, 520 + SLACK):
        near = wlen - SLACK
        base = 100_000
        span = 10 * near                                    # an entry every 10 bp: at most 8 under a 76M record, which so stays a fast record
        pos = np.sort(np.concatenate([[base, base + span + 60, base + span + 99], rng.integers(base, base + span + 100, TILE - 3)]))
        recs = [(int(p), mixed_record(rng, 2 + i // 16) if i % 16 == 5 else [("M", 76)]) for i, p in enumerate(pos.tolist())]
        s = make_shard(oracle_build, recs, [base + 20 + 10 * i for i in range(near)], rng)
        assert window_of(s, 0) == (0, wlen) and len(s["vpos"]) == near and len(s["want"][0]) > 200
        # records behind the last entry probe the padding only: none of them has a call
        behind = [r for r, (p, _) in enumerate(recs) if p > base + 20 + 10 * (near - 1)]
        assert behind and not np.isin(s["want"][0], behind).any()
        shards.append(s)
    return shards


@form
def test_windows_ending_in_padding(padded_windows, monkeypatch, form):
    calls, aux = run(padded_windows, monkeypatch, form)
    check(padded_windows, calls, aux)


# ------------------------------------------------------------------------------------------------------ CIGAR words per tile
def words_tile(rng, base, n_words):
    """256 records, n_words CIGAR words: spliced records (3 words) and at most one 5S71M (2 words) among 76M; the last record is spliced, 3 bp apart"""
    extra = n_words - TILE
    three, two = extra // 2, extra % 2
    kinds = ["M"] * TILE
    if three:
        kinds[TILE - 1] = "N"
        for i in rng.choice(np.arange(1, TILE - 1), three - 1, replace=False).tolist():
            kinds[i] = "N"
    if two:
        kinds[[i for i in range(1, TILE - 1) if kinds[i] == "M"][0]] = "S"
    recs = []
    for i, k in enumerate(kinds):
        ops = [("M", 76)] if k == "M" else [("S", 5), ("M", 71)] if k == "S" else [("M", 30), ("N", 50 + (i % 7)), ("M", 46)]
        recs.append((base + 3 * i, ops))
    assert sum(len(ops) for _, ops in recs) == n_words
    return recs


@pytest.fixture(scope="module")
def cigar_words(oracle_build):
    rng = np.random.default_rng(2204)
    counts = [256, 383, 384, 385, 639, 640, 641]
    recs, snps = [], []
    for t, w in enumerate(counts):
        base = 1_000_000 + 200_000 * t                       # islands: the windows of two tiles do not overlap
        tile = words_tile(rng, base, w)
        recs += tile
        last = tile[-1][0]
        # an entry every 97 bp (a spliced record has one candidate or none: the tile's candidates fit its LDS buffer of 192), one under the first record's
        # second base and one under the last record's last base
        snps += sorted(set(range(base + 40, last + 200, 97)) | {base + 1, last + 75 + (sum(k for o, k in tile[-1][1] if o == "N"))})
    s = make_shard(oracle_build, recs, snps, rng, qual=rng.integers(15, 41, (len(recs), 76)))
    per_rec = np.bincount(s["want"][0], minlength=len(recs)).reshape(len(counts), TILE)
    assert (per_rec[:, 0] > 0).all() and (per_rec[:, -1] > 0).all()                 # het SNPs under the first and the last record of every tile
    multi = np.array([len(ops) > 1 for _, ops in recs]).reshape(len(counts), TILE)
    assert ((per_rec * multi).sum(axis=1) < 192).all() and ((per_rec * multi).sum(axis=1)[1:] > 20).all()
    assert [sum(len(ops) for _, ops in recs[t * TILE:(t + 1) * TILE]) for t in range(len(counts))] == counts
    # one record of 799 words (400 runs of one base, 399 introns of one) between records of 400M: more words than a tile's LDS holds
    L = 400
    long_ops = [("M", 1), ("N", 1)] * (L - 1) + [("M", 1)]
    recs2 = [(5_000 + 2 * i, [("M", L)]) for i in range(300)]
    recs2[150] = (recs2[150][0], long_ops)
    recs2[TILE - 1] = (recs2[TILE - 1][0], [("M", 100), ("N", 40), ("M", 300)])
    s2 = make_shard(oracle_build, recs2, list(range(4_990, 7_000, 17)), rng, L=L, qual=rng.integers(15, 41, (300, L)))
    per2 = np.bincount(s2["want"][0], minlength=300)
    assert per2[0] > 0 and per2[150] > 5 and per2[TILE - 1] > 0 and per2[299] > 0 and len(long_ops) == 799
    return [s, s2]


@form
def test_cigar_words_per_tile(cigar_words, monkeypatch, form):
    calls, aux = run(cigar_words, monkeypatch, form)
    check(cigar_words, calls, aux)


# ---------------------------------------------------------------------------------------------------------------- the flush
@pytest.fixture(scope="module")
def masked_calls(oracle_build):
    """groups 1,000 bp apart: n het SNPs (n = 1, 2, 8) at offsets 5, 13, .. of a 76M record, and one copy of the record per mask -- none, the first, a middle
    one, the last, all -- whose masked bases have a quality below the limit; then a second, ordinary tile"""
    rng = np.random.default_rng(2205)
    recs, snps, quals, want_n = [], [], [], []
    for g, n in enumerate([1, 2, 8] * 4):
        p = 20_000 + 1_000 * g
        offs = [5 + 8 * i for i in range(n)]
        snps += [p + o for o in offs]
        for mask in ([], [0], [n // 2], [n - 1], list(range(n))):
            q = np.full(76, 30); q[[offs[i] for i in mask]] = BASEQ - 1
            recs.append((p, [("M", 76)])); quals.append(q); want_n.append(n - len(set(mask)))
    while len(recs) < TILE + 60:                             # fill the first tile and start an ordinary second one over further entries
        i = len(recs)
        recs.append((40_000 + 5 * i, mixed_record(rng, i))); quals.append(rng.integers(2, 41, 76))
    snps += list(range(40_000, 40_000 + 5 * len(recs) + 300, 19))
    s = make_shard(oracle_build, recs, snps, rng, qual=np.array(quals))
    assert np.bincount(s["want"][0], minlength=len(recs))[:len(want_n)].tolist() == want_n and 0 in want_n and 7 in want_n
    return [s]


@form
def test_masked_bases_leave_holes(masked_calls, monkeypatch, form):
    calls, aux = run(masked_calls, monkeypatch, form)
    check(masked_calls, calls, aux)


@pytest.fixture(scope="module")
def slot_edges(oracle_build):
    """three shards: a first tile of exactly 7, 8 and 9 calls (76M records, good qualities, k of them over one het SNP each) and a second tile with 3 calls"""
    rng = np.random.default_rng(2206)
    shards = []
    for k in (7, 8, 9):
        recs = [(30_000 + 100 * i, [("M", 76)]) for i in range(TILE + 40)]
        snps = [30_000 + 100 * i + 40 for i in list(range(0, 2 * k, 2)) + [TILE + 3, TILE + 20, TILE + 39]]
        s = make_shard(oracle_build, recs, snps, rng, qual=np.full((len(recs), 76), 30))
        per_tile = np.bincount(s["want"][0] // TILE, minlength=2)
        assert per_tile.tolist() == [k, 3]
        shards.append(s)
    return shards


@form
def test_tile_at_the_slot_size(slot_edges, monkeypatch, form):
    """slots of 8 calls: 7 and 8 calls stay in the tile's own slot, 9 take a stretch of the overflow area; the tile behind each is ordinary"""
    calls, aux = run(slot_edges, monkeypatch, form, {"PHZ_MAP_SLOT_CAP": "8"})
    check(slot_edges, calls, aux)


@pytest.fixture(scope="module")
def interleaved(oracle_build):
    """single-run and spliced records alternating, 4 bp apart over a het SNP every 61 bp (one or two under a record: the spliced records' candidates fit the
    tile's LDS buffer of 192): buffered candidates and fast records interleave in the call list"""
    rng = np.random.default_rng(2207)
    recs = [(60_000 + 4 * i, [("M", 76)] if i % 2 == 0 else [("M", 20 + i % 30), ("N", 35), ("M", 56 - i % 30)]) for i in range(TILE + 100)]
    s = make_shard(oracle_build, recs, list(range(59_990, 60_000 + 4 * len(recs) + 200, 61)), rng, qual=rng.integers(20, 41, (len(recs), 76)))
    per_rec = np.bincount(s["want"][0], minlength=len(recs))[:TILE]
    assert 100 < per_rec[1::2].sum() < 192 and per_rec[0::2].sum() > 100              # qualities above the limit: a spliced record's candidates are its calls
    both = (per_rec[:-1] > 0) & (per_rec[1:] > 0)
    assert both.sum() > 60                                                            # neighbours of the two kinds with calls
    return [s]


@form
@pytest.mark.parametrize("slots", [None, "8"], ids=["default_slots", "slots_of_8"])
def test_candidates_between_fast_records(interleaved, monkeypatch, form, slots):
    calls, aux = run(interleaved, monkeypatch, form, {"PHZ_MAP_SLOT_CAP": slots} if slots else None)
    check(interleaved, calls, aux)


# ------------------------------------------------------------------------------ cigar_off[last + 1] from the pre-pass's words
@form
def test_merge_chunks_knob_changes_nothing(cigar_words, partial, monkeypatch, form):
    """full tiles that end in a spliced record (its end offset is the word the tile no longer loads) and partial ones, through both totals paths"""
    shards = cigar_words + [partial[513], partial[256]]
    a, aux = run(shards, monkeypatch, form)
    b, _ = run(shards, monkeypatch, form, {"PHZ_MAP_MERGE_CHUNKS": "1"})
    same_lists(a, b)
    check(shards, b, aux)
