"""K_map's staged-window search at every window length where it changes path, against the C oracle.

One shard of "islands" 200,000 bp apart -- a tile's window covers 65,536 bp past its last record, so the windows of two islands never overlap --
each island exactly one 256-record tile, its staged window length (het SNPs in [first POS, last POS + 65536) + 8) set by construction to
8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512 (around every power of two the depth classes of the search can be cut at) and 513 (the
truncated window: the LDS walkers are off).  The records of an island mix 76M, aM bN cM whose intron lands before the first, between, on the last and
after the last window entry (and far beyond the window), 5S71M, aM 2I bM and aM 3D bM.  Special islands: only multi-op records (the bracket search
of phase 1a gets its "no single-run record" sentinel in every wave), only 76M, one at position 0 with a het SNP under its first base, and three
islands repeated 2,000,000,000 further on.  The same shard runs through the default instantiation, the 256-thread one, the one-byte-plane one and
the profiling one."""
import numpy as np
import pytest
import torch

from helpers import oracle_map_readbatch

pytestmark = pytest.mark.gpu

L = 76
TILE = 256
SPACING = 200_000
FIELD = 300             # an island's het SNPs start this far behind its first record ...
FAR = 100_000           # ... and three more sit this far out: beyond the window (POS of the last record + 65536), reached only through an intron
WINDOW_LENGTHS = [8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]
OP = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4}
BASEQ = 10


def island(rng, base, n_snps, kinds, snp_at_base=False):
    """-> (het SNP positions, [(pos, [(op, len), ...])] of 256 records sorted by position).  n_snps SNPs inside the window."""
    k_field = n_snps - (1 if snp_at_base else 0)
    d = 6 if k_field > 200 else 12
    field = base + FIELD + d * np.arange(k_field, dtype=np.int64)
    f0 = int(field[0]) if k_field else base + FIELD
    fl = int(field[-1]) if k_field else base + FIELD
    end = base + FIELD + d * k_field
    snps = list(field) + [base + FAR, base + FAR + 7, base + FAR + 20] + ([base] if snp_at_base else [])
    single = "76M" in kinds
    multi = [k for k in kinds if k != "76M"]
    pos = np.concatenate([[base], base + 80 + 5 * np.arange(8), rng.integers(base, end + 200, TILE - 9)])
    recs = []
    for i, p in enumerate(pos.tolist()):
        if i < 9:               # the first record (it fixes the window start) and eight records that end before the first SNP of the field: no call
            kind = "76M" if single else "5S71M"
        elif i < 13 and multi:  # four records whose intron reaches the far SNPs: a call whatever the window holds
            kind = "far"
        else:
            kind = kinds[int(rng.integers(0, len(kinds)))]
        if kind == "76M":
            ops = [("M", L)]
        elif kind == "5S71M":
            ops = [("S", 5), ("M", L - 5)]
        elif kind == "2I":
            a = int(rng.integers(5, L - 10)); ops = [("M", a), ("I", 2), ("M", L - 2 - a)]
        elif kind == "3D":
            a = int(rng.integers(5, L - 10)); ops = [("M", a), ("D", 3), ("M", L - a)]
        else:                   # aM bN cM: where the second run starts
            a = int(rng.integers(10, L - 10)); c = L - a
            modes = ["after", "far"] if kind == "N" else ["far"]
            if kind == "N" and p + a < f0 - c - 2: modes.append("before")
            if kind == "N" and k_field >= 2 and p + a < fl - 8: modes.append("between")
            if kind == "N" and p + a < fl - 5: modes.append("last")
            mode = modes[int(rng.integers(0, len(modes)))]
            if mode == "before":
                t = f0 - c - 1                                    # ends one base before the first SNP of the field
            elif mode == "between":
                cand = field[field - 3 > p + a]
                t = int(cand[int(rng.integers(0, len(cand)))]) - 3
            elif mode == "last":
                t = fl - 5                                        # covers the last SNP inside the window
            elif mode == "after":
                t = max(fl + 1, p + a + 1) + int(rng.integers(0, 50))
            else:
                t = base + FAR - int(rng.integers(1, 10))
            ops = [("M", a), ("N", t - (p + a)), ("M", c)]
        assert sum(n for o, n in ops if o in "MIS") == L and all(n > 0 for o, n in ops)
        recs.append((p, ops))
    recs.sort(key=lambda r: r[0])
    assert recs[0][0] == base
    return snps, recs


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


@pytest.fixture(scope="module")
def islands(oracle_build):
    """The shard, its variant table and the oracle's calls (computed once on the CPU; the preconditions are checked here, before any GPU work)."""
    from phaser_amd import synth
    rng = np.random.default_rng(2024)
    mixed = ["76M", "76M", "76M", "N", "N", "N", "N", "5S71M", "2I", "3D"]
    plan = [(0, 28, mixed, True)]                                                               # position 0, a SNP under the first base
    plan += [(1_000_000 + SPACING * i, w - 8, mixed, False) for i, w in enumerate(WINDOW_LENGTHS)]
    b = 1_000_000 + SPACING * len(WINDOW_LENGTHS)
    plan += [(b, 48, ["N", "N", "5S71M", "2I", "3D"], False), (b + SPACING, 48, ["76M"], False)]      # only multi-op records; only 76M
    plan += [(2_000_000_000 + SPACING * i, w - 8, mixed, False) for i, w in enumerate([33, 129, 513])]
    want_wlen = [28 + 8] + WINDOW_LENGTHS + [48 + 8, 48 + 8, 33, 129, 513]
    snps, recs = [], []
    for base, n_snps, kinds, at_base in plan:
        s, r = island(rng, base, n_snps, kinds, at_base)
        snps += s; recs += r
    n = len(recs)
    assert n == TILE * len(plan)
    vpos = np.array(sorted(int(x) for x in snps), dtype=np.int64)
    assert len(np.unique(vpos)) == len(vpos) and vpos[0] == 0 and vpos[-1] < 2**31 - 1
    pos = np.array([p for p, _ in recs], dtype=np.int64)
    assert (np.diff(pos) >= 0).all() and pos[0] == 0
    # the staged window length of every 256-record tile, as the pre-pass computes it
    first = pos[::TILE]; last = pos[TILE - 1::TILE]
    wl = np.searchsorted(vpos, last + 65536) - np.searchsorted(vpos, first) + 8
    assert wl.tolist() == want_wlen
    assert (last + 65536 < first + FAR).all() and (first[1:] - last[:-1] > 65536 + FAR).all()         # windows neither reach the far SNPs nor overlap
    words = [(ln << 4) | OP[o] for _, ops in recs for o, ln in ops]
    coff = np.zeros(n + 1, np.int64); coff[1:] = np.cumsum([len(ops) for _, ops in recs])
    z = torch.zeros(n, dtype=torch.int32)
    rb = synth.ReadBatch("chr1", L, torch.from_numpy(pos.astype(np.int32)), z, torch.full((n,), 255, dtype=torch.uint8), z, z, torch.arange(n, dtype=torch.int32),
                         torch.from_numpy(coff), torch.tensor(words, dtype=torch.int64),
                         torch.from_numpy(rng.integers(0, 4, (n, L)).astype(np.uint8)), torch.from_numpy(rng.integers(2, 41, (n, L)).astype(np.uint8)))
    vpos32 = vpos.astype(np.int32)
    o_r, o_v, o_c, o_t = oracle_map_readbatch(oracle_build, rb, vpos32, BASEQ)
    assert len(o_r) > 3000
    per_rec = np.bincount(o_r, minlength=n).reshape(len(plan), TILE)
    assert (per_rec > 0).any(axis=1).all() and (per_rec == 0).any(axis=1).all()      # every island: a record with a call and one without
    multi_only = per_rec[len(WINDOW_LENGTHS) + 1]; assert all(len(ops) > 1 for _, ops in recs[(len(WINDOW_LENGTHS) + 1) * TILE:(len(WINDOW_LENGTHS) + 2) * TILE]) and multi_only.any()
    assert (o_c == 4).sum() > 5                                                      # an insertion next to a het SNP did occur
    return {"rb": rb, "recs": recs, "vpos": vpos32, "oracle": (o_r, o_v, o_c, o_t)}


@pytest.mark.parametrize("env", [{}, {"PHZ_MAP_BLOCK": "256"}, {"PHZ_MAP_ONE_PLANE": "1"}, {"PHZ_MAP_DBG": "4096"}],
                         ids=["default", "block256", "one_plane", "profiling"])
def test_island_windows_vs_oracle(islands, monkeypatch, env):
    from phaser_amd import soa
    from phaser_amd.mapper import Mapper
    from phaser_amd.read_variant_map import _allele_text
    for k in ("PHZ_MAP_BLOCK", "PHZ_MAP_RPT", "PHZ_MAP_ONE_PLANE", "PHZ_MAP_TWO_PLANES", "PHZ_MAP_DBG", "PHZ_MAP_SLOT_CAP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rb = islands["rb"]; recs = islands["recs"]; vpos = islands["vpos"]
    o_r, o_v, o_c, o_t = islands["oracle"]
    shard = soa.pack_readbatch(rb).to("cuda")
    assert (soa.bq_plane(shard) is not None) == ("PHZ_MAP_ONE_PLANE" in env)
    calls = Mapper(0).map(shard, torch.from_numpy(vpos), BASEQ).cpu()
    assert calls.n == len(o_r)
    assert np.array_equal(calls.read_idx.numpy(), o_r) and np.array_equal(calls.var_idx.numpy(), o_v) and np.array_equal(calls.code.numpy(), o_c)
    # aux0 / aux1: the read offset of the called base for a plain call (worked out from the CIGAR here), the oracle's text for a composite one
    a0 = calls.aux0.numpy().view(np.uint32); a1 = calls.aux1.numpy().view(np.uint32)
    want0 = np.array([read_offset(recs[r][1], recs[r][0], int(vpos[v])) if c < 4 else -1 for r, v, c in zip(o_r.tolist(), o_v.tolist(), o_c.tolist())], dtype=np.int64)
    plain = o_c < 4
    assert np.array_equal(a0[plain].astype(np.int64), want0[plain]) and not a1[plain].any()
    lut = "ACGTN"
    for k in np.nonzero(~plain)[0].tolist():
        r = int(o_r[k])
        seq = "".join(lut[x] for x in rb.seq[r].tolist()); qual = "".join(chr(33 + q) for q in rb.qual[r].tolist())
        assert _allele_text(int(o_c[k]), int(a0[k]), int(a1[k]), seq, qual, BASEQ) == o_t[k]
