"""Designed call lines for K_tally (phaser_amd/csrc/phz_tally.hip): one deterministic builder per named case.  A case is the `saved`-shaped dict
run_tally takes (per chromosome: nv, line_var / line_qid / line_cls / line_bam in line order, bam_offsets; n_qid per chromosome) with its chromosome
list and number of BAMs, and what the case PROMISES: how many far lines, dirty read lists, spilled QNAMEs and out-of-bitmap lines the kernels must meet on
it, whether the variant-pair table must overflow.  The promises come from tiling() below, a mirror of the tiling rules ALONE:

    tiles          TL consecutive lines of a (chromosome, BAM) shard (product 1,024; the emulated variant 256)
    window base    wb = max(0, suffix minimum over the shard's tiles of (variant of the tile's first line) - 64), variants in the call's space
    far line       a kept line with variant - wb outside [0, 256)
    dirty list     a (variant, allele, BAM) read list with a far ref/alt line
    bitmap base    q0 = id of the tile's first line in the call's id space; qb = (q0 - 8192) & ~31 if q0 > 8192 else 0; in the bitmap: qb <= id < qb + 16384
    spilled QNAME  kept lines in two tiles (two BAMs are two tiles), or two kept out-of-bitmap lines in one tile

What the kernels must COMPUTE on a case is tests/tally_restatement.py's business, which knows none of this."""
import functools

import numpy as np

TWT = 256; QW = 16384; PAIR_TABLE_MIN = 1 << 16
CLS_P = [0.45, 0.4, 0.1, 0.05]          # ref, alt, other, dropped


class Case:
    def __init__(self, name, chroms, n_bams, nq, as16=False, redo=False, tile_matters=False, note=""):
        """chroms: [(chromosome, nv, [(bam, var, qid, cls), ...])] with the shards of a chromosome in BAM order (a BAM may be absent, a shard may be empty)"""
        self.name = name; self.n_bams = n_bams; self.as16 = as16; self.redo = redo; self.tile_matters = tile_matters; self.note = note
        self.chrom_list = [c for c, _, _ in chroms]
        self.saved = {"tally": {}, "n_qid": {}}
        for (c, nv, shards), q in zip(chroms, nq):
            offs = []; at = 0
            for b, var, qid, cls in shards:
                assert len(var) == len(qid) == len(cls)
                offs.append((b, at, len(var))); at += len(var)
            cat = lambda k, dt: np.concatenate([np.asarray(s[k], dtype=dt) for s in shards]) if shards else np.zeros(0, dt)
            R = {"nv": nv, "line_var": cat(1, np.int32), "line_qid": cat(2, np.int32), "line_cls": cat(3, np.uint8),
                 "line_bam": np.concatenate([np.full(len(s[1]), s[0], np.int32) for s in shards]) if shards else np.zeros(0, np.int32), "bam_offsets": offs}
            assert len(R["line_var"]) == 0 or (0 <= R["line_var"].min() and R["line_var"].max() < nv and 0 <= R["line_qid"].min() and R["line_qid"].max() < q)
            for a in R.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self.saved["tally"][c] = R; self.saved["n_qid"][c] = q

    @property
    def n_lines(self):
        return sum(len(R["line_var"]) for R in self.saved["tally"].values())

    @property
    def nv(self):
        return sum(R["nv"] for R in self.saved["tally"].values())

    def promise(self, tile=1024):
        return tiling(self, tile)


@functools.lru_cache(maxsize=None)
def tiling(case, TL):
    """the mirror of the tiling rules -> {"far", "dirty", "spilled", "spill_lines", "oob", "tiles", "qnames"} (see the module text), "tiles_of": per QNAME id of
    the call's space {tile: [kept lines, kept out-of-bitmap lines]}, "wb": (chromosome, BAM, window base) per tile"""
    far = 0; dirty = set(); oob = 0; n_tiles = 0; bases = []
    tiles_of = {}                     # QNAME id in the call's space -> {tile: [kept lines, kept out-of-bitmap lines]}
    vb = qb0 = 0
    for c in case.chrom_list:
        R = case.saved["tally"][c]
        for b, base, n in R["bam_offsets"]:
            var = R["line_var"][base:base + n].astype(np.int64) + vb; qid = R["line_qid"][base:base + n].astype(np.int64) + qb0; cls = R["line_cls"][base:base + n]
            nt = (n + TL - 1) // TL
            wb = np.zeros(nt, np.int64); after = 1 << 40
            for t in range(nt - 1, -1, -1):
                after = min(after, int(var[t * TL])); wb[t] = max(0, after - 64)
            bases += [(c, b, int(w)) for w in wb]
            for t in range(nt):
                tid = n_tiles + t
                q0 = int(qid[t * TL]); qb = ((q0 - QW // 2) & ~31) if q0 > QW // 2 else 0
                for i in range(t * TL, min(n, (t + 1) * TL)):
                    if cls[i] == 255:
                        continue
                    if not 0 <= var[i] - wb[t] < TWT:
                        far += 1
                        if cls[i] < 2:
                            dirty.add((int(var[i]), int(cls[i]), b))
                    out = not qb <= qid[i] < qb + QW
                    oob += out
                    rec = tiles_of.setdefault(int(qid[i]), {}).setdefault(tid, [0, 0])
                    rec[0] += 1; rec[1] += out
            n_tiles += nt
        vb += R["nv"]; qb0 += case.saved["n_qid"][c]
    spilled = [q for q, ts in tiles_of.items() if len(ts) > 1 or any(r[1] > 1 for r in ts.values())]
    return {"far": far, "dirty": len(dirty), "spilled": len(spilled), "spill_lines": sum(r[0] for q in spilled for r in tiles_of[q].values()), "oob": int(oob),
            "tiles": n_tiles, "qnames": len(tiles_of), "tiles_of": tiles_of, "wb": bases}


def _cls(rng, n, p=CLS_P):
    return rng.choice([0, 1, 2, 255], size=n, p=p).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the five inputs test_emu_tally.py had
@functools.lru_cache(maxsize=None)
def skewed():
    """read lists of thousands of entries (workgroup bitonic sort, device radix sort), QNAMEs shared by two BAMs (owner = last BAM), dropped lines"""
    rng = np.random.default_rng(7)
    nv = 24; nq = 3000
    shards = []
    for b in range(2):
        n = 30000 if b == 0 else 7000
        var = np.sort(rng.choice(nv, size=n, p=np.array([0.55, 0.2] + [0.25 / 22] * 22)))          # variant 0: thousands of lines
        qid = rng.integers(0, nq, size=n)
        cls = rng.choice([0, 1, 2, 255], size=n, p=[0.45, 0.4, 0.1, 0.05]).astype(np.uint8)
        shards.append((b, var, qid, cls))
    return Case("skewed", [("chrS", nv, shards)], 2, [nq])


@functools.lru_cache(maxsize=None)
def far_lines():
    """a read spliced over hundreds of het SNPs puts call lines outside the variant window of the tile they arrive in: their read lists are filled
    through cursors and put into line order afterwards -- a short one in LDS, one of > 4,096 entries by the device radix sort.  AS as the 2-byte plane"""
    rng = np.random.default_rng(23)
    nv = 900; nq = 5000
    var = [np.zeros(6000, np.int64)]                                   # variant 0: 6,000 lines in a row (six tiles with the same window) ...
    later = np.sort(rng.integers(500, 560, size=3000))                 # ... then lines of variants 500-559, the windows have moved on ...
    far0 = rng.choice(3000, size=12, replace=False); later[far0] = 0   # ... with twelve more lines of variant 0 among them (far: list (0, *) > 4,096 entries)
    far7 = rng.choice(3000, size=5, replace=False); later[far7] = 7    # and five of variant 7, which has no other line (a short dirty list)
    var.append(later)
    var.append(np.sort(rng.integers(560, 900, size=2500)))
    var = np.concatenate(var).astype(np.int32)
    n = len(var)
    qid = rng.integers(0, nq, size=n).astype(np.int32)
    cls = rng.choice([0, 1, 2, 255], size=n, p=[0.5, 0.4, 0.05, 0.05]).astype(np.uint8)
    return Case("far_lines", [("chrS", nv, [(0, var, qid, cls)])], 1, [nq], as16=True, tile_matters=True)


@functools.lru_cache(maxsize=None)
def long_groups():
    """QNAMEs with more than 64 distinct (variant, class) items: groups inside one tile (finished in place; their later items come from the 64-item
    look-ahead and, beyond it, from memory) and groups that straddle tiles (spill path)"""
    rng = np.random.default_rng(11)
    nv = 160; nq = 60
    var = []; qid = []
    for q in range(40):                                   # 40 QNAMEs x 110 lines on 110 different variants, contiguous: tile-local groups
        v = np.sort(rng.choice(nv, size=110, replace=False))
        var.append(v); qid.append(np.full(110, q))
    v2 = rng.integers(0, nv, size=6000); q2 = rng.integers(40, nq, size=6000)      # 20 QNAMEs x ~300 lines spread over everything
    var.append(v2); qid.append(q2)
    var = np.concatenate(var).astype(np.int32); qid = np.concatenate(qid).astype(np.int32)
    n = len(var)
    cls = rng.choice([0, 1, 2, 255], size=n, p=[0.45, 0.4, 0.1, 0.05]).astype(np.uint8)
    return Case("long_groups", [("chrS", nv, [(0, var, qid, cls)])], 1, [nq], tile_matters=True)


@functools.lru_cache(maxsize=None)
def scan_over_many_tiles():
    """the single-launch scan (look-back over the predecessors' status words) on a read-list table of 13 tiles -- more than one round of eight predecessors"""
    rng = np.random.default_rng(5)
    nv = 26000; nq = 500; n = 3000
    var = np.sort(rng.integers(0, nv, size=n)).astype(np.int32); qid = rng.integers(0, nq, size=n).astype(np.int32)
    cls = rng.choice([0, 1, 2, 255], size=n, p=[0.45, 0.4, 0.1, 0.05]).astype(np.uint8)
    return Case("scan_over_many_tiles", [("chrS", nv, [(0, var, qid, cls)])], 1, [nq])


@functools.lru_cache(maxsize=None)
def empty_dropped_live():
    """a shard without lines, a shard whose lines are all dropped by the AS cutoff, the same lines alive: three calls for one context, in this order"""
    nv = 50; nq = 10
    z = np.zeros(0, np.int32)
    empty = Case("empty_shard", [("chrS", nv, [(0, z, z, z.astype(np.uint8))])], 1, [nq])
    n = 300
    rng = np.random.default_rng(2)
    var = np.sort(rng.integers(0, nv, n)).astype(np.int32); qid = rng.integers(0, nq, n).astype(np.int32)
    dropped = Case("all_lines_dropped", [("chrS", nv, [(0, var, qid, np.full(n, 255, np.uint8))])], 1, [nq])
    live = Case("live_after_dropped", [("chrS", nv, [(0, var, qid, rng.choice([0, 1, 2], size=n).astype(np.uint8))])], 1, [nq])
    return (empty, dropped, live)


# ------------------------------------------------------------------------------------------------ the limits no test reached
N_KIND = 48        # designed QNAMEs of each kind in qnames_beyond_the_bitmap


@functools.lru_cache(maxsize=None)
def qnames_beyond_the_bitmap():
    """8,192 lines of one BAM on ids drawn from 40,000: most lines of a tile lie more than 8,192 ids from its first line's id, outside k_line's LDS bitmap,
    and go straight to the global bitmaps.  Three designed kinds of QNAME, N_KIND each (case.kinds): "two_in_one_tile" two out-of-bitmap lines in one tile
    and none elsewhere (they look shared: spill path), "one_in_each_of_two_tiles" out of the bitmap in both, "in_and_out" in the bitmap of one tile and
    outside that of another.  Every other QNAME has one line.  The variants ascend slowly: no far line."""
    rng = np.random.default_rng(97)
    n = 8192; nq = 40000; nv = 400; TL = 1024
    var = np.sort(rng.integers(0, nv, size=n)).astype(np.int32)
    qid = rng.choice(nq, size=n, replace=False).astype(np.int64)
    cls = _cls(rng, n)
    nt = n // TL
    qb = [((int(qid[t * TL]) - QW // 2) & ~31) if qid[t * TL] > QW // 2 else 0 for t in range(nt)]
    inside = lambda q, t: qb[t] <= q < qb[t] + QW
    free = [[i for i in range(t * TL + 1, (t + 1) * TL) if i % 256] for t in range(nt)]          # never a tile's first line (of either tile length)
    for f in free:
        rng.shuffle(f)
    kinds = {"two_in_one_tile": [], "one_in_each_of_two_tiles": [], "in_and_out": []}

    def pair_up(name, t, others, ok):
        """a free line of tile t whose id satisfies ok(id, u) for the first possible tile u of `others` gives its id to a free line of u (whose own id leaves the input)"""
        for u in others:
            k = next((k for k, i in enumerate(free[t]) if ok(int(qid[i]), u)), None)
            if k is not None:
                x = free[t].pop(k); y = free[u].pop()
                qid[y] = qid[x]; cls[x] = 0; cls[y] = 1
                kinds[name].append(int(qid[x]))
                return
        raise AssertionError((name, t))
    for j in range(N_KIND):
        t = j % nt
        others = [(t + 1 + j // nt + d) % nt for d in range(nt)]; others = [u for u in others if u != t]
        pair_up("two_in_one_tile", t, [t], lambda q, u: not inside(q, t))
        pair_up("one_in_each_of_two_tiles", t, others, lambda q, u: not inside(q, t) and not inside(q, u))
        pair_up("in_and_out", t, others, lambda q, u: not inside(q, t) and inside(q, u))
    c = Case("qnames_beyond_the_bitmap", [("chrQ", nv, [(0, var, qid, cls)])], 1, [nq], tile_matters=True)
    c.kinds = kinds
    return c


@functools.lru_cache(maxsize=None)
def spilled_groups_beyond_the_group_window():
    """nv = 3,000; three clusters of 150 variants (around 0, 1,400 and 2,850) of 2,048 lines each, so that no line is far.  300 QNAMEs (two workgroups of k_groups)
    own one line in each of the six tiles: whichever of a workgroup's items arrives first and sets its LDS window (1,024 variants from that variant - 256), two of
    the three clusters lie outside it -- more than 1,024 above or more than 256 below -- and take the global-atomic branch for var_distinct and var_rank"""
    rng = np.random.default_rng(131)
    nv = 3000; n_sp = 300; per = 2048
    var = []; qid = []
    for k, v0 in enumerate((0, 1400, 2850)):
        v = np.sort(rng.integers(v0, v0 + 150, size=per)); q = 1000 + k * per + np.arange(per)          # filler: one line per QNAME
        for half in range(2):
            at = half * 1024 + rng.choice(np.arange(1, 1024), size=n_sp, replace=False)
            q[at] = rng.permutation(n_sp)
        var.append(v); qid.append(q)
    var = np.concatenate(var).astype(np.int32); qid = np.concatenate(qid).astype(np.int32)
    cls = _cls(rng, len(var))
    cls[qid < n_sp] = rng.integers(0, 2, size=int((qid < n_sp).sum()))          # their lines are all kept, all ref/alt
    return Case("spilled_groups_beyond_the_group_window", [("chrG", nv, [(0, var, qid, cls)])], 1, [1000 + 3 * per], tile_matters=True)


@functools.lru_cache(maxsize=None)
def pair_table_redo():
    """nv = 1,140 (the table starts at its minimum of 2^16 slots); six tiles, tile t holds ten QNAMEs of 100 lines on 100 of the 190 variants [190 t, 190 t + 190)
    and 24 single lines: about 17,000 of the 17,955 pairs of every window occur, more than 100,000 distinct pairs from 6,144 lines"""
    rng = np.random.default_rng(61)
    W = 190; T = 6; nv = W * T
    var = []; qid = []
    for t in range(T):
        for j in range(10):
            var.append(W * t + np.sort(rng.choice(W, size=100, replace=False))); qid.append(np.full(100, 10 * t + j))
        var.append(W * t + np.sort(rng.integers(0, W, size=24))); qid.append(100 + 24 * t + np.arange(24))
    var = np.concatenate(var).astype(np.int32); qid = np.concatenate(qid).astype(np.int32)
    cls = _cls(rng, len(var), [0.5, 0.45, 0.05, 0.0])
    return Case("pair_table_redo", [("chrP", nv, [(0, var, qid, cls)])], 1, [100 + 24 * T], redo=True)


def _one_stray_line(name, lo, stray, at):
    """4,096 lines whose variants ascend slowly from lo to lo + 150 (under 64 variants per tile: a window that starts 64 below the NEXT tile's first variant still holds
    the whole tile), except the line at `at` (a multiple of every tile length), which sits on `stray` and shares
    its QNAME with the line before it"""
    rng = np.random.default_rng(len(name))
    n = 4096; nv = 2000; nq = 3000
    var = np.sort(rng.integers(lo, lo + 150, size=n)).astype(np.int32); qid = rng.integers(0, nq, size=n).astype(np.int32)
    cls = _cls(rng, n)
    var[at] = stray; qid[at] = qid[at - 1]; cls[at] = 0; cls[at - 1] = 1
    return Case(name, [("chrT", nv, [(0, var, qid, cls)])], 1, [nq], tile_matters=True)


@functools.lru_cache(maxsize=None)
def tile_starts_far_right():
    """the first line of the third tile sits 1,200 variants to the right of everything around it (the middle of a spliced record): the suffix minimum of
    k_tile_base keeps the window where the tile's other lines are, the one line is far, its list dirty, nothing else"""
    return _one_stray_line("tile_starts_far_right", 0, 1500, 2048)


@functools.lru_cache(maxsize=None)
def tile_starts_far_left():
    """the first line of the fourth tile sits on variant 5, a thousand variants to the left of everything: the suffix minimum pulls the window base of EVERY tile of
    the shard down to 0, so every other kept line is far and every read list but one is dirty"""
    return _one_stray_line("tile_starts_far_left", 1000, 5, 3072)


@functools.lru_cache(maxsize=None)
def chromosome_seams():
    """two chromosomes of 300 and 10 variants, three BAMs.  The lines sit on the last 5 variants of the first and on all of the second: the tile windows of the first
    chromosome run past its end into the second one's variants, those of the second start inside the first.  Shard (chrA, BAM 2) is there with zero lines, BAM 1 has
    no shard on chrB.  400 ids per chromosome, shared by the BAMs: nearly every QNAME has lines in two BAMs (owner rule)"""
    rng = np.random.default_rng(211)
    nq = 400

    def shard(b, n, v0, v1, other_only=False):
        var = np.sort(rng.integers(v0, v1, size=n)).astype(np.int32); qid = rng.integers(0, nq, size=n).astype(np.int32)
        return (b, var, qid, _cls(rng, n, [0.0, 0.0, 0.95, 0.05] if other_only else CLS_P))
    z = np.zeros(0, np.int32)
    A = [shard(0, 1500, 295, 300), shard(1, 1100, 295, 300), (2, z, z, z.astype(np.uint8))]
    B = [shard(0, 1300, 0, 10), shard(2, 700, 0, 10)]
    return Case("chromosome_seams", [("chrA", 300, A), ("chrB", 10, B)], 3, [nq, nq], tile_matters=True)


@functools.lru_cache(maxsize=None)
def two_bams_owner_rule():
    """the skewed input at 3,000 + 1,000 lines, its 600 ids in four bands (case.bands): ref/alt lines only in BAM 0, only in BAM 1, in both, and in BAM 0 with
    nothing but "other"-class lines in BAM 1 (the last BAM holds lines of the QNAME and still does not own it).  Its 24 variants are so deeply covered that some
    QNAME links every pair of them, so three QNAMEs on six variants of their own (24-29) follow, whose pairs hang on the owner rule alone:
      600  ref/alt lines on 24 and 25 in BAM 0, one on variant 0 in BAM 1: BAM 1 owns the list, the pair (24, 25) has cells and is NOT linked, neither variant gets a rank
      601  a ref line on 26 in BAM 0, an alt line on 27 in BAM 1: the pair (26, 27) is not linked either (the item on 26 is no entry of the surviving list)
      602  ref/alt lines on 28 and 29 in BAM 1, one on variant 1 in BAM 0: linked"""
    rng = np.random.default_rng(7)
    nv = 24
    p = np.array([0.55, 0.2] + [0.25 / 22] * 22)
    bands = {"bam0_only": (0, 150), "bam1_only": (150, 300), "both": (300, 450), "bam0_and_other_in_bam1": (450, 600)}
    n0, n1 = 3000, 1000
    var0 = np.sort(rng.choice(nv, size=n0, p=p)); var1 = np.sort(rng.choice(nv, size=n1, p=p))
    q0 = rng.choice(np.r_[0:150, 300:600], size=n0); q1 = rng.choice(np.r_[150:600], size=n1)
    c0 = _cls(rng, n0); c1 = _cls(rng, n1)
    c1[(q1 >= 450) & (c1 < 2)] = 2
    var0 = np.r_[1, var0, 24, 25, 26]; q0 = np.r_[602, q0, 600, 600, 601]; c0 = np.r_[0, c0, 0, 1, 0].astype(np.uint8)
    var1 = np.r_[0, var1, 27, 28, 29]; q1 = np.r_[600, q1, 601, 602, 602]; c1 = np.r_[1, c1, 1, 0, 1].astype(np.uint8)
    c = Case("two_bams_owner_rule", [("chrS", nv + 6, [(0, var0, q0, c0), (1, var1, q1, c1)])], 2, [603])
    c.bands = bands
    return c


def designed_cases():
    """every case, in the order the one-context sequence takes them: a small case right after the redo, the far-left and the spill-heavy ones"""
    e, d, l = empty_dropped_live()
    return [skewed(), l, far_lines(), long_groups(), e, pair_table_redo(), two_bams_owner_rule(), tile_starts_far_left(), d, l, spilled_groups_beyond_the_group_window(),
            chromosome_seams(), qnames_beyond_the_bitmap(), e, tile_starts_far_right(), scan_over_many_tiles(), two_bams_owner_rule()]


def all_cases():
    seen = {}
    for c in designed_cases():
        seen.setdefault(c.name, c)
    return list(seen.values())
