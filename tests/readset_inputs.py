"""Designed inputs for the read-set kernels of the row stage (phaser_amd/csrc/phz_rowsdev.hip: k_seg_small, k_seg_big): one deterministic builder per named design.
A design is a set of call lines in the `saved` form of tests/tally_inputs.py (one chromosome, chrS), the VCF text of its variants, the names of its BAMs and QNAMEs,
and the blocks it is BUILT to give: every read carries the alleles of one haplotype of the truth, so no read conflicts with its block and every pair test has
p = 1 (one conflicting QNAME at zero noise gives p = 0 and dissolves the block).  What the kernels must compute on a design is tests/readset_restatement.py's business;
which segments a design holds (entry counts M, piece counts np, size classes) is asserted from that restatement by tests/test_readset_limits.py before any kernel runs.

A read is (BAM, haplotype, QNAME id, variants): one call line per listed variant (a variant listed twice: two lines of the QNAME in one read list), class =
truth[variant] ^ haplotype.  The lines of a BAM are its reads ordered by their first variant."""
import functools

import numpy as np

import readset_restatement as rr
from tally_inputs import Case

CHROM = "chrS"
BOUNDARY_SIZES = (0, 1, rr.SEG_SMALL - 1, rr.SEG_SMALL, rr.SEG_SMALL + 1, rr.SEG_MID - 1, rr.SEG_MID, rr.SEG_MID + 1, rr.SEG_LDS - 1, rr.SEG_LDS, rr.SEG_LDS + 1, 6001)


def position(v):
    return 1000 + 40 * v


def truth(v):
    """the allele haplotype 0 of the truth carries on variant v"""
    return (v * v + v // 2) & 1


def vcf_text(nv):
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"
    return head + "".join("%s\t%d\trs%d\tA\tG\t.\tPASS\t.\tGT\t%s\n" % (CHROM, position(v), v, "0|1" if v % 3 else "1|0") for v in range(nv))


class Reads:
    def __init__(self, n_bams):
        self.n_bams = n_bams; self.reads = [[] for _ in range(n_bams)]; self.nq = 0

    def add(self, bam, hap, variants, qid=None):
        if qid is None:
            qid = self.nq; self.nq += 1
        self.reads[bam].append((min(variants), qid, hap, list(variants)))
        return qid

    def shards(self):
        out = []
        for b, reads in enumerate(self.reads):
            reads = sorted(reads, key=lambda r: r[0])          # stable: reads with the same first variant stay in the order they were added
            var = [v for _, q, h, vs in reads for v in vs]; qid = [q for _, q, h, vs in reads for v in vs]; cls = [truth(v) ^ h for _, q, h, vs in reads for v in vs]
            out.append((b, np.asarray(var, np.int32), np.asarray(qid, np.int32), np.asarray(cls, np.uint8)))
        return out


class Design:
    def __init__(self, name, nv, n_bams, shards, nq, blocks, blacklist=(), note=""):
        """blocks: the member lists of the blocks the design is built to give (haplotype A of the declared table = haplotype 0 of the truth: which of the two the
        phasing calls A does not change the set of segments)"""
        self.name = name; self.nv = nv; self.n_bams = n_bams; self.note = note
        self.case = Case(name, [(CHROM, nv, shards)], n_bams, [nq])
        self.saved = self.case.saved; self.chrom_list = [CHROM]
        self.saved["qnames"] = {CHROM: ["q%d" % i for i in range(nq)]}
        self.vcf_text = vcf_text(nv)
        self.bam_names = ["bam%d" % b for b in range(n_bams)]
        self.blocks = [(list(m), [truth(v) for v in m]) for m in blocks]
        self.blacklist = frozenset("%s_%d" % (CHROM, position(v)) for v in blacklist)
        self.black = frozenset(blacklist)

    @property
    def n_lines(self):
        return self.case.n_lines

    def read_lists(self):
        """(rl_start, rl_qid): the ref / alt lines grouped by (variant, allele, BAM), in line order -- a stable grouping of the lines, nothing else"""
        R = self.saved["tally"][CHROM]; nb = self.n_bams
        sel = np.flatnonzero(R["line_cls"] < 2)
        key = (R["line_var"][sel].astype(np.int64) * 2 + R["line_cls"][sel]) * nb + R["line_bam"][sel]
        order = np.argsort(key, kind="stable")
        rl_start = np.zeros(self.nv * 2 * nb + 1, np.int64)
        np.cumsum(np.bincount(key, minlength=self.nv * 2 * nb), out=rl_start[1:])
        return rl_start, R["line_qid"][sel][order].astype(np.int64)

    @functools.lru_cache(maxsize=None)
    def declared(self):
        """the restatement on the declared block table (tier 2: no kernel, no phasing)"""
        rs, rq = self.read_lists()
        return rr.restate(rs, rq, self.n_bams, self.blocks, self.black)


def _fill(R, bam, hap, v0, v1, S, reuse=()):
    """exactly S entries of haplotype `hap` in BAM `bam` on the block (v0, v1): QNAMEs with two lines on v0 (a duplicate inside a list), QNAMEs with one line,
    QNAMEs with a line on each variant (they repeat inside the segment and link the block); `reuse`: ids of linking QNAMEs of another BAM to take first"""
    dups = min(3, S // 8); singles = (S - 2 * dups) % 2 + 2 * min(2, S // 8); links = (S - 2 * dups - singles) // 2
    assert 2 * dups + singles + 2 * links == S
    reuse = list(reuse); ids = []
    for i in range(links):
        ids.append(R.add(bam, hap, [v0, v1], reuse.pop() if reuse else None))
        if i < dups:
            R.add(bam, hap, [v0, v0])
        if i < singles:
            R.add(bam, hap, [v1 if i % 2 else v0])
    for i in range(links, max(dups, singles)):
        if i < dups:
            R.add(bam, hap, [v0, v0])
        if i < singles:
            R.add(bam, hap, [v1 if i % 2 else v0])
    return ids


@functools.lru_cache(maxsize=None)
def size_classes():
    """Two BAMs, twelve two-variant blocks, twelve singleton variants.  Block k: haplotype 0 has exactly BOUNDARY_SIZES[k] entries, all in BAM 0 -- a mode-0 segment and
    a mode-1 segment of that size -- next to a small haplotype 1 whose QNAMEs are partly shared by the two BAMs (mode 1 is a union); blocks 7 and 10 carry a few hundred
    entries of haplotype 1 in both BAMs.  Singleton 24 + k: a read list (alt or ref by the truth, BAM 1) of exactly BOUNDARY_SIZES[k] entries, a mode-2 segment."""
    R = Reads(2)
    nblk = len(BOUNDARY_SIZES)
    for k, S in enumerate(BOUNDARY_SIZES):
        v0, v1 = 2 * k, 2 * k + 1
        _fill(R, 0, 0, v0, v1, S)
        big = k in (7, 10)
        shared = _fill(R, 1, 1, v0, v1, 150 if big else 8)
        _fill(R, 0, 1, v0, v1, 200 if big else 6, reuse=shared[:50 if big else 2])
    for k, S in enumerate(BOUNDARY_SIZES):
        v = 2 * nblk + k
        ids = [R.add(1, 0, [v]) for _ in range(S - S // 5)]
        for i in range(S // 5):                                   # a fifth of the entries repeat an earlier QNAME of the list
            R.add(1, 0, [v], ids[(i * 7) % len(ids)])
        for _ in range(3):
            R.add(0, 1, [v])
    return Design("size_classes", 3 * nblk, 2, R.shards(), R.nq, [(2 * k, 2 * k + 1) for k in range(nblk)])


@functools.lru_cache(maxsize=None)
def one_qname():
    """Two blocks whose haplotype 0 in BAM 0 is ONE QNAME: 257 entries (129 lines on the first variant, 128 on the second) and 2,049 (1,025 + 1,024): one slot takes
    every atomicCAS and atomicMin, the count is 1, every label 0, only the first entry is a first appearance"""
    R = Reads(2)
    for k, S in enumerate((rr.SEG_MID + 1, rr.SEG_LDS + 1)):
        v0, v1 = 2 * k, 2 * k + 1
        R.add(0, 0, [v0] * (S - S // 2) + [v1] * (S // 2))
        shared = _fill(R, 1, 1, v0, v1, 6)
        _fill(R, 0, 1, v0, v1, 8, reuse=shared[:2])
    return Design("one_qname", 4, 2, R.shards(), R.nq, [(0, 1), (2, 3)])


@functools.lru_cache(maxsize=None)
def huge_block():
    """Three BAMs.  Block 0: a clean chain of STAT_N + 1 variants -- its segments have more pieces than the LDS piece arrays hold.  BAM 0 covers every adjacent pair
    with three reads per haplotype (3,072 entries each: pieces and table in the pool); BAM 1 covers one pair with 20 reads of haplotype 0 (40 entries: pieces in the
    pool, table in LDS) and another with 5 of haplotype 1 (10 entries: one thread walks 513 pieces); BAM 2 has no read in the block.  Block 1: a clean chain of
    exactly STAT_N variants, one read per pair and haplotype in BAM 0 (1,022 entries: not huge, the LDS piece arrays full up to s_pref[np]), a few reads in BAM 2."""
    n0 = rr.STAT_N + 1; n1 = rr.STAT_N
    R = Reads(3)
    for i in range(n0 - 1):
        for r in range(6):
            R.add(0, r % 2, [i, i + 1])
    for _ in range(20):
        R.add(1, 0, [10, 11])
    for _ in range(5):
        R.add(1, 1, [300, 301])
    for i in range(n0, n0 + n1 - 1):
        for h in (0, 1):
            R.add(0, h, [i, i + 1])
    for _ in range(4):
        R.add(2, 0, [n0 + 7, n0 + 8])
        R.add(2, 1, [n0 + 400, n0 + 401])
    return Design("huge_block", n0 + n1, 3, R.shards(), R.nq, [tuple(range(n0)), tuple(range(n0, n0 + n1))])


@functools.lru_cache(maxsize=None)
def blacklisted_pieces():
    """Two BAMs.  Block 0, variants 0-7: the first member, two adjacent middle members (3, 4) and the last one are blacklisted; in BAM 0 haplotype 0 keeps 48 entries
    on the other four (a wave), haplotype 1 keeps 360 (a workgroup).  Block 1, variants 8-11: every member but variant 10 is blacklisted (40 entries of haplotype 0: a
    wave whose only piece with entries lies between pieces of length zero; 6 of haplotype 1: one thread)"""
    R = Reads(2)
    for i in range(7):
        for _ in range(6):
            R.add(0, 0, [i, i + 1])
        for _ in range(45):
            R.add(0, 1, [i, i + 1])
        for h in (0, 1):
            for _ in range(2):
                R.add(1, h, [i, i + 1])
    for i in range(8, 11):
        for _ in range(20):
            R.add(0, 0, [i, i + 1])
        for _ in range(3):
            R.add(0, 1, [i, i + 1])
        R.add(1, 0, [i, i + 1]); R.add(1, 1, [i, i + 1])
    return Design("blacklisted_pieces", 12, 2, R.shards(), R.nq, [tuple(range(8)), tuple(range(8, 12))], blacklist=(0, 3, 4, 7, 8, 9, 11))


POOL_DISTINCT = 150000          # distinct QNAMEs of the pool-growth segment: labels of six digits


@functools.lru_cache(maxsize=None)
def pool_growth_product():
    """Two BAMs, two two-variant blocks.  Haplotype 0 of block 0 has, in BAM 0, one entry more than the smallest segment whose table the row stage's pool cannot hold
    as first reserved (rr.smallest_overflowing_segment: 2^19 + 1), over 150,000 distinct QNAMEs; a small block follows.  Built with numpy"""
    N = rr.smallest_overflowing_segment(rr.SEG_POOL_BYTES) + 1
    n0 = N - N // 2; n1 = N // 2
    q0 = np.arange(n0, dtype=np.int64) % POOL_DISTINCT; q1 = (np.arange(n1, dtype=np.int64) * 7 + 3) % POOL_DISTINCT
    R = Reads(2); R.nq = POOL_DISTINCT
    shared = _fill(R, 1, 1, 0, 1, 6); _fill(R, 0, 1, 0, 1, 10, reuse=shared[:2]); _fill(R, 1, 0, 0, 1, 4)
    for b in (0, 1):
        for h in (0, 1):
            _fill(R, b, h, 2, 3, 12 - 8 * b)
    small = R.shards()
    b, var, qid, cls = small[0]
    # BAM 0: the big segment's lines (variant 0, then variant 1), then the small reads (four variants: every line inside its tile's variant window)
    var = np.concatenate([np.zeros(n0, np.int32), np.ones(n1, np.int32), var]).astype(np.int32)
    qid = np.concatenate([q0, q1, qid]).astype(np.int32)
    cls = np.concatenate([np.full(n0, truth(0), np.uint8), np.full(n1, truth(1), np.uint8), cls]).astype(np.uint8)
    d = Design("pool_growth_product", 4, 2, [(0, var, qid, cls), small[1]], R.nq, [(0, 1), (2, 3)])
    d.big_entries = N
    return d


# ------------------------------------------------------------------------------------------------ hand-built read lists for phz_tally_import + phz_hap_counts (mode 2 directly)
def mixer(x):
    """the 32-bit mixer the tables hash QNAME ids with, restated as a design tool"""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x


COLLIDING = ((200, 240), (1500, 1800), (3000, 3500))          # (distinct ids, entries): a wave with a 512-slot table, a workgroup with 4,096 LDS slots, one with 8,192 pool slots
BIG_QID = 2 ** 31 - 1


def colliding_ids(n_distinct, n_entries, start):
    """n_entries entries over n_distinct ids that ALL hash into the last 16 slots of the table a list of n_entries gets: linear probing wraps at the mask"""
    cap = rr.table_slots(n_entries)
    ids = np.zeros(0, np.int64); lo = start
    while len(ids) < n_distinct:
        cand = np.arange(lo, lo + (1 << 20), dtype=np.int64); lo += 1 << 20
        ids = np.concatenate([ids, cand[(mixer(cand) & np.uint64(cap - 1)) >= np.uint64(cap - 16)]])
    ids = ids[:n_distinct]
    rng = np.random.default_rng(n_distinct)
    return np.concatenate([ids, rng.choice(ids, size=n_entries - n_distinct)])[rng.permutation(n_entries)]


@functools.lru_cache(maxsize=None)
def direct_lists():
    """{"nv", "nb", "lists": {(variant, allele, BAM): entries}, "named": {name: list key}}: the boundary sizes (random ids, half of them repeats), the two one-QNAME
    lists, the three colliding lists, a list that holds the largest id; the first list (0, 0, 0) and the last one are empty"""
    rng = np.random.default_rng(77)
    nb = 2
    lists = {}; named = {}
    v = 0

    def put(name, entries):
        nonlocal v
        v += 1
        key = (v, int(rng.integers(0, 2)), int(rng.integers(0, nb)))
        lists[key] = np.asarray(entries, dtype=np.int64); named[name] = key
    for S in BOUNDARY_SIZES[1:]:
        put("size_%d" % S, rng.integers(0, S // 2 + 1, size=S))
    for S in (rr.SEG_MID + 1, rr.SEG_LDS + 1):
        put("one_qname_%d" % S, np.full(S, 12345))
    for i, (nd, ne) in enumerate(COLLIDING):
        put("colliding_%d" % nd, colliding_ids(nd, ne, 1000 + (i << 24)))
    put("largest_id", [3, BIG_QID, 3, BIG_QID, 0])
    nv = v + 2
    assert (0, 0, 0) not in lists and (nv - 1, 1, nb - 1) not in lists
    return {"nv": nv, "nb": nb, "lists": lists, "named": named}


@functools.lru_cache(maxsize=None)
def direct_pool_list():
    """one list, one entry more than the table pool of phz_hap_counts holds as first reserved (2^17 + 1), next to two short ones"""
    N = rr.smallest_overflowing_segment(rr.HAP_POOL_BYTES)
    big = (np.arange(N, dtype=np.int64) * 11) % 70001
    return {"nv": 3, "nb": 1, "lists": {(0, 1, 0): np.asarray([5, 5, 6]), (1, 0, 0): big, (2, 0, 0): np.asarray([9])}, "named": {"pool": (1, 0, 0)}, "big_entries": N}


def csr_of(d):
    """(rl_start uint32, rl_qid int32, rl_list uint32) of a direct design: what phz_tally_import adopts"""
    nseg = d["nv"] * 2 * d["nb"]
    sizes = np.zeros(nseg, np.int64)
    for (v, k, b), e in d["lists"].items():
        sizes[(v * 2 + k) * d["nb"] + b] = len(e)
    rs = np.zeros(nseg + 1, np.uint32); np.cumsum(sizes, out=rs[1:])
    rq = np.zeros(int(rs[-1]), np.int32)
    for (v, k, b), e in d["lists"].items():
        s = (v * 2 + k) * d["nb"] + b
        rq[rs[s]:rs[s + 1]] = e
    return rs, rq, np.repeat(np.arange(nseg, dtype=np.uint32), sizes).astype(np.uint32)


def designs():
    """every engine design that runs on both builds, in the order the one-context sequence takes them: a small design right after the huge block"""
    return [size_classes(), huge_block(), one_qname(), blacklisted_pieces(), size_classes(), one_qname()]


def all_designs():
    seen = {}
    for d in designs():
        seen.setdefault(d.name, d)
    return list(seen.values())
