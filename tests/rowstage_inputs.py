"""Designed call lines for the kernels of the row stage that sit between the tally and block phasing and between phasing and the text writers
(phaser_amd/csrc/phz_rowsdev.hip: k_pair_keys / k_keep, the ordering stage order_variants_and_pairs / key_stage, k_blocks / k_blk_edges / k_blk_stats / k_vcf_blocks):
one deterministic builder per named design.  What tests/rowtext_inputs.py keeps fixed -- every pair test has p = 1, reads ascend, VCFs without AF -- is what varies here.

A read is one QNAME with a list of (variant, class) call lines in LINE order; class 0 / 1 is the index into the variant's allele pair, 2 an allele outside it (written
to the oracle's call file as 'T': REF is A, ALT is G throughout).  The lines of a (chromosome, BAM) stay in the order the reads were added, so a read whose first line sits
on its highest variant (mate 2 left of mate 1) makes that variant the first key of the connectivity map.  Every QNAME belongs to one BAM.  Every design has background
variants -- 20 + 20 ref / alt lines and one class-2 line, single-variant reads -- so that the estimated noise is > 0 and a pair with conflicting reads gets 0 < p < 1.

A design has the shape of rowtext_inputs.Design: saved, vcf_text, bam_names, options, call_texts(); its VCF carries INFO AF= where a variant has one, and call_texts()
writes str(maf) into the last column for an option set with gw_phase_method 1 (oracle/phasing_oracle.py variant_table_rows), 'None' otherwise."""
import functools

import numpy as np

from rowtext_inputs import HEAD, Variant
from tally_inputs import Case

OTHER_ALLELE = "T"


class AfVariant(Variant):
    def __init__(self, chrom, pos, vid, gt, af):
        Variant.__init__(self, chrom, pos, vid, "A", "G", gt)
        self.af = af                                  # the text after AF= (None: no AF in INFO)

    @property
    def maf(self):
        """phaser.py:1383-1397 for one ALT allele the individual carries: None without AF"""
        if self.af is None:
            return None
        f = float(self.af)
        return min(f, 1 - f)

    def vcf_line(self):
        return "%s\t%d\t%s\t%s\t%s\t.\tPASS\t%s\tGT\t%s\n" % (self.chrom, self.pos, self.id, self.ref, self.alt, "." if self.af is None else "DP=9;AF=" + self.af, self.gt)


class Builder:
    def __init__(self, name, chroms, n_bams):
        self.name = name; self.chroms = list(chroms); self.n_bams = n_bams
        self.vars = {c: [] for c in chroms}
        self.reads = {c: [[] for _ in range(n_bams)] for c in chroms}          # (QNAME id, [(variant, class)])
        self.nq = {c: 0 for c in chroms}
        self.marks = {}                                                         # names the tier-1 tests look up: variants, pairs, blocks

    def var(self, chrom, gt="0|1", af=None, pos=None):
        vs = self.vars[chrom]
        pos = (vs[-1].pos + 40 if vs else 1000) if pos is None else pos
        assert not vs or vs[-1].pos < pos
        vs.append(AfVariant(chrom, pos, "%s%s%d" % (self.name[0], chrom[-1], len(vs)), gt, af))
        return len(vs) - 1

    def read(self, chrom, bam, calls, n=1):
        for _ in range(n):
            self.reads[chrom][bam].append((self.nq[chrom], list(calls)))
            self.nq[chrom] += 1

    def pair(self, chrom, bam, a, b, cis=0, trans=0, other=0):
        """reads over a and b: `cis` with the same class on both (alternating 0,0 / 1,1), `trans` with opposite classes, `other` with class 2 on a and 0 / 1 on b"""
        for i in range(cis):
            self.read(chrom, bam, [(a, i & 1), (b, i & 1)])
        for i in range(trans):
            self.read(chrom, bam, [(a, i & 1), (b, 1 - (i & 1))])
        for i in range(other):
            self.read(chrom, bam, [(a, 2), (b, i & 1)])

    def chain(self, chrom, bam, members, truth, per_hap=1):
        """a clean block: per adjacent pair `per_hap` reads of haplotype A (truth[i] = class of member i on it) and of haplotype B"""
        for i in range(len(members) - 1):
            for h in (0, 1):
                self.read(chrom, bam, [(members[i], truth[i] ^ h), (members[i + 1], truth[i + 1] ^ h)], per_hap)

    def background(self, chrom, bam, n=3):
        out = []
        for _ in range(n):
            v = self.var(chrom)
            self.read(chrom, bam, [(v, 0)], 20); self.read(chrom, bam, [(v, 1)], 20); self.read(chrom, bam, [(v, 2)], 1)
            out.append(v)
        return out

    def design(self, options, env=None):
        return Design(self, options, env or [{}])


class Design:
    def __init__(self, b, options, env):
        self.name = b.name; self.n_bams = b.n_bams; self.options = options; self.env = env; self.marks = b.marks
        self.chrom_list = list(b.chroms); self.vars = b.vars; self.load = {}
        self.reads = b.reads
        chroms = []
        for c in b.chroms:
            shards = []
            for bam in range(b.n_bams):
                lines = [(v, q, k) for q, calls in b.reads[c][bam] for v, k in calls]
                if lines:
                    shards.append((bam, np.asarray([x[0] for x in lines], np.int32), np.asarray([x[1] for x in lines], np.int32), np.asarray([x[2] for x in lines], np.uint8)))
            chroms.append((c, len(b.vars[c]), shards))
        self.case = Case(b.name, chroms, b.n_bams, [max(1, b.nq[c]) for c in b.chroms])
        self.saved = self.case.saved
        self.saved["qnames"] = {c: ["%sq%d" % (c, i) for i in range(max(1, b.nq[c]))] for c in b.chroms}
        self.vcf_text = HEAD + "".join(v.vcf_line() for c in b.chroms for v in b.vars[c])
        self.bam_names = ["bam%d" % i for i in range(b.n_bams)]
        self.blacklist = frozenset()

    @property
    def n_lines(self):
        return self.case.n_lines

    @property
    def n_vars(self):
        return sum(len(self.vars[c]) for c in self.chrom_list)

    def load_kwargs(self, option):
        """what vcf.load_variants needs of an option set (the loader computes maf itself under gw_phase_method 1)"""
        return {k: v for k, v in self.options[option].items() if k == "gw_phase_method"}

    def call_texts(self, bam, option=0):
        """the mapper's call file of a BAM per chromosome (read_variant_map.py:117), what oracle/phasing_oracle.py reads: '' for a chromosome without a line of that BAM"""
        with_maf = self.options[option].get("gw_phase_method", 0) == 1
        out = []
        for c in self.chrom_list:
            vs = self.vars[c]; qn = self.saved["qnames"][c]
            out.append("".join("%s\t%s\t%s\t%s\t0\t%s\t%s\n" % (qn[q], vs[v].uid, vs[v].id, vs[v].alleles[k] if k < 2 else OTHER_ALLELE, vs[v].gt, str(vs[v].maf) if with_maf else "None")
                               for q, calls in self.reads[c][bam] for v, k in calls))
        return out


# ------------------------------------------------------------------------------------------------ verdicts
def design_noise(b):
    """phaser.py:610-632 on the builder's lines (the restatement computes it again from the call lines; the designs need it to choose a threshold)"""
    match = mism = 0
    for c in b.chroms:
        m = [0] * len(b.vars[c]); mm = [0] * len(b.vars[c])
        for per_bam in b.reads[c]:
            for q, calls in per_bam:
                for v, k in calls:
                    if k < 2:
                        m[v] += 1
                    else:
                        mm[v] += 1
        for x, y in zip(m, mm):
            if x > 0 and float(y) / float(y + x) < 0.05:
                match += x; mism += y
    return float(mism) / (float(match + mism) * 2)


def p_of(noise, sup, tot):
    """the double the row stage gets for a tested (supporting, total) pair: phaser.py:1649 through rowsdev.binom_cdf"""
    import math
    from phaser_amd import rowsdev
    return float(rowsdev.binom_cdf(np.array([sup], np.int64), np.array([tot], np.int64), 1 - ((6 * noise) + (10 * math.pow(noise, 2))))[0])


EQUAL_KEY = (7, 10)          # cc_threshold of the fourth option set = p of this (supporting, total); (6, 10) is the design's next smaller p


@functools.lru_cache(maxsize=None)
def verdicts():
    """One BAM, one chromosome.  Pairs of their own: (8, 10), (7, 10) kept and (6, 10) dropped at the default threshold -- the dropped one is the only pair of its two
    variants, which become singletons --, a pair without a conflicting read (p the int 1), a tie of 1 + 1 reads (kept: configuration -1) and a tie of 5 + 5 (dropped).  A chain
    of four whose middle pair is (6, 10): two components.  A triangle whose third side is (6, 10): the component survives whole.  Option sets: default, cc_threshold 0.0
    (nothing dropped), 1.0 (only p = 1 survives), and the exact double of p(7, 10): that pair is kept, (6, 10) dropped.
    A linked pair always has a supporting read (the read that links it carries ref / alt on both variants, phaser.py:1314 and :1637-1640), so p = the int 0 cannot be
    designed; a pair whose only common reads carry another allele on one side is no pair at all, which the design holds too ("only_other")."""
    b = Builder("verdicts", ["chrV"], 1)
    c = "chrV"
    b.background(c, 0)
    two = lambda: (b.var(c), b.var(c, "1|0"))
    m = b.marks
    m["kept_8_10"] = two(); b.pair(c, 0, *m["kept_8_10"], cis=8, trans=2)
    m["equal_7_10"] = two(); b.pair(c, 0, *m["equal_7_10"], cis=3, trans=7)
    m["dropped_6_10"] = two(); b.pair(c, 0, *m["dropped_6_10"], cis=6, trans=4)
    m["no_conflict"] = two(); b.pair(c, 0, *m["no_conflict"], trans=3)
    m["tie_kept"] = two(); b.pair(c, 0, *m["tie_kept"], cis=1, trans=1)
    m["tie_dropped"] = two(); b.pair(c, 0, *m["tie_dropped"], cis=5, trans=5)
    m["only_other"] = two(); b.pair(c, 0, *m["only_other"], other=2)
    m["with_other"] = two(); b.pair(c, 0, *m["with_other"], cis=7, trans=1, other=2)          # (7, 10) again, through other-class reads
    ch = [b.var(c) for _ in range(4)]
    m["bridge"] = ch
    b.pair(c, 0, ch[0], ch[1], cis=2); b.pair(c, 0, ch[1], ch[2], cis=6, trans=4); b.pair(c, 0, ch[2], ch[3], trans=2)
    tr = [b.var(c) for _ in range(3)]
    m["triangle"] = tr
    b.pair(c, 0, tr[0], tr[1], cis=2); b.pair(c, 0, tr[1], tr[2], cis=2); b.pair(c, 0, tr[0], tr[2], cis=6, trans=4)
    noise = design_noise(b)
    return b.design([{}, {"cc_threshold": 0.0}, {"cc_threshold": 1.0}, {"cc_threshold": p_of(noise, *EQUAL_KEY)}])


# ------------------------------------------------------------------------------------------------ the pair-key table
def ps_hash(key):
    """the finalizer of MurmurHash3 (fmix64) on a 64-bit key, low 32 bits: the hash of the (total << 32 | supporting) set"""
    M = (1 << 64) - 1
    k = key & M
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & M; k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & M; k ^= k >> 33
    return k & 0xFFFFFFFF


def home_slot(sup, tot, n_slots):
    return ps_hash((tot << 32) | sup) & (n_slots - 1)


def pair_table_keys(n):
    """n distinct (supporting, total) with conflicting reads, total <= 20: first three whose home slot among 16 is the last one (they collide, and two of them must wrap to
    slot 0 whatever the order of insertion), then the others in (total, supporting) order"""
    every = [(s, t) for t in range(2, 21) for s in range((t + 1) // 2, t)]
    last = [k for k in every if home_slot(k[0], k[1], 16) == 15][:3]
    assert len(last) == 3
    return last + [k for k in every if k not in last][:n - 3]


@functools.lru_cache(maxsize=None)
def pair_table(n_keys=16):
    """One BAM: n_keys pairs of variants, each with its own (supporting, total) of pair_table_keys(), and one more pair that repeats the first key.  Run with a table of 16
    slots (exactly full at 16 keys: PHZ_OK; at 17 PHZ_E_CAPACITY and one growth), of 64 and of the default size."""
    b = Builder("pair_table_%d" % n_keys, ["chrP"], 1)
    b.background("chrP", 0)
    keys = pair_table_keys(n_keys)
    for s, t in keys + keys[:1]:
        x, y = b.var("chrP"), b.var("chrP", "1|0")
        b.pair("chrP", 0, x, y, cis=s, trans=t - s)
    b.marks["keys"] = keys
    return b.design([{}], env=[{"PHZ_ROWS_PAIR_SLOTS": "16"}, {"PHZ_ROWS_PAIR_SLOTS": "64"}, {}])


# ------------------------------------------------------------------------------------------------ ordering
@functools.lru_cache(maxsize=None)
def ordering():
    """Three chromosomes in the VCF -- chrA, chrM without a single read, chrC -- and three BAMs; BAM 0 has no line on chrA (its blocks then follow chrC's, phaser.py:573).
    chrC, BAM 0: variants low0, low1 (a block) below hi0, hi1, hi2 (a block); the first read carries hi2 before hi0 (the highest variant is the first key: the pair
    (hi0, hi2) is turned round, and the block of the hi variants precedes the block of the low ones).  Covered variants that are never linked, variants without a line.
    chrA: a block seen by BAM 1 and BAM 2, a block whose variants appear in BAM 2 only.  Segments (BAM, chromosome) in table order: (0, A) (0, M) empty, (0, C) keys,
    (1, A) keys, (1, M) (1, C) empty, (2, A) keys, (2, M) empty, (2, C) keys."""
    A, M, C = "chrA", "chrM", "chrC"
    b = Builder("ordering", [A, M, C], 3)
    m = b.marks
    for _ in range(3):
        b.var(M)
    # chrC
    low = [b.var(C), b.var(C, "1|0")]
    m["uncovered"] = [(C, b.var(C))]
    hi = [b.var(C), b.var(C, "1|0"), b.var(C)]
    m["low"] = low; m["hi"] = hi
    b.read(C, 0, [(hi[2], 0), (hi[0], 0)]); b.read(C, 0, [(hi[2], 1), (hi[0], 1)])
    b.read(C, 0, [(hi[0], 0), (hi[1], 1)]); b.read(C, 0, [(hi[0], 1), (hi[1], 0)])
    b.chain(C, 0, low, [0, 1])
    m["unlinked"] = [(C, b.var(C))]
    b.read(C, 0, [(m["unlinked"][0][1], 0)], 2)
    b.background(C, 0)
    late = b.var(C)                                                              # covered by BAM 2 only, never linked: the one key of segment (2, chrC)
    m["bam2_only_single"] = (C, late)
    b.read(C, 2, [(late, 1)], 2); b.read(C, 2, [(low[0], 0), (low[1], 1)])
    # chrA
    a = [b.var(A), b.var(A), b.var(A, "1|0")]
    m["uncovered"].append((A, b.var(A)))
    z = [b.var(A), b.var(A)]
    m["a_block"] = a; m["bam2_only_block"] = z
    b.chain(A, 1, a, [0, 0, 1])
    u = b.var(A); m["unlinked"].append((A, u))
    b.read(A, 1, [(u, 1)], 3)
    b.read(A, 2, [(a[1], 0), (a[0], 0)])                                          # (line order: the higher variant first, in a later BAM: no new key)
    b.chain(A, 2, z, [0, 1])
    return b.design([{}])


# ------------------------------------------------------------------------------------------------ block statistics
# name -> per member (GT, AF text or None, class on haplotype A); the first member's class on haplotype A is 0 (phaser.py:2167 starts from its first allele).
# annotated phase of haplotype A on a member: its class for 0|1, 1 - class for 1|0, unknown for 0/1
STAT_BLOCKS = {
    "all_equal": [("0|1", "0.5", 0), ("1|0", "0.2", 1), ("0|1", "0.3", 0)],                          # phases 0 0 0: the int 1
    "none_phased": [("0/1", "0.1", 0), ("0/1", "0.2", 1), ("0/1", "0.3", 0)],                        # the literal 0.5
    "half": [("0|1", "0.25", 0), ("0|1", "0.75", 1)],                                                # phases 0 1: mean 0.5; maf 0.25 and 0.25: w0 == w1, and tied for max(maf)
    "two_thirds": [("0|1", "0.4", 0), ("0|1", "0.1", 1), ("1|0", "0.9", 0)],                         # phases 0 1 1: mean 2/3; w0 0.4 > w1 0.1 + (1 - 0.9)
    "one_third": [("0|1", "0.1", 0), ("1|0", "0.1", 1), ("0|1", "0.6", 1)],                          # phases 0 0 1: mean 1/3; w0 0.2 < w1 0.4
    "unknown_among_known": [("0|1", "0.3", 0), ("0/1", "0.45", 1), ("1|0", "0.3", 1), ("0/1", None, 0)],      # phases 0 - 0 -: not the int 1 but the float 1.0
    "no_weight": [("0|1", "0", 0), ("0|1", None, 1), ("1|0", None, 0), ("0/1", "1", 0)],              # phases 0 1 1 -: every maf 0: the mean; max(maf) tied between 0.0 and the int 0
    "no_weight_int_first": [("0|1", None, 0), ("0|1", "0", 1)],                                      # ... and with the int 0 first
}


@functools.lru_cache(maxsize=None)
def block_stats():
    """One BAM.  The clean chains of STAT_BLOCKS; a chain of three with a kept tie pair between its ends (inside one final block, not counted); four variants in a chain
    of cis pairs with a trans pair between its ends: a conflict, which --max_block_size 2 splits into two final blocks with two kept pairs between them (not counted).
    Option sets: default, --gw_phase_method 1, --max_block_size 2."""
    c = "chrS"
    b = Builder("block_stats", [c], 1)
    b.background(c, 0)
    for name, members in STAT_BLOCKS.items():
        vs = [b.var(c, gt, af) for gt, af, k in members]
        b.chain(c, 0, vs, [k for gt, af, k in members])
        b.marks[name] = vs
    t = [b.var(c, "0|1", "0.2"), b.var(c, "0|1", "0.3"), b.var(c, "1|0", "0.4")]
    b.chain(c, 0, t, [0, 0, 0]); b.pair(c, 0, t[0], t[2], cis=1, trans=1)
    b.marks["tie_inside"] = t
    s = [b.var(c, "0|1", "0.2"), b.var(c, "1|0", "0.3"), b.var(c, "0|1", "0.4"), b.var(c, "0|1", "0.1")]
    b.chain(c, 0, s, [0, 0, 0, 0]); b.pair(c, 0, s[0], s[3], trans=2)
    b.marks["split"] = s
    return b.design([{}, {"gw_phase_method": 1}, {"max_block_size": 2}])


def all_designs():
    return [verdicts(), pair_table(16), pair_table(17), ordering(), block_stats()]
