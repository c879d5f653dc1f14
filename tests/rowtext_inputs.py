"""Designed inputs for the text writers of the row stage (phaser_amd/csrc/phz_rowsdev.hip: the sinks SCount / SWrite / WCount / WWrite, k_mem_rec, the row functions,
k_row_len / k_row_write / k_row_wave_len / k_row_wave_write, the closed-form allele_config offsets k_cfg_chunks / k_cfg_prefix / k_cfg_prefix_wave / k_cfg_write):
one deterministic builder per named design.  What the other designed suites keep fixed -- VCF text that is always rs<N>, A/G, 0|1 or 1|0 at 1000 + 40 v -- is what
varies here: string lengths, digit counts, genotype kinds, block sizes around 16 and around the multiples of 64.

A design holds its call lines in the `saved` form of tests/tally_inputs.py, its own VCF text, the names of its BAMs and QNAMEs, the blocks it is BUILT to give, its
blacklist, and the option sets it is to be run with.  Blocks are chains: a few reads per adjacent pair of members, every read carrying one haplotype of a fixed truth,
so every pair test has p = 1 and a clean component stays one block whatever its size.  The class 0 / 1 of a call line is the index into the variant's own allele pair
(the individual's two alleles in allele-index order: GT 2|1 with ALT C,G has the pair (C, G)).  IDs are unique and REF differs from every ALT."""
import functools

import numpy as np

from tally_inputs import Case

# ---- mirrors of phaser_amd/csrc/phz_rowsdev.hip (change both): block rows of more members than ROW_WAVE_MIN are formatted by a wave, 64 members a round;
# rows per workgroup and bytes of the LDS stage of every text the writers stage (launch_rows); a row range is staged when its bytes + its misalignment (< 16) fit
ROW_WAVE_MIN = 16
WAVE = 64
LAUNCH = {"conn": (256, 24 * 1024), "hap": (128, 32 * 1024), "ase": (64, 16 * 1024), "allelic": (256, 24 * 1024), "single_ase": (256, 32 * 1024),
          "single_hap": (256, 32 * 1024), "cfg": (128, 12 * 1024)}
WIDE = 65536          # a member with a uid, ID or allele of this many bytes or more is read through the pools (MemRec::wide)

HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"
# member kinds: (REF, ALT, GT, ID is '.')
KINDS = {"0|1": ("A", "G", "0|1", False), "1|0": ("A", "G", "1|0", False), "1|2": ("A", "C,G", "1|2", False), "2|1": ("A", "C,G", "2|1", False),
         "0|2": ("A", "C,G", "0|2", False), "0/1": ("A", "G", "0/1", False), "dot": ("A", "G", "0|1", True)}
BOTH_ALT = ("1|2", "2|1")


class Variant:
    def __init__(self, chrom, pos, vid, ref, alt, gt, kind=None):
        self.chrom = chrom; self.pos = pos; self.id = vid; self.ref = ref; self.alt = alt; self.gt = gt; self.kind = kind or gt
        every = [ref] + alt.split(",")
        assert len(set(every)) == len(every)
        idx = sorted(set(int(x) for x in gt if x.isdigit()))
        assert len(idx) == 2
        self.alleles = [every[i] for i in idx]
        self.uid = "_".join([chrom, str(pos)] + every)
        self.rsid = self.uid if vid == "." else vid
        self.phased = "|" in gt

    def vcf_line(self):
        return "%s\t%d\t%s\t%s\t%s\t.\tPASS\t.\tGT\t%s\n" % (self.chrom, self.pos, self.id, self.ref, self.alt, self.gt)


class Builder:
    """variants per chromosome (ascending positions), reads per (chromosome, BAM): (first variant, QNAME id, haplotype, variants); truth[v] = the index into v's allele
    pair that haplotype 0 carries"""

    def __init__(self, name, chroms, n_bams):
        self.name = name; self.chroms = list(chroms); self.n_bams = n_bams
        self.vars = {c: [] for c in chroms}; self.truth = {c: [] for c in chroms}
        self.reads = {c: [[] for _ in range(n_bams)] for c in chroms}; self.nq = {c: 0 for c in chroms}
        self.blocks = []; self.black = []

    def var(self, chrom, pos, vid, ref, alt, gt, kind=None, truth=None):
        vs = self.vars[chrom]
        assert not vs or vs[-1].pos < pos, (chrom, pos)
        v = len(vs)
        vs.append(Variant(chrom, pos, vid, ref, alt, gt, kind))
        self.truth[chrom].append(((v * v + v // 2) & 1) if truth is None else truth)
        return v

    def kind(self, chrom, pos, vid, kind, truth=None):
        ref, alt, gt, dot = KINDS[kind]
        return self.var(chrom, pos, "." if dot else vid, ref, alt, gt, kind, truth)

    def read(self, chrom, bam, hap, variants, n=1):
        for _ in range(n):
            self.reads[chrom][bam].append((min(variants), self.nq[chrom], hap, list(variants)))
            self.nq[chrom] += 1

    def chain(self, chrom, members, per_pair=((0, 0), (0, 1)), black=()):
        """a block: for every adjacent pair of members one read per (BAM, haplotype) of per_pair (a callable gives them per pair index)"""
        members = list(members)
        for i in range(len(members) - 1):
            for bam, hap in (per_pair(i) if callable(per_pair) else per_pair):
                self.read(chrom, bam, hap, members[i:i + 2])
        self.blocks.append((chrom, members))
        self.black += [(chrom, members[t]) for t in black]

    def design(self, options, load=None, note=""):
        return Design(self, options, load or {}, note)


class Design:
    def __init__(self, b, options, load, note):
        self.name = b.name; self.n_bams = b.n_bams; self.note = note; self.options = options; self.load = load
        self.chrom_list = list(b.chroms); self.vars = b.vars; self.truth = b.truth
        chroms = []
        for c in b.chroms:
            shards = []
            for bam in range(b.n_bams):
                reads = sorted(b.reads[c][bam], key=lambda r: r[0])          # stable: reads with the same first variant stay in the order they were added
                if not reads:
                    continue
                var = [v for _, q, h, vs in reads for v in vs]; qid = [q for _, q, h, vs in reads for v in vs]
                cls = [b.truth[c][v] ^ h for _, q, h, vs in reads for v in vs]
                shards.append((bam, np.asarray(var, np.int32), np.asarray(qid, np.int32), np.asarray(cls, np.uint8)))
            chroms.append((c, len(b.vars[c]), shards))
        self.case = Case(b.name, chroms, b.n_bams, [max(1, b.nq[c]) for c in b.chroms])
        self.saved = self.case.saved
        self.saved["qnames"] = {c: ["%sq%d" % (c, i) for i in range(max(1, b.nq[c]))] for c in b.chroms}
        self.vcf_text = HEAD + "".join(v.vcf_line() for c in b.chroms for v in b.vars[c])
        self.bam_names = ["bam%d" % i for i in range(b.n_bams)]
        self.blocks = [(c, list(m)) for c, m in b.blocks]
        self.black = frozenset(b.black)
        self.blacklist = frozenset("%s_%d" % (c, b.vars[c][v].pos) for c, v in b.black)

    @property
    def n_lines(self):
        return self.case.n_lines

    def block_uids(self):
        """the declared blocks as sorted tuples of uids"""
        return sorted(tuple(self.vars[c][v].uid for v in m) for c, m in self.blocks)

    def call_texts(self, bam):
        """the mapper's call file of a BAM per chromosome (read_variant_map.py:117), what oracle/phasing_oracle.py reads"""
        out = []
        for c in self.chrom_list:
            R = self.saved["tally"][c]; vs = self.vars[c]; qn = self.saved["qnames"][c]
            rows = []
            for b, base, n in R["bam_offsets"]:
                if b != bam:
                    continue
                sl = slice(base, base + n)
                rows += ["%s\t%s\t%s\t%s\t0\t%s\tNone\n" % (qn[q], vs[v].uid, vs[v].id, vs[v].alleles[k], vs[v].gt)
                         for v, q, k in zip(R["line_var"][sl].tolist(), R["line_qid"][sl].tolist(), R["line_cls"][sl].tolist())]
            out.append("".join(rows))
        return out


def _cycle(kinds, n, forced=None):
    out = [kinds[i % len(kinds)] for i in range(n)]
    for t, k in (forced or {}).items():
        out[t] = k
    return out


# ------------------------------------------------------------------------------------------------ genotypes
GENOTYPE_BLOCKS = (
    # name, size, kinds of its members, truth (None: mixed)
    [("mixed_%d" % n, n, _cycle(list(KINDS), n, {0: "1|2", n // 2: "2|1", n - 1: "1|2"}), None) for n in (2, ROW_WAVE_MIN, ROW_WAVE_MIN + 1, WAVE + 1)] +
    [("only_both_alt_%d" % n, n, _cycle(list(BOTH_ALT), n), None) for n in (3, ROW_WAVE_MIN + 1)] +
    [("no_both_alt_%d" % n, n, _cycle([k for k in KINDS if k not in BOTH_ALT], n), None) for n in (ROW_WAVE_MIN, ROW_WAVE_MIN + 1)] +
    [("hap_a_is_ref_%d" % n, n, _cycle([k for k in KINDS if k not in BOTH_ALT], n), 0) for n in (ROW_WAVE_MIN, ROW_WAVE_MIN + 1)])


@functools.lru_cache(maxsize=None)
def genotypes():
    """One BAM.  Blocks of 2, 16 (a thread formats their rows), 17 and 65 members (a wave) over the seven member kinds with a 1|2 / 2|1 member first, in the middle and
    last; blocks of 3 and 17 of nothing but such members (no member whose haplotype-B allele is the reference: NB = 0); blocks of 16 and 17 without one; blocks of 16 and
    17 whose haplotype A carries the reference allele on every member (the block's first member gives haplotype A its first allele: truth 0 throughout); one singleton
    of every kind.  Run with --unique_ids 0 and 1."""
    b = Builder("genotypes", ["chrG"], 1)
    at = 0
    for name, n, kinds, truth in GENOTYPE_BLOCKS:
        m = [b.kind("chrG", 500 + 37 * (at + t), "g%d" % (at + t), kinds[t], truth) for t in range(n)]
        at += n
        b.chain("chrG", m)
        s = b.kind("chrG", 500 + 37 * at, "g%d" % at, list(KINDS)[len(b.blocks) % len(KINDS)]); at += 1          # a singleton between two blocks
        b.read("chrG", 0, 0, [s], 2); b.read("chrG", 0, 1, [s], 3)
    for k in KINDS:
        s = b.kind("chrG", 500 + 37 * at, "g%d" % at, k); at += 1
        b.read("chrG", 0, 0, [s], 2); b.read("chrG", 0, 1, [s], 1)
    return b.design([{}, {"unique_ids": 1}])


# ------------------------------------------------------------------------------------------------ block sizes
BLOCK_SIZES = (2, 3, 16, 17, 63, 64, 65, 127, 128, 129, 193)


@functools.lru_cache(maxsize=None)
def block_sizes():
    """Two BAMs, chains of 2 ... 193 members in one pass: thread rows and wave rows in one file, several blocks in the list of big blocks.  BAM 0 has a read of each
    haplotype on every pair, BAM 1 one read on every third pair (some blocks have no row of BAM 1); a singleton between the blocks.  Run plain and with
    --haplo_count_bam_exclude 1."""
    b = Builder("block_sizes", ["chrB"], 2)
    at = 0
    for n in BLOCK_SIZES:
        m = [b.var("chrB", 1000 + 40 * (at + t), "rs%d" % (at + t), "A", "G", "0|1" if (at + t) % 3 else "1|0") for t in range(n)]
        at += n
        b.chain("chrB", m, lambda i: [(0, 0), (0, 1)] + ([(1, i & 1)] if i % 3 == 0 and n != 3 else []))
        s = b.var("chrB", 1000 + 40 * at, "rs%d" % at, "A", "G", "0|1"); at += 1
        b.read("chrB", at % 2, 0, [s], 2); b.read("chrB", 0, 1, [s], 1)
    return b.design([{}, {"haplo_count_bam_exclude": [0]}])


# ------------------------------------------------------------------------------------------------ blacklisted members over the 64-lane rounds of the wave sinks
def blacklist_patterns(n):
    last = WAVE * ((n - 1) // WAVE)
    return {"first_round": range(WAVE), "middle_round": range(WAVE, 2 * WAVE), "last_partial_round": range(last, n), "all_but_one": [t for t in range(n) if t != n // 2],
            "exactly_one": [n // 3], "every_second": range(0, n, 2)}


@functools.lru_cache(maxsize=None)
def blacklist_rounds():
    """One BAM, blocks of 129 and 193 members (three and four rounds of 64 lanes, the last of one member) with the blacklist patterns of blacklist_patterns(): the
    filters `live` and `black` of RowAse's joins leave whole rounds empty (tk == 0), start a round with and without members placed before it.  One read per pair,
    haplotypes alternating.  Run with --output_read_ids 0 and 1."""
    b = Builder("blacklist_rounds", ["K"], 1)
    at = 0
    b.patterns = []
    for n in (129, 193):
        for name, black in blacklist_patterns(n).items():
            m = [b.var("K", 10 + 3 * (at + t), "r%d" % (at + t), "A", "G", "0|1" if (at + t) % 3 else "1|0") for t in range(n)]
            at += n
            b.chain("K", m, lambda i: [(0, i & 1)], black=list(black))
            b.patterns.append((name, n, sorted(black)))
    d = b.design([{"output_read_ids": 0}, {"output_read_ids": 1}])
    d.patterns = b.patterns
    return d


# ------------------------------------------------------------------------------------------------ string lengths and digit counts
POSITIONS = (1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999, 1000000000, 2147483000)
COUNT_PAIRS = ((9, 10), (99, 100), (999, 1000))


def _bases(n, seed):
    return "".join("ACGT"[x] for x in np.random.default_rng(seed).integers(0, 4, size=n).tolist())


@functools.lru_cache(maxsize=None)
def string_lengths():
    """One BAM, 100 variants: IDs of every length 1 - 24, REF alleles of every length 1 - 40 (ALT one base) and ALT alleles of every length 1 - 40 (REF one base), at
    positions of 1 - 10 digits (1, 9, 10, 99, 100 ... 2,147,483,000; the variant at position 1 is a singleton: its row of haplotypes.txt starts at 0).  Blocks of four
    (a thread) over the first 48, a block of 20 (a wave), singletons.  Then three two-variant blocks and three singletons with 9 / 10, 99 / 100 and 999 / 1,000 reads on
    their two haplotypes / alleles."""
    b = Builder("string_lengths", ["chrL"], 1)
    n = 80
    pos = sorted(set(POSITIONS[:-1]) | set(2000 + 37 * i for i in range(n + 7 - len(POSITIONS))))[:n + 6]
    vs = []
    for i in range(n):
        k = i % 40 + 1
        vid = chr(ord("a") + i // 24) + "x" * (i % 24)                      # lengths 1 - 24, unique
        ref, alt = (_bases(k, i), "T") if i < 40 else ("T", _bases(k, i))
        if k == 1:
            ref, alt = ("C", "T") if i < 40 else ("T", "C")
        vs.append(b.var("chrL", pos[i], vid, ref, alt, ("0|1", "1|0", "0/1")[i % 3]))
    single = [0, 5, 53, 79]
    rest = [v for v in vs if v not in single]
    for k in range(0, 48, 4):
        b.chain("chrL", rest[k:k + 4])
    b.chain("chrL", rest[48:68])
    for k in range(68, len(rest), 2):
        b.chain("chrL", rest[k:k + 2])
    for s in single:
        b.read("chrL", 0, 0, [s], 1 + s % 3); b.read("chrL", 0, 1, [s], 2)
    for i, (n0, n1) in enumerate(COUNT_PAIRS):
        m = [b.var("chrL", pos[n + 2 * i + t], "cnt%d" % (2 * i + t), "A", "G", "0|1") for t in range(2)]
        b.read("chrL", 0, 0, m, n0); b.read("chrL", 0, 1, m, n1)
        b.blocks.append(("chrL", m))
    for i, (n0, n1) in enumerate(COUNT_PAIRS):
        s = b.var("chrL", 1100000000 + i if i < 2 else POSITIONS[-1], "one%d" % i, "A", "G", "1|0")
        b.read("chrL", 0, 0, [s], n0); b.read("chrL", 0, 1, [s], n1)
    return b.design([{}], load={"include_indels": 1})


# ------------------------------------------------------------------------------------------------ staged and unstaged workgroups in one file
OVERFLOW_GROUP = 256          # blocks / singletons per section: a multiple of every ROWS of LAUNCH, so that no workgroup mixes short and long names


@functools.lru_cache(maxsize=None)
def stage_overflow():
    """One BAM, one chromosome, four sections of variants in this order: 256 two-member blocks and 512 singletons with short names, then 256 two-member blocks and 512
    singletons whose ALT is an insertion of 40 - 200 bases.  Every text the writers stage then has workgroups whose rows fit the stage (the short sections) and workgroups
    whose rows do not (the long ones); tests/test_rowtext_limits.py computes which from the row lengths of the oracle's text."""
    b = Builder("stage_overflow", ["chrO"], 1)
    at = 0

    def var(long_):
        nonlocal at
        alt = "A" + _bases(40 + (at * 37) % 161, at) if long_ else "G"
        v = b.var("chrO", 100 + 3 * at, "s%d" % at, "A", alt, "0|1" if at % 3 else "1|0")
        at += 1
        return v
    for long_ in (False, True):
        for k in range(OVERFLOW_GROUP):
            b.chain("chrO", [var(long_), var(long_)], [(0, k & 1)])
        for k in range(2 * OVERFLOW_GROUP):
            b.read("chrO", 0, k & 1, [var(long_)])
    return b.design([{}], load={"include_indels": 1})


# ------------------------------------------------------------------------------------------------ strings on both sides of 65,536 bytes
WIDE_KINDS = (("uid_65535", WIDE - 1), ("uid_65536", WIDE), ("allele_70000", None))


@functools.lru_cache(maxsize=None)
def wide_members():
    """One BAM.  Three kinds of long variant -- a uid of exactly 65,535 bytes (the largest the 16-bit lengths of a member record hold: not wide), a uid of exactly
    65,536 (wide), an ALT allele of 70,000 bytes -- each as the middle member of a three-member block, as a member of one block of 17 (first, ninth and last; the
    65,536 one there with ID '.', so that its rsid is as long) and as a singleton."""
    b = Builder("wide_members", ["chrW"], 1)
    at = 0
    b.wide = []

    def short():
        nonlocal at
        at += 1
        return b.var("chrW", 1000 + 3 * at, "w%d" % at, "A", "G", "0|1" if at % 3 else "1|0")

    def wide(kind, target, dot=False):
        nonlocal at
        at += 1
        pos = 1000 + 3 * at
        n = 70000 if target is None else target - len("chrW_%d_A_" % pos)
        v = b.var("chrW", pos, "." if dot else "w%d" % at, "A", "A" + _bases(n - 1, at), "0|1" if at % 2 else "1|0", kind=kind)
        b.wide.append((kind, v))
        return v
    for kind, target in WIDE_KINDS:
        b.chain("chrW", [short(), wide(kind, target), short()])
    m = []
    for t in range(ROW_WAVE_MIN + 1):
        where = {0: 0, 8: 1, ROW_WAVE_MIN: 2}.get(t)
        m.append(short() if where is None else wide(*WIDE_KINDS[where], dot=(where == 1)))
    b.chain("chrW", m)
    for kind, target in WIDE_KINDS:
        s = wide(kind, target)
        b.read("chrW", 0, 0, [s], 2); b.read("chrW", 0, 1, [s], 1)
    d = b.design([{}], load={"include_indels": 1})
    d.wide = b.wide
    return d


# ------------------------------------------------------------------------------------------------ chromosomes without blocks between chromosomes with blocks
@functools.lru_cache(maxsize=None)
def chromosome_gaps():
    """Four chromosomes with names of different lengths: blocks of 3 and 17 and a singleton; covered singletons only (no block: its allele_config segment is empty and
    the next chromosome's starts at the byte base of ITS first block); blocks of 2 and 18 and a singleton; variants without a single call line."""
    chroms = ["1", "chr2", "chrom3", "c4"]
    b = Builder("chromosome_gaps", chroms, 1)
    for c, sizes in (("1", (3, ROW_WAVE_MIN + 1)), ("chr2", ()), ("chrom3", (2, ROW_WAVE_MIN + 2)), ("c4", ())):
        at = 0
        for n in sizes:
            m = [b.var(c, 700 + 11 * (at + t), "%sv%d" % (c, at + t), "A", "G", "0|1" if (at + t) % 3 else "1|0") for t in range(n)]
            at += n
            b.chain(c, m)
        for k in range(3):
            s = b.var(c, 700 + 11 * at, "%sv%d" % (c, at), "A", "G", "1|0"); at += 1
            if c != "c4":
                b.read(c, 0, 0, [s], 1 + k); b.read(c, 0, 1, [s], 2)
    return b.design([{}])


BUILDERS = (genotypes, block_sizes, blacklist_rounds, string_lengths, stage_overflow, wide_members, chromosome_gaps)
THREAD_FORMATTED = ("genotypes", "block_sizes", "string_lengths", "stage_overflow", "wide_members", "chromosome_gaps")      # designs with blocks of <= ROW_WAVE_MIN members


def all_designs():
    return [f() for f in BUILDERS]
