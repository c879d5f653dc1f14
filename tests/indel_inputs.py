"""Seeded inputs for K_map_general (--include_indels 1) whose reads CARRY the alleles of the table (test side, own code).

synth.make_variants(indel_frac=...) only renames table rows: its reads are never edited, so no read shows a deleted or an
inserted allele.  Here a read of the carrying haplotype takes the ALT at every variant under it -- an M base and a D run for a
deletion, an M base and an I run with the ALT's tail for an insertion, the ALT bases for a substitution -- and, independently of
the variants, gets noise I / D runs (also directly next to a variant, several per segment), N introns, soft clips at both ends,
= / X runs, base errors, N bases and qualities on both sides of any --baseq in use.

Everything is numpy with one seed per shape.  The reference base at a position is synth.ref_base(pos).
"""
import bisect
import dataclasses
import functools
from typing import List

import numpy as np
import torch

from phaser_amd import synth

SNP, DEL, INS, MNP = 0, 1, 2, 3
_CODE = {c: i for i, c in enumerate("ACGT")}
_GAPS = (synth.OP_I, synth.OP_D, synth.OP_N)


@dataclasses.dataclass
class VariantTable:
    chrom: str
    pos: np.ndarray               # int64, sorted, unique, 1-based
    kind: np.ndarray              # SNP / DEL / INS / MNP
    ref_text: List[str]
    alt_text: List[str]
    hap_alt: np.ndarray           # which haplotype (0 / 1) carries ALT
    swap: np.ndarray              # True: allele 0 of the mapper's allele pool is ALT (mapper-level tests only)
    a1_empty: np.ndarray = None   # True: the second allele string is empty (edge test)

    def __len__(self):
        return len(self.pos)

    @property
    def ref_len(self):
        return np.array([len(t) for t in self.ref_text], dtype=np.uint8)

    def alleles(self):
        a0 = [a if s else r for r, a, s in zip(self.ref_text, self.alt_text, self.swap)]
        a1 = [r if s else a for r, a, s in zip(self.ref_text, self.alt_text, self.swap)]
        if self.a1_empty is not None:
            a1 = ["" if e else a for a, e in zip(a1, self.a1_empty)]
        return a0, a1

    def allele_pool(self):
        """(allele_off int32 [2n+1], allele_bytes uint8): the layout phz_variants_general wants (one spare byte at the end, as the drop-in has)."""
        a0, a1 = self.alleles()
        off = [0]; blob = bytearray()
        for x, y in zip(a0, a1):
            blob += x.encode(); off.append(len(blob))
            blob += y.encode(); off.append(len(blob))
        return np.array(off, dtype=np.int32), np.frombuffer(bytes(blob) + b"\0", dtype=np.uint8).copy()

    def take(self, idx):
        idx = np.asarray(idx)
        pick = lambda xs: [xs[i] for i in idx.tolist()]
        return VariantTable(self.chrom, self.pos[idx], self.kind[idx], pick(self.ref_text), pick(self.alt_text), self.hap_alt[idx], self.swap[idx],
                            None if self.a1_empty is None else self.a1_empty[idx])

    def as_synth(self, unphased_frac=0.05, seed=0):
        """synth.Variants with REF / ALT texts (VCF rendering, product side): allele 0 is REF there, whatever `swap` says."""
        rng = np.random.default_rng(seed)
        unph = rng.random(len(self)) < unphased_frac
        gt = ["0/1" if u else ("1|0" if h == 0 else "0|1") for u, h in zip(unph.tolist(), self.hap_alt.tolist())]
        rsid = ["." if i % 9 == 4 else "rs%d" % (1000 + i) for i in range(len(self))]
        first = lambda ts: torch.tensor([_CODE[t[0]] for t in ts], dtype=torch.uint8)
        return synth.Variants(self.chrom, torch.from_numpy(self.pos.astype(np.int32)), first(self.ref_text), first(self.alt_text), gt,
                              torch.from_numpy(self.hap_alt.astype(np.uint8)), rsid, list(self.ref_text), list(self.alt_text))

    def table_text(self, v=None):
        """The mapper's variant table (generate_mapping_table, phaser.py:1402-1404) with REF,ALT alleles and the REF length."""
        v = v or self.as_synth()
        rows = []
        for i, p in enumerate(self.pos.tolist()):
            uid = "%s_%d_%s_%s" % (self.chrom, p, self.ref_text[i], self.alt_text[i])
            rows.append("\t".join([self.chrom, str(p), uid, v.rsid[i], self.ref_text[i] + "," + self.alt_text[i], str(len(self.ref_text[i])), v.gt[i], "None"]))
        return "\n".join(rows) + "\n"


@dataclasses.dataclass(frozen=True)
class Shape:
    name: str
    seed: int
    n: int                        # records
    span: int                     # POS is uniform in [start, start + span)
    var_gap: int                  # mean distance between variants (at least MIN_GAP)
    start: int = 20_000
    L: int = 100
    p_noise: float = 0.004        # per aligned base: a noise I / D / N event starts
    p_adj: float = 0.06           # after a variant: a noise I / D directly next to it
    err: float = 0.05
    n_rate: float = 0.004
    intron: tuple = (50, 3000)
    p_clip: float = 0.2
    p_mixed: float = 0.15         # records whose matches are written as runs of M, = and X


MIN_GAP = 5                       # > the longest REF (4): a carried deletion never swallows the next variant
REACH = 1 << 16                   # how far past start + span the reference bases and the variants go; introns stop before it

SHAPES = {s.name: s for s in [
    Shape("main", 7101, 16 * 1024 + 300, 1_000_000, 60, err=0.06),
    Shape("dense", 7102, 4 * 1024 + 513, 60_000, 12, intron=(50, 600)),                    # > 1024 variants under a tile's window
    Shape("manyop", 7103, 3 * 1024 + 5, 150_000, 40, p_noise=0.09, intron=(20, 400)),     # > 4 CIGAR words per record
    Shape("retry", 7104, 2048, 30_000, 14, p_noise=0.02, p_adj=0.25, err=0.08, intron=(50, 400)),   # calls > n/2 + 4096, text > 4096
    Shape("shifted", 7105, 3 * 1024, 150_000, 40, start=(1 << 30) + 12_345),              # coordinates beyond 2^30
]}


def ref_codes(lo, hi):
    return synth.ref_base(torch.arange(lo, hi, dtype=torch.int64)).numpy()


def make_table(rng, chrom, lo, hi, var_gap):
    """Sorted unique positions in [lo, hi): 40 % SNPs, 20 % deletions (REF = 2-4 reference bases, ALT = its first base), 20 % insertions
    (REF = one base, ALT = that base + 1-3 bases), 20 % same-length substitutions of 2-3 bases."""
    gaps = MIN_GAP + rng.geometric(1.0 / max(1, var_gap - MIN_GAP), size=(hi - lo) // var_gap * 2 + 16)
    pos = lo + np.cumsum(gaps)
    pos = pos[pos < hi - 8].astype(np.int64)
    n = len(pos)
    kind = rng.choice(4, n, p=[0.4, 0.2, 0.2, 0.2])
    extra = rng.integers(1, 4, n)
    rnd = rng.integers(0, 4, (n, 4))
    shift = rng.integers(1, 4, (n, 4))
    ref = ref_codes(lo, hi + 8)
    ref_text = []; alt_text = []
    B = synth.BASES
    for i in range(n):
        p = int(pos[i]) - lo
        k = int(kind[i]); e = int(extra[i])
        if k == SNP:
            r = B[ref[p]]; a = B[(ref[p] + shift[i, 0]) % 4]
        elif k == DEL:
            r = "".join(B[ref[p + d]] for d in range(e + 1)); a = r[0]
        elif k == INS:
            r = B[ref[p]]; a = r + "".join(B[x] for x in rnd[i, :e])
        else:
            m = 2 + (e & 1)
            r = "".join(B[ref[p + d]] for d in range(m)); a = "".join(B[(ref[p + d] + shift[i, d]) % 4] for d in range(m))
        ref_text.append(r); alt_text.append(a)
    return VariantTable(chrom, pos, kind.astype(np.uint8), ref_text, alt_text, rng.integers(0, 2, n).astype(np.uint8), rng.random(n) < 0.5)


def make_reads(rng, vt, pos, hap, sh, ref_lo, ref, **fields):
    """One record per (pos[i], hap[i]), pos sorted.  `ref`: reference base codes from ref_lo on.  fields: flag / mapq / tlen / qid tensors."""
    n = len(pos); L = sh.L
    vpos = vt.pos.tolist(); nv = len(vpos)
    kind = vt.kind.tolist(); hap_alt = vt.hap_alt.tolist()
    refc = [[_CODE[c] for c in t] for t in vt.ref_text]; altc = [[_CODE[c] for c in t] for t in vt.alt_text]
    g_stop = ref_lo + len(ref) - 2 * L - 64              # no intron may carry a record past the reference array
    seq = rng.integers(0, 4, (n, L)).astype(np.uint8)    # clips and noise insertions keep these random bases
    words = []; coff = [0]; n_gaps = np.zeros(n, np.int64)
    OP_M, OP_I, OP_D, OP_N, OP_S = synth.OP_M, synth.OP_I, synth.OP_D, synth.OP_N, synth.OP_S
    match_ops = (synth.OP_M, synth.OP_EQ, synth.OP_X)
    p_noise = sh.p_noise; p_adj = sh.p_adj
    for r in range(n):
        row = seq[r]
        ops = []

        def put(op, k):
            if ops and ops[-1][0] == op:
                ops[-1][1] += k
            else:
                ops.append([op, k])
        lead = int(rng.integers(1, 9)) if rng.random() < sh.p_clip else 0
        trail = int(rng.integers(1, 9)) if rng.random() < sh.p_clip else 0
        mixed = rng.random() < sh.p_mixed
        mop = OP_M
        w = lead; end = L - trail
        if lead:
            put(OP_S, lead)
        g = int(pos[r]); h = int(hap[r])
        vi = bisect.bisect_left(vpos, g)
        to_noise = int(rng.geometric(p_noise))

        def noise(adjacent):
            nonlocal w, g, vi
            t = rng.random()
            if adjacent:
                t *= 0.7                                  # next to a variant: I or D only
            if t < 0.35:
                k = min(int(rng.integers(1, 4)), end - w - 1)
                if k >= 1:
                    put(OP_I, k); w += k
            elif t < 0.7:
                k = int(rng.integers(1, 5)); put(OP_D, k); g += k
                vi = bisect.bisect_left(vpos, g)
            else:
                k = int(rng.integers(sh.intron[0], sh.intron[1]))
                if g + k < g_stop:
                    put(OP_N, k); g += k
                    vi = bisect.bisect_left(vpos, g)
        while w < end:
            if mixed and rng.random() < 0.4:
                mop = match_ops[int(rng.integers(0, 3))]
            nxt = vpos[vi] if vi < nv else 1 << 62
            if nxt == g:
                room = end - w
                carry = h == hap_alt[vi]
                k = kind[vi]; rc = refc[vi]; ac = altc[vi]
                if carry and k == DEL and room >= 2:      # a base follows: no record ends on a gap
                    row[w] = ac[0]; put(mop, 1); w += 1
                    put(OP_D, len(rc) - 1); g += len(rc)
                elif carry and k == INS and room >= len(ac) + 1:
                    row[w] = ac[0]; put(mop, 1); w += 1
                    row[w:w + len(ac) - 1] = ac[1:]; put(OP_I, len(ac) - 1); w += len(ac) - 1
                    g += 1
                else:
                    src = ac if (carry and k in (SNP, MNP)) else rc
                    m = min(len(src), room)
                    row[w:w + m] = src[:m]; put(mop, m); w += m; g += m
                vi = bisect.bisect_left(vpos, g)
                if w < end - 1 and rng.random() < p_adj:
                    noise(True)
                continue
            if to_noise <= 0:
                to_noise = int(rng.geometric(p_noise))
                if lead < w < end - 1:
                    noise(False)
                    continue
            m = min(nxt - g, end - w, max(1, to_noise))
            row[w:w + m] = ref[g - ref_lo:g - ref_lo + m]; put(mop, m); w += m; g += m
            to_noise -= m
        if trail:
            put(OP_S, trail)
        assert sum(k for op, k in ops if op not in (OP_D, OP_N)) == L and ops[-1][0] not in _GAPS and ops[0][0] not in _GAPS
        words += [(k << 4) | op for op, k in ops]; coff.append(len(words))
        n_gaps[r] = sum(1 for op, k in ops if op in (OP_I, OP_D))
    err = rng.random((n, L)) < sh.err
    seq = np.where(err, (seq + rng.integers(1, 4, (n, L))) % 4, seq).astype(np.uint8)
    seq[rng.random((n, L)) < sh.n_rate] = 4
    qual = rng.choice(np.array([2, 11, 25, 37], dtype=np.uint8), (n, L), p=[0.04, 0.06, 0.15, 0.75])
    aln = (2 * L - 2 * err.sum(1) - n_gaps).astype(np.int32)
    z = torch.zeros(n, dtype=torch.int32)
    return synth.ReadBatch(vt.chrom, L, torch.from_numpy(np.asarray(pos, dtype=np.int32)), fields.get("flag", z), fields.get("mapq", torch.full((n,), 255, dtype=torch.uint8)),
                           fields.get("tlen", z), torch.from_numpy(aln), fields.get("qid", torch.arange(n, dtype=torch.int32)),
                           torch.tensor(coff, dtype=torch.int64), torch.tensor(words, dtype=torch.int64), torch.from_numpy(seq), torch.from_numpy(qual),
                           fields.get("qname_prefix", "q"))


def make(sh: Shape, chrom="chr1"):
    """-> (synth.ReadBatch, VariantTable) of one shape."""
    rng = np.random.default_rng(sh.seed)
    lo = sh.start - 64; hi = sh.start + sh.span + REACH
    vt = make_table(rng, chrom, sh.start - 32, hi - 512, sh.var_gap)
    ref = ref_codes(lo, hi)
    pos = np.sort(rng.integers(sh.start, sh.start + sh.span, sh.n))
    return make_reads(rng, vt, pos, rng.integers(0, 2, sh.n), sh, lo, ref), vt


@functools.lru_cache(maxsize=None)
def inputs(name):
    return make(SHAPES[name])


def make_pairs(sh: Shape, chrom, n_pairs, bam_seed, qname_prefix="q"):
    """Paired records (both mates of a template on one haplotype, proper-pair flags, TLEN) over the shape's table: what the product reads from a BAM.
    Templates are numbered the same way for every bam_seed, so two BAMs share their QNAMEs."""
    rng = np.random.default_rng(sh.seed)
    lo = sh.start - 64; hi = sh.start + sh.span + REACH
    vt = make_table(rng, chrom, sh.start - 32, hi - 512, sh.var_gap)
    ref = ref_codes(lo, hi)
    rng = np.random.default_rng([sh.seed, bam_seed])
    frag = rng.integers(sh.start, sh.start + sh.span, n_pairs)
    tl = np.maximum(sh.L, (rng.normal(250, 60, n_pairs)).astype(np.int64))
    hap = rng.integers(0, 2, n_pairs)
    pos = np.stack([frag, frag + tl - sh.L], 1).reshape(-1)
    tlen = np.stack([tl, -tl], 1).reshape(-1)
    flag = np.tile(np.array([0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80]), n_pairs)
    qid = np.repeat(np.arange(n_pairs), 2)
    order = np.argsort(pos, kind="stable")
    t32 = lambda a: torch.from_numpy(a[order].astype(np.int32))
    rb = make_reads(rng, vt, pos[order], np.repeat(hap, 2)[order], sh, lo, ref, flag=t32(flag), tlen=t32(tlen), qid=t32(qid), qname_prefix=qname_prefix)
    return rb, vt


def classify(text, allele0, allele1):
    """The kernel's contract for one call: 5 = the text is allele 0, else 6 = it is allele 1 (first match wins, list.index at phaser.py:1317),
    else 0..3 = a single ACGT base, else 4.  An empty allele string never matches."""
    if allele0 != "" and text == allele0:
        return 5
    if allele1 != "" and text == allele1:
        return 6
    if len(text) == 1 and text in "ACGT":
        return "ACGT".index(text)
    return 4


# ---------------------------------------------------------------------------------------------------- what a record looks like to the mapper
def layout(words):
    """Segments of one record's CIGAR words as split_read (read_variant_map.py:165-234) builds them: [(start, offs, ins, indel)] with
    start = genome offset of the segment from POS, offs[p] = read offset behind pseudo-read character p (-1: a 'D' placeholder),
    ins = {key: (read offset, length)} (the key is counted from POS, not from the segment: the reference's quirk; a later insertion under the
    same key replaces the earlier one), indel = the segment holds an I or a D."""
    segs = []
    start = 0; offs = []; ins = {}; indel = False
    rp = 0; gp = 0
    for w in words:
        op = w & 15; k = w >> 4
        if op in (synth.OP_M, synth.OP_EQ, synth.OP_X):
            offs.extend(range(rp, rp + k)); rp += k; gp += k
        elif op == synth.OP_N:
            segs.append((start, offs, ins, indel))
            gp += k; start = gp; offs = []; ins = {}; indel = False
        elif op == synth.OP_D:
            offs.extend([-1] * k); gp += k; indel = True
        elif op == synth.OP_I:
            ins[gp - 1] = (rp, k); rp += k; indel = True
        elif op == synth.OP_S:
            rp += k
    segs.append((start, offs, ins, indel))
    return segs


def candidates(segs, pos, vpos, ref_len):
    """[(variant, segment index, rs)] of one record: the variants the mapper looks at (0 <= rs and rs + ref_len <= len(pseudo read))."""
    out = []
    for si, (start, offs, ins, indel) in enumerate(segs):
        lo = pos + start; plen = len(offs)
        for v in range(int(np.searchsorted(vpos, lo)), int(np.searchsorted(vpos, lo + plen))):
            rs = int(vpos[v]) - lo
            if rs + int(ref_len[v]) <= plen:
                out.append((v, si, rs))
    return out


def call_offsets(seg, rs, rl):
    """Read offsets behind the characters of identify_allele's text (read_variant_map.py:236-258), and how many of them were spliced in."""
    start, offs, ins, indel = seg
    out = []; spliced = 0
    for p in range(rs, rs + rl):
        if offs[p] >= 0:
            out.append(offs[p])
        if p in ins:
            x, k = ins[p]
            out.extend(range(x, x + k)); spliced += k
    return out, spliced


def expected(oracle_dir, rb, vt, baseq):
    """The C oracle on (rb, vt) with the table's REF lengths -> (read_idx, var_idx, code per classify(), texts)."""
    from helpers import oracle_map_readbatch
    o_r, o_v, _, o_t = oracle_map_readbatch(oracle_dir, rb, vt.pos, baseq, ref_len=vt.ref_len)
    a0, a1 = vt.alleles()
    code = np.array([classify(t, a0[v], a1[v]) for t, v in zip(o_t, o_v.tolist())], dtype=np.uint8)
    return o_r, o_v, code, o_t
