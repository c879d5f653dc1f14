"""What the kernels between the tally and the text writers of the row stage must compute on a design of tests/rowstage_inputs.py, in plain Python from the design's call
lines alone: no kernel code, no tiling, no hashing but the one documented hash of the pair-key set (rowstage_inputs.ps_hash).  Written from the reference's rules as
include/phz.h and SURVEY.md 8.1 cite them (phaser/phaser.py line numbers below); tests/test_rowstage_limits.py checks it against oracle/phasing_oracle.py on every design
before it checks a kernel against it.

    restate(d, option) -> Restated:
      noise                                   :610-632
      keys[(BAM, chromosome)]                 rule 2: variants by their first kept call line, per BAM that brings them (:1310, :558-561)
      rank[chromosome]                        rules 3 and 4: the keys of the connectivity map in order of first appearance (:1271-1283)
      pairs                                   the tested pairs in row order, oriented from the earlier key (:667-678), with cis / trans / other / sup / tot /
                                              configuration / p / verdict / phase_concordant (:1594-1654, :686-700)
      components                              the surviving graph's components in block order (:1861-1882), members by position
    block_facts(d, option, r, hap_text)       per final block of a haplotypes.txt: supporting / total pairs (:876-895), annotated phase, concordance, genome-wide phase,
                                              gwStat value and kind, the member whose maf is printed (:945-1025, :1086)
"""
import math

import numpy as np


class Pair:
    __slots__ = ("chrom", "a", "b", "cis", "trans", "other", "sup", "tot", "cfg", "p", "dropped", "conc")


class Restated:
    pass


def chrom_order(d):
    """the chromosomes in the order of the connectivity map: by the first BAM with a line on them, then VCF order (:573: read_vars gets a chromosome's key when a BAM
    first has a call file with lines for it)"""
    first = {}
    for c in d.chrom_list:
        for b in range(d.n_bams):
            if d.reads[c][b]:
                first[c] = b
                break
    return sorted(first, key=lambda c: (first[c], d.chrom_list.index(c))), first


def restate(d, option=0):
    from phaser_amd import rowsdev
    opts = d.options[option]
    cc = opts.get("cc_threshold", 0.01)
    r = Restated()
    # ---- per variant: QNAME sets per class; noise
    A = {}; O = {}
    match = mism = 0
    for c in d.chrom_list:
        for b in range(d.n_bams):
            for q, calls in d.reads[c][b]:
                for v, k in calls:
                    sets = A.setdefault((c, v), (set(), set())); O.setdefault((c, v), set())
                    if k < 2:
                        sets[k].add(q)
                    else:
                        O[(c, v)].add(q)
    lines = {}
    for c in d.chrom_list:
        for b in range(d.n_bams):
            for q, calls in d.reads[c][b]:
                for v, k in calls:
                    n = lines.setdefault((c, v), [0, 0])
                    n[0 if k < 2 else 1] += 1
    for m, mm in lines.values():
        if m > 0 and float(mm) / float(mm + m) < 0.05:
            match += m; mism += mm
    r.noise = float(mism) / (float(match + mism) * 2)
    prob = 1 - ((6 * r.noise) + (10 * math.pow(r.noise, 2)))
    # ---- rule 2: first appearance among kept call lines, BAM by BAM
    r.keys = {}; seen = set()
    for b in range(d.n_bams):
        for c in d.chrom_list:
            ks = r.keys[(b, c)] = []
            for q, calls in d.reads[c][b]:
                for v, k in calls:
                    if (c, v) not in seen:
                        seen.add((c, v)); ks.append(v)
    # ---- rules 3 and 4: the connectivity map
    r.chroms, r.first_bam = chrom_order(d)
    r.rank = {}; nb = {}
    for c in r.chroms:
        rank = r.rank[c] = []
        for b in range(d.n_bams):
            for q, calls in d.reads[c][b]:
                lst = [v for v, k in calls if k < 2]
                for x in lst:
                    for y in lst:
                        if y != x:
                            if (c, x) not in nb:
                                nb[(c, x)] = set(); rank.append(x)
                            nb[(c, x)].add(y)
    # ---- the pairs, oriented from the earlier key; the second variants of a key in rank order (the reference walks a set there: rule 6)
    r.pairs = []
    for c in r.chroms:
        at = {v: i for i, v in enumerate(r.rank[c])}
        done = set()
        for x in r.rank[c]:
            for y in sorted(nb[(c, x)], key=at.get):
                if (x, y) in done or (y, x) in done:
                    continue
                done.add((x, y))
                p = Pair(); p.chrom = c; p.a = x; p.b = y
                X, Y = A[(c, x)], A[(c, y)]; ox, oy = O[(c, x)], O[(c, y)]
                p.cis = len(X[0] & Y[0]) + len(X[1] & Y[1]); p.trans = len(X[1] & Y[0]) + len(X[0] & Y[1])
                p.other = len(ox & Y[0]) + len(ox & Y[1]) + len(X[0] & oy) + len(X[1] & oy) + len(ox & oy)
                p.sup = max(p.cis, p.trans); p.tot = p.cis + p.trans + p.other
                p.cfg = 0 if p.cis > p.trans else (1 if p.cis < p.trans else -1)
                if p.sup == 0:
                    p.p = 0
                elif p.tot - p.sup > 0:
                    p.p = float(rowsdev.binom_cdf(np.array([p.sup], np.int64), np.array([p.tot], np.int64), prob)[0])
                else:
                    p.p = 1
                p.dropped = p.p < cc
                va, vb = d.vars[c][x], d.vars[c][y]
                p.conc = "."
                if va.phased and vb.phased and p.cfg >= 0:
                    pa = phase_of(va, 0 if p.cfg == 0 else 1); pb = phase_of(vb, 0)          # (:1612-1622)
                    p.conc = 1 if pa == pb else 0
                r.pairs.append(p)
    r.tested = sorted({(p.sup, p.tot) for p in r.pairs if p.sup > 0 and p.tot - p.sup > 0})
    # ---- the surviving graph in block order
    r.components = []
    for c in r.chroms:
        left = {}
        for p in r.pairs:
            if p.chrom == c and not p.dropped:
                left.setdefault(p.a, set()).add(p.b); left.setdefault(p.b, set()).add(p.a)
        taken = set()
        for x in r.rank[c]:
            if x in left and x not in taken:
                comp = {x}; grow = [x]
                while grow:
                    for y in left[grow.pop()]:
                        if y not in comp:
                            comp.add(y); grow.append(y)
                taken |= comp
                r.components.append((c, sorted(comp)))
    r.members = {(c, v) for c, m in r.components for v in m}
    return r


def phase_of(var, k):
    """annotated phase of allele k of the variant's pair: its place in the GT string (:1455-1460), None for an unphased genotype"""
    if not var.phased:
        return None
    return [int(x) for x in var.gt.split("|")].index(k)          # (REF / ALT designs: the pair is (allele 0, allele 1))


def conn_rows(d, r):
    """the rows of variant_connections.txt in restated order"""
    out = []
    for p in r.pairs:
        vs = d.vars[p.chrom]
        out.append("\t".join(str(x) for x in (vs[p.a].uid, vs[p.b].uid, p.sup, p.tot, p.p, p.conc)))
    return out


def block_facts(d, option, r, hap_text):
    """-> per block row of the haplotypes.txt, in file order: dict(chrom, members, alleles (class on haplotype A), sup, tot, phase, conc, cor (genome-wide phase of haplotype
    A per member), stat (value), kind ('int1' / 'half' / 'mean' / 'maf'), maxmaf (member whose maf is the block's max_haplo_maf))"""
    opts = d.options[option]
    method = opts.get("gw_phase_method", 0)
    by_name = {(c, n): i for c in d.chrom_list for i, v in enumerate(d.vars[c]) for n in (v.uid, v.rsid)}
    kept = {}
    for p in r.pairs:
        if not p.dropped and p.cfg >= 0:
            kept[(p.chrom, p.a, p.b)] = p.cfg
    out = []
    for line in hap_text.split("\n")[1:-1]:
        f = line.split("\t")
        if int(f[4]) < 2:
            continue
        c = f[0]; vs = d.vars[c]
        mem = [by_name[(c, x)] for x in f[5].split(",")]
        alle = [vs[v].alleles.index(a) for v, a in zip(mem, f[6].split("|")[0].split(","))]
        cls = dict(zip(mem, alle))
        sup = tot = 0
        for (pc, a, b), cfg in kept.items():
            if pc == c and a in cls and b in cls:
                tot += 1
                sup += (cls[a] == cls[b]) == (cfg == 0)
        phase = [phase_of(vs[v], k) for v, k in zip(mem, alle)]
        known = [x for x in phase if x is not None]
        conc = 1 if len(set(known)) <= 1 else 0
        # the maf of a variant (:1445-1449): a float under --gw_phase_method 1 where the VCF has AF, else the int 0
        maf = [(vs[v].maf if method == 1 and vs[v].maf is not None else 0) for v in mem]
        stat = 0.5; kind = "half"; cor = list(phase); w = None
        if known:
            if len(set(phase)) == 1:                       # (an unknown member is a value of its own there: :962-966)
                stat = 1; kind = "int1"
            else:
                w = [sum(m for x, m in zip(phase, maf) if x == 0), sum(m for x, m in zip(phase, maf) if x == 1)]
                if method == 1 and sum(w) > 0:
                    stat = max(w) / sum(w); kind = "maf"
                    if w[0] != w[1]:
                        cor = [0 if w[0] > w[1] else 1] * len(mem)
                else:
                    mean = float(sum(known)) / len(known); kind = "mean"
                    if mean != 0.5:
                        cor = [0 if mean < 0.5 else 1] * len(mem)
                    stat = max(mean, 1 - mean)
        best = 0
        for i in range(len(mem)):
            if maf[i] > maf[best]:
                best = i
        out.append({"chrom": c, "members": mem, "alleles": alle, "sup": sup, "tot": tot, "phase": phase, "conc": conc, "cor": cor, "stat": stat, "kind": kind,
                    "maxmaf": mem[best], "maf_text": str(maf[best]), "w": w})
    return out


def stat_text(fact):
    return {"int1": "1", "half": "0.5"}.get(fact["kind"]) or repr(float(fact["stat"]))


def hap_row_fields(fact):
    """columns edges_supporting ... gw_confidence of the block's row of haplotypes.txt"""
    sym = lambda xs: "".join("-" if x is None else str(x) for x in xs)
    inv = lambda xs: [None if x is None else 1 - x for x in xs]
    return [str(float(fact["sup"])), str(float(fact["tot"])), sym(fact["phase"]) + "|" + sym(inv(fact["phase"])), str(fact["conc"]),
            sym(fact["cor"]) + "|" + sym(inv(fact["cor"])), stat_text(fact)]
