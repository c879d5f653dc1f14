"""phaser_cis_scan restated in plain Python (test infrastructure): U2 by counting over every (het, hom) pair, T as fractions.Fraction, the Philox stream and the
replicate orders by `sorted`, the tool's pipeline from the texts of its inputs.  Nothing here shares code with phaser_amd/cis_scan.py or the kernels; the GT
classes come from phaser_amd.cis_var._classify, which the issue names as their definition."""
import functools
import gzip
import math
import re
from fractions import Fraction

M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ the stream
def philox4x32_10(q, s, seed):
    c0, c1, c2, c3 = q & M32, (q >> 32) & M32, s & M32, (s >> 32) & M32
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        m0 = 0xD2511F53 * c0; m1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (m1 >> 32) ^ c1 ^ k0, m1 & M32, (m0 >> 32) ^ c3 ^ k1, m0 & M32
        k0 = (k0 + 0x9E3779B9) & M32; k1 = (k1 + 0xBB67AE85) & M32
    return (c0, c1, c2, c3)


def word(b, i, n, subseq, seed):
    at = b * n + i
    return philox4x32_10(at // 4, subseq, seed)[at % 4]


def replicate_order(b, n, subseq, seed):
    """ord_b: i = 0 .. n - 1 ascending by (w(b, i), i)"""
    return sorted(range(n), key=lambda i: (word(b, i, n, subseq, seed), i))


# ------------------------------------------------------------------------------------------------ one pair
def u2_count(het_vals, hom_vals):
    u = 0
    for x in het_vals:
        for y in hom_vals:
            if x > y:
                u += 2
            elif x == y:
                u += 1
    return u


def t_stat(u2, n1, n2):
    return Fraction((u2 - n1 * n2) ** 2, n1 * n2 * (n1 + n2 + 1))


# ------------------------------------------------------------------------------------------------ the scan
def scan_gene(cls_rows, covered, value, subseq, n_perm, seed):
    """cls_rows: the class rows of the gene's variants; covered: its covered samples, ascending; value[sample] = |aFC|.
    -> (n_het, n_hom, u2 per variant, u2_perm[b][variant] for the variants with a het and a hom, else None)"""
    n = len(covered)
    nh, nm, u2 = [], [], []
    for row in cls_rows:
        het = [s for s in covered if row[s] == 1]; hom = [s for s in covered if row[s] == 2]
        nh.append(len(het)); nm.append(len(hom))
        u2.append(u2_count([value[s] for s in het], [value[s] for s in hom]))
    sv = sorted(value[s] for s in covered)                             # the value that stays on each position
    perm = []
    for b in range(n_perm):
        o = replicate_order(b, n, subseq, seed)
        val_b = {covered[o[p]]: sv[p] for p in range(n)}
        perm.append([u2_count([val_b[s] for s in covered if row[s] == 1], [val_b[s] for s in covered if row[s] == 2]) if nh[v] and nm[v] else None
                     for v, row in enumerate(cls_rows)])
    return nh, nm, u2, perm


def best_and_exceed(nh, nm, u2, perm, min_het, min_hom, n_perm):
    """-> (best variant position or -1, exceed over the first n_perm replicates)"""
    testable = [v for v in range(len(nh)) if nh[v] >= min_het and nm[v] >= min_hom]
    if not testable:
        return -1, 0
    ts = {v: t_stat(u2[v], nh[v], nm[v]) for v in testable}
    best = max(testable, key=lambda v: (ts[v], -v))
    exceed = sum(1 for b in range(n_perm) if max(t_stat(perm[b][v], nh[v], nm[v]) for v in testable) >= ts[best])
    return best, exceed


# ------------------------------------------------------------------------------------------------ the tool's inputs
_CELL = re.compile(r"([0-9]+)\|([0-9]+)")


def read_text(path):
    with open(path, "rb") as f:
        raw = f.read()
    return (gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw).decode()


def vcf_records(text):
    """-> (sample names, [(chrom, pos, id, ref, alt, format list, sample fields)]) in file order"""
    names, recs = [], []
    for line in text.split("\n"):
        line = line.rstrip("\r")
        if line.startswith("#CHROM"):
            names = line.split("\t")[9:]
        elif line and not line.startswith("#"):
            f = line.split("\t")
            recs.append((f[0], int(f[1]), f[2], f[3], f[4], f[8].split(":") if len(f) > 8 else [], f[9:]))
    return names, recs


def gt_of(rec, names, sample):
    """GT text of `sample` in the record, None where the VCF, the record or FORMAT lacks it"""
    fmt, fields = rec[5], rec[6]
    if "GT" not in fmt:
        return None
    cols = [j for j, nm in enumerate(names) if nm == sample]
    if not cols or cols[-1] >= len(fields):
        return None
    sub = fields[cols[-1]].split(":")
    gi = fmt.index("GT")
    return sub[gi] if gi < len(sub) else ""


def classify(gt):
    """(class, alt on haplotype 2) by cis_var._classify and its phased test"""
    from phaser_amd.cis_var import _classify
    if gt is None or "|" not in gt:
        return 0, 0
    c, ai = _classify(gt)
    return c, (ai if c == 1 else 0)


def region_records(text, regions, samples):
    """the plain-Python reader of test 4: records inside a region (contig, lo, hi), once, file order -> [(chrom, pos, id, ref, alt, [codes])], code = class | alt2 << 2"""
    names, recs = vcf_records(text)
    out = []
    for rec in recs:
        if any(c == rec[0] and lo <= rec[1] <= hi for c, lo, hi in regions):
            codes = []
            for s in samples:
                c, a2 = classify(gt_of(rec, names, s))
                codes.append(c | (a2 << 2))
            out.append((rec[0], rec[1], rec[2], rec[3], rec[4], codes))
    return out


def median(v):
    v = sorted(v); n = len(v)
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2.0


def z_p(u2, n1, n2):
    from scipy.special import ndtr
    z = ((u2 - n1 * n2) / 2.0) / math.sqrt(n1 * n2 * (n1 + n2 + 1) / 12.0)
    return z, float(2 * ndtr(-abs(z)))


def fmt(x):
    return "NA" if x != x else repr(float(x))


def restate_tool(bed_text, vcf_text, map_text, window=100000, min_cov=8, pc=1, min_het=5, min_hom=5, perm=1000, seed=0, chrom="", fdr=0.05):
    """-> (rows of genes.txt as lists of strings without the q column, perm_p per row or None, pair rows [gene, var_id, pos, n_het, n_hom, z, p])"""
    ml = [l.rstrip("\r").split("\t") for l in map_text.split("\n") if l.strip("\r")]
    iv, ib = ml[0].index("vcf_sample"), ml[0].index("bed_sample")
    smap = {}
    for r in ml[1:]:
        smap[r[iv]] = r[ib]
    smap = list(smap.items())
    lines = [l for l in (l.rstrip("\r") for l in bed_text.split("\n")) if l]
    head = lines[0].split("\t")
    names, recs = vcf_records(vcf_text)
    rows, perm_ps, pairs = [], [], []
    for rownum, line in enumerate(lines[1:]):
        f = line.split("\t")
        if chrom != "" and f[0] != chrom:
            continue
        start, stop = int(f[1]), int(f[2])
        afc = {}
        for s, (vs, bs) in enumerate(smap):
            j = head.index(bs) if bs in head else -1
            m = _CELL.fullmatch(f[j]) if 4 <= j < len(f) else None
            if m is None or int(m.group(1)) + int(m.group(2)) >= 2 ** 31:
                continue
            a, b = int(m.group(1)), int(m.group(2))
            if a + b >= min_cov:
                afc[s] = math.log(float(a + pc) / float(b + pc), 2)
        covered = sorted(afc)
        value = {s: abs(afc[s]) for s in covered}
        mine = [r for r in recs if r[0] == f[0] and start + 1 - window <= r[1] <= stop + window]
        codes = [[classify(gt_of(r, names, vs)) for vs, _ in smap] for r in mine]
        cls_rows = [[c for c, _ in row] for row in codes]
        nh, nm, u2, pu2 = scan_gene(cls_rows, covered, value, rownum, perm, seed)
        best, exceed = best_and_exceed(nh, nm, u2, pu2, min_het, min_hom, perm)
        testable = [v for v in range(len(mine)) if nh[v] >= min_het and nm[v] >= min_hom]
        vid = lambda r: "%s_%d_%s_%s" % (r[0], r[1], r[3], r[4]) if r[2] == "." else r[2]
        for v in testable:
            z, p = z_p(u2[v], nh[v], nm[v])
            pairs.append([f[3], vid(mine[v]), str(mine[v][1]), str(nh[v]), str(nm[v]), fmt(z), fmt(p)])
        out = [f[3], f[0], f[1], f[2], str(len(covered)), str(len(testable))]
        if best < 0:
            out += ["NA"] * 9
            perm_ps.append(None)
        else:
            z, p = z_p(u2[best], nh[best], nm[best])
            hets = [(-afc[s] if codes[best][s][1] == 1 else afc[s]) for s in covered if codes[best][s][0] == 1]
            out += [vid(mine[best]), str(mine[best][1]), str(nh[best]), str(nm[best]), fmt(z), fmt(p), fmt(median(hets))]
            if perm > 0:
                pp = (1.0 + exceed) / (perm + 1.0)
                out += [str(exceed), fmt(pp)]
                perm_ps.append(pp)
            else:
                out += ["NA", "NA"]
                perm_ps.append(None)
        rows.append(out)
    return rows, perm_ps, pairs


def bh(ps):
    """Benjamini-Hochberg over the entries that are not None -> list with None kept"""
    idx = sorted((i for i, p in enumerate(ps) if p is not None), key=lambda i: ps[i])
    m = len(idx)
    q = [None] * len(ps)
    run = 1.0
    for rank in range(m, 0, -1):
        i = idx[rank - 1]
        run = min(run, ps[i] * m / rank)
        q[i] = run
    return q


# ------------------------------------------------------------------------------------------------ the designed call of test 1
DESIGN_S, DESIGN_V, DESIGN_P = 130, 48, 37
LEVELS = (0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0)


@functools.lru_cache(maxsize=None)
def designed_call():
    """-> dict: cls [V][S], per gene (covered list, value per sample, v_lo, v_hi, subseq); see tests/test_cis_scan.py for what it has to contain"""
    import random
    rnd = random.Random(20)
    S, V = DESIGN_S, DESIGN_V
    cls = []
    cls.append([1] * S); cls.append([2] * S); cls.append([0] * S)
    cls.append([1 if s == 7 else 2 for s in range(S)]); cls.append([2 if s == 9 else 1 for s in range(S)])
    while len(cls) < V:
        cls.append([0 if rnd.random() < 0.1 else rnd.choice((1, 2)) for _ in range(S)])
    cls[14] = list(cls[10])                                             # row 14 copies row 10: equal T, the first must win
    genes = []

    def gene(n, v_lo, v_hi, values=None):
        cov = sorted(rnd.sample(range(S), n))
        val = {s: (values[i] if values is not None else rnd.choice(LEVELS)) for i, s in enumerate(cov)}
        genes.append({"covered": cov, "value": val, "v_lo": v_lo, "v_hi": v_hi, "subseq": 3 * len(genes) + 1})

    for k, n in enumerate((0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 130)):
        if n in (3, 130):
            gene(n, 0, V)                                               # all variants
        else:
            gene(n, 4 * k, 4 * k + 10)                                  # ranges shared between neighbours (the emulation walks every pair in every replicate)
    gene(100, 0, V, [0.125 * (p if p < 60 else (60 if p <= 70 else p)) for p in range(100)])     # one run spans positions 60-70
    gene(90, 5, 17, [1.0] * 90)                                         # all tied
    gene(90, 5, 17, [0.01 * (p + 1) for p in range(90)])                # all distinct (ranges shared with the gene before)
    gene(80, 20, 20)                                                    # empty window
    gene(80, 11, 12)                                                    # one variant
    gene(70, 0, 3)                                                      # all het, all hom, all skip: no testable pair
    gene(120, 8, 16)                                                    # rows 10 and 14 are equal
    genes[-1]["value"] = {s: rnd.choice((2.0, 3.0) if cls[10][s] == 1 else (0.0, 0.25, 0.5)) for s in genes[-1]["covered"]}     # row 10 is the best
    return {"cls": cls, "genes": genes}


@functools.lru_cache(maxsize=None)
def designed_reference(seed=5):
    """the restated counts of the designed call at P = DESIGN_P, computed once: per gene (n_het, n_hom, u2, u2 of every replicate)"""
    d = designed_call()
    return [scan_gene(d["cls"][g["v_lo"]:g["v_hi"]], g["covered"], g["value"], g["subseq"], DESIGN_P, seed) for g in d["genes"]]
