"""Plain Python and numpy restatement of phaser_sample_match and of K_match's contract (include/phz.h, phz_sample_match); no product import.

K_match: every term is the correctly rounded value of r L_ref + fl(a L_alt), taken through fractions.Fraction and float(); the terms of a sample are added in
a Python loop over its entries, in entry order, vectorised over the donors only (one IEEE add per entry and donor, as the contract says)."""
import math
from fractions import Fraction

import numpy as np

VERDICTS = ("MATCH", "MISMATCH", "UNCLAIMED", "AMBIGUOUS", "SINGLE_DONOR", "LOW_SITES", "NO_SITES")
I32 = 2 ** 31 - 1


class Fatal(Exception):
    pass


def log_tables(error):
    return (math.log1p(-error), math.log(0.5), math.log(error)), (math.log(error), math.log(0.5), math.log1p(-error))


# ------------------------------------------------------------------------------------------------ K_match
def capped(ref, alt, cap):
    total = ref + alt
    if cap > 0 and total > cap:
        r = (ref * cap + total // 2) // total
        return r, cap - r
    return ref, alt


def entry_terms(ref, alt, cap, log_ref, log_alt, _memo={}):
    """-> (t_1, t_2, t_3): float(r L_ref + fl(a L_alt)) exactly rounded"""
    r, a = capped(ref, alt, cap)
    key = (r, a, log_ref, log_alt)
    t = _memo.get(key)
    if t is None:
        t = _memo[key] = tuple(float(Fraction(r) * Fraction(log_ref[g]) + Fraction(float(a) * log_alt[g])) for g in range(3))
    return t


def observed(ref, alt, het_permille):
    total = ref + alt
    if 1000 * min(ref, alt) >= het_permille * total:
        return 2
    return 1 if ref > alt else 3


def match_reference(geno, e_off, e_site, e_ref, e_alt, log_ref, log_alt, cap, het_permille):
    """-> (loglik float64, n_called int32, n_match int32), each [samples, donors]; an entry out of range is skipped (the PHZ_DEVICE rule)"""
    geno = np.asarray(geno, dtype=np.uint8)
    n_sites, D = geno.shape
    S = len(e_off) - 1
    ll = np.zeros((S, D), dtype=np.float64); nc = np.zeros((S, D), dtype=np.int32); nm = np.zeros((S, D), dtype=np.int32)
    log_ref = tuple(float(x) for x in log_ref); log_alt = tuple(float(x) for x in log_alt)
    for s in range(S):
        ent = [(int(e_site[e]), int(e_ref[e]), int(e_alt[e])) for e in range(int(e_off[s]), int(e_off[s + 1]))]
        ent = [(site, ref, alt) for site, ref, alt in ent if 0 <= site < n_sites and ref >= 0 and alt >= 0 and ref + alt > 0]
        if not ent:
            continue
        codes = geno[[site for site, _, _ in ent]]                    # [entries, donors]
        obs = np.array([observed(ref, alt, het_permille) for _, ref, alt in ent], dtype=np.uint8)
        nc[s] = (codes != 0).sum(axis=0)
        nm[s] = (codes == obs[:, None]).sum(axis=0)
        # column 0 holds +0.0 for a donor without a call: x + 0.0 has the bits of x for every x but -0.0, and no partial sum is -0.0 (the sums start at +0.0 and
        # a term is 0 only for r = a = 0, which is not an entry)
        terms = np.array([(0.0,) + entry_terms(ref, alt, cap, log_ref, log_alt) for _, ref, alt in ent])
        assert not np.any(terms[:, 1:] == 0.0)
        acc = np.zeros(D, dtype=np.float64)
        for e in range(len(ent)):                                     # one IEEE add per entry, in entry order
            acc += terms[e][codes[e]]
        ll[s] = acc
    return ll, nc, nm


# counts (ref, alt) that cover the contract's corners at cap 30, het_permille 100
DESIGNED_COUNTS = [
    (5, 3), (29, 0), (15, 14),                    # totals below the cap
    (30, 0), (15, 15), (0, 30), (1, 29),          # at the cap
    (31, 0), (40, 21), (1, 59), (59, 1), (3, 57), (1, 60), (2, 59), (29, 32), (1000, 1), (1, 1000),   # above: 1|59 gives (30 + 30) / 60 = 1, the rounding half
    (0, 8), (8, 0), (0, 1), (1, 0),               # ref = 0, alt = 0
    (I32, I32), (I32, 1), (1, I32), (I32, 0), (0, I32), (I32 - 1, I32), (2 ** 30, 2 ** 30 + 1),   # the int64 products
    (1, 9), (9, 1), (1, 10), (10, 1), (100, 900), (99, 901), (999, 9001), (1000, 9000),           # het_permille 100 hit exactly and one read short of it
    (7, 7), (1, 1), (500, 500),                   # ref == alt
]


def shape_case(n_donors, entries, n_sites=97, seed=5):
    """entries: the entry count of every sample -> (geno [n_sites, n_donors], e_off, e_site, e_ref, e_alt)
    Codes are random with a fixed seed; donor min(3, n_donors - 1) is all no-call and site 11 is all no-call.  Counts cycle through DESIGNED_COUNTS, then random."""
    rng = np.random.default_rng(seed * 1000003 + n_donors * 131 + sum(entries) * 7 + len(entries))
    geno = rng.integers(0, 4, size=(n_sites, n_donors), dtype=np.uint8)
    geno[:, min(3, n_donors - 1)] = 0
    geno[11, :] = 0
    e_off = np.zeros(len(entries) + 1, dtype=np.int64)
    e_off[1:] = np.cumsum(entries)
    n = int(e_off[-1])
    e_site = rng.integers(0, n_sites, size=n).astype(np.int32)
    e_ref = rng.integers(0, 80, size=n).astype(np.int32); e_alt = rng.integers(1, 80, size=n).astype(np.int32)
    for e in range(n):
        if e % 3 != 2:
            c = DESIGNED_COUNTS[(e - e // 3) % len(DESIGNED_COUNTS)]
            e_ref[e], e_alt[e] = c
    if n > 4:
        e_site[4] = 11
    return geno, e_off, e_site, e_ref, e_alt


DONOR_COUNTS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600)


def entry_counts(tile):
    return (0, 1, tile - 1, tile, tile + 1, 2 * tile + 3, 1000)


def sample_layouts(n):
    """the entry counts of 1, 2 and 7 samples around a sample of n entries; the 7 have an empty sample in the middle and one at the end"""
    return ([n], [n, 3], [2, n, 5, 0, n, 1, 0])


# ------------------------------------------------------------------------------------------------ the VCF reader
def geno_code(gt):
    parts = gt.replace("|", "/").split("/")
    if len(parts) != 2 or any(p not in ("0", "1") for p in parts):
        return 0
    return 1 + (parts[0] == "1") + (parts[1] == "1")


def vcf_header_samples(vcf_text):
    for line in vcf_text.split("\n"):
        if line.startswith("#CHROM"):
            return line.rstrip("\r").split("\t")[9:]
    raise Fatal("no #CHROM line")


def site_genotypes_reference(vcf_text, positions, samples):
    """-> the text phz_vcf_site_genotypes returns for the (contig, pos) positions and the named samples"""
    head = ["#CHROM"] + [""] * 8 + vcf_header_samples(vcf_text)
    col = []
    for s in samples:
        at = [j for j in range(9, len(head)) if head[j] == s]
        col.append(at[-1] if at else -1)
    index = {}
    for k, p in enumerate(positions):
        index.setdefault((p[0], p[1]), k)
    out = []
    for line in vcf_text.split("\n"):
        line = line.rstrip("\r")
        if not line or line.startswith("#"):
            continue
        f = line.split("\t")
        if len(f) < 2 or not f[1].lstrip("-").isdigit() or (f[0], int(f[1])) not in index:
            continue
        fmt = f[8].split(":") if len(f) > 8 else []
        gi = fmt.index("GT") if "GT" in fmt else -1
        codes = ""
        for c in col:
            code = 0
            if gi >= 0 and 0 <= c < len(f):
                sub = f[c].split(":")
                if gi < len(sub):
                    code = geno_code(sub[gi])
            codes += str(code)
        out.append("\t".join([str(index[(f[0], int(f[1]))])] + [f[k] if k < len(f) else "" for k in range(5)] + [str(gi), codes]) + "\n")
    return "".join(out)


# ------------------------------------------------------------------------------------------------ the tool
def _fmt(x):
    return "NA" if x is None else repr(float(x))


def _is_count(s):
    return len(s) > 0 and all(c in "0123456789" for c in s) and len(s) <= 10 and int(s) <= I32


def restate_counts(text, min_cov, chrom):
    head = None
    used = []; seen = set(); malformed = 0
    for raw in text.split("\n"):
        line = raw[:-1] if raw.endswith("\r") else raw
        if line == "":
            continue
        f = line.split("\t")
        if head is None:
            head = f
            for k in ("contig", "position", "refAllele", "altAllele", "refCount", "altCount"):
                if k not in head:
                    raise Fatal("column " + k)
            continue
        get = lambda k: f[head.index(k)] if head.index(k) < len(f) else None
        v = [get(k) for k in ("contig", "position", "refAllele", "altAllele", "refCount", "altCount")]
        need = max(head.index(k) for k in ("contig", "position", "refAllele", "altAllele", "refCount", "altCount")) + 1
        if len(f) < need or v[0] == "" or v[2] == "" or v[3] == "" or not (_is_count(v[1]) and _is_count(v[4]) and _is_count(v[5])):
            malformed += 1
            continue
        if chrom and v[0] != chrom:
            continue
        key = (v[0], int(v[1]), v[2], v[3])
        if key in seen:
            continue
        seen.add(key)
        if int(v[4]) + int(v[5]) >= min_cov:
            used.append((key, int(v[4]), int(v[5])))
    return used, malformed


def restate_tool(samples, vcf_text, map_text=None, min_cov=8, cap=30, error=0.01, het_permille=100, max_sites=50000, min_sites=50, min_lod=10.0, chrom="",
                 output_matrix=0):
    """samples: [(name, text of its counts file)] -> {"matches", "map", "summary", "loglik", "concordance"} as the tool writes them (the matrices before compression)"""
    if not (0 < error < 0.5) or not (1 <= het_permille <= 500) or cap < 0 or min_cov < 1 or max_sites < 0 or min_sites < 1 or not (min_lod >= 0):
        raise Fatal("option")
    names = [s for s, _ in samples]
    if len(set(names)) != len(names):
        raise Fatal("sample twice")
    per = []; malformed = 0
    for _, text in samples:
        u, m = restate_counts(text, min_cov, chrom)
        per.append(u); malformed += m
    # the panel
    contigs = []
    union = set()
    for u in per:
        for key, _, _ in u:
            if key[0] not in contigs:
                contigs.append(key[0])
            union.add(key)
    panel = []
    for c in contigs:
        panel += sorted(k for k in union if k[0] == c)
    n_union = len(panel)
    if max_sites > 0 and n_union > max_sites:
        step = (n_union + max_sites - 1) // max_sites
        panel = [panel[i] for i in range(0, n_union, step)]
    n_thinned = len(panel)
    # the donors' genotypes
    donors = vcf_header_samples(vcf_text)
    D = len(donors)
    geno_of = {}
    for line in vcf_text.split("\n"):
        if not line or line.startswith("#"):
            continue
        f = line.rstrip("\r").split("\t")
        key = (f[0], int(f[1]), f[3], f[4])
        if key in geno_of:
            continue
        fmt = f[8].split(":")
        row = [0] * D
        if "GT" in fmt:
            gi = fmt.index("GT")
            for d in range(D):
                sub = f[9 + d].split(":") if 9 + d < len(f) else []
                row[d] = geno_code(sub[gi]) if gi < len(sub) else 0
        geno_of[key] = row
    panel = [k for k in panel if k in geno_of]
    geno = np.array([geno_of[k] for k in panel], dtype=np.uint8).reshape(len(panel), D)
    row_of = {k: i for i, k in enumerate(panel)}
    e_off = [0]; e_site = []; e_ref = []; e_alt = []
    for u in per:
        ent = sorted((row_of[key], r, a) for key, r, a in u if key in row_of)
        e_site += [x[0] for x in ent]; e_ref += [x[1] for x in ent]; e_alt += [x[2] for x in ent]
        e_off.append(len(e_site))
    lr, la = log_tables(error)
    ll, nc, nm = match_reference(geno, e_off, e_site, e_ref, e_alt, lr, la, cap, het_permille)
    # the claims
    claim = {}
    if map_text is not None:
        lines = [l.rstrip("\r") for l in map_text.split("\n") if l.strip("\r")]
        head = lines[0].split("\t")
        by_vcf = {}
        for l in lines[1:]:
            f = l.split("\t")
            by_vcf[f[head.index("vcf_sample")]] = f[head.index("bed_sample")]
        for v, b in by_vcf.items():
            if b not in claim:
                claim[b] = v
    else:
        claim = {s: s for s in names if s in donors}
    header = ["sample", "n_sites", "claimed", "claimed_rank", "claimed_called", "claimed_loglik", "claimed_concordance", "best", "best_called", "best_loglik",
              "best_concordance", "second", "second_loglik", "lod", "verdict"]
    rows = ["\t".join(header) + "\n"]
    new_map = ["vcf_sample\tbed_sample\n"]
    count = {v: 0 for v in VERDICTS}
    best_of = {}
    verdict_of = {}
    for i, s in enumerate(names):
        cand = [d for d in range(D) if nc[i, d] >= 1]
        cand.sort(key=lambda d: (-float(ll[i, d]), d))
        cname = claim.get(s, "NA")
        c = donors.index(cname) if cname != "NA" and cname in donors else -1
        f = {k: "NA" for k in header}
        f["sample"] = s; f["n_sites"] = str(e_off[i + 1] - e_off[i]); f["claimed"] = cname
        if c >= 0:
            f["claimed_called"] = str(int(nc[i, c]))
            if nc[i, c] >= 1:
                f["claimed_rank"] = str(cand.index(c) + 1); f["claimed_loglik"] = _fmt(ll[i, c]); f["claimed_concordance"] = _fmt(int(nm[i, c]) / int(nc[i, c]))
        lod = None
        if cand:
            b = cand[0]
            f["best"] = donors[b]; f["best_called"] = str(int(nc[i, b])); f["best_loglik"] = _fmt(ll[i, b]); f["best_concordance"] = _fmt(int(nm[i, b]) / int(nc[i, b]))
            best_of.setdefault(b, []).append(s)
            if len(cand) > 1:
                lod = (float(ll[i, b]) - float(ll[i, cand[1]])) / math.log(10.0)
                f["second"] = donors[cand[1]]; f["second_loglik"] = _fmt(ll[i, cand[1]]); f["lod"] = _fmt(lod)
        if not cand:
            v = "NO_SITES"
        elif nc[i, cand[0]] < min_sites:
            v = "LOW_SITES"
        elif D == 1:
            v = "SINGLE_DONOR"
        elif lod is not None and lod < min_lod:
            v = "AMBIGUOUS"
        elif c < 0:
            v = "UNCLAIMED"
        elif cand[0] == c:
            v = "MATCH"
        else:
            v = "MISMATCH"
        f["verdict"] = v
        count[v] += 1
        verdict_of[s] = (v, f["best"])
        if v in ("MATCH", "MISMATCH"):
            new_map.append(f["best"] + "\t" + s + "\n")
        rows.append("\t".join(f[k] for k in header) + "\n")
    summ = ["samples\t%d\n" % len(names), "donors\t%d\n" % D, "union_keys\t%d\n" % n_union, "panel_keys\t%d\n" % n_thinned,
            "keys_not_in_vcf\t%d\n" % (n_thinned - len(panel)), "entries\t%d\n" % len(e_site), "malformed_lines\t%d\n" % malformed]
    for v in VERDICTS:
        summ.append("verdict_%s\t%d\n" % (v, count[v]))
    for d in sorted(best_of):
        if len(best_of[d]) > 1:
            summ.append("shared_best\t%s\t%d\t%s\n" % (donors[d], len(best_of[d]), ",".join(best_of[d])))
    out = {"matches": "".join(rows), "map": "".join(new_map), "summary": "".join(summ), "loglik": None, "concordance": None, "verdicts": verdict_of}
    if output_matrix:
        lt = ["\t".join(["sample"] + donors) + "\n"]; ct = list(lt)
        for i, s in enumerate(names):
            lt.append("\t".join([s] + [_fmt(ll[i, d]) if nc[i, d] >= 1 else "NA" for d in range(D)]) + "\n")
            ct.append("\t".join([s] + [_fmt(int(nm[i, d]) / int(nc[i, d])) if nc[i, d] >= 1 else "NA" for d in range(D)]) + "\n")
        out["loglik"] = "".join(lt); out["concordance"] = "".join(ct)
    return out


# ------------------------------------------------------------------------------------------------ synthetic populations
COUNTS_HEADER = "contig\tposition\tvariantID\trefAllele\taltAllele\trefCount\taltCount\ttotalCount"


def synthetic_population(n_donors, n_samples, n_sites, seed, cov_lo=8, cov_hi=60, error=0.01, n_swaps=3, contigs=("chr1",)):
    """-> (vcf text, [(sample, counts text)], map text, truth {sample: true donor}, the swapped samples)
    Sample i is drawn from donor i's genotypes (binomial read sampling at `error`); the map claims donor i for sample i, except that the swapped samples
    claim each other's donors in a cycle."""
    rng = np.random.default_rng(seed)
    donors = ["D%03d" % d for d in range(n_donors)]
    names = ["S%03d" % i for i in range(n_samples)]
    geno = rng.choice(np.array([1, 2, 3], dtype=np.uint8), size=(n_sites, n_donors), p=[0.45, 0.4, 0.15])
    per = -(-n_sites // len(contigs))
    site = [(contigs[j // per], 1000 + 37 * (j % per), "ACGT"[j % 4], "CGTA"[j % 4]) for j in range(n_sites)]
    gt = {1: "0|0", 2: "0|1", 3: "1|1"}
    lines = ["##fileformat=VCFv4.2", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + donors)]
    for j, (c, p, r, a) in enumerate(site):
        lines.append("\t".join([c, str(p), "v%d" % j, r, a, ".", "PASS", ".", "GT"] + [gt[int(g)] for g in geno[j]]))
    p_alt = {1: error, 2: 0.5, 3: 1.0 - error}
    samples = []
    truth = {}
    for i, s in enumerate(names):
        d = i % n_donors
        truth[s] = donors[d]
        total = rng.integers(cov_lo, cov_hi + 1, size=n_sites)
        alt = rng.binomial(total, np.array([p_alt[int(g)] for g in geno[:, d]]))
        rows = [COUNTS_HEADER]
        for j, (c, p, r, a) in enumerate(site):
            rows.append("%s\t%d\tv%d\t%s\t%s\t%d\t%d\t%d" % (c, p, j, r, a, total[j] - alt[j], alt[j], total[j]))
        samples.append((s, "\n".join(rows) + "\n"))
    swapped = [names[int(k)] for k in sorted(rng.choice(min(n_samples, n_donors), size=n_swaps, replace=False).tolist())] if n_swaps else []
    claim = dict(truth)
    for k, s in enumerate(swapped):
        claim[s] = truth[swapped[(k + 1) % len(swapped)]]
    map_text = "vcf_sample\tbed_sample\n" + "".join("%s\t%s\n" % (claim[s], s) for s in names)
    return "\n".join(lines) + "\n", samples, map_text, truth, swapped
