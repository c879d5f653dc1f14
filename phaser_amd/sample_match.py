"""phaser_sample_match: which donor of a population VCF each sample's reads came from (no counterpart in the reference: the genotype-concordance pass labs
run outside phASER before they trust a sample map).

    python -m phaser_amd.sample_match --counts_dir DIR | --counts_list FILE --vcf POP.vcf.gz --o OUT
            [--map map.txt --min_cov 8 --cap 30 --error 0.01 --het_permille 100 --max_sites 50000 --min_sites 50 --min_lod 10 --chr C --output_matrix 0 --t N]

Every population tool here (expr_matrix, cis_var, cis_scan, ae_test, ae_betabinom, ae_outlier, ae_diff) trusts that a sample's reads belong to the VCF donor
the map names.  This tool checks it from what phASER already wrote: the <o>.allelic_counts.txt of every sample against the genotypes of every donor.

Inputs.  --counts_dir: every *.allelic_counts.txt or *.allelic_counts.txt.gz of the directory, the sample name is the file name in front of
".allelic_counts.txt", samples in sorted name order; --counts_list: lines "sample<TAB>path", in file order.  A counts file has phASER's header (contig position
variantID refAllele altAllele refCount altCount totalCount; the columns are found by name).  A line that lacks a needed column, whose position or counts are
not decimal numbers below 2^31, or that names no contig or allele is malformed: counted and skipped.  With --chr only the lines of that contig are read.  Of two
lines with the same (contig, position, refAllele, altAllele) the first counts, the later ones are ignored.  A line is used when refCount + altCount >= --min_cov.
--map (cis_var.read_map's format): the claimed donor of sample bed_sample is vcf_sample, NA for a sample the map lacks; without --map the claimed donor is the
donor of the sample's name, else NA.

Pipeline:
  python threads over the files                  the used lines of every sample
  numpy / python                                 the panel: the union of the used keys, contigs by first appearance (samples in order), inside a contig by
                                                 (position, ref, alt); with --max_sites M > 0 and n > M keys, the keys at 0, s, 2s, ... with s = ceil(n / M)
  phz_vcf_site_genotypes (libphz.so, threads)    the donors' genotype codes at the panel's positions (0 no call, 1 hom-ref, 2 het, 3 hom-alt); a key's genotypes
                                                 are those of the first record at its position whose REF and ALT equal the key's; keys without one leave the panel
  phz_sample_match       (HIP, K_match)          per (sample, donor): log-likelihood of the counts, called sites, sites whose observed class is the genotype
  numpy                                          candidates = donors called at one site or more, by descending log-likelihood, then ascending donor index;
                                                 lod = (best - second) / ln 10; concordance = matching / called; the verdict
Verdict, the first that applies: NO_SITES (no candidate), LOW_SITES (the best donor is called at fewer than --min_sites sites), SINGLE_DONOR (one donor in the
VCF), AMBIGUOUS (lod < --min_lod), UNCLAIMED (the claimed donor is NA or not in the VCF), MATCH (the best donor is the claimed one), MISMATCH.  A sample with
one candidate among several donors has no lod (NA) and is not AMBIGUOUS.

Writes <o>.matches.txt (one row per sample), <o>.map.txt (vcf_sample, bed_sample: the best donor of every MATCH and MISMATCH sample; cis_var and cis_scan take
it as --map), <o>.summary.txt and, with --output_matrix 1, <o>.loglik.txt.gz and <o>.concordance.txt.gz (samples x donors).  Floats are repr(float), NA where
undefined.  There is no CPU path: without a GPU the run raises.  Two runs on the same input write identical bytes.
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import math
import os
import sys
import time
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .ae_test import _check, _vp
from .cis_var import FatalError, read_map

COUNTS_SUFFIX = ".allelic_counts.txt"
COUNTS_COLUMNS = ("contig", "position", "refAllele", "altAllele", "refCount", "altCount")
MATCHES_HEADER = ["sample", "n_sites", "claimed", "claimed_rank", "claimed_called", "claimed_loglik", "claimed_concordance", "best", "best_called", "best_loglik",
                  "best_concordance", "second", "second_loglik", "lod", "verdict"]
VERDICTS = ("MATCH", "MISMATCH", "UNCLAIMED", "AMBIGUOUS", "SINGLE_DONOR", "LOW_SITES", "NO_SITES")


def _fmt(x) -> str:
    return "NA" if x is None or x != x else repr(float(x))


def check_options(min_cov, cap, error, het_permille, max_sites, min_sites, min_lod):
    if not (0.0 < error < 0.5):
        raise FatalError("FATAL ERROR - --error must lie strictly between 0 and 0.5")
    if het_permille < 1 or het_permille > 500:
        raise FatalError("FATAL ERROR - --het_permille must lie between 1 and 500")
    if cap < 0 or max_sites < 0:
        raise FatalError("FATAL ERROR - --cap and --max_sites must not be negative")
    if min_cov < 1 or min_sites < 1:
        raise FatalError("FATAL ERROR - --min_cov and --min_sites must be at least 1")
    if not (min_lod >= 0.0):
        raise FatalError("FATAL ERROR - --min_lod must not be negative")


# ---------------------------------------------------------------------------------------------------------------- inputs
def _is_count(s: str) -> bool:
    return s.isascii() and s.isdigit() and len(s) <= 10 and int(s) <= 2 ** 31 - 1


def parse_counts(text: str, min_cov: int = 8, chrom: str = ""):
    """the text of one allelic counts file -> ([(contig, position, ref, alt, refCount, altCount)] of the used lines in file order, malformed lines)"""
    cols = None
    need = 0
    used = []
    seen = set()
    malformed = 0
    for line in text.split("\n"):
        line = line.rstrip("\r")
        if not line:
            continue
        f = line.split("\t")
        if cols is None:
            try:
                cols = [f.index(k) for k in COUNTS_COLUMNS]
            except ValueError:
                raise FatalError("FATAL ERROR - an allelic counts file lacks one of the columns %s" % ", ".join(COUNTS_COLUMNS))
            need = max(cols) + 1
            continue
        if len(f) < need:
            malformed += 1
            continue
        contig, pos, ref, alt, rc, ac = (f[j] for j in cols)
        if contig == "" or ref == "" or alt == "" or not (_is_count(pos) and _is_count(rc) and _is_count(ac)):
            malformed += 1
            continue
        if chrom != "" and contig != chrom:
            continue
        key = (contig, int(pos), ref, alt)
        if key in seen:
            continue
        seen.add(key)
        if int(rc) + int(ac) >= min_cov:
            used.append(key + (int(rc), int(ac)))
    return used, malformed


def read_text(path: str) -> str:
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":                             # plain gzip and BGZF alike
        raw = gzip.decompress(raw)
    return raw.decode()


def list_counts_dir(path: str) -> List[Tuple[str, str]]:
    """-> [(sample, path)] in sorted sample order"""
    out = {}
    for name in sorted(os.listdir(path)):
        for suffix in (COUNTS_SUFFIX, COUNTS_SUFFIX + ".gz"):
            if name.endswith(suffix):
                sample = name[:-len(suffix)]
                if sample in out:
                    raise FatalError("FATAL ERROR - sample %s occurs twice in --counts_dir" % sample)
                out[sample] = os.path.join(path, name)
    return sorted(out.items())


def read_counts_list(text: str) -> List[Tuple[str, str]]:
    out = []
    seen = set()
    for line in text.split("\n"):
        line = line.rstrip("\r")
        if not line:
            continue
        f = line.split("\t")
        if len(f) < 2:
            raise FatalError("FATAL ERROR - a line of --counts_list is not sample<TAB>path")
        if f[0] in seen:
            raise FatalError("FATAL ERROR - sample %s occurs twice in --counts_list" % f[0])
        seen.add(f[0])
        out.append((f[0], f[1]))
    return out


def vcf_donors(path: str) -> List[str]:
    """the sample names of the #CHROM line"""
    with gzip.open(path, "rt") as f:
        for line in f:
            if line.startswith("#CHROM"):
                donors = line.rstrip("\r\n").split("\t")[9:]
                if len(set(donors)) != len(donors):
                    raise FatalError("FATAL ERROR - a donor occurs twice in the header of --vcf")
                return donors
            if not line.startswith("#"):
                break
    raise FatalError("FATAL ERROR - --vcf has no #CHROM line")


def build_panel(per_sample, max_sites: int = 0):
    """[the used lines of every sample] -> (the panel keys in panel order, the number of union keys)"""
    contig_rank = {}
    union = set()
    for used in per_sample:
        for u in used:
            if u[0] not in contig_rank:
                contig_rank[u[0]] = len(contig_rank)
            union.add(u[:4])
    keys = sorted(union, key=lambda k: (contig_rank[k[0]], k[1], k[2], k[3]))
    n = len(keys)
    if max_sites > 0 and n > max_sites:
        keys = keys[::-(-n // max_sites)]
    return keys, n


# ---------------------------------------------------------------------------------------------------------------- VCF
def site_genotypes(path: str, positions, donors, threads: int = 1, use_index: bool = True):
    """phz_vcf_site_genotypes: every record at one of the (contig, 1-based pos) positions, in file order
    -> ([(index into positions, CHROM, POS, ID, REF, ALT, gt_index)], codes uint8 [records, donors], contigs of the VCF)"""
    lib = _lib.load()
    cb = [str(c).encode() for c, _ in positions]; sb = [x.encode() for x in donors]
    carr = (C.c_char_p * max(1, len(cb)))(*cb); sarr = (C.c_char_p * max(1, len(sb)))(*sb)
    parr = np.ascontiguousarray([p for _, p in positions] or [0], dtype=np.int64)
    optr = C.c_void_p(); olen = C.c_int64(0); cptr = C.c_void_p(); clen = C.c_int64(0)
    st = lib.phz_vcf_site_genotypes(path.encode(), len(cb), carr, _vp(parr), len(sb), sarr, int(bool(use_index)), max(1, int(threads)),
                                    C.byref(optr), C.byref(olen), C.byref(cptr), C.byref(clen))
    if st != _lib.PHZ_OK:
        raise _lib.PhzError(st, "phz_vcf_site_genotypes(%s) failed" % path)
    try:
        text = C.string_at(optr, olen.value); ctext = C.string_at(cptr, clen.value).decode()
    finally:
        lib.phz_buf_free(optr); lib.phz_buf_free(cptr)
    recs = []; rows = []
    for line in text.split(b"\n"):
        if line:
            f = line.split(b"\t")
            recs.append((int(f[0]), f[1].decode(), int(f[2]), f[3].decode(), f[4].decode(), f[5].decode(), int(f[6])))
            rows.append(f[7])
    D = len(donors)
    codes = (np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), D) - 48) if rows and D else np.zeros((len(rows), D), dtype=np.uint8)
    return recs, codes, set(ctext.split("\n")) - {""}


def panel_genotypes(path: str, keys, donors, threads: int = 1, use_index: bool = True):
    """-> (the keys that have a record whose REF and ALT equal theirs, geno uint8 [those keys, donors])"""
    positions = list(dict.fromkeys((k[0], k[1]) for k in keys))
    recs, codes, _ = site_genotypes(path, positions, donors, threads, use_index)
    first = {}
    for i, (pi, _, _, _, ref, alt, _) in enumerate(recs):
        first.setdefault(positions[pi] + (ref, alt), i)
    kept = [k for k in keys if k in first]
    geno = codes[[first[k] for k in kept]] if kept else np.zeros((0, len(donors)), dtype=np.uint8)
    return kept, np.ascontiguousarray(geno, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- K_match
def log_tables(error: float):
    """-> (log_ref, log_alt) per genotype code 1, 2, 3"""
    return (math.log1p(-error), math.log(0.5), math.log(error)), (math.log(error), math.log(0.5), math.log1p(-error))


def match_call(lib, handle, geno, e_off, e_site, e_ref, e_alt, error: float = 0.01, cap: int = 30, het_permille: int = 100):
    """phz_sample_match on host arrays -> (loglik float64, n_called int32, n_match int32), each [samples, donors]"""
    geno = np.ascontiguousarray(geno, dtype=np.uint8)
    assert geno.ndim == 2
    e_off = np.ascontiguousarray(e_off, dtype=np.int64)
    e_site = np.ascontiguousarray(e_site, dtype=np.int32); e_ref = np.ascontiguousarray(e_ref, dtype=np.int32); e_alt = np.ascontiguousarray(e_alt, dtype=np.int32)
    S, D = len(e_off) - 1, geno.shape[1]
    arg = _lib.phz_match_in()
    arg.n_sites, arg.n_samples, arg.n_donors = geno.shape[0], S, D
    arg.geno, arg.e_off, arg.e_site, arg.e_ref, arg.e_alt = (x.ctypes.data for x in (geno, e_off, e_site, e_ref, e_alt))
    lr, la = log_tables(error)
    arg.log_ref = (C.c_double * 3)(*lr); arg.log_alt = (C.c_double * 3)(*la)
    arg.cap, arg.het_permille = int(cap), int(het_permille)
    ll = np.zeros((S, D), dtype=np.float64); nc = np.zeros((S, D), dtype=np.int32); nm = np.zeros((S, D), dtype=np.int32)
    _check(lib, handle, lib.phz_sample_match(handle, C.byref(arg), _vp(ll), _vp(nc), _vp(nm), _lib.PHZ_HOST))
    return ll, nc, nm


# ---------------------------------------------------------------------------------------------------------------- the tool
def decide(ll, nc, nm, claimed: int, claimed_name: str, n_donors: int, min_sites: int, min_lod: float):
    """one sample's rows of the three matrices -> the fields of its matches row behind (sample, n_sites), as a dict
    claimed: the donor index of the claimed donor, -1 when it is NA or not in the VCF"""
    cand = np.nonzero(nc >= 1)[0]
    order = cand[np.argsort(-ll[cand], kind="stable")]                 # descending log-likelihood, then ascending donor index
    r = {"claimed": claimed_name, "claimed_rank": None, "claimed_called": None, "claimed_loglik": None, "claimed_concordance": None, "best": -1, "best_called": None,
         "best_loglik": None, "best_concordance": None, "second": -1, "second_loglik": None, "lod": None}
    if claimed >= 0:
        r["claimed_called"] = int(nc[claimed])
        if nc[claimed] >= 1:
            r["claimed_rank"] = int(np.nonzero(order == claimed)[0][0]) + 1
            r["claimed_loglik"] = float(ll[claimed]); r["claimed_concordance"] = int(nm[claimed]) / int(nc[claimed])
    if len(order) == 0:
        r["verdict"] = "NO_SITES"
        return r
    b = int(order[0])
    r["best"] = b; r["best_called"] = int(nc[b]); r["best_loglik"] = float(ll[b]); r["best_concordance"] = int(nm[b]) / int(nc[b])
    if len(order) > 1:
        s = int(order[1])
        r["second"] = s; r["second_loglik"] = float(ll[s]); r["lod"] = (float(ll[b]) - float(ll[s])) / math.log(10.0)
    if nc[b] < min_sites:
        r["verdict"] = "LOW_SITES"
    elif n_donors == 1:
        r["verdict"] = "SINGLE_DONOR"
    elif r["lod"] is not None and r["lod"] < min_lod:
        r["verdict"] = "AMBIGUOUS"
    elif claimed < 0:
        r["verdict"] = "UNCLAIMED"
    else:
        r["verdict"] = "MATCH" if b == claimed else "MISMATCH"
    return r


def _matrix_text(samples, donors, values) -> str:
    rows = ["\t".join(["sample"] + list(donors)) + "\n"]
    for s, row in zip(samples, values.tolist()):
        rows.append("\t".join([s] + [_fmt(v) for v in row]) + "\n")
    return "".join(rows)


def sample_match(samples, vcf_path: str, map_text: Optional[str] = None, min_cov: int = 8, cap: int = 30, error: float = 0.01, het_permille: int = 100,
                 max_sites: int = 50000, min_sites: int = 50, min_lod: float = 10.0, chrom: str = "", output_matrix: int = 0, threads: int = 1, ctx=None,
                 stats: Optional[dict] = None, use_index: bool = True) -> dict:
    """The tool on [(sample name, path or None, text or None)]: a sample comes as a path to read or as its text
    -> {"matches", "map", "summary": str, "loglik", "concordance": str or None}.
    ctx: anything with .lib and .h (a _lib.Context; made here when None, which raises without a GPU)."""
    check_options(min_cov, cap, error, het_permille, max_sites, min_sites, min_lod)
    if ctx is None:
        ctx = _lib.Context(0)                          # raises without a GPU: there is no CPU path
    names = [s[0] for s in samples]
    if len(set(names)) != len(names):
        raise FatalError("FATAL ERROR - a sample is named twice")
    t0 = time.perf_counter()

    def load(item):
        return parse_counts(item[2] if item[2] is not None else read_text(item[1]), min_cov, chrom)
    if threads > 1 and len(samples) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(min(int(threads), len(samples))) as ex:
            parsed = list(ex.map(load, samples))
    else:
        parsed = [load(s) for s in samples]
    per_sample = [p[0] for p in parsed]
    malformed = sum(p[1] for p in parsed)
    t1 = time.perf_counter()
    keys, n_union = build_panel(per_sample, max_sites)
    n_thinned = len(keys)
    t2 = time.perf_counter()
    donors = vcf_donors(vcf_path)
    D = len(donors)
    if D == 0:
        raise FatalError("FATAL ERROR - --vcf names no donor")
    keys, geno = panel_genotypes(vcf_path, keys, donors, threads, use_index)
    t3 = time.perf_counter()
    row_of = {k: i for i, k in enumerate(keys)}
    e_off = np.zeros(len(samples) + 1, dtype=np.int64)
    parts = []
    for i, used in enumerate(per_sample):
        ent = sorted((row_of[u[:4]], u[4], u[5]) for u in used if u[:4] in row_of)
        parts.append(np.array(ent, dtype=np.int64).reshape(-1, 3))
        e_off[i + 1] = e_off[i] + len(ent)
    ent = np.concatenate(parts) if parts else np.zeros((0, 3), dtype=np.int64)
    t4 = time.perf_counter()
    ll, nc, nm = match_call(ctx.lib, ctx.h, geno, e_off, ent[:, 0], ent[:, 1], ent[:, 2], error, cap, het_permille)
    t5 = time.perf_counter()
    # ---- rank and decide
    donor_index = {d: i for i, d in enumerate(donors)}
    if map_text is not None:
        claim = {}
        for v, b in read_map(map_text):
            claim.setdefault(b, v)
    else:
        claim = {s: s for s in names if s in donor_index}
    rows = ["\t".join(MATCHES_HEADER) + "\n"]
    new_map = ["vcf_sample\tbed_sample\n"]
    verdicts = {v: 0 for v in VERDICTS}
    best_of = {}
    for i, s in enumerate(names):
        cname = claim.get(s, "NA")
        r = decide(ll[i], nc[i], nm[i], donor_index.get(cname, -1) if cname != "NA" else -1, cname, D, min_sites, min_lod)
        verdicts[r["verdict"]] += 1
        if r["best"] >= 0:
            best_of.setdefault(r["best"], []).append(s)
        if r["verdict"] in ("MATCH", "MISMATCH"):
            new_map.append("%s\t%s\n" % (donors[r["best"]], s))
        ints = lambda x: "NA" if x is None else str(x)
        name = lambda d: "NA" if d < 0 else donors[d]
        rows.append("\t".join([s, str(int(e_off[i + 1] - e_off[i])), r["claimed"], ints(r["claimed_rank"]), ints(r["claimed_called"]), _fmt(r["claimed_loglik"]),
                               _fmt(r["claimed_concordance"]), name(r["best"]), ints(r["best_called"]), _fmt(r["best_loglik"]), _fmt(r["best_concordance"]),
                               name(r["second"]), _fmt(r["second_loglik"]), _fmt(r["lod"]), r["verdict"]]) + "\n")
    summ = ["samples\t%d\n" % len(names), "donors\t%d\n" % D, "union_keys\t%d\n" % n_union, "panel_keys\t%d\n" % n_thinned,
            "keys_not_in_vcf\t%d\n" % (n_thinned - len(keys)), "entries\t%d\n" % int(e_off[-1]), "malformed_lines\t%d\n" % malformed]
    summ += ["verdict_%s\t%d\n" % (v, verdicts[v]) for v in VERDICTS]
    shared = [(d, ss) for d, ss in sorted(best_of.items()) if len(ss) > 1]
    summ += ["shared_best\t%s\t%d\t%s\n" % (donors[d], len(ss), ",".join(ss)) for d, ss in shared]
    out = {"matches": "".join(rows), "map": "".join(new_map), "summary": "".join(summ), "loglik": None, "concordance": None}
    if output_matrix:
        with np.errstate(divide="ignore", invalid="ignore"):
            conc = np.where(nc >= 1, nm / np.maximum(nc, 1), np.nan)
        out["loglik"] = _matrix_text(names, donors, np.where(nc >= 1, ll, np.nan))
        out["concordance"] = _matrix_text(names, donors, conc)
    if stats is not None:
        stats.update({"samples": len(names), "donors": D, "union_keys": n_union, "panel_keys": n_thinned, "keys_in_vcf": len(keys), "entries": int(e_off[-1]),
                      "malformed": malformed, "verdicts": verdicts, "shared_best": len(shared),
                      "seconds": {"parse": round(t1 - t0, 3), "panel": round(t2 - t1, 3), "vcf": round(t3 - t2, 3), "entries": round(t4 - t3, 3),
                                  "match": round(t5 - t4, 3), "decide": round(time.perf_counter() - t5, 3)}})
        if hasattr(ctx, "timing"):
            stats["k_match_ms"] = ctx.timing(_lib.PHZ_T_MATCH)[0]
    return out


class _Parser(argparse.ArgumentParser):
    def error(self, message):                          # one line, status 1
        print("FATAL ERROR - %s" % message)
        sys.exit(1)


def main(argv=None) -> int:
    ap = _Parser()
    ap.add_argument("--counts_dir", type=str, default=""); ap.add_argument("--counts_list", type=str, default="")
    ap.add_argument("--vcf", type=str, required=True); ap.add_argument("--o", type=str, required=True); ap.add_argument("--map", type=str, default="")
    ap.add_argument("--min_cov", type=int, default=8); ap.add_argument("--cap", type=int, default=30); ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--het_permille", type=int, default=100); ap.add_argument("--max_sites", type=int, default=50000)
    ap.add_argument("--min_sites", type=int, default=50); ap.add_argument("--min_lod", type=float, default=10.0); ap.add_argument("--chr", type=str, default="")
    ap.add_argument("--output_matrix", type=int, default=0); ap.add_argument("--t", type=int, default=1)
    args = ap.parse_args(argv)
    stats: dict = {}
    try:
        check_options(args.min_cov, args.cap, args.error, args.het_permille, args.max_sites, args.min_sites, args.min_lod)
        if (args.counts_dir == "") == (args.counts_list == ""):
            raise FatalError("FATAL ERROR - exactly one of --counts_dir and --counts_list must be given")
        print(""); print("##################################################")
        print("        Welcome to phaser_sample_match (phaser_amd, MI355X)")
        print("##################################################"); print("")
        print("#1 Listing the allelic counts files...")
        if args.counts_dir:
            files = list_counts_dir(args.counts_dir)
        else:
            with open(args.counts_list) as f:
                files = read_counts_list(f.read())
        map_text = None
        if args.map:
            with open(args.map) as f:
                map_text = f.read()
        print("#2 Matching %d samples against the donors of %s..." % (len(files), args.vcf))
        out = sample_match([(s, p, None) for s, p in files], args.vcf, map_text, args.min_cov, args.cap, args.error, args.het_permille, args.max_sites, args.min_sites,
                           args.min_lod, args.chr, args.output_matrix, threads=args.t, stats=stats)
    except FatalError as e:
        print(str(e))
        return 1
    print("#3 Saving results...")
    for kind in ("matches", "map", "summary"):
        with open("%s.%s.txt" % (args.o, kind), "w") as f:
            f.write(out[kind])
    if args.output_matrix:
        from . import vcfout
        for kind in ("loglik", "concordance"):
            vcfout.write_bgzf("%s.%s.txt.gz" % (args.o, kind), out[kind].encode(), args.t)
    print("     %d samples x %d donors, %d panel keys (union %d, %d not in the VCF), %d entries, %d malformed lines" %
          (stats["samples"], stats["donors"], stats["keys_in_vcf"], stats["union_keys"], stats["panel_keys"] - stats["keys_in_vcf"], stats["entries"], stats["malformed"]))
    print("     verdicts %s; %d donors are the best of more than one sample" % (" ".join("%s %d" % (v, stats["verdicts"][v]) for v in VERDICTS), stats["shared_best"]))
    print("     seconds %s; K_match %.3f ms" % (stats["seconds"], stats.get("k_match_ms", float("nan"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
