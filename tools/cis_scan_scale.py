"""Synthetic scale run of phaser_cis_scan (python -m phaser_amd.cis_scan): --genes x --samples aCount|bCount cells, genes --spacing bases apart on four contigs,
and a population VCF with one variant every --density bases, so that a gene's window of +-100 kb holds about 2,000 variants.  Genotypes are 0|0, 0|1, 1|0, 1|1
with equal weight and 2 % unphased; the total of a cell is log-uniform from 8 to 10^4 and its ratio N(0.5, 0.05); every 50th gene has a planted variant whose
heterozygotes sit at a ratio of 0.8 or 0.2.

Two in-process runs of the tool on the GPU on the same files: --perm 0 (k_cisscan_obs + k_cisscan_best alone) and --perm P.  Reported: the stage seconds of
both, the device time of the observed pass and, by difference, of k_cisscan_perm (HIP events, PHZ_T_CISSCAN, summed over the contigs), the rates per pair and
per (pair, replicate, position), and a spot check of 20 genes against the restatement of the tests (tests/cis_scan_restatement.py):
  observed   from the files alone: n_covered, and for the printed best variant n_het, n_hom and U2 counted pair by pair, then z and p as strings; 40 other
             variants of the window, none of which may beat the printed one
  permuted   the 20 genes again through phz_cis_scan with a window cut to 24 variants and P = 3, against the full restatement: every array equal
(a full restatement of 1,000 replicates of 2,000 variants is out of reach of plain Python).  A miss ends the tool with status 1.

usage: python tools/cis_scan_scale.py [--seed 0] [--genes 2000] [--samples 800] [--perm 1000] [--spacing 1000] [--density 100] [--out DIR] [--threads 16]
"""
import argparse
import gzip
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

CONTIGS = 4
GT_TEXT = np.frombuffer(b"\t0|0\t0|1\t1|0\t1|1\t0/1", dtype=np.uint8).reshape(5, 4)


def make_inputs(d, seed, n_genes, n_samples, spacing, density, threads):
    from phaser_amd import vcfout
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    names = ["SAMPLE%04d" % s for s in range(n_samples)]
    with open(os.path.join(d, "map.txt"), "w") as f:
        f.write("vcf_sample\tbed_sample\n" + "".join("%s\t%s\n" % (s, s) for s in names))
    per = (n_genes + CONTIGS - 1) // CONTIGS
    span = 100_000 + per * spacing + 3_000 + 100_000
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    parts = [head.encode()]
    gts = {}
    for c in range(CONTIGS):
        pos = np.arange(1 + density // 2, span, density)
        idx = rng.integers(0, 4, (len(pos), n_samples), dtype=np.uint8)
        idx[rng.random(idx.shape) < 0.02] = 4
        gts[c] = (pos, idx)
        body = GT_TEXT[idx].reshape(len(pos), 4 * n_samples)
        for p, row in zip(pos.tolist(), body):
            parts.append(b"chr%d\t%d\t.\tA\tG\t.\tPASS\t.\tGT" % (c + 1, p)); parts.append(row.tobytes()); parts.append(b"\n")
    vcf_path = os.path.join(d, "pop.vcf.gz")
    vcf_text = b"".join(parts)
    if not vcfout.write_bgzf(vcf_path, vcf_text, threads, index="vcf"):
        raise SystemExit("the VCF index was refused")
    lines = ["\t".join(["#contig", "start", "stop", "name"] + names)]
    for g in range(n_genes):
        c, k = g // per, g % per
        start = 100_000 + k * spacing
        n = np.exp(rng.uniform(np.log(8.0), np.log(1e4), n_samples)).astype(np.int64)
        ratio = np.clip(rng.normal(0.5, 0.05, n_samples), 0.02, 0.98)
        if g % 50 == 0:
            pos, idx = gts[c]
            v = int(np.searchsorted(pos, start + 1500))
            ratio = np.where(idx[v] == 1, 0.2, np.where(idx[v] == 2, 0.8, ratio))
        a = rng.binomial(n, ratio)
        cells = np.char.add(np.char.add(a.astype(str), "|"), (n - a).astype(str))
        cells[rng.random(n_samples) < 0.02] = ""
        lines.append("\t".join(["chr%d" % (c + 1), str(start), str(start + 3_000), "ENSG%011d" % g] + cells.tolist()))
    bed_text = "\n".join(lines) + "\n"
    return bed_text, vcf_path, len(vcf_text), open(os.path.join(d, "map.txt")).read()


def spot_check(bed_text, vcf_path, map_text, genes_txt, seed, ctx, n_genes=20):
    import cis_scan_restatement as R
    from phaser_amd import cis_scan as cs
    rng = np.random.default_rng(seed + 1)
    names, recs = R.vcf_records(gzip.open(vcf_path, "rt").read())
    col = {nm: j for j, nm in enumerate(names)}
    by_contig = {}
    for r in recs:
        by_contig.setdefault(r[0], []).append(r)
    rows = [l.split("\t") for l in genes_txt.split("\n")[1:] if l]
    lines = bed_text.split("\n")
    head = lines[0].split("\t")
    tested = [i for i, r in enumerate(rows) if r[6] != "NA"]
    picks = sorted(rng.choice(tested, min(n_genes, len(tested)), replace=False).tolist())
    small = []
    for i in picks:
        f = lines[1 + i].split("\t")
        r = rows[i]
        assert f[3] == r[0]
        afc = {}
        for s, nm in enumerate(head[4:]):
            m = R._CELL.fullmatch(f[4 + s])
            if m and int(m.group(1)) + int(m.group(2)) >= 8:
                afc[s] = math.log(float(int(m.group(1)) + 1) / float(int(m.group(2)) + 1), 2)
        covered = sorted(afc)
        value = {s: abs(afc[s]) for s in covered}
        mine = [x for x in by_contig[f[0]] if int(f[1]) + 1 - 100000 <= x[1] <= int(f[2]) + 100000]
        cls_of = lambda x: [R.classify(x[6][col[nm]])[0] for nm in head[4:]]
        best = next(x for x in mine if "%s_%d_%s_%s" % (x[0], x[1], x[3], x[4]) == r[6])
        others = [mine[k] for k in rng.choice(len(mine), min(40, len(mine)), replace=False).tolist()]
        nh, nm_, u2, _ = R.scan_gene([cls_of(best)] + [cls_of(x) for x in others], covered, value, 0, 0, 0)
        z, p = R.z_p(u2[0], nh[0], nm_[0])
        if (str(len(covered)), str(nh[0]), str(nm_[0]), R.fmt(z), R.fmt(p)) != (r[4], r[8], r[9], r[10], r[11]):
            print("spot check, gene %s: restated %s, printed %s" % (r[0], (len(covered), nh[0], nm_[0], R.fmt(z), R.fmt(p)), r)); sys.exit(1)
        t0 = R.t_stat(u2[0], nh[0], nm_[0])
        for k, x in enumerate(others, 1):
            if nh[k] >= 5 and nm_[k] >= 5 and (R.t_stat(u2[k], nh[k], nm_[k]), -x[1]) > (t0, -best[1]):
                print("spot check, gene %s: variant at %d beats the printed one" % (r[0], x[1])); sys.exit(1)
        at = mine.index(best)
        lo = max(0, min(at - 12, len(mine) - 24))
        small.append({"covered": covered, "value": value, "rows": [cls_of(x) for x in mine[lo:lo + 24]], "subseq": i})
    # ---- the permuted pass of the same genes on a window the restatement can follow
    S = len(head) - 4
    cls = [row for g in small for row in g["rows"]]
    cov = np.zeros((len(small), S), dtype=bool); val = np.zeros((len(small), S))
    for g, ge in enumerate(small):
        for s in ge["covered"]:
            cov[g, s] = True; val[g, s] = ge["value"][s]
    v_lo = np.cumsum([0] + [len(g["rows"]) for g in small])
    si = cs.ScanInput(np.array(cls, dtype=np.uint8), cov, val, v_lo[:-1], v_lo[1:], [g["subseq"] for g in small], 5, 5, 3, seed)
    got = cs.cis_scan_call(ctx.lib, ctx.h, si)
    k = 0
    for g, ge in enumerate(small):
        nh, nm_, u2, pu2 = R.scan_gene(ge["rows"], ge["covered"], ge["value"], ge["subseq"], 3, seed)
        b, e = R.best_and_exceed(nh, nm_, u2, pu2, 5, 5, 3)
        n = len(ge["rows"])
        if (got[0][k:k + n].tolist(), got[1][k:k + n].tolist(), got[2][k:k + n].tolist(), int(got[3][g]), int(got[4][g])) != (nh, nm_, u2, -1 if b < 0 else int(v_lo[g]) + b, e):
            print("spot check, permuted pass: gene %d differs from the restatement" % g); sys.exit(1)
        k += n
    return {"genes": len(picks), "observed": "n_covered, n_het, n_hom, z, p of the best variant equal; 40 other variants each, none beats it",
            "permuted": "24-variant windows, P = 3: every array equal"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--genes", type=int, default=2000); ap.add_argument("--samples", type=int, default=800)
    ap.add_argument("--perm", type=int, default=1000); ap.add_argument("--spacing", type=int, default=1000); ap.add_argument("--density", type=int, default=100)
    ap.add_argument("--out", default="/tmp/cis_scan_scale"); ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    from phaser_amd import _lib, cis_scan as cs
    t0 = time.perf_counter()
    bed_text, vcf_path, vcf_bytes, map_text = make_inputs(args.out, args.seed, args.genes, args.samples, args.spacing, args.density, args.threads)
    t_gen = time.perf_counter() - t0
    print("inputs made in %.1f s" % t_gen, flush=True)
    ctx = _lib.Context(0)
    runs = {}
    for perm in (0, args.perm):
        stats = {}
        t = time.perf_counter()
        out = cs.cis_scan(bed_text, vcf_path, map_text, perm=perm, seed=args.seed, threads=args.threads, ctx=ctx, stats=stats)
        stats["wall_s"] = round(time.perf_counter() - t, 3)
        runs[perm] = (out, stats)
        print("perm %d: %s" % (perm, json.dumps(stats)), flush=True)
    obs, full = runs[0][1], runs[args.perm][1]
    perm_ms = full["k_cisscan_ms"] - obs["k_cisscan_ms"]
    rows = [l.split("\t") for l in runs[args.perm][0]["genes"].split("\n")[1:] if l]
    n_mean = float(np.mean([int(r[4]) for r in rows]))
    tested = sum(int(r[5]) for r in rows)
    res = {"genes": full["genes"], "samples": full["samples"], "variants": full["variants"], "pairs": full["pairs"], "testable_pairs": tested,
           "pairs_per_gene": round(full["pairs"] / max(1, full["genes"]), 1), "mean_covered": round(n_mean, 1), "perm": args.perm,
           "vcf_text_bytes": vcf_bytes, "vcf_bgzf_bytes": os.path.getsize(vcf_path), "matrix_text_bytes": len(bed_text), "generate_s": round(t_gen, 2),
           "stages_s_perm_0": obs["seconds"], "stages_s": full["seconds"], "wall_s_perm_0": obs["wall_s"], "wall_s": full["wall_s"],
           "k_cisscan_obs_best_device_ms": round(obs["k_cisscan_ms"], 3), "k_cisscan_perm_device_ms": round(perm_ms, 3),
           "obs_ns_per_pair": round(1e6 * obs["k_cisscan_ms"] / max(1, full["pairs"]), 2),
           "perm_ns_per_pair_replicate": round(1e6 * perm_ms / max(1, tested * args.perm), 3),
           "perm_ps_per_pair_replicate_position": round(1e9 * perm_ms / max(1.0, tested * args.perm * n_mean), 3),
           "genes_tested": full["genes_tested"], "significant": full["significant"],
           "planted_found": sum(1 for i, r in enumerate(rows) if i % 50 == 0 and r[15] not in ("NA",) and float(r[15]) <= 0.05)}
    res["spot_check"] = spot_check(bed_text, vcf_path, map_text, runs[args.perm][0]["genes"], args.seed, ctx)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
