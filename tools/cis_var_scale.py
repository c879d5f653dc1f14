"""GTEx-shaped synthetic for phaser_cis_var (python -m phaser_amd.cis_var): 670 samples, >= 100 k VCF records (BGZF + .tbi), a
matrix of about 20 k genes, 19,696 pairs -- some without a record, some with a REF/ALT mismatch and an ID match, some at positions
with two records.  Runs the CLI as a fresh process and reports stage times, K_boot's device time (HIP events), draws/s, the
kernel's share of the VALU issue rate from the op count below, and the reference estimator (numpy.random.choice + numpy.median,
bs per set, signed and |aFC| set of every group) timed on the groups of the first --baseline-pairs pairs (2 groups each) on this host,
extrapolated to all groups.

usage: python tools/cis_var_scale.py [--seed 0] [--pairs 19696] [--bs 10000] [--out DIR] [--baseline-pairs 100]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# VALU instructions per draw in K_boot's inner loop (phz_cisvar.hip), counted from the source: Philox4x32-10 = 10 rounds x
# (2 v_mul_hi + 2 v_mul_lo + 4 v_xor + 2 key adds) shared by 4 draws = 25; per draw: 64-bit offset test 4, (word * n) >> 32 1,
# rank split / address 3 -> ~33 VALU ops per draw.  MI355X: 256 CUs x 4 SIMDs, each issuing one wave64 VALU op per 4 cycles
# (16 lane-ops per cycle), at 2.4 GHz.
VALU_OPS_PER_DRAW = 33
VALU_LANE_OPS_PER_S = 256 * 4 * 64 / 4 * 2.4e9


def make_inputs(d, seed=0, n_pairs=19696, n_samples=670, n_records=100_000, n_genes=20_000):
    from phaser_amd import vcfout
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    samples = ["GTEX-%05d" % i for i in range(n_samples)]
    # sample columns: a pool of genotype rows (het rate ~ 0.3 per record, a few unphased / missing)
    gt_pool_codes = np.array(["0|0", "0|1", "1|0", "1|1", "0/1", "./."])
    pool = []
    for _ in range(512):
        maf = rng.uniform(0.05, 0.5)
        h1 = rng.random(n_samples) < maf; h2 = rng.random(n_samples) < maf
        code = np.where(h1 & h2, 3, np.where(h1, 2, np.where(h2, 1, 0)))
        code[rng.random(n_samples) < 0.01] = 4; code[rng.random(n_samples) < 0.005] = 5
        dp = rng.integers(0, 60, n_samples).astype(str)           # a per-sample subfield, as real VCFs carry: most sample fields are distinct texts
        pool.append("\t".join(np.char.add(np.char.add(gt_pool_codes[code], ":"), dp).tolist()))
    contigs = ["chr%d" % c for c in range(1, 23)]
    per = n_records // len(contigs) + 1
    lines = ["##fileformat=VCFv4.2", "#" + "\t".join(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples)]
    recs = []
    k = 0
    for c in contigs:
        pos = np.cumsum(rng.integers(50, 5000, per)) + 10_000
        for p in pos.tolist():
            if k >= n_records:
                break
            rid = "rs%d" % k
            lines.append("%s\t%d\t%s\tA\tG\t.\tPASS\t.\tGT:DP\t%s" % (c, p, rid, pool[int(rng.integers(0, len(pool)))]))
            recs.append((c, p, rid))
            if k % 97 == 5:            # a second record at the same position
                lines.append("%s\t%d\t%s_b\tA\tC\t.\tPASS\t.\tGT:DP\t%s" % (c, p, rid, pool[int(rng.integers(0, len(pool)))]))
            k += 1
    vcf = os.path.join(d, "gtex.vcf.gz")
    vcfout.write_bgzf(vcf, "\n".join(lines) + "\n", 16, index="vcf")
    # matrix: genes along the contigs, counts a|b from a pool of rows
    cpool = []
    for _ in range(256):
        tot = rng.negative_binomial(3, 0.05, n_samples)
        a = rng.binomial(tot, rng.beta(8, 8, n_samples))
        gw = rng.random(n_samples) < 0.9
        cpool.append("\t".join(np.where(gw, np.char.add(np.char.add(a.astype(str), "|"), (tot - a).astype(str)), "0|0").tolist()))
    gl = ["\t".join(["#contig", "start", "stop", "name"] + samples)]
    genes = []
    for i in range(n_genes):
        c = contigs[i * len(contigs) // n_genes]
        g = "ENSG%011d.%d" % (i, 1 + i % 9)
        genes.append(g)
        gl.append("%s\t%d\t%d\t%s\t%s" % (c, 10_000 + 1000 * i, 12_000 + 1000 * i, g, cpool[int(rng.integers(0, len(cpool)))]))
    bed = os.path.join(d, "gtex.gw_phased.bed.gz")
    vcfout.write_bgzf(bed, "\n".join(gl) + "\n", 16)
    pl = ["gene_id\tvar_id\tvar_contig\tvar_pos\tvar_ref\tvar_alt"]
    for j in range(n_pairs):
        c, p, rid = recs[int(rng.integers(0, len(recs)))]
        g = genes[int(rng.integers(0, n_genes))]
        if j % 50 == 7:
            p = p + 1                                  # no record
        pl.append("%s\t%s\t%s\t%d\t%s\t%s" % (g, rid, c, p, "C" if j % 23 == 3 else "A", "T" if j % 23 == 3 else "G"))
    pairs = os.path.join(d, "pairs.txt")
    open(pairs, "w").write("\n".join(pl) + "\n")
    mp = os.path.join(d, "map.txt")
    open(mp, "w").write("vcf_sample\tbed_sample\n" + "".join("%s\t%s\n" % (s, s) for s in samples))
    return {"vcf": vcf, "bed": bed, "pairs": pairs, "map": mp}


def reference_estimator_seconds(groups, bs):
    """the reference's bootstrap_ci on each group's signed and |aFC| set: bs x (numpy.random.choice + numpy.median) each"""
    t = time.perf_counter()
    for v in groups:
        for x in (v, np.abs(v)):
            for _ in range(bs):
                np.median(np.random.choice(x, replace=True, size=len(x)))
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--pairs", type=int, default=19696)
    ap.add_argument("--bs", type=int, default=10000); ap.add_argument("--out", default="/tmp/cis_var_scale")
    ap.add_argument("--baseline-pairs", type=int, default=100); ap.add_argument("--t", type=int, default=16)
    args = ap.parse_args()
    t0 = time.perf_counter()
    paths = make_inputs(args.out, args.seed, args.pairs)
    t_gen = time.perf_counter() - t0
    o = os.path.join(args.out, "cis_var.txt")
    cmd = [sys.executable, "-m", "phaser_amd.cis_var", "--bed", paths["bed"], "--vcf", paths["vcf"], "--pairs", paths["pairs"], "--map", paths["map"],
           "--o", o, "--bs", str(args.bs), "--t", str(args.t), "--seed", str(args.seed)]
    t1 = time.perf_counter()
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
    wall = time.perf_counter() - t1
    print(r.stdout[-3000:], r.stderr[-3000:])
    if r.returncode != 0:
        sys.exit(r.returncode)
    # stage times and device time of the same work in this process (the CLI prints no timings)
    from phaser_amd import _lib, cis_var
    st = {}
    ctx = _lib.Context(0)
    cis_var.cis_var(cis_var.read_text(paths["bed"]), paths["vcf"], open(paths["pairs"]).read(), open(paths["map"]).read(), bs=args.bs,
                    threads=args.t, seed=args.seed, stats=st, ctx=ctx)
    draws = st["draws"]
    dev_s = st["k_boot_ms"] / 1e3
    # CPU baseline on the first pairs' groups
    captured = {}

    def cap(bi):
        captured["bi"] = bi
        return np.full((bi.n_groups, 2, 4), np.nan), np.zeros((bi.n_groups, 2, 2), np.int64)
    cis_var.cis_var(cis_var.read_text(paths["bed"]), paths["vcf"], open(paths["pairs"]).read(), open(paths["map"]).read(), bs=args.bs,
                    seed=args.seed, _bootstrap=cap)
    bi = captured["bi"]
    nb = min(2 * args.baseline_pairs, bi.n_groups)             # a pair has a het and a hom group
    cpu_s = reference_estimator_seconds([bi.values[bi.off[g]:bi.off[g + 1]] for g in range(nb)], args.bs)
    res = {"pairs": args.pairs, "samples": 670, "bs": args.bs, "rows": st["rows"], "groups": st["groups"], "draws": draws,
           "generate_s": round(t_gen, 2), "cli_wall_s": round(wall, 3), "stages_s": st["seconds"], "k_boot_device_s": round(dev_s, 4),
           "draws_per_s": draws / dev_s if dev_s else None,
           "valu_share": draws * VALU_OPS_PER_DRAW / dev_s / VALU_LANE_OPS_PER_S if dev_s else None,
           "reference_estimator_cpu_s_timed": round(cpu_s, 2), "reference_estimator_groups_timed": nb,
           "reference_estimator_cpu_s_extrapolated": round(cpu_s / max(1, nb) * bi.n_groups, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
