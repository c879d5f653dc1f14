"""Genome-shaped synthetic for phaser_annotate (python -m phaser_amd.annotate): one sample whose variants sit in --genes genes with a heavy-tailed
size distribution (a Pareto body, the largest genes at --max-gene entries), a CADD-shaped table (100 columns, BGZF + .tbi) with a row for every
variant, genotypes phased in GT (70 %), phased by reads only (PG + PI, 20 %) or in both with a PI block.

Steps, each GPU step under its own `timeout -k 10`, the next one only after the last one succeeded:
  1. the CLI as a fresh process: wall time, its stage seconds and K_annot's device time (HIP events, PHZ_T_ANNOT) from its summary lines;
  2. `rocprofv3 --kernel-trace --stats -- python -m phaser_amd.annotate ...` in a run of its own: the k_annot dispatches' total, as a cross-check.
Then, on this host's CPU, the restatement's pair loop (tests/annotate_restatement.py: gene_rows) is timed on a stated subset of the genes and
extrapolated to all genes by ordered-pair count -- an extrapolation, printed as such.

usage: python tools/annotate_scale.py [--seed 0] [--genes 6000] [--max-gene 2000] [--out DIR] [--threads 16] [--baseline-pairs 400000] [--no-rocprof]
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SAMPLE = "SAMPLE1"
EFFECTS = ["INTRONIC", "SYNONYMOUS", "NON_SYNONYMOUS", "UPSTREAM", "DOWNSTREAM", "3PRIME_UTR", "SPLICE_SITE", "STOP_GAINED"]


def gene_sizes(rng, n_genes, max_gene):
    s = np.minimum((rng.pareto(1.3, n_genes) * 5).astype(np.int64) + 1, max_gene)
    s[rng.integers(0, n_genes, 3)] = max_gene                  # the tail: three genes at the cap
    return s


def make_inputs(d, seed=0, n_genes=6000, max_gene=2000):
    """-> paths + per-gene (vcf lines, cadd lines) so that a subset can be replayed by the restatement"""
    from phaser_amd import vcfout
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    sizes = gene_sizes(rng, n_genes, max_gene)
    filler = ["f%d" % i for i in range(100)]
    head = "##fileformat=VCFv4.2\n#" + "\t".join(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT", SAMPLE]) + "\n"
    vcf, cadd, per_gene = [], [], []
    block = 0
    in_contig = {}
    for g, n in enumerate(sizes.tolist()):
        contig = str(1 + g * 22 // n_genes)
        gene = "ENSG%011d" % g
        in_contig[contig] = in_contig.get(contig, -1) + 1
        start = 10_000 + in_contig[contig] * 60 * max_gene          # genes do not overlap: a gene spans less than 60 x max_gene bases
        pos = start + np.cumsum(rng.integers(1, 60, n))
        kind = rng.random(n)
        hap = rng.integers(0, 2, n)
        vl, cl = [], []
        for i, p in enumerate(pos.tolist()):
            if i % 64 == 0:
                block += 1                                     # a read-backed block spans up to 64 neighbouring variants
            gt = "0|1" if hap[i] else "1|0"
            if kind[i] < 0.02:
                gt = "1|1"
            if kind[i] < 0.70:
                cell, fmt = gt, "GT"
            elif kind[i] < 0.90:
                cell, fmt = "0/1:%s:%d" % (gt, block), "GT:PG:PI"
            else:
                cell, fmt = "%s:%s:%d" % (gt, gt, block), "GT:PG:PI"
            vl.append("%s\t%d\trs%d_%d\tA\tG\t.\tPASS\tAF=%.4f\t%s\t%s" % (contig, p, g, i, float(rng.random()), fmt, cell))
            f = list(filler)
            f[0], f[1], f[2], f[3], f[4], f[10], f[92], f[95], f[99] = contig, str(p), "A", "NA", "G", EFFECTS[i % 8], gene, "GENE%d" % g, "%.3f" % (40 * float(rng.random()))
            cl.append("\t".join(f))
        vcf.extend(vl); cadd.extend(cl); per_gene.append((vl, cl))
    # both files sorted by (contig, position): genes of one contig interleave
    def key(line):
        c = line.split("\t", 2)
        return int(c[0]), int(c[1])
    vcf.sort(key=key); cadd.sort(key=key)
    paths = {"vcf": os.path.join(d, "sample.vcf"), "cadd": os.path.join(d, "cadd.tsv.gz")}
    open(paths["vcf"], "w").write(head + "\n".join(vcf) + "\n")
    assert vcfout.write_bgzf(paths["cadd"], "## CADD-shaped synthetic\n#Chrom\tPos\tRef\tAnc\tAlt\n" + "\n".join(cadd) + "\n", 16, index="vcf")
    return paths, sizes, per_gene, head


def restatement_seconds(per_gene, head, sizes, budget_pairs):
    """the restatement's step 4 on the first genes in file order (the largest skipped) until `budget_pairs` ordered pairs are covered"""
    import annotate_restatement as R
    pick, pairs = [], 0
    for g, n in enumerate(sizes.tolist()):
        if n > 400:
            continue
        pick.append(g); pairs += 2 * n * n          # an upper bound; the exact count comes from the tables below
        if pairs >= budget_pairs:
            break
    vcf_text = head + "".join(l + "\n" for g in pick for l in per_gene[g][0])
    rows = {}
    for g in pick:
        for l in per_gene[g][1]:
            f = l.split("\t")
            rows.setdefault((f[0], int(f[1])), []).append(f)
    T = R.build_tables(vcf_text, SAMPLE, rows)
    t = time.perf_counter()
    n_rows = 0
    for gene in T["gene_order"]:
        n_rows += len(R.gene_rows(T, gene))
    return time.perf_counter() - t, R.pair_count(T), len(pick), n_rows


def run(cmd, limit, log):
    full = ["timeout", "-k", "10", str(limit)] + cmd
    t = time.perf_counter()
    r = subprocess.run(full, cwd=REPO, capture_output=True, text=True)
    wall = time.perf_counter() - t
    log.write(r.stdout[-4000:] + r.stderr[-2000:])
    if r.returncode != 0:
        print(r.stdout[-3000:], r.stderr[-3000:])
        print("step failed with status %d: nothing more is started" % r.returncode)
        sys.exit(r.returncode)
    return r.stdout, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--genes", type=int, default=6000)
    ap.add_argument("--max-gene", type=int, default=2000); ap.add_argument("--out", default="/tmp/annotate_scale")
    ap.add_argument("--threads", type=int, default=16); ap.add_argument("--baseline-pairs", type=int, default=400000)
    ap.add_argument("--no-rocprof", action="store_true")
    args = ap.parse_args()
    t0 = time.perf_counter()
    paths, sizes, per_gene, head = make_inputs(args.out, args.seed, args.genes, args.max_gene)
    t_gen = time.perf_counter() - t0
    o = os.path.join(args.out, "annotate.txt")
    cli = [sys.executable, "-m", "phaser_amd.annotate", "--geno_vcf", paths["vcf"], "--sample", SAMPLE, "--cadd_file", paths["cadd"], "--o", o,
           "--threads", str(args.threads)]
    log = open(os.path.join(args.out, "steps.log"), "w")
    out, wall = run(cli, 900, log)
    print(out[-1500:])
    m = re.search(r"(\d+) genes, (\d+) variants, (\d+) ordered pairs -> (\d+) rows in (\d+) batch\(es\); K_annot ([0-9.]+) ms", out)
    stages = dict((k, float(v)) for k, v in re.findall(r"(\w+) ([0-9.]+)", out[out.index("seconds:"):].split("\n")[0]))
    genes, variants, pairs, rows, batches = (int(x) for x in m.groups()[:5])
    dev_s = float(m.group(6)) / 1e3
    res = {"genes": genes, "variants": variants, "largest_gene": int(sizes.max()), "genes_over_1000": int((sizes > 1000).sum()), "pairs": pairs, "rows": rows,
           "batches": batches, "output_bytes": os.path.getsize(o), "generate_s": round(t_gen, 2), "cli_wall_s": round(wall, 3), "stages_s": stages,
           "k_annot_device_s": round(dev_s, 6), "pairs_per_s": pairs / dev_s if dev_s else None, "rows_per_s": rows / dev_s if dev_s else None}
    if not args.no_rocprof:
        pdir = os.path.join(args.out, "rocprof")
        run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "annot", "--"] + cli, 900, log)
        total_ns, calls = 0, 0
        for f in glob.glob(os.path.join(pdir, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "k_annot" in r["Name"]:
                    total_ns += int(r["TotalDurationNs"]); calls += int(r["Calls"])
            import shutil
            shutil.copy(f, os.path.join(args.out, "annotate_kernel_stats.csv"))
        res["rocprof_k_annot_s"] = round(total_ns / 1e9, 6); res["rocprof_k_annot_dispatches"] = calls
    cpu_s, cpu_pairs, cpu_genes, cpu_rows = restatement_seconds(per_gene, head, sizes, args.baseline_pairs)
    res.update({"restatement_pair_loop_cpu_s_timed": round(cpu_s, 3), "restatement_genes_timed": cpu_genes, "restatement_pairs_timed": cpu_pairs,
                "restatement_rows_timed": cpu_rows,
                "restatement_pair_loop_cpu_s_extrapolated_by_pairs": round(cpu_s / max(1, cpu_pairs) * pairs, 1)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
