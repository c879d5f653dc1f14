"""Population-pair synthetic for phaser_ae_diff (python -m phaser_amd.ae_diff): two --genes x --samples aCount|bCount matrices of the same individuals.  A
cell's total is drawn log-uniform from 1 to --max_n per condition; aCount is binomial at 0.5 in both conditions, except that --changed of the genes have the
second condition's ratio moved by +-0.15 in every sample, and 2 % of the cells of either matrix are empty.  --heavy F replaces that fraction of the cells'
totals by about 50,000 per condition (N about 10^5): the heavy-tailed variant of the PHZ_FISHER_WAVE_N A/B.

--mode cli (default): both matrices are written BGZF-compressed, as phaser_expr_matrix writes them, and the CLI runs as a fresh process under its own
`timeout -k 10`.  Reported: its wall time, its stage seconds, the device times of K_fisher, K_cmh and K_bh (HIP events) from its summary lines, the sizes
of what it wrote, and a spot check of a few hundred printed p-values against scipy.stats.fisher_exact at the six digits of the text.
--mode kernels: no text; phz_fisher_test and phz_cmh_test on the arrays, --reps times, through whatever library PHZ_LIB_PATH selects (tools/build_variant.py):
the device ms of each, the cells per second they imply, and scipy.stats.fisher_exact looped over --scipy of the tested cells on one core, as a ratio of
seconds per tested cell.

usage: python tools/ae_diff_scale.py [--mode cli|kernels] [--seed 0] [--genes 20000] [--samples 1000] [--max_n 2000] [--heavy 0] [--changed 0.05] [--out DIR]
                                     [--threads 16] [--reps 3] [--scipy 10000]
"""
import argparse
import ast
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_counts(seed, n_genes, n_samples, max_n, heavy, changed, g0=0, g1=None):
    """-> a1, b1, a2, b2 int32 [g1 - g0, samples] of genes g0 .. g1: every gene from its own generator, so a slice equals the rows of the whole"""
    g1 = n_genes if g1 is None else g1
    out = [np.empty((g1 - g0, n_samples), dtype=np.int32) for _ in range(4)]
    for g in range(g0, g1):
        rng = np.random.default_rng([seed, g])
        shift = 0.15 * rng.choice([-1.0, 1.0]) if rng.random() < changed else 0.0
        for cond, ratio in ((0, 0.5), (1, 0.5 + shift)):
            n = np.exp(rng.uniform(0.0, np.log(max_n), n_samples)).astype(np.int64)
            if heavy > 0.0:
                big = rng.random(n_samples) < heavy
                n[big] = rng.integers(45000, 55000, int(big.sum()))
            a = rng.binomial(n, ratio)
            gone = rng.random(n_samples) < 0.02
            a[gone] = -1; n[gone] = -1
            out[2 * cond][g - g0] = a; out[2 * cond + 1][g - g0] = np.where(gone, -1, n - a)
    return out


def write_matrices(d, seed, n_genes, n_samples, max_n, heavy, changed, threads):
    from phaser_amd import vcfout
    os.makedirs(d, exist_ok=True)
    head = "\t".join(["#contig", "start", "stop", "name"] + ["SAMPLE%04d" % s for s in range(n_samples)])
    lines = [[head], [head]]
    per_contig = (n_genes + 21) // 22
    for g0 in range(0, n_genes, 500):                                  # 500 genes at a time: the cell text through numpy's string routines
        m = make_counts(seed, n_genes, n_samples, max_n, heavy, changed, g0, min(n_genes, g0 + 500))
        for cond in (0, 1):
            a, b = m[2 * cond], m[2 * cond + 1]
            cells = np.char.add(np.char.add(a.astype(str), "|"), b.astype(str))
            cells[a < 0] = ""
            for i, row in enumerate(cells.tolist()):
                g = g0 + i
                start = 10_000 + (g % per_contig) * 5_000
                lines[cond].append("\t".join(["chr%d" % (1 + g // per_contig), str(start), str(start + 3_000), "ENSG%011d" % g] + row))
    paths, sizes = [], []
    for cond in (0, 1):
        path = os.path.join(d, "cond%d.bed.gz" % (cond + 1))
        text = "\n".join(lines[cond]) + "\n"
        vcfout.write_bgzf(path, text, threads)
        paths.append(path); sizes.append(len(text))
    return paths, sizes


def spot_check(args, o, n_cells=300):
    """printed p-values of a few hundred cells against scipy.stats.fisher_exact on the generator's counts; a difference above 2e-5, twice the rounding of the
    text, ends the tool with status 1"""
    import gzip
    from scipy.stats import fisher_exact
    rng = np.random.default_rng(args.seed + 1)
    text = gzip.open(o + ".pvalue.bed.gz", "rt").read().split("\n")[1:-1]
    worst = 0.0
    for _ in range(n_cells):
        r, c = int(rng.integers(0, args.genes)), int(rng.integers(0, args.samples))
        a1, b1, a2, b2 = (int(m[0, c]) for m in make_counts(args.seed, args.genes, args.samples, args.max_n, args.heavy, args.changed, r, r + 1))
        got = text[r].split("\t")[4 + c]
        if a1 < 0 or a2 < 0 or a1 + b1 < 8 or a2 + b2 < 8:
            assert got == "NA", (r, c, got)
            continue
        want = fisher_exact([[a1, b1], [a2, b2]])[1]
        if want < 1e-250:
            assert float(got) < 1e-240, (r, c, got)
            continue
        worst = max(worst, abs(float(got) - want) / want)
    res = {"cells": n_cells, "largest_relative_p_difference": worst}
    if worst > 2e-5:
        print(json.dumps(res)); print("the spot check against scipy failed")
        sys.exit(1)
    return res


def run_cli(args):
    t0 = time.perf_counter()
    paths, sizes = write_matrices(args.out, args.seed, args.genes, args.samples, args.max_n, args.heavy, args.changed, args.threads)
    t_gen = time.perf_counter() - t0
    o = os.path.join(args.out, "out")
    cli = ["timeout", "-k", "10", "900", sys.executable, "-m", "phaser_amd.ae_diff", "--bed1", paths[0], "--bed2", paths[1], "--o", o, "--t", str(args.threads)]
    t = time.perf_counter()
    r = subprocess.run(cli, cwd=REPO, capture_output=True, text=True)
    wall = time.perf_counter() - t
    print(r.stdout[-2500:])
    if r.returncode != 0:
        print(r.stderr[-3000:])
        print("the CLI failed with status %d" % r.returncode)
        sys.exit(r.returncode)
    m = re.search(r"(\d+) genes x (\d+) samples: (\d+) cells tested, (\d+) with q <= \S+ (\d+) genes tested, (\d+) with q <=", r.stdout)
    s = re.search(r"seconds (\{.*?\}); K_fisher ([0-9.]+) ms, K_cmh ([0-9.]+) ms, K_bh ([0-9.]+) ms", r.stdout)
    cells = int(m.group(1)) * int(m.group(2))
    res = {"genes": int(m.group(1)), "samples": int(m.group(2)), "cells": cells, "tested": int(m.group(3)), "significant": int(m.group(4)),
           "genes_tested": int(m.group(5)), "genes_significant": int(m.group(6)), "max_n": args.max_n, "heavy": args.heavy,
           "matrix_text_bytes": sizes, "matrix_bgzf_bytes": [os.path.getsize(p) for p in paths], "generate_s": round(t_gen, 2), "cli_wall_s": round(wall, 3),
           "stages_s": ast.literal_eval(s.group(1)), "k_fisher_device_ms": float(s.group(2)), "k_cmh_device_ms": float(s.group(3)), "k_bh_device_ms": float(s.group(4)),
           "fisher_cells_per_s": round(cells / (float(s.group(2)) * 1e-3)),
           "output_bytes": {k: os.path.getsize("%s.%s" % (o, k)) for k in ("pvalue.bed.gz", "qvalue.bed.gz", "delta.bed.gz", "cells.txt", "genes.txt", "summary.txt")}}
    res["spot_check"] = spot_check(args, o)
    print(json.dumps(res))


def run_kernels(args):
    from phaser_amd import _lib, ae_diff
    os.makedirs(args.out, exist_ok=True)
    cache = os.path.join(args.out, "counts_s%d_g%d_c%d_n%d_h%g_d%g.npy" % (args.seed, args.genes, args.samples, args.max_n, args.heavy, args.changed))
    if os.path.exists(cache):
        m = list(np.load(cache))
    else:
        m = make_counts(args.seed, args.genes, args.samples, args.max_n, args.heavy, args.changed)
        np.save(cache, np.stack(m))
    ctx = _lib.Context(0)
    fisher_ms, cmh_ms = [], []
    for _ in range(args.reps):
        p = ae_diff.fisher_test(ctx.lib, ctx.h, *m, 8)
        fisher_ms.append(ctx.timing(_lib.PHZ_T_FISHER)[0])
        ae_diff.cmh_test(ctx.lib, ctx.h, *m, 8, 2, 1)
        cmh_ms.append(ctx.timing(_lib.PHZ_T_CMH)[0])
    cells = int(m[0].size)
    N = m[0].astype(np.int64) + m[1] + m[2] + m[3]
    res = {"library": os.environ.get("PHZ_LIB_PATH", "phaser_amd/libphz.so"), "genes": args.genes, "samples": args.samples, "cells": cells, "tested": int((~np.isnan(p)).sum()),
           "max_n": args.max_n, "heavy": args.heavy, "cells_with_N_above": {str(t): int((N[~np.isnan(p)] > t).sum()) for t in (512, 2048, 8192, 32768)},
           "k_fisher_ms": [round(x, 3) for x in fisher_ms], "k_cmh_ms": [round(x, 3) for x in cmh_ms],
           "fisher_cells_per_s": round(cells / (min(fisher_ms) * 1e-3)), "fisher_tested_cells_per_s": round(int((~np.isnan(p)).sum()) / (min(fisher_ms) * 1e-3)),
           "cmh_cells_per_s": round(cells / (min(cmh_ms) * 1e-3))}
    if args.scipy > 0:
        from scipy.stats import fisher_exact
        rng = np.random.default_rng(args.seed + 2)
        tested = np.flatnonzero(~np.isnan(p).reshape(-1))
        pick = rng.choice(tested, min(args.scipy, len(tested)), replace=False)
        tabs = [[[int(m[0].flat[i]), int(m[1].flat[i])], [int(m[2].flat[i]), int(m[3].flat[i])]] for i in pick]
        t = time.perf_counter()
        sp = np.array([fisher_exact(x)[1] for x in tabs])
        dt = time.perf_counter() - t
        ours = p.reshape(-1)[pick]
        ok = sp >= 1e-250
        rel = np.abs(ours[ok] - sp[ok]) / sp[ok]
        # fisher_exact counts an index as tied with k within a relative 1e-14 of its own pmf, the rule of K_fisher (R's) within 1e-7: a table with an index in
        # between differs by that index's whole pmf.  Those cells are counted, the largest difference is taken over the others.
        res["scipy"] = {"cells": int(len(pick)), "seconds_one_core": round(dt, 3), "seconds_per_cell": dt / len(pick),
                        "cells_differing_above_1e-6": int((rel > 1e-6).sum()), "largest_relative_difference_of_the_others": float(np.max(rel[rel <= 1e-6])),
                        "ratio_to_k_fisher_per_tested_cell": round((dt / len(pick)) / (min(fisher_ms) * 1e-3 / len(tested)))}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["cli", "kernels"], default="cli")
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--genes", type=int, default=20000); ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--max_n", type=int, default=2000); ap.add_argument("--heavy", type=float, default=0.0); ap.add_argument("--changed", type=float, default=0.05)
    ap.add_argument("--out", default="/tmp/ae_diff_scale"); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--scipy", type=int, default=10000)
    args = ap.parse_args()
    (run_cli if args.mode == "cli" else run_kernels)(args)


if __name__ == "__main__":
    main()
