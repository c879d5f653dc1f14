"""GTEx-shaped synthetic for phaser_ae_outlier (python -m phaser_amd.ae_outlier): --genes x --samples aCount|bCount cells with ae_test_scale.py's defaults,
the total of a cell drawn log-uniform from 1 to 10^5 and 2 % of the cells empty.  The counts are drawn from the model: every gene has its own s, log-uniform
in [0.01, 1.5], every cell its own x ~ N(0, s^2), aCount ~ Binomial(total, sigma(x)).  The matrix is written BGZF-compressed, as phaser_expr_matrix writes it.

One step on the GPU, under its own `timeout -k 10`: the CLI as a fresh process, once.  Reported: its wall time, its stage seconds, the device times of
K_blnfit, K_blntest and K_bh (HIP events, PHZ_T_BLNFIT / PHZ_T_BLNTEST / PHZ_T_BH) from its summary lines, the sizes of what it wrote, and a spot check
against the restatement of the tests (tests/ae_outlier_restatement.py, piecewise scipy.integrate.quad):
  p-values   200 cells whose reference is 1e-6 or more, at the printed sigma of their gene.  Six digits of sigma move such a p-value by (z^2 + 1) 5e-6 with
             z < 5 the cell's distance in sd, the text of the p-value by 5e-6 more: the bound is 2e-4.
  fits       three genes: a bounded Brent in ln s on the restated likelihood; the printed sigma may not lose more than 1e-3 in that likelihood.
  BH         the q-values of three whole columns from the printed p-values (scipy.stats.false_discovery_control), at 2e-5.
A miss ends the tool with status 1.

usage: python tools/ae_outlier_scale.py [--seed 0] [--genes 20000] [--samples 800] [--out DIR] [--threads 16] [--sigma auto]
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
sys.path.insert(0, os.path.join(REPO, "tests"))


def make_matrix(d, seed=0, n_genes=20000, n_samples=800, threads=16):
    from phaser_amd import vcfout
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    lines = ["\t".join(["#contig", "start", "stop", "name"] + ["SAMPLE%04d" % s for s in range(n_samples)])]
    per_contig = (n_genes + 21) // 22
    for g0 in range(0, n_genes, 500):                                  # 500 genes at a time: the cell text through numpy's string routines
        shape = (min(500, n_genes - g0), n_samples)
        n = np.exp(rng.uniform(0.0, np.log(1e5), shape)).astype(np.int64)
        s = np.exp(rng.uniform(np.log(0.01), np.log(1.5), (shape[0], 1)))
        a = rng.binomial(n, 1.0 / (1.0 + np.exp(-rng.normal(0.0, 1.0, shape) * s)))
        cells = np.char.add(np.char.add(a.astype(str), "|"), (n - a).astype(str))
        cells[rng.random(shape) < 0.02] = ""
        for i, row in enumerate(cells.tolist()):
            g = g0 + i
            start = 10_000 + (g % per_contig) * 5_000
            lines.append("\t".join(["chr%d" % (1 + g // per_contig), str(start), str(start + 3_000), "ENSG%011d" % g] + row))
    path = os.path.join(d, "matrix.bed.gz")
    text = "\n".join(lines) + "\n"
    vcfout.write_bgzf(path, text, threads)
    return path, len(text)


def spot_check(matrix_path, o, seed, fitted, n_genes=3, n_cells=200):
    import gzip
    from scipy.optimize import minimize_scalar
    from scipy.stats import false_discovery_control
    import ae_outlier_restatement as R
    rng = np.random.default_rng(seed + 1)
    text = {k: gzip.open("%s.%s.bed.gz" % (o, k), "rt").read().split("\n")[1:-1] for k in ("pvalue", "qvalue")}
    counts = gzip.open(matrix_path, "rt").read().split("\n")[1:-1]
    gene_var = [l.split("\t") for l in open(o + ".gene_var.txt").read().split("\n")[1:-1]]
    sigma = [float("nan") if f[5] == "NA" else float(f[5]) for f in gene_var]
    n_samples = len(counts[0].split("\t")) - 4
    worst_q = worst_p = 0.0
    for c in rng.choice(n_samples, 3, replace=False).tolist():
        cells = {k: [l.split("\t")[4 + c] for l in text[k]] for k in text}
        ok = [i for i, x in enumerate(cells["pvalue"]) if x != "NA"]
        assert [i for i, x in enumerate(cells["qvalue"]) if x != "NA"] == ok
        want = false_discovery_control(np.array([float(cells["pvalue"][i]) for i in ok]), method="bh")
        got = np.array([float(cells["qvalue"][i]) for i in ok])
        worst_q = max(worst_q, float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
    fits = []
    if fitted:
        for r in rng.choice(len(counts), n_genes, replace=False).tolist():
            ab = np.array([list(map(int, x.split("|"))) for x in counts[r].split("\t")[4:] if x != ""], dtype=np.int64)
            k, n = R.tested_cells(ab[:, 0], ab[:, 1], 8)
            assert int(gene_var[r][4]) == len(k)
            brent = R.fit_brent(k, n, 0.5)
            ll = R.restated_ll(k, n, 0.5, [brent, sigma[r]])
            fits.append({"gene": r, "cells": int(len(k)), "sigma": sigma[r], "sigma_brent": brent, "loglik_lost": float(ll[0] - ll[1]),
                         "printed_loglik_minus_restated": float(gene_var[r][6]) - float(ll[1])})
    checked = 0
    while checked < n_cells:
        r, c = int(rng.integers(0, len(counts))), int(rng.integers(0, n_samples))
        cell = counts[r].split("\t")[4 + c]
        got = text["pvalue"][r].split("\t")[4 + c]
        if cell == "" or sum(map(int, cell.split("|"))) < 8 or sigma[r] != sigma[r]:
            assert got == "NA", (r, c, cell, got)
            continue
        a, b = map(int, cell.split("|"))
        want, err = R.p_quad(a, a + b, 0.5, sigma[r])
        if want < 1e-6 or err > 1e-10:
            continue
        checked += 1
        worst_p = max(worst_p, abs(float(got) - want) / want)
    res = {"columns": 3, "cells": n_cells, "largest_relative_q_difference": worst_q, "largest_relative_p_difference": float(worst_p), "fitted_sigma": fits}
    if worst_q > 2e-5 or worst_p > 2e-4 or any(f["loglik_lost"] > 1e-3 for f in fits):
        print(json.dumps(res)); print("the spot check against the restatement failed")
        sys.exit(1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--genes", type=int, default=20000); ap.add_argument("--samples", type=int, default=800)
    ap.add_argument("--out", default="/tmp/ae_outlier_scale"); ap.add_argument("--threads", type=int, default=16); ap.add_argument("--sigma", default="auto")
    args = ap.parse_args()
    t0 = time.perf_counter()
    path, text_bytes = make_matrix(args.out, args.seed, args.genes, args.samples, args.threads)
    t_gen = time.perf_counter() - t0
    o = os.path.join(args.out, "out")
    cli = ["timeout", "-k", "10", "900", sys.executable, "-m", "phaser_amd.ae_outlier", "--bed", path, "--o", o, "--t", str(args.threads), "--sigma", args.sigma]
    t = time.perf_counter()
    r = subprocess.run(cli, cwd=REPO, capture_output=True, text=True)
    wall = time.perf_counter() - t
    print(r.stdout[-2500:])
    if r.returncode != 0:
        print(r.stderr[-3000:])
        print("the CLI failed with status %d" % r.returncode)
        sys.exit(r.returncode)
    m = re.search(r"(\d+) genes x (\d+) samples: (\d+) genes fitted, (\d+) cells tested, (\d+) with q <=", r.stdout)
    s = re.search(r"seconds (\{.*?\}); K_blnfit ([0-9.]+) ms, K_blntest ([0-9.]+) ms, K_bh ([0-9.]+) ms", r.stdout)
    res = {"genes": int(m.group(1)), "samples": int(m.group(2)), "cells": int(m.group(1)) * int(m.group(2)), "fitted": int(m.group(3)), "tested": int(m.group(4)),
           "significant": int(m.group(5)), "matrix_text_bytes": text_bytes, "matrix_bgzf_bytes": os.path.getsize(path), "generate_s": round(t_gen, 2),
           "cli_wall_s": round(wall, 3), "sigma": args.sigma, "stages_s": ast.literal_eval(s.group(1)), "k_blnfit_device_ms": float(s.group(2)),
           "k_blntest_device_ms": float(s.group(3)), "k_bh_device_ms": float(s.group(4)),
           "output_bytes": {k: os.path.getsize("%s.%s" % (o, k)) for k in ("gene_var.txt", "pvalue.bed.gz", "qvalue.bed.gz", "outliers.txt", "summary.txt")}}
    res["spot_check"] = spot_check(path, o, args.seed, args.sigma == "auto")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
