"""GTEx-shaped synthetic for phaser_ae_test (python -m phaser_amd.ae_test): --genes x --samples aCount|bCount cells, the total of a cell drawn
log-uniform from 1 to 10^5, aCount binomial at 0.5 -- or, for --imbalanced of the cells, at 0.5 +- 0.15 -- and 2 % of the cells empty.  The matrix is
written BGZF-compressed, as phaser_expr_matrix writes it.  With --true_rho the ratio of every cell is itself drawn from a beta distribution around that
mean (overdispersion rho: the counts are beta-binomial); it defaults to 0.02 when --overdispersion is on, to 0 (binomial counts) otherwise.

One step on the GPU, under its own `timeout -k 10`: the CLI as a fresh process.  Reported: its wall time, its stage seconds (parse, the two entry points
with their staging copies, the text of the two matrices, the significant / summary lists) and the device times of K_binom and K_bh (HIP events,
PHZ_T_BINOM / PHZ_T_BH) from its summary lines, and the sizes of what it wrote.  --overdispersion {auto | RHO} runs python -m phaser_amd.ae_betabinom with it; the device times
are then those of K_bbfit, K_bbtest and K_bh (PHZ_T_BBFIT / PHZ_T_BBTEST / PHZ_T_BH), and the spot check holds a sample of p-values and the fitted rho of
three columns against scipy.stats.betabinom.

usage: python tools/ae_test_scale.py [--seed 0] [--genes 20000] [--samples 800] [--imbalanced 0.05] [--out DIR] [--threads 16] [--overdispersion 0] [--true_rho RHO]
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


def make_matrix(d, seed=0, n_genes=20000, n_samples=800, imbalanced=0.05, threads=16, true_rho=0.0):
    from phaser_amd import vcfout
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    lines = ["\t".join(["#contig", "start", "stop", "name"] + ["SAMPLE%04d" % s for s in range(n_samples)])]
    per_contig = (n_genes + 21) // 22
    for g0 in range(0, n_genes, 500):                                  # 500 genes at a time: the cell text through numpy's string routines
        shape = (min(500, n_genes - g0), n_samples)
        n = np.exp(rng.uniform(0.0, np.log(1e5), shape)).astype(np.int64)
        ratio = np.where(rng.random(shape) < imbalanced, 0.5 + 0.15 * rng.choice([-1.0, 1.0], shape), 0.5)
        if true_rho > 0.0:                                                 # beta-binomial: the cell's own ratio around the mean
            spread = (1.0 - true_rho) / true_rho
            ratio = rng.beta(ratio * spread, (1.0 - ratio) * spread)
        a = rng.binomial(n, ratio)
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


def spot_check(matrix_path, o, seed, n_columns=3, n_cells=200):
    """what the run wrote against scipy, at the six digits of the text: the q-values of a few whole columns from the printed p-values, and the p-values
    of a few hundred cells from the matrix's counts -> the largest relative differences (a difference above 2e-5, twice the rounding of the text, ends the tool with status 1)"""
    import gzip
    from scipy.stats import binomtest, false_discovery_control
    rng = np.random.default_rng(seed + 1)
    text = {k: gzip.open("%s.%s.bed.gz" % (o, k), "rt").read().split("\n")[1:-1] for k in ("pvalue", "qvalue")}
    counts = gzip.open(matrix_path, "rt").read().split("\n")[1:-1]
    n_samples = len(counts[0].split("\t")) - 4
    worst_q = worst_p = 0.0
    for c in rng.choice(n_samples, n_columns, replace=False).tolist():
        cells = {k: [l.split("\t")[4 + c] for l in text[k]] for k in text}
        ok = [i for i, x in enumerate(cells["pvalue"]) if x != "NA"]
        assert [i for i, x in enumerate(cells["qvalue"]) if x != "NA"] == ok
        want = false_discovery_control(np.array([float(cells["pvalue"][i]) for i in ok]), method="bh")
        got = np.array([float(cells["qvalue"][i]) for i in ok])
        worst_q = max(worst_q, float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
    for _ in range(n_cells):
        r, c = int(rng.integers(0, len(counts))), int(rng.integers(0, n_samples))
        cell = counts[r].split("\t")[4 + c]
        got = text["pvalue"][r].split("\t")[4 + c]
        if cell == "" or sum(map(int, cell.split("|"))) < 8:
            assert got == "NA", (r, c, cell, got)
            continue
        a, b = map(int, cell.split("|"))
        want = binomtest(a, a + b, 0.5).pvalue
        if want < 1e-250:                                      # scipy's own tails underflow there
            assert float(got) < 1e-240, (r, c, cell, got)
            continue
        worst_p = max(worst_p, abs(float(got) - want) / max(want, 1e-300))
    res = {"columns": n_columns, "cells": n_cells, "largest_relative_q_difference": worst_q, "largest_relative_p_difference": float(worst_p)}
    if worst_q > 2e-5 or worst_p > 2e-5:
        print(json.dumps(res)); print("the spot check against scipy failed")
        sys.exit(1)
    return res


def betabinom_two_sided(k, n, p0, rho):
    """min(1, the sum of pmf(i) over all i in [0, n] with pmf(i) <= pmf(k) (1 + 1e-7)), scipy's pmf over the full support"""
    from scipy.stats import betabinom
    spread = (1.0 - rho) / rho
    pmf = betabinom.pmf(np.arange(n + 1), n, p0 * spread, (1.0 - p0) * spread)
    return min(1.0, float(pmf[pmf <= pmf[k] * (1 + 1e-7)].sum()))


def spot_check_betabinom(matrix_path, o, seed, fitted, n_columns=3, n_cells=200):
    """the overdispersed run against scipy.  The rho of a sample is read from summary.txt, six digits of it.  p-values: a few hundred cells whose reference is
    1e-6 or more, at the printed rho; six digits of rho move such a p-value by a few 1e-5 at most, the bound is 2e-4.  Fitted rho (--overdispersion auto): for
    three columns a bounded Brent in ln rho on scipy's summed log pmf; the printed rho may not lose more than 1e-3 in that likelihood (where the counts are
    binomial the likelihood is flat next to the lower bound, so the rho itself is only reported).  BH: as spot_check.  A miss ends the tool with status 1."""
    import gzip
    from scipy.optimize import minimize_scalar
    from scipy.stats import betabinom, false_discovery_control
    rng = np.random.default_rng(seed + 1)
    text = {k: gzip.open("%s.%s.bed.gz" % (o, k), "rt").read().split("\n")[1:-1] for k in ("pvalue", "qvalue")}
    counts = gzip.open(matrix_path, "rt").read().split("\n")[1:-1]
    summary = [l.split("\t") for l in open(o + ".summary.txt").read().split("\n")[1:-1]]
    rho = [float("nan") if f[4] == "NA" else float(f[4]) for f in summary]
    n_samples = len(rho)
    worst_q = worst_p = 0.0
    fits = []
    for c in rng.choice(n_samples, n_columns, replace=False).tolist():
        cells = {k: [l.split("\t")[4 + c] for l in text[k]] for k in text}
        ok = [i for i, x in enumerate(cells["pvalue"]) if x != "NA"]
        want = false_discovery_control(np.array([float(cells["pvalue"][i]) for i in ok]), method="bh")
        got = np.array([float(cells["qvalue"][i]) for i in ok])
        worst_q = max(worst_q, float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
        if fitted:
            ab = np.array([list(map(int, l.split("\t")[4 + c].split("|"))) for i, l in enumerate(counts) if cells["pvalue"][i] != "NA"], dtype=np.int64)
            k, n = ab[:, 0], ab[:, 0] + ab[:, 1]
            ll = lambda r: float(betabinom.logpmf(k, n, 0.5 * (1 - r) / r, 0.5 * (1 - r) / r).sum())
            res = minimize_scalar(lambda x: -ll(np.exp(x)), bounds=(np.log(1e-6), np.log(1.0 / 3.0)), method="bounded", options={"xatol": 1e-10})
            brent = float(np.exp(res.x))
            fits.append({"column": c, "cells": int(len(k)), "rho": rho[c], "rho_brent": brent, "loglik_lost": ll(brent) - ll(rho[c])})
    checked = 0
    while checked < n_cells:
        r, c = int(rng.integers(0, len(counts))), int(rng.integers(0, n_samples))
        cell = counts[r].split("\t")[4 + c]
        got = text["pvalue"][r].split("\t")[4 + c]
        if cell == "" or sum(map(int, cell.split("|"))) < 8:
            assert got == "NA", (r, c, cell, got)
            continue
        a, b = map(int, cell.split("|"))
        want = betabinom_two_sided(a, a + b, 0.5, rho[c])
        if want < 1e-6:
            continue
        checked += 1
        worst_p = max(worst_p, abs(float(got) - want) / want)
    res = {"columns": n_columns, "cells": n_cells, "largest_relative_q_difference": worst_q, "largest_relative_p_difference": float(worst_p), "fitted_rho": fits}
    if worst_q > 2e-5 or worst_p > 2e-4 or any(f["loglik_lost"] > 1e-3 for f in fits):
        print(json.dumps(res)); print("the spot check against scipy failed")
        sys.exit(1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--genes", type=int, default=20000); ap.add_argument("--samples", type=int, default=800)
    ap.add_argument("--imbalanced", type=float, default=0.05); ap.add_argument("--out", default="/tmp/ae_test_scale"); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--overdispersion", default="0"); ap.add_argument("--true_rho", type=float, default=None)
    args = ap.parse_args()
    on = args.overdispersion not in ("0", "0.0")
    true_rho = args.true_rho if args.true_rho is not None else (0.02 if on else 0.0)
    t0 = time.perf_counter()
    path, text_bytes = make_matrix(args.out, args.seed, args.genes, args.samples, args.imbalanced, args.threads, true_rho)
    t_gen = time.perf_counter() - t0
    o = os.path.join(args.out, "out")
    cli = ["timeout", "-k", "10", "900", sys.executable, "-m", "phaser_amd.ae_betabinom" if on else "phaser_amd.ae_test", "--bed", path, "--o", o, "--t", str(args.threads)] + \
          (["--overdispersion", args.overdispersion] if on else [])
    t = time.perf_counter()
    r = subprocess.run(cli, cwd=REPO, capture_output=True, text=True)
    wall = time.perf_counter() - t
    print(r.stdout[-2500:])
    if r.returncode != 0:
        print(r.stderr[-3000:])
        print("the CLI failed with status %d" % r.returncode)
        sys.exit(r.returncode)
    m = re.search(r"(\d+) genes x (\d+) samples: (\d+) cells tested, (\d+) with q <=", r.stdout)
    if on:
        s = re.search(r"seconds (\{.*?\}); K_bbfit ([0-9.]+) ms, K_bbtest ([0-9.]+) ms, K_bh ([0-9.]+) ms", r.stdout)
        device = {"k_bbfit_device_ms": float(s.group(2)), "k_bbtest_device_ms": float(s.group(3)), "k_bh_device_ms": float(s.group(4))}
    else:
        s = re.search(r"seconds (\{.*?\}); K_binom ([0-9.]+) ms, K_bh ([0-9.]+) ms", r.stdout)
        device = {"k_binom_device_ms": float(s.group(2)), "k_bh_device_ms": float(s.group(3))}
    res = {"genes": int(m.group(1)), "samples": int(m.group(2)), "cells": int(m.group(1)) * int(m.group(2)), "tested": int(m.group(3)), "significant": int(m.group(4)),
           "matrix_text_bytes": text_bytes, "matrix_bgzf_bytes": os.path.getsize(path), "generate_s": round(t_gen, 2), "cli_wall_s": round(wall, 3),
           "overdispersion": args.overdispersion, "true_rho": true_rho, "stages_s": ast.literal_eval(s.group(1)), **device,
           "output_bytes": {k: os.path.getsize("%s.%s" % (o, k)) for k in ("pvalue.bed.gz", "qvalue.bed.gz", "significant.txt", "summary.txt")}}
    res["spot_check"] = spot_check_betabinom(path, o, args.seed, args.overdispersion == "auto") if on else spot_check(path, o, args.seed)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
