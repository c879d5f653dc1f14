"""Population synthetic for phaser_sample_match (python -m phaser_amd.sample_match), generated on the fly: --donors donors with random genotypes (hom-ref
0.45, het 0.4, hom-alt 0.15, and --nocall of the cells without a call) at --sites panel sites; --samples samples, sample i drawn from donor i mod donors at
--covered of the sites, coverage 8 to 60, binomial read sampling at --error; --swaps of the samples claim each other's donors in a cycle.

--mode cli (default): the counts files, the bgzipped and indexed VCF and the map are written, and the CLI runs as a fresh process under its own
`timeout -k 10`.  Reported: its wall time, its stage seconds, the device time of K_match (HIP events) from its summary lines, and whether exactly the
planted swaps came back as MISMATCH with the true donor as best while every other sample is a MATCH.
--mode kernels: no text; phz_sample_match on device arrays, once to warm up and --reps times more: the device ms of each repeat, whether the repeats give
identical bits, the (sample, donor, entry) look-ups per second of the best repeat, and the same sums by a vectorised numpy gather on one core over
--numpy_samples of the samples, as a ratio of seconds per look-up.

usage: python tools/sample_match_scale.py [--mode cli|kernels] [--seed 0] [--donors 1000] [--samples 1000] [--sites 50000] [--covered 3000] [--swaps 20]
                                          [--error 0.01] [--nocall 0.01] [--out DIR] [--threads 16] [--reps 3] [--numpy_samples 8]
"""
import argparse
import ast
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_population(args):
    """-> geno uint8 [sites, donors], per sample (sorted site indices, ref counts, alt counts), the swapped samples, claimed donor per sample"""
    rng = np.random.default_rng(args.seed)
    geno = rng.choice(np.array([1, 2, 3], dtype=np.uint8), size=(args.sites, args.donors), p=[0.45, 0.4, 0.15])
    geno[rng.random(geno.shape) < args.nocall] = 0
    p_alt = np.array([0.5, args.error, 0.5, 1.0 - args.error])          # a donor without a call: the reads of a het
    samples = []
    for i in range(args.samples):
        d = i % args.donors
        sites = np.sort(rng.choice(args.sites, size=min(args.covered, args.sites), replace=False))
        total = rng.integers(8, 61, size=len(sites))
        alt = rng.binomial(total, p_alt[geno[sites, d]])
        samples.append((sites, (total - alt).astype(np.int32), alt.astype(np.int32)))
    swapped = np.sort(rng.choice(min(args.samples, args.donors), size=args.swaps, replace=False)) if args.swaps else np.zeros(0, dtype=np.int64)
    claimed = np.arange(args.samples) % args.donors
    for k, s in enumerate(swapped):
        claimed[s] = swapped[(k + 1) % len(swapped)] % args.donors
    return geno, samples, swapped.tolist(), claimed


def site_key(j):
    return "chr%d" % (1 + j % 22), 1000 + 50 * (j // 22), "ACGT"[j % 4], "CGTA"[j % 4]


def write_inputs(args, geno, samples, claimed):
    from phaser_amd import vcfout
    cdir = os.path.join(args.out, "counts")
    os.makedirs(cdir, exist_ok=True)
    donors = ["DONOR%05d" % d for d in range(args.donors)]
    names = ["SAMPLE%05d" % i for i in range(args.samples)]
    keys = [site_key(j) for j in range(args.sites)]
    order = sorted(range(args.sites), key=lambda j: (j % 22, j // 22))          # position-sorted inside each contig
    gt = np.array(["./.", "0|0", "0|1", "1|1"])
    lines = ["##fileformat=VCFv4.2", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + donors)]
    for j in order:
        c, p, r, a = keys[j]
        lines.append("\t".join([c, str(p), "v%d" % j, r, a, ".", "PASS", ".", "GT"] + gt[geno[j]].tolist()))
    vcf = os.path.join(args.out, "pop.vcf.gz")
    text = "\n".join(lines) + "\n"
    assert vcfout.write_bgzf(vcf, text, args.threads, index="vcf")
    head = "contig\tposition\tvariantID\trefAllele\taltAllele\trefCount\taltCount\ttotalCount"
    n_bytes = 0
    for name, (sites, ref, alt) in zip(names, samples):
        rows = [head] + ["%s\t%d\tv%d\t%s\t%s\t%d\t%d\t%d" % (keys[j][0], keys[j][1], j, keys[j][2], keys[j][3], r, a, r + a)
                         for j, r, a in zip(sites.tolist(), ref.tolist(), alt.tolist())]
        body = "\n".join(rows) + "\n"
        n_bytes += len(body)
        with open(os.path.join(cdir, name + ".allelic_counts.txt"), "w") as f:
            f.write(body)
    mp = os.path.join(args.out, "map.txt")
    with open(mp, "w") as f:
        f.write("vcf_sample\tbed_sample\n" + "".join("%s\t%s\n" % (donors[claimed[i]], names[i]) for i in range(args.samples)))
    return cdir, vcf, mp, donors, names, len(text), n_bytes


def run_cli(args):
    t0 = time.perf_counter()
    geno, samples, swapped, claimed = make_population(args)
    cdir, vcf, mp, donors, names, vcf_bytes, counts_bytes = write_inputs(args, geno, samples, claimed)
    t_gen = time.perf_counter() - t0
    o = os.path.join(args.out, "out")
    cli = ["timeout", "-k", "10", "900", sys.executable, "-m", "phaser_amd.sample_match", "--counts_dir", cdir, "--vcf", vcf, "--map", mp, "--o", o, "--error", repr(args.error),
           "--max_sites", str(args.sites), "--t", str(args.threads)]
    t = time.perf_counter()
    r = subprocess.run(cli, cwd=REPO, capture_output=True, text=True)
    wall = time.perf_counter() - t
    print(r.stdout[-2500:])
    if r.returncode != 0:
        print(r.stderr[-3000:])
        print("the CLI failed with status %d" % r.returncode)
        sys.exit(r.returncode)
    m = re.search(r"(\d+) samples x (\d+) donors, (\d+) panel keys \(union (\d+), (\d+) not in the VCF\), (\d+) entries", r.stdout)
    s = re.search(r"seconds (\{.*?\}); K_match ([0-9.]+) ms", r.stdout)
    rows = [l.split("\t") for l in open(o + ".matches.txt").read().split("\n")[1:] if l]
    truth = {names[i]: donors[i % args.donors] for i in range(args.samples)}
    planted = {names[i] for i in swapped}
    reported = {x[0] for x in rows if x[-1] == "MISMATCH"}
    wrong_best = [x[0] for x in rows if x[7] != truth[x[0]]]
    other = sorted({x[-1] for x in rows if x[-1] not in ("MATCH", "MISMATCH")})
    lookups = int(m.group(6)) * int(m.group(2))
    res = {"samples": int(m.group(1)), "donors": int(m.group(2)), "panel_keys": int(m.group(3)), "union_keys": int(m.group(4)), "entries": int(m.group(6)),
           "vcf_text_bytes": vcf_bytes, "vcf_bgzf_bytes": os.path.getsize(vcf), "counts_text_bytes": counts_bytes, "generate_s": round(t_gen, 2), "cli_wall_s": round(wall, 3),
           "stages_s": ast.literal_eval(s.group(1)), "k_match_device_ms": float(s.group(2)), "lookups": lookups, "lookups_per_s": round(lookups / (float(s.group(2)) * 1e-3)),
           "planted_swaps": len(planted), "reported_mismatches": len(reported), "planted_not_reported": sorted(planted - reported), "invented": sorted(reported - planted),
           "samples_whose_best_is_not_the_true_donor": wrong_best, "verdicts_other_than_match_and_mismatch": other}
    print(json.dumps(res))
    if planted != reported or wrong_best or other:
        print("the planted swaps did not come back as planted")
        sys.exit(1)


def run_kernels(args):
    import torch
    from phaser_amd import _lib, sample_match
    geno, samples, _, _ = make_population(args)
    e_off = np.zeros(args.samples + 1, dtype=np.int64)
    e_off[1:] = np.cumsum([len(s[0]) for s in samples])
    e_site = np.concatenate([s[0] for s in samples]).astype(np.int32); e_ref = np.concatenate([s[1] for s in samples]); e_alt = np.concatenate([s[2] for s in samples])
    ctx = _lib.Context(0)
    dev = torch.device("cuda", ctx.device)
    t = [torch.from_numpy(x).to(dev) for x in (geno, e_off, e_site, e_ref, e_alt)]
    S, D = args.samples, args.donors
    arg = _lib.phz_match_in()
    arg.n_sites, arg.n_samples, arg.n_donors = args.sites, S, D
    arg.geno, arg.e_off, arg.e_site, arg.e_ref, arg.e_alt = (x.data_ptr() for x in t)
    lr, la = sample_match.log_tables(args.error)
    arg.log_ref = (C.c_double * 3)(*lr); arg.log_alt = (C.c_double * 3)(*la)
    arg.cap, arg.het_permille = 30, 100
    ms, outs = [], []
    for _ in range(1 + args.reps):
        o = [torch.zeros((S, D), dtype=torch.float64, device=dev), torch.zeros((S, D), dtype=torch.int32, device=dev), torch.zeros((S, D), dtype=torch.int32, device=dev)]
        torch.cuda.synchronize(dev)
        ctx.check(ctx.lib.phz_sample_match(ctx.h, C.byref(arg), C.c_void_p(o[0].data_ptr()), C.c_void_p(o[1].data_ptr()), C.c_void_p(o[2].data_ptr()), _lib.PHZ_DEVICE))
        ms.append(ctx.timing(_lib.PHZ_T_MATCH)[0])
        outs.append([x.cpu().numpy() for x in o])
    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for k in range(1, len(outs)) for a, b in zip(outs[0], outs[k]))
    lookups = int(e_off[-1]) * D
    best = min(ms[1:])
    res = {"library": os.environ.get("PHZ_LIB_PATH", "phaser_amd/libphz.so"), "samples": S, "donors": D, "sites": args.sites, "entries": int(e_off[-1]), "lookups": lookups,
           "k_match_ms_first": round(ms[0], 3), "k_match_ms": [round(x, 3) for x in ms[1:]], "repeats_give_identical_bits": bool(same),
           "lookups_per_s": round(lookups / (best * 1e-3)), "geno_bytes": int(geno.size), "packed_bytes": int(args.sites * ((D + 15) // 16) * 4)}
    if args.numpy_samples > 0:
        # the same sums on one core: per sample one gather of the donors' codes at its sites, one gather of the terms by code, one sum over the entries
        n = min(args.numpy_samples, S)
        worst = 0.0
        t0 = time.perf_counter()
        for i in range(n):
            sites, ref, alt = samples[i]
            total = ref.astype(np.int64) + alt
            r = np.where(total > 30, (ref.astype(np.int64) * 30 + total // 2) // total, ref); a = np.where(total > 30, 30 - r, alt)
            terms = np.zeros((len(sites), 4))
            for g in range(3):
                terms[:, g + 1] = r * lr[g] + a * la[g]
            codes = geno[sites]
            ll = np.take_along_axis(terms, codes.astype(np.int64), axis=1).sum(axis=0)
            nc = (codes != 0).sum(axis=0)
            if i == 0:
                t_first = time.perf_counter() - t0
            worst = max(worst, float(np.max(np.abs(ll - outs[-1][0][i]) / np.maximum(1.0, np.abs(ll)))))
            assert np.array_equal(nc, outs[-1][1][i])
        dt = time.perf_counter() - t0
        n_look = int(e_off[n]) * D
        res["numpy"] = {"samples": n, "lookups": n_look, "seconds_one_core": round(dt, 3), "seconds_per_lookup": dt / n_look,
                        "largest_relative_difference_of_loglik": worst, "ratio_to_k_match_per_lookup": round((dt / n_look) / (best * 1e-3 / lookups))}
        if worst > 1e-9 * math.sqrt(args.covered):
            print(json.dumps(res)); print("the numpy sums differ from K_match's")
            sys.exit(1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["cli", "kernels"], default="cli")
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--donors", type=int, default=1000); ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--sites", type=int, default=50000); ap.add_argument("--covered", type=int, default=3000); ap.add_argument("--swaps", type=int, default=20)
    ap.add_argument("--error", type=float, default=0.01); ap.add_argument("--nocall", type=float, default=0.01)
    ap.add_argument("--out", default="/tmp/sample_match_scale"); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--numpy_samples", type=int, default=8)
    args = ap.parse_args()
    (run_cli if args.mode == "cli" else run_kernels)(args)


if __name__ == "__main__":
    main()
