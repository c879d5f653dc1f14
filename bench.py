#!/usr/bin/env python3
"""Headline benchmark: het-SNP allele calls/s + phased variants/s of the read-backed phasing hot path, whole-genome RNA-seq shape.

python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]       (N>1: launched by torch.distributed.run, one rank per GPU)

A plain run sets up, warms up, times the K steps, writes the call lists of the last step when --dump-outputs is given, and prints the line (`value`,
`ms_per_step`).  --full adds everything else: the re-checks of the call lists, the text-plane series and the roofline, the phasing pass, the CPU baselines,
the configs[1] entry, the from-files entries and the RCCL self-check.

Workload = BASELINE.json configs[2]: one GTEx-shape sample over the 22 autosomes, ~80M records of 76 bp and
~1.5M het SNPs distributed in proportion to chromosome length, packed as structure-of-arrays shards resident in HBM.
  * step (the K timed steps, `value`): K_map over every chromosome shard this rank owns, submitted as one batch
    (phz_map_reads_batch: the reference's pool.map over chromosomes, phaser.py:533) -> allele calls/s.
  * phasing pass (`phasing.value`, --full): stages T1-O2 on the same call lists -- AS cutoff (histogram + all-reduce), K_tally, noise
    all-reduce, pair tests, components, block phasing, the rows of the five files, gather to rank 0 -> phased variants/s.
With N GPUs the SAME 22 chromosomes are LPT-assigned to ranks by record count (strong scaling); both regions are bracketed by a
barrier + synchronize on every rank and the max over ranks is reported.
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import numpy as np
import torch
import torch.distributed as dist

HBM_PEAK_GBS = 8000.0     # MI355X spec (MI355X_MICROARCH.md); measured copy peak is ~6290 GB/s
CALL_BYTES = 9            # read_idx 4 + var_idx 4 + code 1: the call list the phasing stage reads (the two planes behind the mapper drop-in's allele TEXT, 8 B more, are timed apart)


DUMP_SAMPLE = 1 << 20     # calls per plane written by --dump-outputs (a seeded sample of them when the step made more)


def dump_calls(out_dir, planes, seed=0):
    """--dump-outputs: the call lists the timed step handed back in its last step, `planes` = [(read_idx, var_idx, code)] per shard in shard order, as
    float64 .npy files in out_dir (about 32 MB, whatever the workload):
      read_idx / var_idx / code  the shards' lists concatenated, at the positions call_index names: all of them up to DUMP_SAMPLE calls, beyond that a sample
                                 drawn with a fixed seed (the same positions in every run that made the same number of calls);
      calls_per_shard            the length of every shard's list;
      calls_sum_per_shard        per shard the sums of read_idx, var_idx and code over ALL its calls (int64 sums, exact in float64)."""
    os.makedirs(out_dir, exist_ok=True)
    counts = [int(p[0].numel()) for p in planes]
    total = sum(counts)
    sums = [[float(p[k].to(torch.int64).sum()) if counts[i] else 0.0 for k in range(3)] for i, p in enumerate(planes)]
    if total > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(seed).choice(total, DUMP_SAMPLE, replace=False))
    else:
        idx = np.arange(total)
    for k, name in enumerate(("read_idx", "var_idx", "code")):
        cat = torch.cat([p[k].to(torch.int64) for p in planes]) if total else torch.zeros(0, dtype=torch.int64)
        np.save(os.path.join(out_dir, name + ".npy"), cat[torch.from_numpy(idx).to(cat.device)].cpu().numpy().astype(np.float64))
        del cat
    np.save(os.path.join(out_dir, "call_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, "calls_per_shard.npy"), np.asarray(counts, dtype=np.float64))
    np.save(os.path.join(out_dir, "calls_sum_per_shard.npy"), np.asarray(sums, dtype=np.float64).reshape(len(planes), 3))


@contextlib.contextmanager
def reproducible_gene_draw():
    """The workload generator (synth.make_read_plan) places read pairs on genes with torch.multinomial.  On the GPU that draw is not reproducible
    for the ~12,000 genes of chr1 and chr2: about one call in ten returns a different draw (a few hundred of 20 M samples), so two runs would map
    different reads.  torch's deterministic mode makes it reproducible; this turns that mode on around torch.multinomial alone while the
    workload is generated, and leaves every other op as it is."""
    orig = torch.multinomial

    def multinomial(*args, **kw):
        prev = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)
        try:
            return orig(*args, **kw)
        finally:
            torch.use_deterministic_algorithms(prev)
    torch.multinomial = multinomial
    try:
        yield
    finally:
        torch.multinomial = orig


def file_sha(*paths):
    h = hashlib.sha256()
    for p in paths:
        h.update(open(os.path.join(REPO, p), "rb").read())
    return h.hexdigest()[:16]


def calibration():
    """The newest memory-counter calibration under profiles/ (tools/prof_calib.sh -> calibration.json): what rocprofv3's FETCH_SIZE / WRITE_SIZE report
    on gfx950 for access patterns with a KNOWN byte count -- coalesced streams of 4 and 16 bytes per lane, 1-byte gathers at one load per 32..512-byte
    unit in permuted and in address order (K_map's base / quality bytes under a het SNP), coalesced stores.  -> factors to multiply the counters by."""
    import glob
    for f in reversed(sorted(glob.glob(os.path.join(REPO, "profiles", "r*", "calib", "calibration.json")))):
        c = json.load(open(f))
        pt = c["patterns"]
        stream = [pt[k]["factor"] for k in ("stream4", "stream16") if pt.get(k, {}).get("factor")]
        # a gather that touches ONE byte of every 128-byte line must pull every line: bytes the DRAM side delivers = requests x 128 when the
        # launch takes as long as streaming the array (it does: see the table), and FETCH_SIZE reports 64 per request
        gather = [128.0 / pt[k]["fetch_bytes_reported_per_request"] for k in pt if k.startswith("gather_") and pt[k]["unit"] >= 128 and pt[k].get("fetch_bytes_reported_per_request")]
        write = [pt[k]["factor"] for k in ("write4", "write8", "write16") if pt.get(k, {}).get("factor")]
        # where the pass with the raw request counters exists: bytes by request size (128 x RDREQ_128B + 64 x RDREQ_64B + 32 x RDREQ_32B) over FETCH_SIZE
        by_size = []
        for k in pt:
            c = pt[k].get("counters_per_launch", {})
            if not k.startswith("write") and c.get("TCC_EA0_RDREQ_sum") and c.get("FETCH_SIZE"):
                by_size.append((128.0 * c.get("TCC_EA0_RDREQ_128B_sum", 0) + 64.0 * c.get("TCC_EA0_RDREQ_64B_sum", 0) + 32.0 * c.get("TCC_EA0_RDREQ_32B_sum", 0)) / (c["FETCH_SIZE"] * 1024))
        if stream and gather and write:
            return {"source": os.path.relpath(f, REPO), "fetch_factor_stream": sum(stream) / len(stream), "fetch_factor_gather": sum(gather) / len(gather),
                    "write_factor": sum(write) / len(write),
                    "fetch_factor_by_request_size": {"min": min(by_size), "max": max(by_size), "patterns": len(by_size)} if by_size else None,
                    "note": "FETCH_SIZE counts 64 B per read request while every read request of these patterns is a 128-byte one (TCC_EA0_RDREQ_128B = "
                            "TCC_EA0_RDREQ; rocprofv3's formula prices 128-byte requests through TCC_BUBBLE, which stays 0 on gfx950): streams report half their known "
                            "bytes, a lone 1-byte gather costs a 128-byte line and reports 64; WRITE_SIZE is exact for coalesced 4 / 8 / 16-byte stores (64-byte requests)"}
    return None


def _pmc_rows(d, name, kernel):
    import csv
    f = os.path.join(d, name + ".csv")
    acc = {}
    if os.path.exists(f):
        for r in csv.DictReader(open(f)):
            if kernel in r["Kernel_Name"]:
                acc.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    return {k: sum(v) / len(v) for k, v in acc.items()}


def pmc_traffic():
    """HBM bytes per k_map launch from a PMC summary committed under profiles/ (tools/prof_pmc_c3.sh: FETCH_SIZE, WRITE_SIZE and the raw TCC_EA0 request
    counters by size in separate rocprofv3 --pmc passes of this same command), priced with the CALIBRATED factors of calibration() -- and, where the
    request-size counters were collected, directly as 128 x RDREQ_128B + 64 x RDREQ_64B + 32 x RDREQ_32B.  The summary carries the hash of the kernel
    source it was measured on; a summary of an older kernel is NOT reported (None)."""
    import glob
    dirs = sorted(glob.glob(os.path.join(REPO, "profiles", "r*", "pmc_kmap_*")))
    src = file_sha("phaser_amd/csrc/phz_map.hip")
    cal = calibration()
    for d in reversed(dirs):
        meta = os.path.join(d, "meta.json")
        if not os.path.exists(meta):
            continue
        m = json.load(open(meta))
        if m.get("kernel_source_sha16") != src or m.get("workload") != "configs[2]":
            continue
        fetch = _pmc_rows(d, "fetch", "k_map").get("FETCH_SIZE"); write = _pmc_rows(d, "write", "k_map").get("WRITE_SIZE")
        if fetch is None or write is None:
            return None
        ff = cal["fetch_factor_gather"] if cal else 2.0          # K_map's misses are line misses of both kinds; the two factors agree (2.0)
        wf = cal["write_factor"] if cal else 1.0
        out = {"fetch_raw_kib": fetch, "write_kib": write, "fetch_factor": ff, "write_factor": wf,
               "bytes_per_launch": ff * fetch * 1024 + wf * write * 1024, "source": os.path.relpath(d, REPO), "kernel_source_sha16": src,
               "calibration": cal,
               "note": "mean over the k_map launches of this command; FETCH_SIZE x the calibrated factor + WRITE_SIZE x its factor (profiles/*/calib: gathers and "
                       "streams both cost a 128-byte line per L2 miss, reported as 64)"}
        ea = _pmc_rows(d, "ea_rd", "k_map"); ew = _pmc_rows(d, "ea_wr", "k_map")
        if ea.get("TCC_EA0_RDREQ_sum"):
            # the raw request counters of the same command: exact bytes by request size; this is the figure reported, FETCH_SIZE x factor stays as the cross-check
            n32 = ea.get("TCC_EA0_RDREQ_32B_sum", 0.0); n64 = ea.get("TCC_EA0_RDREQ_64B_sum", 0.0); n128 = ea.get("TCC_EA0_RDREQ_128B_sum", 0.0)
            rd = 32.0 * n32 + 64.0 * n64 + 128.0 * n128
            out["read_requests"] = {"all": ea["TCC_EA0_RDREQ_sum"], "32B": n32, "64B": n64, "128B": n128, "bytes_by_request_size": rd}
            wr = wf * write * 1024
            if ew.get("TCC_EA0_WRREQ_sum"):
                w64 = ew.get("TCC_EA0_WRREQ_64B_sum", 0.0)
                wr = 64.0 * w64 + 32.0 * (ew["TCC_EA0_WRREQ_sum"] - w64)
                out["write_requests"] = {"all": ew["TCC_EA0_WRREQ_sum"], "64B": w64, "bytes_by_request_size": wr}
            out["bytes_per_launch_from_fetch_size"] = out["bytes_per_launch"]
            out["bytes_per_launch"] = rd + wr
        insts = {k.replace("SQ_INSTS_", "").lower(): v for k, v in _pmc_rows(d, "sq1", "k_map").items() if k.startswith("SQ_INSTS_")}
        out["wave_insts_per_launch"] = insts
        return out
    return None


SURVEY_BYTES_PER_RECORD = 115.0          # L = 76, 1.6 CIGAR ops, 0.19 calls per record


def issue_rates(ctx):
    """Issue ceilings of the chip, measured live (phz_microbench: wave64 VALU / SALU / LDS instructions per second, best over 2..8 waves
    per SIMD); the figures of tools/ubench.py kept under profiles/ are the same measurement."""
    import ctypes as C
    out = {}
    for kind, name in ((0, "valu"), (1, "salu"), (2, "lds")):
        best = 0.0
        for w in (2, 4, 8):
            r = C.c_double(0); cu = C.c_int(0); mhz = C.c_int(0)
            ctx.check(ctx.lib.phz_microbench(ctx.h, kind, w, 4000, C.byref(r), C.byref(cu), C.byref(mhz)))
            best = max(best, r.value)
        out[name] = best
    return out


def pmc_traffic_tally():
    """HBM bytes per phasing pass of the K_tally family and of the device row stage from a PMC summary committed under profiles/
    (tools/prof_pmc_tally.sh; same rules as pmc_traffic: separate --pmc passes, FETCH_SIZE doubled, reported only while the kernel source
    hashes match)."""
    import glob
    src = file_sha("phaser_amd/csrc/phz_tally.hip"); src_rows = file_sha("phaser_amd/csrc/phz_rowsdev.hip")
    for d in reversed(sorted(glob.glob(os.path.join(REPO, "profiles", "r*", "pmc_ktally_*")))):
        meta = os.path.join(d, "meta.json")
        if not os.path.exists(meta):
            continue
        m = json.load(open(meta))
        if m.get("kernel_source_sha16") != src or m.get("workload") != "configs[2]" or not m.get("passes") or "kib" not in m:
            continue
        t = m["kib"]["tally"]
        cal = calibration(); ff = cal["fetch_factor_gather"] if cal else 2.0; wf = cal["write_factor"] if cal else 1.0
        out = {"bytes_per_pass": (ff * t["fetch"] + wf * t["write"]) * 1024 / m["passes"], "fetch_raw_kib_per_pass": t["fetch"] / m["passes"], "fetch_factor": ff, "write_factor": wf,
               "write_kib_per_pass": t["write"] / m["passes"], "source": os.path.relpath(d, REPO), "kernel_source_sha16": src,
               "note": "sum over the K_tally family (k_as_hist .. k_edge_final, incl. the scans / sorts in between) of one pass; FETCH_SIZE x the calibrated factor (profiles/*/calib) + WRITE_SIZE"}
        if m.get("rows_source_sha16") == src_rows:
            r = m["kib"]["rows"]
            out["row_stage_bytes_per_pass"] = (ff * r["fetch"] + wf * r["write"]) * 1024 / m["passes"]
        return out
    return None


def cpu_mapper_baseline(sample, vpos, baseq):
    """Mapper oracle (C restatement, kind 'port') on one host core and on all cores over a bounded sample."""
    import subprocess
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from helpers import oracle_map_readbatch, oracle_map_readbatch_threads
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle")])
    t0 = time.perf_counter()
    o_r, o_v, o_c, _ = oracle_map_readbatch(os.path.join(REPO, "oracle"), sample, vpos, baseq, with_text=False)
    dt = time.perf_counter() - t0
    cores = max(1, min(64, os.cpu_count() or 1))
    t0 = time.perf_counter()
    m_all = oracle_map_readbatch_threads(os.path.join(REPO, "oracle"), sample, vpos, baseq, cores)
    dt_all = time.perf_counter() - t0
    assert m_all == len(o_r)
    return (o_r, o_v, o_c), dt, (cores, dt_all)


def cpu_phasing_baseline(sample_chroms, vsets, shards, calls_of, mapper, baseq, all_cores_chroms=()):
    """oracle/phasing_oracle.py (CPU restatement of process_vcf's stages T1-O2, one core) on whole chromosomes of the same
    sample; the product path is run on exactly those chromosomes as well and the five files must agree (canonical form)."""
    sys.path.insert(0, os.path.join(REPO, "oracle")); sys.path.insert(0, os.path.join(REPO, "tests"))
    import phasing_oracle as po
    from helpers import OUTPUTS, canonical, call_text
    from phaser_amd import synth, vcf as pvcf
    from phaser_amd.engine import Engine, Config
    vs_list = [vsets[c] for c in sample_chroms]
    vcf_text = "\n".join(synth.vcf_lines(vs_list)) + "\n"
    texts = [call_text(vsets[c], shards[c], calls_of[c]) for c in sample_chroms]
    n_lines = sum(t.count("\n") for t in texts)
    t0 = time.perf_counter()
    ph = po.Phaser(["bench"], baseq=baseq)
    ph.add_bam(texts)
    want = ph.finish()
    dt = time.perf_counter() - t0
    eng = Engine(pvcf.load_variants(vcf_text), ["bench"], Config(baseq=baseq, host_threads=8, want_vcf=False), mapper=mapper)
    for c in sample_chroms:
        eng.add_mapped(0, c, shards[c], calls_of[c], int(shards[c].qid.max()) + 1)
    eng.close_bam(0)
    got = eng.finish()
    same = all(canonical(n, got[n]) == canonical(n, want[n]) for n in OUTPUTS) and eng.phased == ph.phased
    assert same, "product != phasing oracle on the sampled chromosomes"
    out = {"value": ph.phased / dt, "unit": "phased variants/s", "cores": 1, "kind": "port",
           "sample": "chromosomes %s of the same sample (%d call lines, %d phased variants) through oracle/phasing_oracle.py, %.1f s"
                     % ("+".join(sample_chroms), n_lines, ph.phased, dt),
           "parity_on_sample": "five output files identical in canonical form (%d phased variants)" % ph.phased,
           "reference_note": "the Python restatement is slower than the code it restates: the reference's own phasing core ran ~9e3 phased variants/s on one core in the build "
                             "container (BASELINE.md, stages #3-#6 of configs[0]); ratios of the GPU figure to THIS value overstate the distance to the reference about tenfold"}
    if all_cores_chroms:
        # one oracle process per chromosome, all at once (the reference's `parallelize` over contigs, phaser.py:2077-2094, "1 thread per contig")
        import subprocess, tempfile, shutil
        tmp = tempfile.mkdtemp(prefix="phz_bench_oracle_")
        try:
            paths = []
            for c in all_cores_chroms:
                pth = os.path.join(tmp, c + ".tsv")
                open(pth, "w").write(call_text(vsets[c], shards[c], calls_of[c]))
                paths.append(pth)
            t0 = time.perf_counter()
            procs = [subprocess.Popen([sys.executable, os.path.join(REPO, "tools", "oracle_chrom_worker.py"), pth, str(baseq)], stdout=subprocess.PIPE, text=True)
                     for pth in paths]
            res = [p_.communicate()[0].split() for p_ in procs]
            wall = time.perf_counter() - t0
            assert all(p_.returncode == 0 for p_ in procs)
            phased = sum(int(r[0]) for r in res)
            out["all_cores"] = {"value": phased / wall, "unit": "phased variants/s", "processes": len(paths), "cores": min(len(paths), os.cpu_count() or 1),
                                "seconds": wall, "cpu_seconds": sum(float(r[1]) for r in res),
                                "sample": "one oracle process per chromosome, all started together: %s (%d phased variants)" % ("+".join(all_cores_chroms), phased)}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return out


def tally_roofline(tally_bytes, tally_ms, world):
    """K_tally family: frac = measured HBM bytes per pass (committed PMC passes, calibrated) / HIP-event time of the family / 8 TB/s when a summary of the current
    source exists, else SURVEY 8(d)'s algorithmic bytes over the same time (a lower bound)."""
    tr = pmc_traffic_tally() if world == 1 else None
    sec = tally_ms / 1e3
    moved = tr["bytes_per_pass"] if tr else tally_bytes
    ach = moved / sec / 1e9 if sec > 0 else None
    return {"bound": "hbm", "kernel": "K_tally (all kernels of phz_tally, HIP events on the ctx stream)", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS if ach else None, "traffic": tr["bytes_per_pass"] if tr else None, "traffic_detail": tr,
            "traffic_over_algorithmic": (tr["bytes_per_pass"] / tally_bytes) if tr and tally_bytes else None,
            "algorithmic_bytes": tally_bytes, "algorithmic_frac": tally_bytes / sec / 1e9 / HBM_PEAK_GBS if sec > 0 else None}


def kmap_roofline(ctx, tot_recs, alg, k_avg_s, k_launches, steps, k_ms_max_rank, world):
    """K_map against the chip, in PHYSICAL terms only (round-4 verdict: the line must not carry a fraction above 1):
      frac / achieved  = the HBM bytes the kernel really moves per launch (committed PMC passes, FETCH_SIZE / WRITE_SIZE priced with the calibration of
                         profiles/*/calib) / HIP-event time of the launch, against the 8 TB/s peak; when no PMC summary matches the current kernel
                         source, the gather-aware algorithmic minimum below stands in (a lower bound of the traffic, so still a true fraction);
      issue_*          = its wave64 instruction counts (PMC SQ_INSTS_*) against the chip's measured issue rates (phz_microbench, run live);
      bound            = the largest of those physical fractions;
      algorithmic_bytes_per_launch = what ANY kernel with this design must move: the per-record arrays it streams (pos, cigar_off, seq_off, CIGAR words,
                         the het-SNP positions) + one 128-byte DRAM line per DISTINCT line of the quality / base arrays that holds a byte under an
                         emitted call (the granule the calibration measured) + 9 bytes per emitted call; traffic / that = wasted re-reads;
      model_streaming  = SURVEY.md 8(d)'s 115 B per record (every base and quality of every record streamed): the bytes of a DIFFERENT algorithm, kept as
                         the rate a streaming mapper would need -- not a fraction of anything this kernel does."""
    recs_per_launch = tot_recs / max(1.0, k_launches / steps)
    alg_min = alg["stream_bytes"] + 128.0 * (alg["qual_lines"] + alg["seq_lines"]) + CALL_BYTES * alg["calls"]
    tr = pmc_traffic() if world == 1 else None
    fr = {}
    issue = None
    if tr is not None:
        fr["hbm_measured_traffic"] = tr["bytes_per_launch"] / k_avg_s / 1e9 / HBM_PEAK_GBS
        if tr.get("wave_insts_per_launch"):
            rates = issue_rates(ctx)
            wi = tr["wave_insts_per_launch"]
            issue = {k: {"wave_insts_per_launch": wi.get(k), "peak_wave_insts_per_s": rates[k], "frac": wi[k] / rates[k] / k_avg_s} for k in ("valu", "salu", "lds") if k in wi}
            for k, v in issue.items():
                fr["issue_" + k] = v["frac"]
    else:
        fr["hbm_algorithmic_minimum"] = alg_min / k_avg_s / 1e9 / HBM_PEAK_GBS
    traffic = tr["bytes_per_launch"] if tr is not None else None
    moved = traffic if traffic is not None else alg_min
    achieved = moved / k_avg_s / 1e9
    bound = max(fr, key=lambda k: fr[k])
    return {"bound": bound, "bound_class": "hbm" if bound.startswith("hbm") else "instruction issue / memory latency (integer-branch kernel: no MFMA work on this path)",
            "kernel": "k_map", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic, "traffic_over_algorithmic": (traffic / alg_min) if traffic is not None else None,
            "algorithmic_bytes_per_launch": alg_min,
            "algorithmic_detail": {"streamed_arrays": alg["stream_bytes"], "qual_lines_128B": alg["qual_lines"], "seq2_lines_128B": alg["seq_lines"],
                                   "emitted_calls": alg["calls"], "bytes_per_call_out": CALL_BYTES, "per_record": alg_min / recs_per_launch,
                                   "streamed_arrays_per_record": alg["stream_bytes"] / recs_per_launch},
            "fractions": fr, "traffic_detail": tr, "issue": issue,
            "model_streaming": {"bytes_per_record": SURVEY_BYTES_PER_RECORD, "bytes_per_launch": SURVEY_BYTES_PER_RECORD * recs_per_launch,
                                "GBps_a_streaming_mapper_would_need_at_this_speed": SURVEY_BYTES_PER_RECORD * recs_per_launch / k_avg_s / 1e9,
                                "note": "SURVEY.md 8(d): all arrays of a record incl. ALL its bases and qualities.  K_map reads bases / qualities only under a het SNP, so it "
                                        "does not move these bytes; the figure is not a fraction of this kernel's ceiling and is not reported as one"},
            "kernel_ms_avg": k_avg_s * 1e3, "launches": int(k_launches), "kernel_ms_per_step_max_rank": k_ms_max_rank / steps,
            "note": "frac = measured HBM bytes per launch (calibrated PMC counters) / HIP-event kernel time / 8 TB/s.  The kernel is paced by memory LATENCY at the "
                    "hardware's occupancy limit and by the scalar issue port (DESIGN 4), not by bandwidth: bound names the busiest physical resource"}


def algorithmic_minimum(shards, vposs, bufs_aux, n_calls):
    """Gather-aware lower bound of K_map's HBM traffic on this rank's shards (kmap_roofline): bytes of the arrays every record streams, and the DISTINCT
    128-byte lines of qual / seq2 that hold a byte under an emitted call (aux0 = the base's read offset, from the submission with the text planes)."""
    out = {"stream_bytes": 0.0, "qual_lines": 0.0, "seq_lines": 0.0, "calls": 0.0}
    for sh, vp, b, m in zip(shards, vposs, bufs_aux, n_calls):
        out["stream_bytes"] += float(sum(int(t.numel()) * t.element_size() for t in (sh.pos, sh.cigar_off, sh.cigar, sh.seq_off)) + 4 * int(vp.numel()))
        out["calls"] += float(m)
        if m == 0:
            continue
        rd = b[0][:m].to(torch.int64); a0 = b[3][:m].to(torch.int64) & 0xFFFFFFFF
        ok = a0 != 0xFFFFFFFF
        so = sh.seq_off.to(torch.int64)[rd]
        out["qual_lines"] += float(torch.unique(((so * 4 + a0)[ok]) >> 7).numel())
        out["seq_lines"] += float(torch.unique(((so + (a0 >> 2))[ok]) >> 7).numel())
    return out


def rccl_selfcheck(local):
    """N = 1 has no collective on its path (dist.py short-circuits them), so the line of a one-GPU box would never show RCCL running.  This runs the
    multi-rank layer's own collectives (dist.allreduce_sum_, allreduce_counts, the int64 all-gather) over a world-size-1 process group on backend
    "nccl" (= RCCL) after the measurements, and reports whether librccl is mapped into the process.  (The whole CLI through that path:
    tests/test_gpu_pipeline.py::test_one_rank_forced_through_every_collective.)"""
    from phaser_amd import dist as pdist
    out = {"backend": "nccl (RCCL)", "world_size": 1}
    old = os.environ.get("PHZ_DIST_FORCE_COLLECTIVES")
    try:
        os.environ["PHZ_DIST_FORCE_COLLECTIVES"] = "1"
        t0 = time.perf_counter()
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % (29500 + os.getpid() % 2000), rank=0, world_size=1, device_id=torch.device("cuda", local))
        t = torch.arange(8, dtype=torch.int64, device="cuda:%d" % local)
        pdist.allreduce_sum_(t); torch.cuda.synchronize()
        out["init_plus_first_all_reduce_s"] = time.perf_counter() - t0
        ok = bool((t.cpu() == torch.arange(8)).all()) and pdist.allreduce_counts(5, 7) == (5, 7) and pdist._all_gather_i64([3, 1, 4]) == [[3, 1, 4]]
        h = torch.zeros(65536, dtype=torch.int64, device="cuda:%d" % local); h[100] = 3
        t1 = time.perf_counter()
        for _ in range(20):
            pdist.allreduce_sum_(h)
        torch.cuda.synchronize()
        out["as_histogram_all_reduce_us"] = (time.perf_counter() - t1) / 20 * 1e6
        out["rccl_ranks"] = int(dist.get_world_size()); out["collectives_ok"] = ok and int(h[100]) == 3
        out["librccl_mapped"] = "librccl" in open("/proc/self/maps").read()
        dist.destroy_process_group()
    except Exception as e:                       # a side entry must never cost the bench line
        out["error"] = "%s: %s" % (type(e).__name__, e)
    finally:
        if old is None:
            os.environ.pop("PHZ_DIST_FORCE_COLLECTIVES", None)
        else:
            os.environ["PHZ_DIST_FORCE_COLLECTIVES"] = old
    return out


def self_launch(n):
    """Replace this process by `python -m torch.distributed.run --nnodes=1 --nproc-per-node n bench.py <same arguments>` (rendezvous on 127.0.0.1, a
    free port).  Never returns."""
    import socket
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush(); sys.stderr.flush()
    os.execvpe(sys.executable, cmd, env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # 200 steps = 0.3 s of timed steps by default (twenty 1.5 ms steps were a fragile headline); --from-files: 5 steps of ~0.3 s by default
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: the re-checks of the call lists, the text-plane series and the roofline, the phasing pass, "
                         "the CPU baselines, the configs[1] entry, the from-files entries and the RCCL self-check (the --no-* switches below prune this set)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the call lists of the last step to DIR/*.npy (float64; a seeded sample of 2^20 calls, see dump_calls)")
    ap.add_argument("--records", type=int, default=80_000_000)
    ap.add_argument("--snps", type=int, default=1_500_000)
    ap.add_argument("--baseq", type=int, default=10)
    ap.add_argument("--phasing-passes", type=int, default=5)
    ap.add_argument("--from-files", action="store_true", help="second strong-scaling mode: the sample is a BAM on disk; a step decodes the rank's chromosomes on its GPU and maps them")
    ap.add_argument("--no-phasing", action="store_true", help="skip the phasing-stage measurement")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baselines")
    ap.add_argument("--no-c2", action="store_true", help="skip the secondary configs[1] entry (chr1, 50M records, 40k het SNPs)")
    ap.add_argument("--no-bam", action="store_true", help="skip the from-files entries (a whole-genome BAM + VCF written to /tmp: bam_path = decoded on the GPU and on the host, end_to_end_files = the CLI on them)")
    a = ap.parse_args()
    if a.steps is None:
        a.steps = 5 if a.from_files else 200
    if a.steps < 1:
        ap.error("--steps must be at least 1")

    # `python bench.py --gpus N` by itself (no launcher): start N ranks of this script, one per GPU, under torch.distributed.run and let them
    # print the line (the reference's fan-out, phaser.py:2077-2094, is one Pool worker per chromosome; here one process per GPU)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(a.gpus)
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d: the launcher and the flag disagree (refusing to print a line for another rank count)" % (a.gpus, world))
    if os.environ.get("PHZ_BENCH_BACKEND", "nccl") == "nccl" and torch.cuda.device_count() < a.gpus:
        sys.exit("bench.py: --gpus %d needs %d visible GPUs, this node shows %d (PHZ_BENCH_BACKEND=gloo lets ranks share a GPU for plumbing checks only)"
                 % (a.gpus, a.gpus, torch.cuda.device_count()))
    # the container's CPU quota (cpu.max), not the host's core count, bounds what torch's intra-op pool may use: 256 OpenMP threads
    # spinning on a 16-CPU quota get the whole cgroup throttled, timed regions included
    from phaser_amd import dist as pdist
    torch.set_num_threads(max(1, min(torch.get_num_threads(), pdist.effective_cpus() // max(1, world))))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # one rank per GPU over RCCL ("nccl"); PHZ_BENCH_BACKEND=gloo lets several ranks share a GPU (used only to exercise the
    # multi-rank path on a 1-GPU box)
    backend = os.environ.get("PHZ_BENCH_BACKEND", "nccl")
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    dev = "cuda:%d" % local
    red_dev = dev if backend == "nccl" else "cpu"
    dev_names = ["rank %d: cuda:%d" % (rank, local)]
    if world > 1:
        names = [None] * world
        dist.all_gather_object(names, dev_names[0])
        dev_names = names

    if a.from_files:
        from_files_mode(a, rank, world, local, dev, red_dev, backend, dev_names)
        if world > 1:
            dist.destroy_process_group()
        return
    from phaser_amd import workloads, synth, vcf as pvcf
    from phaser_amd import dist as pdist
    from phaser_amd.mapper import Mapper, Calls
    from phaser_amd.engine import Engine, Config
    from phaser_amd import _lib

    plan = workloads.genome_plan(a.records, a.snps)
    owner = pdist.assign_chromosomes({p[0]: float(p[3]) for p in plan}, world)       # LPT by record count
    mine = [p for p in plan if owner[p[0]] == rank]
    want_cpu = a.full and rank == 0 and world == 1 and not a.no_cpu
    t_gen = time.perf_counter()
    vsets = {}; shards = {}; sample = None
    with reproducible_gene_draw():
        for chrom, ln, n_snps, n_rec, seed in mine:
            v, shard, smp = workloads.make_shard(chrom, ln, n_snps, n_rec, seed, dev, keep_sample=n_rec if (want_cpu and chrom == "chr1") else 0)
            vsets[chrom] = v; shards[chrom] = shard
            if smp is not None:
                sample = smp
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t_gen
    mapper = Mapper(local)
    chroms = [p[0] for p in mine]
    sh_list = [shards[c] for c in chroms]
    vp_list = [vsets[c].pos for c in chroms]

    # first (untimed) pass sizes the output buffers; the timed passes reuse exact-size buffers through the raw ABI
    first = mapper.map_batch(sh_list, vp_list, a.baseq)
    n_calls = [c.n for c in first]
    # the timed step produces what Engine.add_shards asks K_map for -- (record, variant, allele code) per call, SURVEY.md 8(a) M1's GPU form; the
    # same submission with the two extra planes of the mapper drop-in's text output is timed after it (config.step_with_text_planes_ms)
    call, bufs, N = mapper.prepare_batch(sh_list, vp_list, a.baseq, [n + 16 for n in n_calls], aux=False)

    def step():
        mapper.ctx.check(call())

    for _ in range(a.warmup):
        step()
    import gc
    time.sleep(0.12)                    # let a CPU-quota period that the set-up may have exhausted run out before the timed region starts
    gc.collect(); gc.disable()          # before the barrier: a collector pause inside the timed steps (1.5 ms each) would be a visible share of a short run
    mapper.ctx.reset_timing()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stamps = [t0]
    for _ in range(a.steps):
        step()                                   # returns after the submission's own host wait: the stamps are per-step wall times
        stamps.append(time.perf_counter())
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    gc.enable()
    per_step = sorted((stamps[i + 1] - stamps[i]) * 1e3 for i in range(a.steps))
    _, k_total_ms, k_n = mapper.ctx.timing(_lib.PHZ_T_MAP)
    assert [int(N[i]) for i in range(len(chroms))] == n_calls
    if a.dump_outputs:
        dump_calls(a.dump_outputs if world == 1 else os.path.join(a.dump_outputs, "rank%d" % rank),
                   [[b[:n_calls[i]] for b in bufs[i][:3]] for i in range(len(chroms))])

    ms_with_text = None
    alg_loc = {"stream_bytes": 0.0, "qual_lines": 0.0, "seq_lines": 0.0}
    if a.full:
        # idempotence + mapper order (sortedness) on every shard at full size
        for i, c in enumerate(chroms):
            m = n_calls[i]
            f = first[i]
            assert all(bool(torch.equal(b[:m], t)) for b, t in zip(bufs[i][:3], (f.read_idx, f.var_idx, f.code))), "repeated passes differ"
            key = bufs[i][0][:m].to(torch.int64) * (len(vsets[c]) + 1) + bufs[i][1][:m].to(torch.int64)
            assert bool((key[1:] > key[:-1]).all()), "call list not in mapper order"

        # the same submission with the text planes (what the mapper drop-in asks for): a short series, reported next to the headline
        call5, bufs5, N5 = mapper.prepare_batch(sh_list, vp_list, a.baseq, [n + 16 for n in n_calls], aux=True)
        for _ in range(2):
            mapper.ctx.check(call5())
        torch.cuda.synchronize(); t5 = time.perf_counter()
        for _ in range(max(1, min(a.steps, 20))):
            mapper.ctx.check(call5())
        torch.cuda.synchronize(); ms_with_text = (time.perf_counter() - t5) / max(1, min(a.steps, 20)) * 1e3
        for i in range(len(chroms)):
            m = n_calls[i]; f = first[i]
            assert all(bool(torch.equal(b[:m], t)) for b, t in zip(bufs5[i], (f.read_idx, f.var_idx, f.code, f.aux0, f.aux1))), "text planes differ between passes"
            assert all(bool(torch.equal(bufs5[i][k][:m], bufs[i][k][:m])) for k in range(3)), "call list differs with / without the text planes"
        alg_loc = algorithmic_minimum(sh_list, vp_list, bufs5, n_calls)
        del call5, bufs5
    loc_calls = float(sum(n_calls)); loc_recs = float(sum(s.n for s in sh_list)); loc_snps = float(sum(len(vsets[c]) for c in chroms))
    red = torch.tensor([loc_calls, loc_recs, loc_snps, alg_loc["stream_bytes"], k_total_ms, float(k_n), 1.0, alg_loc["qual_lines"], alg_loc["seq_lines"]],
                       device=red_dev, dtype=torch.float64)
    tmax = torch.tensor([dt, k_total_ms], device=red_dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(red); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    tot_calls, tot_recs, tot_snps, tot_stream, k_ms_sum, k_launches, ranks_seen, tot_ql, tot_sl = [float(x) for x in red.tolist()]
    alg = {"stream_bytes": tot_stream, "qual_lines": tot_ql, "seq_lines": tot_sl, "calls": tot_calls}
    assert int(ranks_seen) == world == a.gpus, "the all-reduce saw %d ranks, --gpus says %d" % (int(ranks_seen), a.gpus)
    dt = float(tmax[0]); k_ms_max_rank = float(tmax[1])

    # ---- second rate of the metric: phased variants/s over stages T1-O2 on the same call lists
    phasing = None
    gc.enable()
    if a.full and not a.no_phasing:
        vs = pvcf.load_variants("\n".join(synth.vcf_lines([workloads_variants(plan, vsets, p) for p in plan])))
        # host threads of the row writer: four per CPU the container may really use (quota-aware; the phases are short and bursty), shared by the ranks of the node
        host_threads = max(1, min(64, 4 * pdist.effective_cpus() // max(1, world)))
        if os.environ.get("PHZ_BENCH_HOST_THREADS"):
            host_threads = int(os.environ["PHZ_BENCH_HOST_THREADS"])
        calls_now = [Calls(*[None if t is None else t[:n_calls[i]] for t in bufs[i]]) for i in range(len(chroms))]
        # two series of passes: row text left in HBM (`value`: inputs and outputs resident, like the mapper step) and copied to page-locked
        # host memory (`d2h_inclusive`: what the CLI pays before it can write the files; PCIe-bound, ~1 GB per genome)
        series = {"resident": [], "d2h": []}
        for mode in ("resident", "d2h"):
            for rep in range(max(1, a.phasing_passes) + 1):          # the first pass of a series sizes buffers: not reported
                eng = Engine(vs, ["bench"], Config(baseq=a.baseq, host_threads=host_threads, want_vcf=False, fetch_text=(mode == "d2h"),
                                                   device_rows=os.environ.get("PHZ_BENCH_HOST_ROWS") != "1"), mapper=mapper)
                eng.set_owned(chroms)
                for i, c in enumerate(chroms):
                    eng.add_mapped(0, c, shards[c], calls_now[i], int(shards[c].qid.max()) + 1)
                mapper.ctx.reset_timing()
                gc.collect(); gc.disable()
                if world > 1:
                    dist.barrier()
                torch.cuda.synchronize()
                prof = None
                if os.environ.get("PHZ_BENCH_PYPROFILE") and mode == "resident" and rep == max(1, a.phasing_passes):      # host-side profile of the last resident pass
                    import cProfile
                    prof = cProfile.Profile(); prof.enable()
                tp0 = time.perf_counter()
                eng.close_bam(0)                       # AS histogram per shard + all-reduce + percentile
                tp1 = time.perf_counter()
                files = eng.finish(chunks=True)        # K_tally, noise all-reduce, pair tests, components, block phasing, rows, gather
                if prof is not None:
                    prof.disable()
                    import pstats
                    pstats.Stats(prof, stream=sys.stderr).sort_stats("tottime").print_stats(28)
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                tp2 = time.perf_counter()
                gc.enable()
                tt = torch.tensor([tp2 - tp0], device=red_dev, dtype=torch.float64)
                gpu_ms = sum(mapper.ctx.timing(sl)[1] for sl in (_lib.PHZ_T_ASHIST, _lib.PHZ_T_TALLY, _lib.PHZ_T_COMPONENTS, _lib.PHZ_T_ROWS))
                cnt = torch.tensor([float(mapper.ctx.counter(_lib.PHZ_C_LINES)), float(mapper.ctx.counter(_lib.PHZ_C_PAIR_EVENTS)),
                                    float(mapper.ctx.counter(_lib.PHZ_C_ITEMS)), float(mapper.ctx.counter(_lib.PHZ_C_EDGES)),
                                    mapper.ctx.timing(_lib.PHZ_T_TALLY)[1], float(eng.stats.get("rowsdev_text_bytes", 0.0))], device=red_dev, dtype=torch.float64)
                gm = torch.tensor([gpu_ms], device=red_dev, dtype=torch.float64)
                if world > 1:
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX); dist.all_reduce(cnt); dist.all_reduce(gm, op=dist.ReduceOp.MAX)
                if rank == 0 and rep > 0:
                    lines, events, items, edges, tally_ms, text_bytes = [float(x) for x in cnt.tolist()]
                    tally_bytes = 8.0 * lines + 16.0 * events
                    host_bytes = int(sum(len(x) for v_ in files.values() for x in v_))
                    series[mode].append({"value": eng.phased / float(tt[0]), "unit": "phased variants/s", "phased_variants": eng.phased,
                                 "seconds_per_pass": float(tt[0]), "call_lines_kept": eng.total_lines, "rows": getattr(eng, "rows_path", "host"),
                                 "output_bytes": int(text_bytes) if text_bytes else host_bytes,
                                 "gpu_ms_per_pass_max_rank": float(gm[0]), "gpu_share": float(gm[0]) / 1e3 / float(tt[0]),
                                 "seconds": {"as_cutoff": tp1 - tp0, "tally_to_rows_and_gather": tp2 - tp1,
                                             **{k: round(v_, 4) for k, v_ in eng.stats.items() if k.endswith("_s")}},
                                 "counts": {k: int(v_) for k, v_ in eng.stats.items() if k.startswith("rowsdev_n_")},
                                 "host_threads": host_threads,
                                 "roofline": tally_roofline(tally_bytes, tally_ms, world) | {
                                              "model": "8 B x call lines + 16 B x pair events (SURVEY.md 8(d))", "call_lines": lines,
                                              "pair_events": events, "items": items, "edges": edges, "kernel_ms_sum_over_ranks": tally_ms}})
                del eng, files
                pdist.cleanup_spool()          # every rank: the spooled row text of this pass is no longer needed
        if rank == 0:
            med = lambda runs: sorted(runs, key=lambda r: r["value"])[len(runs) // 2]
            phasing = dict(med(series["resident"]))
            phasing["passes"] = [round(r["value"]) for r in series["resident"]]
            phasing["statistic"] = ("value / seconds_per_pass = the MEDIAN of the listed passes; inputs (call lists) and outputs (the text of the five "
                                    "files) resident in HBM; d2h_inclusive = the same pass with the text copied to page-locked host memory")
            m2 = med(series["d2h"])
            phasing["d2h_inclusive"] = {"value": m2["value"], "seconds_per_pass": m2["seconds_per_pass"], "passes": [round(r["value"]) for r in series["d2h"]],
                                        "seconds": m2["seconds"], "gpu_share": m2["gpu_share"]}

    if rank == 0:
        k_avg_s = k_ms_sum / max(1.0, k_launches) / 1e3
        out = {
            "metric": "het-SNP allele calls/sec + phased variants/sec, whole-genome RNA-seq, 1→8 GPUs",
            "value": tot_calls * a.steps / dt, "unit": "allele calls/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "u8/int32", "data": "synthetic",
            "collective": {"backend": ("nccl (RCCL over xGMI)" if backend == "nccl" else backend) if world > 1 else "none (one rank)",
                           "rccl_ranks": int(ranks_seen) if backend == "nccl" and world > 1 else 0, "ranks_seen_by_all_reduce": int(ranks_seen),
                           "devices": sorted(set(dev_names))},
            "config": {"workload": "configs[2]: whole genome (22 autosomes), one GTEx-shape RNA-seq sample, %d records x 76 bp, %d het SNPs, "
                                   "one shard per chromosome; chromosomes LPT-assigned to GPUs by record count" % (int(tot_recs), int(tot_snps)),
                       "records": int(tot_recs), "het_snps": int(tot_snps), "calls_per_step": int(tot_calls), "shards": len(plan),
                       "records_per_s": tot_recs * a.steps / dt, "gen_seconds": round(t_gen, 1),
                       "step": "K_map over all chromosome shards of the rank in one batched submission (phz_map_reads_batch); call list = (record, variant, allele "
                               "code) per call, the form the phasing stage reads (SURVEY.md 8(a) M1)",
                       "step_ms_spread": {"min": per_step[0], "median": per_step[len(per_step) // 2], "p90": per_step[min(len(per_step) - 1, int(0.9 * len(per_step)))],
                                          "max": per_step[-1], "note": "wall time of the individual timed steps on rank 0 (ms_per_step is their mean incl. the closing barrier)"}},
        }
        if a.full:
            out["config"]["step_with_text_planes_ms"] = ms_with_text
            out["config"]["step_with_text_planes_note"] = ("the same submission also writing the two planes behind the mapper drop-in's allele text (read offset, "
                                                           "inserted bases: 8 more bytes per call), rank 0's shards, mean of a short series")
            out["full_output_step"] = {"ms_per_step": ms_with_text, "value": tot_calls / (ms_with_text / 1e3) if world == 1 else None, "unit": "allele calls/s",
                                       "bytes_per_call": 17,
                                       "note": "the same submission writing all five planes of a call (record, variant, code + read offset of the base + inserted-bases word), what "
                                               "the mapper drop-in (read_variant_map.do_read_variant_map) needs to print the allele text; rounds 1-3 reported THIS form as the "
                                               "headline, since round 4 `value` is the 9-byte form the phasing stage reads"}
            out["roofline"] = kmap_roofline(mapper.ctx, tot_recs, alg, k_avg_s, k_launches, a.steps, k_ms_max_rank, world)
        if phasing is not None:
            out["phasing"] = phasing
            out["end_to_end"] = {"seconds": dt / a.steps + phasing["seconds_per_pass"], "unit": "s per sample, shards resident in HBM -> rows of the five files on rank 0",
                                 "allele_calls_per_s": tot_calls / (dt / a.steps + phasing["seconds_per_pass"]),
                                 "phased_variants_per_s": phasing["phased_variants"] / (dt / a.steps + phasing["seconds_per_pass"])}
        if want_cpu and sample is not None:
            (o_r, o_v, o_c), cpu_dt, (cpu_cores, cpu_dt_all) = cpu_mapper_baseline(sample, vsets["chr1"].pos.numpy(), a.baseq)
            m = len(o_r)
            i1 = chroms.index("chr1")
            # at-scale parity: the GPU call list of the sampled chromosome equals the oracle's
            assert m == n_calls[i1] and np.array_equal(bufs[i1][0][:m].cpu().numpy(), o_r) and np.array_equal(bufs[i1][1][:m].cpu().numpy(), o_v) \
                and np.array_equal(bufs[i1][2][:m].cpu().numpy(), o_c), "GPU != oracle on the sampled chromosome"
            out["cpu_baseline"] = {"value": m / cpu_dt, "unit": "allele calls/s", "cores": 1, "kind": "port",
                                   "sample": "all %d records of chr1 of the same sample through oracle/rvm_oracle.c (array front end, "
                                             "no SAM text parsing), %.1f s; %.0f records/s" % (len(sample), cpu_dt, len(sample) / cpu_dt),
                                   "parity_on_sample": "bit-exact (%d calls)" % m,
                                   "all_cores": {"value": m / cpu_dt_all, "unit": "allele calls/s", "cores": cpu_cores,
                                                 "records_per_s": len(sample) / cpu_dt_all},
                                   "reference_note": "the reference's own Cython mapper ran 1.03e5 records/s/core in the build container "
                                                     "(BASELINE.md); this port is the faster, parity-locked stand-in on the GPU box"}
            del sample
            if phasing is not None:
                calls_of = {c: Calls(*[None if t is None else t[:n_calls[i]] for t in bufs[i]]) for i, c in enumerate(chroms)}
                phasing["cpu_baseline"] = cpu_phasing_baseline(["chr21", "chr22"], vsets, shards, calls_of, mapper, a.baseq,
                                                               all_cores_chroms=["chr%d" % i for i in range(15, 23)])
        if a.full and world == 1 and not a.no_c2:
            out["secondary"] = configs1_entry(mapper, a, dev)
        if a.full and world == 1 and not a.no_bam:
            try:
                out["bam_path"], out["end_to_end_files"] = files_entries(mapper, dev, a)
            except Exception as e:                      # a side entry must never cost the bench line
                out["bam_path"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if a.full and world == 1 and backend == "nccl":
            out["collective"]["rccl_selfcheck"] = rccl_selfcheck(local)
            out["collective"]["rccl_ranks"] = int(out["collective"]["rccl_selfcheck"].get("rccl_ranks", 0))
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


def workloads_variants(plan, vsets, p):
    """Variants of chromosome p for the VCF text every rank parses (chromosomes owned by other ranks are regenerated from the
    plan's seeds: the table is tiny next to the reads)."""
    from phaser_amd import synth
    if p[0] in vsets:
        return vsets[p[0]]
    v, _, _, _ = synth.make_variants(p[0], 1, p[1], p[2], p[4], n_genes=max(1, p[2] // 10))
    return v


def write_genome_files(tmp, a, dev):
    """The whole-genome sample of configs[2] as FILES in `tmp`: an unfiltered coordinate-sorted BAM (duplicates, improper pairs, low MAPQ present) and its
    bgzipped VCF, generated on `dev` and written by the library's native writers.  -> (bam path, vcf.gz path, variants per chromosome, BAM records, seconds)"""
    from phaser_amd import bamio, synth, workloads, vcfout
    path = os.path.join(tmp, "g.bam"); vcfgz = os.path.join(tmp, "g.vcf.gz")
    items = [("chr%d" % (i + 1), ln) for i, ln in enumerate(workloads.HG38_AUTOSOMES)]
    total_len = float(sum(workloads.HG38_AUTOSOMES))
    frac = a.records / 80_000_000.0
    batches = []; nrec = 0; vsets = []
    t0 = time.perf_counter()
    for i, (chrom, ln) in enumerate(items):
        n_snps = int(a.snps * ln / total_len); n_pairs = int(40_000_000 * frac * ln / total_len)
        v, gs, ge, w = synth.make_variants(chrom, 1, ln, n_snps, 777 + i, n_genes=max(1, n_snps // 10))
        with reproducible_gene_draw():
            plan = synth.make_read_plan(v, gs, ge, w, n_pairs, 1777 + i, device=dev)
        for lo in range(0, len(plan), 2_000_000):
            rb = synth.fill_reads(plan, lo, min(len(plan), lo + 2_000_000), v, qname_prefix="s0.b0.%d." % i)
            batches.append(synth.ReadBatch(rb.chrom, rb.L, rb.pos.cpu(), rb.flag.cpu(), rb.mapq.cpu(), rb.tlen.cpu(), rb.aln_score.cpu(), rb.qid.cpu(),
                                           rb.cigar_off.cpu(), rb.cigar.cpu(), rb.seq.cpu(), rb.qual.cpu(), rb.qname_prefix))
            nrec += len(rb)
            del rb
        vsets.append(v)
        del plan
    bamio.readbatch_to_bam_native(path, batches, [(c, l) for c, l in items], 0)
    vcfout.write_bgzf(vcfgz, "\n".join(synth.vcf_lines(vsets)) + "\n", 0, index="vcf")          # "must be gzipped and tabix indexed" (phaser.py:31)
    del batches
    torch.cuda.empty_cache()
    return path, vcfgz, vsets, nrec, time.perf_counter() - t0


def from_files_mode(a, rank, world, local, dev, red_dev, backend, dev_names):
    """`bench.py --from-files [--gpus N]`: the second strong-scaling entry (round-4 verdict, next #3).  The sample is a BAM on disk; a step is, on every rank,
    file -> BGZF members of the rank's chromosomes copied to ITS GPU -> K_inflate -> record hop / filters / k_pack / QNAME ids (phz_bamdev_*) -> K_map over the
    shards just decoded.  Chromosomes are LPT-assigned by the compressed bytes they occupy in the BAM (bamio.bam_ref_weights: known from the member table before
    anything is decoded; the reference's fan-out is one samtools | mapper pipeline per chromosome, phaser.py:533, :1330-1353).  No collective inside the step; the
    counts are all-reduced afterwards.  value = allele calls / s FROM THE FILE (PCIe, page cache and host CPUs included: not comparable with the resident line)."""
    import shutil, tempfile
    from phaser_amd import bamio, workloads, synth, _lib
    from phaser_amd import dist as pdist
    from phaser_amd.mapper import Mapper
    mapper = Mapper(local)
    tmp = os.environ.get("PHZ_BENCH_FILES_DIR") or os.path.join(tempfile.gettempdir(), "phz_bench_from_files_%s" % os.environ.get("MASTER_PORT", "single"))
    path = os.path.join(tmp, "g.bam")
    nrec_t = torch.zeros(1, dtype=torch.float64, device=red_dev)
    if rank == 0:
        shutil.rmtree(tmp, ignore_errors=True); os.makedirs(tmp)
        path, vcfgz, vsets_list, nrec, t_write = write_genome_files(tmp, a, dev)
        nrec_t[0] = nrec
    if world > 1:
        dist.barrier(); dist.all_reduce(nrec_t)
    nrec = int(nrec_t[0])
    try:
        items = [("chr%d" % (i + 1), ln) for i, ln in enumerate(workloads.HG38_AUTOSOMES)]
        total_len = float(sum(workloads.HG38_AUTOSOMES))
        w = bamio.bam_ref_weights(path, 0)
        owner = pdist.assign_chromosomes({c: float(w.get(c, 0)) for c, _ in items}, world)
        mine = [c for c, _ in items if owner[c] == rank]
        vpos = {}
        for i, (chrom, ln) in enumerate(items):
            if owner[chrom] == rank:          # the variants of the rank's chromosomes (the generator is seeded: the same table rank 0 wrote into the VCF)
                v, _, _, _ = synth.make_variants(chrom, 1, ln, int(a.snps * ln / total_len), 777 + i, n_genes=max(1, int(a.snps * ln / total_len) // 10))
                vpos[chrom] = v.pos
        def step():
            sh = bamio.shards_from_bam_device(mapper.ctx, path, {}, 255, True, True, 0.0, chroms=mine, device=dev) if mine else {}
            if sh is None:
                raise RuntimeError("the device BAM path declined the file")
            calls = mapper.map_batch([sh[c] for c in mine if c in sh], [vpos[c] for c in mine if c in sh], a.baseq, aux=False) if sh else []
            if a.dump_outputs:
                last[:] = calls           # the lists of the last step, for dump_calls
            return sum(c.n for c in calls), sum(s_.n for s_ in sh.values())
        last = []
        for _ in range(max(1, min(a.warmup, 2))):
            step()
        steps = a.steps
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(steps):
            n_calls, n_kept = step()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        if a.dump_outputs:
            dump_calls(a.dump_outputs if world == 1 else os.path.join(a.dump_outputs, "rank%d" % rank), [(c.read_idx, c.var_idx, c.code) for c in last])
        red = torch.tensor([float(n_calls), float(n_kept), 1.0, float(sum(w.get(c, 0) for c in mine))], device=red_dev, dtype=torch.float64)
        tmax = torch.tensor([dt], device=red_dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(red); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        if rank == 0:
            tot_calls, tot_kept, ranks_seen, tot_bytes = [float(x) for x in red.tolist()]
            dt = float(tmax[0])
            assert int(ranks_seen) == world == a.gpus
            shares = {}
            for c, _ in items:
                shares[owner[c]] = shares.get(owner[c], 0) + w.get(c, 0)
            print(json.dumps({
                "metric": "het-SNP allele calls/sec + phased variants/sec, whole-genome RNA-seq, 1→8 GPUs", "mode": "from-files",
                "value": tot_calls * steps / dt, "unit": "allele calls/s", "n_gpus": world, "steps": steps, "warmup": max(1, min(a.warmup, 2)), "ms_per_step": dt / steps * 1e3,
                "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u8/int32", "data": "synthetic",
                "collective": {"backend": ("nccl (RCCL over xGMI)" if backend == "nccl" else backend) if world > 1 else "none (one rank)",
                               "rccl_ranks": int(ranks_seen) if backend == "nccl" and world > 1 else 0, "ranks_seen_by_all_reduce": int(ranks_seen), "devices": sorted(set(dev_names))},
                "config": {"workload": "configs[2] FROM FILES: one unfiltered whole-genome BAM (%d records, %.2f GB of BGZF) on local disk; step = BGZF members of the rank's "
                                       "chromosomes -> its GPU -> K_inflate -> record hop / filters / pack / QNAME ids -> K_map; chromosomes LPT-assigned by compressed bytes"
                                       % (nrec, os.path.getsize(path) / 1e9),
                           "bam_records": nrec, "records_kept": int(tot_kept), "calls_per_step": int(tot_calls), "bam_records_per_s": nrec * steps / dt,
                           "file_GBps": os.path.getsize(path) * steps / dt / 1e9,
                           "largest_rank_share_of_bytes": max(shares.values()) / max(1.0, float(sum(shares.values())))}}))
    finally:
        if world > 1:
            dist.barrier()
        if rank == 0:
            shutil.rmtree(tmp, ignore_errors=True)


def files_entries(mapper, dev, a):
    """Side entries FROM FILES at the full size of configs[2] (round-4 verdict: the line carried a quarter genome): an unfiltered whole-genome BAM (22 chromosomes,
    ~80M records, 3.8 GB of BGZF; duplicates, improper pairs and low MAPQ present) and its bgzipped VCF are written to /tmp (native writers, not timed), then
      bam_path          file -> resident shards on the GPU (phz_bamdev_*: K_inflate, record hop, filters, k_pack, QNAME ids) and by the host
                        decoder, shards compared array by array;
      end_to_end_files  the drop-in CLI (phaser_amd.phaser.main, the reference's command line, --write_vcf 1) on those files, exactly as a user runs it: wall time
                        and its stages, best of two runs in this warm process.  PCIe, the host's page cache and its CPU quota are all inside this number.
    -> (bam_path, end_to_end_files)"""
    import shutil, tempfile
    from phaser_amd import bamio, synth, workloads, vcfout, _lib, phaser
    torch.cuda.empty_cache()
    tmp = tempfile.mkdtemp(prefix="phz_bench_files_")
    try:
        path, vcfgz, vsets, nrec, t_write = write_genome_files(tmp, a, dev)
        torch.cuda.empty_cache()
        size = os.path.getsize(path)
        ctx = mapper.ctx
        best = None
        for rep in range(3):
            ctx.reset_timing()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            dev_sh = bamio.shards_from_bam_device(ctx, path, {}, 255, True, True, 0.0, device=dev)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if dev_sh is None:
                return {"error": "device path declined the file"}, None
            infl = ctx.timing(_lib.PHZ_T_INFLATE)[0]
            if best is None or dt < best[0]:
                best = (dt, infl)
            if rep < 2:
                del dev_sh
        t0 = time.perf_counter()
        host_sh = bamio.shards_from_bam_native(path, {}, 255, True, True, 0.0, threads=0)
        t_host = time.perf_counter() - t0
        same = list(host_sh) == list(dev_sh) and all(torch.equal(getattr(host_sh[c], f), getattr(dev_sh[c], f).cpu()) for c in host_sh
                                                     for f in ("pos", "cigar_off", "cigar", "seq_off", "seq2", "qual", "qid", "aln_score", "has_as"))
        kept = sum(s.n for s in dev_sh.values())
        del host_sh, dev_sh
        torch.cuda.empty_cache()
        bam_path = {"workload": "whole genome: 22 chromosomes, %d BAM records unfiltered (dups, improper pairs, low MAPQ present), %.0f MB BGZF, "
                                "filters -q 255 -f 2 -F 0x400" % (nrec, size / 1e6),
                    "value": nrec / best[0], "unit": "BAM records/s, file -> resident shards (GPU)", "seconds": best[0],
                    "file_GBps": size / best[0] / 1e9, "records_kept": kept, "copy_plus_inflate_ms": best[1],
                    "host_decoder": {"seconds": t_host, "records_per_s": nrec / t_host, "threads": "library default (<= 32), container CPU quota applies"},
                    "shards_identical_to_host_decoder": bool(same), "inputs_written_in_s": t_write}
        # ---- the CLI on the same files
        from phaser_amd import dist as pdist
        threads = max(1, min(64, 4 * pdist.effective_cpus()))
        runs = []
        out_prefix = os.path.join(tmp, "out")
        # In a FRESH process each time, as a user runs it (the runtime's start-up inside the timed total): in this process the decoder's first hipMalloc of 19 GB
        # right after torch has handed tens of GB back takes 0.25-0.4 s on some boxes (2 ms in a fresh process), which is the benchmark's doing, not the CLI's
        import re, subprocess
        wall = []
        for rep in range(2):
            env = dict(os.environ, PHZ_TIMING="1", PYTHONPATH=os.path.dirname(os.path.abspath(__file__)) + os.pathsep + os.environ.get("PYTHONPATH", ""))
            for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK", "ROLE_RANK", "TORCHELASTIC_RUN_ID"):
                env.pop(k, None)
            t0 = time.perf_counter()
            pr = subprocess.run([sys.executable, "-m", "phaser_amd.phaser", "--vcf", vcfgz, "--bam", path, "--sample", "S1", "--mapq", "255", "--baseq", str(a.baseq), "--paired_end", "1",
                                 "--o", out_prefix, "--threads", str(threads), "--write_vcf", "1"], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                                cwd=os.path.dirname(os.path.abspath(__file__)))
            wall.append(time.perf_counter() - t0)
            st_ = {}
            for line in pr.stderr.split("\n"):
                m_ = re.match(r"^\[phz timing\] (\S.*?)\s+([0-9.]+) s$", line)
                if m_:
                    st_[m_.group(1)] = float(m_.group(2))
            runs.append((st_.get("total", wall[-1]), st_, pr.returncode))
        dt, stages, rc = min(runs, key=lambda r: r[0])
        sizes = {n: os.path.getsize("%s.%s.txt" % (out_prefix, n)) for n in ("allelic_counts", "variant_connections", "haplotypes", "haplotypic_counts", "allele_config")}
        e2e = {"workload": bam_path["workload"] + "; %d het SNPs in a bgzipped VCF; --write_vcf 1 --threads %d" % (sum(len(v) for v in vsets), threads),
               "command": "python -m phaser_amd.phaser --vcf g.vcf.gz --bam g.bam --sample S1 --mapq 255 --baseq %d --paired_end 1 --o out --threads %d --write_vcf 1" % (a.baseq, threads),
               "seconds": dt, "rc": rc, "bam_records_per_s": nrec / dt, "runs_s": [round(r[0], 3) for r in runs],
               "process_wall_s": [round(w, 2) for w in wall], "seconds_is": "the CLI's own clock around main() in a fresh process (runtime start-up, device context, all stages); process_wall_s adds the interpreter and `import torch`",
               "stages_s": {k: round(v_, 3) for k, v_ in stages.items()}, "output_bytes": sizes,
               "phased_vcf_bytes": os.path.getsize(out_prefix + ".vcf.gz") if os.path.exists(out_prefix + ".vcf.gz") else None,
               "note": "files in /tmp (page cache); everything a user's run pays is inside: VCF read, BGZF inflate + BAM decode on the GPU (H2D of the compressed file), "
                       "K_map, phasing pass, D2H of ~1 GB of row text, the five files, the phased VCF (text + bgzip + tabix)"}
        return bam_path, e2e
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def configs1_entry(mapper, a, dev):
    """Secondary, labelled entry: the configs[1] shard of round 1 (chr1 full, 40k het SNPs, 50M records) through the same ABI."""
    from phaser_amd import workloads, _lib, synth, vcf as pvcf
    from phaser_amd import dist as pdist
    from phaser_amd.mapper import Calls
    from phaser_amd.engine import Engine, Config
    torch.cuda.empty_cache()
    v, shard, _ = workloads.make_shard("chr1", workloads.CHR1_LEN, 40_000, 50_000_000, 20240807, dev)
    first = mapper.map_batch([shard], [v.pos], a.baseq)
    call, bufs, N = mapper.prepare_batch([shard], [v.pos], a.baseq, [first[0].n + 16], aux=False)
    for _ in range(3):
        mapper.ctx.check(call())
    mapper.ctx.reset_timing()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 10
    for _ in range(steps):
        mapper.ctx.check(call())
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    _, tot, n = mapper.ctx.timing(_lib.PHZ_T_MAP)
    # gather-aware algorithmic minimum of this shard (see kmap_roofline): from one submission with the text planes (aux0 = the base's read offset)
    call5, bufs5, N5 = mapper.prepare_batch([shard], [v.pos], a.baseq, [first[0].n + 16], aux=True)
    mapper.ctx.check(call5()); torch.cuda.synchronize()
    am = algorithmic_minimum([shard], [v.pos], bufs5, [first[0].n])
    del call5, bufs5
    alg_min = am["stream_bytes"] + 128.0 * (am["qual_lines"] + am["seq_lines"]) + CALL_BYTES * am["calls"]
    k = tot / n / 1e3
    out = {"workload": "configs[1]: chr1 full, 40000 het SNPs, 50000000 records x 76 bp, one shard", "value": first[0].n / dt,
           "unit": "allele calls/s", "ms_per_step": dt * 1e3, "kernel_ms_avg": k * 1e3,
           "roofline_frac": alg_min / k / 1e9 / HBM_PEAK_GBS,
           "roofline_note": "k_map's gather-aware algorithmic minimum (streamed per-record arrays + one 128-byte line per distinct qual / seq2 line under an emitted call + "
                            "9 B per call) / kernel time / 8 TB/s: a LOWER bound of the kernel's HBM fraction (no PMC pass exists for this shard)",
           "algorithmic_bytes_per_launch": alg_min, "algorithmic_bytes_per_record": alg_min / shard.n,
           "streaming_model_GBps_needed": SURVEY_BYTES_PER_RECORD * shard.n / k / 1e9}
    if not a.no_phasing:
        # stages T1-O2 on the same shard (round 1 measured 76 ms here)
        vs = pvcf.load_variants("\n".join(synth.vcf_lines([v])))
        calls = Calls(*[None if t is None else t[:first[0].n] for t in bufs[0]])
        best = None
        for _ in range(max(1, a.phasing_passes)):
            eng = Engine(vs, ["bench"], Config(baseq=a.baseq, host_threads=max(1, min(64, 4 * pdist.effective_cpus())), want_vcf=False), mapper=mapper)
            eng.add_mapped(0, "chr1", shard, calls, int(shard.qid.max()) + 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.close_bam(0)
            files = eng.finish(chunks=True)
            torch.cuda.synchronize()
            dtp = time.perf_counter() - t0
            if best is None or dtp < best[0]:
                best = (dtp, eng.phased, int(sum(len(x) for v_ in files.values() for x in v_)))
            del eng, files
        out["phasing"] = {"ms_per_pass": best[0] * 1e3, "phased_variants": best[1], "value": best[1] / best[0], "unit": "phased variants/s",
                          "output_bytes": best[2]}
    return out


if __name__ == "__main__":
    main()
