#!/usr/bin/env python3
"""GPU-box measurement of --output_haplotag_bam at BASELINE.json configs[2] shape (autosomes, ~1.5 M het SNPs, ~80 M records unfiltered, one sample, one GPU) FROM
FILES: a synthetic coordinate-sorted BAM and a bgzipped VCF are written to /tmp first (native writers, not timed, as tools/run_cli_scale.py does), then the command line
runs on them ONCE with --output_haplotag_bam 1.  Writes the records written, the records tagged, the uncompressed bytes and the times of pick / size / fill / D2H /
deflate to profiles/r25/haplotag_scale.txt.  pick, size and fill are HIP events on the ctx stream between two phz_ctx_sync around the library call (its host waits
included; size and fill summed over the references); D2H (device -> pageable host buffer, one copy per reference) and deflate (phz_bgzf_write of the whole buffer,
the file write included) are wall clock.  Measured once; no comparison is claimed.
usage: tools/haplotag_scale.py [scale=1.0] [threads=16] [--out FILE]"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, REPO)
import torch  # noqa: E402

HG38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309,
        114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468]


def main():
    from phaser_amd import bamio, haplotag, phaser, synth, vcfout
    argv = sys.argv[1:]
    out_file = os.path.join(REPO, "profiles", "r25", "haplotag_scale.txt")
    if "--out" in argv:
        k = argv.index("--out")
        out_file = argv[k + 1]
        del argv[k:k + 2]
    scale = float(argv[0]) if argv else 1.0
    threads = int(argv[1]) if len(argv) > 1 else 16
    total_len = sum(HG38)
    refs = [("chr%d" % (i + 1), ln) for i, ln in enumerate(HG38)]
    vsets = []; batches = []; nrec = 0
    for i, ln in enumerate(HG38):
        chrom = "chr%d" % (i + 1)
        n_snps = int(1_500_000 * scale * ln / total_len); n_pairs = int(40_000_000 * scale * ln / total_len)
        v, gs, ge, w = synth.make_variants(chrom, 1, ln, n_snps, 777 + i, n_genes=max(1, n_snps // 10))
        plan = synth.make_read_plan(v, gs, ge, w, n_pairs, 1777 + i, device="cuda")
        for lo in range(0, len(plan), 2_000_000):
            rb = synth.fill_reads(plan, lo, min(len(plan), lo + 2_000_000), v, qname_prefix="s0.b0.%d." % i)
            batches.append(synth.ReadBatch(rb.chrom, rb.L, rb.pos.cpu(), rb.flag.cpu(), rb.mapq.cpu(), rb.tlen.cpu(), rb.aln_score.cpu(), rb.qid.cpu(),
                                           rb.cigar_off.cpu(), rb.cigar.cpu(), rb.seq.cpu(), rb.qual.cpu(), rb.qname_prefix))
            nrec += len(rb)
        vsets.append(v)
        del plan
    bam = "/tmp/haplotag_scale.bam"; vcfgz = "/tmp/haplotag_scale.vcf.gz"; prefix = "/tmp/haplotag_scale_out"
    bamio.readbatch_to_bam_native(bam, batches, refs, threads)
    del batches
    vcfout.write_bgzf(vcfgz, "\n".join(synth.vcf_lines(vsets)) + "\n", threads, index="vcf")
    print("inputs: %d records in %.2f GB of BAM, %d het SNPs" % (nrec, os.path.getsize(bam) / 1e9, sum(len(v) for v in vsets)), flush=True)
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    # the command line's own run, with the measuring clock handed to its haplotag stage (phaser.main does the same without one)
    run = phaser._Run(phaser.build_parser().parse_args(["--vcf", vcfgz, "--bam", bam, "--sample", "S1", "--mapq", "255", "--baseq", "10", "--paired_end", "1", "--o", prefix,
                                                        "--threads", str(threads), "--write_vcf", "0", "--output_haplotag_bam", "1"]))
    run.haplotag_clock = haplotag.DeviceClock
    try:
        rc = phaser._main(run)
    finally:
        run.join_tasks()
    wall = time.perf_counter() - t0
    st = run.haplotag_results[0]
    stage = phaser.LAST_STAGE_SECONDS.get("haplotagged BAMs", float("nan"))
    ms = st["ms"]
    line = ("configs[2] x %.2f, one run: %d BAM records in, %d het SNPs; --output_haplotag_bam 1 wrote %d records, %d of them tagged HP / PS, %d bytes uncompressed "
            "(%.2f GB BGZF); pick %.2f ms, size %.2f ms, fill %.2f ms (HIP events, the calls' host waits included; size and fill over %d references), D2H %.1f ms, "
            "deflate + file write %.1f ms (wall clock, %d threads); the whole stage %.2f s (device re-open, pack and QNAME ids included) of a %.2f s run (rc %d)\n"
            % (scale, nrec, sum(len(v) for v in vsets), st["records"], st["tagged"], st["bytes"], os.path.getsize(prefix + ".haplotag.1.bam") / 1e9, ms["pick"], ms["size"],
               ms["fill"], len(HG38), ms["d2h"], ms["deflate"], threads, stage, wall, rc))
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, "w") as f:
        f.write(line)
    print(line, flush=True)
    for p in (bam, vcfgz, prefix + ".haplotag.1.bam"):
        os.remove(p)


if __name__ == "__main__":
    main()
