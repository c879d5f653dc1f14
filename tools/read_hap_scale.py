#!/usr/bin/env python3
"""GPU-box measurement of Engine.read_haplotypes at BASELINE.json configs[2] shape (autosomes, ~1.5 M het SNPs, ~80 M records, one sample, one GPU): one full pass, then
three calls of phz_read_haplotypes on the resident tally.  Prints the read-list entries, the rows, the median time of the fill call (HIP events on the ctx stream between
two phz_ctx_sync; the count call that precedes it in the protocol does the same device work once more) and the time of the text layer on the first 4 M rows.  QNAMEs are synthetic, ten digits
per id and chromosome, handed over as the interner's pool (blob, offsets).  Measured once, no comparison.
usage: tools/read_hap_scale.py [share=1.0] [--check]      --check: the records against readhap.rows_from_lists on the fetched read lists"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402


TEXT_ROWS = 4_000_000


def digit_pool(n):
    """(blob, offsets) of the names '0000000000' .. of n ids"""
    ids = np.arange(n, dtype=np.int64)
    blob = ((ids[:, None] // 10 ** np.arange(9, -1, -1, dtype=np.int64)[None, :]) % 10 + 48).astype(np.uint8).reshape(-1)
    return blob, np.arange(n + 1, dtype=np.int64) * 10


def main():
    share = float(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 1.0
    from phaser_amd import _lib, readhap, synth, workloads, vcf as pvcf
    from phaser_amd.engine import Config, Engine
    from phaser_amd.mapper import Mapper
    dev = "cuda:0"
    mapper = Mapper(0)
    plan = workloads.genome_plan(int(80_000_000 * share), int(1_500_000 * share))
    vsets = {}; shards = {}
    for chrom, ln, n_snps, n_rec, seed in plan:
        v, shard, _ = workloads.make_shard(chrom, ln, n_snps, n_rec, seed, dev)
        vsets[chrom] = v; shards[chrom] = shard
    chroms = [p[0] for p in plan]
    calls = mapper.map_batch([shards[c] for c in chroms], [vsets[c].pos for c in chroms], 10)
    vs = pvcf.load_variants("\n".join(synth.vcf_lines([vsets[c] for c in chroms])))
    eng = Engine(vs, ["scale"], Config(baseq=10, host_threads=16, want_vcf=True, fetch_text=False), mapper=mapper)
    for i, c in enumerate(chroms):
        n_qid = int(shards[c].qid.max()) + 1
        eng.add_mapped(0, c, shards[c], calls[i], n_qid, qnames=digit_pool(n_qid))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.close_bam(0)
    eng.finish(chunks=True)
    t_pass = time.perf_counter() - t0
    table = readhap.block_table(eng)
    ctx = eng.ctx; lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.phz_ctx_stream(ctx.h))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    args = (len(table["blk_off"]) - 1, vp(table["blk_off"]), vp(table["blk_var"]), vp(table["blk_hap"]), vp(table["var_skip"]), vp(table["bam_skip"]))
    n = C.c_int64(0)
    ctx.check(lib.phz_read_haplotypes(ctx.h, *args, None, 0, C.byref(n), _lib.PHZ_HOST), allow=(_lib.PHZ_E_CAPACITY,))
    rows = np.zeros(int(n.value), dtype=readhap.READHAP_DTYPE)
    ms = []
    for _ in range(3):
        ctx.check(lib.phz_ctx_sync(ctx.h))
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx.check(lib.phz_read_haplotypes(ctx.h, *args, vp(rows), len(rows), C.byref(n), _lib.PHZ_HOST))
        e1.record(stream)
        ctx.check(lib.phz_ctx_sync(ctx.h))
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    print("configs[2] x %.2f: pass %.2f s; %d read-list entries, %d blocks in the table (%d phased), %d rows; phz_read_haplotypes fill call %s ms (median %.2f ms; host "
          "arguments and rows, their copies included)" % (share, t_pass, eng.G["n_read_list"], len(table["blk_off"]) - 1, table["n_phased"], len(rows),
                                                         ", ".join("%.2f" % x for x in ms), sorted(ms)[1]), flush=True)
    if "--check" in sys.argv:
        eng._fetch_tally()
        want = readhap.rows_from_lists(eng.G["rl_start"], eng.G["rl_qid"], 1, table["blk_off"], table["blk_var"], table["blk_hap"], table["var_skip"], table["bam_skip"])
        print("records %s the numpy restatement on the fetched read lists (%d rows, %d with entries on both sides)" % (
            "EQUAL" if want.tobytes() == rows.tobytes() else "DIFFER FROM", len(want), int(((want["a"] > 0) & (want["b"] > 0)).sum())), flush=True)
    part = rows[:TEXT_ROWS]          # (the numpy gathers hold three int64 index arrays per output byte of a column: the first rows only, the figure says how many)
    t1 = time.perf_counter()
    text = readhap.text(eng, part, table=table)
    print("text(): %.2f s for the first %d rows, %d bytes" % (time.perf_counter() - t1, len(part), len(text)), flush=True)


if __name__ == "__main__":
    main()
