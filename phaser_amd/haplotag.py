"""--output_haplotag_bam 1: the reads phASER used, written out again with the haplotype they vote for.

    <o>.haplotag.<k>.bam       for input BAM k (1-based position in --bam): the input's header unchanged and, in file order, exactly the records that passed this run's
                               filters (--mapq, --paired_end, --remove_dups, --isize) on the chromosomes of this run -- the records the mapper saw.  Each record is byte
                               for byte as in the input, except that a tagged record has HP:C (1 = haplotype A of haplotypes.txt, 2 = the other one) and PS:I (the
                               block's start: column 2 of its haplotypic_counts row) appended, in this order, and its block_size raised by 11.  BGZF with the EOF member.

The rule -- one tag per (BAM, chromosome, template id), both mates of a template get it:
  * only phased blocks vote: the first n_phased entries of readhap.block_table (the one-variant blocks of --unphased_vars behind them never tag); the haplotype-count
    blacklist and --haplo_count_bam_exclude apply as in read_haplotypes, so an excluded BAM is written without tags;
  * among the phz_read_haplotypes records of the template the block with the largest a + b wins, the smallest block index among equal totals;
  * a > b: HP 1, b > a: HP 2, a == b in the WINNING block: no tag (the template does not fall through to its next block);
  * PS = the winning block's start.
The result depends on the inputs alone.  Nothing is tallied, mapped or decoded on the host: the votes are phz_read_haplotypes' records left in HBM, the join is
phz_haplotag_pick (K_tagpick), the input is re-opened through the device BAM path with the run's filters (bamio.open_packed_bam_device), its QNAMEs get their ids from
the run's interners, and phz_bamdev_haplotag (K_tagsize, K_tagwrite) rewrites the kept records from the inflated stream.  The host sees the finished stream once, behind
the header bytes in ONE buffer that holds the whole output BAM uncompressed (that is this option's host memory need), and deflates it (phz_bgzf_write).  pick() and
tag_stream() of tests/haplotag_restatement.py restate both kernels in plain Python.

Not served: several ranks, .sam inputs (phaser.check_args), and a BAM the host decoder read -- its file is skipped with a line that says so.  No .bai index, no tag for
a record the filters dropped, no stripping of HP / PS the input already carries (such a file is refused), no streaming writer."""
from __future__ import annotations

import ctypes as C
import time
from typing import Dict

import numpy as np
import torch

from . import _lib, bamio, readhap
from .network import check_resident


def _dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class Votes:
    """What every BAM of a run shares: the records of ONE phz_read_haplotypes call, left on the device, and the three small tables of the join."""

    def __init__(self, eng):
        check_resident(eng)
        ctx = eng.ctx; dev = torch.device("cuda", ctx.device)
        self.gen = eng.G["gen"]
        self.table = t = readhap.block_table(eng)
        self.n_blocks = len(t["blk_off"]) - 1; self.n_phased = int(t["n_phased"])
        _, qb, _, nq = eng._bases()
        self.chroms = list(t["chroms"])
        self.tmpl_base = np.array([qb[c] for c in self.chroms] + [nq], dtype=np.int64)
        self.n_templates = int(nq)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.d_tmpl_base = up(self.tmpl_base, np.int64)
        self.d_blk_chrom = up(t["chrom"], np.int32)
        self.d_blk_ps = up(t["start"].astype(np.uint32).view(np.int32), np.int32)          # (torch has no uint32 arithmetic: the words travel as int32)
        d_in = [up(t["blk_off"], np.int64), up(t["blk_var"], np.int32), up(t["blk_hap"], np.uint8), up(t["var_skip"], np.uint8), up(t["bam_skip"], np.uint8)]
        torch.cuda.synchronize(dev)
        args = (self.n_blocks,) + tuple(_dp(x) for x in d_in)
        n = C.c_int64(0)
        st = ctx.check(ctx.lib.phz_read_haplotypes(ctx.h, *args, None, 0, C.byref(n), _lib.PHZ_DEVICE), allow=(_lib.PHZ_E_CAPACITY,))
        self.n_rows = int(n.value)
        self.d_rows = torch.empty(max(1, self.n_rows) * readhap.READHAP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        if st == _lib.PHZ_E_CAPACITY:
            ctx.check(ctx.lib.phz_read_haplotypes(ctx.h, *args, _dp(self.d_rows), self.n_rows, C.byref(n), _lib.PHZ_DEVICE))

    def pick(self, ctx, bam: int) -> torch.Tensor:
        """tag words (int32 storage of the uint32 words) of every template of one BAM, on the device"""
        tag = torch.empty(max(1, self.n_templates), dtype=torch.int32, device=self.d_rows.device)
        torch.cuda.synchronize(tag.device)
        ctx.check(ctx.lib.phz_haplotag_pick(ctx.h, _dp(self.d_rows) if self.n_rows else None, self.n_rows, self.n_blocks, self.n_phased, int(bam), _dp(self.d_blk_chrom),
                                            len(self.chroms), _dp(self.d_tmpl_base), self.n_templates, _dp(tag), _lib.PHZ_DEVICE))
        return tag


def votes_of(eng) -> Votes:
    """The Votes of the Engine's finished pass: made once, kept while that pass is the context's resident one."""
    v = getattr(eng, "_haplotag_votes", None)
    if v is None or v.gen != eng.G.get("gen"):
        v = eng._haplotag_votes = Votes(eng)
    return v


class DeviceClock:
    """milliseconds of a call on the ctx stream: HIP events between two phz_ctx_sync.  Measuring only: write() takes one as `clock` (tools/haplotag_scale.py);
    an ordinary run has none, and its calls are neither bracketed nor waited for."""

    def __init__(self, ctx):
        self.ctx = ctx; self.stream = torch.cuda.ExternalStream(ctx.lib.phz_ctx_stream(ctx.h)); self.ms: Dict[str, float] = {}

    def __call__(self, name, fn):
        ctx = self.ctx
        ctx.check(ctx.lib.phz_ctx_sync(ctx.h))
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        out = fn()
        e1.record(self.stream)
        ctx.check(ctx.lib.phz_ctx_sync(ctx.h))
        e1.synchronize()
        self.ms[name] = self.ms.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def write(eng, bam_index: int, bam_path: str, out_path: str, interners, mapq: int, remove_dups: bool, paired_end: bool, isize_cutoff: float = 0.0,
          threads: int = 0, level: int = 6, clock=None) -> dict:
    """One input BAM -> its haplotagged copy at out_path.  -> {"records", "tagged", "bytes" (uncompressed, header included), "ms": {d2h, deflate: wall clock; with a
    `clock` (DeviceClock) also pick, size, fill}}, or {"skipped": why} when the device BAM path does not take the file (nothing is written then)."""
    ctx = eng.ctx; lib = ctx.lib
    votes = votes_of(eng)
    if clock is None:
        clock = lambda _name, fn: fn()
    header = bamio.bam_header_bytes(bam_path)
    packed, why = bamio.open_packed_bam_device(ctx, bam_path, mapq, remove_dups, paired_end, isize_cutoff, chroms=set(eng.chrom_list), device="cuda:%d" % ctx.device)
    if packed is None:
        return {"skipped": "the device BAM path declined it (%s)" % why}
    with packed:
        tag = clock("pick", lambda: votes.pick(ctx, bam_index))
        chrom_index = {c: i for i, c in enumerate(votes.chroms)}
        jobs = []; total = len(header); records = tagged = 0
        nbytes = C.c_int64(0); ntag = C.c_int64(0)
        for ref, name, n, qnames, qname_off in packed.refs:
            ci = chrom_index[name]
            lo = int(votes.tmpl_base[ci]); n_tag = int(votes.tmpl_base[ci + 1]) - lo
            qid = packed.qids(interners, name, qnames, qname_off, n).contiguous()
            if len(interners[name]) > n_tag:
                raise _lib.PhzError(_lib.PHZ_E_ARG, "haplotag: chromosome %s has more QNAMEs than the pass that was tallied" % name)
            args = (packed.h, ref, _dp(qid), C.c_void_p(tag.data_ptr() + 4 * lo), n_tag, _dp(votes.d_blk_ps), votes.n_blocks)
            st = clock("size", lambda: lib.phz_bamdev_haplotag(*args, None, 0, C.byref(nbytes), C.byref(ntag)))
            ctx.check(st, allow=(_lib.PHZ_E_CAPACITY,))
            jobs.append((args, qid, int(nbytes.value), total))
            total += int(nbytes.value); records += n; tagged += int(ntag.value)
        host = np.empty(total, dtype=np.uint8)          # the whole output BAM, uncompressed
        host[:len(header)] = np.frombuffer(header, dtype=np.uint8)
        t_d2h = 0.0
        for args, qid, nb, at in jobs:
            if nb == 0:
                continue
            out = torch.empty(nb, dtype=torch.uint8, device=tag.device)
            torch.cuda.synchronize(out.device)
            ctx.check(clock("fill", lambda: lib.phz_bamdev_haplotag(*args, _dp(out), nb, C.byref(nbytes), C.byref(ntag))))
            t0 = time.perf_counter()
            torch.from_numpy(host[at:at + nb]).copy_(out)
            t_d2h += time.perf_counter() - t0
            del out
    t0 = time.perf_counter()
    st = lib.phz_bgzf_write(out_path.encode(), C.c_void_p(host.ctypes.data), total, int(threads), int(level))          # (writes the EOF member too)
    if st != _lib.PHZ_OK:
        raise _lib.PhzError(st, "phz_bgzf_write(%s) failed" % out_path)
    ms = dict(getattr(clock, "ms", {})); ms["d2h"] = t_d2h * 1e3; ms["deflate"] = (time.perf_counter() - t0) * 1e3
    return {"records": records, "tagged": tagged, "bytes": total, "ms": ms}

