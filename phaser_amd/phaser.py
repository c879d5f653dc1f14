"""phASER command line, MI355X hot path underneath.

Same flags, defaults and output files as phaser/phaser.py:26-178 (`main`), :182-321 (`parse_sample`) and
:378-1263 (`process_vcf`).  What differs is below the CLI: no samtools / bedtools / tabix subprocesses (BAM,
BED and VCF are read in-process) and the seven multiprocessing stages are one `Engine` driving libphz.so.
The phased VCF (`write_vcf`) is written as BGZF `<o>.vcf.gz` with its tabix index `<o>.vcf.gz.tbi`.  `--output_network VARIANT`
writes `<o>.network.links.txt` / `<o>.network.nodes.txt` for the block that holds the variant (phaser_amd/network.py).  `--output_read_haplotypes 1`
(not an option of the reference) writes `<o>.read_haplotypes.txt`: per (block, BAM, read) its call lines on haplotype A's alleles and on the other ones
(phaser_amd/readhap.py).  `--output_haplotag_bam 1` (not an option of the reference either) writes `<o>.haplotag.<k>.bam` for the k-th input BAM: the records that passed the
filters, tagged HP / PS with the haplotype their template votes for (phaser_amd/haplotag.py).  Not supported: `--process_slow`.

    python -m phaser_amd.phaser --vcf S.vcf.gz --bam a.bam,b.bam --sample S1 --mapq 255 --baseq 10 --paired_end 1 --o out

`_main` reads top to bottom as the run: one function per stage, the run's state in one `_Run`.  Work that overlaps a stage (device context, BAM
prefetch, page-locked arena, row-table warm-up, file writer, scipy warm-up) runs as a `_Task` on `_Run.tasks`; `main()` joins them all however it ends.
"""
from __future__ import annotations

import argparse
import datetime
import os
import sys
import threading
import time
from collections import OrderedDict
from typing import Dict, List

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, bamio, samio, vcf
from . import dist as pdist
from .engine import Config, Engine, binom_cdf_dedup

VERSION = "1.2.0"


def out(text=""):
    print(text)
    sys.stdout.flush()


def fatal_error(text):
    out("     FATAL ERROR: " + text)
    sys.exit(1)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--bam", required=False, default='')
    p.add_argument("--vcf", required=True, default='')
    p.add_argument("--sample", required=False, default='')
    p.add_argument("--mapq", required=True)
    p.add_argument("--baseq", type=int, required=True)
    p.add_argument("--paired_end", required=True)
    p.add_argument("--o", required=True)
    p.add_argument("--python_string", default="python3")
    p.add_argument("--haplo_count_bam_exclude", default="")
    p.add_argument("--haplo_count_blacklist", default="")
    p.add_argument("--cc_threshold", type=float, default=0.01)
    p.add_argument("--isize", default="0")
    p.add_argument("--as_q_cutoff", type=float, default=0.05)
    p.add_argument("--blacklist", default="")
    p.add_argument("--write_vcf", type=int, default=1)
    p.add_argument("--include_indels", type=int, default=0)
    p.add_argument("--output_read_ids", type=int, default=0)
    p.add_argument("--remove_dups", type=int, default=1)
    p.add_argument("--pass_only", type=int, default=1)
    p.add_argument("--unphased_vars", type=int, default=1)
    p.add_argument("--chr_prefix", type=str, default="")
    p.add_argument("--gw_phase_method", type=int, default=0)
    p.add_argument("--gw_af_field", default="AF")
    p.add_argument("--gw_phase_vcf", type=int, default=0)
    p.add_argument("--gw_phase_vcf_min_confidence", type=float, default=0.90)
    p.add_argument("--threads", type=int, default=1)
    p.add_argument("--max_block_size", type=int, default=15)
    p.add_argument("--temp_dir", default="")
    p.add_argument("--max_items_per_thread", type=int, default=100000)
    p.add_argument("--show_warning", type=int, default=0)
    p.add_argument("--debug", type=int, default=0)
    p.add_argument("--chr", default="")
    p.add_argument("--unique_ids", type=int, default=0)
    p.add_argument("--py_hash_order", type=int, default=0,
                   help="1: rows and read labels of variant_connections / haplotypes / haplotypic_counts in the order CPython 3.10 gives the reference's sets "
                        "run under PYTHONHASHSEED=0, i.e. files byte-identical to the reference's (the str hash and the set of that interpreter are restated "
                        "in libphz: works under any Python, costs seconds at whole-genome scale; PHZ_PYORDER_PYTHON=1 selects the pure-Python twin)")
    p.add_argument("--id_separator", default="_")
    p.add_argument("--output_network", default="")
    p.add_argument("--output_read_haplotypes", type=int, default=0,
                   help="1: also write <o>.read_haplotypes.txt -- per (block, BAM, read) the number of its call lines on haplotype A's alleles and on the other "
                        "ones, and the haplotype they vote for (not an option of the reference; one rank only)")
    p.add_argument("--output_haplotag_bam", type=int, default=0,
                   help="1: also write <o>.haplotag.<k>.bam for the k-th input BAM -- the records that passed --mapq / --paired_end / --remove_dups / --isize on the "
                        "chromosomes of the run, each tagged HP:C (1 = haplotype A, 2 = the other one) and PS:I (the block's start) when its template votes for a "
                        "haplotype of a phased block (not an option of the reference; one rank only, BAM inputs only; the whole output BAM is held uncompressed in "
                        "host memory)")
    p.add_argument("--process_slow", type=int, default=0, required=False)
    return p


def load_bed(path: str) -> List[tuple]:
    """BED file -> [(chrom, start, end)] (0-based, half-open); header / track lines skipped."""
    iv = []
    with open(path) as f:
        for line in f:
            c = line.rstrip("\n").split("\t")
            if len(c) >= 3 and not line.startswith(("#", "track", "browser")):
                iv.append((c[0], int(c[1]), int(c[2])))
    return iv


# ---- pure helpers: no device, no run state

def check_args(args, world):
    """The fatal checks on the arguments, in the reference's order.  The two `world > 1` refusals hit every rank alike (all see the same arguments) and
    come before the first collective: nobody is left waiting in a barrier."""
    if args.id_separator == ":" or args.id_separator == "":
        fatal_error("ID separator must not be ':' or blank. Please choose another separator that is not found in the contig names.")
    if args.process_slow != 0:
        fatal_error("--process_slow is not supported by this build (the GPU path holds all chromosomes; SURVEY.md section 2).")
    if args.py_hash_order and world > 1:
        fatal_error("--py_hash_order 1 needs all chromosomes on one rank (run it without torch.distributed).")
    if args.output_read_haplotypes and world > 1:
        fatal_error("--output_read_haplotypes 1 needs all chromosomes on one rank (run it without torch.distributed).")
    if args.output_haplotag_bam and world > 1:
        fatal_error("--output_haplotag_bam 1 needs all chromosomes on one rank (run it without torch.distributed).")
    if args.output_haplotag_bam and any(b.endswith(".sam") for b in args.bam.split(",")):
        fatal_error("--output_haplotag_bam 1 needs BAM inputs (a .sam input has no records to copy).")
    if not os.path.isfile(args.vcf):
        fatal_error("VCF file does not exist.")
    for xfile in [args.blacklist, args.haplo_count_blacklist] + args.bam.split(","):
        if xfile != "" and not os.path.isfile(xfile):
            fatal_error("File: %s not found." % xfile)


def find_sample_column(data, sample):
    """Column of `sample` in the `#CHROM` line of VCF text (bytes, or a uint8 array over the reader's buffer); fatal when it is not there.
    The header sits at the top: only the first 20,000 lines are looked at, and only they are split (split(b"\\n", 20000) on the whole text copied
    the 75 MB behind them once more, 0.05 s); of an array the first 8 MB are looked at (a header beyond that: sample not found)."""
    text = data if isinstance(data, (bytes, bytearray)) else bytes(memoryview(data)[:8 << 20])
    head_end = 0
    for _ in range(20000):
        nxt = text.find(b"\n", head_end)
        if nxt < 0:
            head_end = len(text); break
        head_end = nxt + 1
        if text[head_end:head_end + 1] not in (b"#", b"\n", b"\r", b""):          # the first record: one more line is taken (it ends the loop below)
            nxt = text.find(b"\n", head_end)
            head_end = len(text) if nxt < 0 else nxt + 1
            break
    for raw in text[:head_end].split(b"\n"):
        if b"#CHR" in raw:
            cols = raw.decode().rstrip().split("\t")
            m = {cols[i]: i for i in range(9, len(cols))}
            if sample in m:
                return m[sample]
            break
        if raw and raw[0:1] != b"#":
            break
    fatal_error("Sample '%s' not found in the input VCF file." % sample)


def per_bam(value, n_bams, what):
    """A comma-separated per-BAM option -> one string per BAM: a single value serves all BAMs (phaser.py:469-513)."""
    lst = value.split(",")
    if len(lst) == 1 and n_bams > 1:
        lst = lst * n_bams
    elif len(lst) != n_bams:
        fatal_error("Number of %s values and input BAMs does not match. Supply either one %s to be used for all BAMs or one %s per input BAM." % (what, what, what))
    return lst


def bam_display_names(bam_list):
    """The names the output files give the BAMs (phaser.py:469-513): the basename without every ".bam"; a name that occurs more than once
    gets .1, .2, ... in order of appearance."""
    base = [os.path.basename(x).replace(".bam", "") for x in bam_list]
    counter = OrderedDict(); names = []
    for x in base:
        if base.count(x) > 1:
            counter[x] = counter.get(x, 0) + 1
            names.append(x + "." + str(counter[x]))
        else:
            names.append(x)
    return names


def prefetch_verdict(error, guess, mine, prefetch_key, key, have_shards):
    """What becomes of a finished BAM prefetch -> (outcome, the text of its timing line).  It was made for the chromosomes `guess` and the
    filters `prefetch_key`; the parsed table has the chromosomes `mine` and the BAM's real filters are `key`.  outcome: "used", "declined"
    (the device path declined the file: straight to the host decoder) or "discarded" (the BAM is read as if there had been no prefetch)."""
    if error:
        return "discarded", "discarded (error in the prefetch)"
    if not mine <= guess:
        return "discarded", "discarded (chromosomes %s not in the guess)" % sorted(mine - guess)
    if prefetch_key != key:
        return "discarded", "discarded (filters differ)"
    if not have_shards:
        return "declined", "device path declined the file"
    return "used", "used"


# ---- timing (PHZ_TIMING=1: on stderr, not part of the reference's output)

LAST_STAGE_SECONDS = {}          # stage name -> seconds of the last main() of this process (rank 0): read by bench.py's end_to_end_files entry


def timing_line(text):
    if os.environ.get("PHZ_TIMING"):
        sys.stderr.write("[phz timing] %s\n" % text)


class StageClock:
    """The stages of a run: mark(name) ends the stage `name` now.  The names are an interface: bench.py reads them from report()'s lines."""

    def __init__(self):
        self.wall_start = time.time()
        self.marks = [("start", time.perf_counter())]

    def mark(self, name):
        self.marks.append((name, time.perf_counter()))

    def since_start(self):
        return time.perf_counter() - self.marks[0][1]

    def report(self):
        global LAST_STAGE_SECONDS
        stages = [(name, t - t_prev) for (_, t_prev), (name, t) in zip(self.marks[:-1], self.marks[1:])]
        stages.append(("total", self.marks[-1][1] - self.marks[0][1]))
        LAST_STAGE_SECONDS = dict(stages)
        for name, seconds in stages:
            timing_line("%-55s %8.3f s" % (name, seconds))


# ---- the run: its state and its helper threads

class _Task:
    """A helper thread, started at once: what `target()` returned, the exception it raised, its wall seconds.  join() only waits;
    result() waits, then re-raises the exception or returns the value."""

    def __init__(self, name, target, daemon=True):
        self.value = self.error = self.seconds = None

        def work():
            t0 = time.perf_counter()
            try:
                self.value = target()
            except BaseException as e:
                self.error = e
            self.seconds = time.perf_counter() - t0

        self.thread = threading.Thread(target=work, name=name, daemon=daemon)
        self.thread.start()

    def join(self):
        self.thread.join()

    def result(self):
        self.join()
        if self.error is not None:
            raise self.error
        return self.value


class _Run:
    """What one main() carries from stage to stage.  Every helper thread is a _Task on `tasks`: main() joins them all when it ends."""

    def __init__(self, args):
        self.args = args
        self.rank, self.world, self.local, self.n_dev = 0, 1, 0, 0          # set by init_ranks
        self.say = out
        self.clock = None
        self.tasks: List[_Task] = []
        self.ctx_task = self.arena_task = self.warm_task = None
        self.prefetch = None
        self.bam_list = args.bam.split(",")
        self.any_sam = any(b.endswith(".sam") for b in self.bam_list)       # text inputs keep everything on the Python reader
        self.threads = max(1, args.threads)
        self.pool_threads = max(0, args.threads if args.threads > 1 else 0)          # 0: the library's default
        self.vs = self.eng = self.mine = None          # set by load_variant_table / make_engine
        self.interners: Dict[str, object] = {}
        self.haplotag_clock = None     # a measuring caller (tools/haplotag_scale.py) sets haplotag.DeviceClock: ctx -> the clock of one file's device calls
        self.haplotag_results = []     # what Engine.haplotag returned for every BAM that got that far (write_haplotag_bams)
        self.bam_paths = []            # which decoder read each BAM: "device" (phz_bamdev_*), "host" (phz_bam_*: the file was declined or PHZ_BAM_HOST=1), "sam" (text)

    @property
    def device(self):
        return "cuda:%d" % self.local

    def task(self, name, target, daemon=True):
        self.tasks.append(_Task(name, target, daemon))
        return self.tasks[-1]

    def join_tasks(self):
        for t in self.tasks:
            t.join()


class BamPrefetch:
    """The first BAM is inflated / decoded / filtered on the GPU (PCIe- and GPU-bound) WHILE the host reads and parses the VCF: the stages share
    nothing but the names of the chromosomes to keep.  Those come from the VCF's tabix index when there is one (its sequence names: a few KB,
    before the VCF itself is touched), else they are guessed from the text once it is gunzipped (vcf.contig_names_guess); either way take()
    checks them against the parsed table -- names that do not cover the table discard the prefetch and the BAM is read as before."""

    def __init__(self, run, guess, key):
        self.guess, self.key = set(guess), key

        def work():
            t0 = time.perf_counter()
            mapper = run.ctx_task.result()          # the prefetch takes the early context over; no context, no prefetch
            timing_line("  device context %.3f s on its own thread; the BAM prefetch waited %.3f s for it and starts %.3f s into the run" % (
                run.ctx_task.seconds, time.perf_counter() - t0, run.clock.since_start()))
            its = {}
            mq, isz, pe = key
            return bamio.shards_from_bam_device(mapper.ctx, run.bam_list[0], its, mq, run.args.remove_dups == 1, pe == 1, isz, chroms=guess, device=run.device), its

        self.task = run.task("phz-bam-prefetch", work)          # an error in it is reported by take(): the ordinary path runs instead

    @staticmethod
    def start(run, guess):
        """Prefetch the first BAM for the chromosomes `guess` with the first value of each per-BAM filter.  A value that does not parse
        means no prefetch (the ordinary path trips over it when it comes to that BAM)."""
        args = run.args
        try:
            key = (int(args.mapq.split(",")[0]), float(args.isize.split(",")[0]), int(args.paired_end.split(",")[0]))
        except ValueError:
            return
        run.prefetch = BamPrefetch(run, guess, key)

    def take(self, mine, key):
        """-> (shards | None, interners, declined, verdict) for the parsed table's chromosomes `mine` and the BAM's real (mapq, isize, paired_end)."""
        self.task.join()
        shards, interners = self.task.value or (None, {})
        self.task.value = None          # the shards are the caller's now, or nobody's
        outcome, verdict = prefetch_verdict(self.task.error is not None, self.guess, mine, self.key, key, shards is not None)
        if outcome != "used":
            return None, {}, outcome == "declined", verdict
        return {c: s for c, s in shards.items() if c in mine}, {c: it for c, it in interners.items() if c in mine}, False, verdict


# ---- the stages, in the order _main runs them

def init_ranks(run):
    """torch's thread cap, the current device, and the process group when there is more than one rank."""
    run.rank, run.world = pdist.world()
    # torch's intra-op pool sized by the container's CPU quota, not by the host's core count (see dist.effective_cpus)
    torch.set_num_threads(max(1, min(torch.get_num_threads(), pdist.effective_cpus() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1"))))))
    run.n_dev = n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    run.local = local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, n_dev)
    if n_dev:
        torch.cuda.set_device(local)          # before any collective: NCCL / barrier use the current device
    force_pg = os.environ.get("PHZ_DIST_FORCE_COLLECTIVES") == "1"        # one rank, yet every collective of the multi-rank path runs (dist.collectives_live)
    if run.world == 1 and (int(os.environ.get("WORLD_SIZE", "1")) > 1 or (force_pg and not dist.is_initialized())):
        # one rank per GPU over RCCL ("nccl"); PHZ_DIST_BACKEND=gloo lets several ranks share a GPU (tests on a 1-GPU box)
        backend = os.environ.get("PHZ_DIST_BACKEND", "nccl" if n_dev else "gloo")
        if force_pg and "WORLD_SIZE" not in os.environ:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
            os.environ["RANK"] = "0"; os.environ["WORLD_SIZE"] = "1"
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
        run.rank, run.world = pdist.world()
    run.say = out if run.rank == 0 else (lambda *_: None)


def banner(say):
    say("")
    say("##################################################")
    say("              Welcome to phASER v%s" % VERSION)
    say("  Author: Stephane Castel (stephanecastel@gmail.com)")
    say("  Updated by: Bishwa K. Giri (bkgiri@uncg.edu)")
    say("  MI355X hot path: phaser_amd (K_map / K_tally on gfx950)")
    say("##################################################")
    say("")


def start_background(run):
    """The work that needs nothing from the VCF, started before it is read."""
    args = run.args
    # scipy's binomial machinery initialises lazily on the first call (~80 ms): pay for it on a side thread while the BAM is being
    # inflated and decoded on the GPU instead of in the middle of the pair tests.  Nobody asks for its result.
    run.task("phz-scipy-warmup", lambda: binom_cdf_dedup(np.array([1]), np.array([3]), 0.99))
    # The device context (HIP runtime start-up, the library's code objects, the K_map stream: 0.1-0.2 s in a fresh process) is created
    # from the first moment on -- the VCF is being read and gunzipped meanwhile.  The BAM prefetch takes it over; without a prefetch it
    # serves the ordinary path (make_engine).
    if (run.world == 1 and args.chr == "" and run.n_dev and os.environ.get("PHZ_BAM_HOST") != "1" and os.environ.get("PHZ_BAM_PREFETCH", "1") == "1"
            and not run.any_sam):
        def context():
            from .mapper import Mapper
            return Mapper(run.local)

        run.ctx_task = run.task("phz-ctx", context)
    # the host region that will receive the row text is page-locked while the VCF is read (~0.1 s per GB, independent of everything
    # else); sized from the BAMs, grown later if it turns out too small.  Best effort: finish() only join()s it, and page-locks the
    # region itself when this failed.
    if not run.any_sam and os.environ.get("PHZ_EARLY_ARENA", "1") == "1":
        def arena():
            if torch.cuda.is_available():
                from . import rowsdev
                total = sum(os.path.getsize(b) for b in run.bam_list if os.path.exists(b))
                rowsdev.prepare_arena(int(min(4 << 30, max(64 << 20, total // 4))))

        run.arena_task = run.task("phz-arena", arena)


def load_variant_table(run):
    """VCF file -> (the het-variant table, the VCF text, the sample's column); the BAM prefetch starts as soon as chromosome names are known."""
    args, say = run.args, run.say
    prefetch_ok = run.ctx_task is not None
    if prefetch_ok:
        names = vcf.contig_names_from_tbi(args.vcf + ".tbi")
        if names:
            BamPrefetch.start(run, [args.chr_prefix + c for c in names])
    t0 = time.perf_counter()
    data = vcf.read_bytes(args.vcf, as_array=True)          # bgzipped: a uint8 array over the native reader's buffer (no 75 MB Python bytes object)
    t1 = time.perf_counter()
    if prefetch_ok and run.prefetch is None:
        guess = [args.chr_prefix + c for c in vcf.contig_names_guess(data)]
        if guess:
            BamPrefetch.start(run, guess)
    sample_col = find_sample_column(data, args.sample)
    if args.blacklist != "":
        say("    removing blacklisted variants and processing VCF...")
    if args.haplo_count_blacklist != "":
        say("#1b. Loading haplotypic count blacklist intervals...")
    t2 = time.perf_counter()
    # cut -f 1-9,S | grep -v '0|0\|1|1' [| bedtools intersect -v -b blacklist]   (phaser.py:220-225) and the bedtools intersect of
    # --haplo_count_blacklist (:232-241) all run inside the native loader (interval lookups by binary search)
    vs = vcf.load_variants(data, sample_column=sample_col, grep_hom=True, drop_bed=load_bed(args.blacklist) if args.blacklist != "" else None,
                           # with --chr_prefix the reference's blacklist keys (VCF names) never match its lookups (prefixed names, :1070)
                           mark_bed=load_bed(args.haplo_count_blacklist) if (args.haplo_count_blacklist != "" and args.chr_prefix == "") else None,
                           chrom_of_interest=args.chr, pass_only=args.pass_only, include_indels=args.include_indels, chr_prefix=args.chr_prefix,
                           id_separator=args.id_separator, gw_phase_method=args.gw_phase_method, gw_af_field=args.gw_af_field,
                           contig_ban=(args.id_separator, ":"), threads=run.threads)
    timing_line("  vcf: read + inflate %.3f s, contig guess + header %.3f s, parse + tables %.3f s (%d bytes of text)" % (
        t1 - t0, t2 - t1, time.perf_counter() - t2, len(data)))
    run.clock.mark("vcf read + het-variant table")
    say("     creating variant mapping table...")
    say("          %d heterozygous sites being used for phasing (%d filtered, %d indels excluded, %d unphased)" %
        (vs.het_count, vs.filter_count, vs.indels_excluded, vs.unphased_count))
    say()
    if vs.het_count == 0:
        fatal_error("No heterozygous sites that passed all filters were included in the analysis, phASER cannot continue. "
                    "Check blacklist and pass_only arguments.")
    run.vs = vs
    return data, sample_col


def make_engine(run):
    """The per-BAM lists and the Engine on the early device context -> [(bam, mapq, isize, paired_end)]; starts the row-table warm-up."""
    args, vs, n = run.args, run.vs, len(run.bam_list)
    mapq_list = per_bam(args.mapq, n, "mapq")
    isize_list = list(map(float, per_bam(args.isize, n, "isize")))
    pe_list = per_bam(args.paired_end, n, "paired_end")
    excl = [x - 1 for x in map(int, args.haplo_count_bam_exclude.split(","))] if args.haplo_count_bam_exclude != "" else []
    cfg = Config(baseq=args.baseq, as_q_cutoff=args.as_q_cutoff, cc_threshold=args.cc_threshold, max_block_size=args.max_block_size,
                 id_separator=args.id_separator, unphased_vars=args.unphased_vars, gw_phase_method=args.gw_phase_method,
                 output_read_ids=args.output_read_ids, unique_ids=args.unique_ids, haplo_count_bam_exclude=excl, py_hash_order=args.py_hash_order,
                 include_indels=args.include_indels, host_threads=run.threads)
    if args.output_network != "" or args.output_read_haplotypes == 1 or args.output_haplotag_bam == 1:
        cfg.want_vcf = True            # the per-block arrays (the switch write_vcf and --py_hash_order set): the block of the variant is looked up in them
    mapper0 = None
    if run.ctx_task is not None:
        run.ctx_task.join()            # (a prefetch goes on decoding on this context's stream meanwhile)
        mapper0 = run.ctx_task.value           # None when it failed: the Engine makes its own, and reports what is wrong
    run.eng = eng = Engine(vs, bam_display_names(run.bam_list), cfg, device=run.local, mapper=mapper0)
    eng.spool_dir = os.path.dirname(os.path.abspath(args.o))       # ranks hand their row text to rank 0 through files next to the outputs
    # multi-GPU: chromosomes are sharded across ranks by record count (LPT).  Before anything is decoded the count is not known; its
    # proxy is the compressed bytes each chromosome occupies in the BAMs (a few dozen BGZF member inflations per file); text inputs
    # fall back to the variant count
    if run.world > 1:
        weights = {c: 0.0 for c in vs.chroms}
        if not run.any_sam:
            for bam in run.bam_list:
                for name, nbytes in bamio.bam_ref_weights(bam, threads=run.pool_threads).items():
                    if name in weights:              # VCF names already carry --chr_prefix (they are the BAM's names)
                        weights[name] += float(nbytes)
        if sum(weights.values()) <= 0:
            weights = {c: float(len(v)) for c, v in vs.chroms.items()}
        owner = pdist.assign_chromosomes(weights, run.world)
        eng.set_owned([c for c in vs.chroms if owner[c] == run.rank])
    run.mine = set(eng.chrom_list)
    # While the BAMs are read: the per-variant tables of the row stage go to the GPU (0.07 s at genome scale, independent of the reads).
    # Best effort: finish() only join()s it, and uploads the tables itself when they are not there.
    if not run.any_sam and cfg.device_rows:
        def warm():
            if torch.cuda.is_available():
                from . import rowsdev
                from ._lib import Context
                # its OWN phz_ctx (stream, scratch, error string): the BAM prefetch thread may still be inside phz_bamdev_* on the
                # Engine's ctx, and a phz_ctx serves one thread at a time (include/phz.h)
                rowsdev.tables_for(eng, ctx=Context(run.local))

        run.warm_task = run.task("phz-warm-tables", warm)
    return list(zip(run.bam_list, mapq_list, isize_list, pe_list))


def read_bam(run, bi, bam, mq, isz, pe):
    """One input file -> its shards, one per chromosome of `run.mine`, QNAMEs interned into run.interners."""
    args, say, interners, mine = run.args, run.say, run.interners, run.mine
    say("     file: %s" % bam)
    say("          minimum mapq: %s" % mq)
    say("          mapping reads to variants...")
    if bam.endswith(".sam"):
        run.bam_paths.append("sam")
        return samio.shards_from_sam(open(bam).read(), interners, isz)
    if run.any_sam:
        run.bam_paths.append("host")
        return bamio.shards_from_bam(bam, interners, int(mq), args.remove_dups == 1, int(pe) == 1, isz, chroms=mine)
    # BGZF inflate + record decode + filters + packing on the GPU (phz_bamdev_*); files it declines, and PHZ_BAM_HOST=1, go
    # through the host decoder (phz_bam_*, --threads host threads).  QNAME interning is host-side in both.
    shards, declined = None, False
    if bi == 0 and run.prefetch is not None:
        shards, its, declined, verdict = run.prefetch.take(mine, (int(mq), isz, int(pe)))
        interners.update(its)
        timing_line("  bam prefetch during the VCF parse: %s" % verdict)
    if shards is None and not declined and os.environ.get("PHZ_BAM_HOST") != "1":
        shards = bamio.shards_from_bam_device(run.eng.ctx, bam, interners, int(mq), args.remove_dups == 1, int(pe) == 1, isz, chroms=mine, device=run.device)
    run.bam_paths.append("device" if shards is not None else "host")
    if shards is None:
        shards = bamio.shards_from_bam_native(bam, interners, int(mq), args.remove_dups == 1, int(pe) == 1, isz, chroms=mine, threads=run.pool_threads)
    return shards


def map_bam(run, bi, shards):
    """The BAM's shards to the GPU and through K_map (all its chromosomes in one submission), then its alignment-score cutoff."""
    args, say, eng, interners = run.args, run.say, run.eng, run.interners
    items = []
    for chrom in run.vs.chroms:
        if chrom in shards and chrom in run.mine:
            names = None
            if args.output_read_ids == 1 or (args.py_hash_order == 1 and os.environ.get("PHZ_PYORDER_PYTHON") == "1"):
                names = interners[chrom].names          # a list of str: the host row twin and the pure-Python raw-byte twin index it
            elif args.py_hash_order == 1 or args.output_read_haplotypes == 1:
                names = interners[chrom].pool() if hasattr(interners[chrom], "pool") else interners[chrom].names      # (blob, offsets): what the native raw-byte tier reads
            items.append((chrom, shards[chrom].to(run.device), len(interners[chrom]), names))
    eng.add_shards(bi, items)
    for it in items:
        say("               completed chromosome %s..." % it[0])
    for chrom in interners:
        if chrom in eng.n_qid:
            eng.n_qid[chrom] = len(interners[chrom])
    run.clock.mark("H2D + K_map")
    say("          processing mapped reads...")
    n_before = len(eng.log)
    eng.close_bam(bi)
    eng.resolve_cutoffs()          # (the CLI prints the BAM's cutoff line here; a caller that streams passes leaves it to finish())
    run.clock.mark("AS cutoff")
    for line in eng.log[n_before:]:
        say(line)


def finish(run):
    """Tally, pair tests, components, block phasing and the row text of the five files -> {file name: chunks}, or None on the ranks that write nothing."""
    for t in (run.warm_task, run.arena_task):          # best effort both: what is not there, finish() does itself
        if t is not None:
            t.join()
    files = run.eng.finish(chunks=True)
    run.clock.mark("tally + pair tests + components + block phasing + rows")
    timing_line("  finish: %s" % ", ".join("%s %.3f" % (k, v) for k, v in run.eng.stats.items()))
    return files


def write_network(run):
    """--output_network (phaser.py:1127-1157): the rank that owns the variant's chromosome has its block and the pair cells of its tally still
    in HBM: it writes the two files (all ranks share the node's file system, as for the spool files)."""
    args = run.args
    net = run.eng.network(args.output_network)
    if net is not None:
        pdist.write_files([(args.o + ".network.links.txt", [net["links"]]), (args.o + ".network.nodes.txt", [net["nodes"]])], threads=2)
    found, _ = pdist.allreduce_counts(1 if net is not None else 0, 0)
    if found == 0:
        run.say("     variant %s is in no phased block: no network files written" % args.output_network)
    run.clock.mark("network of " + args.output_network)


def write_read_haplotypes(run):
    """--output_read_haplotypes: every block's reads at once, from the read lists the tally left in HBM (phaser_amd/readhap.py)."""
    rh = run.eng.read_haplotypes()
    pdist.write_files([(run.args.o + ".read_haplotypes.txt", [rh["text"]])], threads=1)
    run.say("     %d (block, bam, read) rows written to %s.read_haplotypes.txt" % (len(rh["records"]), run.args.o))
    run.clock.mark("read haplotypes")


def write_haplotag_bams(run, bams):
    """--output_haplotag_bam: every input BAM again through the device BAM path with its own filters, its kept records rewritten with HP / PS on the GPU
    (phaser_amd/haplotag.py).  A BAM that the host decoder read is skipped with a line that says so."""
    args, say = run.args, run.say
    for bi, (bam, mq, isz, pe) in enumerate(bams):
        path = "%s.haplotag.%d.bam" % (args.o, bi + 1)
        if run.bam_paths[bi] != "device":
            say("     no haplotagged BAM for %s: the %s decoder read it, and the records are rewritten from the device BAM path's stream" % (bam, run.bam_paths[bi]))
            continue
        try:
            res = run.eng.haplotag(bi, bam, path, run.interners, int(mq), args.remove_dups == 1, int(pe) == 1, isz, threads=run.pool_threads,
                                   clock=run.haplotag_clock(run.eng.ctx) if run.haplotag_clock else None)
        except _lib.PhzError as e:          # a file the record rewrite refuses (it already carries HP / PS): the other outputs are still written
            if e.status != _lib.PHZ_E_UNSUPPORTED:
                raise
            res = {"skipped": str(e)}
        if "skipped" in res:
            say("     no haplotagged BAM for %s: %s" % (bam, res["skipped"]))
        else:
            say("     %d records written to %s, %d of them tagged HP / PS" % (res["records"], path, res["tagged"]))
        run.haplotag_results.append(res)
    run.clock.mark("haplotagged BAMs")


def write_outputs(run, files, data, sample_col):
    """The five files and, with --write_vcf 1, the phased VCF -> (genome-wide phased, phase corrected) counts of the VCF."""
    args, say = run.args, run.say
    say("#4. Identifying haplotype blocks...")
    say("#5. Phasing blocks...")
    say("#6. Outputting haplotypes...")
    five = [(args.o + "." + name + ".txt", body) for name, body in files.items()]

    def write_five():
        pdist.write_files(five, threads=max(1, min(16, args.threads)))

    if args.write_vcf != 1:
        write_five()
        run.clock.mark("write the five files")
        return 0, 0
    writer = run.task("phz-write-files", write_five, daemon=False)          # beside the phased VCF text; its error is raised below
    from . import vcfout
    say("#7. Outputting phased VCF...")
    if args.gw_phase_vcf == 1:
        say("     GT field is being updated with phASER genome wide phase when applicable. This can be changed using the --gw_phase_vcf argument.")
    elif args.gw_phase_vcf == 2:
        say("     GT field is being updated with either phASER genome wide phase or phASER block phase with PS specified, depending on phase anchoring quality.")
    else:
        say("     GT field is not being updated with phASER genome wide phase. This can be changed using the --gw_phase_vcf argument.")
    vtxt, up, pc = vcfout.phased_vcf_text(data, sample_col, run.eng, args.id_separator, args.chr, args.gw_phase_vcf,
                                          args.gw_phase_vcf_min_confidence, threads=run.threads, as_bytes=True)
    writer.result()
    run.clock.mark("phased VCF text (+ the five files on a helper thread)")
    say("     Compressing and tabix indexing output VCF...")
    if not vcfout.write_bgzf(args.o + ".vcf.gz", vtxt, run.pool_threads, index="vcf"):
        say("     WARNING: the VCF is not position-sorted, no tabix index written")
    run.clock.mark("phased VCF bgzf + tabix")
    return up, pc


def print_summary(run, up, pc):
    args, say, eng, vs = run.args, run.say, run.eng, run.vs
    say('')
    say("     COMPLETED using %d reads in %d seconds using %d GPU(s)" % (eng.total_lines, time.time() - run.clock.wall_start, run.world))
    say("     PHASED  %d of %d all variants (= %f) with at least one other variant" %
        (eng.phased, vs.het_count, float(eng.phased) / float(vs.het_count)))
    if args.write_vcf == 1:
        if vs.unphased_count > 0:
            say("     GENOME WIDE PHASED  %d of %d unphased variants (= %f)" % (up, vs.unphased_count, float(up) / float(vs.unphased_count)))
        say("     GENOME WIDE PHASE CORRECTED  %d of %d variants (= %f)" % (pc, vs.het_count, float(pc) / float(vs.het_count)))
    # which of this build's paths did the work (not a line of the reference): a run that fell back to a host twin says so
    say("     HOT PATH  bam: %s, rows: %s%s" % (",".join(run.bam_paths) if run.bam_paths else "-", getattr(eng, "rows_path", "-"),
                                                " (%s)" % eng.rows_fallback if getattr(eng, "rows_fallback", None) else ""))
    say('')
    say("The End.")


def main(argv=None):
    """The CLI.  Whatever way it ends (result, fatal_error, exception), every helper thread of the run (`_Run.tasks`: device context, BAM
    prefetch, arena, row-table warm-up, file writer, scipy warm-up) is waited for: the interpreter must not start tearing down with GPU
    work of ours in flight."""
    run = _Run(build_parser().parse_args(argv))
    try:
        return _main(run)
    finally:
        run.join_tasks()


def _main(run):
    args = run.args
    init_ranks(run)
    say = run.say                  # rank 0 speaks, the others stay silent
    banner(say)
    check_args(args, run.world)
    run.clock = StageClock()
    start_background(run)          # scipy warm-up, device context, arena
    say('STARTED "Read backed phasing and ASE/haplotype analyses" ... ')
    say("    DATE, TIME : %s" % (datetime.datetime.now().strftime('%Y-%m-%d, %H:%M:%S')))
    say("#1. Loading heterozygous variants into intervals...")
    data, sample_col = load_variant_table(run)          # starts the BAM prefetch
    say("#2. Retrieving reads that overlap heterozygous sites...")
    bams = make_engine(run)        # waits for the device context, starts the row-table warm-up
    for bi, (bam, mq, isz, pe) in enumerate(bams):
        shards = read_bam(run, bi, bam, mq, isz, pe)
        run.clock.mark("bam decode + filters + qname interning")
        map_bam(run, bi, shards)
    say("#3. Identifying connected variants...")
    say("     calculating sequencing noise level...")
    n_before = len(run.eng.log)
    files = finish(run)            # joins warm-up and arena first
    if args.output_network != "":
        write_network(run)
    if args.output_read_haplotypes == 1:
        write_read_haplotypes(run)
    if args.output_haplotag_bam == 1:
        write_haplotag_bams(run, bams)
    if files is not None:
        for line in run.eng.log[n_before:]:
            say(line)
        up, pc = write_outputs(run, files, data, sample_col)          # the five files on a helper thread beside the phased VCF text
        print_summary(run, up, pc)
        run.clock.report()
    pdist.cleanup_spool()          # (barrier) every rank removes its spool file once rank 0 has written the outputs
    return 0


if __name__ == "__main__":
    sys.exit(main())
