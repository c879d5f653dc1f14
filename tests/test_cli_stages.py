"""The parts of the drop-in CLI (phaser_amd/phaser.py) that need no device: the header scan, the per-BAM lists, the display names of the BAMs, the
argument checks, what becomes of a BAM prefetch, the owner of the helper threads and the stage clock.  The CLI end to end: tests/test_gpu_pipeline.py."""
import re
import threading

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository on sys.path)
from phaser_amd import phaser

HEADER = b"##fileformat=VCFv4.2\n##contig=<ID=chr1>\n##INFO=<ID=AF,Number=A,Type=Float,Description=\"x\">\n"
CHROM = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"
RECORD = b"chr1\t100\t.\tA\tG\t50\tPASS\t.\tGT\t0|1\t0|1\t1|0\n"
NOT_FOUND = "     FATAL ERROR: Sample '%s' not found in the input VCF file.\n"


def both_forms(text):
    return [text, np.frombuffer(text, dtype=np.uint8)]


def fatal_text(capsys, fn, *a):
    """fn(*a) must end in fatal_error: -> what it wrote on stdout."""
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        fn(*a)
    assert e.value.code == 1
    return capsys.readouterr().out


# ---- find_sample_column

@pytest.mark.parametrize("form", [0, 1])
def test_sample_column_of_three_samples(form):
    data = both_forms(HEADER + CHROM + b"\tS1\tS2\tS3\n" + RECORD * 3)[form]
    assert [phaser.find_sample_column(data, s) for s in ("S1", "S2", "S3")] == [9, 10, 11]


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
def test_sample_in_the_last_column_with_and_without_cr(form, eol):
    data = both_forms(HEADER + CHROM + b"\tS1\tS2\tLAST" + eol + RECORD)[form]
    assert phaser.find_sample_column(data, "LAST") == 11


@pytest.mark.parametrize("form", [0, 1])
def test_text_without_a_final_newline(form):
    assert phaser.find_sample_column(both_forms(HEADER + CHROM + b"\tS1\tS2")[form], "S2") == 10          # the header is the whole text
    assert phaser.find_sample_column(both_forms(HEADER + CHROM + b"\tS1\tS2\n" + RECORD[:-1])[form], "S2") == 10          # the first record is its last line


@pytest.mark.parametrize("form", [0, 1])
def test_missing_sample_is_fatal(form, capsys):
    data = both_forms(HEADER + CHROM + b"\tS1\tS2\tS3\n" + RECORD)[form]
    assert fatal_text(capsys, phaser.find_sample_column, data, "S4") == NOT_FOUND % "S4"
    assert fatal_text(capsys, phaser.find_sample_column, data, "FORMAT") == NOT_FOUND % "FORMAT"          # the fixed columns are no samples


@pytest.mark.parametrize("form", [0, 1])
def test_no_chrom_line_before_the_first_record_is_fatal(form, capsys):
    data = both_forms(HEADER + RECORD + CHROM + b"\tS1\n" + RECORD)[form]
    assert fatal_text(capsys, phaser.find_sample_column, data, "S1") == NOT_FOUND % "S1"


# ---- per_bam

def test_per_bam_replicates_one_value_and_keeps_n():
    assert phaser.per_bam("255", 3, "mapq") == ["255", "255", "255"]
    assert phaser.per_bam("1,2,3", 3, "mapq") == ["1", "2", "3"]
    assert phaser.per_bam("255", 1, "mapq") == ["255"]


@pytest.mark.parametrize("what", ["mapq", "isize", "paired_end"])
def test_per_bam_refuses_any_other_count(what, capsys):
    want = ("     FATAL ERROR: Number of %s values and input BAMs does not match. Supply either one %s to be used for all BAMs or one %s per input BAM.\n"
            % (what, what, what))
    assert fatal_text(capsys, phaser.per_bam, "1,2", 3, what) == want
    assert fatal_text(capsys, phaser.per_bam, "1,2", 1, what) == want


# ---- bam_display_names

def test_bam_display_names():
    assert phaser.bam_display_names(["a.bam", "d/a.bam", "b.bam", "x/a.bam"]) == ["a.1", "a.2", "b", "a.3"]
    assert phaser.bam_display_names(["o1.sam"]) == ["o1.sam"]
    assert phaser.bam_display_names(["d/s.bam.sorted.bam", "t.bam"]) == ["s.sorted", "t"]          # ".bam" anywhere in the basename
    assert phaser.bam_display_names(["x.bam", "y.bam", "q/y.bam", "r/x.bam"]) == ["x.1", "y.1", "y.2", "x.2"]


# ---- prefetch_verdict

KEY = (255, 0.0, 1)
GUESS = {"chr20", "chr21", "chr22"}


@pytest.mark.parametrize("want,error,mine,key,have_shards", [
    (("used", "used"), False, {"chr20", "chr22"}, KEY, True),
    (("discarded", "discarded (error in the prefetch)"), True, {"chr20"}, KEY, False),
    (("discarded", "discarded (chromosomes ['chrM', 'chrX'] not in the guess)"), False, {"chrX", "chr20", "chrM"}, KEY, True),
    (("discarded", "discarded (filters differ)"), False, GUESS, (255, 500.0, 1), True),
    (("declined", "device path declined the file"), False, GUESS, KEY, False),
    # precedence: an error before everything, a guess that does not cover the table before the filters
    (("discarded", "discarded (chromosomes ['chrM'] not in the guess)"), False, {"chrM"}, (10, 0.0, 0), True),
    (("discarded", "discarded (error in the prefetch)"), True, {"chrM"}, (10, 0.0, 0), False),
    (("discarded", "discarded (filters differ)"), False, GUESS, (10, 0.0, 1), False),
])
def test_prefetch_verdict(want, error, mine, key, have_shards):
    assert phaser.prefetch_verdict(error, GUESS, mine, KEY, key, have_shards) == want


# ---- _Task and the run's task list

def some_run():
    return phaser._Run(phaser.build_parser().parse_args(["--vcf", "v", "--mapq", "255", "--baseq", "10", "--paired_end", "1", "--o", "o", "--bam", "a.bam,b.bam"]))


def test_task_returns_the_value():
    t = phaser._Task("phz-test-value", lambda: 41 + 1)
    assert t.result() == 42 and t.error is None
    assert t.seconds is not None and t.seconds >= 0.0
    assert t.thread.name == "phz-test-value" and not t.thread.is_alive()


def test_task_keeps_the_exception_for_result():
    def boom():
        raise KeyError("boom")
    t = phaser._Task("phz-test-raise", boom)
    t.join()                                  # only waits
    assert isinstance(t.error, KeyError) and t.value is None and t.seconds is not None
    with pytest.raises(KeyError, match="boom"):
        t.result()


def test_join_tasks_waits_for_a_slow_target():
    run = some_run()
    release = threading.Event()
    order = []

    def slow():
        release.wait()
        order.append("target ended")

    run.task("phz-test-quick", lambda: None)
    slow_task = run.task("phz-test-slow", slow)
    joiner = threading.Thread(target=lambda: (run.join_tasks(), order.append("joined")))
    joiner.start()
    joiner.join(0.2)
    assert joiner.is_alive() and order == []          # still waiting: the target has not been released
    release.set()
    joiner.join()
    assert order == ["target ended", "joined"] and not slow_task.thread.is_alive()
    assert [t.thread.name for t in run.tasks] == ["phz-test-quick", "phz-test-slow"]


def test_run_computes_the_shared_facts_once():
    run = some_run()
    assert run.bam_list == ["a.bam", "b.bam"] and not run.any_sam and (run.threads, run.pool_threads) == (1, 0)


# ---- StageClock

def test_stage_clock_fills_last_stage_seconds(monkeypatch, capsys):
    monkeypatch.delenv("PHZ_TIMING", raising=False)
    clock = phaser.StageClock()
    clock.mark("a"); clock.mark("b")
    clock.report()
    got = phaser.LAST_STAGE_SECONDS
    assert list(got) == ["a", "b", "total"] and all(v >= 0.0 for v in got.values())
    assert abs(got["total"] - (got["a"] + got["b"])) < 1e-9
    assert capsys.readouterr().err == ""


def test_stage_clock_lines_are_what_the_benchmark_parses(monkeypatch, capsys):
    monkeypatch.setenv("PHZ_TIMING", "1")
    clock = phaser.StageClock()
    names = ["vcf read + het-variant table", "bam decode + filters + qname interning", "H2D + K_map", "AS cutoff",
             "tally + pair tests + components + block phasing + rows", "network of chr1_100_A_G", "read haplotypes", "write the five files",
             "phased VCF text (+ the five files on a helper thread)", "phased VCF bgzf + tabix"]
    for n in names:
        clock.mark(n)
    clock.report()
    lines = capsys.readouterr().err.split("\n")
    assert lines[-1] == "" and len(lines) == len(names) + 2
    parsed = [re.match(r"^\[phz timing\] (\S.*?)\s+([0-9.]+) s$", line) for line in lines[:-1]]
    assert all(parsed)
    assert [m.group(1) for m in parsed] == names + ["total"]
    assert lines[3] == "[phz timing] %-55s %8.3f s" % ("AS cutoff", phaser.LAST_STAGE_SECONDS["AS cutoff"])


# ---- check_args

def cli_args(tmp_path, **over):
    (tmp_path / "in.vcf").write_text("x")
    a = {"vcf": str(tmp_path / "in.vcf"), "mapq": "255", "baseq": "10", "paired_end": "1", "o": str(tmp_path / "o"), "bam": ""}
    a.update(over)
    return phaser.build_parser().parse_args([x for k, v in a.items() for x in ("--" + k, v)])


def test_check_args_passes_good_arguments(tmp_path, capsys):
    (tmp_path / "a.bam").write_text("x")
    assert phaser.check_args(cli_args(tmp_path, bam=str(tmp_path / "a.bam")), 1) is None
    assert phaser.check_args(cli_args(tmp_path), 4) is None
    assert capsys.readouterr().out == ""


def test_check_args_refusals(tmp_path, capsys):
    fatal = "     FATAL ERROR: "
    sep = fatal + "ID separator must not be ':' or blank. Please choose another separator that is not found in the contig names.\n"
    assert fatal_text(capsys, phaser.check_args, cli_args(tmp_path, id_separator=":"), 1) == sep
    assert fatal_text(capsys, phaser.check_args, cli_args(tmp_path, id_separator=""), 1) == sep
    assert fatal_text(capsys, phaser.check_args, cli_args(tmp_path, process_slow="1"), 1) == (
        fatal + "--process_slow is not supported by this build (the GPU path holds all chromosomes; SURVEY.md section 2).\n")
    missing = str(tmp_path / "not_there")
    assert fatal_text(capsys, phaser.check_args, cli_args(tmp_path, vcf=missing), 1) == fatal + "VCF file does not exist.\n"
    for option in ("blacklist", "haplo_count_blacklist"):
        assert fatal_text(capsys, phaser.check_args, cli_args(tmp_path, **{option: missing}), 1) == fatal + "File: %s not found.\n" % missing
    (tmp_path / "a.bam").write_text("x")
    assert fatal_text(capsys, phaser.check_args, cli_args(tmp_path, bam=str(tmp_path / "a.bam") + "," + missing), 1) == fatal + "File: %s not found.\n" % missing


def test_check_args_refuses_one_rank_options_on_every_rank(tmp_path, capsys):
    """Both refusals come before the file checks (nothing here exists on disk): every rank stops at the same place, ahead of any collective."""
    fatal = "     FATAL ERROR: "
    nothing = dict(vcf=str(tmp_path / "not_there"), bam=str(tmp_path / "no.bam"))
    assert fatal_text(capsys, phaser.check_args, cli_args(tmp_path, py_hash_order="1", **nothing), 2) == (
        fatal + "--py_hash_order 1 needs all chromosomes on one rank (run it without torch.distributed).\n")
    assert fatal_text(capsys, phaser.check_args, cli_args(tmp_path, output_read_haplotypes="1", **nothing), 2) == (
        fatal + "--output_read_haplotypes 1 needs all chromosomes on one rank (run it without torch.distributed).\n")
    assert fatal_text(capsys, phaser.check_args, cli_args(tmp_path, py_hash_order="1", **nothing), 1) == fatal + "VCF file does not exist.\n"
