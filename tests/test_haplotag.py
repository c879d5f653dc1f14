"""--output_haplotag_bam without a GPU: the plain restatement of the rule (tests/haplotag_restatement.py) on hand-built rows, one case per clause; the record rewrite
of the restatement on a small BAM; the header reader; the option and its refusals in check_args."""
import gzip
import struct

import numpy as np
import pytest

from haplotag_restatement import pick, read_tags, tag_stream, tags_from_text

REC = np.dtype([("block", "<i4"), ("bam", "<i4"), ("qid", "<i4"), ("a", "<i4"), ("b", "<i4")])


def rows(*tuples):
    return np.array(list(tuples), dtype=REC)


# one chromosome of 10 templates, 4 blocks of which 3 are phased
ONE = dict(n_phased=3, bam=0, blk_chrom=np.zeros(4, np.int32), tmpl_base=np.array([0, 10], np.int64), n_templates=10)


def word(block, hp):
    return ((block + 1) << 2) | hp


def test_two_blocks_with_different_totals_the_larger_wins():
    tag = pick(rows((0, 0, 4, 2, 1), (2, 0, 4, 1, 5)), **ONE)
    assert tag[4] == word(2, 2) and int((tag != 0).sum()) == 1
    assert pick(rows((2, 0, 4, 1, 5), (0, 0, 4, 2, 1)), **ONE).tolist() == tag.tolist()          # the order of the rows does not matter


def test_equal_totals_the_smaller_block_index_wins():
    tag = pick(rows((1, 0, 7, 0, 3), (0, 0, 7, 2, 1), (2, 0, 7, 3, 0)), **ONE)
    assert tag[7] == word(0, 1)


def test_a_tie_in_the_winning_block_gives_hp_0_and_does_not_fall_through():
    tag = pick(rows((0, 0, 3, 2, 2), (1, 0, 3, 3, 0)), **ONE)
    assert tag[3] == word(0, 0)                     # block 1 is decisive (3 : 0) but lost on the total (3 < 4)


def test_a_block_behind_n_phased_is_ignored():
    tag = pick(rows((3, 0, 5, 9, 0), (1, 0, 5, 0, 1)), **ONE)
    assert tag[5] == word(1, 2)
    assert not pick(rows((3, 0, 6, 9, 0)), **ONE).any()


def test_rows_of_another_bam_are_ignored():
    tag = pick(rows((0, 1, 2, 9, 0), (1, 0, 2, 0, 1)), **ONE)
    assert tag[2] == word(1, 2)
    assert pick(rows((0, 1, 2, 9, 0), (1, 0, 2, 0, 1)), **dict(ONE, bam=1))[2] == word(0, 1)


def test_templates_of_two_chromosomes_share_nothing_and_no_rows_give_zeros():
    two = dict(n_phased=2, bam=0, blk_chrom=np.array([0, 1], np.int32), tmpl_base=np.array([0, 3, 8], np.int64), n_templates=8)
    tag = pick(rows((0, 0, 2, 1, 0), (1, 0, 2, 0, 1), (1, 0, 4, 2, 2)), **two)
    assert tag.tolist() == [0, 0, word(0, 1), 0, 0, word(1, 2), 0, word(1, 0)]
    assert not pick(rows(), **two).any()


# ------------------------------------------------------------------------------------------------ the record rewrite of the restatement
def small_bam(tmp_path):
    from phaser_amd import bamio
    recs = [dict(ref_id=0, pos=10 + i, mapq=255 if i != 2 else 3, flag=0x63, tlen=200, qname="t%d" % (i // 2), cigar=[(0, 4)], seq="ACGT", qual=[30] * 4,
                 tags={"AS": 7} if i % 2 else {}) for i in range(6)]
    path = str(tmp_path / "s.bam")
    bamio.write_bam(path, [("c1", 1000), ("c2", 1000)], recs)
    return path, gzip.open(path, "rb").read()


def test_tag_stream_appends_hp_and_ps_and_raises_block_size(tmp_path):
    from phaser_amd import bamio
    path, raw = small_bam(tmp_path)
    refs, off = bamio.parse_header(raw)
    tag = {"c1": np.array([word(1, 2), 0, word(0, 0)], np.uint32)}
    out = tag_stream(raw, dict(mapq=255), {"c1"}, {"c1": {"t0": 0, "t1": 1, "t2": 2}}, tag, np.array([111, 70000], np.uint32))
    got = read_tags(raw[:off] + out)
    assert got == [("c1", "t0", 2, 70000), ("c1", "t0", 2, 70000), ("c1", "t1", None, None), ("c1", "t2", None, None), ("c1", "t2", None, None)]
    first, = struct.unpack_from("<i", raw, off)
    assert struct.unpack_from("<i", out, 0)[0] == first + 11 and out[4:4 + first] == raw[off + 4:off + 4 + first]
    assert out[4 + first:4 + first + 11] == b"HPC\x02PSI" + struct.pack("<I", 70000)
    assert tag_stream(raw, dict(mapq=255), {"c2"}, {}, {}, []) == b""
    assert bamio.bam_header_bytes(path) == raw[:off]


def test_header_bytes_of_a_header_that_spans_many_members(tmp_path):
    """300 references cut into BGZF members of 64 bytes: the header ends in the middle of a member, more than a hundred members in"""
    from phaser_amd import bamio
    refs = [("contig_%d_%s" % (i, "x" * (i % 9)), 1000 + i) for i in range(300)]
    rec = dict(ref_id=299, pos=5, mapq=60, flag=0x63, tlen=100, qname="r", cigar=[(0, 4)], seq="ACGT", qual=[30] * 4, tags={})
    for k, member_bytes in enumerate((64, 61, 60000)):
        path = str(tmp_path / ("many_%d.bam" % k))
        bamio.write_bam(path, refs, [rec, rec], member_bytes=member_bytes)
        raw = gzip.open(path, "rb").read()
        got_refs, off = bamio.parse_header(raw)
        assert got_refs == refs and off > 100 * 64 and bamio.bam_header_bytes(path) == raw[:off]
    bamio.write_bam(str(tmp_path / "none.bam"), [], [], member_bytes=5)               # no reference, no record: the header is the whole file
    assert bamio.bam_header_bytes(str(tmp_path / "none.bam")) == gzip.open(str(tmp_path / "none.bam"), "rb").read()
    open(str(tmp_path / "cut.bam"), "wb").write(open(path, "rb").read()[:40])         # the file ends inside the header
    with pytest.raises(ValueError):
        bamio.bam_header_bytes(str(tmp_path / "cut.bam"))


def test_tags_from_text_follows_the_rule():
    text = (b"contig\tstart\tstop\tbam\tread\taCount\tbCount\thaplotype\n"
            b"c\t5\t90\tx\tr1\t2\t1\tA\nc\t5\t90\tx\tr2\t1\t1\t-\nc\t5\t90\ty\tr1\t0\t4\tB\nc\t200\t300\tx\tr1\t0\t3\tB\nc\t200\t300\tx\tr2\t0\t1\tB\nc\t400\t400\tx\tr3\t5\t0\tA\n")
    phased = lambda contig, start, stop: start != stop
    assert tags_from_text(text, "x", phased) == {("c", "r1"): (1, 5)}          # r1: 3 = 3, the first block stays; r2: its winning block tied; r3: a one-variant block
    assert tags_from_text(text, "y", phased) == {("c", "r1"): (2, 5)}


# ------------------------------------------------------------------------------------------------ the command line
BASE = ["--vcf", "in.vcf.gz", "--sample", "S1", "--mapq", "255", "--baseq", "10", "--paired_end", "1", "--o", "out"]


def test_the_option_parses():
    from phaser_amd import phaser
    assert phaser.build_parser().parse_args(BASE + ["--bam", "a.bam"]).output_haplotag_bam == 0
    assert phaser.build_parser().parse_args(BASE + ["--bam", "a.bam", "--output_haplotag_bam", "1"]).output_haplotag_bam == 1


def test_check_args_refuses_several_ranks(capsys):
    from phaser_amd import phaser
    args = phaser.build_parser().parse_args(BASE + ["--bam", "a.bam", "--output_haplotag_bam", "1"])
    with pytest.raises(SystemExit):
        phaser.check_args(args, 2)
    assert "--output_haplotag_bam 1 needs all chromosomes on one rank (run it without torch.distributed)." in capsys.readouterr().out


def test_check_args_refuses_a_sam_input(capsys):
    from phaser_amd import phaser
    args = phaser.build_parser().parse_args(BASE + ["--bam", "a.bam,b.sam", "--output_haplotag_bam", "1"])
    with pytest.raises(SystemExit):
        phaser.check_args(args, 1)
    assert "--output_haplotag_bam 1 needs BAM inputs" in capsys.readouterr().out
    args = phaser.build_parser().parse_args(BASE + ["--bam", "a.bam,b.sam"])          # without the option a .sam input gets as far as the file checks
    with pytest.raises(SystemExit):
        phaser.check_args(args, 1)
    assert "VCF file does not exist" in capsys.readouterr().out
