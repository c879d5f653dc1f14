"""The device BAM decoder (phz_bamdev.hip: k_seg_start, k_hop, BamOpen::counting_hop) on files with planted fake record chains
(tests/bam_boundary_inputs.py), against the sequential pure-Python reader bamio.shards_from_bam -- never against the host decoder.

k_seg_start guesses the first record boundary of every 262,144-byte segment from 12 plausible headers in coordinate order; k_hop verifies (segment k must
arrive where segment k + 1 starts) and counting_hop repairs: the start of a segment whose predecessor is clean and arrives elsewhere is replaced by that
arrival, and the hop runs again.  The layouts put a run of fake records under chosen guesses (and prove on the CPU that each guess lands on it), the
repairs are read from the PHZ_TIMING line of every pass.  What the counts below say about the loop:
  * a mismatch is repaired only when the segment before it was clean in that pass, so a run of r fakes at consecutive guesses takes r passes, one repair
    each (the fake chain of segment k makes segment k unclean for k + 1, until k's own start has been repaired);
  * passes are numbered from 0 and pass 7 must be clean: 7 fakes in a row converge, 8 send the file to the host decoder;
  * a "corrupt chain" on a segment whose predecessor is unclean (a dead-end fake chain) does not fail the file."""
import re

import pytest

import bam_boundary_inputs as bb

pytestmark = pytest.mark.gpu
REPAIR = r"bam device: (\d+) guessed record boundaries were fakes, repaired from the preceding chain \(pass (\d+)\)\n"


@pytest.fixture(scope="module")
def ctx():
    from phaser_amd.mapper import Mapper
    return Mapper(0).ctx


def _device(ctx, lay, chroms, monkeypatch, capfd):
    """-> (shards or None, interners, [(repairs, pass)] of the call's repair lines, its stderr)"""
    from phaser_amd import bamio
    monkeypatch.setenv("PHZ_TIMING", "1")
    before = capfd.readouterr().out
    it = {}
    dev = bamio.shards_from_bam_device(ctx, lay.path, it, 0, False, False, chroms=chroms)
    err = capfd.readouterr().err
    repairs = [(int(n), int(p)) for n, p in re.findall(REPAIR, err)]
    print(before, end="")                          # (what an earlier call of the same test printed stays in the report)
    print(lay.name, chroms, "repairs (count, pass):", repairs, "declined" if dev is None else "%d records" % sum(s.n for s in dev.values()))
    return dev, it, repairs, err


class Declined(Exception):
    """the device path answered None for a valid file"""


def _equal(lay, chroms, dev, it):
    if dev is None:
        raise Declined((lay.name, chroms))
    want, names = lay.reference(chroms)
    bb.same_shards(want, names, dev, it, (lay.name, chroms, "device"))


# (repairs, pass) lines expected of a whole-file decode, from reading counting_hop
ONE_PER_PASS = {"isolated": 1, "three_in_a_row": 3, "seven": 7, "last_segment": 1}
CONVERGING = [(n, f) for n in ONE_PER_PASS for f in bb.SEGMENT_FLAVOURS[n] if f != "unordered"]


@pytest.mark.parametrize("name,flavour", CONVERGING)
def test_fakes_at_segment_guesses_are_repaired(ctx, name, flavour, monkeypatch, capfd):
    """r carriers at consecutive guesses: the reference's shards after exactly r repairs, one in each of the passes 0 .. r-1.  dead_end: the fake chain
    of a segment ends in a negative block_size ("corrupt chain") while its predecessor is unclean, which must not fail the file; last_segment: the
    chain from the fake runs to the end of the piece."""
    lay = bb.segment_layout(name, flavour)
    dev, it, repairs, _ = _device(ctx, lay, None, monkeypatch, capfd)
    _equal(lay, None, dev, it)
    assert repairs == [(1, p) for p in range(ONE_PER_PASS[name])]


def test_fakes_out_of_coordinate_order_are_not_taken(ctx, monkeypatch, capfd):
    """The fakes' positions descend: k_seg_start's key rule skips the whole run (the host rule takes fake #6, the layout checks both) and nothing
    has to be repaired."""
    lay = bb.segment_layout("isolated", "unordered")
    dev, it, repairs, _ = _device(ctx, lay, None, monkeypatch, capfd)
    _equal(lay, None, dev, it)
    assert repairs == []


@pytest.mark.parametrize("flavour", ["resync", "dead_end"])
def test_eight_fakes_in_a_row_go_to_the_host_decoder(ctx, flavour, monkeypatch, capfd):
    """Eight carriers at consecutive guesses need a ninth pass: the device path declines ("did not converge") after one repair in each of the passes
    0 .. 7 and never returns shards; the same ctx then decodes `isolated`."""
    lay = bb.segment_layout("eight", flavour)
    dev, _, repairs, err = _device(ctx, lay, None, monkeypatch, capfd)
    assert dev is None
    assert "record boundaries did not converge" in err
    assert repairs == [(1, p) for p in range(8)]
    lay = bb.segment_layout("isolated", flavour)
    dev, it, repairs, _ = _device(ctx, lay, None, monkeypatch, capfd)
    _equal(lay, None, dev, it)
    assert repairs == [(1, 0)]


def test_record_longer_than_two_segments(ctx, monkeypatch, capfd):
    """Guesses inside one 600 KB record find the same boundary, the segments between them are empty: equal, nothing repaired, whole file (the
    layout's self-check is about its segments) and restricted (other pieces, or the whole stream where 8 members prove no boundary)."""
    lay = bb.long_record_layout()
    for chroms in CHROM_SETS.values():
        dev, it, repairs, _ = _device(ctx, lay, chroms, monkeypatch, capfd)
        _equal(lay, chroms, dev, it)
        assert repairs == []


CHROM_SETS = {"whole": None, "chr21": {"chr21"}, "chr22": {"chr22"}, "both": {"chr21", "chr22"}}


@pytest.mark.parametrize("flavour,variant,key", [(f, v, k) for f in ("dead_end", "resync") for v in bb.MEMBER_VARIANTS for k in CHROM_SETS])
def test_members_that_start_on_a_fake(ctx, flavour, variant, key, monkeypatch, capfd):
    """The device path works from the same plan as the host's restricted open and takes a piece's start as exact: with every member but the first
    starting on a fake, whole file and restricted sets equal the reference."""
    lay = bb.member_layout(flavour, variant)
    dev, it, _, _ = _device(ctx, lay, CHROM_SETS[key], monkeypatch, capfd)
    _equal(lay, CHROM_SETS[key], dev, it)


def covered_params():
    out = []
    for variant in bb.MEMBER_VARIANTS:
        for key in CHROM_SETS:
            why = bb.COVERED_XFAIL.get((variant, key))
            marks = [pytest.mark.xfail(strict=True, raises=Declined, reason=why)] if why else []
            out.append(pytest.param(variant, key, marks=marks, id="%s-%s" % (variant, key)))
    return out


@pytest.fixture
def covered_layout(variant):
    return bb.member_layout("resync", variant, covered=True)


@pytest.mark.parametrize("variant,key", covered_params())
def test_members_that_hold_nothing_but_resyncing_fakes(ctx, covered_layout, variant, key, monkeypatch, capfd):
    """The limit of the plan (tests/test_bam_boundaries.py has the host's side of it).  Where the reference boundaries of this file cannot be proven -- the
    walk arrives on fakes of refID 0 inside chr22, the refIDs sampled by the search do not ascend -- the device plan takes the whole record stream as one
    piece, as the host takes its full open, so nothing is declined for that: whole file and restricted sets equal the reference.  The one case in which the
    device path declines is the host's expected failure: the piece of chr21 ends inside a record, its chain breaks, and the host decoder then reports it."""
    dev, it, _, _ = _device(ctx, covered_layout, CHROM_SETS[key], monkeypatch, capfd)
    _equal(covered_layout, CHROM_SETS[key], dev, it)
