"""The host BAM decoder (phz_bam.cpp) on files with planted fake record chains (tests/bam_boundary_inputs.py), against the sequential pure-Python
reader bamio.shards_from_bam.  CPU only.

Two guess points are exercised: the parallel record hop of phz_bam_decode (a fake at a segment's guess must send the file through the sequential hop,
never into the shards) and `probe` / `probe_from_before` of bam_plan (a member that starts on a fake must not become a reference boundary or a piece
limit; before the plan verified its candidates, restricted opens of these files raised or returned 11 of 300 records).  Every layout
checks itself when it is built -- each guess lands on the planted fake or on a true boundary, as intended -- so a test cannot pass by not reaching
its path."""
import pytest

import bam_boundary_inputs as bb


def _decode(lay, chroms, threads, monkeypatch, what):
    from phaser_amd import bamio
    if threads > 1:
        monkeypatch.setenv("PHZ_BAM_PAR_MIN", "0")
    else:
        monkeypatch.delenv("PHZ_BAM_PAR_MIN", raising=False)
    want, names = lay.reference(chroms)
    it = {}
    got = bamio.shards_from_bam_native(lay.path, it, 0, False, False, chroms=chroms, threads=threads)
    bb.same_shards(want, names, got, it, (lay.name, what, "threads=%d" % threads))
    return want


SEGMENT_CASES = [(n, f) for n in bb.SEGMENT_LAYOUTS for f in bb.SEGMENT_FLAVOURS[n]]


@pytest.mark.parametrize("name,flavour", SEGMENT_CASES)
def test_segment_layouts_whole_file(name, flavour, monkeypatch):
    """The device's segment layouts through the host decoder: sequential, and the parallel hop with 8 and 28 segments (its guesses lie elsewhere than
    the device's, wherever they fall the shards are the reference's)."""
    lay = bb.segment_layout(name, flavour)
    for threads in (1, 2, 7):
        want = _decode(lay, None, threads, monkeypatch, "whole file")
    assert sum(s.n for s in want.values()) == len(lay.true)         # no fake was taken for a record by the reference either


@pytest.mark.parametrize("flavour", ["resync", "dead_end", "unordered"])
def test_fake_at_a_guess_of_the_parallel_hop(flavour, monkeypatch, capfd):
    """A carrier at guess 4 of 8 of the host's parallel hop (threads = 2; the layout proves with the host rule that the guess lands on fake #6): the
    verification -- segment 3 must arrive where segment 4 began -- fails, the sequential hop decodes the file, and says so."""
    lay = bb.host_layout(flavour)
    monkeypatch.setenv("PHZ_TIMING", "1")
    capfd.readouterr()
    _decode(lay, None, 2, monkeypatch, "whole file")
    assert "bam record hop: sequential" in capfd.readouterr().err
    for threads in (1, 7):
        _decode(lay, None, threads, monkeypatch, "whole file")


def test_long_record_whole_and_restricted(monkeypatch, capfd):
    """A record longer than two segments: guesses inside it find the same boundary, the segments between are empty, and the parallel hop still verifies."""
    lay = bb.long_record_layout()
    monkeypatch.setenv("PHZ_TIMING", "1")
    for chroms in (None, {"chr21"}, {"chr22"}, {"chr21", "chr22"}):
        for threads in (1, 2, 7):
            capfd.readouterr()
            _decode(lay, chroms, threads, monkeypatch, chroms)
            if threads > 1:
                assert "bam record hop: parallel segments, boundaries verified" in capfd.readouterr().err


CHROM_SETS = {"whole": None, "chr21": {"chr21"}, "chr22": {"chr22"}, "both": {"chr21", "chr22"}}


MEMBER_CASES = [(f, v, k) for f in ("dead_end", "resync") for v in bb.MEMBER_VARIANTS for k in CHROM_SETS]


@pytest.mark.parametrize("flavour,variant,key", MEMBER_CASES)
def test_members_that_start_on_a_fake(flavour, variant, key, monkeypatch):
    """Every member but the first starts on fake #5 of a run of 40: whatever `probe` is asked, its first candidate is a fake.  Whole file and restricted
    to either reference or both, sequential and parallel: the reference's shards, and nothing raises."""
    lay = bb.member_layout(flavour, variant)
    for threads in (1, 4):
        want = _decode(lay, CHROM_SETS[key], threads, monkeypatch, key)
    assert sorted(want) == sorted(CHROM_SETS[key] or {"chr21", "chr22"}) and all(s.n == bb.PER_REF for s in want.values())


def covered_params():
    from phaser_amd import _lib
    out = []
    for variant in bb.MEMBER_VARIANTS:
        for key in CHROM_SETS:
            why = bb.COVERED_XFAIL.get((variant, key))
            marks = [pytest.mark.xfail(strict=True, raises=_lib.PhzError, reason=why)] if why else []      # the documented refusal, nothing else
            out.append(pytest.param(variant, key, marks=marks, id="%s-%s" % (variant, key)))
    return out


@pytest.fixture
def covered_layout(variant):
    """built (and self-checked) in the set-up: an AssertionError of the builder is an error of the test, never its expected failure"""
    return bb.member_layout("resync", variant, covered=True)


@pytest.mark.parametrize("variant,key", covered_params())
def test_members_that_hold_nothing_but_resyncing_fakes(covered_layout, variant, key, monkeypatch):
    """The limit of the plan: a member that starts on a resyncing fake and is followed by a member that starts in the SAME run.  The walk from the first
    arrives on a fake of the second.  Whole-file decodes do not use the plan and must be right; the restricted case that is wrong is an expected failure,
    and only as the refusal it is known to be (PhzError)."""
    for threads in (1, 4):
        _decode(covered_layout, CHROM_SETS[key], threads, monkeypatch, key)


@pytest.mark.parametrize("flavour", ["dead_end", "resync"])
@pytest.mark.parametrize("variant", bb.MEMBER_VARIANTS)
def test_ref_weights_of_members_that_start_on_a_fake(flavour, variant):
    """bam_ref_weights runs the reference boundary search alone: it answers for every file, names in header order, bytes that add up to no more than the file"""
    import os
    from phaser_amd import bamio
    lay = bb.member_layout(flavour, variant)
    w = bamio.bam_ref_weights(lay.path)
    assert list(w) == ["chr21", "chr22"] and all(v >= 0 for v in w.values()) and sum(w.values()) <= os.path.getsize(lay.path)
    if flavour == "dead_end":                  # every fake is rejected: the search sees the true references, about half of the file each
        assert all(0.4 * os.path.getsize(lay.path) < v for v in w.values()), w
