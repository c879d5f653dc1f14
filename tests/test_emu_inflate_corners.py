"""K_inflate (phaser_amd/csrc/phz_inflate.hip) under the host-side HIP emulation on DEFLATE streams that zlib's encoder never writes -- every stream
tests/test_emu_inflate.py feeds it comes from zlib.compressobj, a narrow subset of RFC 1951, while BAMs in the field are mostly written by libdeflate.
tests/deflate_builder.py writes the streams bit by bit: code-length runs across the literal/length | distance boundary, 15-bit codes and the cold table
slots behind them, one / no / only-the-last distance code, a literal/length code that is only end-of-block, length 258 as symbol 284 + 31, empty and
misaligned stored blocks, a match as a member's last token for every (distance, length) around the copy widths, distance 32768 and distance == position;
every source alignment; streams from libdeflate (a committed fixture); and invalid streams, each with the status code it must end in.  The expected
bytes are zlib's decode of the same stream, and no byte outside a member's output may change (tests/inflate_corners.py holds the shared checks).
The same checks on the GPU: tests/test_gpu_inflate_corners.py."""
import pytest

import inflate_corners as IC


@pytest.fixture(scope="module")
def device():
    return IC.EmuDevice()


def test_catalogue_holds_what_it_should():
    """every stream of the catalogue is valid for zlib (a builder bug must not pass as an agreed rejection), and the listed corners are all there"""
    cat = IC.expected_catalogue()
    B = IC.B
    for d in B.OVERLAP_DISTS:
        assert "overlap_mid_d%d" % d in cat
        for l in B.OVERLAP_LENS:
            s, want = cat["overlap_final_d%d_l%d" % (d, l)]
            assert want[-l:] == (want[-l - d:-l] * (l // d + 1))[:l] and len(want) >= l + d          # really ends in that match
    assert set(B.OVERLAP_DISTS) == set(range(1, 20)) | {31, 32, 33, 63, 64, 65}
    assert set(B.OVERLAP_LENS) == {3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 258}
    for name in IC.WORKGROUP_STREAMS:
        assert name in cat
    assert B.deep_lengths(263, 15) == [1, 2, 3, 4, 5, 6, 7] + [15] * 256
    for n, depth in ((263, 15), (30, 15), (19, 7), (286, 15), (5, 3), (2, 1)):
        L = B.deep_lengths(n, depth)
        assert len(L) == n and max(L) == depth and B.kraft_left(L) == 0
    assert max(len(w) for _, w in cat.values()) > 33000 and min(len(w) for _, w in cat.values()) <= 4


def test_each_member_alone(device):
    IC.check_each_alone(device)


def test_shuffled_among_zlib_members(device):
    IC.check_shuffled_among_zlib_members(device)


@pytest.mark.parametrize("name", IC.WORKGROUP_STREAMS)
def test_full_workgroup_plus_one(device, name):
    IC.check_full_workgroup_plus_one(device, name)


def test_source_alignment(device):
    IC.check_source_alignment(device)


def test_streams_of_another_encoder(device):
    IC.check_other_encoder(device)


@pytest.mark.parametrize("case", IC.INVALID, ids=[c[0] for c in IC.INVALID])
def test_invalid_stream_ends_in_its_status_code(device, case):
    IC.check_invalid(device, case)


@pytest.mark.parametrize("case", IC.LENIENT, ids=[c[0] for c in IC.LENIENT])
def test_what_the_kernel_accepts_and_zlib_does_not(device, case):
    IC.check_lenient(device, case)
