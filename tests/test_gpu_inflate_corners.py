"""K_inflate and k_crc32 on an MI355X (libphz.so through Mapper(0).ctx, as tests/test_gpu_bamdev.py) on the corner streams of tests/deflate_builder.py:
what tests/test_emu_inflate_corners.py checks under the host emulation, here with the real unaligned 16-byte accesses, the LDS [slot][lane] tables
and 64 divergent lanes.  Expected bytes from zlib; 32-byte canaries between the members' outputs; a few calls in all, plus one small call per catalogue
member and per invalid stream (an invalid stream ends in a status code: every bound it probes is checked before the access)."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import inflate_corners as IC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    from phaser_amd.mapper import Mapper
    return IC.GpuDevice(Mapper(0).ctx)


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
