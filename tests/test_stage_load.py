"""The descriptor lengths of a K_map tile's staging loads as a unit on the CPU: phaser_amd/csrc/phz_stageload.h is plain C++ up to the two device macros, so
tests/stage_load_unit.cpp includes it, is built with the host compiler (no GPU toolchain) and checks, for every tile of shards of 1 .. 770 records, for
windows that start up to 520 entries before (and at, and behind) the end of tables of 0 .. 2^31 - 1 entries and for CIGAR word counts around the LDS cap,
that a lane's word lies inside the descriptor exactly when the guard the load used to sit under let the lane load."""
import os
import subprocess

from conftest import REPO


def test_descriptor_lengths_match_the_old_guards(tmp_path):
    src = os.path.join(REPO, "tests", "stage_load_unit.cpp")
    exe = str(tmp_path / "stage_load_unit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "phaser_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1_000_000, r.stdout
