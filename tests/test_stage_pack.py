"""K_map's narrow staging word as a unit on the CPU: phaser_amd/csrc/phz_stagepack.h is plain C++, so tests/stage_pack_unit.cpp includes it, is built with
the host compiler (no GPU toolchain) and round-trips var[0:20) | rec[20:28) | code[28:32) at the field limits -- var 0 and 2^20 - 1, rec 0 and 255, all
sixteen values of the code field (the kernels emit 0 .. 4) -- with every record number and every single bit of the variant field in between, and checks
the host predicate that chooses between the 4-byte and the 8-byte form (text planes, records per tile, table size, PHZ_MAP_WIDE_STAGE)."""
import os
import subprocess

from conftest import REPO


def test_stage_word_round_trip_and_form_predicate(tmp_path):
    src = os.path.join(REPO, "tests", "stage_pack_unit.cpp")
    exe = str(tmp_path / "stage_pack_unit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "phaser_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 8_000, r.stdout
