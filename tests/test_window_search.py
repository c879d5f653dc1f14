"""K_map's window search as a unit on the CPU: phaser_amd/csrc/phz_lbound.h is plain C++, so tests/window_search_unit.cpp includes it, is built
with the host compiler (no sanitizer, no GPU toolchain) and compares window_lower_bound<D> with std::lower_bound for every depth D = 0 .. 9, every
window length 0 .. 2^D (padded with INT_MAX), windows that start at entry 0, runs of consecutive positions, repeated positions, entries near
2,000,000,000 and just below INT_MAX, and the keys: every entry, entry +- 1, 0, INT_MAX, -1, INT_MIN (= the sentinel the phase-1a bracket passes for
"no single-run record in this wave").  Negative keys must yield 0, which is what the compare form of the search gave for them."""
import os
import subprocess

from conftest import REPO


def test_window_lower_bound_matches_std_lower_bound(tmp_path):
    src = os.path.join(REPO, "tests", "window_search_unit.cpp")
    exe = str(tmp_path / "window_search_unit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "phaser_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1_000_000, r.stdout
