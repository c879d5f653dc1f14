"""The per-op step of K_map's lean walker as a unit on the CPU: phaser_amd/csrc/phz_leanwalk.h is plain C++, so tests/lean_walk_unit.cpp includes it, is
built with the host compiler (no sanitizer, no GPU toolchain) and walks records op by op, with std::lower_bound over a sorted window in place of the
kernel's LDS search.  A record the walker keeps must give the candidate list (window index, read offset, inserted-text word, ordinal) of a direct
restatement of walk_read<0>'s position rule; a record it poisons must have one of the restated causes, and every cause must poison (only the verdict
is compared then).  The records:
  * every sequence of 1-3 words over M I D N S H P = X G with lengths 0, 1, 2, 7 and an N of 70,000 (which puts a later run past `cover`);
  * every sequence of 4-5 ops, six seeded draws of those lengths each (every combination would be 41^5 records);
  * 200,000 seeded sequences of 6-12 ops with up to four insertions;
each against a window with a het SNP on the first and the last base of every run and one before and one behind every run boundary, and against an
empty window.  The neutral word (a zero-length P, what the kernel feeds the lanes whose record has ended) appended 1-3 times must change nothing.
Every poison cause and both kinds of clean record with inserted text (first segment: found by looking one op ahead; later segment: carried forward)
must have occurred."""
import os
import subprocess

from conftest import REPO

CAUSES = ("G", "third_insertion", "ins_after_I", "ins_after_S", "ins_after_H", "ins_after_P", "ins_after_G", "ins_after_empty", "beyond_cover")


def test_lean_step_matches_walk_read_rule(tmp_path):
    src = os.path.join(REPO, "tests", "lean_walk_unit.cpp")
    exe = str(tmp_path / "lean_walk_unit")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "phaser_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.strip().splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1_000_000, r.stdout
    count = {}
    for ln in lines[:-1]:
        f = ln.split()
        count[" ".join(f[:-1])] = int(f[-1])
    for c in CAUSES:
        assert count["cause " + c] > 0, (c, r.stdout)
    for k in ("clean", "poisoned", "candidates", "clean_ins_first", "clean_ins_later", "neutral"):
        assert count[k] > 0, (k, r.stdout)
