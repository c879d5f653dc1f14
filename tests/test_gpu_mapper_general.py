"""K_map_general (phz_map_general.hip, the mapper behind --include_indels 1) against the C oracle on records that CARRY indel and multi-base
alleles (tests/indel_inputs.py; tests/test_indel_inputs.py checks on the CPU that those inputs reach what is exercised here: the work list of
several workgroups, the tile scan, truncated windows, CIGAR words beyond the staged ones, both capacity retries, coordinates beyond 2^30)."""
import dataclasses
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import indel_inputs as ii
from indel_inputs import DEL, INS, MNP, SNP

pytestmark = pytest.mark.gpu

LUT = np.frombuffer(b"ACGTN", dtype=np.uint8)


@pytest.fixture(scope="module")
def mapper():
    from phaser_amd.mapper import Mapper
    return Mapper(0)


def run_general(mapper, shard, vt, baseq, want_text):
    off, ab = vt.allele_pool()
    return mapper.map_general(shard, torch.from_numpy(vt.pos.astype(np.int32)), torch.from_numpy(vt.ref_len), torch.from_numpy(off),
                              torch.from_numpy(ab), baseq, want_text=want_text)


def check_calls(calls, want, what):
    o_r, o_v, code, _ = want
    c = calls.cpu()
    assert c.n == len(o_r), (what, c.n, len(o_r))
    for name, got, exp in (("read_idx", c.read_idx, o_r), ("var_idx", c.var_idx, o_v), ("code", c.code, code)):
        got = got.numpy()
        if not np.array_equal(got, exp):
            k = int(np.nonzero(got != exp)[0][0])
            raise AssertionError("%s: %s differs first at call %d of %d: got %d, oracle %d (record %d, variant %d, text %r)"
                                 % (what, name, k, len(exp), got[k], exp[k], o_r[k], o_v[k], want[3][k]))


def check_pool(pool, rb, want, baseq, what):
    """The text of EVERY code-4 call, rebuilt from the pool's read offsets the way the drop-in prints it (read_variant_map.py:314), is the oracle's;
    the first and last offset frame the pool exactly and no other call owns characters."""
    o_r, o_v, code, o_t = want
    toff = pool.call_off.numpy().astype(np.int64); ro = pool.roff.numpy().astype(np.int64)
    assert len(toff) == len(o_r) + 1 and toff[0] == 0 and toff[-1] == len(ro), (what, toff[:1], toff[-1:], len(ro))
    span = np.diff(toff)
    assert np.all(span >= 0) and np.array_equal(span > 0, code == 4), what
    assert len(ro) == sum(len(t) for t, c in zip(o_t, code.tolist()) if c == 4), what
    assert ro.min(initial=0) >= 0 and ro.max(initial=0) < rb.L
    rec = np.repeat(o_r.astype(np.int64), span)
    ch = LUT[rb.seq.numpy()[rec, ro]]
    ch = np.where(rb.qual.numpy()[rec, ro] >= baseq, ch, ord("N")).astype(np.uint8)
    for k in np.nonzero(code == 4)[0].tolist():
        got = ch[toff[k]:toff[k + 1]].tobytes().decode().replace("D", "")
        assert got == o_t[k], "%s: text of call %d (record %d, variant %d): got %r, oracle %r" % (what, k, o_r[k], o_v[k], got, o_t[k])


def check_all_paths(mapper, rb, vt, want, baseq, what):
    from phaser_amd import soa
    host = soa.pack_readbatch(rb)
    for space, shard in (("device", host.to("cuda")), ("host", host)):
        calls, pool = run_general(mapper, shard, vt, baseq, True)
        check_calls(calls, want, "%s, %s shard, with text" % (what, space))
        check_pool(pool, rb, want, baseq, "%s, %s shard" % (what, space))
        calls, pool = run_general(mapper, shard, vt, baseq, False)              # what the Engine asks for (engine.py add_shard)
        assert pool is None
        check_calls(calls, want, "%s, %s shard, without text" % (what, space))


@pytest.mark.parametrize("baseq", [0, 10, 30])
@pytest.mark.parametrize("name", list(ii.SHAPES))
def test_shapes_vs_oracle(mapper, oracle_build, name, baseq):
    """(record, variant, code) lists element for element and every other-allele text, on the device-resident and the host shard, with and without
    the text pool."""
    rb, vt = ii.inputs(name)
    want = ii.expected(oracle_build, rb, vt, baseq)
    assert len(want[0]) > 5000
    check_all_paths(mapper, rb, vt, want, baseq, name)


def head(rb, n):
    keep = torch.zeros(len(rb), dtype=torch.bool); keep[:n] = True
    return rb.select(keep)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2048])
def test_shard_sizes_around_a_tile(mapper, oracle_build, n):
    """One record; one short of, exactly and one more than a tile of 1024 records; exactly two tiles."""
    rb, vt = ii.inputs("retry")
    rb = head(rb, n)
    assert len(rb) == n
    want = ii.expected(oracle_build, rb, vt, 10)
    assert len(want[0]) >= 3
    check_all_paths(mapper, rb, vt, want, 10, "n = %d" % n)


def test_one_variant(mapper, oracle_build):
    rb, vt = ii.inputs("dense")
    for kind in (DEL, INS, MNP, SNP):
        of_kind = np.nonzero(vt.kind == kind)[0]
        one = vt.take([int(of_kind[len(of_kind) // 4])])
        want = ii.expected(oracle_build, rb, one, 10)
        assert len(want[0]) >= 3
        check_all_paths(mapper, rb, one, want, 10, "one variant of kind %d" % kind)


@pytest.mark.parametrize("where", ["before", "after"])
def test_all_variants_off_the_reads(mapper, oracle_build, where):
    rb, vt = ii.inputs("shifted" if where == "before" else "manyop")
    away = dataclasses.replace(vt, pos=vt.pos + (-(1 << 29) if where == "before" else 1 << 20))
    if where == "before":
        assert away.pos.min() > 0 and away.pos.max() + 4 < rb.pos.min()
    else:
        assert away.pos.min() > int(rb.pos.max()) + 2 * ii.REACH                 # REACH bounds what introns add to a record
    want = ii.expected(oracle_build, rb, away, 10)
    assert len(want[0]) == 0
    check_all_paths(mapper, rb, away, want, 10, "variants %s the reads" % where)


def records(rows, L):
    """[(POS, CIGAR text, base codes or None)] -> ReadBatch with bases from a fixed seed and qualities above any baseq in use."""
    from phaser_amd import synth
    from phaser_amd.soa import parse_cigar
    rng = np.random.default_rng(77)
    n = len(rows)
    words = []; coff = [0]
    for pos, cg, _ in rows:
        ops = parse_cigar(cg)
        assert sum(k for op, k in ops if op in (0, 1, 4, 7, 8)) == L
        words += [(k << 4) | op for op, k in ops]; coff.append(len(words))
    z = torch.zeros(n, dtype=torch.int32)
    return synth.ReadBatch("chr1", L, torch.tensor([r[0] for r in rows], dtype=torch.int32), z, torch.full((n,), 255, dtype=torch.uint8), z, z,
                           torch.arange(n, dtype=torch.int32), torch.tensor(coff, dtype=torch.int64), torch.tensor(words, dtype=torch.int64),
                           torch.from_numpy(rng.integers(0, 4, (n, L)).astype(np.uint8)), torch.full((n, L), 37, dtype=torch.uint8))


def test_ref_run_at_the_end_of_a_segment(mapper, oracle_build):
    """A REF of three bases whose run ends exactly with a segment is called, one that needs a base more is not -- at the end of a record, in front of an intron
    (where the genome goes on but the segment does not), in front of a soft clip, with a deletion under the run's first base and with an insertion keyed at the run's last base."""
    L = 50
    rows = [(1000, "50M", None),                # segment = [1000, 1050)
            (2000, "20M100N30M", None),         # segments [2000, 2020) and [2120, 2150)
            (3000, "40M10S", None),             # [3000, 3040)
            (4000, "10S38M2D2M", None),         # [4000, 4042): the pseudo read ends D D and two bases
            (5000, "48M2I", None)]              # [5000, 5048), an insertion keyed at its last base
    rb = records(rows, L)
    ends = [1050, 2020, 2150, 3040, 4042, 5048]
    pos = sorted(e - 3 for e in ends) + sorted(e - 2 for e in ends)
    pos = np.array(sorted(pos), dtype=np.int64)
    nv = len(pos)
    vt = ii.VariantTable("chr1", pos, np.full(nv, MNP, np.uint8), ["ACG"] * nv, ["TTT"] * nv, np.zeros(nv, np.uint8), np.zeros(nv, bool))
    want = ii.expected(oracle_build, rb, vt, 10)
    called = set(pos[want[1]].tolist())
    assert called == {e - 3 for e in ends}                     # the inputs do what the docstring says, by the oracle
    assert any(len(t) == 5 for t in want[3])                   # ... and the insertion at the last base is part of a text
    check_all_paths(mapper, rb, vt, want, 10, "REF run at a segment's end")


def test_empty_second_allele_never_matches(mapper, oracle_build):
    rb, vt = ii.inputs("shifted")
    vt = dataclasses.replace(vt, a1_empty=np.arange(len(vt)) % 2 == 0)
    a0, a1 = vt.alleles()
    assert a1[0] == "" and a1[1] != ""
    want = ii.expected(oracle_build, rb, vt, 10)
    o_v, code = want[1], want[2]
    emptied = vt.a1_empty[o_v]
    assert not (code[emptied] == 6).any() and (code[~emptied] == 6).sum() > 500 and (code[emptied] == 5).sum() > 500
    check_all_paths(mapper, rb, vt, want, 10, "empty second allele")


def test_dropin_bytes_vs_oracle_binary(mapper, oracle_build, tmp_path):
    """read_variant_map.do_read_variant_map on the main shape rendered as SAM + variant table: the rvm_oracle binary's TSV, byte for byte."""
    from phaser_amd import read_variant_map, synth
    rb, vt = ii.inputs("main")
    sam = "\n".join(synth.sam_lines(rb, [("chr1", 248956422)])) + "\n"
    tp = tmp_path / "t.tsv"; tp.write_text(vt.table_text())
    op = tmp_path / "oracle.tsv"
    subprocess.run([os.path.join(oracle_build, "rvm_oracle"), "--variant_table", str(tp), "--baseq", "10", "--o", str(op)], input=sam.encode(), check=True)
    want = op.read_text()
    old = sys.stdin
    sys.stdin = io.StringIO(sam)
    try:
        read_variant_map.do_read_variant_map(str(tp), 10, str(tmp_path / "o.tsv"), 1, 0, _mapper=mapper)
    finally:
        sys.stdin = old
    got = (tmp_path / "o.tsv").read_text()
    assert want.count("\n") > 20000
    assert got == want
