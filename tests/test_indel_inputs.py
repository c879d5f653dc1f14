"""The inputs of tests/test_gpu_mapper_general.py are what they claim to be: conditions on the generated records, the variant tables and the
C oracle's output alone -- nothing here measures the kernel, nothing needs a GPU."""
import os
import re

import numpy as np
import pytest

import indel_inputs as ii
from conftest import REPO
from indel_inputs import DEL, INS

# phz_map_general.hip: GEN_RPL records per lane x 256 lanes = GEN_TILE records per workgroup, GEN_WIN variants and GEN_CIG CIGAR words staged
# per tile, the staged window reaching POS(last record of the tile) + GEN_COVER
GEN_RPL = 4
GEN_TILE = 256 * GEN_RPL
GEN_WIN = 1024
GEN_COVER = 1 << 16
GEN_CIG = 4 * GEN_TILE
BASEQS = (0, 10, 30)


def test_tile_constants_follow_the_kernel_source():
    src = open(os.path.join(REPO, "phaser_amd", "csrc", "phz_map_general.hip")).read()
    val = lambda name: re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1).strip()
    assert val("GEN_RPL") == "4" and val("GEN_TILE") == "256 * GEN_RPL" and val("GEN_CIG") == "4 * GEN_TILE"
    assert val("GEN_WIN") == "1024" and val("GEN_COVER") == "65536"
    assert (GEN_TILE, GEN_WIN, GEN_COVER, GEN_CIG) == (1024, 1024, 65536, 4096)


def class_counts(vt, o_v, code):
    a0, a1 = vt.alleles()
    l0 = np.array([len(x) for x in a0])[o_v]; l1 = np.array([len(x) for x in a1])[o_v]
    return {"allele 0 multi-base": int(((code == 5) & (l0 > 1)).sum()), "allele 1 multi-base": int(((code == 6) & (l1 > 1)).sum()),
            "allele 0 single": int(((code == 5) & (l0 == 1)).sum()), "allele 1 single": int(((code == 6) & (l1 == 1)).sum()),
            "other single base": int((code < 4).sum()), "other text": int((code == 4).sum())}


def record_views(rb, vt):
    """Per record: its segments (indel_inputs.layout) and its candidates; and whether the fast pass MUST decline it: a candidate with
    ref_len > 1, a candidate in a segment with I / D, or more than two candidates."""
    pos = rb.pos.numpy().astype(np.int64); coff = rb.cigar_off.tolist(); words = rb.cigar.tolist()
    rl = vt.ref_len
    segs = []; cands = []
    decline = np.zeros(len(rb), bool); multi = np.zeros(len(rb), bool)
    for r in range(len(rb)):
        s = ii.layout(words[coff[r]:coff[r + 1]])
        c = ii.candidates(s, int(pos[r]), vt.pos, rl)
        segs.append(s); cands.append(c)
        multi[r] = any(rl[v] > 1 for v, si, rs in c)
        decline[r] = multi[r] or len(c) > 2 or any(s[si][3] for v, si, rs in c)
    return segs, cands, decline, multi


def tiles(rb, vt):
    """Per tile of GEN_TILE records: variants under its window (from the first variant at or after the tile's first POS up to its last POS + GEN_COVER),
    its CIGAR words."""
    pos = rb.pos.numpy().astype(np.int64); coff = rb.cigar_off.numpy()
    n = len(pos)
    first = np.arange(0, n, GEN_TILE); last = np.minimum(first + GEN_TILE, n) - 1
    window = np.searchsorted(vt.pos, pos[last] + GEN_COVER) - np.searchsorted(vt.pos, pos[first])
    return first, last, window, coff[last + 1] - coff[first]


@pytest.mark.parametrize("name", list(ii.SHAPES))
def test_inputs_hold_what_the_gpu_tests_rely_on(oracle_build, name):
    rb, vt = ii.inputs(name)
    n = len(rb)
    a0, a1 = vt.alleles()
    pos = rb.pos.numpy().astype(np.int64)
    assert np.all(np.diff(vt.pos) > 0) and np.all(np.diff(pos) >= 0)
    kinds = np.bincount(vt.kind, minlength=4)
    assert kinds.min() > 0.1 * len(vt) and vt.swap.any() and not vt.swap.all()
    ops = rb.cigar.numpy() & 15
    for op in (0, 1, 2, 3, 4, 7, 8):                                  # M I D N S = X all occur
        assert (ops == op).sum() > 20, op
    assert (rb.seq.numpy() == 4).sum() > 100
    want = {}
    for baseq in BASEQS:
        q = rb.qual.numpy()
        assert baseq == 0 or ((q < baseq).mean() > 0.03 and (q >= baseq).mean() > 0.5)      # qualities on both sides of baseq
        o_r, o_v, code, o_t = want[baseq] = ii.expected(oracle_build, rb, vt, baseq)
        # 1. every class occurs often enough; 2. the 32-byte slot of the oracle never cut a text
        for cls, cnt in class_counts(vt, o_v, code).items():
            assert cnt >= (500 if name == "main" else 50), (name, baseq, cls, cnt)
        assert max(len(t) for t in o_t) <= 30
    segs, cands, decline, multi = record_views(rb, vt)
    first, last, window, n_words = tiles(rb, vt)
    o_r, o_v, code, o_t = want[10]
    if name == "main":
        assert n // GEN_TILE >= 8                                      # 4. the tile scan has something to join
        assert 0.10 <= decline.mean() <= 0.90                          # 5. both the fast pass and the work list are busy, in every tile
        per_tile = np.add.reduceat(decline.astype(np.int64), first)
        assert per_tile.min() > 0 and (per_tile < last - first + 1).all()
        assert (np.bincount(o_r, minlength=n) >= 3).sum() > 100        # ... and records with three or more calls exist
        # 3. the four ways a multi-character text comes about, counted on the oracle's calls (the read offsets behind each text come from
        # indel_inputs.call_offsets, which must reproduce the oracle's text first)
        lut = "ACGTN"
        for baseq in (10, 30):
            o_r, o_v, code, o_t = want[baseq]
            seq = rb.seq.numpy(); qual = rb.qual.numpy(); rl = vt.ref_len
            spliced_other = del_match = ins_match = lowq_n = 0
            where = [{v: (si, rs) for v, si, rs in c} for c in cands]
            for r, v, c, t in zip(o_r.tolist(), o_v.tolist(), code.tolist(), o_t):
                si, rs = where[r][v]
                offs, spliced = ii.call_offsets(segs[r][si], rs, int(rl[v]))
                assert "".join(lut[seq[r, x]] if qual[r, x] >= baseq else "N" for x in offs) == t
                spliced_other += spliced > 0 and c not in (5, 6)
                # a REF of 2-4 bases gives a one-character text only when its other characters were 'D' placeholders, a REF of one base gives
                # several characters only through a spliced insertion
                del_match += vt.kind[v] == DEL and t == vt.alt_text[v]
                ins_match += vt.kind[v] == INS and t == vt.alt_text[v]
                lowq_n += rl[v] > 1 and any(qual[r, x] < baseq and seq[r, x] != 4 for x in offs)
            assert min(spliced_other, del_match, ins_match, lowq_n) >= 100, (baseq, spliced_other, del_match, ins_match, lowq_n)
    if name == "dense":
        # 6. windows beyond the staged GEN_WIN variants, with records in them that have a REF > 1 candidate (and so must be declined)
        big = window > GEN_WIN
        assert big.sum() >= 2
        for t in np.nonzero(big)[0]:
            assert multi[first[t]:last[t] + 1].sum() > 100
    if name == "manyop":
        # 7. tiles with more CIGAR words than are staged, and records with calls whose words start beyond the staged ones
        coff = rb.cigar_off.numpy()
        big = n_words > GEN_CIG
        assert big.sum() >= 2
        has_call = np.bincount(o_r, minlength=n) > 0
        for t in np.nonzero(big)[0]:
            beyond = coff[first[t]:last[t] + 1] - coff[first[t]] >= GEN_CIG
            assert (beyond & has_call[first[t]:last[t] + 1]).sum() > 100
    if name == "retry":
        # 8. both retries of Mapper.map_general run: more calls than its first capacity (n // 2 + 4096), more text than its first pool (4096)
        for baseq in BASEQS:
            o_r, o_v, code, o_t = want[baseq]
            assert len(o_r) > n // 2 + 4096
            assert sum(len(t) for t, c in zip(o_t, code.tolist()) if c == 4) > 4096
    if name == "shifted":
        assert pos.min() >= 1 << 30 and vt.pos.min() >= 1 << 30        # 9.
