"""Native block phasing (phz_phase_block = the routine phz_rows_format runs per component) vs the pinned Python
restatement of phase_v3 (oracle/phasing_oracle.py, phaser.py:2107-2324) on random connected components:
conflicting edges, ties, weak points, brute force, stitching."""
import ctypes as C
import os
import random
import sys
from collections import OrderedDict

import numpy as np
import pytest

from conftest import REPO


def _oracle_inputs(n, edges, mbs):
    """-> (Phaser, variant names, variant-level neighbours, allele-level neighbours): what phase_block takes"""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import phasing_oracle as po
    ph = po.Phaser(["x"], max_block_size=mbs)
    names = ["chr1_%d_A_C" % (100 + 7 * i) for i in range(n)]
    vc = OrderedDict((u, set()) for u in names)
    ac = OrderedDict()
    for u in names:
        ac[u + ":0"] = set(); ac[u + ":1"] = set()
    for i, j, k in edges:
        a, b = names[i], names[j]
        vc[a].add(b); vc[b].add(a)
        if k == 0:
            ac[a + ":0"].add(b + ":0"); ac[b + ":0"].add(a + ":0"); ac[a + ":1"].add(b + ":1"); ac[b + ":1"].add(a + ":1")
        elif k == 1:
            ac[a + ":0"].add(b + ":1"); ac[b + ":0"].add(a + ":1"); ac[a + ":1"].add(b + ":0"); ac[b + ":1"].add(a + ":0")
    return ph, names, vc, ac


def _oracle_phase(n, edges, mbs):
    ph, names, vc, ac = _oracle_inputs(n, edges, mbs)
    res = ph.phase_block(names, vc, ac)
    idx = {u: i for i, u in enumerate(names)}
    return [[(idx[x.split(":")[0]], x.split(":")[1]) for x in sub] for sub in res if sub]


def _native_phase(lib, n, edges, mbs):
    ei = np.asarray([e[0] for e in edges], dtype=np.int32); ej = np.asarray([e[1] for e in edges], dtype=np.int32)
    ek = np.asarray([e[2] for e in edges], dtype=np.int8)
    first = np.zeros(n, dtype=np.int32); ln = np.zeros(n, dtype=np.int32); cfg = np.zeros(n + 1, dtype=np.uint8); ns = C.c_int32(0)
    st = lib.phz_phase_block(n, len(edges), ei.ctypes.data, ej.ctypes.data, ek.ctypes.data, mbs, first.ctypes.data, ln.ctypes.data,
                             cfg.ctypes.data, C.byref(ns))
    assert st == 0, st
    out = []; w = 0
    for k in range(ns.value):
        out.append([(int(first[k]) + t, chr(cfg[w + t])) for t in range(int(ln[k]))]); w += int(ln[k])
    return out


def _random_component(rng, n, extra, p_conflict, p_tie):
    truth = [rng.randint(0, 1) for _ in range(n)]
    pairs = set()
    for i in range(1, n):                         # spanning chain with occasional longer jumps keeps it connected
        j = max(0, i - rng.choice([1, 1, 1, 2, 3]))
        pairs.add((j, i))
    for _ in range(extra):
        i = rng.randrange(n); j = min(n - 1, i + rng.randint(1, 4))
        if i != j:
            pairs.add((min(i, j), max(i, j)))
    edges = []
    for i, j in sorted(pairs):
        k = 0 if truth[i] == truth[j] else 1
        r = rng.random()
        if r < p_tie:
            k = -1
        elif r < p_tie + p_conflict:
            k = 1 - k
        if rng.random() < 0.5:
            i, j = j, i
        edges.append((i, j, k))
    rng.shuffle(edges)
    return edges


@pytest.mark.parametrize("seed", range(6))
def test_native_phase_matches_oracle_on_random_components(seed):
    from phaser_amd import _lib
    _lib.build()
    lib = _lib.load()
    rng = random.Random(1000 + seed)
    checked = split = 0
    for t in range(220):
        n = rng.randint(2, 26)
        mbs = rng.choice([3, 4, 5, 6, 8, 9])
        edges = _random_component(rng, n, rng.randint(0, n), rng.choice([0.0, 0.05, 0.15, 0.3]), rng.choice([0.0, 0.05, 0.2]))
        try:
            want = _oracle_phase(n, edges, mbs)
        except (IndexError, ValueError):
            continue                               # the reference itself fails on this block (e.g. empty configuration)
        got = _native_phase(lib, n, edges, mbs)
        assert got == want, (n, mbs, edges)
        checked += 1
        split += len(want) != 1 or len(want[0]) != n
    assert checked > 150 and split > 20
