"""Everything phz_tally hands out (every array of phz_tally_fetch, every field of phz_tally_sizes), restated from the call lines
(variant, QNAME id, class, BAM) of every chromosome with dicts, sets and sorts.  The definitions are those of oracle/phasing_oracle.py
(Phaser.add_bam, Phaser.finish up to the pair test); nothing here knows about tiles, windows, hash tables or cursors.

    line space      the chromosomes in list order, inside a chromosome the BAMs in order, inside a BAM the lines as they arrive
    class           0 ref / 1 alt / 2 other / 255 dropped by the alignment-score cutoff (add_bam: such a line is never seen)
    item            a distinct (QNAME, variant, class) of the kept lines
    owner BAM       of a QNAME: the LAST BAM that holds a ref/alt line of it (add_bam: `tgt[q] = lst` overwrites the list of an earlier BAM)
    linked item     a ref/alt item with a line in the owner BAM (= an entry of the surviving read_vars list)
    linked pair     some QNAME holds linked items on both variants (= the pair is in finish()'s overlap dictionary)
    var_rank        finish() walks read_vars in insertion order (QNAMEs by their first ref/alt line over all BAMs) and, inside a list with two or
                    more distinct variants, the variants in line order: variant a becomes a key of the overlap dictionary at
                    (first ref/alt line of the QNAME) << 32 | (first linked line of a in that QNAME); the smallest such value over the QNAMEs, all-ones if none
    cells           the nine set intersections of the pair test: cell (i, j) of (a, b) = QNAMEs with an item (a, i) and an item (b, j)
    cto, stats      finish()'s cis / trans / oth and sup / tot / cfg of a pair
    noise           finish()'s 5 % rule over the per-variant line counters

QNAME ids are per chromosome (the ids of two chromosomes never meet), variants and lines are offset per chromosome into the call's spaces."""
import numpy as np

NONE_RANK = np.uint64(0xFFFFFFFFFFFFFFFF)


def n_qid_of(saved, c):
    R = saved["tally"][c]
    return max(1, saved["n_qid"].get(c, int(R["line_qid"].max()) + 1 if len(R["line_qid"]) else 1))


def n_bams_of(saved, chrom_list):
    return 1 + max([b for c in chrom_list for b, _, _ in saved["tally"][c]["bam_offsets"]] + [0])


def chromosome_lines(R):
    """(variant, QNAME id, class, BAM) of a chromosome in line order, as plain int lists; the BAM of a line from bam_offsets (ascending, back to back)"""
    n = len(R["line_var"])
    bam = np.zeros(n, np.int64)
    at = 0
    for b, base, m in R["bam_offsets"]:
        assert base == at, "the shards of a chromosome lie back to back in BAM order"
        bam[base:base + m] = b
        at += m
    assert at == n
    if "line_bam" in R:
        assert np.array_equal(bam, np.asarray(R["line_bam"], dtype=np.int64))
    return (np.asarray(R["line_var"], dtype=np.int64).tolist(), np.asarray(R["line_qid"], dtype=np.int64).tolist(),
            np.asarray(R["line_cls"], dtype=np.int64).tolist(), bam.tolist())


def restate(saved, chrom_list, n_bams):
    nb = n_bams
    NV = sum(saved["tally"][c]["nv"] for c in chrom_list)
    var_count = np.zeros((NV, 3), np.int32); var_distinct = np.zeros((NV, 3), np.int32)
    var_first = np.full(NV, -1, np.int64); var_rank = np.full(NV, NONE_RANK, np.uint64)
    line_cls = []
    lists = {}                       # (variant, allele, BAM) -> chromosome-local QNAME ids in line order
    pairs = {}                       # (a, b), a < b -> [nine cells, linked]
    n_items = pair_events = 0
    V0 = L0 = 0
    for c in chrom_list:
        R = saved["tally"][c]
        var, qid, cls, bam = chromosome_lines(R)
        line_cls += cls
        groups = {}                  # QNAME id -> its kept lines (line, variant, class, BAM), in line order
        for i, (v, q, k, b) in enumerate(zip(var, qid, cls, bam)):
            if k == 255:
                continue
            assert 0 <= v < R["nv"] and 0 <= k <= 2 and 0 <= b < nb
            v += V0; g = L0 + i
            var_count[v, k] += 1
            if var_first[v] < 0:
                var_first[v] = g
            if k < 2:
                lists.setdefault((v, k, b), []).append(q)
            groups.setdefault(q, []).append((g, v, k, b))
        for q, lines in groups.items():
            items = sorted({(v, k) for g, v, k, b in lines})
            n_items += len(items)
            for v, k in items:
                var_distinct[v, k] += 1
            refalt = [x for x in lines if x[2] < 2]
            linked_items = set(); first_linked = {}
            if refalt:
                owner = max(b for g, v, k, b in refalt)
                first = min(g for g, v, k, b in refalt)
                for g, v, k, b in refalt:
                    if b == owner:
                        linked_items.add((v, k))
                        first_linked[v] = min(first_linked.get(v, g), g)
                if len(first_linked) >= 2:
                    for v, g in first_linked.items():
                        r = np.uint64((first << 32) | g)
                        if r < var_rank[v]:
                            var_rank[v] = r
            for x in range(len(items)):
                a, ka = items[x]
                for y in range(x + 1, len(items)):
                    b2, kb = items[y]
                    if b2 == a:
                        continue
                    pair_events += 1
                    rec = pairs.get((a, b2))
                    if rec is None:
                        rec = pairs[(a, b2)] = [[0] * 9, 0]
                    rec[0][ka * 3 + kb] += 1
                    if (a, ka) in linked_items and (b2, kb) in linked_items:
                        rec[1] = 1
        V0 += R["nv"]; L0 += len(var)
    keys = sorted(pairs)
    ne = len(keys)
    ea = np.array([k[0] for k in keys], dtype=np.int32); eb = np.array([k[1] for k in keys], dtype=np.int32)
    cells = np.array([pairs[k][0] for k in keys], dtype=np.int32).reshape(ne, 9)
    linked = np.array([pairs[k][1] for k in keys], dtype=np.uint8)
    x = cells.astype(np.int64)
    cis = x[:, 0] + x[:, 4]                                   # |A0 & B0| + |A1 & B1|
    trans = x[:, 3] + x[:, 1]                                 # |A1 & B0| + |A0 & B1|
    oth = x[:, 6] + x[:, 7] + x[:, 2] + x[:, 5] + x[:, 8]
    cto = np.stack([cis, trans, oth], 1).astype(np.int32).reshape(ne, 3)
    cfg = np.where(cis > trans, 0, np.where(cis < trans, 1, -1))
    stats = np.stack([cis, trans, np.maximum(cis, trans), cis + trans + oth, cfg], 0).astype(np.int32).reshape(5, ne)
    rl_start = np.zeros(NV * 2 * nb + 1, np.uint32)
    rl_qid = []
    for v in range(NV):
        for k in range(2):
            for b in range(nb):
                rl_qid += lists.get((v, k, b), [])
                rl_start[(2 * v + k) * nb + b + 1] = len(rl_qid)
    match = mism = 0
    for m0, m1, mm in var_count.tolist():
        m = m0 + m1
        if m > 0 and (float(mm) / float(mm + m)) < 0.05:
            match += m; mism += mm
    out = {"nv": NV, "nb": nb, "var_count": var_count, "var_first": var_first, "var_distinct": var_distinct, "var_rank": var_rank,
           "line_cls": np.array(line_cls, dtype=np.uint8), "ea": ea, "eb": eb, "cells": cells, "linked": linked, "cto": cto, "stats": stats,
           "rl_start": rl_start, "rl_qid": np.array(rl_qid, dtype=np.int32),
           "sizes": {"n_lines": L0, "n_kept": int(var_count.sum()), "n_edges": ne, "n_read_list": len(rl_qid), "n_items": n_items, "pair_events": pair_events,
                     "noise_match": match, "noise_mismatch": mism}}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


ARRAYS = (("var_count", (-1, 3)), ("var_first", (-1,)), ("var_distinct", (-1, 3)), ("var_rank", (-1,)), ("ea", (-1,)), ("eb", (-1,)), ("cells", (-1, 9)),
          ("linked", (-1,)), ("cto", (-1, 3)), ("stats", (5, -1)), ("rl_start", (-1,)), ("rl_qid", (-1,)))


def assert_equal(got, sizes, want, where=""):
    """got / sizes: what run_tally returns (flat arrays of phz_tally_fetch, the phz_tally_sizes structure); want: restate().  Exact, every array, every field."""
    for f, val in want["sizes"].items():
        assert int(getattr(sizes, f)) == val, (where, f, int(getattr(sizes, f)), val)
    n = want["sizes"]["n_lines"]
    assert np.array_equal(got["line_cls"][:n], want["line_cls"]), (where, "line_cls")
    for name, shape in ARRAYS:
        g = np.asarray(got[name]); w = want[name]
        assert g.size == w.size, (where, name, g.size, w.size)
        g = g.reshape(shape) if g.size else g.reshape(w.shape)
        if not np.array_equal(g, w.astype(g.dtype) if name == "linked" else w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s: %d of %d entries differ, first at %s: got %s, want %s" % (where, name, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))
