"""--output_network VARIANT (phaser/phaser.py:1127-1157): the allele links of the haplotype block that holds a variant.

    <o>.network.links.txt    variantA  variantB  connections  inferred -- for every pair v < o of the block's sorted variants and alleles x, y in (0, 1):
                             n = distinct reads (all BAMs) carrying allele x of v and allele y of o (generate_hap_network_all, :1928-1949); when n > 0 the
                             direct row  id_v:allele_v[x]  id_o:allele_o[y]  n  0  and then the inferred row  id_v:allele_v[1-x]  id_o:allele_o[1-y]  n  1
    <o>.network.nodes.txt    id  index  assigned_hap -- one row per distinct node of the links rows: its variant's place in the block, A when haplotype A carries
                             that allele there, else B.  The reference walks set(nodes): canonical tier = first appearance in the links rows, hash_order = the
                             order of that CPython 3.10 set (the native restatement behind --py_hash_order 1)

The counts are not computed here: they are cells 0, 1, 3, 4 of the variant pairs phz_tally left in HBM, gathered for the block by phz_variant_links (one small
launch over the resident edge list).  links_from_edges is its plain numpy restatement (tests).  The texts are put together with numpy gathers, no Python loop per
row: a block of 1,300 variants has millions of link rows."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

LINK_DTYPE = np.dtype(_lib.LINK_DTYPE)
HEAD_LINKS = b"variantA\tvariantB\tconnections\tinferred\n"
HEAD_NODES = b"id\tindex\tassigned_hap\n"


# ---------------------------------------------------------------- the block of a variant
def _local_blocks(eng):
    blocks = getattr(eng, "_net_blocks", None)
    if blocks is None:
        raise _lib.PhzError(_lib.PHZ_E_ARG, "the network of a variant needs a finished pass (Engine.finish) with the per-block arrays (Config.want_vcf)")
    return blocks


def block_of(eng, variant_id: str) -> Optional[Tuple[str, np.ndarray, np.ndarray]]:
    """-> (chromosome, the block's variants as indices of the tally's joint variant space in ascending order, allele index on haplotype A per variant) of the
    FINAL block (after phase_v3's splits, blocks starting with '-' dropped) of this rank's chromosomes that holds the unique id, or None: an id the variant set
    does not know, a variant of another rank's chromosome, a variant in no block (a singleton)."""
    blocks = _local_blocks(eng)
    vb = eng.G["var_base"]
    want = variant_id.encode()
    for c in eng.chrom_list:
        cv = eng.vs.chroms[c]
        off, blob = cv.pools()["uid"]
        at = blob.find(want + b"\n")
        while at > 0 and blob[at - 1:at] != b"\n":
            at = blob.find(want + b"\n", at + 1)
        if at < 0:
            continue
        v = int(np.searchsorted(off, at))
        b = blocks.get(c)
        if b is None:
            return None
        var = np.asarray(b["var"]); size = np.asarray(b["size"]).astype(np.int64)
        hit = np.flatnonzero(var == v)
        if len(hit) == 0:
            return None
        ends = np.cumsum(size)
        k = int(np.searchsorted(ends, hit[0], side="right"))
        lo = int(ends[k] - size[k]); hi = int(ends[k])
        members = var[lo:hi].astype(np.int64); hap = np.asarray(b["hap"])[lo:hi].astype(np.uint8)
        order = np.argsort(members, kind="stable")          # sort_var_ids (:869): by position = by index
        return c, (members[order] + vb[c]).astype(np.int32), hap[order]
    return None


# ---------------------------------------------------------------- the link records
def links_from_edges(edge_a, edge_b, edge_cells, vars) -> np.ndarray:
    """Plain restatement of phz_variant_links on fetched arrays: edges sorted by (a, b), nine cells per edge, `vars` strictly ascending."""
    vars = np.asarray(vars, dtype=np.int64)
    ea = np.asarray(edge_a, dtype=np.int64); eb = np.asarray(edge_b, dtype=np.int64)
    cells = np.asarray(edge_cells).reshape(-1, 9)
    n = len(vars)
    if n < 2 or len(ea) == 0:
        return np.zeros(0, dtype=LINK_DTYPE)
    i = np.searchsorted(vars, ea); j = np.searchsorted(vars, eb)
    member = (i < n) & (j < n)
    member &= (vars[np.minimum(i, n - 1)] == ea) & (vars[np.minimum(j, n - 1)] == eb)
    sel = np.flatnonzero(member)
    four = cells[sel][:, [0, 1, 3, 4]]
    e, k = np.nonzero(four > 0)                   # row-major: edge order, then (x, y) = (0,0) (0,1) (1,0) (1,1)
    out = np.zeros(2 * len(e), dtype=LINK_DTYPE)
    for inferred in (0, 1):
        r = out[inferred::2]
        r["i"] = i[sel][e]; r["j"] = j[sel][e]; r["count"] = four[e, k]
        r["allele_i"] = (k >> 1) ^ inferred; r["allele_j"] = (k & 1) ^ inferred; r["inferred"] = inferred
    return out


def links(eng, vars, _links=None) -> np.ndarray:
    """Link records (LINK_DTYPE) of the ascending variant set `vars` (joint variant space of the Engine's resident tally), through phz_variant_links.
    _links(vars) replaces the launch (CPU tests)."""
    vars = np.ascontiguousarray(vars, dtype=np.int32)
    if _links is not None:
        return np.asarray(_links(vars), dtype=LINK_DTYPE)
    check_resident(eng)
    ctx = eng.ctx; lib = eng.lib
    n = C.c_int64(0)
    vp = C.c_void_p(vars.ctypes.data) if len(vars) else None
    st = ctx.check(lib.phz_variant_links(ctx.h, vp, len(vars), None, 0, C.byref(n), _lib.PHZ_HOST), allow=(_lib.PHZ_E_CAPACITY,))
    rows = np.zeros(int(n.value), dtype=LINK_DTYPE)
    if st == _lib.PHZ_E_CAPACITY:
        ctx.check(lib.phz_variant_links(ctx.h, vp, len(vars), C.c_void_p(rows.ctypes.data), len(rows), C.byref(n), _lib.PHZ_HOST))
    return rows[:int(n.value)]


def check_resident(eng):
    """The pair cells are those of the LAST tally on the ctx: refuse when another pass (another Engine on the same context, a direct phz_tally) has replaced the
    one this Engine's blocks belong to -- the stamp the device row stage uses between its two stages."""
    want = eng.G.get("gen") if getattr(eng, "G", None) else None
    if want is None:
        return
    gen = C.c_uint64(0)
    eng.ctx.check(eng.lib.phz_tally_generation(eng.ctx.h, C.byref(gen)))
    if int(gen.value) != int(want):
        raise _lib.PhzError(_lib.PHZ_E_ARG, "the resident tally is no longer the one of this Engine's pass (another pass ran on the same context): run the pass again")


# ---------------------------------------------------------------- text
def _pool(items: Sequence[bytes]):
    """byte strings -> (uint8 blob, int64 offsets [n + 1])"""
    off = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in items], out=off[1:])
    return np.frombuffer(b"".join(items), dtype=np.uint8), off


def _gather_rows(pieces, n_rows: int) -> bytes:
    """Row r = the concatenation over pieces (blob, off, idx) of blob[off[idx[r]] : off[idx[r] + 1]]."""
    if n_rows == 0:
        return b""
    lens = [p[1][p[2] + 1] - p[1][p[2]] for p in pieces]
    row_len = np.sum(lens, axis=0)
    row_off = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(row_len, out=row_off[1:])
    out = np.empty(int(row_off[-1]), dtype=np.uint8)
    at = row_off[:-1].copy()
    for (blob, off, idx), ln in zip(pieces, lens):
        total = int(ln.sum())
        if total:
            first = np.zeros(n_rows, dtype=np.int64)
            np.cumsum(ln[:-1], out=first[1:])
            within = np.arange(total, dtype=np.int64) - np.repeat(first, ln)
            out[np.repeat(at, ln) + within] = blob[np.repeat(off[idx], ln) + within]
        at += ln
    return out.tobytes()


def _node_pool(ids: Sequence[bytes], alleles: Sequence[bytes], tail: bytes):
    """node 2 v + k = id_v ':' allele_v[k] + tail"""
    return _pool([ids[v >> 1] + b":" + alleles[v] + tail for v in range(2 * len(ids))])


def _b(x) -> bytes:
    return x if isinstance(x, (bytes, bytearray)) else str(x).encode()


def links_text(records: np.ndarray, ids, alleles) -> bytes:
    """The links file.  ids[v]: unique id of the set's v-th variant; alleles[2 v + k]: its allele strings in allele-index order."""
    ids = [_b(x) for x in ids]; alleles = [_b(x) for x in alleles]
    rec = np.asarray(records, dtype=LINK_DTYPE)
    n = len(rec)
    if n == 0:
        return HEAD_LINKS
    nodes = _node_pool(ids, alleles, b"\t")
    cu, ci = np.unique(rec["count"], return_inverse=True)
    counts = _pool([b"%d\t" % int(c) for c in cu])
    tails = _pool([b"0\n", b"1\n"])
    a = rec["i"].astype(np.int64) * 2 + rec["allele_i"]; b = rec["j"].astype(np.int64) * 2 + rec["allele_j"]
    return HEAD_LINKS + _gather_rows([nodes + (a,), nodes + (b,), counts + (ci.astype(np.int64),), tails + (rec["inferred"].astype(np.int64),)], n)


def node_order(records: np.ndarray, ids, alleles, hash_order: bool = False) -> np.ndarray:
    """The distinct nodes (2 v + k) of the link rows: in first-appearance order, or as CPython 3.10 (PYTHONHASHSEED=0) lists set(nodes) (phaser.py:1146)."""
    rec = np.asarray(records, dtype=LINK_DTYPE)
    seq = np.empty(2 * len(rec), dtype=np.int64)
    seq[0::2] = rec["i"].astype(np.int64) * 2 + rec["allele_i"]; seq[1::2] = rec["j"].astype(np.int64) * 2 + rec["allele_j"]
    uniq, first = np.unique(seq, return_index=True)
    order = uniq[np.argsort(first, kind="stable")]
    if not hash_order or len(order) == 0:
        return order
    blob, off = _pool([_b(ids[v >> 1]) + b":" + _b(alleles[v]) for v in order.tolist()])
    if off[-1] >= 2 ** 32:
        raise ValueError("node names exceed 4 GiB")
    off32 = np.ascontiguousarray(off, dtype=np.uint32); blob = np.ascontiguousarray(blob)
    out = np.zeros(len(order), dtype=np.int32)
    k = _lib.load().phz_py_set_order(C.c_void_p(blob.ctypes.data), C.c_void_p(off32.ctypes.data), len(order), len(order), 0, C.c_void_p(out.ctypes.data))
    if k != len(order):
        raise _lib.PhzError(_lib.PHZ_E_ARG, "phz_py_set_order")
    return order[out]


def nodes_text(records: np.ndarray, ids, alleles, hap_a, hash_order: bool = False) -> bytes:
    """The nodes file.  hap_a[v]: allele index haplotype A carries at the set's v-th variant."""
    order = node_order(records, ids, alleles, hash_order)
    if len(order) == 0:
        return HEAD_NODES
    ids = [_b(x) for x in ids]; alleles = [_b(x) for x in alleles]
    nodes = _node_pool(ids, alleles, b"\t")
    index = _pool([b"%d\t" % v for v in range(len(ids))])
    haps = _pool([b"B\n", b"A\n"])
    v = order >> 1
    on_a = (np.asarray(hap_a, dtype=np.int64)[v] == (order & 1)).astype(np.int64)
    return HEAD_NODES + _gather_rows([nodes + (order,), index + (v,), haps + (on_a,)], len(order))


def block_strings(eng, chrom: str, vars: np.ndarray) -> Tuple[List[bytes], List[bytes]]:
    """(unique ids, allele strings 2 v + k) of a block's variants from the variant set's string pools."""
    cv = eng.vs.chroms[chrom]
    local = np.asarray(vars, dtype=np.int64) - eng.G["var_base"][chrom]
    P = cv.pools()
    uoff, ublob = P["uid"]; aoff, ablob = P["allele"]
    ids = [ublob[int(uoff[v]):int(uoff[v + 1]) - 1] for v in local.tolist()]
    alleles = [ablob[int(aoff[2 * v + k]):int(aoff[2 * v + k + 1]) - 1] for v in local.tolist() for k in (0, 1)]
    return ids, alleles


def network(eng, variant_id: str, _links=None) -> Optional[dict]:
    """-> {"links": bytes, "nodes": bytes, "chrom", "variants"} for the block of `variant_id` among this rank's chromosomes, or None when it is in no block."""
    blk = block_of(eng, variant_id)
    if blk is None:
        return None
    chrom, vars, hap = blk
    rec = links(eng, vars, _links=_links)
    ids, alleles = block_strings(eng, chrom, vars)
    return {"chrom": chrom, "variants": vars, "records": rec, "links": links_text(rec, ids, alleles),
            "nodes": nodes_text(rec, ids, alleles, hap, hash_order=bool(eng.cfg.py_hash_order))}
