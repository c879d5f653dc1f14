"""--output_read_haplotypes 1: which read belongs to which haplotype of which block.

    <o>.read_haplotypes.txt    contig  start  stop  bam  read  aCount  bCount  haplotype -- one row per (block, BAM, template) with at least one kept call line on a
                               voting variant of the block: aCount = its lines on alleles haplotype A carries, bCount = on the other allele (the two mates of a
                               template count twice, as in reads[idx], phaser.py:1318), haplotype = A / B / - (a tie).  contig, start, stop, bam are columns 1-3 and
                               the bam column of the block's row in haplotypic_counts; with --unphased_vars 1 a variant in no block is a block of its own whose
                               haplotype A is allele 0 (the singleton rows, :1194-1206)

The reference answers half of this: --output_read_ids 1 puts two comma-joined QNAME lists into every haplotypic_counts row (:1086-1123, :1196-1217) -- no counts, and a
read on both sides looks like two reads.  Nothing is tallied again here: the votes are read from the per-(variant, allele, BAM) read lists phz_tally left in HBM, for all
blocks at once, by phz_read_haplotypes (key generation over the read-list array, a device sort, a run reduction).  rows_from_lists is its plain numpy restatement
(tests).  The text is put together with numpy gathers, no Python loop per row."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .network import _gather_rows, _pool, check_resident

READHAP_DTYPE = np.dtype(_lib.READHAP_DTYPE)
HEAD = b"contig\tstart\tstop\tbam\tread\taCount\tbCount\thaplotype\n"


# ---------------------------------------------------------------- the caller's table
def _blacklisted(eng, c: str) -> Optional[np.ndarray]:
    """--haplo_count_blacklist per variant of a chromosome (the loader's marks + Config.haplo_blacklist names, phaser.py:1070), or None"""
    cv = eng.vs.chroms[c]; nv = len(cv)
    bl = cv.blacklisted if getattr(cv, "blacklisted", None) is not None and len(cv.blacklisted) == nv and cv.blacklisted.any() else None
    if eng.cfg.haplo_blacklist:
        named = np.fromiter((c + "_" + str(int(p)) in eng.cfg.haplo_blacklist for p in cv.pos), dtype=np.uint8, count=nv)
        bl = named if bl is None else (bl | named)
    return bl


def block_table(eng) -> dict:
    """The block table phz_read_haplotypes takes, from the per-block arrays of a finished pass: the chromosomes in the order haplotypic_counts lists them
    (engine.block_chrom_order), the blocks of a chromosome in block order, variant indices of the tally's joint variant space; with unphased_vars every variant in
    no block follows as a one-variant block whose haplotype A is allele 0.  Per block also what the text needs: chromosome, smallest and largest position over ALL
    its variants (blacklisted ones included, :1068)."""
    blocks = getattr(eng, "_net_blocks", None)
    if blocks is None:
        raise _lib.PhzError(_lib.PHZ_E_ARG, "read_haplotypes needs a finished pass (Engine.finish) with the per-block arrays (Config.want_vcf)")
    order = getattr(eng, "_net_order", None) or list(eng.chrom_list)
    vb = eng.G["var_base"]; NV = int(eng.G["nv"]); nb = len(eng.bam_names)
    chroms = list(eng.chrom_list)
    pos = np.zeros(NV, dtype=np.int64); chrom_of_var = np.zeros(NV, dtype=np.int32); var_skip = np.zeros(NV, dtype=np.uint8)
    for ci, c in enumerate(chroms):
        n = len(eng.vs.chroms[c])
        pos[vb[c]:vb[c] + n] = eng.vs.chroms[c].pos; chrom_of_var[vb[c]:vb[c] + n] = ci
        bl = _blacklisted(eng, c)
        if bl is not None:
            var_skip[vb[c]:vb[c] + n] = bl != 0
    sizes = []; var = []; hap = []
    for c in order:
        b = blocks.get(c)
        if b is None:
            continue
        sizes.append(np.asarray(b["size"]).astype(np.int64)); var.append(np.asarray(b["var"]).astype(np.int64) + vb[c]); hap.append(np.asarray(b["hap"]).astype(np.uint8))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    sizes = cat(sizes, np.int64); var = cat(var, np.int64); hap = cat(hap, np.uint8)
    n_phased = len(sizes)
    if eng.cfg.unphased_vars == 1:
        free = np.ones(NV, dtype=bool); free[var] = False
        single = np.flatnonzero(free)
        sizes = np.concatenate([sizes, np.ones(len(single), np.int64)]); var = np.concatenate([var, single]); hap = np.concatenate([hap, np.zeros(len(single), np.uint8)])
    blk_off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=blk_off[1:])
    start = np.zeros(len(sizes), dtype=np.int64); stop = np.zeros(len(sizes), dtype=np.int64); chrom = np.zeros(len(sizes), dtype=np.int32)
    if len(var):
        filled = np.flatnonzero(sizes > 0)
        p = pos[var]
        start[filled] = np.minimum.reduceat(p, blk_off[:-1][filled]); stop[filled] = np.maximum.reduceat(p, blk_off[:-1][filled])
        chrom[filled] = chrom_of_var[var[blk_off[:-1][filled]]]
    bam_skip = np.zeros(nb, dtype=np.uint8)
    for b in eng.cfg.haplo_count_bam_exclude:
        if 0 <= int(b) < nb:
            bam_skip[int(b)] = 1
    return {"blk_off": blk_off, "blk_var": np.ascontiguousarray(var, dtype=np.int32), "blk_hap": np.ascontiguousarray(hap, dtype=np.uint8), "var_skip": var_skip,
            "bam_skip": bam_skip, "n_phased": n_phased, "chroms": chroms, "chrom": chrom, "start": start, "stop": stop}


# ---------------------------------------------------------------- the records
def rows_from_lists(rl_start, rl_qid, n_bams, blk_off, blk_var, blk_hap, var_skip=None, bam_skip=None) -> np.ndarray:
    """Plain restatement of phz_read_haplotypes on fetched arrays: the read lists as phz_tally_fetch returns them (list (2 v + allele) * n_bams + bam holds
    rl_qid[rl_start[list] : rl_start[list + 1]]) and the caller's block table."""
    rs = np.asarray(rl_start, dtype=np.int64); nb = int(n_bams)
    n_lists = len(rs) - 1; nv = n_lists // (2 * nb)
    blk_off = np.asarray(blk_off, dtype=np.int64); blk_var = np.asarray(blk_var, dtype=np.int64); blk_hap = np.asarray(blk_hap, dtype=np.int64)
    vblk = np.full(nv, -1, dtype=np.int64); vside = np.zeros(nv, dtype=np.int64)
    vblk[blk_var] = np.repeat(np.arange(len(blk_off) - 1), np.diff(blk_off)); vside[blk_var] = blk_hap
    if var_skip is not None:
        vblk[np.asarray(var_skip)[:nv] != 0] = -1
    lst = np.repeat(np.arange(n_lists), np.diff(rs))                       # the list every entry belongs to
    qid = np.asarray(rl_qid)[rs[0]:rs[-1]].astype(np.int64)
    bam = lst % nb; v = (lst // nb) >> 1; allele = (lst // nb) & 1
    live = vblk[v] >= 0
    if bam_skip is not None:
        live &= np.asarray(bam_skip)[bam] == 0
    block = vblk[v][live]; bam = bam[live]; qid = qid[live]; side = (allele[live] != vside[v[live]]).astype(np.int64)
    order = np.lexsort((qid & 0xFFFFFFFF, bam, block))
    block = block[order]; bam = bam[order]; qid = qid[order]; side = side[order]
    n = len(block)
    out = np.zeros(0, dtype=READHAP_DTYPE)
    if n == 0:
        return out
    head = np.ones(n, dtype=bool)
    head[1:] = (block[1:] != block[:-1]) | (bam[1:] != bam[:-1]) | (qid[1:] != qid[:-1])
    at = np.flatnonzero(head)
    out = np.zeros(len(at), dtype=READHAP_DTYPE)
    out["block"] = block[at]; out["bam"] = bam[at]; out["qid"] = qid[at]
    out["b"] = np.add.reduceat(side, at); out["a"] = np.diff(np.append(at, n)) - out["b"]
    return out


def records(eng, _launch=None, table: Optional[dict] = None) -> np.ndarray:
    """The records (READHAP_DTYPE) of the Engine's finished pass through phz_read_haplotypes: the row count first (rows_cap = 0), then the rows.
    _launch(table) replaces the call (CPU tests)."""
    table = block_table(eng) if table is None else table
    if _launch is not None:
        return np.asarray(_launch(table), dtype=READHAP_DTYPE)
    check_resident(eng)
    return call(eng.ctx, table["blk_off"], table["blk_var"], table["blk_hap"], table["var_skip"], table["bam_skip"])


def call(ctx, blk_off, blk_var, blk_hap, var_skip=None, bam_skip=None) -> np.ndarray:
    """phz_read_haplotypes on host arrays with the count-then-fill protocol."""
    blk_off = np.ascontiguousarray(blk_off, dtype=np.int64); blk_var = np.ascontiguousarray(blk_var, dtype=np.int32); blk_hap = np.ascontiguousarray(blk_hap, dtype=np.uint8)
    var_skip = None if var_skip is None else np.ascontiguousarray(var_skip, dtype=np.uint8)
    bam_skip = None if bam_skip is None else np.ascontiguousarray(bam_skip, dtype=np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None
    n_blocks = max(0, len(blk_off) - 1)
    args = (n_blocks, vp(blk_off), vp(blk_var), vp(blk_hap), vp(var_skip), vp(bam_skip))
    n = C.c_int64(0)
    st = ctx.check(ctx.lib.phz_read_haplotypes(ctx.h, *args, None, 0, C.byref(n), _lib.PHZ_HOST), allow=(_lib.PHZ_E_CAPACITY,))
    rows = np.zeros(int(n.value), dtype=READHAP_DTYPE)
    if st == _lib.PHZ_E_CAPACITY:
        ctx.check(ctx.lib.phz_read_haplotypes(ctx.h, *args, C.c_void_p(rows.ctypes.data), len(rows), C.byref(n), _lib.PHZ_HOST))
    return rows[:int(n.value)]


# ---------------------------------------------------------------- text
def _qname_pool(eng, chrom: str):
    """(uint8 blob, int64 offsets [n + 1]) of a chromosome's QNAMEs in id order, from either form the Engine keeps them in (a list of str, or the interner's pool)"""
    names = eng.qnames.get(chrom)
    if names is None:
        raise _lib.PhzError(_lib.PHZ_E_ARG, "read_haplotypes: the Engine has no QNAME table for chromosome %s (hand the names to add_shard / add_shards)" % chrom)
    if isinstance(names, tuple):
        blob, off = names
        blob = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else np.asarray(blob, dtype=np.uint8)
        return blob, np.asarray(off, dtype=np.int64)
    return _pool([x if isinstance(x, bytes) else x.encode() for x in names])


def _numbers(values: np.ndarray, tail: bytes):
    """pool of the distinct values as decimal text + tail, and every value's index into it"""
    uniq, inv = np.unique(values, return_inverse=True)
    return _pool([b"%d" % int(x) + tail for x in uniq.tolist()]) + (inv.astype(np.int64),)


def text(eng, rec: np.ndarray, table: Optional[dict] = None) -> bytes:
    """The bytes of <o>.read_haplotypes.txt for the records of this Engine's pass; row order = record order."""
    rec = np.asarray(rec, dtype=READHAP_DTYPE)
    n = len(rec)
    if n == 0:
        return HEAD
    table = block_table(eng) if table is None else table
    blk = rec["block"].astype(np.int64)
    chrom = table["chrom"][blk].astype(np.int64)
    # the QNAME pools of the chromosomes that have records, one behind the other
    blobs = []; offs = []; first = np.zeros(len(table["chroms"]), dtype=np.int64)
    n_names = 0; n_bytes = 0
    for ci in np.unique(chrom).tolist():
        blob, off = _qname_pool(eng, table["chroms"][ci])
        if int(rec["qid"][chrom == ci].astype(np.int64).max()) >= len(off) - 1 or int(rec["qid"][chrom == ci].min()) < 0:
            raise _lib.PhzError(_lib.PHZ_E_ARG, "read_haplotypes: the QNAME table of chromosome %s is shorter than its template ids" % table["chroms"][ci])
        first[ci] = n_names
        blobs.append(blob); offs.append(off[:-1] + n_bytes)
        n_names += len(off) - 1; n_bytes += int(off[-1])
    qblob = np.concatenate(blobs); qoff = np.concatenate(offs + [np.array([n_bytes], dtype=np.int64)])
    contigs = _pool([c.encode() + b"\t" for c in table["chroms"]])
    bams = _pool([(x if isinstance(x, bytes) else str(x).encode()) + b"\t" for x in eng.bam_names])
    tab = _pool([b"\t"])
    haps = _pool([b"A\n", b"B\n", b"-\n"])
    a = rec["a"].astype(np.int64); b = rec["b"].astype(np.int64)
    which = np.where(a > b, 0, np.where(b > a, 1, 2)).astype(np.int64)
    return HEAD + _gather_rows([contigs + (chrom,), _numbers(table["start"][blk], b"\t"), _numbers(table["stop"][blk], b"\t"), bams + (rec["bam"].astype(np.int64),),
                                (qblob, qoff, first[chrom] + rec["qid"].astype(np.int64)), tab + (np.zeros(n, dtype=np.int64),), _numbers(a, b"\t"), _numbers(b, b"\t"),
                                haps + (which,)], n)
