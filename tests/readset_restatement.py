"""The read sets of the haplotypes (phaser_amd/csrc/phz_rowsdev.hip: k_seg_small, k_seg_big; phz_hap_counts), restated from the per-(variant, allele, BAM)
read lists with dicts, sets and numpy.unique.  The definitions are those of oracle/phasing_oracle.py (Phaser._write_blocks; phaser.py:865-1043, :1048-1125,
:1180-1239); nothing here knows about hash tables, tickets, pieces in LDS or pools -- except the SIZE CLASS of a segment, which is told from its entry count M and
its piece count np by the thresholds mirrored below, and what a segment asks of the table pool.

    read list       rl_qid[rl_start[e] : rl_start[e + 1]], e = (variant * 2 + allele) * n_bams + bam: the QNAME ids of the kept ref / alt lines, in line order
    block table     [(members, alleles)]: the variants of a block in position order and, per member, the allele (0 / 1) haplotype A carries there
    mode 0          per (block, haplotype, BAM): the lists of the haplotype's alleles on the NON-blacklisted members, member after member; every entry is labelled
                    with the number of its QNAME by first appearance (aReads / bReads), the QNAMEs by first appearance are read_ids_a / read_ids_b, their number
                    is aCount / bCount
    mode 1          per (block, haplotype): distinct QNAMEs over ALL members and ALL BAMs (reads_hap_a / reads_hap_b)
    mode 2          per list: distinct QNAMEs and the first-appearance flags (singleton rows of haplotypic_counts.txt, phz_hap_counts)

A segment's pieces are its lists: np = members of the block (blacklisted ones included: they are pieces of length 0 in mode 0), 1 in mode 2."""
import numpy as np

# ---- the mirror of the thresholds compiled into phaser_amd/csrc/phz_rowsdev.hip (SEG_SMALL, SEG_MID, SEG_LDS, PHZ_STAT_N, PHZ_SEG_POOL_BYTES, PHZ_HAP_POOL_BYTES)
SEG_SMALL, SEG_MID, SEG_LDS, STAT_N = 32, 256, 2048, 512
SEG_POOL_BYTES, HAP_POOL_BYTES = 12 << 20, 4 << 20
CLASSES = ("empty", "thread", "wave", "workgroup_lds", "workgroup_pool", "huge_lds", "huge_pool")


def size_class(M, n_pieces):
    """empty: nothing to do; thread: one thread, labels in registers; wave: one wave, 512-slot LDS table; workgroup_lds: one workgroup, 4,096-slot LDS table;
    workgroup_pool: its table in a slice of the pool; huge_*: more than STAT_N pieces, the piece arrays in the pool, the table in LDS or in the pool"""
    if M == 0:
        return "empty"
    if M <= SEG_SMALL:
        return "thread"
    if n_pieces > STAT_N:
        return "huge_lds" if M <= SEG_LDS else "huge_pool"
    if M <= SEG_MID:
        return "wave"
    return "workgroup_lds" if M <= SEG_LDS else "workgroup_pool"


def table_slots(M):
    """slots of the open-addressing table of a segment of M entries: the power of two from 64 that holds 2 M"""
    cap = 64
    while cap < 2 * M:
        cap *= 2
    return cap


def pool_words(M, n_pieces):
    """32-bit words a segment takes from the pool: keys, first positions and ranks of a table beyond the 4,096 LDS slots, two piece arrays of a huge segment"""
    cls = size_class(M, n_pieces)
    return (3 * table_slots(M) if cls in ("workgroup_pool", "huge_pool") else 0) + (2 * (n_pieces + 2) if cls.startswith("huge") else 0)


def pool_capacity_words(nbytes):
    """what a pool reserved with nbytes holds (the library reserves a quarter more than asked, plus 256 bytes)"""
    return (nbytes + nbytes // 4 + 256) // 4


def grown_pool_bytes(nbytes):
    """what the redo loops ask for after a pool reserved with nbytes overflowed: four times what it held"""
    return 4 * 4 * pool_capacity_words(nbytes)


def smallest_overflowing_segment(nbytes):
    """the smallest one-piece segment whose table alone does not fit a pool reserved with nbytes"""
    M = SEG_LDS + 1
    while 3 * table_slots(M) <= pool_capacity_words(nbytes):
        M = table_slots(M) // 2 + 1
    return M


def first_appearance(ids):
    """ids in entry order -> (label of every entry = number of its id by first appearance, distinct ids, flag: the entry is the first of its id)"""
    ids = np.asarray(ids, dtype=np.int64)
    flags = np.zeros(len(ids), dtype=bool)
    if len(ids) == 0:
        return np.zeros(0, np.int64), 0, flags
    uniq, first, inverse = np.unique(ids, return_index=True, return_inverse=True)
    number = np.empty(len(uniq), np.int64)
    number[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    flags[first] = True
    return number[inverse.reshape(-1)], len(uniq), flags


def restate(rl_start, rl_qid, n_bams, blocks, black=frozenset(), excluded=()):
    """blocks: [(members, alleles of haplotype A)]; black: set of blacklisted variants; excluded: BAMs of --haplo_count_bam_exclude (their mode-0 segments are
    still segments -- they are sized and classified -- but give no row).  -> {"mode0": {(block, haplotype, BAM): {...}}, "mode1": {(block, haplotype): {...}},
    "mode2": count per list, "mode2_flags": flag per entry of rl_qid, "segments": {mode: [(key, M, np, class)]}}"""
    rs = np.asarray(rl_start, dtype=np.int64); rq = np.asarray(rl_qid, dtype=np.int64); nb = n_bams
    lst = lambda v, k, b: rq[rs[(v * 2 + k) * nb + b]:rs[(v * 2 + k) * nb + b + 1]]
    out = {"mode0": {}, "mode1": {}, "segments": {0: [], 1: [], 2: []}, "nb": nb, "excluded": tuple(excluded), "blocks": blocks, "black": frozenset(black)}
    for bi, (members, alleles) in enumerate(blocks):
        for h in (0, 1):
            everything = []
            for b in range(nb):
                pieces = [lst(v, a ^ h, b) for v, a in zip(members, alleles) if v not in black]
                entries = np.concatenate(pieces) if pieces else np.zeros(0, np.int64)
                labels, count, flags = first_appearance(entries)
                cut = np.cumsum([0] + [len(p) for p in pieces])
                out["mode0"][(bi, h, b)] = {"entries": entries, "labels": labels, "count": count, "flags": flags, "M": len(entries), "np": len(members),
                                           "piece_labels": [labels[cut[i]:cut[i + 1]] for i in range(len(pieces))], "row": b not in excluded}
                out["segments"][0].append(((bi, h, b), len(entries), len(members), size_class(len(entries), len(members))))
                everything += [lst(v, a ^ h, b) for v, a in zip(members, alleles)]
            whole = np.concatenate(everything) if everything else np.zeros(0, np.int64)
            out["mode1"][(bi, h)] = {"count": len(set(whole.tolist())), "M": len(whole), "np": len(members)}
            out["segments"][1].append(((bi, h), len(whole), len(members), size_class(len(whole), len(members))))
    nseg = len(rs) - 1
    counts = np.zeros(nseg, np.int32); flags2 = np.zeros(len(rq), dtype=bool)
    sizes = np.diff(rs)
    for e in np.flatnonzero(sizes).tolist():
        _, counts[e], flags2[rs[e]:rs[e + 1]] = first_appearance(rq[rs[e]:rs[e + 1]])
    out["mode2"] = counts; out["mode2_flags"] = flags2; out["_lists"] = (rs, rq, flags2)
    out["segments"][2] = [(e, int(sizes[e]), 1, size_class(int(sizes[e]), 1)) for e in range(nseg)]
    return out


def class_table(r, modes=(0, 1, 2)):
    """{mode: {class: segments}}"""
    return {m: {c: sum(1 for s in r["segments"][m] if s[3] == c) for c in CLASSES} for m in modes}


def big_segments(r, modes):
    """segments left to the wave / workgroup / huge kernels (more than SEG_SMALL entries), over the modes that ran"""
    return sum(1 for m in modes for s in r["segments"][m] if s[1] > SEG_SMALL)


def pool_overflows(r, modes, nbytes):
    """does some mode ask more of a pool reserved with nbytes than it holds (every mode starts at the pool's beginning)"""
    return any(sum(pool_words(s[1], s[2]) for s in r["segments"][m]) > pool_capacity_words(nbytes) for m in modes)


# ------------------------------------------------------------------------------------------------ the read-set columns of the two files
def expected_columns(r, variants, bam_names, qname_of=None, unphased_vars=1, sorted_ids=False):
    """What the restatement says the read-set columns hold.  variants: per variant {"uid", "chrom", "name" (its entry in variant_ids)}; qname_of(variant, id) ->
    QNAME text (None: no --output_read_ids columns).  -> (counts rows, haplotypes rows):
      counts rows      {(variants column, BAM name): (aCount, bCount, aReads, bReads[, read_ids_a, read_ids_b])}, blocks and singletons
      haplotypes rows  {(contig, variant_ids column): (reads_hap_a, reads_hap_b)}, blocks only
    sorted_ids: the QNAME lists sorted (the canonical form of a file whose lists are in set order)"""
    nb = r["nb"]; black = r["black"]
    ids_text = lambda names: ",".join(sorted(names) if sorted_ids else names)
    ase = {}; hap = {}
    in_block = set()
    for bi, (members, alleles) in enumerate(r["blocks"]):
        in_block.update(members)
        hap[(variants[members[0]]["chrom"], ",".join(variants[v]["name"] for v in members))] = (str(r["mode1"][(bi, 0)]["count"]), str(r["mode1"][(bi, 1)]["count"]))
        used = [v for v in members if v not in black]
        for b in range(nb):
            A = r["mode0"][(bi, 0, b)]; B = r["mode0"][(bi, 1, b)]
            if b in r["excluded"] or A["count"] + B["count"] == 0:
                continue
            row = [str(A["count"]), str(B["count"])] + [";".join(",".join(str(x) for x in p.tolist()) for p in S["piece_labels"]) for S in (A, B)]
            if qname_of is not None:
                row += [ids_text([qname_of(members[0], q) for q in S["entries"][S["flags"]].tolist()]) for S in (A, B)]
            ase[(",".join(variants[v]["uid"] for v in used), bam_names[b])] = tuple(row)
    if unphased_vars == 1:
        for v in range(len(variants)):
            if v in in_block or v in black:
                continue
            for b in range(nb):
                if b in r["excluded"]:
                    continue
                ea = (v * 2) * nb + b; eb = (v * 2 + 1) * nb + b
                if r["mode2"][ea] + r["mode2"][eb] == 0:
                    continue
                row = [str(r["mode2"][ea]), str(r["mode2"][eb]), "", ""]
                if qname_of is not None:
                    rs, rq, fl = r["_lists"]
                    row += [ids_text([qname_of(v, q) for q in rq[rs[e]:rs[e + 1]][fl[rs[e]:rs[e + 1]]].tolist()]) for e in (ea, eb)]
                ase[(variants[v]["uid"], bam_names[b])] = tuple(row)
    return ase, hap


def file_columns(counts_text, haplotypes_text):
    """the same two dicts from the text of haplotypic_counts.txt and haplotypes.txt"""
    ase = {}; hap = {}
    rows = counts_text.split("\n")
    ids = len(rows[0].split("\t")) == 20
    for line in rows[1:]:
        if line:
            f = line.split("\t")
            key = (f[3], f[-3])
            assert key not in ase, key
            ase[key] = (f[9], f[10], f[-2], f[-1]) + ((f[14], f[15]) if ids else ())
    for line in haplotypes_text.split("\n")[1:]:
        if line:
            f = line.split("\t")
            if int(f[4]) > 1:
                assert (f[0], f[5]) not in hap, f[5]
                hap[(f[0], f[5])] = (f[7], f[8])
    return ase, hap


def blocks_of_file(haplotypes_text, index_of, alleles_of):
    """the block table a haplotypes.txt states: index_of(contig, entry of variant_ids) -> variant, alleles_of(variant) -> its two allele texts"""
    blocks = []
    for line in haplotypes_text.split("\n")[1:]:
        if line:
            f = line.split("\t")
            if int(f[4]) > 1:
                members = [index_of(f[0], x) for x in f[5].split(",")]
                a_side = f[6].split("|")[0].split(",")
                assert len(members) == len(a_side) == int(f[4])
                blocks.append((members, [list(alleles_of(v)).index(a) for v, a in zip(members, a_side)]))
    return blocks
