"""Plain Python / numpy restatement of --output_haplotag_bam, written from the rule and not from the kernels: what phz_haplotag_pick and phz_bamdev_haplotag
must give.

The rule: one tag per (BAM, chromosome, template id).  Only the rows of this BAM in phased blocks (block < n_phased) vote.  Among a template's rows the block with the
largest a + b wins, the smallest block index among equal totals.  a > b: HP 1, b > a: HP 2, a == b in the winning block: no tag, and the template does not fall through
to its next block.  PS = the winning block's start.  A tagged record = the input record + HP:C + PS:I, its block_size raised by 11; every other kept record is copied."""
import struct

import numpy as np

from phaser_amd import bamio


def pick(rows, n_phased, bam, blk_chrom, tmpl_base, n_templates):
    """rows: records with fields block, bam, qid, a, b (any order).  -> uint32 [n_templates]: 0 = no vote, else (block + 1) << 2 | hp, hp 0 = the winning block tied."""
    tag = np.zeros(n_templates, dtype=np.uint32)
    best = {}
    for r in rows:
        block, b_, qid, a, b = int(r["block"]), int(r["bam"]), int(r["qid"]), int(r["a"]), int(r["b"])
        if b_ != bam or block >= n_phased:
            continue
        slot = int(tmpl_base[int(blk_chrom[block])]) + qid
        cur = best.get(slot)
        if cur is None or a + b > cur[0] or (a + b == cur[0] and block < cur[1]):
            best[slot] = (a + b, block, a, b)
    for slot, (_total, block, a, b) in best.items():
        tag[slot] = ((block + 1) << 2) | (1 if a > b else 2 if b > a else 0)
    return tag


def kept(ref_name, mq, flag, tlen, filters, chroms):
    """the filters of the run: what samtools would pass on (bamio.shards_from_bam)"""
    if ref_name is None or (chroms is not None and ref_name not in chroms):
        return False
    if mq < filters["mapq"] or (filters.get("remove_dups", True) and (flag & 0x400)) or (filters.get("paired_end", True) and not (flag & 0x2)):
        return False
    isz = filters.get("isize", 0)
    return isz == 0 or abs(tlen) <= isz


def tag_stream(bam_bytes, filters, chroms, qid_of_name, tag, blk_ps):
    """bam_bytes: an uncompressed BAM.  qid_of_name[chrom][QNAME] = chromosome-local template id, tag[chrom] = that chromosome's tag words, blk_ps[block] = PS.
    -> the record bytes the output must hold behind the header."""
    refs, off = bamio.parse_header(bam_bytes)
    out = bytearray()
    for ref_id, _pos, mq, flag, tlen, qname, _cigar, _l_seq, _seq, _qual, _aux in bamio.iter_records(bam_bytes, off):
        bs, = struct.unpack_from("<i", bam_bytes, off)
        raw = bam_bytes[off:off + 4 + bs]
        off += 4 + bs
        name = refs[ref_id][0] if 0 <= ref_id < len(refs) else None
        if not kept(name, mq, flag, tlen, filters, chroms):
            continue
        t = int(tag[name][qid_of_name[name][qname]])
        if t & 3:
            out += struct.pack("<i", bs + 11) + raw[4:] + b"HPC" + bytes([t & 3]) + b"PSI" + struct.pack("<I", int(blk_ps[(t >> 2) - 1]))
        else:
            out += raw
    return bytes(out)


def read_tags(bam_bytes):
    """[(reference name, QNAME, HP or None, PS or None)] of every record of an uncompressed BAM, from its aux fields"""
    refs, off = bamio.parse_header(bam_bytes)
    out = []
    for ref_id, _pos, _mq, _flag, _tlen, qname, _cigar, _l_seq, _seq, _qual, aux in bamio.iter_records(bam_bytes, off):
        hp = ps = None
        p = 0
        while p + 3 <= len(aux):
            key = aux[p:p + 2]; ty = chr(aux[p + 2]); p += 3
            if ty in "ZH":
                p = aux.index(b"\0", p) + 1
            elif ty == "B":
                p += 5 + struct.unpack_from("<i", aux, p + 1)[0] * {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[chr(aux[p])]
            else:
                size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[ty]
                if key == b"HP":
                    assert ty == "C"; hp = aux[p]
                if key == b"PS":
                    assert ty == "I"; ps = struct.unpack_from("<I", aux, p)[0]
                p += size
        assert p == len(aux)
        out.append((refs[ref_id][0] if ref_id >= 0 else None, qname, hp, ps))
    return out


def tags_from_text(text, bam_name, phased):
    """(contig, QNAME) -> (HP, PS) of one BAM by the rule, from the bytes of <o>.read_haplotypes.txt alone.  Its rows come in block order, so the first of equal totals
    is the smallest block index.  phased(contig, start, stop) says whether a row's block is a phased one (the one-variant blocks of --unphased_vars never tag)."""
    best = {}
    for line in text.split(b"\n")[1:]:
        if not line:
            continue
        contig, start, stop, bam, read, a, b, _h = line.decode().split("\t")
        if bam != bam_name or not phased(contig, int(start), int(stop)):
            continue
        a = int(a); b = int(b)
        cur = best.get((contig, read))
        if cur is None or a + b > cur[0]:
            best[(contig, read)] = (a + b, 1 if a > b else 2 if b > a else 0, int(start))
    return {k: (hp, ps) for k, (_t, hp, ps) in best.items() if hp}
