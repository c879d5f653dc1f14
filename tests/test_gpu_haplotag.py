"""--output_haplotag_bam on the GPU: phz_haplotag_pick (K_tagpick) and phz_bamdev_haplotag (K_tagsize, K_tagwrite) against the plain Python restatement of
tests/haplotag_restatement.py, and the command line on the cli_inputs fixture."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest
import torch

from haplotag_restatement import kept, pick, read_tags, tag_stream, tags_from_text
from helpers import OUTPUTS
from test_gpu_network import cli_inputs          # noqa: F401  (fixture: pipe_one as an unfiltered BAM + gzipped VCF)

pytestmark = pytest.mark.gpu

REC = np.dtype([("block", "<i4"), ("bam", "<i4"), ("qid", "<i4"), ("a", "<i4"), ("b", "<i4")])
CANARY = 0xA5A5A5A5
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def ctx():
    from phaser_amd import _lib
    return _lib.Context(0)


# ------------------------------------------------------------------------------------------------ 1. K_tagpick
N_BLOCKS, N_PHASED = 300, 250
TMPL_BASE = np.array([0, 2000, 2500, 4000], np.int64)          # three chromosomes; no block lies on the middle one, so it has no rows
BLK_CHROM = np.where(np.arange(N_BLOCKS) < 150, 0, 2).astype(np.int32)


@pytest.fixture(scope="module")
def pick_rows():
    """~5,000 distinct (block, bam, qid) rows over 300 blocks (250 phased), 2 BAMs, chromosomes 0 and 2: more than one workgroup of 256.  Templates 0-9 of chromosome
    0 and the last template of chromosome 2 are built in; the 64 rows of template 6 come first, so one whole wave contends for one slot."""
    rng = np.random.default_rng(77)
    built = [(k, 0, 6, 1 if k == 0 else 3, 3 if k == 0 else 1) for k in range(64)]          # 64 blocks, equal totals: block 0 wins, and there b > a
    built += [(0, 0, 0, 3, 1),                                        # the template whose id is 0
              (5, 0, 1, 2, 1), (9, 0, 1, 1, 5),                        # two blocks with different totals
              (8, 0, 2, 0, 3), (7, 0, 2, 2, 1), (30, 0, 2, 3, 0),     # equal totals: the smallest block index
              (3, 0, 3, 2, 2), (4, 0, 3, 3, 0),                        # the winning block tied; the loser is decisive
              (N_PHASED, 0, 4, 9, 0), (N_BLOCKS - 1, 0, 4, 0, 9),      # only blocks behind n_phased
              (2, 1, 5, 9, 0),                                         # only rows of the other BAM
              (299 - 60, 0, 1499, 0, 2)]                               # the last template of the last chromosome: the last slot of tag
    seen = {(r[0], r[1], r[2]) for r in built}
    rows = list(built)
    while len(rows) < 5000:
        block = int(rng.integers(0, N_BLOCKS)); c = int(BLK_CHROM[block])
        qid = int(rng.integers(10, 1499 if c == 2 else 2000))
        key = (block, int(rng.integers(0, 2)), qid)
        if key in seen:
            continue
        seen.add(key)
        a = int(rng.integers(0, 4)); b = int(rng.integers(0 if a else 1, 4))
        rows.append(key + (a, b))
    head, rest = rows[:64], sorted(rows[64:])
    return np.array(head + rest, dtype=REC)


def gpu_pick(ctx, rows, bam, device, n_blocks=N_BLOCKS, n_phased=N_PHASED):
    """-> (status, tag words); the word behind tag must keep its canary"""
    from phaser_amd import _lib
    n_t = int(TMPL_BASE[-1])
    tag = np.full(n_t + 1, CANARY, dtype=np.uint32)
    host = [np.ascontiguousarray(rows), BLK_CHROM, TMPL_BASE, tag]
    if device:
        dev = [torch.from_numpy(a.view(np.uint8)).cuda() for a in host]
        torch.cuda.synchronize()
        p = [C.c_void_p(t.data_ptr()) if t.numel() else None for t in dev]
    else:
        p = [C.c_void_p(a.ctypes.data) if a.size else None for a in host]
    st = ctx.lib.phz_haplotag_pick(ctx.h, p[0], len(rows), n_blocks, n_phased, bam, p[1], 3, p[2], n_t, p[3], _lib.PHZ_DEVICE if device else _lib.PHZ_HOST)
    if device:
        tag = dev[3].cpu().numpy().view(np.uint32)
    assert tag[n_t] == CANARY
    return st, tag[:n_t]


@pytest.mark.parametrize("device", [False, True], ids=["host_args", "device_args"])
def test_pick_equals_the_restatement(ctx, pick_rows, device):
    word = lambda block, hp: ((block + 1) << 2) | hp
    for bam in (0, 1):
        want = pick(pick_rows, N_PHASED, bam, BLK_CHROM, TMPL_BASE, int(TMPL_BASE[-1]))
        st, got = gpu_pick(ctx, pick_rows, bam, device)
        assert st == 0 and got.tolist() == want.tolist()
        assert not want[2000:2500].any() and int((want != 0).sum()) > 1000          # the chromosome without rows; the others are populated
        if bam == 0:
            assert [int(want[q]) for q in range(7)] == [word(0, 1), word(9, 2), word(7, 1), word(3, 0), 0, 0, word(0, 2)]
            assert int(want[3999]) == word(239, 2)
        else:
            assert int(want[5]) == word(2, 1)
    st, got = gpu_pick(ctx, pick_rows[:0], 0, device)
    assert st == 0 and not got.any()                                                  # n_rows == 0: all zeros, no error


@pytest.mark.parametrize("device", [False, True], ids=["host_args", "device_args"])
def test_pick_refuses_bad_rows_and_goes_on(ctx, pick_rows, device):
    from phaser_amd import _lib
    want = pick(pick_rows, N_PHASED, 0, BLK_CHROM, TMPL_BASE, int(TMPL_BASE[-1])).tolist()

    def bad(i, field, value, n_blocks=N_BLOCKS):
        rows = pick_rows.copy()
        rows[field][i] = value
        st, _ = gpu_pick(ctx, rows, 0, device, n_blocks=n_blocks)
        msg = ctx.lib.phz_last_error(ctx.h).decode()
        ok_st, ok = gpu_pick(ctx, pick_rows, 0, device)                               # a good call on the same ctx
        assert ok_st == 0 and ok.tolist() == want
        return st, msg

    for value in (N_BLOCKS, -1):
        st, msg = bad(700, "block", value)
        assert st == _lib.PHZ_E_ARG and "block is outside" in msg
    i0 = int(np.flatnonzero(BLK_CHROM[pick_rows["block"]] == 0)[500]); i2 = int(np.flatnonzero(BLK_CHROM[pick_rows["block"]] == 2)[5])
    for i, value in ((i0, 2000), (i2, 1500), (i2, -1)):          # one past the chromosome's ids: for the last chromosome that is one past tag, too
        st, msg = bad(i, "qid", value)
        assert st == _lib.PHZ_E_ARG and "qid is outside" in msg
    held = [np.ascontiguousarray(pick_rows[:8]), BLK_CHROM, np.zeros(4, np.int64)]          # rows, and no template at all
    if device:
        held = [torch.from_numpy(a.view(np.uint8)).cuda() for a in held]
        torch.cuda.synchronize()
    p = [C.c_void_p(a.data_ptr() if device else a.ctypes.data) for a in held]
    st = ctx.lib.phz_haplotag_pick(ctx.h, p[0], 8, N_BLOCKS, N_PHASED, 0, p[1], 3, p[2], 0, None, int(device))
    assert st == _lib.PHZ_E_ARG and "qid is outside" in ctx.lib.phz_last_error(ctx.h).decode()
    st, _ = gpu_pick(ctx, pick_rows, 0, device, n_blocks=1 << 30, n_phased=N_PHASED)
    assert st == _lib.PHZ_E_ARG and "2^30" in ctx.lib.phz_last_error(ctx.h).decode()
    ok_st, ok = gpu_pick(ctx, pick_rows, 0, device)
    assert ok_st == 0 and ok.tolist() == want


# ------------------------------------------------------------------------------------------------ 2. K_tagsize + K_tagwrite
REFS = [("rA", 100000), ("rLow", 100000), ("rB", 100000), ("rNone", 100000)]
FILTERS = dict(mapq=30, remove_dups=True, paired_end=True, isize=0)
Z_AND_B = b"RGZgroup\0" + b"ZBBS" + np.array([3], "<i4").tobytes() + np.array([7, 8, 9], "<u2").tobytes() + b"XAA!"


def designed_records(extra=None):
    """Two references with kept and dropped records interleaved, one whose records all fail --mapq, one without records.  The kinds cycle: no aux; AS:i alone; a Z and
    a B array aux; SEQ '*' (l_seq 0); QNAMEs of 1 and 254 characters; 0 and 40 CIGAR ops.  Mates share names; QNAME lengths run through every residue."""
    recs = []
    for ref_id in (0, 1, 2):
        for i in range(330):
            t = i // 2
            name = "q" * (1 + t % 7) + "%d" % t
            kind = i % 6
            r = dict(ref_id=ref_id, pos=100 + 3 * i, mapq=60, flag=0x63 if i % 2 == 0 else 0x93, tlen=150, qname=name, cigar=[(0, 10)], seq="ACGTACGTAC", qual=[30] * 10, tags={})
            if kind == 1:
                r["tags"] = {"AS": -5 - i}
            elif kind == 2:
                r["aux_raw"] = Z_AND_B
            elif kind == 3:
                r.update(seq="", qual=None, cigar=[])
            elif kind == 4:
                r.update(cigar=[(0, 1), (1, 1)] * 20, seq="ACGT" * 10, qual=[20] * 40, tags={"AS": 11})
            if i % 5 == 3 or ref_id == 1:
                r["mapq"] = 10                                   # fails --mapq 30
            if i in (40, 41):
                r["qname"] = "L" * 254
            if i in (60, 61):
                r["qname"] = "S"
            recs.append(r)
    for r in (extra or []):
        recs.append(r)
    recs.sort(key=lambda r: (r["ref_id"], r["pos"]))
    return recs


def designed_bam(tmp_path, name, extra=None):
    from phaser_amd import bamio
    path = str(tmp_path / name)
    bamio.write_bam(path, REFS, designed_records(extra), member_bytes=3001)          # ~70 members: most of them start inside a record
    return path, gzip.open(path, "rb").read()


def kept_names(raw):
    """{reference: QNAMEs of its kept records in file order}"""
    from phaser_amd import bamio
    refs, off = bamio.parse_header(raw)
    out = {}
    for ref_id, _pos, mq, flag, tlen, qname, *_ in bamio.iter_records(raw, off):
        if kept(refs[ref_id][0], mq, flag, tlen, FILTERS, None):
            out.setdefault(refs[ref_id][0], []).append(qname)
    return out


def tag_tables(names):
    """ids in first-appearance order, and tag words that tag the first and the last kept record of every reference and mix all four kinds behind them"""
    rng = np.random.default_rng(5)
    blk_ps = np.array([1, 70000, 4_000_000_000, 12345], np.uint32)
    qid_of, tag = {}, {}
    for ref, lst in names.items():
        ids = {}
        for q in lst:
            ids.setdefault(q, len(ids))
        words = np.zeros(len(ids) + 3, np.uint32)                                     # (three ids nobody uses behind them)
        for q, i in ids.items():
            kind = int(rng.integers(0, 4))
            words[i] = 0 if kind == 0 else ((int(rng.integers(0, 4)) + 1) << 2) | (kind - 1)
        words[ids[lst[0]]] = (3 << 2) | 1; words[ids[lst[-1]]] = (1 << 2) | 2
        qid_of[ref] = ids; tag[ref] = words
    return qid_of, tag, blk_ps


def haplotag_call(packed, ref, qid, tag, blk_ps, cap=None, n_tag=None):
    """-> (status, out_bytes, n_tagged, the buffer with 16 canary bytes behind cap); cap None: the count call with out == NULL"""
    lib = packed.lib
    nbytes = C.c_int64(-1); ntag = C.c_int64(-1)
    p = lambda t: C.c_void_p(t.data_ptr())
    if cap is None:
        st = lib.phz_bamdev_haplotag(packed.h, ref, p(qid), p(tag), len(tag) if n_tag is None else n_tag, p(blk_ps), len(blk_ps), None, 0, C.byref(nbytes), C.byref(ntag))
        return st, nbytes.value, ntag.value, None
    out = torch.full((cap + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = lib.phz_bamdev_haplotag(packed.h, ref, p(qid), p(tag), len(tag) if n_tag is None else n_tag, p(blk_ps), len(blk_ps), p(out), cap, C.byref(nbytes), C.byref(ntag))
    return st, nbytes.value, ntag.value, out.cpu().numpy()


def device_tables(packed, names, qid_of, tag, blk_ps):
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
    per_ref = {}
    for ref, name, n, _qn, _qo in packed.refs:
        assert n == len(names[name])
        per_ref[name] = (ref, up(np.array([qid_of[name][q] for q in names[name]], np.int32), np.int32), up(tag[name], np.int32))
    d_ps = up(blk_ps, np.int32)
    torch.cuda.synchronize()
    return per_ref, d_ps


def open_designed(ctx, path):
    from phaser_amd import bamio
    packed, why = bamio.open_packed_bam_device(ctx, path, FILTERS["mapq"], True, True, 0.0, chroms=[r[0] for r in REFS])
    assert packed is not None, why
    return packed


def test_writer_equals_the_restatement_byte_for_byte(ctx, tmp_path):
    from phaser_amd import _lib, bamio
    path, raw = designed_bam(tmp_path, "designed.bam")
    names = kept_names(raw)
    assert set(names) == {"rA", "rB"} and all(len(v) > 256 for v in names.values())          # rLow: all filtered; rNone: no records; more than one workgroup
    qid_of, tag, blk_ps = tag_tables(names)
    with open_designed(ctx, path) as packed:
        assert [r[1] for r in packed.refs] == ["rA", "rB"]
        per_ref, d_ps = device_tables(packed, names, qid_of, tag, blk_ps)
        sizes = set()
        for name in ("rA", "rB"):
            ref, d_qid, d_tag = per_ref[name]
            want = tag_stream(raw, FILTERS, {name}, qid_of, tag, blk_ps)
            tags = read_tags(raw[:bamio.parse_header(raw)[1]] + want)
            n_tagged = sum(1 for t in tags if t[2] is not None)
            assert tags[0][2] == 1 and tags[-1][2] == 2 and 0 < n_tagged < len(tags)          # the first and the last kept record are tagged
            p = 0
            while p < len(want):
                size = 4 + int(np.frombuffer(want, "<i4", 1, p)[0]); sizes.add((size % 4, p % 4)); p += size
            st, nbytes, ntag, _ = haplotag_call(packed, ref, d_qid, d_tag, d_ps)
            assert (st, nbytes, ntag) == (_lib.PHZ_E_CAPACITY, len(want), n_tagged)
            st, nbytes, ntag, out = haplotag_call(packed, ref, d_qid, d_tag, d_ps, cap=len(want) - 1)          # one byte short: nothing written
            assert (st, nbytes) == (_lib.PHZ_E_CAPACITY, len(want)) and np.all(out == 0xA5)
            st, nbytes, ntag, out = haplotag_call(packed, ref, d_qid, d_tag, d_ps, cap=len(want))              # the handle still serves the exact fill
            assert (st, nbytes, ntag) == (0, len(want), n_tagged)
            assert out[:len(want)].tobytes() == want and np.all(out[len(want):] == 0xA5)
        assert {s for s, _ in sizes} == {0, 1, 2, 3} and {a for _, a in sizes} == {0, 1, 2, 3}                  # every record size and every start, mod 4
        # the references without kept records: 0 bytes, no error
        for ref in (1, 3):
            assert haplotag_call(packed, ref, per_ref["rA"][1], per_ref["rA"][2], d_ps)[:3] == (0, 0, 0)
        # a qid outside the tag slice is an argument error, and the handle goes on
        ref, d_qid, d_tag = per_ref["rA"]
        st, _, _, _ = haplotag_call(packed, ref, d_qid, d_tag, d_ps, n_tag=max(qid_of["rA"].values()))
        assert st == _lib.PHZ_E_ARG and "qid outside" in packed.lib.phz_last_error(ctx.h).decode()
        assert haplotag_call(packed, ref, d_qid, d_tag, d_ps)[0] == _lib.PHZ_E_CAPACITY


@pytest.mark.parametrize("aux,why", [(b"HPC\x01", "already carries HP or PS"), (b"NHi\x01\0\0\0PSi\x05\0\0\0", "already carries HP or PS"),
                                     (b"XYZunterminated", "do not end at its block_size"), (b"XQi\x01\0", "do not end at its block_size")],
                         ids=["HP:C", "PS:i", "Z_without_NUL", "short_i"])
def test_writer_refuses_records_it_cannot_extend(ctx, tmp_path, aux, why):
    from phaser_amd import _lib, bamio
    odd = dict(ref_id=0, pos=500, mapq=60, flag=0x63, tlen=150, qname="odd", cigar=[(0, 10)], seq="ACGTACGTAC", qual=[30] * 10, tags={}, aux_raw=aux)
    path, raw = designed_bam(tmp_path, "refused.bam", extra=[odd])
    names = kept_names(raw)
    qid_of, tag, blk_ps = tag_tables(names)
    refs, off0 = bamio.parse_header(raw)
    at = raw.index(b"odd\0") - 36                                                     # the record's block_size word
    with open_designed(ctx, path) as packed:
        per_ref, d_ps = device_tables(packed, names, qid_of, tag, blk_ps)
        ref, d_qid, d_tag = per_ref["rA"]
        st, nbytes, _, _ = haplotag_call(packed, ref, d_qid, d_tag, d_ps)
        msg = packed.lib.phz_last_error(ctx.h).decode()
        assert st == _lib.PHZ_E_UNSUPPORTED and why in msg and ("offset %d " % at) in msg, msg
        ref, d_qid, d_tag = per_ref["rB"]                                             # the handle still serves a good call
        want = tag_stream(raw, FILTERS, {"rB"}, qid_of, tag, blk_ps)
        st, nbytes, _, out = haplotag_call(packed, ref, d_qid, d_tag, d_ps, cap=len(want))
        assert st == 0 and out[:len(want)].tobytes() == want


# ------------------------------------------------------------------------------------------------ 3. the command line
def run_cli(cli_inputs, tag, *extra):          # noqa: F811
    from phaser_amd import phaser
    tmp, bam, vcfgz = cli_inputs
    prefix = str(tmp / tag)
    rc = phaser.main(["--vcf", vcfgz, "--bam", bam, "--sample", "S1", "--mapq", "255", "--baseq", "10", "--paired_end", "1", "--o", prefix, "--write_vcf", "0", "--threads", "3"]
                     + list(extra))
    return rc, prefix


@pytest.fixture(scope="module")
def cli_runs(cli_inputs):          # noqa: F811
    runs = {}
    for tag, extra in (("plain", ()), ("both", ("--output_haplotag_bam", "1", "--output_read_haplotypes", "1")), ("tag_only", ("--output_haplotag_bam", "1")),
                       ("text_only", ("--output_read_haplotypes", "1"))):
        rc, prefix = run_cli(cli_inputs, "ht_" + tag, *extra)
        assert rc == 0
        runs[tag] = prefix
    return runs


def expected_from_text(cli_inputs, prefix_text):          # noqa: F811
    """-> (header, expected record stream, {(contig, QNAME): (HP, PS)}) of the one input BAM, from <o>.read_haplotypes.txt and <o>.haplotypes.txt by the rule"""
    from phaser_amd import bamio
    tmp, bam, vcfgz = cli_inputs
    raw = gzip.open(bam, "rb").read()
    refs, off = bamio.parse_header(raw)
    blocks = set()
    for line in open(prefix_text + ".haplotypes.txt").read().split("\n")[1:]:
        c = line.split("\t")
        if len(c) > 4 and int(c[4]) > 1:
            blocks.add((c[0], int(c[1]), int(c[2])))
    want_tags = tags_from_text(open(prefix_text + ".read_haplotypes.txt", "rb").read(), "a", lambda c, s, e: (c, s, e) in blocks)
    chroms = {l.split("\t")[0] for l in gzip.open(vcfgz, "rt").read().split("\n") if l and not l.startswith("#")}
    filters = dict(mapq=255, remove_dups=True, paired_end=True, isize=0)
    qid_of, tag, blk_ps = {}, {}, []
    for ref_id, _pos, mq, flag, tlen, qname, *_ in bamio.iter_records(raw, off):
        name = refs[ref_id][0] if ref_id >= 0 else None
        if kept(name, mq, flag, tlen, filters, chroms):
            qid_of.setdefault(name, {}).setdefault(qname, len(qid_of[name]))
    for name, ids in qid_of.items():
        tag[name] = np.zeros(len(ids), np.uint32)
        for q, i in ids.items():
            if (name, q) in want_tags:
                hp, ps = want_tags[(name, q)]
                blk_ps.append(ps); tag[name][i] = (len(blk_ps) << 2) | hp
    return raw[:off], tag_stream(raw, filters, chroms, qid_of, tag, blk_ps), want_tags


@pytest.mark.parametrize("which", ["both", "tag_only"])
def test_cli_writes_the_haplotagged_bam(cli_inputs, cli_runs, which):          # noqa: F811
    header, want, want_tags = expected_from_text(cli_inputs, cli_runs["both" if which == "both" else "text_only"])
    data = open(cli_runs[which] + ".haplotag.1.bam", "rb").read()
    assert data[-28:] == EOF
    got = gzip.decompress(data)
    assert got == header + want
    tags = read_tags(got)
    by_name = {}
    for ref, qname, hp, ps in tags:
        assert by_name.setdefault((ref, qname), (hp, ps)) == (hp, ps)                # both mates carry the same tag
    assert {k: v for k, v in by_name.items() if v[0] is not None} == want_tags
    hps = [v[0] for v in by_name.values()]
    assert hps.count(1) > 0 and hps.count(2) > 0 and hps.count(None) > 0           # an empty result cannot pass
    assert all((hp is None) == (ps is None) for _, _, hp, ps in tags)
    for name in OUTPUTS:                                                             # the five standard outputs do not change
        assert open(cli_runs[which] + "." + name + ".txt", "rb").read() == open(cli_runs["plain"] + "." + name + ".txt", "rb").read(), name
    assert not os.path.exists(cli_runs["plain"] + ".haplotag.1.bam") and not os.path.exists(cli_runs["text_only"] + ".haplotag.1.bam")


def test_engine_haplotag_with_the_names_in_either_home(cli_inputs, cli_runs, ctx):          # noqa: F811
    """Engine.haplotag in process: first with the QNAMEs still in the interner's device store, then after they have moved to the host table for good
    (NativeInterner.h drops the store) -- the same file both times, the one the command line wrote."""
    from phaser_amd import bamio, vcf
    from phaser_amd.engine import Config, Engine
    from phaser_amd.mapper import Mapper
    tmp, bam, vcfgz = cli_inputs
    mapper = Mapper(0)
    vs = vcf.load_variants(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipe_one", "in.vcf")).read())
    its = {}
    shards = bamio.shards_from_bam_device(mapper.ctx, bam, its, 255, True, True, 0.0, chroms=set(vs.chroms), device="cuda:0")
    assert shards is not None and all(it._store is not None for it in its.values())
    eng = Engine(vs, ["a"], Config(want_vcf=True), mapper=mapper)
    eng.add_shards(0, [(c, shards[c].to("cuda:0"), len(its[c]), None) for c in vs.chroms if c in shards])
    for c in its:
        eng.n_qid[c] = len(its[c])
    eng.close_bam(0)
    eng.finish()
    want = gzip.decompress(open(cli_runs["tag_only"] + ".haplotag.1.bam", "rb").read())
    sizes = {c: len(it) for c, it in its.items()}
    for home in ("device_store", "host_table"):
        if home == "host_table":
            for it in its.values():
                assert it.h is not None and it._store is None
        out = str(tmp / ("engine_%s.bam" % home))
        res = eng.haplotag(0, bam, out, its, 255, True, True, 0.0, threads=2)
        assert gzip.decompress(open(out, "rb").read()) == want
        assert res["records"] == len(read_tags(want)) and res["tagged"] == sum(1 for t in read_tags(want) if t[2] is not None) and res["bytes"] == len(want)
        assert {c: len(it) for c, it in its.items()} == sizes                         # no new name
    # a record whose name the run never saw: refused, and the interner is not what says so silently
    from phaser_amd import _lib
    with pytest.raises(_lib.PhzError, match="had not seen"):
        eng.haplotag(0, bam, str(tmp / "engine_mapq0.bam"), its, 0, True, True, 0.0)


def test_cli_skips_a_bam_that_already_carries_hp(cli_inputs, cli_runs, capsys):          # noqa: F811
    """the first kept record of the input gets an HP:C field: the record rewrite refuses the file, the run says so and writes everything else"""
    import struct
    from phaser_amd import _lib, bamio, phaser
    tmp, bam, vcfgz = cli_inputs
    raw = gzip.open(bam, "rb").read()
    refs, off = bamio.parse_header(raw)
    filters = dict(mapq=255, remove_dups=True, paired_end=True, isize=0)
    for ref_id, _pos, mq, flag, tlen, *_ in bamio.iter_records(raw, off):
        bs, = struct.unpack_from("<i", raw, off)
        if kept(refs[ref_id][0], mq, flag, tlen, filters, {"chr22"}):
            break
        off += 4 + bs
    data = raw[:off] + struct.pack("<i", bs + 4) + raw[off + 4:off + 4 + bs] + b"HPC\x01" + raw[off + 4 + bs:]
    tagged_in = str(tmp / "carries_hp.bam")
    assert _lib.load().phz_bgzf_write(tagged_in.encode(), data, len(data), 2, 1) == 0
    prefix = str(tmp / "ht_carries")
    rc = phaser.main(["--vcf", vcfgz, "--bam", tagged_in, "--sample", "S1", "--mapq", "255", "--baseq", "10", "--paired_end", "1", "--o", prefix, "--write_vcf", "0",
                      "--threads", "3", "--output_haplotag_bam", "1"])
    text = capsys.readouterr().out
    assert rc == 0 and "no haplotagged BAM for" in text and "already carries HP or PS" in text and not os.path.exists(prefix + ".haplotag.1.bam")
    for name in ("haplotypes", "variant_connections", "allelic_counts"):             # (haplotypic_counts names the BAM, which has another name here)
        assert open(prefix + "." + name + ".txt", "rb").read() == open(cli_runs["plain"] + "." + name + ".txt", "rb").read(), name


def test_cli_skips_a_bam_the_host_decoder_read(cli_inputs, monkeypatch, capsys):          # noqa: F811
    monkeypatch.setenv("PHZ_BAM_HOST", "1")
    rc, prefix = run_cli(cli_inputs, "ht_host", "--output_haplotag_bam", "1")
    text = capsys.readouterr().out
    assert rc == 0 and "no haplotagged BAM for" in text and "host decoder read it" in text
    assert os.path.exists(prefix + ".haplotypic_counts.txt") and not os.path.exists(prefix + ".haplotag.1.bam")
