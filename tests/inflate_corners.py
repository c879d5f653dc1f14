"""TEST INFRASTRUCTURE shared by tests/test_emu_inflate_corners.py (host emulation) and tests/test_gpu_inflate_corners.py (MI355X): K_inflate and k_crc32
on the streams of tests/deflate_builder.py.  A `device` is anything with run(comp, rec, out, want_crc) -> (inflate status, output array, CRC status or None).

The EXPECTED bytes are always zlib's decode of the stream, never the builder's idea of it; every member's output sits between 32-byte gaps of
0xEE that must come back untouched, so a store past a member's end is seen whatever lies next to it."""
import base64
import ctypes as C
import gzip
import json
import os
import random
import zlib

import numpy as np

import deflate_builder as B

MEMBER = np.dtype([("src", "<u8"), ("csize", "<u4"), ("isize", "<u4"), ("dst", "<u8")])
GAP = 32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate", "libdeflate_streams.json.gz")


def aligned_bytes(n, fill):
    """uint8 [n] whose first byte is 16-byte aligned (what phz_bgzf_inflate_device asks of comp)"""
    raw = np.full(n + 16, fill, dtype=np.uint8)
    off = (-raw.ctypes.data) & 15
    return raw[off:off + n]


class EmuDevice:
    """phz_bgzf_inflate_device / phz_bgzf_crc_device of the emulation library, host pointers"""

    def __init__(self):
        from helpers import EmuContext, emu_library
        self.ctx = EmuContext(emu_library())

    def run(self, comp, rec, out, want):
        ctx = self.ctx; bad = C.c_int(0); crc_bad = None
        ctx.check(ctx.lib.phz_bgzf_inflate_device(ctx.h, C.c_void_p(comp.ctypes.data), C.c_void_p(rec.ctypes.data), len(rec), C.c_void_p(out.ctypes.data), C.byref(bad)))
        if want is not None and bad.value == 0:
            b2 = C.c_int(0)
            ctx.check(ctx.lib.phz_bgzf_crc_device(ctx.h, C.c_void_p(out.ctypes.data), C.c_void_p(rec.ctypes.data), len(rec), C.c_void_p(want.ctypes.data), C.byref(b2)))
            crc_bad = b2.value
        return bad.value, out, crc_bad


class GpuDevice:
    """the same two entry points of libphz.so on a Context of the product (phaser_amd.mapper.Mapper(0).ctx), device tensors"""

    def __init__(self, ctx):
        self.ctx = ctx

    def run(self, comp, rec, out, want):
        import torch
        ctx = self.ctx; bad = C.c_int(0); crc_bad = None
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
        dcomp = up(comp); drec = up(rec); dout = up(out)
        assert dcomp.data_ptr() % 16 == 0
        ctx.check(ctx.lib.phz_bgzf_inflate_device(ctx.h, C.c_void_p(dcomp.data_ptr()), C.c_void_p(drec.data_ptr()), len(rec), C.c_void_p(dout.data_ptr()), C.byref(bad)))
        if want is not None and bad.value == 0:
            dwant = up(want); b2 = C.c_int(0)
            ctx.check(ctx.lib.phz_bgzf_crc_device(ctx.h, C.c_void_p(dout.data_ptr()), C.c_void_p(drec.data_ptr()), len(rec), C.c_void_p(dwant.data_ptr()), C.byref(b2)))
            crc_bad = b2.value
        return bad.value, dout.cpu().numpy(), crc_bad


def run_members(device, streams, sizes, crcs=None, src_mod=None, fill=0xAA):
    """One call for all `streams` (raw DEFLATE; sizes: the ISIZE each member claims).  src_mod[i]: the member's src & 15 (default: odd offsets as they
    come); `fill`: the bytes before, between and after the members in the compressed buffer.  -> (inflate status, [output bytes], CRC status or None);
    asserts that no byte outside the members' outputs was written."""
    n = len(streams)
    at = 0; srcs = []
    for i, s in enumerate(streams):
        at += 1 + (3 * (i + 1)) % 7
        if src_mod is not None:
            at += (src_mod[i] - at) % 16
        srcs.append(at); at += len(s)
    comp = aligned_bytes(at + 32, fill)          # readable (and not zero unless asked for) well past the 16 bytes the interface requires
    rec = np.zeros(n, dtype=MEMBER); dst = GAP
    for i, (s, size) in enumerate(zip(streams, sizes)):
        comp[srcs[i]:srcs[i] + len(s)] = np.frombuffer(s, dtype=np.uint8)
        rec[i] = (srcs[i], len(s), size, dst)
        dst += size + GAP
    out = np.full(dst, 0xEE, dtype=np.uint8)
    want = None if crcs is None else np.asarray(crcs, dtype=np.uint32)
    bad, got, crc_bad = device.run(comp, rec, out, want)
    keep = np.ones(dst, dtype=bool)
    for r in rec:
        keep[int(r["dst"]):int(r["dst"]) + int(r["isize"])] = False
    touched = np.nonzero(keep & (got != 0xEE))[0]
    if len(touched):
        before = [i for i, r in enumerate(rec) if int(r["dst"]) + int(r["isize"]) <= touched[0]]
        raise AssertionError("bytes outside the members' outputs were written: offsets %s (first one after member %s)" % (touched[:8].tolist(), before[-1] if before else None))
    return bad, [got[int(r["dst"]):int(r["dst"]) + int(r["isize"])].tobytes() for r in rec], crc_bad


def zlib_decode(stream):
    """zlib's decode of a raw DEFLATE stream, or None where zlib refuses it"""
    try:
        d = zlib.decompressobj(-15)
        out = d.decompress(stream)
        return out if d.eof else None
    except zlib.error:
        return None


_cache = {}


def expected_catalogue():
    """{name: (stream, zlib's decode)} of the builder's catalogue; asserts that zlib accepts every stream and that members have BGZF sizes"""
    if "cat" not in _cache:
        cat = {}
        for name, s in B.catalogue().items():
            want = zlib_decode(s)
            assert want is not None, "zlib refuses %s: the builder wrote an invalid stream" % name
            assert 0 < len(want) <= 65536 and len(s) <= 65536, name
            cat[name] = (s, want)
        _cache["cat"] = cat
    return _cache["cat"]


def zlib_members():
    """ordinary members from zlib's encoder (every block type), to stand between the corner streams"""
    if "zl" not in _cache:
        rng = random.Random(7)
        text = b"".join(b"chr%d\t%d\trs%d\tA\tG\t.\tPASS\n" % (rng.randrange(1, 23), rng.randrange(10 ** 8), rng.randrange(10 ** 7)) for _ in range(600))
        rnd = bytes(rng.getrandbits(8) for _ in range(5000))
        out = []
        for data in (text, rnd, b"A" * 9000, text[:100], b"x"):
            for level, strategy in ((6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY)):
                co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
                out.append((co.compress(data) + co.flush(), data))
        _cache["zl"] = out
    return _cache["zl"]


def compare(names, got, want):
    wrong = [n for n, g, w in zip(names, got, want) if g != w]
    assert not wrong, "%d of %d members differ from zlib's decode: %s" % (len(wrong), len(names), wrong[:10])


# ------------------------------------------------------------------ the checks (same code under the emulation and on the GPU)
def check_each_alone(device):
    """(a) 1: every catalogue member in a call of its own (n_members = 1: lane 0 of a workgroup whose other lanes leave at once)"""
    failed = []
    for name, (s, want) in expected_catalogue().items():
        bad, got, crc_bad = run_members(device, [s], [len(want)], crcs=[zlib.crc32(want)])
        if bad != 0 or got[0] != want or crc_bad != 0:
            failed.append((name, bad, crc_bad, got[0] == want))
    assert not failed, "%d members (name, status, CRC status, bytes equal): %s" % (len(failed), failed[:10])


def check_shuffled_among_zlib_members(device):
    """(a) 2: the whole catalogue in one call, shuffled among zlib-written members: the 64 lanes of a workgroup are in different block kinds, with different
    tables, at different depths of their copy loops"""
    items = [(n, s, w) for n, (s, w) in expected_catalogue().items()]
    items += [("zlib_%d" % i, s, w) for i, (s, w) in enumerate(zlib_members() * 4)]
    random.Random(2).shuffle(items)
    names, streams, want = zip(*items)
    assert len(items) > 8 * 64
    crcs = [zlib.crc32(w) for w in want]
    bad, got, crc_bad = run_members(device, streams, [len(w) for w in want], crcs=crcs)
    compare(names, got, want)
    assert bad == 0 and crc_bad == 0
    # .. and the CRC pass sees one wrong trailer among them
    crcs[len(crcs) // 3] ^= 1
    assert run_members(device, streams, [len(w) for w in want], crcs=crcs)[2] == 7


WORKGROUP_STREAMS = ("deep15_hlit286_hdist30", "cl_run16_first_copy_is_last_litlen", "overlap_final_d63_l65", "stored_at_bit_offset_5_after_fixed", "dist_only_symbol_29")


def check_full_workgroup_plus_one(device, name):
    """(a) 3: one corner stream in 65 lanes: all 64 lanes of a workgroup take the rare path together (same LDS slots, same cold table offsets in their own
    scratch), and one lane of a second workgroup"""
    s, want = expected_catalogue()[name]
    bad, got, crc_bad = run_members(device, [s] * 65, [len(want)] * 65, crcs=[zlib.crc32(want)] * 65)
    compare(["%s[%d]" % (name, i) for i in range(65)], got, [want] * 65)
    assert bad == 0 and crc_bad == 0


def check_source_alignment(device):
    """(b): a dynamic, a fixed and a stored member at every src & 15 with every compressed size mod 16, 0xFF all around them: the first and last 16-byte
    units that BitIn::start reads hold bytes of the neighbours, which must not reach the output"""
    names = []; streams = []; want = []; mods = []
    for name, s in B.alignment_streams():
        w = zlib_decode(s)
        assert w, name
        for a in range(16):
            names.append("%s at src%%16=%d" % (name, a)); streams.append(s); want.append(w); mods.append(a)
    assert len(streams) == 3 * 16 * 16
    assert len(set((n.split("_")[0], len(s) % 16, m) for n, s, m in zip(names, streams, mods))) == 768
    order = list(range(len(streams))); random.Random(3).shuffle(order)
    pick = lambda xs: [xs[i] for i in order]
    bad, got, crc_bad = run_members(device, pick(streams), [len(w) for w in pick(want)], crcs=[zlib.crc32(w) for w in pick(want)], src_mod=pick(mods), fill=0xFF)
    compare(pick(names), got, pick(want))
    assert bad == 0 and crc_bad == 0


def fixture_streams():
    with gzip.open(FIXTURE, "rt") as f:
        doc = json.load(f)
    return [(e["name"], base64.b64decode(e["deflate"])) for e in doc["streams"]]


def check_other_encoder(device):
    """(c): streams written by libdeflate (tools/make_inflate_fixtures.py; only the compressed bytes are kept), decoded on the device and by zlib"""
    items = fixture_streams()
    assert len(items) >= 48
    names = [n for n, _ in items]; streams = [s for _, s in items]
    want = [zlib_decode(s) for s in streams]
    assert all(w is not None for w in want)
    assert len(set(want)) >= 18 and max(len(w) for w in want) == 8192 and min(len(w) for w in want) == 1          # six payload kinds, whole and cut
    bad, got, crc_bad = run_members(device, streams, [len(w) for w in want], crcs=[zlib.crc32(w) for w in want])
    compare(names, got, want)
    assert bad == 0 and crc_bad == 0


INVALID = B.invalid_streams()
LENIENT = B.lenient_streams()


def check_invalid(device, case):
    """(d): zlib refuses the stream (or decodes another number of bytes than the member claims), and the kernel answers with the status code of its enum"""
    name, s, isize, code = case
    z = zlib_decode(s)
    assert z is None or len(z) != isize, "%s: zlib accepts it" % name
    bad, got, _ = run_members(device, [s], [isize])
    assert bad == code, "%s: status %d, expected %d" % (name, bad, code)


def check_lenient(device, case):
    """What K_inflate accepts and zlib's decoder does not (Device BAM path): status 0, the bytes of the builder's token expansion, and a CRC pass
    that agrees with zlib's CRC of those bytes.  (Zero bytes follow the member: one of the streams is cut short and reads them.)"""
    name, s, want = case
    assert zlib_decode(s) is None, "%s: zlib accepts it, so it belongs in the catalogue" % name
    bad, got, crc_bad = run_members(device, [s], [len(want)], crcs=[zlib.crc32(want)], fill=0)
    assert bad == 0 and got[0] == want and crc_bad == 0, (name, bad, crc_bad)
    assert run_members(device, [s], [len(want)], crcs=[zlib.crc32(want) ^ 0x80000000], fill=0)[2] == 7
