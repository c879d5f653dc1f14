"""BAM files with PLANTED fake record chains, for the three places that guess a record boundary from 12 plausible headers in a row: `probe` in bam_plan
(phz_bam.cpp), the host's parallel record hop in phz_bam_decode, and k_seg_start of the device decoder (phz_bamdev.hip).  Plain Python, no GPU.

Every file is a valid, coordinate-sorted BAM.  A FAKE is 38 bytes that read as a minimal record (block_size 34, a one-character name, no CIGAR, no
SEQ); a CARRIER is an ordinary record whose last tag, XF:B:C, holds a run of 40 fakes back to back, so a 12-chain that starts on one of them holds.
Flavours of a carrier:
    resync     the run ends at the carrier's end: the fake chain lands on the true next record
    dead_end   the run is followed by 64 bytes of 0xEE: a negative block_size stops any chain there
    unordered  as resync, but the fakes' positions descend: only a rule that wants coordinate order along the chain tells them from records
A PLAIN record has no aux array; a guess that falls inside it meets a true boundary first.

The module also RESTATES the guess (`plausible`, `chain_start`) in two forms -- the device rule (keys (ref, pos+1) must not descend along the chain)
and the host rule (no key rule) -- and every layout checks itself with it when it is built: each guess must land where the layout intends, on a
planted fake or on a true boundary.  A layout that stops exercising its path (or random bytes that form an accidental chain) fails there, on the CPU,
before any decoder is asked.

The members are written here, one per chosen cut (bamio.write_bam cuts every 60,000 bytes and cannot place a member boundary)."""
import atexit
import functools
import os
import shutil
import struct
import tempfile

import numpy as np

REFS = [("chr21", 46709983), ("chr22", 50818468)]
SEG = 262144            # BamLayout::SEG: the device cuts a piece every SEG bytes
FAKE = 38
N_FAKES = 40
CHAIN = 12
REG = 600               # bases of an ordinary plain record
FIELDS = ("pos", "cigar_off", "cigar", "seq_off", "seq2", "qual", "qid", "aln_score", "has_as")


# ------------------------------------------------------------------------------------------------------------ records
def header(refs=REFS) -> bytes:
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return out


def fake(ref: int, pos0: int, ch: int) -> bytes:
    """38 bytes: block_size 34, l_read_name 2, n_cigar 0, flag 0, l_seq 0, mate refID -1, mate pos -1, name = one printable byte + NUL"""
    assert 33 <= ch <= 126
    b = struct.pack("<iiiBBHHHiiii", 34, ref, pos0, 2, 0, 0, 0, 0, 0, -1, -1, 0) + bytes([ch, 0])
    assert len(b) == FAKE
    return b


def _size(name: str, L: int) -> int:          # bytes of a plain record: block_size, fixed fields, name, one CIGAR op, SEQ, QUAL, AS:i
    return 4 + 32 + len(name) + 1 + 4 + (L + 1) // 2 + L + 7


def _record(ref, pos0, name, L, rng, tail=b"") -> bytes:
    assert L >= 1
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)[rng.integers(0, 4, 2 * ((L + 1) // 2))]
    seq = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
    qual = rng.integers(2, 42, L, dtype=np.uint8).tobytes()
    qn = name.encode() + b"\0"
    body = (struct.pack("<iiBBHHHiiii", ref, pos0, len(qn), 60, 4680, 1, 0, L, -1, -1, 0) + qn + struct.pack("<I", L << 4) + seq + qual +
            b"ASi" + struct.pack("<i", int(rng.integers(-50, 200))) + tail)
    return struct.pack("<i", len(body)) + body


class Stream:
    """The inflated stream under construction: header, then records in coordinate order.  `true` = offsets where a record starts, `runs` = per
    carrier the offsets of its fakes, `cuts` = offsets where a member starts (besides 0)."""

    def __init__(self, seed, switch_at=None):
        self.buf = bytearray(header())
        self.first = len(self.buf)
        self.rng = np.random.default_rng(seed)
        self.true = []; self.runs = []; self.cuts = []
        self.ref = 0; self.pos0 = 100; self.i = 0
        self.switch_at = switch_at              # stream offset after which the records are the second reference's

    def off(self):
        return len(self.buf)

    def _next(self, prefix):
        if self.switch_at is not None and self.ref == 0 and self.off() >= self.switch_at:
            self.ref = 1; self.pos0 = 100
        self.pos0 += int(self.rng.integers(0, 40))
        self.i += 1
        return "%s%05d" % (prefix, self.i)

    def next_ref(self):
        self.ref += 1; self.pos0 = 100

    def plain(self, L=REG, name=None):
        name = name or self._next("p")
        self.true.append(self.off())
        self.buf += _record(self.ref, self.pos0, name, L, self.rng)

    def exact(self, size):
        """a plain record of exactly `size` bytes (the name is padded by up to two characters: SEQ + QUAL alone reach only two sizes of three)"""
        name = self._next("p")
        for pad in range(3):
            rem = size - _size(name + "x" * pad, 0)
            if rem >= 2 and rem % 3 != 1:
                L = 2 * rem // 3 if rem % 3 == 0 else (2 * rem - 1) // 3
                before = self.off()
                self.plain(L, name + "x" * pad)
                assert self.off() - before == size
                return
        raise AssertionError("no plain record of %d bytes" % size)

    def fill_to(self, target):
        """plain records up to exactly `target`"""
        small = _size("p00000xx", 0) + 8
        assert target - self.off() >= small, (target, self.off())
        while target - self.off() >= _size("p00000", REG) + small:
            self.plain()
        self.exact(target - self.off())

    def carrier_head(self, L):                 # bytes of a carrier before its first fake (names have one length)
        return _size("c00000", L) + 8

    def carrier(self, flavour, L=100, fake_ref=None):
        name = self._next("c")
        fr = self.ref if fake_ref is None else fake_ref
        run = b"".join(fake(fr, self.pos0 + (1000 - 7 * k if flavour == "unordered" else 0), 65 + k % 26) for k in range(N_FAKES))
        payload = run + (b"\xee" * 64 if flavour == "dead_end" else b"")
        start = self.off()
        self.true.append(start)
        self.buf += _record(self.ref, self.pos0, name, L, self.rng, b"XFBC" + struct.pack("<i", len(payload)) + payload)
        at = start + _size(name, L) + 8
        assert bytes(self.buf[at:at + FAKE]) == run[:FAKE]
        self.runs.append([at + FAKE * k for k in range(N_FAKES)])
        if flavour != "dead_end":
            assert at + FAKE * N_FAKES == self.off()
        return self.runs[-1]


# ------------------------------------------------------------------------------------------------------------ the guess, restated
def plausible(d, n, p, n_ref):
    """Can offset p of d[0, n) start a record?  -> (offset of the next record, sort key) or None.  The header test of the decoders' `plausible` (host lambda in phz_bam_decode, device function in phz_bamdev.hip)."""
    if p + 36 > n:
        return None
    bs, ref, pos0, l_rn, _mq, _bin, n_cig, flag, l_seq, nref, npos = struct.unpack_from("<iiiBBHHHiii", d, p)
    if bs < 32 or bs > (1 << 24) or p + 4 + bs > n:
        return None
    if ref < -1 or ref >= n_ref or nref < -1 or nref >= n_ref or pos0 < -1 or l_seq < 0 or l_rn < 2 or flag >= 4096 or npos < -1:
        return None
    if 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return None
    name = d[p + 36:p + 36 + l_rn]
    if name[-1] != 0 or any(c < 33 or c > 126 for c in name[:-1]):
        return None
    return p + 4 + bs, ((0x7fffffff if ref < 0 else ref), pos0 + 1)


def chain_holds(d, end, p, n_ref, ordered):
    """12 plausible headers in a row from p (the chain may run into `end`); ordered = the device rule: keys must not descend along the chain"""
    q = p; prev = (0, 0)
    for _ in range(CHAIN):
        r = plausible(d, end, q, n_ref)
        if r is None or (ordered and r[1] < prev):
            return False
        q, prev = r
        if q + 4 > end:
            return True
    return True


def _candidates(d, n_ref):
    """offsets whose first header fields pass (block_size, refID and name length in range): a necessary condition of `plausible`, vectorised so that a
    scan through hundreds of kilobytes of SEQ / QUAL bytes does not call it at every byte"""
    u = np.frombuffer(bytes(d), dtype=np.uint8).astype(np.int64)
    m = len(u) - 36
    w = lambda at: u[at:at + m] | (u[at + 1:at + 1 + m] << 8) | (u[at + 2:at + 2 + m] << 16) | (u[at + 3:at + 3 + m] << 24)
    bs = w(0); ref = w(4)
    ref = np.where(ref >= 1 << 31, ref - (1 << 32), ref)
    return np.flatnonzero((bs >= 32) & (bs <= 1 << 24) & (ref >= -1) & (ref < n_ref) & (u[12:12 + m] >= 2))


def chain_start(d, cand, guess, end, n_ref, ordered, limit=32 << 20):
    """what k_seg_start (ordered) / the host's guess loop (not ordered) answer: the first p in [guess, min(guess + limit, end)) where a chain holds;
    `end` where none does"""
    stop = min(guess + limit, end)
    for p in cand[np.searchsorted(cand, guess):]:
        if p >= stop:
            break
        if chain_holds(d, end, int(p), n_ref, ordered):
            return int(p)
    return end


# ------------------------------------------------------------------------------------------------------------ files
_DIR = tempfile.mkdtemp(prefix="bam_boundaries_")
atexit.register(shutil.rmtree, _DIR, True)


class Layout:
    def __init__(self, name, s: Stream):
        from phaser_amd import bamio
        self.name = name
        self.stream = bytes(s.buf); self.first = s.first; self.n = len(self.stream)
        self.true = set(s.true); self.runs = s.runs
        self.fakes = {f for run in s.runs for f in run}
        self.n_ref = len(REFS)
        self.cand = _candidates(self.stream, self.n_ref)
        cuts = sorted(set(s.cuts))
        if not cuts:                           # no chosen cut: members end at the last record start within 60,000 bytes, mid-record only inside a longer record
            starts = sorted(self.true); at = 0
            while self.n - at > 60000:
                k = int(np.searchsorted(starts, at + 60000, side="right")) - 1
                at = starts[k] if k >= 0 and starts[k] > at else at + 60000
                cuts.append(at)
        self.cuts = cuts
        edges = [0] + cuts + [self.n]
        assert all(0 < b - a <= 65536 for a, b in zip(edges, edges[1:]))
        self.path = os.path.join(_DIR, name + ".bam")
        with open(self.path, "wb") as f:
            for a, b in zip(edges, edges[1:]):
                f.write(bamio._bgzf_block(self.stream[a:b]))
            f.write(bamio._EOF)
        assert bamio.read_bam_bytes(self.path) == self.stream

    def lands(self, guess, end=None, ordered=True):
        return chain_start(self.stream, self.cand, guess, self.n if end is None else end, self.n_ref, ordered)

    def seg_guesses(self):                     # the device's guesses in a whole-file decode: the piece starts at the first record
        return list(range(self.first + SEG, self.n, SEG))

    @functools.lru_cache(maxsize=None)
    def _reference(self, chroms):
        from phaser_amd import bamio
        it = {}
        sh = bamio.shards_from_bam(self.path, it, 0, False, False, chroms=None if chroms is None else set(chroms))
        return sh, {c: list(x.names) for c, x in it.items()}

    def reference(self, chroms=None):
        """(shards, QNAMEs per chromosome in id order) of the sequential pure-Python reader; computed once per file and restriction, never changed"""
        return self._reference(None if chroms is None else tuple(sorted(chroms)))


SEGMENT_LAYOUTS = {            # name -> (guesses that a carrier straddles; None = the last one, length of the piece in segments)
    "isolated": ([2], 3.4),
    "three_in_a_row": ([2, 3, 4], 5.4),
    "seven": (list(range(2, 9)), 9.4),
    "eight": (list(range(2, 10)), 10.4),
    "last_segment": (None, 3.3),
}
SEGMENT_FLAVOURS = {name: ("resync", "dead_end") + (("unordered",) if name == "isolated" else ()) for name in SEGMENT_LAYOUTS}


@functools.lru_cache(maxsize=None)
def segment_layout(name, flavour) -> Layout:
    """A carrier at every chosen guess of a whole-file device decode, so that the guess falls 3 bytes into fake #5 of its run and k_seg_start answers
    fake #6; plain records everywhere else; the second reference begins half way."""
    ks, segs = SEGMENT_LAYOUTS[name]
    s = Stream(sum(name.encode()) * 7 + len(flavour))
    end = s.first + int(segs * SEG)
    if ks is None:
        ks = [(end - 1 - s.first) // SEG]
    s.switch_at = s.first + int(segs * SEG / 2) + 5000
    for k in ks:
        s.fill_to(s.first + k * SEG - 3 - 5 * FAKE - s.carrier_head(100))
        run = s.carrier(flavour)
        assert run[5] + 3 == s.first + k * SEG
    s.fill_to(end)
    lay = Layout("%s_%s" % (name, flavour), s)
    lay.carrier_ks = ks
    # self-check, device rule: the guesses at the carriers land on fake #6 (unordered: on the true boundary behind the carrier, and it is the key rule
    # alone that skips the fakes -- the host rule takes #6), every other guess lands on a true boundary
    g = lay.seg_guesses()
    assert len(g) + 1 == int(np.ceil(segs)) and lay.n == end
    for k, guess in enumerate(g, start=1):
        got = lay.lands(guess)
        if k in ks:
            run = lay.runs[ks.index(k)]
            if flavour == "unordered":
                assert got == run[-1] + FAKE and got in lay.true, (name, flavour, k, got)
                assert lay.lands(guess, ordered=False) == run[6]
            else:
                assert got == run[6] and got not in lay.true, (name, flavour, k, got)
        else:
            assert got in lay.true, (name, flavour, k, got)
    return lay


HOST_K = 8                     # threads = 2: the host's parallel hop cuts the stream into 4 * threads segments


@functools.lru_cache(maxsize=None)
def host_layout(flavour) -> Layout:
    """A carrier at guess 4 of 8 of the HOST's parallel hop, whose guesses are first_record + (n - first_record) / 8 * k: they depend on the stream's
    length n, so the last record is sized to make n come out right."""
    s = Stream(4242 + len(flavour))
    q = 40000
    guess = s.first + 4 * q
    s.fill_to(guess - 3 - 5 * FAKE - s.carrier_head(100))
    run = s.carrier(flavour)
    s.next_ref()
    s.fill_to(s.first + HOST_K * q + 7)
    lay = Layout("host_%s" % flavour, s)
    step = (lay.n - lay.first) // HOST_K
    assert step == q
    for k in range(1, HOST_K):
        got = lay.lands(lay.first + step * k, ordered=False)
        assert (got == run[6] and got not in lay.true) if k == 4 else got in lay.true, (flavour, k, got)
    return lay


@functools.lru_cache(maxsize=None)
def long_record_layout() -> Layout:
    """In each reference one plain record of 400,000 bases (about 600 KB) among short ones: a whole segment lies inside the record, two (or three)
    consecutive guesses find the same boundary and the segments between them are empty."""
    s = Stream(31337)
    longs = []
    for r in range(2):
        if r:
            s.next_ref()
        for _ in range(60 + 45 * r):
            s.plain()
        longs.append(s.off())
        s.plain(400000)
        longs.append(s.off())
        for _ in range(80):
            s.plain()
    lay = Layout("long_record", s)
    g = lay.seg_guesses()
    for a, b in zip(longs[0::2], longs[1::2]):
        inside = [x for x in g if a < x < b]
        assert len(inside) >= 2 and b in lay.true
        assert all(lay.lands(x) == b for x in inside)
    assert all(lay.lands(x) in lay.true for x in g)
    return lay


MEMBER_VARIANTS = ("same", "last", "first")     # refID of the fakes: the carrier's own, always the last reference, always the first
PER_REF = 300
# What bam_plan still gets wrong, (variant, restriction) -> why: members of `member_layout(..., covered=True)`.  The plan reaches a member's first boundary by
# walking the chain from the member before it, which leaves a resyncing run of fakes together with its record -- unless the run covers the rest of that
# member and the start of the next one, where the walk arrives on a fake again.  No local rule tells such fakes from a stretch of records.
COVERED_XFAIL = {
    ("last", "chr21"): "fakes of refID 1 under member starts inside chr21: the piece of chr21 ends on one of them, inside a record, and the open is refused",
}


@functools.lru_cache(maxsize=None)
def member_layout(flavour, variant, covered=False) -> Layout:
    """2 x 300 carriers; a member starts at fake #5 of every 12th record's run, so every guess of `probe` but the first begins on a fake.
    covered: another member starts at fake #20 of the same run, so the member before it holds nothing but fakes #5 .. #19."""
    s = Stream(977 + 3 * len(flavour) + MEMBER_VARIANTS.index(variant))
    for r in range(2):
        if r:
            s.next_ref()
        for i in range(PER_REF):
            run = s.carrier(flavour, fake_ref={"same": None, "last": len(REFS) - 1, "first": 0}[variant])
            if (r * PER_REF + i) % 12 == 0 and r + i:
                s.cuts.append(run[5])
                if covered:
                    s.cuts.append(run[20])
    lay = Layout("members_%s_%s%s" % (flavour, variant, "_covered" if covered else ""), s)
    # self-check, host rule (all that `probe` once asked of a candidate): every member but the first starts on a chain of 12 fakes
    assert len(lay.cuts) == (2 * PER_REF // 12 - 1) * (2 if covered else 1)
    for c in lay.cuts:
        assert c in lay.fakes and chain_holds(lay.stream, lay.n, c, lay.n_ref, False), c
    return lay


def same_shards(want, names, got, got_interners, what):
    """array by array, and the interner's names in order; `got` may live on the device"""
    import torch
    assert list(got) == list(want), (what, list(got), list(want))
    for c in want:
        for f in FIELDS:
            a = getattr(want[c], f); b = getattr(got[c], f).cpu()
            assert torch.equal(a.to(b.dtype), b), (what, c, f)
        assert list(got_interners[c].names) == names[c], (what, c)
