"""TEST INFRASTRUCTURE: a DEFLATE (RFC 1951) *writer* that emits exactly the blocks, code lengths and tokens it is told to -- the streams
that zlib's encoder never writes and K_inflate (phaser_amd/csrc/phz_inflate.hip) must still decode, and damaged streams it must refuse.
Pure Python, written from the RFC.  Nothing here checks that a stream is valid: the tests ask zlib's decoder for that, and for the
expected bytes (tests/test_emu_inflate_corners.py, tests/test_gpu_inflate_corners.py).

    Deflate().stored(b"abc", last=False).fixed([97, 98, (5, 2)], last=True).done()      # -> bytes

Tokens: an int is a literal; (length, distance) is a match; ("lsym", s) / ("dsym", s) write the code of literal/length / distance symbol s
with no extra bits after it; ("raw", value, nbits) writes nbits of value, least significant first."""
import random

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5: length symbols 257..285 and distance symbols 0..29
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """Bits least significant first into bytes (RFC 1951 3.1.1); Huffman codes most significant bit first."""

    def __init__(self):
        self.buf = bytearray(); self.acc = 0; self.n = 0

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n; self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 0xFF); self.acc >>= 8; self.n -= 8
        return self

    def huff(self, code, n):
        rev = 0
        for i in range(n):
            rev |= ((code >> (n - 1 - i)) & 1) << i
        return self.bits(rev, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def bit_length(self):
        return 8 * len(self.buf) + self.n

    def done(self):
        """the bytes so far, the last one padded with zero bits"""
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def canonical_codes(lengths):
    """RFC 1951 3.2.2; lengths are taken as they come (an over-subscribed set gives codes cut to their length)"""
    top = max(list(lengths) + [1])
    count = [0] * (top + 2)
    for l in lengths:
        if l:
            count[l] += 1
    nxt = [0] * (top + 2); code = 0
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l] & ((1 << l) - 1)); nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft_left(lengths):
    """2^15 minus the Kraft sum in units of 2^-15: 0 complete, > 0 incomplete, < 0 over-subscribed"""
    return (1 << 15) - sum(1 << (15 - l) for l in lengths if l)


def length_symbol(length, len258_as_284=False):
    """-> (symbol - 257, extra value)"""
    if length == 258 and not len258_as_284:
        return 28, 0
    s = max(i for i in range(28) if LBASE[i] <= length)
    assert length - LBASE[s] < (1 << LEXT[s]), length
    return s, length - LBASE[s]


def dist_symbol(dist):
    s = max(i for i in range(30) if DBASE[i] <= dist)
    assert dist - DBASE[s] < (1 << DEXT[s]), dist
    return s, dist - DBASE[s]


def rle_ops(lengths):
    """Greedy run-length coding of ONE array of code lengths (the caller passes literal/length + distance lengths concatenated, so a run
    crosses the boundary between them whenever the values allow): [(code-length symbol, extra value or None)]"""
    ops = []; i = 0; n = len(lengths)
    while i < n:
        v = lengths[i]; j = i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138); ops.append((18, r - 11)); run -= r
            if run >= 3:
                ops.append((17, run - 3)); run = 0
        else:
            ops.append((v, None)); run -= 1
            while run >= 3:
                r = min(run, 6); ops.append((16, r - 3)); run -= r
        ops += [(v, None)] * run
        i = j
    return ops


def ops_spans(ops):
    """[(symbol, first index written, one past the last)] of a list of run-length ops"""
    out = []; at = 0
    for sym, extra in ops:
        n = 1 if sym < 16 else (3 + extra if sym in (16, 17) else 11 + extra)
        out.append((sym, at, at + n)); at += n
    return out


def complete_code(size, symbols):
    """Code lengths [size]: a complete code over `symbols` (most frequent first), as balanced as it can be; a lone symbol gets one bit and a
    second, unused symbol the other, so that the code is complete"""
    symbols = list(symbols)
    if len(symbols) == 1:
        symbols.append(next(s for s in range(size) if s != symbols[0]))
    k = len(symbols); d = (k - 1).bit_length()
    short = (1 << d) - k
    out = [0] * size
    for i, s in enumerate(symbols):
        out[s] = d - 1 if i < short else d
    return out


def fill_code(size, fixed, fillers):
    """Code lengths [size] with the lengths of `fixed` {symbol: length} as given and every symbol of `fillers` given a length such that the whole
    set is Kraft-complete (earlier fillers get the shorter codes)"""
    left = kraft_left(fixed.values())
    assert left > 0 and fillers
    pieces = [l for l in range(1, 16) if (left >> (15 - l)) & 1]          # the free code space as a sum of 2^-l
    assert len(pieces) <= len(fillers), "too few fillers"
    while len(pieces) < len(fillers):
        pieces.sort()
        l = pieces.pop(0); assert l < 15, "too many fillers"
        pieces += [l + 1, l + 1]
    pieces.sort()
    out = [0] * size
    for s, l in fixed.items():
        out[s] = l
    for s, l in zip(fillers, pieces):
        out[s] = l
    assert kraft_left(out) == 0
    return out


def deep_lengths(n, depth):
    """n code lengths, ascending, Kraft-complete, the longest exactly `depth`: a chain 1, 2, .., c and the other n - c symbols balanced below it.
    deep_lengths(263, 15) = 1..7 and 256 codes of 15 bits: code-order slots far beyond the decoder's hot table."""
    for c in range(min(depth, n - 1) - 1, -1, -1):
        m = n - c; d = (m - 1).bit_length()          # m >= 2 symbols share the chain's last 2^-c of code space
        if c + d != depth:
            continue
        short = (1 << d) - m
        out = list(range(1, c + 1)) + [c + d - 1] * short + [c + d] * (m - short)
        assert kraft_left(out) == 0 and max(out) == depth
        return out
    raise ValueError("no chain code of %d symbols is %d deep" % (n, depth))


def assign_lengths(size, symbols, lengths):
    """code lengths [size]: symbols[i] gets lengths[i], every other symbol 0"""
    assert len(symbols) == len(lengths) == len(set(symbols))
    out = [0] * size
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


class Deflate(BitWriter):
    """A raw DEFLATE stream, block by block (every method returns self)."""

    def stored(self, data, last):
        self.bits(1 if last else 0, 1); self.bits(0, 2); self.align()
        self.bits(len(data), 16); self.bits(len(data) ^ 0xFFFF, 16)
        assert self.n == 0
        self.buf += data
        return self

    def fixed(self, tokens, last, len258_as_284=False, eob=True):
        self.bits(1 if last else 0, 1); self.bits(1, 2)
        return self._tokens(tokens, FIXED_LITLEN, FIXED_DIST, eob, len258_as_284)

    def dynamic(self, tokens, last, litlen_lengths, dist_lengths, cl_ops=None, cl_lengths=None, eob=True, len258_as_284=False):
        """HLIT = len(litlen_lengths) - 257 and HDIST = len(dist_lengths) - 1, whatever they are (5 bits each).  The two arrays are run-length
        coded as one (cl_ops: the run-length ops to write instead) with a complete code-length code of its own (cl_lengths [19]: that code instead)."""
        nlen, ndist = len(litlen_lengths), len(dist_lengths)
        assert 0 <= nlen - 257 < 32 and 0 <= ndist - 1 < 32
        ops = list(cl_ops) if cl_ops is not None else rle_ops(list(litlen_lengths) + list(dist_lengths))
        if cl_lengths is None:
            freq = {}
            for s, _ in ops:
                freq[s] = freq.get(s, 0) + 1
            cl_lengths = complete_code(19, sorted(freq, key=lambda s: (-freq[s], s)))
        assert len(cl_lengths) == 19 and max(cl_lengths) <= 7
        ncode = max([4] + [i + 1 for i in range(19) if cl_lengths[CL_ORDER[i]]])
        self.bits(1 if last else 0, 1); self.bits(2, 2)
        self.bits(nlen - 257, 5); self.bits(ndist - 1, 5); self.bits(ncode - 4, 4)
        for i in range(ncode):
            self.bits(cl_lengths[CL_ORDER[i]], 3)
        codes = canonical_codes(cl_lengths)
        for s, extra in ops:
            assert cl_lengths[s], "code-length symbol %d has no code" % s
            self.huff(codes[s], cl_lengths[s])
            if s >= 16:
                self.bits(extra, {16: 2, 17: 3, 18: 7}[s])
        return self._tokens(tokens, litlen_lengths, dist_lengths, eob, len258_as_284)

    def _tokens(self, tokens, ll, dl, eob, as284):
        lc = canonical_codes(ll); dc = canonical_codes(dl)

        def lsym(s):
            assert s < len(ll) and ll[s], "literal/length symbol %d has no code" % s
            self.huff(lc[s], ll[s])

        def dsym(s):
            assert s < len(dl) and dl[s], "distance symbol %d has no code" % s
            self.huff(dc[s], dl[s])
        for t in tokens:
            if isinstance(t, int):
                lsym(t)
            elif t[0] == "lsym":
                lsym(t[1])
            elif t[0] == "dsym":
                dsym(t[1])
            elif t[0] == "raw":
                self.bits(t[1], t[2])
            else:
                length, dist = t
                s, x = length_symbol(length, as284)
                lsym(257 + s); self.bits(x, LEXT[s])
                s, x = dist_symbol(dist)
                dsym(s); self.bits(x, DEXT[s])
        if eob:
            lsym(256)
        return self


def expand(tokens, before=b""):
    """what a list of literal and match tokens stands for, after `before` (the builder's OWN idea of the output: the tests use it only where
    zlib refuses a stream that the kernel accepts)"""
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            assert 1 <= dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(before):])


def tokens_size(tokens):
    return sum(1 if isinstance(t, int) else t[0] for t in tokens)


def used_symbols(tokens, len258_as_284=False):
    """-> (literal/length symbols incl. 256, distance symbols) that a token list needs, each most frequent first"""
    fl = {256: 1}; fd = {}
    for t in tokens:
        if isinstance(t, int):
            fl[t] = fl.get(t, 0) + 1
        else:
            s = 257 + length_symbol(t[0], len258_as_284)[0]; fl[s] = fl.get(s, 0) + 1
            s = dist_symbol(t[1])[0]; fd[s] = fd.get(s, 0) + 1
    return sorted(fl, key=lambda s: (-fl[s], s)), sorted(fd, key=lambda s: (-fd[s], s))


def plain_lengths(tokens, nlen=None, ndist=None, len258_as_284=False):
    """complete, balanced literal/length and distance code lengths for a token list (HLIT / HDIST as small as the symbols allow unless given)"""
    ls, ds = used_symbols(tokens, len258_as_284)
    nlen = nlen or max(257, max(ls) + 1); ndist = ndist or max(1, max(ds + [0]) + 1)
    if ndist == 1 and len(ds) <= 1:
        return complete_code(nlen, ls), [1]
    return complete_code(nlen, ls), (complete_code(ndist, ds) if ds else [0] * ndist)


def random_tokens(rng, n_tokens, literals, lengths, dists, start=0, limit=65000):
    """literals and matches drawn from the given lists (a match only where its distance is available), `start` bytes already out"""
    out = []; op = start
    for _ in range(n_tokens):
        if op > start + 2 and rng.random() < 0.35:
            d = rng.choice(dists); l = rng.choice(lengths)
            if d <= op and op + l <= limit:
                out.append((l, d)); op += l
                continue
        if op < limit:
            out.append(rng.choice(literals)); op += 1
    return out


def _bytes(rng, n, alphabet=None):
    return bytes(rng.choice(alphabet) for _ in range(n)) if alphabet else bytes(rng.getrandbits(8) for _ in range(n))


# ------------------------------------------------------------------ the catalogue of valid corner streams
OVERLAP_DISTS = tuple(range(1, 20)) + (31, 32, 33, 63, 64, 65)
OVERLAP_LENS = (3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 258)
ALL_LENGTHS = tuple(sorted(set(LBASE) | {b + (1 << e) - 1 for b, e in zip(LBASE, LEXT)}))        # both ends of every length symbol


def _deep_litlen(nlen):
    """15 bits deep: literals 0..5 in 1..6 bits, end-of-block in 7, and 256 symbols of 15 bits -- every length symbol among them"""
    if nlen == 285:
        deep = list(range(6, 234)) + list(range(257, 285))
    else:
        deep = list(range(6, 233)) + list(range(257, 286))
    return assign_lengths(nlen, list(range(6)) + [256] + deep, deep_lengths(263, 15))


def catalogue():
    """{name: raw DEFLATE stream}: valid streams (zlib's decoder accepts every one) from the parts of RFC 1951 that zlib's encoder leaves alone"""
    rng = random.Random(1951)
    C = {}

    # --- code-length runs across the literal/length | distance boundary
    lits = list(b"abcdefghijklmnop")
    toks = random_tokens(rng, 400, lits, [3, 4, 5], [1, 2, 3, 4, 5, 6, 7])
    for name, fixed_ll, want in (("cl_run16_first_copy_is_last_litlen", {257: 3, 258: 4, 259: 4}, (16, 259, 264)),
                                 ("cl_run16_across_boundary", {256: 3, 257: 4, 258: 4, 259: 4}, (16, 258, 264))):
        ll = fill_code(260, fixed_ll, [s for s in lits + [256] if s not in fixed_ll])
        dl = fill_code(7, {0: 4, 1: 4, 2: 4, 3: 4}, [4, 5, 6])
        assert want in ops_spans(rle_ops(ll + dl)), name
        C[name] = Deflate().dynamic(toks, True, ll, dl).done()
    # a zero run (symbol 17) over the last literal/length lengths and the first distance lengths
    ll = complete_code(265, lits + [256, 257, 258, 259, 260, 261]); dl = [0, 0, 0] + complete_code(5, [0, 1, 2, 3, 4])
    assert (17, 262, 268) in ops_spans(rle_ops(ll + dl))
    C["cl_run17_across_boundary"] = Deflate().dynamic(random_tokens(rng, 300, lits, [3, 4, 5, 6, 7], [4, 5, 7, 9, 13, 16]), True, ll, dl).done()
    # symbol 18 across the boundary.  A stream with an end-of-block code has at most 29 + 30 zero lengths after it, so the longest run that can cross is 59 ..
    toks = [rng.choice(lits) for _ in range(200)]
    ll = complete_code(286, lits + [256]); dl = [0] * 30
    assert (18, 257, 316) in ops_spans(rle_ops(ll + dl))
    C["cl_run18_across_boundary_59"] = Deflate().dynamic(toks, True, ll, dl).done()
    # .. and the full 138 (extra bits 127) inside the literals, followed by a second run that crosses
    ll = complete_code(286, [0, 1, 2, 141, 142, 143, 256]); dl = [0] * 12 + [1, 1]
    sp = ops_spans(rle_ops(ll + dl))
    assert (18, 3, 141) in sp and (18, 257, 298) in sp
    C["cl_run18_138_then_across_boundary"] = Deflate().dynamic([rng.choice([0, 1, 2, 141, 142, 143]) for _ in range(60)], True, ll, dl).done()

    # --- 15-bit codes: literals, length symbols and distance symbols at the deepest level, cold table slots up to 262
    dl15 = assign_lengths(30, list(range(30)), deep_lengths(30, 15))
    for name, nlen in (("deep15_hlit285", 285), ("deep15_hlit286_hdist30", 286)):
        ll = _deep_litlen(nlen)
        deep_lits = [s for s in range(256) if ll[s] == 15]
        toks = random_tokens(rng, 2500, list(range(6)) * 8 + deep_lits, ALL_LENGTHS, [DBASE[s] for s in range(30)] + [b + (1 << e) - 1 for b, e in zip(DBASE, DEXT)])
        as284 = nlen == 285          # no symbol 285 in this one: its 258s go out as 284 + extra bits 31
        assert any(not isinstance(t, int) and t[1] > 16384 for t in toks)
        assert len(set(length_symbol(t[0], as284)[0] for t in toks if not isinstance(t, int))) == 29 - as284
        C[name] = Deflate().dynamic(toks, True, ll, dl15, len258_as_284=as284).done()
    toks = [rng.choice(lits) for _ in range(100)]
    C["hlit257_hdist1"] = Deflate().dynamic(toks, True, complete_code(257, lits + [256]), [1]).done()

    # --- unusual distance codes
    toks = random_tokens(rng, 200, lits, [3, 4, 10, 258], [1])
    C["dist_one_symbol_of_length_1"] = Deflate().dynamic(toks, True, plain_lengths(toks)[0], [1]).done()
    toks = [rng.choice(lits) for _ in range(300)]
    C["dist_no_symbol_hdist5"] = Deflate().dynamic(toks, True, complete_code(257, lits + [256]), [0] * 5).done()
    C["dist_no_symbol_hdist30"] = Deflate().dynamic(toks, True, complete_code(257, lits + [256]), [0] * 30).done()
    head = _bytes(rng, 32768)
    toks = random_tokens(rng, 150, lits, [3, 17, 64, 258], [24577, 24578, 30000, 32767, 32768], start=32768)
    assert sum(1 for t in toks if not isinstance(t, int)) > 20
    C["dist_only_symbol_29"] = Deflate().stored(head, False).dynamic(toks, True, plain_lengths(toks)[0], [0] * 29 + [1]).done()

    # --- a literal/length code that is only the end-of-block symbol
    C["litlen_only_end_of_block"] = Deflate().stored(b"only the end-of-block code follows", False).dynamic([], True, [0] * 256 + [1], [0]).done()
    C["litlen_only_end_of_block_twice"] = Deflate().dynamic([], False, [0] * 256 + [1], [0]).dynamic([], False, [0] * 256 + [1], [0, 0]).fixed(list(b"xyz"), True).done()

    # --- length 258 as symbol 284 + extra bits 31
    toks = [65, (258, 1), 66, 67, (258, 2), (258, 260), 68, (258, 1)]
    C["len258_as_284_fixed"] = Deflate().fixed(toks, True, len258_as_284=True).done()
    ll, dl = plain_lengths(toks, len258_as_284=True)
    C["len258_as_284_dynamic"] = Deflate().dynamic(toks, True, ll, dl, len258_as_284=True).done()
    C["len258_as_284_final_token"] = Deflate().fixed([65, 66, 67, (258, 3)], True, len258_as_284=True).done()

    # --- unusual block sequences
    C["empty_stored_blocks"] = (Deflate().stored(b"", False).stored(b"", False).stored(b"between empties", False).stored(b"", False)
                                .fixed(list(b"fixed"), False).stored(b"", False).stored(b"", True).done())
    C["only_empty_stored_then_one_byte"] = Deflate().stored(b"", False).stored(b"z", False).stored(b"", True).done()
    C["empty_fixed_blocks_not_final"] = (Deflate().fixed([], False).fixed([], False).fixed([], False).fixed(list(b"after three empty fixed blocks"), False)
                                         .fixed([], False).stored(b"!", False).fixed([], False).fixed([], True).done())
    for k in range(8):          # a fixed block of 3 + 8 * 8 + 9 * k + 7 bits: the stored block's header starts at every bit offset
        d = Deflate().fixed(list(b"ABCDEFGH") + [200 + i for i in range(k)], False)
        off = d.bit_length() % 8
        C["stored_at_bit_offset_%d_after_fixed" % off] = d.stored(_bytes(rng, 37 + k), True).done()
    assert sum(1 for n in C if n.startswith("stored_at_bit_offset_")) == 8
    toks = random_tokens(rng, 500, lits, [3, 4, 5, 9, 30], [1, 2, 3, 8, 20, 100])
    ll, dl = plain_lengths(toks)
    for k in range(8):
        d = Deflate().dynamic(toks + [rng.choice(lits) for _ in range(k)], False, ll, dl)
        C["ends_in_stored_after_dynamic_%d" % k] = d.stored(_bytes(rng, 300), False).stored(_bytes(rng, 11), True).done()

    # --- the longest distance, and a distance that reaches the member's first byte
    C["dist_32768_equals_op"] = Deflate().stored(head, False).fixed([(258, 32768), 1, 2, 3, (100, 32768), (3, 32768)], True).done()
    C["dist_equals_op_small"] = Deflate().fixed([120, (3, 1)], True).done()
    C["dist_equals_op_5"] = Deflate().fixed(list(b"hello") + [(20, 5), 33], True).done()
    C["dist_equals_op_64"] = Deflate().fixed(list(_bytes(rng, 64)) + [(258, 64), (65, 322)], True).done()

    # --- overlapping copies: every (distance, length) pair mid-member (all lengths of one distance in one member) and as the member's last token
    for d in OVERLAP_DISTS:
        toks = list(_bytes(rng, d + 3))
        for l in OVERLAP_LENS:
            toks += [(l, d)] + list(_bytes(rng, 2))
        toks += list(_bytes(rng, 70))
        C["overlap_mid_d%d" % d] = Deflate().fixed(toks, True).done()
        for l in OVERLAP_LENS:
            toks = list(_bytes(rng, d + (l + d) % 7)) + [(l, d)]
            C["overlap_final_d%d_l%d" % (d, l)] = Deflate().fixed(toks, True).done()
    # far distances as the last token (the widest copy), in a dynamic block
    for l in OVERLAP_LENS:
        toks = list(_bytes(rng, 700, b"ACGT")) + [(l, 100 + l), 65, (l, 699)]
        ll, dl = plain_lengths(toks)
        C["far_final_l%d" % l] = Deflate().dynamic(toks, True, ll, dl).done()
    return C


def alignment_streams():
    """[(name, stream)]: a dynamic, a fixed and a stored member for every compressed size mod 16 (48 streams); the test puts each at every src & 15"""
    rng = random.Random(16)
    out = []
    lits = list(b"ACGTN")
    for kind in ("dynamic", "fixed", "stored"):
        have = {}
        n = 40
        while len(have) < 16:
            n += 1
            toks = random_tokens(rng, n, lits, [3, 4, 5, 19, 40], [1, 2, 5, 9, 17])
            if kind == "dynamic":
                ll, dl = plain_lengths(toks)
                s = Deflate().dynamic(toks, True, ll, dl).done()
            elif kind == "fixed":
                s = Deflate().fixed(toks, True).done()
            else:
                s = Deflate().stored(expand(toks), True).done()
            have.setdefault(len(s) % 16, s)
            assert n < 2000
        out += [("%s_size%%16=%d" % (kind, r), have[r]) for r in range(16)]
    return out


# ------------------------------------------------------------------ streams that must be refused, and those the kernel accepts although zlib does not
def invalid_streams():
    """[(name, stream, ISIZE the member claims, K_inflate's status code)]; zlib refuses every one (or gives another size than ISIZE)"""
    lits = list(b"abcdefgh")
    ok_ll = complete_code(257, lits + [256])
    body = list(b"abcabc")
    R = []
    R.append(("block_type_3", BitWriter().bits(1, 1).bits(3, 2).bits(0, 13).done(), 4, 1))
    s = bytearray(Deflate().stored(b"abcd", True).done()); s[3] ^= 0x01
    R.append(("stored_len_nlen_mismatch", bytes(s), 4, 1))
    R.append(("hlit_287", Deflate().dynamic(body, True, complete_code(287, lits + [256]), [1]).done(), 6, 6))
    R.append(("hlit_288", Deflate().dynamic(body, True, complete_code(288, lits + [256]), [1]).done(), 6, 6))
    R.append(("hdist_31", Deflate().dynamic(body, True, ok_ll, [0] * 30 + [1]).done(), 6, 6))
    R.append(("hdist_32", Deflate().dynamic(body, True, ok_ll, [0] * 31 + [1]).done(), 6, 6))
    cl = [0] * 19; cl[0] = 1; cl[1] = 1; cl[2] = 2; cl[17] = 2; cl[18] = 2
    ll2 = assign_lengths(257, [97, 98, 99, 256], [2, 2, 2, 2])
    R.append(("oversubscribed_code_length_code", Deflate().dynamic(body, True, ll2, [1], cl_lengths=cl).done(), 6, 6))
    R.append(("oversubscribed_litlen", Deflate().dynamic(body, True, assign_lengths(257, [97, 98, 99, 256], [1, 2, 2, 2]), [1]).done(), 6, 6))
    R.append(("oversubscribed_litlen_15", Deflate().dynamic([97], True, assign_lengths(257, [97, 256] + list(range(100, 228)), [1, 1] + [8] * 128), [1]).done(), 1, 6))
    R.append(("oversubscribed_dist", Deflate().dynamic(body, True, ok_ll, [1, 1, 1]).done(), 6, 6))
    R.append(("oversubscribed_dist_deep", Deflate().dynamic(body, True, ok_ll, [1, 2, 3, 4, 4, 15]).done(), 6, 6))
    R.append(("no_end_of_block_code", Deflate().dynamic(body, True, complete_code(257, lits), [1], eob=False).done(), 6, 6))
    ops = [(16, 0)] + rle_ops(ok_ll[3:] + [1])
    R.append(("repeat16_first", Deflate().dynamic(body, True, ok_ll, [1], cl_ops=ops).done(), 6, 6))
    for sym, extra, name in ((16, 3, "repeat16_past_the_end"), (17, 0, "repeat17_past_the_end"), (18, 127, "repeat18_past_the_end")):
        ops = rle_ops(ok_ll[:256]) + [(ok_ll[256], None), (sym, extra)]          # one length (the distance code's) is left, and the repeat writes at least three
        R.append((name, Deflate().dynamic(body, True, ok_ll, [1], cl_ops=ops).done(), 6, 6))
    # a bit pattern that an incomplete code leaves unused: the one-bit distance code 0, and the stream says 1
    toks = [97, ("lsym", 257), ("raw", 1, 1), 98]
    R.append(("pattern_outside_incomplete_dist_code", Deflate().dynamic(toks, True, complete_code(258, lits + [256, 257]), [1]).done(), 5, 2))
    R.append(("pattern_with_no_dist_code_at_all", Deflate().dynamic([97, ("lsym", 257), ("raw", 0, 1), 98], True, complete_code(258, lits + [256, 257]), [0, 0]).done(), 5, 2))
    for s in (286, 287):
        R.append(("fixed_length_symbol_%d" % s, Deflate().fixed([97, ("lsym", s), ("dsym", 0), 98], True).done(), 5, 2))
    for s in (30, 31):
        R.append(("fixed_distance_symbol_%d" % s, Deflate().fixed([97, ("lsym", 257), ("dsym", s), 98], True).done(), 5, 2))
    R.append(("distance_one_beyond_op", Deflate().fixed([97, (3, 2)], True).done(), 4, 3))
    R.append(("distance_one_beyond_op_far", Deflate().fixed(list(b"x" * 300) + [(3, 301)], True).done(), 303, 3))
    R.append(("distance_at_op_0", Deflate().fixed([(3, 1)], True).done(), 3, 3))
    R.append(("literal_past_isize", Deflate().fixed(list(b"abcdefghi"), True).done(), 8, 4))
    R.append(("match_past_isize", Deflate().fixed([97, (8, 1)], True).done(), 8, 4))
    R.append(("match_far_past_isize", Deflate().fixed(list(b"q" * 70) + [(258, 65)], True).done(), 327, 4))
    R.append(("stored_past_isize", Deflate().fixed([97], False).stored(b"1234567", True).done(), 7, 4))
    R.append(("one_byte_short_of_isize", Deflate().fixed(list(b"abcdefg"), True).done(), 8, 5))
    R.append(("match_one_byte_short_of_isize", Deflate().fixed([97, (40, 1)], True).done(), 42, 5))
    return R


def lenient_streams():
    """[(name, stream, the bytes it stands for)]: streams zlib's decoder refuses and K_inflate accepts (DESIGN.md lists them); the expected bytes are
    the builder's token expansion, since zlib gives none"""
    lits = list(b"lenity")
    R = []
    # an incomplete code-length code: fewer than eight symbols, three bits each
    toks = list(b"lenitytinelyline")
    ll = complete_code(257, lits + [256])
    ops = rle_ops(ll + [1])
    syms = sorted(set(s for s, _ in ops))
    assert 4 < len(syms) < 8, syms
    cl = assign_lengths(19, syms, [3] * len(syms))
    R.append(("incomplete_code_length_code", Deflate().dynamic(toks, True, ll, [1], cl_lengths=cl).done(), expand(toks)))
    # the only literal/length code (end-of-block) is two bits long
    R.append(("single_litlen_code_of_2_bits", Deflate().stored(b"stored first", False).dynamic([], True, [0] * 256 + [2], [0]).done(), b"stored first"))
    # the only distance code is three bits long
    toks = [108, (5, 1), 101, (9, 1), (258, 1)]
    ll, _ = plain_lengths(toks)
    R.append(("single_dist_code_of_3_bits", Deflate().dynamic(toks, True, ll, [3]).done(), expand(toks)))
    # the stream is cut before its last bits (here: inside the end-of-block code); what follows the member in memory is zero and reads as that code
    s = Deflate().fixed([108], True).done()
    assert len(s) == 3
    R.append(("cut_inside_end_of_block", s[:2], b"l"))
    # a member whose ISIZE is 0 is not decoded at all, whatever its bytes say (here: block type 3)
    R.append(("isize_0_is_not_decoded", b"\x07", b""))
    return R
