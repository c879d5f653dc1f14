// K_map: read -> het-variant allele mapper for gfx950 (MI355X).
//
// Computes what phaser/read_variant_map.py:3-258 computes (do_read_variant_map -> split_read ->
// identify_allele), restated as a stateless rule per (record, N-split segment, variant) -- SURVEY.md 3.3:
//   emit iff  seg_start <= var.pos - POS  and  var.pos - POS + ref_len <= seg_start + len(pseudo_read)
//   and the extracted text is neither "" nor "N".
// Integer / branch work on an HBM-resident structure of arrays; no MFMA.
//
// Launch shape: one 128-thread workgroup per tile of 256 consecutive (coordinate-sorted) reads (template
// parameters; 64..256 threads x 2..4 reads per lane were swept on MI355X, 128 x 2 is fastest), two
// reads per lane strided by the workgroup size so every streaming load (pos, cigar_off, seq_off, cigar words) is coalesced.
// Per tile (k_map):
//   1. LDS staging with coalesced block-wide loads: the tile's cigar_off slice, its contiguous run of packed
//      CIGAR words, and the het-SNP window that starts at lower_bound(vpos, POS of the tile's first read),
//      sized by a pre-pass (k_tile_window) to what the tile's reads reach without introns; lanes binary-search
//      the window per aligned run and fall through to global memory only for introns reaching past it,
//   2. records made of one aligned run (the common case) stay in registers: a branch-free LDS binary search
//      with a tile-uniform trip count yields (first het SNP, count); their seq/qual bytes are gathered in a
//      per-lane `for o < count` loop, so iteration o is one gather for every lane that has an o-th SNP,
//   3. spliced / gapped / clipped records are re-packed densely and walk their CIGAR out of LDS; their
//      candidates go to an LDS buffer tagged (read, ordinal) and are resolved by all lanes at once
//      (seq/qual bytes are touched only under a variant: two bytes per call),
//   4. a wave shuffle scan + LDS combine turns per-read call counts into offsets and the calls are flushed in
//      exact mapper order into the tile's slot of a staging area (tile x slot_cap calls); a tile whose
//      candidates overflow the LDS buffer resolves its complex records in-lane instead.
// k_chunk_scan / k_chunk_base prefix-sum the per-tile totals; k_compact copies every slot to its final
// offset, so the call list is in mapper order with no inter-workgroup dependency inside k_map (a
// decoupled look-back was measured 0.8 ms slower here: tiles finish faster than descriptors travel).
// A step is five launches (k_tile_window, k_map, k_chunk_scan, k_chunk_base, k_compact) and one host wait.  k_chunk_base also computes the per-shard
// totals and stores the words the host reads -- calls of the batch, densest tile, calls per shard, overflow cursor -- straight into their page-locked
// host image: no copy follows the last kernel.  (A submission of more than a million tiles has a sixth launch, k_shard_totals, for those.)
// A staged call has one of two forms, chosen by the host for the whole submission (stage_narrow_form, phz_stagepack.h):
//   * narrow: one 32-bit word, var[0:20) | rec[20:28) | code[28:32) -- when no shard asks for the text planes, a tile has at most 256 records and every
//     het-SNP table at most 2^20 entries (the headline step; what Engine.add_shards asks for).  k_map<.., NARROW> stores one dword per call, carries neither
//     the read offsets nor the inserted-text lookup to its flush and has no side planes; k_compact<false, true> loads one dword per call; the staging area is
//     4 bytes per slot;
//   * general: the 8-byte record of stage_put plus two side planes (16 bytes per slot) -- everything else, and PHZ_MAP_WIDE_STAGE=1.
// Slot indices, slot_cap, the overflow area, its cursor and the redo are the same in both.
#include "phz_internal.h"
#include "phz_lbound.h"
#include "phz_leanwalk.h"
#include "phz_stagepack.h"
#include "phz_stageload.h"
#include <assert.h>
#include <stdlib.h>
#include <string.h>

namespace {

#ifndef PHZ_MAP_WIN
#define PHZ_MAP_WIN 512
#endif
#ifndef PHZ_CIG_X2
#define PHZ_CIG_X2 5
#endif
#ifndef PHZ_CAND_X4
#define PHZ_CAND_X4 3
#endif
constexpr int MAP_WIN = PHZ_MAP_WIN;       // het-SNP positions staged per tile (max)

constexpr uint32_t OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_EQ = 7, OP_X = 8, OP_G = 9;

struct MapArgs {
    const int32_t *pos;
    const uint32_t *cigar_off, *cigar, *seq_off;
    const uint8_t *seq2, *qual;
    const uint8_t *bq;            // one byte per base (phz_reads.bq), or NULL
    int64_t n;
    const int32_t *vpos;
    int nv;
    int baseq;
    // staging slots: global tile t owns stage[t*slot_cap, (t+1)*slot_cap); one packed 8-byte record per call (stage_put):
    // one store per call here, one load in k_compact.  (The narrow instantiations index the same area as 32-bit words: phz_stagepack.h.)
    uint2 *stage;
    uint32_t *side;               // [2*slots] aux words that do not fit the packed record (insertions, offsets >= 2^16)
    int64_t slots;
    const int32_t *tile_w0;       // [4*ntiles]: window start, window length | complete flag, first CIGAR word, CIGAR word count
    int32_t *tile_total;          // [ntiles] calls per tile
    int slot_cap;
    int64_t ntiles;
    int dbg;          // ablation switches for profiling (PHZ_MAP_DBG env); 0 in production
    bool one;         // base and quality of a call from the one-byte plane `bq` (a compile-time constant of the instantiation, like dbg == 0)
    const struct ShardDev *shp;   // ONE instantiation: the shard record, read again by the rare escape (seq2 / qual stay out of the registers)
};

// one shard of a batch; the array lives in device memory for the duration of the launches
struct ShardDev {
    const int32_t *pos;
    const uint32_t *cigar_off, *cigar, *seq_off;
    const uint8_t *seq2, *qual;
    const uint8_t *bq;
    int64_t n;
    const int32_t *vpos;
    int nv, pad;
    int32_t *o_read, *o_var;          // final (dense, mapper-order) outputs of the shard
    uint8_t *o_code;
    uint32_t *o_aux0, *o_aux1;
    int64_t cap;
};

// all shards of one submission share ONE grid: global tile T belongs to the shard s with tile0[s] <= T < tile0[s+1]
struct MapBatch {
    const ShardDev *shards;
    const int64_t *tile0;         // [n_shards + 1]
    int n_shards, baseq;
    uint2 *stage;                 // staging slots: global tile T owns [T*slot_cap, (T+1)*slot_cap)
    uint32_t *side; int64_t slots;
    int32_t *tile_w0;             // [4*ntiles]
    int32_t *tile_total;          // [ntiles]
    int slot_cap, dbg;
    int64_t ntiles;
    unsigned long long *prof;     // PHZ_MAP_DBG bit 2048 (profiling build of the kernel only): 8 clock stamps per tile
    // overflow area of the staging slots: a tile with more calls than slot_cap takes a stretch of [ovf->base, ovf->base + ovf->cap) (slot indices of the same
    // stage / side arrays) with one cursor step and leaves its first slot in ovf->tile_first[tile] (0xFFFFFFFF: the area was too small; the host redoes the
    // batch).  Behind ONE pointer, read by the rare tile that needs it: four more kernel arguments cost the kernel 50 scalar registers spilled to vector lanes
    const struct OvfArea *ovf;
};
struct OvfArea { uint32_t *tile_first; unsigned long long *cursor; long long base, cap; };

__device__ __forceinline__ int shard_of(const int64_t *tile0, int n_shards, int64_t T) {
    int lo = 0, hi = n_shards - 1;          // largest s with tile0[s] <= T
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (tile0[m] <= T) lo = m; else hi = m - 1;
    }
    return lo;
}

// the escape of the one-byte plane (a non-ACGT base or a phred above 62: one base in two thousand): the two planes, found through the shard record
__device__ __noinline__ int masked_base_escape(const MapArgs &a, uint32_t soff, int x) {
    const uint8_t *qual = a.shp->qual, *seq2 = a.shp->seq2;
    const uint32_t q = qual[(size_t)soff * 4 + x], s = (seq2[(size_t)soff + (x >> 2)] >> (2 * (x & 3))) & 3;
    if ((int)(q & 0x7f) < a.baseq) return 4;
    if (q & 0x80) return s == 0 ? 4 : 5;
    return (int)s;
}

struct VarWin {
    const int32_t *g;
    const int32_t *lds;
    int w0, nv, wlen;
    __device__ __forceinline__ int at(int i) const {
        unsigned d = (unsigned)(i - w0);
        return d < (unsigned)wlen ? lds[d] : g[i];
    }
    // first index in [lo, nv) whose position is >= key
    __device__ __forceinline__ int lower_bound(int lo, int key) const {
        int hi = nv;
        if (lo >= hi) return hi;
        // gallop first: the answer is almost always within a few entries of lo
        int step = 1;
        while (lo + step < hi && at(lo + step) < key) { lo += step; step <<= 1; }
        if (lo < hi && at(lo) >= key) return lo;
        int h = lo + step < hi ? lo + step : hi;
        int l = lo + 1;
        while (l < h) {
            int m = (l + h) >> 1;
            if (at(m) < key) l = m + 1; else h = m;
        }
        return l;
    }
};

// Staging record of one call: {variant index, rec[0:10) | code[10:14) | wide1[14] | wide0[15] | aux0[16:32)}.  aux0 (offset of the
// base in the read) below 2^16 and aux1 == 0 (no inserted text) is all but a handful of calls; the others keep the full words in the
// side planes at the same slot, so that the common call is 8 bytes out of k_map and 8 bytes into k_compact.
__device__ __forceinline__ void stage_put(uint2 *stage, uint32_t *side, int64_t slots, int64_t g, uint32_t var, uint32_t a0, uint32_t a1,
                                          uint32_t rec, uint32_t code) {
    const bool w0 = a0 >= 0x10000u, w1 = a1 != 0u;
    stage[g] = make_uint2(var, rec | (code << 10) | ((uint32_t)w1 << 14) | ((uint32_t)w0 << 15) | (w0 ? 0u : a0 << 16));
    if (w0) side[g] = a0;
    if (w1) side[slots + g] = a1;
}

// the tile's packed CIGAR words: LDS for the staged prefix, global beyond it
struct CigWin {
    const uint32_t *g;
    const uint32_t *lds;
    uint32_t c_begin, cap;
    __device__ __forceinline__ uint32_t at(uint32_t k) const {
        const uint32_t d = k - c_begin;
        return d < cap ? lds[d] : g[k];
    }
};

// LDS candidate buffer (one per workgroup): every (read, variant) pair that passes the position rule.  Eight bytes per entry plus a
// short side list (the buffer's size decides how many tiles a CU holds, and the kernel's time follows the residency): the variant as a
// 16-bit offset from the tile's window start, the base's read offset in 16 bits, inserted text -- one candidate in hundreds -- in the side
// list.  What does not fit those widths (a variant 65,535 entries beyond the window start, a base beyond offset 65,534, more than
// CAND_INS insertion candidates in a tile) flags the buffer as overflowed: the tile then takes the in-lane fallback, which needs no buffer.
#ifndef PHZ_CAND_INS
#define PHZ_CAND_INS 16
#endif
constexpr int CAND_INS = PHZ_CAND_INS;
constexpr uint32_t KEY_HAS_INS = 0x4000u;
struct CandBuf {
    uint32_t *key;    // local read index << 16 | lean-origin << 15 | has inserted text << 14 | ordinal within the read << 8 | code (filled by the resolve phase)
    uint16_t *var;    // variant index - w0
    uint16_t *x0;     // read offset of the base, 0xFFFF = none (deleted base)
    unsigned long long *ins;      // slot << 32 | (offset << 12 | length) of the inserted text
    int *n;           // candidates appended; > cap (or an ordinal >= 32) sends the tile down the in-lane fallback
    int *nins;
    int cap, w0;
};
__device__ __forceinline__ void cand_put(const CandBuf &cb, int slot, uint32_t key, int var, uint32_t x0, uint32_t x1) {
    const uint32_t dv = (uint32_t)(var - cb.w0);
    bool wide = dv >= 0xFFFFu || (x0 != 0xFFFFFFFFu && x0 >= 0xFFFFu);
    if (x1 != 0u) {
        const int t = atomicAdd(cb.nins, 1);
        if (t < CAND_INS) cb.ins[t] = ((unsigned long long)(uint32_t)slot << 32) | x1; else wide = true;
        key |= KEY_HAS_INS;
    }
    if (wide) atomicOr(cb.n, 1 << 30);
    cb.key[slot] = key;
    cb.var[slot] = (uint16_t)dv;
    cb.x0[slot] = (uint16_t)(x0 == 0xFFFFFFFFu ? 0xFFFFu : x0);
}
__device__ __forceinline__ uint32_t cand_x0(const CandBuf &cb, int e) { const uint32_t v = cb.x0[e]; return v == 0xFFFFu ? 0xFFFFFFFFu : v; }
__device__ __forceinline__ uint32_t cand_x1(const CandBuf &cb, int e, uint32_t key) {
    if (!(key & KEY_HAS_INS)) return 0u;
    const int m = *cb.nins < CAND_INS ? *cb.nins : CAND_INS;
    for (int t = 0; t < m; t++) { const unsigned long long w = cb.ins[t]; if ((int)(w >> 32) == e) return (uint32_t)w; }
    return 0u;
}

// experiment (PHZ_MAP_DBG bit 1024, timing only -- wrong bases): the byte that holds a base's two bits is read from the quality plane, inside the
// 4-byte group of its quality byte, i.e. what a layout with both in one memory sector would fetch
#define PHZ_SEQ_BYTE(a, soff, x) (((a).dbg & 1024) ? (a).qual[(size_t)(soff) * 4 + ((x) | 3)] : (a).seq2[(size_t)(soff) + ((x) >> 2)])
// Base and quality of a call from ONE byte (phz_reads.bq: base << 6 | min(phred, 62), 63 = escape to the two planes): one 128-byte line per call instead of two.
// The ONE instantiations of the kernel read it (every shard of the submission carries the plane); A/B on the profiling instantiation: PHZ_MAP_DBG bit 4096
// (tools/ab_kmap_oneplane.py: -3.7 % on the profiling instantiation, -0.1 % on the production one, call lists identical)
#define PHZ_ONEPLANE(a) ((a).one)
__device__ __forceinline__ int masked_base_two(const MapArgs &a, uint32_t soff, int x) {
    const uint32_t q = a.qual[(size_t)soff * 4 + x], s = (a.seq2[(size_t)soff + (x >> 2)] >> (2 * (x & 3))) & 3;
    if ((int)(q & 0x7f) < a.baseq) return 4;
    if (q & 0x80) return s == 0 ? 4 : 5;
    return (int)s;
}
__device__ int masked_base_escape(const MapArgs &a, uint32_t soff, int x);
__device__ __forceinline__ int sym_from_bq(const MapArgs &a, uint32_t soff, int x, uint32_t b) {
    const uint32_t q6 = b & 63u;
    if (q6 == 63u) return a.qual ? masked_base_two(a, soff, x) : masked_base_escape(a, soff, x);
    return (int)q6 < a.baseq ? 4 : (int)(b >> 6);
}
// symbol of read base x after baseq masking: 0..3 = ACGT, 4 = 'N', 5 = other IUPAC character
__device__ __forceinline__ int masked_base(const MapArgs &a, uint32_t soff, int x) {
    if (PHZ_ONEPLANE(a)) return sym_from_bq(a, soff, x, a.bq[(size_t)soff * 4 + x]);
    uint32_t q = a.qual[(size_t)soff * 4 + x];
    uint32_t s = (PHZ_SEQ_BYTE(a, soff, x) >> (2 * (x & 3))) & 3;
    if ((int)(q & 0x7f) < a.baseq) return 4;
    if (q & 0x80) return s == 0 ? 4 : 5;
    return (int)s;
}

// MODE 0: position rule only, candidates appended to the LDS buffer (no global loads in the divergent walk)
// MODE 1: count calls, resolving bases in-lane (fallback)      MODE 2: emit calls in-lane (fallback)
// NARROW (MODE 2 only): the call is staged as the 4-byte word of phz_stagepack.h
template <int MODE, bool NARROW = false>
__device__ int walk_read(const MapArgs &a, const VarWin &vw, const CigWin &cw, const CandBuf &cb, int j, int64_t r, int pos,
                         uint32_t c0, uint32_t c1, uint32_t soff, int64_t out_base, int64_t out_limit) {
    int i = vw.lower_bound(vw.w0, pos);
    if (i >= vw.nv) return 0;
    int cnt = 0;
    int gpos = 0, rpos = 0, seg_start = 0, plen = 0, seg_rpos = 0;
    uint32_t seg_op = c0;
    for (uint32_t k = c0; k < c1; k++) {
        uint32_t w = cw.at(k);
        const int len = (int)(w >> 4);
        const uint32_t op = w & 15;
        if (op == OP_M || op == OP_EQ || op == OP_X || op == OP_D) {
            const int lo = pos + seg_start + plen, hi = lo + len;
            if (i < vw.nv && vw.at(i) < lo) i = vw.lower_bound(i, lo);
            while (i < vw.nv && !(a.dbg & 16)) {
                const int vp = vw.at(i);
                if (vp >= hi) break;
                const int p = vp - pos - seg_start;            // index into the segment's pseudo read
                const int rb = rpos + (p - plen);              // read offset of that base (M runs only)
                // insertion recorded under key == p in THIS segment (key is read-relative: quirk kept)
                int ioff = 0, ilen = 0;
                if (c1 - c0 > 1) {
                    int g2 = seg_start, r2 = seg_rpos;
                    for (uint32_t k2 = seg_op; k2 < c1; k2++) {
                        uint32_t w2 = cw.at(k2);
                        const int l2 = (int)(w2 >> 4);
                        const uint32_t o2 = w2 & 15;
                        if (o2 == OP_N) break;
                        if (o2 == OP_M || o2 == OP_EQ || o2 == OP_X) { g2 += l2; r2 += l2; }
                        else if (o2 == OP_D || o2 == OP_G) g2 += l2;
                        else if (o2 == OP_I) { if (g2 - 1 == p) { ioff = r2; ilen = l2; } r2 += l2; }
                        else if (o2 == OP_S) r2 += l2;
                    }
                }
                const int nchars = (op != OP_D) + ilen;
                if (nchars > 0) {
                    const uint32_t x0 = op != OP_D ? (uint32_t)rb : 0xFFFFFFFFu;
                    const uint32_t x1 = ilen > 0 ? (((uint32_t)ioff << 12) | (uint32_t)(ilen > 4095 ? 4095 : ilen)) : 0u;
                    if (MODE == 0) {
                        // code 7 = one character, to be resolved from seq/qual; 4 = composite text (always a call)
                        const int slot = cnt < 32 ? atomicAdd(cb.n, 1) : (atomicOr(cb.n, 1 << 30), 1 << 30);      // OR, not ADD: thousands of these in one tile must not wrap the counter
                        if (slot < cb.cap) cand_put(cb, slot, ((uint32_t)j << 16) | ((uint32_t)cnt << 8) | (nchars == 1 ? 7u : 4u), i, x0, x1);
                        cnt++;
                    } else {
                        int code = 4;
                        if (nchars == 1) {
                            const int s = masked_base(a, soff, op != OP_D ? rb : ioff);
                            code = s < 4 ? s : (s == 4 ? -1 : 4);
                        }
                        if (code >= 0) {
                            if (MODE == 2) {
                                const int64_t o = out_base + cnt;
                                if (o < out_limit) {
                                    if (NARROW) reinterpret_cast<uint32_t *>(a.stage)[o] = stage4_pack((uint32_t)i, (uint32_t)j, (uint32_t)code);
                                    else stage_put(a.stage, a.side, a.slots, o, (uint32_t)i, x0, x1, (uint32_t)j, (uint32_t)code);
                                }
                            }
                            cnt++;
                        }
                    }
                }
                i++;
            }
            plen += len; gpos += len;
            if (op != OP_D) rpos += len;
        } else if (op == OP_I || op == OP_S) {
            rpos += len;
        } else if (op == OP_N) {
            gpos += len; seg_start = gpos; plen = 0; seg_op = k + 1; seg_rpos = rpos;
        } else if (op == OP_G) {
            gpos += len;
        }
    }
    return cnt;
}

// Lean walker for multi-op records: any mix of M / = / X / D / N / S / H / P and up to two insertions, every run inside the staged
// window and every CIGAR word in LDS.  Same rule as walk_read<0> (candidates appended to the LDS buffer, position rule only), organised
// for a short, branch-light instruction stream -- this phase is VALU-issue bound, and a wave pays the stream once whatever its lanes do:
//   * ONE pass over the ops: the window search runs unconditionally (empty interval for ops that are not runs), wave-uniform ballots
//     skip the insertion bookkeeping and the search when no lane needs them;
//   * what the pass cannot express ('G' ops, a third insertion, an insertion not directly after a non-empty reference-consuming op,
//     a run beyond the window) is found on the way: the record is POISONED (its lean-origin candidates, key bit 15, are dropped by
//     the resolve phase) and left to the general walker.
// (Tried and dropped, round 3: a second, bookkeeping-free walker for the pure spliced shapes M N M / M N M N M, listed apart.  It runs
// in half the instructions of this one, but a 256-record tile has ~80 multi-op records: split by shape they fill three partial waves
// instead of two, the instruction total does not move and the extra barrier lengthens the tile: 1.57 ms against 1.28 ms.)
// Insertions follow the reference's keying (key = genome offset - 1 at the I op, looked up SEGMENT-relative): while seg_start is 0
// that is the last base of the op before the I (found by peeking at the next op); after an N the key lands seg_start bases further
// on, i.e. in a later run of the same segment (carried forward in two register slots, the later insertion wins).
// Lower bound over the staged window: window_lower_bound<D> of phz_lbound.h, a fully unrolled chain of D halving steps and a closing probe over a
// window padded with INT_MAX up to 2^D entries -- five issue slots per probe (LDS read with an immediate offset, wait, subtract, shift, and-or), no
// compare / select pair (its VCC hazard costs an s_nop per probe) and nothing on the scalar unit between probes.  The depth is a template
// parameter: a tile belongs to one of a few DEPTH CLASSES by its window length (wave-uniform, computed once per tile); the bracket search of phase 1a
// picks its class with one scalar if/else (lds_lower_bound), the lean walker is instantiated once per class (walk_lean<D>).  (Until round 10 the depth
// was the entry point of a `switch` with fall-through cases: the compiler turned that ladder into scalar compares, branches and 64-bit mask moves
// BETWEEN the probes, 25-30 scalar instructions per search on the busier port.)
// Two classes, from the staged window lengths of the whole-genome sample (profiles/r10/kmap_search_ab.txt: 75 % of the tiles stage at most 64 entries, 25 %
// 65..128, one in a thousand more): D = 7, whose padding is one round of the 128-thread workgroup, and the full window.  (D = 6 saves three quarters of
// the tiles one probe but sends the fourth quarter through the ten probes and four padding rounds of the full window: the same instruction total, more LDS
// traffic; a third class costs the production kernel a spilled vector register -- the first probe of every class is hoisted out of the op loop.)
#ifndef PHZ_WIN_DSMALL
#define PHZ_WIN_DSMALL 7
#endif
constexpr int WIN_DMAX = 31 - __builtin_clz((unsigned)MAP_WIN);                      // the class of the largest window: 2^WIN_DMAX == MAP_WIN entries
constexpr int WIN_DSMALL = WIN_DMAX < PHZ_WIN_DSMALL ? WIN_DMAX : PHZ_WIN_DSMALL;    // the class of the typical tile
static_assert(MAP_WIN >= 2 && MAP_WIN <= 1024 && (MAP_WIN & (MAP_WIN - 1)) == 0, "MAP_WIN: a power of two up to 1024");
__device__ __forceinline__ int window_depth(int wlen) {          // depth class of a window: the chain reaches every count <= 2^depth >= wlen
    return wlen <= (1 << WIN_DSMALL) ? WIN_DSMALL : WIN_DMAX;
}
// s_vpos is padded with INT_MAX up to 2^wdepth entries; a negative key (the bracket's "no record" sentinel, a wrapped position) yields 0
__device__ __forceinline__ int lds_lower_bound(const int32_t *w, int wdepth, int key) {
    return wdepth == WIN_DSMALL ? window_lower_bound<WIN_DSMALL>(w, key) : window_lower_bound<WIN_DMAX>(w, key);
}

// D: the depth class of the tile's window (one instantiation per class, picked once per tile by the caller: no if/else at the search).
// The position rule of one op -- interval, flags, insertion keys, state update, poison -- is lean_step of phz_leanwalk.h; every per-lane flag is an
// integer there (a per-lane bool carried round a divergent loop is a lane mask on the scalar unit, three instructions per update and loop level).
// The trip count is the wave's longest record: lanes whose record has ended walk the neutral word, so the loop's exit is one ballot and no lane
// leaves early; the hit loop is entered only when some lane of the wave has a het SNP under its run (one LDS read, a compare and a ballot).
template <int D>
__device__ bool walk_lean(const int32_t *s_vpos, int wlen, int w0, const uint32_t *s_cig, uint32_t c_begin, uint32_t cig_cap,
                          const CandBuf &cb, uint32_t *s_poison, int j, int pos, uint32_t c0, uint32_t c1, long long cover, int dbg) {
    if (c1 - c_begin > cig_cap) return false;
    LeanWalk s; lean_init(s);
    const uint32_t nops = c1 - c0;
    const uint32_t *cig = s_cig + (c0 - c_begin);
    for (uint32_t u = 0; __builtin_amdgcn_ballot_w64(u < nops) != 0; u++) {
        const uint32_t w = u < nops ? cig[u] : LEAN_NEUTRAL;
        LeanOp o = lean_step(s, w, pos, (dbg & 64) ? 0x7fffffffffffffffll : cover);
        if (dbg & 64) { o.search = 0; o.hi = o.lo; }
        if (__builtin_amdgcn_ballot_w64(o.search != 0) != 0) {
            int i = window_lower_bound<D>(s_vpos, o.lo);
            // (entries [wlen, 2^D) are INT_MAX, never below hi; i == 2^D == MAP_WIN, one past the array, only when wlen == MAP_WIN: the index wraps, i < wlen decides)
            int vp = s_vpos[i & (MAP_WIN - 1)];
            bool hit = i < wlen && vp < o.hi && !(dbg & 128);
            if (__builtin_amdgcn_ballot_w64(hit) != 0) {
                while (hit) {
                    const uint32_t x1 = s.seg_start == 0 ? lean_ins_ahead(o, vp, u + 1 < nops ? cig[u + 1] : LEAN_NEUTRAL) : lean_ins_carried(s, vp, pos);
                    const int nchars = (int)(o.mlike & 1u) + (int)(x1 & LEAN_INS_MAX);
                    if (nchars > 0) {
                        const int slot = s.cnt < 32 ? atomicAdd(cb.n, 1) : (atomicOr(cb.n, 1 << 30), 1 << 30);      // OR, not ADD: thousands of these in one tile must not wrap the counter
                        if (slot < cb.cap)
                            cand_put(cb, slot, ((uint32_t)j << 16) | ((uint32_t)(s.cnt | 0x80) << 8) | (nchars == 1 ? 7u : 4u), w0 + i,
                                     o.mlike ? o.rbase + (uint32_t)(vp - o.lo) : 0xFFFFFFFFu, x1);
                        s.cnt++;
                    }
                    i++;
                    vp = s_vpos[i & (MAP_WIN - 1)];
                    hit = i < wlen && vp < o.hi;
                }
            }
        }
    }
    if (s.bad) atomicOr(&s_poison[j >> 5], 1u << (j & 31));
    return s.bad == 0;
}

// one pass of the lean walker over the tile's multi-op list: RPT rounds of the workgroup (the list has at most TILE entries).  -> non-zero when this
// lane left a record to the general walker.  An integer, and straight-line rounds: the flag is not carried round a divergent loop.
template <int D, int MAP_BLOCK, int RPT>
__device__ __forceinline__ uint32_t lean_pass(bool lean_on, int tid, int ncx, int nshort, uint16_t *s_cx, const int32_t *s_vpos, int wlen, int w0,
                                              const uint32_t *s_cig, uint32_t c_begin, const CandBuf &cb, uint32_t *s_poison, const int32_t *s_pos,
                                              const uint32_t *s_coff, long long cover, int dbg) {
    constexpr int TILE = MAP_BLOCK * RPT;
    uint32_t redo_any = 0;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int t = k * MAP_BLOCK + tid;
        if (t < ncx) {
            const int ts = t < nshort ? t : TILE - 1 - (t - nshort);
            const int j = s_cx[ts];
            const bool done = lean_on && walk_lean<D>(s_vpos, wlen, w0, s_cig, c_begin, (uint32_t)(TILE * PHZ_CIG_X2 / 2), cb, s_poison, j, s_pos[j], s_coff[j], s_coff[j + 1], cover, dbg);
            if (!done) { s_cx[ts] = (uint16_t)(j | 0x8000); redo_any = 1u; }
        }
    }
    return redo_any;
}

constexpr int MAP_COVER = 65536;   // the staged window holds every het SNP below POS(last read of the tile) + MAP_COVER ...
constexpr int MAP_SLACK = 8;       // ... plus this many further entries (probe overshoot / loop sentinels)

// per-tile het-SNP window: start = lower_bound(vpos, POS of the tile's first read); tile_w[4t+1] = staged length,
// bit 30 set when the window is complete (not truncated by MAP_WIN), which enables the LDS-only fast path
__global__ void k_tile_window(MapBatch bt, int tile_reads) {
    const int64_t T = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (T == 0) *bt.ovf->cursor = 0ull;                     // the overflow area of this submission's staging starts empty
    const bool live = T < bt.ntiles;
    const int si = live ? shard_of(bt.tile0, bt.n_shards, T) : 0;
    const ShardDev &sh = bt.shards[si];
    const int64_t t = live ? T - bt.tile0[si] : 0;
    const int32_t *pos = sh.pos; const uint32_t *cigar_off = sh.cigar_off; const int32_t *vpos = sh.vpos;
    const int nv = sh.nv; const int64_t n = sh.n;
    int32_t *tile_w = bt.tile_w0;
    // Two scattered lines per tile, not four (round 17): a thread loads the FIRST position and the FIRST CIGAR offset of its tile and takes the
    // two words that end the tile from lane + 1, whose tile starts where this one ends -- cigar_off[last + 1] is the neighbour's first offset, and its first
    // position is >= pos[last] (records are sorted), so the upper key only grows and the window is a superset of the one pos[last] gave.  The neighbour
    // serves only when it is the next tile of the SAME shard in the same wave; lane 63 and the last tile of a shard load both words themselves, as does
    // -- its position only -- a tile whose neighbour starts more than MAP_COVER further on (a gene boundary that falls on a tile boundary: the table
    // entries inside the jump must not push the tile over MAP_WIN).  Every lane of the wave takes part in the shuffles: the early return is behind them.
    const int key = live ? pos[t * tile_reads] : 0;
    const uint32_t coff0 = live ? cigar_off[t * tile_reads] : 0u;
    const int nb_key = __shfl_down(key, 1);
    const uint32_t nb_coff0 = (uint32_t)__shfl_down((int)coff0, 1);
    if (!live) return;
    const bool more = (t + 1) * tile_reads < n;             // the shard has a next tile: global tile T + 1, which is lane + 1 unless this is lane 63
    const int64_t last = more ? (t + 1) * tile_reads - 1 : n - 1;
    const bool nb = more && (threadIdx.x & 63) != 63;
    const uint32_t coff_end = nb ? nb_coff0 : cigar_off[last + 1];
    const int pos_end = (nb && (long long)nb_key - key <= MAP_COVER) ? nb_key : pos[last];
    const long long key2 = (long long)pos_end + MAP_COVER;
    // both lower bounds in ONE loop over the whole table: their probes are independent, so the two chains of dependent loads
    // overlap instead of following each other.  (Round 15: a 9-way search, 8 independent probes per bound and round, 6 rounds instead of 17 -- the pre-pass
    // took 37.5 us against 35.0: its time was the four scattered lines every thread fetched (pos and cigar_off at both ends of its tile), not this chain.)
    int lo = 0, hi = nv, lo2 = 0, hi2 = nv;
    while (lo < hi || lo2 < hi2) {
        const int m = (lo + hi) >> 1, m2 = (lo2 + hi2) >> 1;
        const bool go = lo < hi, go2 = lo2 < hi2;
        const int v = go ? vpos[m] : 0, v2 = go2 ? vpos[m2] : 0;
        if (go) { if (v < key) lo = m + 1; else hi = m; }
        if (go2) { if ((long long)v2 < key2) lo2 = m2 + 1; else hi2 = m2; }
    }
    int len = lo2 - lo + MAP_SLACK;
    int complete = 1 << 30;
    if (len > MAP_WIN) { len = MAP_WIN; complete = 0; }
    const uint32_t n_ops = coff_end - coff0;
    tile_w[4 * T] = lo;
    tile_w[4 * T + 1] = len | complete | (si << 16);          // bits 0-15 window length, 16-28 shard of the tile, 30 window complete
    tile_w[4 * T + 2] = (int32_t)coff0;                                // first CIGAR word of the tile
    tile_w[4 * T + 3] = (int32_t)n_ops;
}

// inclusive prefix sum over the 64 lanes of a wave in seven DPP adds (row shifts inside the rows of 16 lanes, then the row
// broadcasts of gfx9): the shuffle version is six ds_bpermute round trips with their address arithmetic and selects
__device__ __forceinline__ int wave_incl_scan(int v0) {
    int v1 = v0 + __builtin_amdgcn_update_dpp(0, v0, 0x111, 0xf, 0xf, true);      // row_shr:1
    v1 += __builtin_amdgcn_update_dpp(0, v0, 0x112, 0xf, 0xf, true);              // row_shr:2
    v1 += __builtin_amdgcn_update_dpp(0, v0, 0x113, 0xf, 0xf, true);              // row_shr:3  -> sums of 4
    v1 += __builtin_amdgcn_update_dpp(0, v1, 0x114, 0xf, 0xe, true);              // row_shr:4, banks 1-3 -> sums of 8
    v1 += __builtin_amdgcn_update_dpp(0, v1, 0x118, 0xf, 0xc, true);              // row_shr:8, banks 2-3 -> sums inside the row
    v1 += __builtin_amdgcn_update_dpp(0, v1, 0x142, 0xa, 0xf, true);              // row_bcast:15 into rows 1 and 3
    v1 += __builtin_amdgcn_update_dpp(0, v1, 0x143, 0xc, 0xf, true);              // row_bcast:31 into rows 2 and 3
    return v1;
}

// maximum over the 64 lanes of a wave (same DPP ladder, the result of lane 63 read into a scalar)
__device__ __forceinline__ int wave_max(int v0) {
    const int lo = (int)0x80000000;
    auto mx = [](int a, int b) { return a > b ? a : b; };
    int v1 = mx(v0, __builtin_amdgcn_update_dpp(lo, v0, 0x111, 0xf, 0xf, false));
    v1 = mx(v1, __builtin_amdgcn_update_dpp(lo, v0, 0x112, 0xf, 0xf, false));
    v1 = mx(v1, __builtin_amdgcn_update_dpp(lo, v0, 0x113, 0xf, 0xf, false));
    v1 = mx(v1, __builtin_amdgcn_update_dpp(lo, v1, 0x114, 0xf, 0xe, false));
    v1 = mx(v1, __builtin_amdgcn_update_dpp(lo, v1, 0x118, 0xf, 0xc, false));
    v1 = mx(v1, __builtin_amdgcn_update_dpp(lo, v1, 0x142, 0xa, 0xf, false));
    v1 = mx(v1, __builtin_amdgcn_update_dpp(lo, v1, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(v1, 63);
}

// block-wide exclusive scan of RPT per-thread values laid out at [k*MAP_BLOCK + tid]; returns the block total
template <int MAP_BLOCK, int RPT>
__device__ __forceinline__ int block_scan(const int (&cnt)[RPT], int (&excl)[RPT], int (*s_wsum)[MAP_BLOCK / 64], int lane, int wave) {
    int incl[RPT];
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int x = wave_incl_scan(cnt[k]);
        incl[k] = x;
        if (lane == 63) s_wsum[k][wave] = x;
    }
    __syncthreads();
    int running = 0;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        int before = running;
#pragma unroll
        for (int w2 = 0; w2 < MAP_BLOCK / 64; w2++) {
            const int s = s_wsum[k][w2];
            if (w2 < wave) before += s;
            running += s;
        }
        excl[k] = before + incl[k] - cnt[k];
    }
    return running;
}

// ABL: the ablation switches of PHZ_MAP_DBG are live (profiling build of the same code); the production instantiation sees dbg == 0 at
// compile time, so none of its tests reach the scalar unit
// NARROW: the 4-byte staging word (phz_stagepack.h); the flush then carries neither the read offsets nor the inserted-text lookup and never touches `side`
template <int MAP_BLOCK, int RPT, bool ABL, bool ONE, bool NARROW>
__device__ __forceinline__ void map_tile(const MapBatch &bt, const int64_t gtile) {
    const int4 tw = *reinterpret_cast<const int4 *>(bt.tile_w0 + 4 * gtile);      // the pre-pass left the tile's shard here: no search
    const int si = (tw.y >> 16) & 0x1FFF;
    MapArgs a;
    {
        const ShardDev &sh = bt.shards[si];
        a.pos = sh.pos; a.cigar_off = sh.cigar_off; a.cigar = sh.cigar; a.seq_off = sh.seq_off; a.bq = sh.bq; a.shp = &sh;
        if (ONE && !ABL) { a.seq2 = nullptr; a.qual = nullptr; } else { a.seq2 = sh.seq2; a.qual = sh.qual; }
        a.n = sh.n; a.vpos = sh.vpos; a.nv = sh.nv; a.baseq = bt.baseq;
        a.stage = bt.stage; a.side = bt.side; a.slots = bt.slots;
        a.tile_w0 = bt.tile_w0; a.tile_total = bt.tile_total; a.slot_cap = bt.slot_cap; a.ntiles = bt.ntiles; a.dbg = ABL ? bt.dbg : 0;
        a.one = ABL ? ((bt.dbg & 4096) != 0 && sh.bq != nullptr) : ONE;
    }
#define PHZ_STAMP(K) do { if (ABL && (bt.dbg & 2048) && threadIdx.x == 0) bt.prof[8 * gtile + (K)] = wall_clock64(); } while (0)
    PHZ_STAMP(0);
    constexpr int TILE = MAP_BLOCK * RPT;
    constexpr int CIG = TILE * PHZ_CIG_X2 / 2;          // packed CIGAR words staged per tile (max)
    constexpr int CAND = TILE * PHZ_CAND_X4 / 4;         // candidate buffer entries (complex records only)
    __shared__ int32_t s_vpos[MAP_WIN];
    __shared__ uint32_t s_coff[TILE + 1];      // cigar_off slice; reused as per-read output offsets after the walk
    __shared__ uint32_t s_soff[TILE];
    __shared__ int32_t s_pos[TILE];            // record positions for the multi-op walk; after it the same words are s_mask
    uint32_t *s_mask = reinterpret_cast<uint32_t *>(s_pos);      // per read: bit o set <=> candidate with ordinal o is a call (resolve phase on)
    __shared__ uint16_t s_cx[TILE];            // reads that need the general CIGAR walk
    __shared__ uint32_t s_cig[CIG];
    __shared__ uint32_t s_key[CAND];
    __shared__ uint16_t s_var[CAND];
    __shared__ uint16_t s_x0[CAND];
    __shared__ unsigned long long s_ins[CAND_INS];
    __shared__ int s_wsum[RPT][MAP_BLOCK / 64];
    __shared__ int s_ncand, s_ncx, s_nlong, s_nins;
    __shared__ uint32_t s_poison[TILE / 32];   // records the lean walker gave up on after it had appended candidates

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = gtile - bt.tile0[si];          // tile index inside the shard
    const int64_t r0 = tile * TILE;
    const int nr = stage_tile_records(a.n, r0, TILE);

    // ---- coalesced streaming loads: pos / seq_off / cigar_off slices, the het-SNP window and the tile's CIGAR words into LDS.
    //      Every load a lane needs (the window and the CIGAR words almost always fit one and three rounds of the workgroup) is
    //      REQUESTED before the first LDS store waits for anything: one global round trip at the start of a tile instead of three.
    VarWin vw;
    vw.g = a.vpos; vw.lds = s_vpos; vw.nv = a.nv; vw.w0 = tw.x;
    vw.wlen = tw.y & 0xFFFF;
    const bool complete = (tw.y >> 30) & 1;
    CigWin cw;
    cw.g = a.cigar; cw.lds = s_cig; cw.c_begin = (uint32_t)tw.z; cw.cap = CIG;
    const uint32_t cnt_w = stage_cigar_words((uint32_t)tw.w, (uint32_t)CIG);
    int rpos_[RPT];
    uint32_t soff_[RPT], coff_[RPT];
    uint32_t cg[3] = {0, 0, 0};
#ifndef PHZ_MAP_FLAT_STAGE
    // One bounds-checked descriptor per slice, built from the tile's uniform values (phz_stageload.h): a lane past a slice's end loads 0, so no load
    // below sits under a lane mask or computes a 64-bit address.  The window's descriptor ends at the table's end: entries past it are padding.
    const auto d_pos = PHZ_STAGE_RSRC(a.pos + r0, nr), d_soff = PHZ_STAGE_RSRC(a.seq_off + r0, nr);
    const auto d_coff = PHZ_STAGE_RSRC(a.cigar_off + r0, stage_coff_words(nr));
    const uint32_t wlive = stage_window_words(vw.wlen, a.nv, vw.w0);
    const auto d_win = PHZ_STAGE_RSRC(a.vpos + vw.w0, wlive);
    const auto d_cig = PHZ_STAGE_RSRC(a.cigar + cw.c_begin, cnt_w);
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int j = k * MAP_BLOCK + tid;
        rpos_[k] = (int)PHZ_STAGE_WORD(d_pos, j);
        soff_[k] = PHZ_STAGE_WORD(d_soff, j);
        coff_[k] = PHZ_STAGE_WORD(d_coff, stage_coff_index(j, nr));      // a lane past the tile keeps cigar_off[r0 + nr]: phase 1a reads s_coff[j + 1]
    }
    // cigar_off[r0 + nr] without a load: the pre-pass stored cigar_off[first] and cigar_off[last + 1] - cigar_off[first] of the SAME records (k_tile_window
    // is launched with tile_reads == TILE: launch_k_map asserts it on the host), and their sum is that word
    const uint32_t coff_end = (uint32_t)tw.z + (uint32_t)tw.w;
    const uint32_t v_raw = PHZ_STAGE_WORD(d_win, tid);
#pragma unroll
    for (int u = 0; u < 3; u++) cg[u] = PHZ_STAGE_WORD(d_cig, (uint32_t)tid + (uint32_t)u * MAP_BLOCK);
    const int v_first = (uint32_t)tid < wlive ? (int)v_raw : 0x7fffffff;
#else
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int j = k * MAP_BLOCK + tid;
        const bool ok = j < nr;
        rpos_[k] = ok ? a.pos[r0 + j] : 0;
        soff_[k] = ok ? a.seq_off[r0 + j] : 0;
        coff_[k] = a.cigar_off[r0 + (ok ? j : nr)];
    }
    const uint32_t coff_end = a.cigar_off[r0 + nr];
    int v_first = 0x7fffffff;
    if (tid < vw.wlen) { const int idx = vw.w0 + tid; v_first = idx < a.nv ? a.vpos[idx] : 0x7fffffff; }
#pragma unroll
    for (int u = 0; u < 3; u++) { const uint32_t j = (uint32_t)tid + (uint32_t)u * MAP_BLOCK; if (j < cnt_w) cg[u] = a.cigar[cw.c_begin + j]; }
#endif
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int j = k * MAP_BLOCK + tid;
        s_pos[j] = rpos_[k]; s_soff[j] = soff_[k]; s_coff[j] = coff_[k];
    }
    if (tid == 0) { s_coff[TILE] = coff_end; s_ncand = 0; s_ncx = 0; s_nlong = 0; s_nins = 0; }
    if (tid < TILE / 32) s_poison[tid] = 0;
    const int wdepth = window_depth(vw.wlen);
    // INT_MAX beyond the window: the search probes without a bounds test, up to index 2^wdepth - 1 (the depth class of the tile) -- and the scans of
    // phase 1a read up to wlen -- so the padding stops at max(wlen, 2^wdepth)
#ifdef PHZ_FILL_ALL
    const int wfill = MAP_WIN;
#else
    const int wfill = (1 << wdepth) > vw.wlen ? (1 << wdepth) : vw.wlen;
#endif
    if (tid < wfill) s_vpos[tid] = v_first;
#ifndef PHZ_MAP_FLAT_STAGE
    for (int j = tid + MAP_BLOCK; j < wfill; j += MAP_BLOCK) {
        const uint32_t v = PHZ_STAGE_WORD(d_win, j);
        s_vpos[j] = (uint32_t)j < wlive ? (int)v : 0x7fffffff;
    }
    // the three unrolled rounds store without a test: 3 * MAP_BLOCK words are inside s_cig, and a word past cnt_w (loaded as 0) is read by nobody
    static_assert(3 * MAP_BLOCK <= CIG, "the unrolled CIGAR rounds stay inside s_cig");
#pragma unroll
    for (int u = 0; u < 3; u++) s_cig[(uint32_t)tid + (uint32_t)u * MAP_BLOCK] = cg[u];
    for (uint32_t j = (uint32_t)tid + 3u * MAP_BLOCK; j < cnt_w; j += MAP_BLOCK) s_cig[j] = PHZ_STAGE_WORD(d_cig, j);
#else
    for (int j = tid + MAP_BLOCK; j < wfill; j += MAP_BLOCK) {
        const int idx = vw.w0 + j;
        s_vpos[j] = (j < vw.wlen && idx < a.nv) ? a.vpos[idx] : 0x7fffffff;
    }
#pragma unroll
    for (int u = 0; u < 3; u++) { const uint32_t j = (uint32_t)tid + (uint32_t)u * MAP_BLOCK; if (j < cnt_w) s_cig[j] = cg[u]; }
    for (uint32_t j = (uint32_t)tid + 3u * MAP_BLOCK; j < cnt_w; j += MAP_BLOCK) s_cig[j] = a.cigar[cw.c_begin + j];
#endif
    __syncthreads();
    PHZ_STAMP(1);
    CandBuf cb;
    cb.key = s_key; cb.var = s_var; cb.x0 = s_x0; cb.ins = s_ins; cb.n = &s_ncand; cb.nins = &s_nins; cb.cap = CAND; cb.w0 = vw.w0;
    const long long cover = (long long)s_pos[nr - 1] + MAP_COVER;     // every het SNP below this is inside the window

    // ---- phase 1a: records made of one aligned run (the common case) never leave registers: an LDS-only,
    //      uniform-trip-count binary search yields (first window index, count) of the het SNPs under the read
    uint32_t c0_[RPT], c1_[RPT];
    int base_[RPT], n_[RPT];
    uint32_t vmask_[RPT], codes_[RPT];
    bool fast_[RPT];
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int j = k * MAP_BLOCK + tid;
        c0_[k] = s_coff[j]; c1_[k] = s_coff[j + 1];
        base_[k] = 0; n_[k] = 0; vmask_[k] = 0; codes_[k] = 0; fast_[k] = false;
    }
    const bool walk_on = !(a.dbg & 8);
    // Records are position-sorted, so the het SNPs any single-run record of a wave can touch lie in ONE narrow index range
    // [lo, hi) of the window: lo = lower_bound(position of the wave's first record), hi = lower_bound(largest end).  All
    // 2*RPT bounds come out of a single uniform-trip search (lane group g looks for bound g); each record then needs only a
    // scan over hi - lo entries (0 for most waves: nothing under any of their records) instead of its own search.
    int len_[RPT]; bool one_[RPT];
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int j = k * MAP_BLOCK + tid;
        one_[k] = false; len_[k] = 0;
        const uint32_t d = c0_[k] - cw.c_begin;
        if (j < nr && walk_on && complete && c1_[k] - c0_[k] == 1 && d < (uint32_t)CIG) {
            const uint32_t w = s_cig[d];
            const uint32_t op = w & 15;
            len_[k] = (int)(w >> 4);
            one_[k] = (op == OP_M || op == OP_EQ || op == OP_X) && (long long)rpos_[k] + len_[k] <= cover;
        }
    }
    constexpr int GROUP = 64 / (2 * RPT);
    int target = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int e = wave_max(one_[k] ? rpos_[k] + len_[k] : (int)0x80000000);
        const int first = __builtin_amdgcn_readfirstlane(rpos_[k]);
        if ((lane / GROUP) == 2 * k) target = first;
        if ((lane / GROUP) == 2 * k + 1) target = e;
    }
    const int bound = lds_lower_bound(s_vpos, wdepth, target);
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int j = k * MAP_BLOCK + tid;
        const int lo = __builtin_amdgcn_readlane(bound, 2 * k * GROUP), hi = __builtin_amdgcn_readlane(bound, (2 * k + 1) * GROUP);
        {
            const int pos = rpos_[k], end = (int)((uint32_t)pos + (uint32_t)len_[k]);
            if (hi - lo <= 24) {
                // wave-uniform bounds and every lane of the wave in the loop (one_ is applied afterwards, by a select): the loop's control is a scalar
                // counter and one branch, no lane mask is saved or restored per entry.  pos <= end: the entries in [pos, end) are those below end less those below pos
                int below = 0, below_end = 0;
                for (int e = lo; e < hi; e++) {
                    const int vp = s_vpos[e];
                    below += vp < pos ? 1 : 0;
                    below_end += vp < end ? 1 : 0;
                }
                const int c = below_end - below;
                if (one_[k] && c <= 8) { fast_[k] = true; base_[k] = lo + below; n_[k] = c; }
            } else if (one_[k]) {
                const int base = lds_lower_bound(s_vpos, wdepth, pos);
                int c = 0;
                while (base + c < vw.wlen && s_vpos[base + c] < end && c <= 8) c++;
                if (c <= 8) { fast_[k] = true; base_[k] = base; n_[k] = c; }
            }
        }
        if (j < nr && walk_on && !fast_[k]) {
            // two lists in one array: records of <= 3 ops from the front, longer ones from the back -- the walk's trip count is the
            // longest CIGAR of the wave, so the first wave gets the short records and the stragglers share the last one
            if (s_coff[j + 1] - s_coff[j] > 3u) s_cx[TILE - 1 - atomicAdd(&s_nlong, 1)] = (uint16_t)j;
            else s_cx[atomicAdd(&s_ncx, 1)] = (uint16_t)j;
        }
    }
    // ---- phase 2a, first half: the quality / base bytes under the FIRST het SNP of every fast record are requested now and used
    //      after the multi-op walk below -- the two gathers are dependent global round trips that nothing else in this phase hides
    uint32_t pre_q[RPT], pre_s[RPT];
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        pre_q[k] = 0; pre_s[k] = 0;
        if (fast_[k] && n_[k] > 0 && !(a.dbg & 1)) {
            const uint32_t soff = s_soff[k * MAP_BLOCK + tid];
            const int x = s_vpos[base_[k]] - rpos_[k];
            if (PHZ_ONEPLANE(a)) pre_q[k] = a.bq[(size_t)soff * 4 + x];
            else { pre_q[k] = a.qual[(size_t)soff * 4 + x]; pre_s[k] = PHZ_SEQ_BYTE(a, soff, x); }
        }
    }
    PHZ_STAMP(2);
    __syncthreads();
    PHZ_STAMP(3);
    // ---- phase 1b: spliced / gapped / clipped records, densely re-packed so the divergent walk runs on full waves
    const int nshort = walk_on ? s_ncx : 0;
    const int ncx = (walk_on && !(a.dbg & 256)) ? nshort + s_nlong : 0;       // dbg 256: multi-op records listed but not walked
    const bool lean_on = complete && !(a.dbg & 32);
    // 1b: the lean walker first (one lane per multi-op record, densely packed); what it declines is redone by the general walker
    const uint32_t redo_any = wdepth == WIN_DSMALL
        ? lean_pass<WIN_DSMALL, MAP_BLOCK, RPT>(lean_on, tid, ncx, nshort, s_cx, s_vpos, vw.wlen, vw.w0, s_cig, cw.c_begin, cb, s_poison, s_pos, s_coff, cover, a.dbg)
        : lean_pass<WIN_DMAX, MAP_BLOCK, RPT>(lean_on, tid, ncx, nshort, s_cx, s_vpos, vw.wlen, vw.w0, s_cig, cw.c_begin, cb, s_poison, s_pos, s_coff, cover, a.dbg);
    const bool redo = __syncthreads_or((int)redo_any) != 0;
    // the lean walk was the last reader of s_pos: its words become the per-record call masks (zeroed here, OR-ed after the next barrier);
    // the few records left to the general walker fetch their position again
#pragma unroll
    for (int k = 0; k < RPT; k++) s_mask[k * MAP_BLOCK + tid] = 0;
    if (redo) {
        for (int t = tid; t < ncx; t += MAP_BLOCK) {
            const int jf = s_cx[t < nshort ? t : TILE - 1 - (t - nshort)];
            if (jf & 0x8000) { const int j = jf & 0x7FFF; walk_read<0>(a, vw, cw, cb, j, r0 + j, a.pos[r0 + j], s_coff[j], s_coff[j + 1], 0, 0, 0); }
        }
    }
    __syncthreads();
    PHZ_STAMP(4);
    const int ncand = s_ncand;
    const bool fb = ncand > CAND;             // candidate buffer overflow: complex records fall back to in-lane work
    // the bytes of this lane's buffered candidate (if it has one) are requested now and used after the arithmetic below
    uint32_t cq = 0, cs = 0; int cx_off = -1;
    if (!fb && tid < ncand && !(a.dbg & 1)) {
        const uint32_t key = s_key[tid];
        if ((key & 0xFF) == 7u) {
            const uint32_t x0 = cand_x0(cb, tid);
            cx_off = x0 != 0xFFFFFFFFu ? (int)x0 : (int)(cand_x1(cb, tid, key) >> 12);
            const uint32_t soff = s_soff[key >> 16];
            if (PHZ_ONEPLANE(a)) cq = a.bq[(size_t)soff * 4 + cx_off];
            else { cq = a.qual[(size_t)soff * 4 + cx_off]; cs = PHZ_SEQ_BYTE(a, soff, cx_off); }
        }
    }
    // ---- phase 2a, second half: resolve the fast records' bases (the first one from the bytes requested above)
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        if (!fast_[k]) continue;
        const int j = k * MAP_BLOCK + tid;
        const uint32_t soff = s_soff[j];
        for (int o = 0; o < n_[k]; o++) {
            const int x = s_vpos[base_[k] + o] - rpos_[k];
            int sy;
            if (a.dbg & 1) sy = x & 3;
            else if (o == 0) {
                if (PHZ_ONEPLANE(a)) sy = sym_from_bq(a, soff, x, pre_q[k]);
                else {
                    const uint32_t q = pre_q[k], sb = (pre_s[k] >> (2 * (x & 3))) & 3;
                    sy = (int)(q & 0x7f) < a.baseq ? 4 : ((q & 0x80) ? (sb == 0 ? 4 : 5) : (int)sb);
                }
            } else sy = masked_base(a, soff, x);
            if (sy != 4) { vmask_[k] |= 1u << o; codes_[k] |= (uint32_t)(sy < 4 ? sy : 4) << (4 * o); }
        }
    }
    int cnt[RPT], off[RPT];
    if (!fb) {
        // ---- phase 2b: resolve the buffered candidates with all lanes gathering at once
        for (int e = tid; e < ncand; e += MAP_BLOCK) {
            uint32_t key = s_key[e];
            const int j = (int)(key >> 16);
            int code = (int)(key & 0xFF);
            if ((key & 0x8000u) && ((s_poison[j >> 5] >> (j & 31)) & 1u)) code = -1;      // lean-origin candidate of a poisoned record
            else if (code == 7) {
                const uint32_t x0 = cand_x0(cb, e);
                const int x = x0 != 0xFFFFFFFFu ? (int)x0 : (int)(cand_x1(cb, e, key) >> 12);
                int sy;
                if (a.dbg & 1) sy = x & 3;
                else if (e == tid && cx_off == x) {
                    if (PHZ_ONEPLANE(a)) sy = sym_from_bq(a, s_soff[j], x, cq);
                    else {
                        const uint32_t sb = (cs >> (2 * (x & 3))) & 3;
                        sy = (int)(cq & 0x7f) < a.baseq ? 4 : ((cq & 0x80) ? (sb == 0 ? 4 : 5) : (int)sb);
                    }
                } else sy = masked_base(a, s_soff[j], x);
                code = sy < 4 ? sy : (sy == 4 ? -1 : 4);
            }
            if (code >= 0) {
                atomicOr(&s_mask[j], 1u << ((key >> 8) & 31));
                s_key[e] = (key & 0xFFFFFF00u) | (uint32_t)code;
            } else {
                s_key[e] = key | 0xFFu;            // not a call
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RPT; k++) cnt[k] = fast_[k] ? __popc(vmask_[k]) : __popc(s_mask[k * MAP_BLOCK + tid]);
    } else {
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int j = k * MAP_BLOCK + tid;
            // (NARROW: the in-lane fallback -- here and in phase 4 -- fetches the record's position and CIGAR range again instead of taking them from rpos_ /
            // c0_ / c1_.  Those six registers would otherwise stay live to the end of the kernel for this cold path alone, and the two-plane narrow
            // instantiation then spills a vector register across the walk -- an LDS address, 8 B of scratch -- where the 8-byte form spills none.)
            cnt[k] = fast_[k] ? __popc(vmask_[k])
                              : (j < nr && walk_on ? walk_read<1>(a, vw, cw, cb, j, r0 + j, NARROW ? a.pos[r0 + j] : rpos_[k], NARROW ? s_coff[j] : c0_[k],
                                                                  NARROW ? s_coff[j + 1] : c1_[k], s_soff[j], 0, 0) : 0);
        }
    }
    PHZ_STAMP(5);
    // ---- phase 3: per-record counts -> offsets (s_coff is free now)
    const int T = block_scan<MAP_BLOCK, RPT>(cnt, off, s_wsum, lane, wave);
#pragma unroll
    for (int k = 0; k < RPT; k++) s_coff[k * MAP_BLOCK + tid] = (uint32_t)off[k];
    if (tid == 0) {
        a.tile_total[gtile] = T;
        // where the tile's calls are staged: its own slot, or -- a tile denser than a slot -- a stretch of the overflow area behind the slots, taken with one
        // cursor step (the slots are sized for the typical tile, not for the densest of a submission: a deep sample with one dense region would have cost
        // tiles x densest x 16 bytes).  Published through two LDS words that are dead by now (slot indices fit 32 bits: checked by the host).
        uint32_t first = (uint32_t)(gtile * (int64_t)a.slot_cap);
        int room = a.slot_cap;
        if (T > a.slot_cap) {
            const OvfArea ov = *bt.ovf;
            const unsigned long long at = atomicAdd(ov.cursor, (unsigned long long)T);
            const bool fits = at + (unsigned long long)T <= (unsigned long long)ov.cap;
            if (fits) { first = (uint32_t)(ov.base + (long long)at); room = T; }
            ov.tile_first[gtile] = fits ? first : 0xFFFFFFFFu;
        }
        s_ncx = (int)first; s_nlong = room;
    }
    __syncthreads();
    PHZ_STAMP(6);
    if (a.dbg & 2) return;
    const int64_t slot0 = (int64_t)(uint32_t)s_ncx;
    const int slot_n = s_nlong;               // calls the tile's stretch of the staging area holds
    // ---- phase 4: ordered flush into the tile's staging slot
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int j = k * MAP_BLOCK + tid;
        if (fast_[k]) {
            int o2 = off[k];
            for (int o = 0; o < n_[k]; o++) {
                if (!((vmask_[k] >> o) & 1)) continue;
                if (o2 < slot_n) {
                    const int64_t g = slot0 + o2;
                    if (NARROW) reinterpret_cast<uint32_t *>(a.stage)[g] = stage4_pack((uint32_t)(vw.w0 + base_[k] + o), (uint32_t)j, (codes_[k] >> (4 * o)) & 15u);
                    else stage_put(a.stage, a.side, a.slots, g, (uint32_t)(vw.w0 + base_[k] + o), (uint32_t)(s_vpos[base_[k] + o] - rpos_[k]), 0u,
                                   (uint32_t)j, (codes_[k] >> (4 * o)) & 15u);
                }
                o2++;
            }
        } else if (fb && cnt[k] > 0) {
            walk_read<2, NARROW>(a, vw, cw, cb, j, r0 + j, NARROW ? a.pos[r0 + j] : rpos_[k], NARROW ? a.cigar_off[r0 + j] : c0_[k],
                                 NARROW ? a.cigar_off[r0 + j + 1] : c1_[k], s_soff[j], slot0 + off[k], slot0 + slot_n);
        }
    }
    if (!fb) {
        for (int e = tid; e < ncand; e += MAP_BLOCK) {
            const uint32_t key = s_key[e];
            if ((key & 0xFF) == 0xFF) continue;
            const int j = (int)(key >> 16);
            const uint32_t ord = (key >> 8) & 31;
            const int o = (int)s_coff[j] + __popc(s_mask[j] & ((1u << ord) - 1));
            if (o < slot_n) {
                const int64_t g = slot0 + o;
                if (NARROW) reinterpret_cast<uint32_t *>(a.stage)[g] = stage4_pack((uint32_t)(vw.w0 + (int)s_var[e]), (uint32_t)j, key & 15u);
                else stage_put(a.stage, a.side, a.slots, g, (uint32_t)(vw.w0 + (int)s_var[e]), cand_x0(cb, e), cand_x1(cb, e, key), (uint32_t)j, key & 15u);
            }
        }
    }
    PHZ_STAMP(7);
#undef PHZ_STAMP
}

// Eight waves per SIMD: the kernel's time follows the number of resident tiles (measured by padding the workgroups with unused LDS:
// 12 / 11 / 10 / 8 / 6 tiles per CU = 1.21 / 1.39 / 1.51 / 1.67 / 2.56 ms), so the tile's LDS is kept under 10 KB (16 tiles per CU: tools/occ_probe2.hip
// maps LDS bytes to resident workgroups) and the register allocation is held to 64 VGPRs (the scalar registers that no longer fit spill to
// lanes of a vector register): 1.21 -> 1.09 ms.
#ifndef PHZ_MAP_WAVES
#define PHZ_MAP_WAVES 8
#endif
#if PHZ_MAP_WAVES > 0
#define PHZ_MAP_OCC __attribute__((amdgpu_waves_per_eu(PHZ_MAP_WAVES, PHZ_MAP_WAVES)))
#else
#define PHZ_MAP_OCC
#endif
template <int MAP_BLOCK, int RPT, bool ABL, bool ONE = false, bool NARROW = false>
__global__ __launch_bounds__(MAP_BLOCK) PHZ_MAP_OCC void k_map(MapBatch bt) {
    // (XCD-contiguous tile order -- workgroup i runs on XCD i % 8; every XCD given one contiguous eighth of the tiles -- was measured in
    // round 4 for k_map, k_line, k_tile and k_pairs: no gain anywhere, 1.291 against 1.282 ms here.  Neighbouring tiles share only their
    // het-SNP window, which the memory-side cache serves.)
    map_tile<MAP_BLOCK, RPT, ABL, ONE, NARROW>(bt, (int64_t)blockIdx.x);
}

// two-level exclusive prefix sum of the per-tile totals: 1024-tile chunks in parallel, then one small pass
__global__ __launch_bounds__(1024) void k_chunk_scan(const int32_t *tile_total, int64_t ntiles, int32_t *tile_pref, int64_t *chunk_sum,
                                                     int32_t *chunk_max) {
    __shared__ int s_w[16], s_m[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * 1024 + tid;
    const int v = i < ntiles ? tile_total[i] : 0;
    int x = v, mx = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { int y = __shfl_xor(mx, d); mx = y > mx ? y : mx; }
    if (lane == 63) s_w[wave] = x;
    if (lane == 0) s_m[wave] = mx;
    __syncthreads();
    int before = 0;
    for (int w2 = 0; w2 < wave; w2++) before += s_w[w2];
    if (i < ntiles) tile_pref[i] = before + x - v;
    if (tid == 1023) chunk_sum[blockIdx.x] = before + x;
    if (tid == 0) {
        int m = 0;
        for (int w2 = 0; w2 < 16; w2++) m = s_m[w2] > m ? s_m[w2] : m;
        chunk_max[blockIdx.x] = m;
    }
}

// calls before global tile T over all shards (T < ntiles)
__device__ __forceinline__ int64_t calls_before(const int64_t *chunk_base, const int32_t *tile_pref, int64_t T) {
    return chunk_base[T >> 10] + tile_pref[T];
}

// What the host reads when the stream has drained, and where it goes: `host` is the page-locked image of the MapScalars words (hipHostMalloc memory is mapped
// into the device's address space, so the kernel stores straight into it -- as PhzMail's gather kernel does -- and no copy follows the last kernel of a step).
struct TotalsOut {
    const int64_t *tile0; int n_shards; int64_t ntiles;
    const int32_t *tile_pref;
    int64_t *shard_base;                      // [n_shards], device: first call of the shard in the batch-wide numbering (k_compact)
    const unsigned long long *cursor;         // the overflow area's cursor: final once k_map has completed, i.e. for every kernel behind it on the stream
    unsigned long long *host;                 // [0] calls of the batch, [1] densest tile, [2 + s] calls of shard s, [2 + n_shards] the cursor
};
// per shard: offset of its first call in the batch-wide numbering and its number of calls (chunk_base: the LDS copy or the array in global memory)
__device__ __forceinline__ void shard_total(const TotalsOut &o, int s, const int64_t *chunk_base, int64_t total) {
    const int64_t a = o.tile0[s], b = o.tile0[s + 1];
    const int64_t lo = a < o.ntiles ? calls_before(chunk_base, o.tile_pref, a) : total;
    const int64_t hi = b < o.ntiles ? calls_before(chunk_base, o.tile_pref, b) : total;
    o.shard_base[s] = lo;
    o.host[2 + s] = (unsigned long long)(hi - lo);
}
__device__ __forceinline__ void batch_words(const TotalsOut &o, unsigned long long total, unsigned long long max_tile) {
    o.host[0] = total; o.host[1] = max_tile; o.host[2 + o.n_shards] = *o.cursor;
}

// One workgroup: the exclusive scan of the chunk sums and the densest tile -> scal[0] total, scal[1] max tile.  While the chunk bases fit its LDS copy
// (BASE_LDS chunks = a million tiles; `merged`) it also does k_shard_totals' work after its last barrier, from that copy: one launch fewer per step, and
// no reading back of global memory it has just written.
constexpr int BASE_LDS = 1024;
__global__ __launch_bounds__(1024) void k_chunk_base(const int64_t *chunk_sum, const int32_t *chunk_max, int nchunks, int64_t *chunk_base,
                                                     unsigned long long *scal, bool merged, TotalsOut o) {
    __shared__ long long s_w[16];
    __shared__ long long s_carry;
    __shared__ int s_m[16];
    __shared__ int64_t s_base[BASE_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    int mx = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nchunks; b0 += 1024) {
        const int i = b0 + tid;
        const long long v = i < nchunks ? chunk_sum[i] : 0;
        if (i < nchunks) mx = chunk_max[i] > mx ? chunk_max[i] : mx;
        long long x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            long long y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        long long before = s_carry;
        for (int w2 = 0; w2 < wave; w2++) before += s_w[w2];
        if (i < nchunks) { chunk_base[i] = before + x - v; if (merged) s_base[i] = before + x - v; }      // (merged: nchunks <= BASE_LDS)
        __syncthreads();
        if (tid == 1023) s_carry = before + x;
        __syncthreads();
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { int y = __shfl_xor(mx, d); mx = y > mx ? y : mx; }
    if (lane == 0) s_m[wave] = mx;
    __syncthreads();
    const long long total = s_carry;
    if (tid == 0) {
        int m = 0;
        for (int w2 = 0; w2 < 16; w2++) m = s_m[w2] > m ? s_m[w2] : m;
        scal[0] = (unsigned long long)total;
        scal[1] = (unsigned long long)m;
        if (merged) batch_words(o, (unsigned long long)total, (unsigned long long)m);
    }
    if (merged)
        for (int s = tid; s < o.n_shards; s += 1024) shard_total(o, s, s_base, total);
}

// the per-shard totals of a submission of more than BASE_LDS chunks, from the chunk bases in global memory
__global__ void k_shard_totals(const int64_t *chunk_base, const unsigned long long *scal, TotalsOut o) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s == 0) batch_words(o, scal[0], scal[1]);
    if (s < o.n_shards) shard_total(o, s, chunk_base, (int64_t)scal[0]);
}

struct CompactArgs {
    const uint2 *stage; const uint32_t *side; int64_t slots;
    const ShardDev *shards; const int64_t *tile0; int n_shards;
    const int32_t *tile_total; const int32_t *tile_pref; const int64_t *chunk_base; const int64_t *shard_base;
    const int32_t *tile_w0;
    int slot_cap, tile_reads; int64_t ntiles;
    const uint32_t *tile_ovf;             // first slot of a tile with more than slot_cap calls (overflow area), 0xFFFFFFFF: it did not fit
};

// One wave per CT consecutive tiles.  A lane first fetches one tile's bookkeeping (count, shard, destination, first record), so the
// chain of dependent loads a tile needs is paid once per CT tiles; the wave then walks the CT slots as ONE flat list of calls, UNR
// elements per lane in flight, each finding its tile by a lower bound over the wave's prefix in LDS.  One wave per tile was bound
// by that chain (~5 round trips for ~60 calls: 254 us per genome whatever the record size); larger CT amortises it further but
// leaves the tail to the waves that drew the densest tiles (CT 4 / 8 / 16 / 64: 1.50 / 1.49 / 1.50 / 1.52 ms per genome step,
// 0.91 / 0.93 / 0.96 / 1.08 ms on configs[1], whose calls sit in a few tiles).
#ifndef PHZ_CT
#define PHZ_CT 4
#endif
constexpr int CT = PHZ_CT, CT_UNR = 4;
// where a shard's calls go (the output part of its ShardDev record)
struct ShardOut { int32_t *o_read, *o_var; uint8_t *o_code; uint32_t *o_aux0, *o_aux1; int64_t cap; };
__device__ __forceinline__ ShardOut shard_out(const ShardDev &sh) { return ShardOut{sh.o_read, sh.o_var, sh.o_code, sh.o_aux0, sh.o_aux1, sh.cap}; }

// UNI: all CT tiles of the wave belong to one shard (all but 21 waves of a genome), whose output pointers `out0` were loaded once, right after the shard was
// known -- inside the loop they are loaded again in every round, behind the staging loads, because the stores between them may alias the record
// (114 -> 81 us per genome step).
// AUX: some shard of the submission has the two text planes (decided by the host; without them the branch and its side-plane loads are not compiled in:
// 114 -> 105 us alone, 81 -> 70 us on top of the hoisted loads).  (The workgroup barrier below as a wave-local ordering point -- the four waves share
// nothing -- was worth 0.3 us: left as it was.)
// NARROW: the slots hold the 4-byte word of phz_stagepack.h (never together with AUX): half the bytes in, no side planes
template <bool UNI, bool AUX, bool NARROW>
__device__ __forceinline__ void compact_run(const CompactArgs &c, const int *pref, const int64_t *dstv, const int32_t *r0v, const int32_t *siv, const int64_t *slotv,
                                            int M, int lane, const ShardOut &out0) {
    static_assert(!(AUX && NARROW), "the narrow staging word carries no text planes");
    if (NARROW) {
        const uint32_t *stage4 = reinterpret_cast<const uint32_t *>(c.stage);
        for (int e0 = lane; e0 < M; e0 += 64 * CT_UNR) {
            int k_[CT_UNR]; uint32_t w_[CT_UNR];
#pragma unroll
            for (int u = 0; u < CT_UNR; u++) {
                const int e = e0 + 64 * u;
                int k = 0;
#pragma unroll
                for (int st = CT / 2; st > 0; st >>= 1) k += (pref[k + st] <= e) ? st : 0;     // last k with pref[k] <= e
                k_[u] = k;
                w_[u] = e < M ? stage4[slotv[k] + (e - pref[k])] : 0u;
            }
#pragma unroll
            for (int u = 0; u < CT_UNR; u++) {
                const int e = e0 + 64 * u;
                if (e >= M) break;
                const int k = k_[u];
                const uint32_t w = w_[u];
                const ShardOut sh = UNI ? out0 : shard_out(c.shards[siv[k]]);
                const int64_t o = dstv[k] + (e - pref[k]);
                if (o < sh.cap) {
                    sh.o_read[o] = r0v[k] + (int32_t)stage4_rec(w);
                    sh.o_var[o] = (int32_t)stage4_var(w);
                    sh.o_code[o] = (uint8_t)stage4_code(w);
                }
            }
        }
        return;
    }
    for (int e0 = lane; e0 < M; e0 += 64 * CT_UNR) {
        int k_[CT_UNR]; uint2 w_[CT_UNR]; int64_t g_[CT_UNR];
#pragma unroll
        for (int u = 0; u < CT_UNR; u++) {
            const int e = e0 + 64 * u;
            int k = 0;
#pragma unroll
            for (int st = CT / 2; st > 0; st >>= 1) k += (pref[k + st] <= e) ? st : 0;     // last k with pref[k] <= e
            k_[u] = k;
            g_[u] = slotv[k] + (e - pref[k]);
            w_[u] = e < M ? c.stage[g_[u]] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < CT_UNR; u++) {
            const int e = e0 + 64 * u;
            if (e >= M) break;
            const int k = k_[u];
            const uint2 w = w_[u];
            const ShardOut sh = UNI ? out0 : shard_out(c.shards[siv[k]]);
            const int64_t o = dstv[k] + (e - pref[k]);
            if (o < sh.cap) {
                sh.o_read[o] = r0v[k] + (int32_t)(w.y & 0x3FFu);
                sh.o_var[o] = (int32_t)w.x;
                sh.o_code[o] = (uint8_t)((w.y >> 10) & 15u);
                if (AUX && sh.o_aux0) {      // the two planes only the mapper's text output reads (NULL for a caller that wants (record, variant, code))
                    uint32_t a0 = w.y >> 16, a1 = 0u;
                    if (w.y & 0x8000u) a0 = c.side[g_[u]];
                    if (w.y & 0x4000u) a1 = c.side[c.slots + g_[u]];
                    sh.o_aux0[o] = a0;
                    sh.o_aux1[o] = a1;
                }
            }
        }
    }
}

template <bool AUX, bool NARROW = false>
__global__ __launch_bounds__(256) void k_compact(CompactArgs c) {
    __shared__ int s_pref[4][CT + 1];
    __shared__ int64_t s_dst[4][CT], s_slot[4][CT];
    __shared__ int32_t s_r0[4][CT], s_si[4][CT];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t T0 = ((int64_t)blockIdx.x * 4 + w) * CT;
    const int64_t T = T0 + lane;
    int n = 0, si = -1;
    if (lane < CT && T < c.ntiles) {
        n = c.tile_total[T];
        int64_t first = T * (int64_t)c.slot_cap;
        if (n > c.slot_cap) {
            const uint32_t ov = c.tile_ovf[T];
            if (ov != 0xFFFFFFFFu) first = (int64_t)ov; else n = c.slot_cap;         // (no room in the overflow area: the batch is redone with a larger one)
        }
        s_slot[w][lane] = first;
        si = (c.tile_w0[4 * T + 1] >> 16) & 0x1FFF;
        s_dst[w][lane] = calls_before(c.chunk_base, c.tile_pref, T) - c.shard_base[si];
        s_r0[w][lane] = (int32_t)((T - c.tile0[si]) * c.tile_reads);
        s_si[w][lane] = si;
    }
    const int incl = wave_incl_scan(n);
    if (lane < CT) s_pref[w][lane + 1] = incl;
    if (lane == 0) s_pref[w][0] = 0;
    __syncthreads();
    const int M = __builtin_amdgcn_readlane(incl, CT - 1);
    if (M == 0) return;
    const int si0 = __builtin_amdgcn_readfirstlane(si);      // (lane 0 holds tile T0 < ntiles whenever M > 0)
    const bool uni = __ballot(si >= 0 && si != si0) == 0ull;
    if (uni) compact_run<true, AUX, NARROW>(c, s_pref[w], s_dst[w], s_r0[w], s_si[w], s_slot[w], M, lane, shard_out(c.shards[si0]));
    else compact_run<false, AUX, NARROW>(c, s_pref[w], s_dst[w], s_r0[w], s_si[w], s_slot[w], M, lane, ShardOut{});
}

// ---- layouts of the buffers the driver carves into parts: byte offsets computed once, typed pointers handed out for a device buffer or its pinned image
template <class T> static T *part_at(const DevBuf &b, size_t off) { return (T *)((char *)b.p + off); }

// ctx->map.tab and its image ctx->map.tab_host: [ShardDev x m][tile0 x (m+1)][shard_base x m][OvfArea].  [0, table_bytes) is the shard table a repeated
// submission does not upload again; shard_base exists on the device only (the totals kernel recomputes it in every attempt)
struct MapTab {
    size_t off_tile0, off_base, off_ovf;
    explicit MapTab(int m) : off_tile0((size_t)m * sizeof(ShardDev)), off_base(off_tile0 + (size_t)(m + 1) * 8), off_ovf(off_base + (size_t)m * 8) {}
    size_t table_bytes() const { return off_base; }
    size_t bytes() const { return off_ovf + 64; }
    ShardDev *shards(const DevBuf &b) const { return part_at<ShardDev>(b, 0); }
    OvfArea *ovf(const DevBuf &b) const { return part_at<OvfArea>(b, off_ovf); }
    int64_t *tile0(const DevBuf &b) const { return part_at<int64_t>(b, off_tile0); }
    int64_t *shard_base(const DevBuf &b) const { return part_at<int64_t>(b, off_base); }
};
// ctx->map.desc: [tile_pref x ntiles][chunk_sum x nchunks][chunk_base x nchunks][chunk_max x nchunks]
struct MapDesc {
    size_t off_sum, off_base, off_max, bytes;
    MapDesc(int64_t ntiles, int nchunks) : off_sum(((size_t)ntiles * 4 + 15) & ~(size_t)15), off_base(off_sum + (size_t)nchunks * 8), off_max(off_base + (size_t)nchunks * 8),
                                           bytes((size_t)ntiles * 4 + (size_t)nchunks * 24 + 64) {}
    int32_t *tile_pref(const DevBuf &b) const { return part_at<int32_t>(b, 0); }
    int64_t *chunk_sum(const DevBuf &b) const { return part_at<int64_t>(b, off_sum); }
    int64_t *chunk_base(const DevBuf &b) const { return part_at<int64_t>(b, off_base); }
    int32_t *chunk_max(const DevBuf &b) const { return part_at<int32_t>(b, off_max); }
};
// ctx->scalars, the device block, 8-byte words: [0] calls of the batch, [1] densest tile, [2] the overflow-area cursor k_map steps.
// ctx->h_scalars, its page-locked image, written by the totals kernel (TotalsOut) and read by the host: [0] calls of the batch, [1] densest tile,
// [2, 2 + m) calls per shard -- these exist in the image only --, [2 + m] the cursor
struct MapScalars {
    int m;
    size_t dev_bytes() const { return (size_t)8 * 3 + 128; }
    size_t host_bytes() const { return (size_t)8 * (m + 3) + 128; }
    unsigned long long *dev_words(const DevBuf &b) const { return part_at<unsigned long long>(b, 0); }
    unsigned long long *dev_cursor(const DevBuf &b) const { return dev_words(b) + 2; }
    unsigned long long *words(const DevBuf &b) const { return part_at<unsigned long long>(b, 0); }
    unsigned long long &shard_calls(const DevBuf &b, int k) const { return words(b)[2 + k]; }
    unsigned long long *cursor(const DevBuf &b) const { return words(b) + 2 + m; }
};

// the PHZ_MAP_* switches of one submission (read per call: tests change them between calls on one ctx)
struct MapKnobs {
    int blk, rpt, dbg, merge_chunks; unsigned dyn_lds; bool two_planes;
    bool wide_stage = positive("PHZ_MAP_WIDE_STAGE", 0) != 0;      // PHZ_MAP_WIDE_STAGE=1: the 8-byte staging record even where the 4-byte word would do (tests, A/B)
    static int positive(const char *name, int dflt) { const char *e = getenv(name); return e && atoi(e) > 0 ? atoi(e) : dflt; }
    // (PHZ_MAP_DYNLDS, an experiment: bytes of dynamic LDS nobody uses, to bound the workgroups per CU)
    // PHZ_MAP_MERGE_CHUNKS: the largest chunk count whose per-shard totals k_chunk_base computes itself (tests: 1, so that a submission of two chunks takes the
    // separate k_shard_totals launch of a submission beyond a million tiles)
    MapKnobs() : blk(positive("PHZ_MAP_BLOCK", 128)), rpt(positive("PHZ_MAP_RPT", 2)), merge_chunks(positive("PHZ_MAP_MERGE_CHUNKS", BASE_LDS)), dyn_lds((unsigned)positive("PHZ_MAP_DYNLDS", 0)), two_planes(getenv("PHZ_MAP_TWO_PLANES") != nullptr) {
        const char *e = getenv("PHZ_MAP_DBG"); dbg = e ? atoi(e) : 0;
    }
};

// What one submission knows.  Its functions are the sections of launch_map_batch in stream order; the one host wait of an attempt is the end of attempt().
struct MapSubmission {
    phz_ctx *ctx; hipStream_t sm; DevBuf *S;
    const int n; const phz_reads *r; const phz_variants *v; const int baseq; const phz_calls *out; int64_t *n_calls;
    const MapKnobs knobs; int tile_reads = 0;
    std::vector<int> live; std::vector<int64_t> tile0;          // live shards (records and variants present); first tile of each, then the tile count
    int m = 0, nchunks = 0; int64_t ntiles = 0, max_nv = 0; bool one_plane = false, text_planes = false, narrow = false;
    MapTab tab{0}; MapDesc desc{0, 0}; MapScalars scal{0};
    float ms_total = 0;

    MapSubmission(phz_ctx *c, int n_, const phz_reads *r_, const phz_variants *v_, int baseq_, const phz_calls *out_, int64_t *n_calls_)
        : ctx(c), sm(c->stream), S(c->scratch), n(n_), r(r_), v(v_), baseq(baseq_), out(out_), n_calls(n_calls_) {}
    template <class T> T *scr(int slot) const { return (T *)S[slot].p; }

    // ---- the live shards and their tile ranges; the limits of the tile word (13 bits of shard, 31 of tile)
    int live_shards_and_tiles() {
        // (64 x 2 / 64 x 4 / 128 x 4 / 256 x 4 records per tile were swept in rounds 1-3 -- 1.84 ms and worse against 1.28 -- and are no longer built:
        // their tiles cannot be held at eight waves per SIMD)
        if (!((knobs.blk == 128 || knobs.blk == 256) && knobs.rpt == 2)) return phz_fail(ctx, PHZ_E_ARG, "bad PHZ_MAP_BLOCK / PHZ_MAP_RPT");
        tile_reads = knobs.blk * knobs.rpt;
        for (int i = 0; i < n; i++) {
            if (v[i].n > 0x7fffffff) return phz_fail(ctx, PHZ_E_ARG, "too many variants in one shard");
            if (r[i].n_reads > 0 && v[i].n > 0) { live.push_back(i); tile0.push_back(ntiles); ntiles += (r[i].n_reads + tile_reads - 1) / tile_reads; }
        }
        tile0.push_back(ntiles);
        m = (int)live.size();
        if (ntiles >= (1ll << 31)) return phz_fail(ctx, PHZ_E_ARG, "too many tiles in one submission");
        if (m > 0x1FFF) return phz_fail(ctx, PHZ_E_ARG, "more than 8191 shards in one submission");
        nchunks = (int)((ntiles + 1023) / 1024);
        tab = MapTab(m); desc = MapDesc(ntiles, nchunks); scal = MapScalars{m};
        return PHZ_OK;
    }
    // ---- the shard table built in K_map's pinned image and uploaded unless the device holds these very bytes (same shards, same output buffers)
    int shard_table() {
        auto &M = ctx->map;
        if (int s = phz_reserve_host(ctx, M.tab_host, tab.bytes())) return s;
        if (int s = phz_reserve(ctx, M.tab, tab.bytes())) return s;
        ShardDev *hs = tab.shards(M.tab_host);
        // every shard of the submission carries the one-byte plane (a caller's choice: phz_reads.bq; PHZ_MAP_ONE_PLANE=1 for the Python host): the ONE instantiation
        // reads it (PHZ_MAP_TWO_PLANES=1: the two-plane instantiation regardless).  Same-box A/B of the two production instantiations on the whole-genome sample:
        // 1.0940 against 1.0928 ms -- the plane buys nothing there, so nothing in the product builds it by default
        one_plane = !knobs.two_planes;
        for (int k = 0; k < m; k++) {
            const int i = live[(size_t)k];
            ShardDev &d = hs[k];
            d.pos = r[i].pos; d.cigar_off = r[i].cigar_off; d.cigar = r[i].cigar; d.seq_off = r[i].seq_off; d.seq2 = r[i].seq2; d.qual = r[i].qual; d.bq = r[i].bq;
            d.n = r[i].n_reads; d.vpos = v[i].pos; d.nv = (int)v[i].n; d.pad = 0;
            d.o_read = out[i].read_idx; d.o_var = out[i].var_idx; d.o_code = out[i].code; d.o_aux0 = out[i].aux0; d.o_aux1 = out[i].aux1;
            if (!d.o_aux0 || !d.o_aux1) { d.o_aux0 = nullptr; d.o_aux1 = nullptr; }           // both or none
            d.cap = out[i].cap;
            if (!d.bq) one_plane = false;
            if (d.o_aux0) text_planes = true;           // some shard wants the two text planes: k_compact's instantiation that writes them
            if (d.nv > max_nv) max_nv = d.nv;
        }
        // the staging form of the submission (phz_stagepack.h); the profiling instantiation of k_map exists in the general form only
        narrow = stage_narrow_form(text_planes, tile_reads, max_nv, knobs.wide_stage || knobs.dbg != 0);
        memcpy(tab.tile0(M.tab_host), tile0.data(), (size_t)(m + 1) * 8);
        const char *img = (const char *)hs;
        if (M.tab_image.size() != tab.table_bytes() || M.tab_dev != M.tab.p || memcmp(M.tab_image.data(), img, tab.table_bytes()) != 0) {
            PHZ_HIP(ctx, hipMemcpyAsync(M.tab.p, img, tab.table_bytes(), hipMemcpyHostToDevice, sm));
            M.tab_image.assign(img, img + tab.table_bytes());
            M.tab_dev = M.tab.p;
        }
        for (hipEvent_t &e : M.ev) if (!e) PHZ_HIP(ctx, hipEventCreate(&e));
        return PHZ_OK;
    }
    // ---- every buffer whose size the tile count decides; the slot size of the staging area, fixed at the ctx's first submission
    // Staging: every tile owns a slot of slot_cap calls (half a tile's records: the typical RNA-seq tile has ~60) and a tile with more takes a stretch of
    // the OVERFLOW AREA behind the slots (one cursor step per such tile).  The area starts at a quarter of the slots' size and is kept at what the densest
    // submission so far needed; a submission that needs more is redone once with exactly that (round 4 sized EVERY slot for the densest tile: 50 GB for a
    // deep sample with one dense region).  PHZ_MAP_SLOT_CAP: another slot size (tests: 8, so that most tiles overflow).
    int reserve() {
        auto &M = ctx->map;
        if (int s = reserve_all(ctx, {{M.tile_w0, (size_t)ntiles * 16}, {S[SC_MAP_TILE_TOTAL], (size_t)ntiles * 4}, {M.desc, desc.bytes}, {ctx->scalars, scal.dev_bytes()}})) return s;
        if (int s = phz_reserve_host(ctx, ctx->h_scalars, scal.host_bytes())) return s;
        if (int s = phz_reserve(ctx, S[SC_MAP_TILE_OVF], (size_t)ntiles * 4)) return s;
        if (M.slot_cap <= 0 || M.tile_reads != tile_reads) {
            M.slot_cap = tile_reads / 2 < 64 ? 64 : tile_reads / 2; M.tile_reads = tile_reads;
            const char *e = getenv("PHZ_MAP_SLOT_CAP"); if (e && atoi(e) >= 1) M.slot_cap = atoi(e);
        }
        return PHZ_OK;
    }
    // ---- the staging area at the overflow area's current size: bt's view of it, and the OvfArea record on the device (in K_map's own buffer: ctx->scalars is
    // shared scratch), uploaded only when it changed -- like the shard table --; the cursor is zeroed by the pre-pass kernel: no extra operation on the stream per step
    int staging_area(MapBatch &bt) {
        auto &M = ctx->map;
        const size_t base_slots = (size_t)ntiles * (size_t)M.slot_cap;
        if (M.ovf_cap < (int64_t)(base_slots / 4)) M.ovf_cap = (int64_t)(base_slots / 4);
        if (M.ovf_cap < 65536) M.ovf_cap = 65536;
        const size_t slots = base_slots + (size_t)M.ovf_cap;
        if (slots >= 0xFFFFFFF0ull) return phz_fail(ctx, PHZ_E_ARG, "K_map staging area beyond 2^32 slots: submit the shards in smaller batches");
        if (int s = phz_reserve(ctx, S[SC_MAP_STAGE], slots * (narrow ? 4 : 16))) return s;
        bt.stage = scr<uint2>(SC_MAP_STAGE); bt.slots = (int64_t)slots;
        bt.side = narrow ? nullptr : (uint32_t *)(bt.stage + slots);        // general form: [packed record x slots][side word x 2 slots]; narrow form: [word x slots]
        bt.slot_cap = M.slot_cap;
        OvfArea *h_ov = tab.ovf(M.tab_host), *d_ov = tab.ovf(M.tab);
        h_ov->tile_first = scr<uint32_t>(SC_MAP_TILE_OVF); h_ov->cursor = scal.dev_cursor(ctx->scalars); h_ov->base = (long long)base_slots; h_ov->cap = (long long)M.ovf_cap;
        const long long img[5] = {(long long)(intptr_t)h_ov->tile_first, (long long)(intptr_t)h_ov->cursor, h_ov->base, h_ov->cap, (long long)(intptr_t)d_ov};
        if (memcmp(img, M.ovf_image, sizeof img) != 0) {
            PHZ_HIP(ctx, hipMemcpyAsync(d_ov, h_ov, sizeof(OvfArea), hipMemcpyHostToDevice, sm));
            memcpy(M.ovf_image, img, sizeof img);
        }
        bt.ovf = d_ov;
        return PHZ_OK;
    }
    template <int B, int R> void launch_k_map(const MapBatch &bt) const {
        const dim3 grid((unsigned)ntiles), block(B);
        // k_map takes cigar_off[last + 1] of a tile from the pre-pass's words: both must cut the shard into the same tiles.  A host check, one integer compare
        // per launch; the library's build (_lib.build) does not define NDEBUG, so it is compiled in -- a build with -DNDEBUG drops it
        assert(tile_reads == B * R);
        if constexpr (B * R <= STAGE4_MAX_TILE_READS) {
            if (narrow) {
                if (one_plane) hipLaunchKernelGGL((k_map<B, R, false, true, true>), grid, block, knobs.dyn_lds, sm, bt);
                else hipLaunchKernelGGL((k_map<B, R, false, false, true>), grid, block, knobs.dyn_lds, sm, bt);
                return;
            }
        }
        if (bt.dbg) hipLaunchKernelGGL((k_map<B, R, true>), grid, block, knobs.dyn_lds, sm, bt);
        else if (one_plane) hipLaunchKernelGGL((k_map<B, R, false, true>), grid, block, knobs.dyn_lds, sm, bt);
        else hipLaunchKernelGGL((k_map<B, R, false>), grid, block, knobs.dyn_lds, sm, bt);
    }
    // ---- one attempt: pre-pass, k_map between its two events, the scan of the tile totals, chunk bases + per-shard totals + the host's words, compaction.  WAIT
    int attempt() {
        auto &M = ctx->map;
        MapBatch bt;
        bt.shards = tab.shards(M.tab); bt.tile0 = tab.tile0(M.tab); bt.n_shards = m; bt.baseq = baseq;
        bt.tile_w0 = (int32_t *)M.tile_w0.p; bt.tile_total = scr<int32_t>(SC_MAP_TILE_TOTAL); bt.ntiles = ntiles;
        if (int s = staging_area(bt)) return s;
        bt.dbg = knobs.dbg; bt.prof = nullptr;
        if (bt.dbg & 2048) { if (int s = phz_reserve(ctx, S[SC_MAP_PROFILE], (size_t)ntiles * 64)) return s; bt.prof = scr<unsigned long long>(SC_MAP_PROFILE); }
        hipLaunchKernelGGL(k_tile_window, dim3(nblk(ntiles)), dim3(256), 0, sm, bt, tile_reads);
        PHZ_HIP(ctx, hipEventRecord(M.ev[0], sm));
        if (knobs.blk == 128) launch_k_map<128, 2>(bt); else launch_k_map<256, 2>(bt);
        PHZ_HIP(ctx, hipEventRecord(M.ev[1], sm));
        int32_t *tile_pref = desc.tile_pref(M.desc); int64_t *chunk_sum = desc.chunk_sum(M.desc), *chunk_base = desc.chunk_base(M.desc); int32_t *chunk_max = desc.chunk_max(M.desc);
        unsigned long long *d_words = scal.dev_words(ctx->scalars);
        hipLaunchKernelGGL(k_chunk_scan, dim3((unsigned)nchunks), dim3(1024), 0, sm, (const int32_t *)bt.tile_total, ntiles, tile_pref, chunk_sum, chunk_max);
        // the words the host reads after the wait are stored into their page-locked image by the totals kernel: no copy ends the step
        TotalsOut to;
        to.tile0 = bt.tile0; to.n_shards = m; to.ntiles = ntiles; to.tile_pref = tile_pref; to.shard_base = tab.shard_base(M.tab);
        to.cursor = scal.dev_cursor(ctx->scalars); to.host = scal.words(ctx->h_scalars);
        const bool merged = nchunks <= BASE_LDS && nchunks <= knobs.merge_chunks;
        hipLaunchKernelGGL(k_chunk_base, dim3(1), dim3(1024), 0, sm, (const int64_t *)chunk_sum, (const int32_t *)chunk_max, nchunks, chunk_base, d_words, merged, to);
        if (!merged) hipLaunchKernelGGL(k_shard_totals, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, sm, (const int64_t *)chunk_base, (const unsigned long long *)d_words, to);
        CompactArgs c;
        c.stage = bt.stage; c.side = bt.side; c.slots = bt.slots;
        c.shards = bt.shards; c.tile0 = bt.tile0; c.n_shards = m;
        c.tile_total = bt.tile_total; c.tile_pref = tile_pref; c.chunk_base = chunk_base; c.shard_base = tab.shard_base(M.tab);
        c.tile_w0 = bt.tile_w0;
        c.slot_cap = bt.slot_cap; c.tile_reads = tile_reads; c.ntiles = ntiles; c.tile_ovf = scr<const uint32_t>(SC_MAP_TILE_OVF);
        const dim3 cgrid((unsigned)((ntiles + 4 * CT - 1) / (4 * CT)));
        if (narrow) hipLaunchKernelGGL((k_compact<false, true>), cgrid, dim3(256), 0, sm, c);
        else if (text_planes) hipLaunchKernelGGL(k_compact<true>, cgrid, dim3(256), 0, sm, c);
        else hipLaunchKernelGGL(k_compact<false>, cgrid, dim3(256), 0, sm, c);
        PHZ_HIP(ctx, hipGetLastError());
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        float ms = 0;
        PHZ_HIP(ctx, hipEventElapsedTime(&ms, M.ev[0], M.ev[1]));
        if (bt.prof) if (int s = profile_report(bt.prof, ms)) return s;
        ms_total += ms;
        return PHZ_OK;
    }
    // ---- PHZ_MAP_DBG & 2048: mean time between the stamps of a tile (wall_clock64: 100 MHz), first wave's view
    int profile_report(const unsigned long long *prof, float ms) {
        std::vector<unsigned long long> pr((size_t)ntiles * 8);
        PHZ_HIP(ctx, hipMemcpy(pr.data(), prof, pr.size() * 8, hipMemcpyDeviceToHost));
        double seg[7] = {0, 0, 0, 0, 0, 0, 0}; double life = 0;
        for (int64_t t = 0; t < ntiles; t++) { for (int k = 0; k < 7; k++) seg[k] += (double)(pr[8 * t + k + 1] - pr[8 * t + k]); life += (double)(pr[8 * t + 7] - pr[8 * t]); }
        fprintf(stderr, "[k_map profile] %lld tiles, kernel %.3f ms, tile lifetime %.2f us: stage loads -> LDS %.2f | single-run records + first gathers %.2f | barrier %.2f | "
                        "multi-op walk %.2f | candidate gathers + resolve %.2f | scan %.2f | flush %.2f us\n", (long long)ntiles, ms, life / ntiles / 100.0,
                seg[0] / ntiles / 100.0, seg[1] / ntiles / 100.0, seg[2] / ntiles / 100.0, seg[3] / ntiles / 100.0, seg[4] / ntiles / 100.0, seg[5] / ntiles / 100.0, seg[6] / ntiles / 100.0);
        return PHZ_OK;
    }
    // ---- the overflow area: did every dense tile of the last attempt find room; if not, sized for the calls of all dense tiles (+ slack for the next submission)
    bool overflow_area_held() const { return (int64_t)*scal.cursor(ctx->h_scalars) <= ctx->map.ovf_cap; }
    void grow_overflow_area() { const unsigned long long need = *scal.cursor(ctx->h_scalars); ctx->map.ovf_cap = (int64_t)need + (int64_t)(need / 16) + 4096; }
    // ---- timing; calls per shard, PHZ_E_CAPACITY when a shard's buffers were too small for them (its first `cap` calls are in place)
    int results() {
        ctx->last_ms[PHZ_T_MAP] = ms_total; ctx->total_ms[PHZ_T_MAP] += ms_total; ctx->launches[PHZ_T_MAP]++;
        if (narrow) ctx->counters[PHZ_C_MAP_NARROW]++;
        int st = PHZ_OK;
        for (int k = 0; k < m; k++) {
            const int i = live[(size_t)k];
            n_calls[i] = (int64_t)scal.shard_calls(ctx->h_scalars, k);
            if (n_calls[i] > out[i].cap) st = PHZ_E_CAPACITY;
        }
        return st;
    }
};

}  // namespace

// All shards of a submission run through ONE grid per stage (pre-pass, k_map, tile scan, per-shard totals, compaction): a whole
// genome is 5 launches and one host wait (no read-back copy: the totals kernel stores the host's words itself), with no per-shard ramp-up / tail.
// (Tried and dropped, round 3: k_map writing every call to its final place, the calls before a tile found by decoupled look-back over
// per-tile status words -- no staging, no k_compact.  A tile knows its count only at the END of its work (the count needs the quality
// bytes), so its flush waits for every earlier tile still in flight: 3.01 ms against 1.32 + 0.16 ms for k_map + k_compact.)  A batch whose densest tiles overflow
// the staging area is redone with a larger overflow area (rare: its size is kept across calls).
static int launch_map_batch(phz_ctx *ctx, int n, const phz_reads *r, const phz_variants *v, int baseq, const phz_calls *out, int64_t *n_calls) {
    for (int i = 0; i < n; i++) n_calls[i] = 0;
    if (n <= 0) return PHZ_OK;
    MapSubmission sub(ctx, n, r, v, baseq, out, n_calls);
    if (int s = sub.live_shards_and_tiles()) return s;
    if (sub.m == 0) return PHZ_OK;
    if (int s = sub.shard_table()) return s;
    if (int s = sub.reserve()) return s;
    for (int attempt = 0; ; attempt++) {
        if (int s = sub.attempt()) return s;
        if (sub.overflow_area_held()) break;
        if (attempt == 2) return phz_fail(ctx, PHZ_E_HIP, "K_map staging overflow area did not converge");
        sub.grow_overflow_area();
    }
    return sub.results();
}

int phz_launch_map_batch(phz_ctx *ctx, int n, const phz_reads *r, const phz_variants *v, int baseq, const phz_calls *out,
                         int64_t *n_calls) {
    const int s = launch_map_batch(ctx, n, r, v, baseq, out, n_calls);
    // map.tab_image and map.ovf_image claim "these bytes are in ctx->map.tab".  A submission that failed anywhere between an upload and its stream wait may not
    // have delivered them: forget both.
    if (s != PHZ_OK && s != PHZ_E_CAPACITY) { ctx->map.tab_image.clear(); ctx->map.tab_dev = nullptr; memset(ctx->map.ovf_image, 0, sizeof ctx->map.ovf_image); }
    return s;
}

int phz_launch_map(phz_ctx *ctx, const phz_reads &r, const phz_variants &v, int baseq, const phz_calls &out,
                   int64_t *n_calls) {
    return phz_launch_map_batch(ctx, 1, &r, &v, baseq, &out, n_calls);
}
