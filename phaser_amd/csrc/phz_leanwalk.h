// Per-op step of K_map's lean walker (walk_lean, phz_map.hip): plain C++, compiled by hipcc for the device and by any host compiler for the unit
// test (tests/test_lean_walk.py).  The walker visits the packed CIGAR words of one multi-op record (len << 4 | op) in order; this header holds the
// POSITION RULE of one visit -- where the op's aligned run lies, what inserted text its last base carries, what the op does to the walk's state and
// whether the record has left what the lean walker can express.  The window search, the candidate buffer and the ballots stay in the kernel.
//
// The rule is walk_read<0>'s (phz_map.hip), restricted to what one pass with two carried insertions can express:
//   * an M / = / X / D op of `len` bases at reference offset g covers [pos + g, pos + g + len); every het SNP inside is a candidate, with the read
//     offset r + (vp - lo) for M / = / X and none for D;
//   * insertions follow the reference's keying (key = reference offset - 1 at the I op, looked up SEGMENT-relative): while seg_start is 0 that is
//     the last base of the op before the I (lean_ins_ahead, from the NEXT word); after an N the key lands seg_start bases further on, i.e. in a
//     later run of the same segment (carried in two slots, the later insertion wins: lean_ins_carried);
//   * what the pass cannot express POISONS the record (it is left to the general walker): a 'G' op, a third insertion, an insertion directly after
//     I / S / H / P / G or after a zero-length op, a run that ends beyond `cover` (the end of what the staged window is known to hold).
//
// Every per-lane flag is an INTEGER, taken from bit tables by and / shift: a loop-carried `bool` that differs per lane lives as a 64-bit lane mask
// in a scalar register pair on gfx950, and every update of it inside a divergent loop is an and-not / and / or triple on the scalar unit, per loop
// level.  The walker's instruction stream is bound by that unit, not by the vector ALUs.
//
// LEAN_NEUTRAL is a word that changes nothing: a zero-length 'P'.  It is not a run, not an insertion, not 'G', advances neither offset, and no
// 'I' can follow it inside one record (the walker feeds it to the lanes whose record has ended, so that a wave's trip count is uniform).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PHZ_LW_FN __device__ __forceinline__
#else
#define PHZ_LW_FN inline
#endif

// all ones when bit `op` of `table` is set, else 0
PHZ_LW_FN uint32_t lean_mask(uint32_t table, uint32_t op) {
#if defined(__HIP_DEVICE_COMPILE__)
    // one signed bit-field extract: no compare into VCC and no hazard wait before a select (written as plain arithmetic the compiler folds it
    // back into that pair)
    return (uint32_t)__builtin_amdgcn_sbfe((int)table, op, 1u);
#else
    return 0u - ((table >> op) & 1u);
#endif
}

constexpr uint32_t LEAN_OP_I = 1, LEAN_OP_N = 3;
constexpr uint32_t LEAN_T_MLIKE = 0x181u;      // M = X: a base of the read under every position
constexpr uint32_t LEAN_T_SEARCH = 0x185u;     // M D = X: an aligned run, het SNPs are looked for under it
constexpr uint32_t LEAN_T_REF = 0x38Du;        // M D N = X G advance the reference
constexpr uint32_t LEAN_T_READ = 0x193u;       // M I S = X advance the read
constexpr uint32_t LEAN_T_NOINS = 0x272u;      // I S H P G: an insertion directly after one of these is left to the general walker
constexpr uint32_t LEAN_T_G = 0x200u;
constexpr uint32_t LEAN_NEUTRAL = 6u;          // 0P
constexpr uint32_t LEAN_INS_MAX = 4095u;       // inserted-text length field of a candidate: 12 bits

struct LeanWalk {
    int g;                  // reference offset of the next op from the record's position
    uint32_t r;             // read offset of the next op
    int seg_start;          // reference offset at which the current N-split segment starts
    int cnt;                // candidates so far (the ordinal of the next one)
    uint32_t nins;          // insertions so far
    int t0, t1;             // keys (reference offsets from the record's position) of the two carried insertions, -1 = none; t0 is the later one
    uint32_t x0, x1;        // their inserted-text words, read offset << 12 | length
    uint32_t prev, prev_len;   // one-hot op bit and length of the previous op
    uint32_t bad;           // poison flag: non-zero <=> the record is left to the general walker
};

PHZ_LW_FN void lean_init(LeanWalk &s) {
    s.g = 0; s.r = 0; s.seg_start = 0; s.cnt = 0; s.nins = 0; s.t0 = -1; s.t1 = -1; s.x0 = 0; s.x1 = 0;
    s.prev = 0x10u; s.prev_len = 1; s.bad = 0;          // "previous op" of the first op: S-like
}

// what the kernel needs for one op
struct LeanOp {
    int lo, hi;             // het SNPs at positions [lo, hi) are candidates of this op; empty (hi == lo) unless the op is a clean aligned run
    uint32_t mlike;         // all ones: every candidate has a read base, at read offset rbase + (vp - lo); 0: none (a deleted base)
    uint32_t rbase;         // read offset of the op's first base
    uint32_t rnext;         // read offset behind the op: where the text of an insertion that follows it starts
    uint32_t search;        // all ones when the op is an aligned run (the window search can be skipped when no lane of the wave has one)
};

// one op: the interval to search, and the state update.  `pos` is the record's position, `cover` the end of what the staged window holds.
PHZ_LW_FN LeanOp lean_step(LeanWalk &s, uint32_t w, int pos, long long cover) {
    const int len = (int)(w >> 4); const uint32_t op = w & 15u, bit = 1u << op;
    LeanOp o;
    o.mlike = lean_mask(LEAN_T_MLIKE, op);
    o.search = lean_mask(LEAN_T_SEARCH, op);
    if (op == LEAN_OP_I) {
        // after I / S / H / P / G / an empty op; a third insertion
        s.bad |= (s.prev & LEAN_T_NOINS) | (uint32_t)(s.prev_len == 0) | (uint32_t)(s.nins == 2);
        s.nins++;
        const uint32_t l = (uint32_t)len > LEAN_INS_MAX ? LEAN_INS_MAX : (uint32_t)len;
        s.t1 = s.t0; s.x1 = s.x0; s.t0 = s.g - 1 + s.seg_start; s.x0 = (s.r << 12) | l;
    }
    s.bad |= bit & LEAN_T_G;
    o.lo = pos + s.g;
    s.bad |= o.search & (uint32_t)((long long)o.lo + len > cover);          // the run must lie inside the staged window
    o.hi = o.lo + (s.bad == 0 ? (len & (int)o.search) : 0);
    o.rbase = s.r;
    s.g += len & (int)lean_mask(LEAN_T_REF, op);
    s.r += (uint32_t)len & lean_mask(LEAN_T_READ, op);
    o.rnext = s.r;
    if (op == LEAN_OP_N) { s.seg_start = s.g; s.t0 = -1; s.t1 = -1; }
    s.prev = bit; s.prev_len = (uint32_t)len;
    return o;
}

// inserted text of a candidate in the first segment (seg_start == 0 before the op): the op's LAST base carries the insertion that directly follows
// the op.  `wnext` is the record's next word, or LEAN_NEUTRAL behind its last one.  -> read offset << 12 | length, 0 = none
PHZ_LW_FN uint32_t lean_ins_ahead(const LeanOp &o, int vp, uint32_t wnext) {
    if (vp != o.hi - 1 || (wnext & 15u) != LEAN_OP_I) return 0u;
    const uint32_t l = (wnext >> 4) > LEAN_INS_MAX ? LEAN_INS_MAX : (wnext >> 4);
    return l ? ((o.rnext << 12) | l) : 0u;
}

// inserted text of a candidate in a later segment: a carried insertion whose key is the candidate's offset from the record's position
PHZ_LW_FN uint32_t lean_ins_carried(const LeanWalk &s, int vp, int pos) {
    const int off = vp - pos;
    const uint32_t x = s.t0 == off ? s.x0 : (s.t1 == off ? s.x1 : 0u);
    return (x & LEAN_INS_MAX) ? x : 0u;
}
