// K_tally family: what phaser/phaser.py does between the mapper's call files and the binomial test, for ANY number of
// (chromosome, BAM) shards in one submission (variant and QNAME ids are offset per chromosome into one index space, so a whole
// genome is one call and nothing ever pairs across chromosomes):
//   k_as_hist      :545-553   AS column histogram (host turns it into numpy.percentile's value)
//   k_tile_base               window base of every tile of 1,024 call lines: the variant of its first line, made monotone over the shard's tiles
//   k_line         :1287-1328 process_mapping_result: AS cutoff, allele class, first-appearance index; per TILE the kept lines of every
//                             (window variant, class) -- the band matrix M -- and the tile's QNAMEs as bits of two bitmaps over the QNAME ids
//                             ("seen by a tile", "seen by a second tile")
//   k_colscan                 column sums and column prefixes of M: per-variant line counters, lines per (variant, allele, BAM) read list, and
//                             for every (tile, list) the number of the list's entries in EARLIER tiles -- so that k_tile can put a read-list
//                             entry at its final, line-ordered place (:1318, :917-931, :1086-1115) without a sort
//   k_tile         :636-640, :558-581, :1265-1285  the lines of a QNAME are its mates' records, a few hundred bases apart: nearly every QNAME has
//                             all its lines inside one tile.  A workgroup groups its tile's lines by QNAME in LDS (hash on the id); a group whose
//                             QNAME no other tile has seen is finished in place: sorted, its first ref/alt line, the connectivity-map rank of its
//                             variants, the distinct (variant, class) items and the per-variant distinct-QNAME counters.  Lines of the few QNAMEs
//                             that straddle tiles (or BAMs) are spilled.  Read-list entries go straight to their place: list start + entries in
//                             earlier tiles (k_colscan) + entries in earlier rows of the tile + rank inside the row (wave ballots)
//   k_groups                  the spilled QNAMEs (a per cent of them): gathered into groups through cursors, one thread per group, incl. the
//                             owner BAM of the read_vars list ("last BAM wins", stale-variable quirk)
//   k_pairs        :1602-1632 every QNAME contributes one count to cell (class_a, class_b) of every variant pair it touches -- the nine set
//                             intersections of test_variant_connection for all pairs at once (LDS hash -> global hash)
//   k_edge_*                  edge list in (a, b) order: counting sort by a over the USED hash slots, tiny groups sorted by b; the table is
//                             cleaned slot by slot while it is read (no per-call memset of a 400 MB table)
//   k_rl_sort_dirty           the few read lists with a line outside its tile's variant window (a read spliced over hundreds of het SNPs) are
//                             filled through cursors and sorted afterwards
//   k_components   :1861-1882/:1985-1998 connected components (lock-free union-find)
// Integer work, hand-written kernels and primitives only (phz_sort.h).  Nothing is swept by the number of QNAME ids per call except two
// bitmaps (one bit per id each, cleared per call); the per-QNAME cursor array is touched for spilled QNAMEs only and returns to zero.
#include <cmath>
#include <cstring>
#include "phz_internal.h"
#include "phz_sort.h"
#include "phz_uf.h"

namespace {

constexpr uint64_t KEY_DROPPED = ~0ull;
// Statistics that every workgroup of a kernel adds to live in SPREAD counters: N_SPREAD copies, one memory sector each, picked by the
// workgroup number (atomics on one address are served one after the other, ~8 ns each: ten thousand workgroups x 3 counters on one sector
// would be a quarter of a millisecond of queueing); the host adds the copies up.  spread[c][0] distinct items, [1] pair events, [2] kept lines
constexpr int N_SPREAD = 32, SPREAD_WORDS = 8;
constexpr int AS_LDS_BINS = 8192;       // AS in [-4096, 4096) is histogrammed in LDS

struct LinesDev {
    int64_t n;
    const int32_t *read_idx, *var_idx;
    const uint8_t *code;
    const int32_t *read_qid, *read_as;
    const uint8_t *read_has_as;
    double cutoff;
    int use_cutoff, bam;
    int32_t var_base;          // first variant of the shard's chromosome in the call's variant space
    uint32_t qid_base;         // first QNAME id of the shard's chromosome in the call's id space
    int64_t line_base;         // index of the shard's first line in the call's line space (shards ordered chromosome, BAM)
    const int16_t *read_as16;  // 2-byte AS plane with the has-AS flag folded in (phz.h), or NULL
    int32_t nv_chrom;          // variants of the shard's chromosome: [var_base, var_base + nv_chrom) of the call's variant space
    const double *cut_dev;     // phz_lines.as_cutoff_dev: {cutoff, found, ...} computed on the device (phz_as_cutoff_enqueue), or NULL
};
// AS of record r from whichever form the shard carries; false = the record has no AS tag.  *range = the value lies outside the band the
// histogram accepts (the caller refuses the input)
__device__ __forceinline__ bool as_of(const LinesDev &L, int r, int *a, bool *range) {
    if (L.read_as16) {
        const int x = L.read_as16[r];
        *a = x; *range = x == PHZ_AS16_RANGE || x == -PHZ_AS16_RANGE;
        return x != PHZ_AS16_NONE;
    }
    if (L.read_has_as && !L.read_has_as[r]) { *a = 0; *range = false; return false; }
    const int x = L.read_as[r];
    *a = x; *range = x < -32768 || x >= 32768;
    return true;
}

// All shards of a call go through ONE grid per per-line stage: block b belongs to the shard s with blk0[s] <= b < blk0[s+1]
// (a genome is 22+ shards of well under a million lines each: one launch per shard is mostly ramp-up and tail).
struct LinesTab {
    const LinesDev *L;
    const uint32_t *blk0;      // [n + 1]
    int n;
};
__device__ __forceinline__ int tab_find(const LinesTab &t, uint32_t blk) {
    int lo = 0, hi = t.n - 1;          // largest s with blk0[s] <= blk (shards without blocks share their successor's start)
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (t.blk0[m] <= blk) lo = m; else hi = m - 1;
    }
    return lo;
}
// BAM of a line of the call's line space (shards ordered by line_base)
__device__ __forceinline__ int bam_of_line(const LinesTab &t, uint32_t g) {
    int lo = 0, hi = t.n - 1;
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if ((uint64_t)t.L[m].line_base <= g) lo = m; else hi = m - 1;
    }
    return t.L[lo].bam;
}

__global__ __launch_bounds__(256) void k_as_hist(LinesTab T, unsigned long long *hist, unsigned int *out_of_range) {
    const int sh_ = tab_find(T, blockIdx.x);
    const LinesDev L = T.L[sh_];
    const uint32_t bx = blockIdx.x - T.blk0[sh_], gx = T.blk0[sh_ + 1] - T.blk0[sh_];
    __shared__ unsigned int s_h[AS_LDS_BINS];
    for (int j = threadIdx.x; j < AS_LDS_BINS; j += 256) s_h[j] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < L.n; i += (int64_t)gx * 256) {
        const int r = L.read_idx[i];
        int a; bool range;
        if (!as_of(L, r, &a, &range)) continue;
        const int b = a + AS_LDS_BINS / 2;
        if (range) { if (out_of_range) atomicOr(out_of_range, 1u); }    // an alignment score outside int16: the caller refuses the input
        else if ((unsigned)b < (unsigned)AS_LDS_BINS) atomicAdd(&s_h[b], 1u);
        else atomicAdd(&hist[a + 32768], 1ull);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < AS_LDS_BINS; j += 256)
        if (s_h[j]) atomicAdd(&hist[j - AS_LDS_BINS / 2 + 32768], (unsigned long long)s_h[j]);
}

// the occupied bins of the 64 Ki-bin histogram as (bin, count) pairs (alignment scores live in a narrow band: a few dozen bins), so that the
// host reads a few hundred bytes instead of 512 KB.  One thread per bin, one cursor step per workgroup with occupied bins: the pairs come out
// in no particular order (the caller sorts the handful); n_out[0] = number of pairs (may exceed cap: the caller then takes the dense path)
__global__ __launch_bounds__(1024) void k_hist_compact(const unsigned long long *hist, int cap, int32_t *bins, unsigned long long *counts, int32_t *n_out) {
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bin = blockIdx.x * 1024 + tid;
    const unsigned long long c = hist[bin];
    const unsigned long long m = __ballot(c != 0ull);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int w = 0; w < 16; w++) { const int x = s_w[w]; s_w[w] = tot; tot += x; }
        s_base = tot ? atomicAdd(n_out, tot) : 0;
    }
    __syncthreads();
    if (c) {
        const int at = s_base + s_w[wave] + __popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
        if (at < cap) { bins[at] = bin; counts[at] = c; }
    }
}

// ------------------------------------------------------------------------------------------------ tiles, windows, the per-line pass
// Call lines arrive in mapper order (record, then variant) and records are coordinate-sorted, so a TILE of TL consecutive lines of a shard
// touches a narrow run of variant indices -- its WINDOW [wb, wb + TWT) -- and deeply covered variants repeat hundreds of times in a row.
// k_line and k_tile work on the same tiles (workgroup = tile) and the same windows.
constexpr int TW = 1024;            // variants per LDS window of k_groups
#ifndef PHZ_TALLY_TILE
#define PHZ_TALLY_TILE 1024        // (the emulation tests also build a 256-line variant so that small fixtures straddle tiles)
#endif
constexpr int TL = PHZ_TALLY_TILE; // lines per tile
static_assert(TL == 1024 || TL == 512 || TL == 256, "tile of 256 / 512 / 1024 lines");
constexpr int TWT = 256;           // variants per tile window (1,024 lines span ~100 variants)
constexpr int QW = 16384;          // QNAME ids of the LDS bitmap of k_line (a tile's QNAMEs: the ids handed out while its ~4,000 records went by, and their mates')
#ifndef PHZ_LINE_TB
#define PHZ_LINE_TB 512
#endif
constexpr int LINE_TB = PHZ_LINE_TB < TL ? PHZ_LINE_TB : TL;   // threads per workgroup of k_line

// Window base of every tile: the variant of the tile's first line minus a little room (mate pairs / overlapping records), then made
// non-decreasing over the shard's tiles by a suffix minimum.  (The first line of a tile can sit in the middle of a spliced record, far to the
// right of the records that follow: without the suffix minimum such a tile would push later, lower windows out of order, and k_colscan finds
// the tiles of a variant block by bisection over these bases.)  A line outside its tile's window -- a read spliced over hundreds of het SNPs --
// is a FAR line: global atomics, and its read list is filled through a cursor and sorted afterwards (k_rl_sort_dirty).
// One workgroup per shard.
__global__ __launch_bounds__(256) void k_tile_base(LinesTab TT, int32_t *tile_wb) {
    const LinesDev L = TT.L[blockIdx.x];
    const uint32_t T0 = TT.blk0[blockIdx.x], n = TT.blk0[blockIdx.x + 1] - T0;
    if (n == 0) return;
    __shared__ int s_min[256];
    const uint32_t per = (n + 255u) / 256u;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    int m = 0x7FFFFFFF;
    for (uint32_t t = lo; t < hi; t++) { const int v = L.var_idx[(int64_t)t * TL] + L.var_base; m = v < m ? v : m; }
    s_min[threadIdx.x] = m;
    __syncthreads();
    int after = 0x7FFFFFFF;                                  // minimum over the chunks behind this thread's
    for (int j = threadIdx.x + 1; j < 256; j++) after = s_min[j] < after ? s_min[j] : after;
    for (uint32_t t = hi; t-- > lo;) {
        const int v = L.var_idx[(int64_t)t * TL] + L.var_base;
        after = v < after ? v : after;
        tile_wb[T0 + t] = after - 64 > 0 ? after - 64 : 0;
    }
}

struct LineOut {
    const uint8_t *a0, *a1;
    uint8_t *line_cls;               // [n_lines] 0 ref / 1 alt / 2 other / 255 dropped by the AS cutoff
    uint32_t *line_q;                // [n_lines] QNAME id of the line in the call's id space
    int32_t *var_count;              // [nv*3]   (far lines only: the rest comes from k_colscan)
    unsigned long long *var_first;   // [nv]
    uint32_t *rl_cnt;                // [nv*2*nb] kept ref/alt lines per (variant, allele, BAM)  (far lines only)
    const int32_t *tile_wb;          // [tiles] window base
    uint16_t *tile_m;                // [tiles][TWT*3] kept lines per (window variant, class)
    uint32_t *q_seen, *q_dup;        // one bit per QNAME id: some tile holds a kept line of it / a second tile (or BAM) does too
    uint32_t *rl_dirty, *dirty_list; // one bit per read list: it has a far line; the lists with the bit, once each (cursor: counters[11])
    unsigned long long *counters;    // [12] far lines
    int nb;
    unsigned long long *prof;        // PHZ_TALLY_PROFILE=1: start / end clock of every workgroup
};

__global__ __launch_bounds__(LINE_TB) void k_line(LinesTab T, LineOut O) {
    if (O.prof && threadIdx.x == 0) O.prof[2 * (size_t)blockIdx.x] = wall_clock64();
    const int sh_ = tab_find(T, blockIdx.x);
    const LinesDev L = T.L[sh_];
    const uint32_t bx = blockIdx.x - T.blk0[sh_];
    __shared__ int s_cnt[TWT * 3];
    __shared__ unsigned long long s_first[TWT];
    __shared__ uint32_t s_qb[QW / 32];
    __shared__ unsigned int s_kept, s_far;
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)bx * TL;
    for (int j = tid; j < TWT * 3; j += LINE_TB) s_cnt[j] = 0;
    for (int j = tid; j < TWT; j += LINE_TB) s_first[j] = ~0ull;
    for (int j = tid; j < QW / 32; j += LINE_TB) s_qb[j] = 0u;
    if (tid == 0) { s_kept = 0; s_far = 0; }
    const int wb = O.tile_wb[blockIdx.x];
    // the LDS bitmap covers the QNAME ids around the tile's first line (ids are handed out in coordinate order: a tile's QNAMEs are the
    // ones that first appeared while its records went by, and mates of slightly earlier ones)
    const uint32_t q0 = L.qid_base + (uint32_t)L.read_qid[L.read_idx[i0]];
    const uint32_t qb = q0 > (uint32_t)(QW / 2) ? ((q0 - (uint32_t)(QW / 2)) & ~31u) : 0u;
    unsigned int kept = 0, far = 0;
    // all loads of a lane's lines are requested before the first one is used (two dependent rounds: the line, then its record / variant)
    constexpr int K = TL / LINE_TB;
    int l_r[K], l_v[K], l_as[K]; uint32_t l_q[K]; uint8_t l_code[K], l_a0[K], l_a1[K]; bool l_in[K], l_has[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int64_t i = i0 + tid + LINE_TB * k;
        l_in[k] = i < L.n;
        l_r[k] = l_in[k] ? L.read_idx[i] : 0; l_v[k] = l_in[k] ? L.var_idx[i] + L.var_base : 0; l_code[k] = l_in[k] ? L.code[i] : (uint8_t)4;
    }
    // the cutoff of the shard's BAM: a host value, or the block the device-side percentile left (phz_as_cutoff_enqueue; [1] == 0: no AS tag in the BAM, every line kept)
    const bool use_cut = L.use_cutoff != 0 && (L.cut_dev == nullptr || L.cut_dev[1] != 0.0);
    const double cut = L.cut_dev != nullptr ? L.cut_dev[0] : L.cutoff;
    if (bx == 0 && tid == 0 && L.cut_dev != nullptr && L.cut_dev[2] != 0.0) O.counters[13] = 1ull;      // the histogram saw an AS value outside int16: phz_tally refuses the input at its first wait
#pragma unroll
    for (int k = 0; k < K; k++) {
        l_as[k] = 0; l_has[k] = true;
        if (l_in[k] && use_cut) { bool range; l_has[k] = as_of(L, l_r[k], &l_as[k], &range); }
        l_q[k] = l_in[k] ? L.qid_base + (uint32_t)L.read_qid[l_r[k]] : 0u;
        l_a0[k] = l_in[k] ? O.a0[l_v[k]] : (uint8_t)0; l_a1[k] = l_in[k] ? O.a1[l_v[k]] : (uint8_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (!l_in[k]) continue;
        const int64_t g = L.line_base + i0 + tid + LINE_TB * k;
        const int v = l_v[k];
        const bool keep = !use_cut || (l_has[k] && (double)l_as[k] >= cut);
        if (!keep) { O.line_cls[g] = 255; continue; }
        kept++;
        const uint8_t c = l_code[k];
        // codes 5 / 6 come from the general (indel) mapper, which compared the text with the allele strings itself
        const int cls = c == 5 ? 0 : (c == 6 ? 1 : ((c < 4 && c == l_a0[k]) ? 0 : ((c < 4 && c == l_a1[k]) ? 1 : 2)));
        O.line_cls[g] = (uint8_t)cls;
        O.line_q[g] = l_q[k];
        const unsigned d = (unsigned)(v - wb);
        if (d < (unsigned)TWT) {
            atomicAdd(&s_cnt[d * 3 + cls], 1);
            atomicMin(&s_first[d], (unsigned long long)g);
        } else {                                                 // a far line
            far++;
            atomicAdd(&O.var_count[(int64_t)v * 3 + cls], 1);
            atomicMin(&O.var_first[v], (unsigned long long)g);
            if (cls < 2) {
                const uint32_t e = ((uint32_t)v * 2u + (uint32_t)cls) * (uint32_t)O.nb + (uint32_t)L.bam;
                atomicAdd(&O.rl_cnt[e], 1u);
                const uint32_t bit = 1u << (e & 31u);
                if (!(atomicOr(&O.rl_dirty[e >> 5], bit) & bit)) O.dirty_list[atomicAdd(&O.counters[11], 1ull)] = e;      // the first far line of the list puts it on the work list
            }
        }
        const uint32_t dq = l_q[k] - qb;
        if (dq < (uint32_t)QW) atomicOr(&s_qb[dq >> 5], 1u << (dq & 31u));
        else {                                                   // outside the LDS bitmap (a deep region: mates thousands of ids back): straight to the global ones.  Two such
            const uint32_t bit = 1u << (l_q[k] & 31u);           // lines of one tile make their QNAME look shared -- it then takes the general (spill) path, which is always right
            if (atomicOr(&O.q_seen[l_q[k] >> 5], bit) & bit) atomicOr(&O.q_dup[l_q[k] >> 5], bit);
        }
    }
    if (kept) atomicAdd(&s_kept, kept);
    if (far) atomicAdd(&s_far, far);
    __syncthreads();
    // the tile's row of M, two 16-bit counters per store (a tile holds at most TL <= 1,024 lines)
    {
        uint32_t *row = (uint32_t *)(O.tile_m + (size_t)blockIdx.x * (TWT * 3));
        for (int j = tid; j < TWT * 3 / 2; j += LINE_TB) row[j] = (uint32_t)s_cnt[2 * j] | ((uint32_t)s_cnt[2 * j + 1] << 16);
    }
    for (int j = tid; j < TWT; j += LINE_TB) {
        const unsigned long long f = s_first[j];
        if (f != ~0ull) atomicMin(&O.var_first[wb + j], f);
    }
    // the tile's QNAMEs: one atomic per occupied word; the bits somebody else had set before mark QNAMEs that live in more than one tile
    for (int j = tid; j < QW / 32; j += LINE_TB) {
        const uint32_t bits = s_qb[j];
        if (bits) {
            const uint32_t w = (qb >> 5) + (uint32_t)j;
            const uint32_t dup = atomicOr(&O.q_seen[w], bits) & bits;
            if (dup) atomicOr(&O.q_dup[w], dup);
        }
    }
    if (tid == 0 && s_kept) atomicAdd(&O.counters[16 + (blockIdx.x % N_SPREAD) * SPREAD_WORDS + 2], (unsigned long long)s_kept);
    if (tid == 0 && s_far) atomicAdd(&O.counters[12], (unsigned long long)s_far);
    if (O.prof && tid == 0) O.prof[2 * (size_t)blockIdx.x + 1] = wall_clock64();
}

// Columns of the band matrix M (tiles x variants): for every variant of a block of TWT variants the kept lines per class over all tiles of the
// shard -- the per-variant counters and the sizes of the read lists -- and, tile by tile, the running sum BEFORE the tile (tile_b), i.e. the
// number of entries of list (variant, allele, BAM) that lie in earlier tiles = earlier lines.  One workgroup per (shard, variant block); its
// tiles are found by bisection over the monotone window bases; long tile ranges (deep coverage) are cut into CS_PARTS parts that first add up
// their own stretch.
constexpr int CS_PARTS = 4;
struct ColScan { const int32_t *tile_wb; const uint16_t *tile_m; uint32_t *tile_b; int32_t *var_count; uint32_t *rl_cnt; int nb; };
__global__ __launch_bounds__(TWT * CS_PARTS) void k_colscan(LinesTab TC, LinesTab TT, ColScan O) {
    const int sh_ = tab_find(TC, blockIdx.x);
    const LinesDev L = TC.L[sh_];
    const int blk = (int)(blockIdx.x - TC.blk0[sh_]);
    const int a = L.var_base + blk * TWT;                        // first variant of the block
    const int j = threadIdx.x & (TWT - 1), part = threadIdx.x / TWT;
    const int v = a + j;
    const bool live = blk * TWT + j < L.nv_chrom;
    const uint32_t T0 = TT.blk0[sh_], T1 = TT.blk0[sh_ + 1];
    // tiles whose window [wb, wb + TWT) meets [a, a + TWT): a - TWT < wb < a + TWT
    uint32_t lo, hi;
    { uint32_t x = T0, y = T1; while (x < y) { const uint32_t m = (x + y) >> 1; if (O.tile_wb[m] > a - TWT) y = m; else x = m + 1; } lo = x; }
    { uint32_t x = lo, y = T1; while (x < y) { const uint32_t m = (x + y) >> 1; if (O.tile_wb[m] >= a + TWT) y = m; else x = m + 1; } hi = x; }
    const uint32_t n = hi - lo;
    const bool split = n > 16u;
    const uint32_t per = split ? (n + CS_PARTS - 1) / CS_PARTS : n;
    uint32_t t0 = lo + (uint32_t)part * per; t0 = t0 < hi ? t0 : hi;
    const uint32_t t1 = t0 + per < hi ? t0 + per : hi;
    __shared__ uint32_t s_tot[CS_PARTS][TWT * 3];
    uint32_t off0 = 0, off1 = 0, off2 = 0;
    if (split) {
        uint32_t c0 = 0, c1 = 0, c2 = 0;
#pragma unroll 4
        for (uint32_t t = t0; t < t1; t++) {
            const unsigned d = (unsigned)(v - O.tile_wb[t]);
            if (d < (unsigned)TWT) { const uint16_t *m = O.tile_m + (size_t)t * (TWT * 3) + d * 3; c0 += m[0]; c1 += m[1]; c2 += m[2]; }
        }
        s_tot[part][j * 3] = c0; s_tot[part][j * 3 + 1] = c1; s_tot[part][j * 3 + 2] = c2;
        __syncthreads();
        for (int p = 0; p < part; p++) { off0 += s_tot[p][j * 3]; off1 += s_tot[p][j * 3 + 1]; off2 += s_tot[p][j * 3 + 2]; }
    }
    uint32_t r0 = off0, r1 = off1, r2 = off2;
#pragma unroll 4
    for (uint32_t t = t0; t < t1; t++) {
        const unsigned d = (unsigned)(v - O.tile_wb[t]);
        if (d < (unsigned)TWT) {
            const uint16_t *m = O.tile_m + (size_t)t * (TWT * 3) + d * 3;
            uint32_t *bb = O.tile_b + (size_t)t * (TWT * 2) + d * 2;
            const uint32_t c0 = m[0], c1 = m[1], c2 = m[2];
            bb[0] = r0; bb[1] = r1;
            r0 += c0; r1 += c1; r2 += c2;
        }
    }
    if (!live) return;
    r0 -= off0; r1 -= off1; r2 -= off2;                          // this part's own lines (several BAMs of a chromosome add to the same variant: atomics)
    if (r0) { atomicAdd(&O.var_count[(int64_t)v * 3], (int)r0); atomicAdd(&O.rl_cnt[((uint32_t)v * 2u) * (uint32_t)O.nb + (uint32_t)L.bam], r0); }
    if (r1) { atomicAdd(&O.var_count[(int64_t)v * 3 + 1], (int)r1); atomicAdd(&O.rl_cnt[((uint32_t)v * 2u + 1u) * (uint32_t)O.nb + (uint32_t)L.bam], r1); }
    if (r2) atomicAdd(&O.var_count[(int64_t)v * 3 + 2], (int)r2);
}

// group of every spilled QNAME: its line count (the counter goes back to zero and serves as the fill cursor of k_items_spill)
__global__ __launch_bounds__(256) void k_group_plan(int64_t nt, const uint32_t *touched, uint32_t *qcount, uint32_t *cnt_t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const uint32_t q = touched[i];
    cnt_t[i] = qcount[q]; qcount[q] = 0u;                        // the spilled lines of the QNAME, added up by the tiles that hold them
}
// ... and the counter becomes the QNAME's write cursor: it starts at the group's base, k_items takes slots from it, k_groups returns it to zero
__global__ __launch_bounds__(256) void k_group_base(int64_t nt, const uint32_t *touched, const uint32_t *base_t, uint32_t *qcount) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nt) qcount[touched[i]] = base_t[i];
}
// item = variant:28 | class:2 | line:32 (sorts by variant, class, line); read-list entry = line:32 | chromosome-local QNAME id:32
__device__ __forceinline__ uint64_t item_pack(uint32_t v, uint32_t cls, uint32_t g) { return ((uint64_t)v << 34) | ((uint64_t)cls << 32) | g; }
// distinct item of a group = QNAME id:32 | variant:28 << 4 | class << 2 | linked (the QNAME id in the high word keeps the groups apart in k_pairs)
__device__ __forceinline__ uint64_t dist_pack(uint32_t q, uint32_t v, uint32_t cls, uint32_t linked) { return ((uint64_t)q << 32) | ((uint64_t)v << 4) | ((uint64_t)cls << 2) | linked; }

constexpr int TH = 2 * TL;         // LDS hash slots (at most TL distinct QNAMEs: load factor <= 0.5)
#ifndef PHZ_TILE_TB
#define PHZ_TILE_TB 512
#endif
constexpr int TILE_TB = PHZ_TILE_TB < TL ? PHZ_TILE_TB : TL;   // threads per workgroup of k_tile
constexpr int TSP = TH / TILE_TB;  // slots per thread
constexpr int TH_SHIFT = TL == 1024 ? 21 : (TL == 512 ? 22 : 23);
constexpr int NROWS = TL / 64;     // rows of 64 consecutive lines in a tile (a wave holds one row per round)
constexpr uint32_t Q_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t RL_DIRTY = 0xFFFFFFFFu;      // base of a dirty list in the tile's LDS table: its entries go through the cursor

struct TileOut {
    const uint8_t *line_cls; const uint32_t *line_q;
    const uint32_t *q_dup;           // bit per QNAME id: lines in more than one tile / BAM (k_line)
    uint32_t *qcount;                // [nq] spilled lines per QNAME, added up here (all zero between calls; k_group_plan / k_groups return it to zero)
    uint64_t *items;                 // [tiles * TL] distinct items of the complete groups in the slots of their tile, holes = KEY_DROPPED
    uint32_t *sp_q; uint64_t *sp_item;       // spilled lines (cursor: low word of counters[10])
    uint32_t *touched;               // spilled QNAMEs, once each (cursor: high word of counters[10])
    unsigned long long *var_rank; int32_t *var_distinct;
    const int32_t *tile_wb; const uint32_t *tile_b;      // window base; entries of every window list in earlier tiles (k_colscan)
    const uint32_t *rl_start, *rl_dirty;
    int32_t *rl_qid; uint32_t *rl_list;                  // the read lists, written in place
    uint32_t *rl_cursor; uint64_t *rl_tmp;               // dirty lists only: entries in arrival order, line | QNAME id (sorted by k_rl_sort_dirty)
    unsigned long long *counters;
    int nb; int64_t nv;
    unsigned long long *prof;
};

__global__ __launch_bounds__(TILE_TB) void k_tile(LinesTab T, TileOut O) {
    if (O.prof && threadIdx.x == 0) O.prof[2 * (size_t)blockIdx.x] = wall_clock64();
    const int sh_ = tab_find(T, blockIdx.x);
    const LinesDev L = T.L[sh_];
    const uint32_t bx = blockIdx.x - T.blk0[sh_];
    __shared__ uint32_t s_q[TH];                 // QNAME id of the slot
    __shared__ uint32_t s_c[TH];                 // lines of the slot's QNAME in this tile -> write cursor of its group -> end of its group (groups lie in slot order)
    __shared__ uint64_t s_it[TL];                // the tile's kept lines as items, group by group; before that: entries per (row, window list), one byte each
    __shared__ int s_cnt[TWT * 3];
    __shared__ unsigned long long s_rank[TWT];
    __shared__ uint32_t s_rl[TL / 2 > TWT * 2 ? TL / 2 : TWT * 2];   // place of the tile's first entry in every window list (RL_DIRTY: the list goes through its cursor);
                                                 // later: the slots whose QNAMEs this tile puts on the list of spilled QNAMEs (16 bits each)
    __shared__ uint16_t s_grp[TL];               // the occupied slots, densely: group g of the tile lives in slot s_grp[g]
    __shared__ uint32_t s_part[TILE_TB / 64];
    __shared__ uint32_t s_nspill, s_ntouch, s_nkept, s_ngroups;
    __shared__ unsigned long long s_obase;
    uint16_t *s_touch = (uint16_t *)s_rl;
    uint8_t *s_mat = (uint8_t *)s_it;            // [NROWS][TWT * 2]
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t i0 = (int64_t)bx * TL;
    if (tid == 0) { s_nspill = 0; s_ntouch = 0; }
    for (int j = tid; j < TH; j += TILE_TB) { s_q[j] = Q_EMPTY; s_c[j] = 0u; }
    for (int j = tid; j < TWT * 3; j += TILE_TB) s_cnt[j] = 0;
    for (int j = tid; j < TWT; j += TILE_TB) s_rank[j] = ~0ull;
    for (int j = tid; j < TL; j += TILE_TB) s_it[j] = 0ull;
    const int vbase = O.tile_wb[blockIdx.x];
    // ---- 0. where the tile's entries of every window list start: list start + entries in earlier tiles
    for (int x = tid; x < TWT * 2; x += TILE_TB) {
        const int64_t v = (int64_t)vbase + (x >> 1);
        uint32_t base = RL_DIRTY;
        if (v < O.nv) {
            const uint32_t e = ((uint32_t)v * 2u + (uint32_t)(x & 1)) * (uint32_t)O.nb + (uint32_t)L.bam;
            if (!((O.rl_dirty[e >> 5] >> (e & 31u)) & 1u)) base = O.rl_start[e] + O.tile_b[(size_t)blockIdx.x * (TWT * 2) + x];
        }
        s_rl[x] = base;
    }
    // ---- 1. the tile's lines: QNAME -> slot (count); read-list entry -> rank among the row's entries of its list (wave ballots), the row's
    //         entries per list into s_mat
    constexpr int K = TL / TILE_TB;
    uint32_t l_cls[K], l_q[K], l_v[K], l_slot[K], l_rank[K], l_base[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int64_t i = i0 + tid + TILE_TB * k;
        l_cls[k] = 255u; l_q[k] = 0u; l_v[k] = 0u;
        if (i < L.n) {
            const int64_t g = L.line_base + i;
            l_cls[k] = O.line_cls[g]; l_q[k] = O.line_q[g]; l_v[k] = (uint32_t)(L.var_idx[i] + L.var_base);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        l_slot[k] = Q_EMPTY;
        if (l_cls[k] != 255u) {
            const uint32_t q = l_q[k];
            uint32_t s = (q * 2654435761u) >> TH_SHIFT;
            for (;;) {
                const uint32_t prev = atomicCAS(&s_q[s], Q_EMPTY, q);
                if (prev == Q_EMPTY || prev == q) break;
                s = (s + 1) & (TH - 1);
            }
            atomicAdd(&s_c[s], 1u);
            l_slot[k] = s;
        }
        // every lane gets here: the lanes of a row with the same list key find each other by nine ballots
        const bool isrl = l_cls[k] < 2u;
        const unsigned d = l_v[k] - (unsigned)vbase;
        const uint32_t key = (d * 2u + (l_cls[k] & 1u)) & (uint32_t)(TWT * 2 - 1);
        l_base[k] = (isrl && d < (unsigned)TWT) ? s_rl[key] : RL_DIRTY;      // a far line's list is dirty by construction (k_line flagged it)
        const bool ord = isrl && l_base[k] != RL_DIRTY;
        unsigned long long same = __ballot(ord);
#pragma unroll
        for (int b = 0; b < 9; b++) {
            const bool bit = (key >> b) & 1u;
            const unsigned long long bal = __ballot(ord && bit);
            same &= bit ? bal : ~bal;
        }
        const uint32_t inrow = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        l_rank[k] = isrl ? inrow : Q_EMPTY;
        if (ord && inrow == 0u) s_mat[((tid >> 6) + (TILE_TB / 64) * k) * (TWT * 2) + key] = (uint8_t)__popcll(same);
    }
    __syncthreads();
    // ---- 2. read-list entries to their final places (the entries of earlier rows come from s_mat, which step 3 overwrites); meanwhile the
    //         group ranges (exclusive scan of the slot counts)
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (l_rank[k] == Q_EMPTY) continue;
        const int64_t i = i0 + tid + TILE_TB * k;
        const uint32_t g = (uint32_t)(L.line_base + i);
        const uint32_t e = (l_v[k] * 2u + l_cls[k]) * (uint32_t)O.nb + (uint32_t)L.bam;
        if (l_base[k] != RL_DIRTY) {
            const unsigned d = l_v[k] - (unsigned)vbase;
            const uint32_t key = d * 2u + l_cls[k];
            const int row = (tid >> 6) + (TILE_TB / 64) * k;
            uint32_t before = 0;
            for (int r = 0; r < row; r++) before += s_mat[r * (TWT * 2) + key];
            const uint32_t at = l_base[k] + before + l_rank[k];
            O.rl_qid[at] = (int32_t)(l_q[k] - L.qid_base); O.rl_list[at] = e;
        } else {
            const uint32_t at = O.rl_start[e] + atomicAdd(&O.rl_cursor[e], 1u);
            O.rl_tmp[at] = ((uint64_t)g << 32) | (uint32_t)(l_q[k] - L.qid_base); O.rl_list[at] = e;
        }
    }
    {
        // one scan for both: lines (low half) and occupied slots (high half) before every slot
        uint32_t c[TSP], sum = 0;
#pragma unroll
        for (int j = 0; j < TSP; j++) { c[j] = s_c[tid * TSP + j]; sum += c[j] + (c[j] ? 0x10000u : 0u); }
        const uint32_t incl = gs_wave_incl(sum, tid & 63);
        if ((tid & 63) == 63) s_part[tid >> 6] = incl;
        __syncthreads();
        uint32_t base = incl - sum;
        for (int w = 0; w < (tid >> 6); w++) base += s_part[w];
        if (tid == TILE_TB - 1) { s_nkept = (base + sum) & 0xFFFFu; s_ngroups = (base + sum) >> 16; }
#pragma unroll
        for (int j = 0; j < TSP; j++) {
            s_c[tid * TSP + j] = base & 0xFFFFu;
            if (c[j]) s_grp[base >> 16] = (uint16_t)(tid * TSP + j);
            base += c[j] + (c[j] ? 0x10000u : 0u);
        }
    }
    __syncthreads();
    // ---- 3. lines into their groups; whether some other tile holds lines of the QNAMEs of this lane's groups is requested first (used after
    //         the next barrier)
    constexpr int GK = TL / TILE_TB;                            // groups per lane (a tile of TL lines holds at most TL groups)
    const uint32_t ngroups = s_ngroups;
    uint32_t dupw[GK], my_q[GK], my_slot[GK];
#pragma unroll
    for (int j = 0; j < GK; j++) {
        const uint32_t gi = (uint32_t)tid + (uint32_t)TILE_TB * (uint32_t)j;
        my_slot[j] = gi < ngroups ? (uint32_t)s_grp[gi] : Q_EMPTY;
        my_q[j] = my_slot[j] != Q_EMPTY ? s_q[my_slot[j]] : Q_EMPTY;
        dupw[j] = my_q[j] != Q_EMPTY ? O.q_dup[my_q[j] >> 5] : 0u;
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (l_slot[k] == Q_EMPTY) continue;
        const int64_t i = i0 + tid + TILE_TB * k;
        const uint32_t g = (uint32_t)(L.line_base + i);
        s_it[atomicAdd(&s_c[l_slot[k]], 1u)] = item_pack(l_v[k], l_cls[k], g);
    }
    __syncthreads();
    // ---- 4. one thread per group.  A group holding every line of its QNAME is finished here (all its lines come from this shard's BAM: that
    //         BAM owns the read_vars list, every ref/alt line is linked; "all" = no other tile has set the QNAME's bit): its distinct items stay at the front of its range, the rest of the
    //         range becomes KEY_DROPPED.  The others hand their lines to the spill list (ranges inside the tile's share from LDS counters)
    uint32_t sp_beg[GK], sp_n[GK], sp_at[GK];
#pragma unroll
    for (int j = 0; j < GK; j++) {
        sp_n[j] = 0; sp_beg[j] = 0; sp_at[j] = 0;
        if (my_q[j] == Q_EMPTY) continue;
        const int slot = (int)my_slot[j];
        const uint32_t q = my_q[j];
        const uint32_t beg = slot ? s_c[slot - 1] : 0u, n = s_c[slot] - beg;        // the cursors stopped at the groups' ends
        uint64_t *it = s_it + beg;
        if ((dupw[j] >> (q & 31u)) & 1u) {
            if (atomicAdd(&O.qcount[q], n) == 0u) s_touch[atomicAdd(&s_ntouch, 1u)] = (uint16_t)slot;   // the first tile to add its lines lists the QNAME
            sp_n[j] = n; sp_beg[j] = beg; sp_at[j] = atomicAdd(&s_nspill, n);
            continue;
        }
        if (n == 1u) {                                         // most QNAMEs: one line, nothing to sort, no pair, no rank
            const uint64_t x = it[0];
            const uint32_t v = (uint32_t)(x >> 34), cls = (uint32_t)(x >> 32) & 3u;
            const unsigned d = v - (unsigned)vbase;
            if (d < (unsigned)TWT) atomicAdd(&s_cnt[d * 3 + cls], 1); else atomicAdd(&O.var_distinct[(int64_t)v * 3 + cls], 1);
            it[0] = dist_pack(q, v, cls, cls < 2u ? 1u : 0u);
            continue;
        }
        for (uint32_t a = 1; a < n; a++) {
            const uint64_t x = it[a];
            uint32_t b = a;
            while (b > 0 && it[b - 1] > x) { it[b] = it[b - 1]; b--; }
            it[b] = x;
        }
        uint32_t first = 0xFFFFFFFFu, vmin = 0xFFFFFFFFu, vmax = 0;
        for (uint32_t a = 0; a < n; a++) {
            const uint64_t x = it[a];
            if (((x >> 32) & 3ull) >= 2ull) continue;
            const uint32_t g = (uint32_t)x, v = (uint32_t)(x >> 34);
            first = g < first ? g : first;
            vmin = v < vmin ? v : vmin; vmax = v > vmax ? v : vmax;
        }
        const bool multi = vmin != 0xFFFFFFFFu && vmin != vmax;
        uint32_t w = 0, a = 0;
        while (a < n) {
            const uint64_t key = it[a] >> 32;                  // variant:28 | class:2
            const uint32_t v = (uint32_t)(key >> 2), cls = (uint32_t)(key & 3ull);
            const uint32_t gl = (uint32_t)it[a];               // the run is sorted by line: its first line
            while (a < n && (it[a] >> 32) == key) a++;
            const uint32_t linked = cls < 2u ? 1u : 0u;
            const unsigned d = v - (unsigned)vbase;
            if (multi && linked) {
                const unsigned long long rk = ((unsigned long long)first << 32) | gl;
                if (d < (unsigned)TWT) atomicMin(&s_rank[d], rk); else atomicMin(&O.var_rank[v], rk);
            }
            if (d < (unsigned)TWT) atomicAdd(&s_cnt[d * 3 + cls], 1); else atomicAdd(&O.var_distinct[(int64_t)v * 3 + cls], 1);
            it[w++] = dist_pack(q, v, cls, linked);
        }
        for (uint32_t k = w; k < n; k++) it[k] = KEY_DROPPED;
    }
    __syncthreads();
    // ---- 5. ONE global cursor step per tile (spilled lines in the low word, listed QNAMEs in the high word) -- while it is under way the
    //         tile's slots of the item array are written in one sweep (groups in place, holes = KEY_DROPPED) -- then the spilled lines go
    //         out and their slots of the item array are crossed out
    unsigned long long cur = 0;
    if (tid == 0) {
        const unsigned long long add = ((unsigned long long)s_ntouch << 32) | s_nspill;
        if (add) cur = atomicAdd(&O.counters[10], add);
    }
    uint64_t *dst = O.items + ((int64_t)blockIdx.x * TL);
    {
        const uint32_t nk = s_nkept;
        for (int j = tid; j < TL; j += TILE_TB) dst[j] = (uint32_t)j < nk ? s_it[j] : KEY_DROPPED;
    }
    for (int j = tid; j < TWT * 3; j += TILE_TB) {
        const int cc = s_cnt[j];
        if (cc) atomicAdd(&O.var_distinct[(int64_t)(vbase + j / 3) * 3 + (j % 3)], cc);
    }
    for (int j = tid; j < TWT; j += TILE_TB) {
        const unsigned long long f = s_rank[j];
        if (f != ~0ull) atomicMin(&O.var_rank[vbase + j], f);
    }
    if (tid == 0) s_obase = cur;
    __syncthreads();
    if (O.prof && tid == 0) O.prof[2 * (size_t)blockIdx.x + 1] = wall_clock64();
    if (s_nspill == 0) return;
    const uint32_t spill_base = (uint32_t)s_obase, touch_base = (uint32_t)(s_obase >> 32);
#pragma unroll
    for (int j = 0; j < GK; j++) {
        if (!sp_n[j]) continue;
        for (uint32_t a = 0; a < sp_n[j]; a++) {
            O.sp_q[spill_base + sp_at[j] + a] = my_q[j]; O.sp_item[spill_base + sp_at[j] + a] = s_it[sp_beg[j] + a];
            dst[sp_beg[j] + a] = KEY_DROPPED;
        }
    }
    for (uint32_t j = tid; j < s_ntouch; j += TILE_TB) O.touched[touch_base + j] = s_q[s_touch[j]];
}

// the spilled lines into the groups of their QNAMEs (ranges from the scan over the spilled QNAMEs' line counts)
__global__ __launch_bounds__(256) void k_items_spill(int64_t n, const uint32_t *sp_q, const uint64_t *sp_item, uint32_t *qcount, uint64_t *items) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) items[atomicAdd(&qcount[sp_q[i]], 1u)] = sp_item[i];
}

// One thread per QNAME group.  Sorts the group (insertion sort: a QNAME owns a handful of lines), then
//   owner  = last BAM holding a ref/alt line of the QNAME (the stale-variable overwrite at phaser.py:578: a later BAM replaces the read_vars list)
//   first  = first ref/alt line of the QNAME over all BAMs
//   linked = ref/alt line of the owner BAM (an entry of the surviving read_vars list)
//   rank   : overlap-dictionary key order (SURVEY.md 8.1 rule 4, phaser.py:1271-1283): for QNAMEs whose surviving list holds >= 2 distinct
//            variants, every variant gets (first << 32 | its first linked line) as a candidate for its smallest key
//   the distinct (variant, class) items (linked = max over the run of equal lines), written back at the front of the group as
//            QNAME id:32 | variant:28 << 4 | class << 2 | linked (the rest of the group becomes KEY_DROPPED), and the per-variant distinct-QNAME counters
struct GroupOut {
    uint32_t *qcount; uint64_t *items; uint32_t *cnt_t; const uint32_t *base_t, *touched;
    unsigned long long *var_rank; int32_t *var_distinct; unsigned long long *counters;      // [0] distinct items
    int single_bam;
};
__global__ __launch_bounds__(256) void k_groups(int64_t nt, LinesTab T, GroupOut O) {
    __shared__ int s_cnt[TW * 3];
    __shared__ unsigned long long s_rank[TW];
    __shared__ int s_vbase;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    for (int j = tid; j < TW * 3; j += 256) s_cnt[j] = 0;
    for (int j = tid; j < TW; j += 256) s_rank[j] = ~0ull;
    if (tid == 0) { const int64_t i0 = (int64_t)blockIdx.x * 256; s_vbase = (int)(O.items[O.base_t[i0]] >> 34); }
    __syncthreads();
    const int vbase = s_vbase - 256 > 0 ? s_vbase - 256 : 0;
    if (i < nt) {
        const uint32_t b = O.base_t[i], c = O.cnt_t[i];
        O.qcount[O.touched[i]] = 0u;                         // the fill cursor goes back to zero: clean for the next call
        uint64_t *it = O.items + b;
        for (uint32_t a = 1; a < c; a++) {
            const uint64_t x = it[a];
            uint32_t j = a;
            while (j > 0 && it[j - 1] > x) { it[j] = it[j - 1]; j--; }
            it[j] = x;
        }
        int owner = -1; uint32_t first = 0xFFFFFFFFu;
        for (uint32_t a = 0; a < c; a++) {
            const uint64_t x = it[a];
            if (((x >> 32) & 3ull) >= 2ull) continue;
            const uint32_t g = (uint32_t)x;
            first = g < first ? g : first;
            if (!O.single_bam) { const int bm = bam_of_line(T, g); owner = bm > owner ? bm : owner; }
        }
        uint32_t vmin = 0xFFFFFFFFu, vmax = 0;
        for (uint32_t a = 0; a < c; a++) {
            const uint64_t x = it[a];
            if (((x >> 32) & 3ull) >= 2ull) continue;
            if (!O.single_bam && bam_of_line(T, (uint32_t)x) != owner) continue;
            const uint32_t v = (uint32_t)(x >> 34);
            vmin = v < vmin ? v : vmin; vmax = v > vmax ? v : vmax;
        }
        const bool multi = vmin != 0xFFFFFFFFu && vmin != vmax;
        // runs of equal (variant, class): one distinct item each; the variant's first linked line competes for its rank
        uint32_t w = 0, a = 0;
        while (a < c) {
            const uint64_t key = it[a] >> 32;                  // variant:28 | class:2
            const uint32_t v = (uint32_t)(key >> 2), cls = (uint32_t)(key & 3ull);
            uint32_t linked = 0, gl = 0xFFFFFFFFu;
            while (a < c && (it[a] >> 32) == key) {
                const uint32_t g = (uint32_t)it[a];
                if (cls < 2u && (O.single_bam || bam_of_line(T, g) == owner)) { linked = 1u; gl = g < gl ? g : gl; }
                a++;
            }
            if (multi && linked) {
                const unsigned long long rk = ((unsigned long long)first << 32) | gl;
                const unsigned d = (unsigned)((int)v - vbase);
                if (d < (unsigned)TW) atomicMin(&s_rank[d], rk); else atomicMin(&O.var_rank[v], rk);
            }
            {
                const unsigned d = (unsigned)((int)v - vbase);
                if (d < (unsigned)TW) atomicAdd(&s_cnt[d * 3 + cls], 1); else atomicAdd(&O.var_distinct[(int64_t)v * 3 + cls], 1);
            }
            it[w++] = dist_pack(O.touched[i], v, cls, linked);
        }
        for (uint32_t k = w; k < c; k++) it[k] = KEY_DROPPED;
        O.cnt_t[i] = w;
    }
    __syncthreads();
    for (int j = tid; j < TW * 3; j += 256) {
        const int cc = s_cnt[j];
        if (cc) atomicAdd(&O.var_distinct[(int64_t)(vbase + j / 3) * 3 + (j % 3)], cc);
    }
    for (int j = tid; j < TW; j += 256) {
        const unsigned long long f = s_rank[j];
        if (f != ~0ull) atomicMin(&O.var_rank[vbase + j], f);
    }
}

__device__ __forceinline__ uint32_t hash64(uint64_t k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
    return (uint32_t)k;
}

constexpr int PH_SLOTS = 1024;     // LDS hash slots per workgroup
constexpr int PH_WORDS = 5;        // LDS counters of a slot: the nine cells as 16-bit halves (a tile holds < 2^16 QNAMEs), linked flag = bit 16 of word 4
constexpr int PH_PROBES = 24;
constexpr int GH_PROBES = 256;     // global probe bound; beyond it the table is declared too small and the pass is redone with a larger one (once
                                   // that is decided nobody probes any more: a full table made every insertion a walk of the whole bound)
// the global table: one 64-byte entry per slot = one memory sector: key (words 0-1, 0 = empty: a pair key (a << 32 | b) has b > a >= 0),
// the nine cells (words 2-10), the linked flag (word 11)
constexpr int GE_WORDS = 16;
constexpr int GE_CELL0 = 2, GE_LINKED = 11;

// counters[]: 2 global hash overflow, 3 kept lines, 4/5 noise, 7 used hash slots, 10 spilled lines | spilled QNAMEs << 32
// -> slot of the pair in the global table, claiming it if new (*claimed); -1 when the probe bound is hit
// Home slot of a pair: a scattering hash.  (A table kept in variant order -- the pairs of variant a from slot 4a on, so that a tile's pairs
// share a few dozen KB -- was measured: k_pairs 0.38 -> 1.65 ms.  The workgroups in flight work on neighbouring tiles, their atomics
// then queue on the few L2 channels that own that stretch of the table.)
__device__ __forceinline__ uint32_t pair_home(uint64_t key, uint32_t gmask) { return hash64(key) & gmask; }
__device__ __forceinline__ int global_slot(uint32_t *tab, uint32_t gmask, uint64_t key, unsigned long long *counters, bool *claimed) {
    uint32_t s = pair_home(key, gmask);
    *claimed = false;
    for (int t = 0; t < GH_PROBES; t++) {
        // a long probe sequence is the sign of a table that is filling up: look whether the pass is lost already (not on every call: the
        // flag shares a memory sector with the used-slot cursor, and a load per insertion tripled the kernel's time)
        if ((t & 15) == 15 && __hip_atomic_load(&counters[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) return -1;
        const unsigned long long prev = atomicCAS((unsigned long long *)(tab + (size_t)s * GE_WORDS), 0ull, (unsigned long long)key);
        if (prev == 0ull) { *claimed = true; return (int)s; }
        if (prev == key) return (int)s;
        s = (s + 1) & gmask;
    }
    atomicAdd(&counters[2], 1ull);
    return -1;
}

// QNAME groups hold their distinct items sorted by (variant, class): every pair of items on different variants adds 1 to cell
// (class_a, class_b) of that variant pair.  One thread per item slot (the pairs of an item with the later items of its group): PAIR_ITEMS
// slots per workgroup.  The slots this workgroup claims in the global table go to the list of used slots.
constexpr int PAIR_ITEMS = 2048;      // item slots per round
#ifndef PHZ_PAIRS_TB
#define PHZ_PAIRS_TB 512
#endif
constexpr int PAIRS_TB = PHZ_PAIRS_TB;   // threads per workgroup of k_pairs
constexpr int PAIR_ROUNDS = 1;        // rounds per workgroup sharing one LDS table and one flush (2: the table overflows, 0.35 -> 0.43 ms)
template <int MODE> __global__ __launch_bounds__(PAIRS_TB) void k_pairs(const uint64_t *items, int64_t m, uint32_t *tab, uint32_t gmask, uint32_t *used, uint64_t *used_key, uint32_t *deg,
                                                                       unsigned long long *counters) {
    __shared__ unsigned long long s_keys[PH_SLOTS];
    __shared__ uint32_t s_vals[PH_SLOTS * PH_WORDS];
    __shared__ uint32_t s_claim[PH_SLOTS];
    __shared__ uint16_t s_claim_l[PH_SLOTS];     // LDS slot of the claim (its key is still there when the list goes out)
    __shared__ unsigned int s_part[PAIRS_TB / 64], s_ipart[PAIRS_TB / 64], s_nclaim;
    __shared__ unsigned long long s_ubase;
    for (int j = threadIdx.x; j < PH_SLOTS; j += PAIRS_TB) s_keys[j] = KEY_DROPPED;
    for (int j = threadIdx.x; j < PH_SLOTS * PH_WORDS; j += PAIRS_TB) s_vals[j] = 0;
    if (threadIdx.x == 0) s_nclaim = 0;
    __syncthreads();
    unsigned int n_event = 0, n_item = 0;
    constexpr int KI = PAIR_ITEMS / PAIRS_TB;
    // A wave holds 64 consecutive items per round (one per lane) plus the 64 after them: the later items of a lane's group are read from the
    // neighbouring lanes (the groups are a handful of items long), no memory access inside the pair loop
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < PAIR_ROUNDS; round++) {
    const int64_t i0 = ((int64_t)blockIdx.x * PAIR_ROUNDS + round) * PAIR_ITEMS;
    if (i0 >= m) break;
    unsigned long long my_item[KI], nx_item[KI];
#pragma unroll
    for (int t = 0; t < KI; t++) {                           // all of the lane's items requested together
        const int64_t i = i0 + threadIdx.x + PAIRS_TB * t;
        my_item[t] = i < m ? items[i] : KEY_DROPPED;
        nx_item[t] = i + 64 < m ? items[i + 64] : KEY_DROPPED;
    }
#pragma unroll
    for (int t = 0; t < KI; t++) {
        const int64_t i = i0 + threadIdx.x + PAIRS_TB * t;
        const unsigned long long k = my_item[t];
        bool active = k != KEY_DROPPED;
        if (active) n_item++;
        if (MODE == 2) continue;
        const uint32_t q = (uint32_t)(k >> 32), v = (uint32_t)(k >> 4) & 0x0FFFFFFFu, cls = (uint32_t)(k >> 2) & 3u, ln = (uint32_t)k & 1u;
        for (int d = 1; __any(active); d++) {
            unsigned long long k2;
            if (d < 64) {
                const int src = lane + d;
                const unsigned long long a_ = __shfl(k, src & 63), b_ = __shfl(nx_item[t], src & 63);
                k2 = src < 64 ? a_ : b_;
            } else k2 = (active && i + d < m) ? items[i + d] : KEY_DROPPED;      // a group of more than 64 distinct items
            bool ev = active;                                  // this lane pairs its item with k2 in this round
            if (ev && (k2 == KEY_DROPPED || (uint32_t)(k2 >> 32) != q)) { active = false; ev = false; }        // the distinct items of a group sit at its front
            const uint32_t v2 = (uint32_t)(k2 >> 4) & 0x0FFFFFFFu;
            if (v2 == v) ev = false;
            bool claimed = false;
            int gs = -1;
            uint64_t ck = 0;
            if (ev) {
                n_event++;
                const uint32_t cls2 = (uint32_t)(k2 >> 2) & 3u, ln2 = (uint32_t)k2 & 1u;
                const uint64_t pk = ((uint64_t)v << 32) | v2;          // v < v2 because the group is sorted
                const int cell = (int)(cls * 3 + cls2);
                const int linked = (int)(ln & ln2);
                uint32_t s = hash64(pk) & (PH_SLOTS - 1);
                bool done = false;
                for (int pr = 0; pr < PH_PROBES; pr++) {
                    const unsigned long long prev = atomicCAS(&s_keys[s], (unsigned long long)KEY_DROPPED, (unsigned long long)pk);
                    if (prev == KEY_DROPPED || prev == pk) {
                        atomicAdd(&s_vals[s * PH_WORDS + (cell >> 1)], 1u << ((cell & 1) * 16));
                        if (linked) atomicOr(&s_vals[s * PH_WORDS + 4], 0x10000u);
                        done = true;
                        break;
                    }
                    s = (s + 1) & (PH_SLOTS - 1);
                }
                // the LDS table is full (a tile whose QNAMEs pair up variants all over the chromosome: QNAME ids shared by unrelated reads of
                // several BAMs): straight to the global table
                if (!done) {
                    ck = pk;
                    gs = global_slot(tab, gmask, pk, counters, &claimed);
                    if (gs >= 0) {
                        atomicAdd(&tab[(size_t)gs * GE_WORDS + GE_CELL0 + cell], 1u);
                        if (linked) atomicOr(&tab[(size_t)gs * GE_WORDS + GE_LINKED], 1u);
                    }
                }
            }
            // the lanes that claimed a slot there take their places in the used-slot list with ONE cursor step per wave and round (one
            // same-address atomic per claim was 48 ms for such a sample); every lane of the wave gets here
            const unsigned long long cm = __ballot(claimed ? 1 : 0);
            if (cm) {
                const int leader = __builtin_ctzll(cm);
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(&counters[7], (unsigned long long)__popcll(cm));
                base = __shfl(base, leader);
                if (claimed) {
                    const unsigned long long at = base + (unsigned long long)__popcll(cm & ((1ull << lane) - 1ull));
                    used[at] = (uint32_t)gs; used_key[at] = ck;
                    atomicAdd(&deg[(uint32_t)(ck >> 32)], 1u);
                }
            }
        }
    }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { n_event += __shfl_xor(n_event, d); n_item += __shfl_xor(n_item, d); }
    if ((threadIdx.x & 63) == 0) { s_part[threadIdx.x >> 6] = n_event; s_ipart[threadIdx.x >> 6] = n_item; }
    __syncthreads();
    if (MODE != 0) { if (n_item == 12345678u) used[0] = s_vals[threadIdx.x]; return; }
    {
        constexpr int KS = PH_SLOTS / PAIRS_TB;
        uint64_t pk[KS]; uint32_t hs[KS]; unsigned long long prev[KS];
#pragma unroll
        for (int t = 0; t < KS; t++) {                       // the first probe of each of the lane's slots requested together
            pk[t] = s_keys[threadIdx.x + PAIRS_TB * t];
            hs[t] = pair_home(pk[t], gmask); prev[t] = 0ull;
            if (pk[t] != KEY_DROPPED) prev[t] = atomicCAS((unsigned long long *)(tab + (size_t)hs[t] * GE_WORDS), 0ull, (unsigned long long)pk[t]);
        }
#pragma unroll
        for (int t = 0; t < KS; t++) {
            if (pk[t] == KEY_DROPPED) continue;
            const int j = threadIdx.x + PAIRS_TB * t;
            bool claimed = prev[t] == 0ull;
            int gs = (int)hs[t];
            if (!claimed && prev[t] != pk[t]) gs = global_slot(tab, gmask, pk[t], counters, &claimed);      // taken by another pair: probe on
            if (gs < 0) continue;
            if (claimed) { const uint32_t at = atomicAdd(&s_nclaim, 1u); s_claim[at] = (uint32_t)gs; s_claim_l[at] = (uint16_t)j; }
            uint32_t *e = tab + (size_t)gs * GE_WORDS;
#pragma unroll
            for (int c = 0; c < 9; c++) {
                const uint32_t val = (s_vals[j * PH_WORDS + (c >> 1)] >> ((c & 1) * 16)) & 0xFFFFu;
                if (val) atomicAdd(&e[GE_CELL0 + c], val);
            }
            if (s_vals[j * PH_WORDS + 4] & 0x10000u) atomicOr(&e[GE_LINKED], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = 0, ni = 0;
        for (int w = 0; w < PAIRS_TB / 64; w++) { b += s_part[w]; ni += s_ipart[w]; }
        unsigned long long *spread = counters + 16 + (blockIdx.x % N_SPREAD) * SPREAD_WORDS;
        if (b) atomicAdd(&spread[1], b);
        if (ni) atomicAdd(&spread[0], ni);                    // distinct (QNAME, variant, class) items
        s_ubase = s_nclaim ? atomicAdd(&counters[7], (unsigned long long)s_nclaim) : 0ull;      // one global atomic per workgroup
    }
    __syncthreads();
    // the claimed slots go to the used-slot list together with their keys, and every claim counts as one edge of its first variant: the
    // counting sort of the edges by variant starts from finished degrees and never has to look a key up in the table
    for (unsigned j = threadIdx.x; j < s_nclaim; j += PAIRS_TB) {
        const unsigned long long key = s_keys[s_claim_l[j]];
        used[s_ubase + j] = s_claim[j]; used_key[s_ubase + j] = key;
        atomicAdd(&deg[(uint32_t)(key >> 32)], 1u);
    }
}

// ---- edge list in (a, b) order: counting sort of the used table slots by a (the degrees were counted by k_pairs as it claimed the slots);
//      the position of an edge inside its variant's (small) group is the number of group members with a smaller b
constexpr uint32_t EDGE_RANK_MAX = 128;     // groups up to this size are ranked by counting (<= 128 cached loads per edge); larger ones are sorted first
__global__ __launch_bounds__(256) void k_edge_scatter(const uint32_t *used, const uint64_t *used_key, int64_t n_used, const uint32_t *eoff, uint32_t *deg,
                                                      uint32_t *e_a, uint32_t *e_b, uint32_t *e_slot) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_used) return;
    const uint64_t k = used_key[i];
    const uint32_t a = (uint32_t)(k >> 32);
    const uint32_t old = atomicSub(&deg[a], 1u);               // the counters go back to zero
    const uint32_t p = eoff[a] + old - 1;
    e_a[p] = a; e_b[p] = (uint32_t)k; e_slot[p] = used[i];
}
// one thread per variant with more than EDGE_RANK_MAX edges (QNAME ids shared by unrelated reads pair a variant with thousands of others):
// heap sort of its group in place, the keys are distinct
__global__ __launch_bounds__(256) void k_edge_sort_big(int64_t nv, const uint32_t *eoff, uint32_t *e_b, uint32_t *e_slot) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= nv) return;
    const uint32_t lo = eoff[a], hi = eoff[a + 1], d = hi - lo;
    if (d <= EDGE_RANK_MAX) return;
    uint32_t *kb = e_b + lo, *ks = e_slot + lo;
    auto sift = [&](uint32_t root, uint32_t n) {
        const uint32_t xb = kb[root], xs = ks[root];
        for (;;) {
            uint32_t c = 2 * root + 1;
            if (c >= n) break;
            if (c + 1 < n && kb[c + 1] > kb[c]) c++;
            if (kb[c] <= xb) break;
            kb[root] = kb[c]; ks[root] = ks[c]; root = c;
        }
        kb[root] = xb; ks[root] = xs;
    };
    for (uint32_t i = d / 2; i-- > 0;) sift(i, d);
    for (uint32_t n = d - 1; n > 0; n--) {
        const uint32_t tb = kb[0], ts = ks[0];
        kb[0] = kb[n]; ks[0] = ks[n]; kb[n] = tb; ks[n] = ts;
        sift(0, n);
    }
}
// one thread per edge: its place in the (a, b)-ordered list, its table entry (one sector) read, the result columns written, the entry returned
// to "empty" -- the table is left clean slot by slot, so the next call needs no memset of it
__global__ __launch_bounds__(256) void k_edge_out(int64_t ne, const uint32_t *eoff, const uint32_t *e_a, const uint32_t *e_b, const uint32_t *e_slot, uint32_t *tab,
                                                  int32_t *ea, int32_t *eb, int32_t *cells, uint8_t *linked, int32_t *cto, int32_t *stats) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= ne) return;
    uint4 *e = (uint4 *)(tab + (size_t)e_slot[p] * GE_WORDS);
    const uint4 w0 = e[0], w1 = e[1], w2 = e[2];                      // requested before the group is looked at
    const uint32_t a = e_a[p], b = e_b[p];
    const uint32_t lo = eoff[a], hi = eoff[a + 1];
    uint32_t rank = (uint32_t)p - lo;                                 // a sorted group
    if (hi - lo <= EDGE_RANK_MAX) {
        rank = 0;
        for (uint32_t j = lo; j < hi; j++) rank += e_b[j] < b ? 1u : 0u;
    }
    const int64_t i = (int64_t)lo + rank;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    e[0] = z; e[1] = z; e[2] = z;
    ea[i] = (int32_t)a; eb[i] = (int32_t)b;
    const int32_t x[9] = {(int32_t)w0.z, (int32_t)w0.w, (int32_t)w1.x, (int32_t)w1.y, (int32_t)w1.z, (int32_t)w1.w, (int32_t)w2.x, (int32_t)w2.y, (int32_t)w2.z};
#pragma unroll
    for (int c = 0; c < 9; c++) cells[i * 9 + c] = x[c];
    linked[i] = (uint8_t)(w2.w & 1u);
    // test_variant_connection's three sums (phaser.py:1634-1636): same configuration rr+aa, opposite ar+ra, the five "other" cells
    const int32_t cis = x[0] + x[4], trans = x[3] + x[1], oth = x[6] + x[7] + x[2] + x[5] + x[8];
    cto[i * 3] = cis; cto[i * 3 + 1] = trans; cto[i * 3 + 2] = oth;
    // the derived columns of the pair test (:1637-1649), one plane each: same-configuration / opposite counts, supporting =
    // the larger of the two, total, chosen configuration (0 same, 1 opposite, -1 tie)
    stats[i] = cis; stats[ne + i] = trans; stats[2 * ne + i] = cis > trans ? cis : trans; stats[3 * ne + i] = cis + trans + oth;
    stats[4 * ne + i] = cis > trans ? 0 : (cis < trans ? 1 : -1);
}

// ---- read lists with a far line (dirty lists): their entries were placed through a cursor, in arrival order; one workgroup per list puts them
//      into line order (bitonic sort in LDS) and keeps the QNAME ids; a list beyond the LDS stage goes to the host-driven radix sort.
//      counters32[1] = lists left to that sort.  The list's cursor returns to zero (it is persistent, like the per-QNAME one).
constexpr int RL_LDS = 4096;
__global__ __launch_bounds__(256) void k_rl_sort_dirty(const uint32_t *dirty_list, const uint32_t *rl_start, const uint64_t *rl_tmp, int32_t *rl_qid, uint32_t *rl_cursor,
                                                       uint32_t *big_list, uint32_t *counters32) {
    __shared__ unsigned long long s_x[RL_LDS];
    const uint32_t e = dirty_list[blockIdx.x];
    const uint32_t lo = rl_start[e], n = rl_start[e + 1] - lo;
    if (threadIdx.x == 0) rl_cursor[e] = 0u;
    if (n > (uint32_t)RL_LDS) { if (threadIdx.x == 0) big_list[atomicAdd(&counters32[1], 1u)] = e; return; }
    uint32_t m = 64;
    while (m < n) m <<= 1;
    for (uint32_t t = threadIdx.x; t < m; t += 256) s_x[t] = t < n ? rl_tmp[lo + t] : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < m; t += 256) {
                const uint32_t p = t ^ j;
                if (p > t) {
                    const unsigned long long a = s_x[t], b = s_x[p];
                    const bool up = (t & k) == 0;
                    if ((a > b) == up) { s_x[t] = b; s_x[p] = a; }
                }
            }
            __syncthreads();
        }
    for (uint32_t t = threadIdx.x; t < n; t += 256) rl_qid[lo + t] = (int32_t)(uint32_t)s_x[t];
}
__global__ __launch_bounds__(256) void k_rl_take_qid(const uint64_t *src, int64_t n, int32_t *dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (int32_t)(uint32_t)src[i];
}

// sequencing-noise counters (phaser.py:610-632): over the variants with ref+alt lines and an "other" share below 5 %, the ref+alt
// lines (match) and the other-allele lines (mismatch); the caller all-reduces them over chromosomes / ranks
__global__ __launch_bounds__(256) void k_noise(const int32_t *var_count, int64_t nv, unsigned long long *out /* [0] match, [1] mismatch */) {
    __shared__ unsigned long long s_m[4], s_x[4];
    unsigned long long m = 0, x = 0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (int64_t)gridDim.x * 256) {       // few workgroups: two same-address atomics each
        const long long mm = (long long)var_count[v * 3] + var_count[v * 3 + 1], oo = var_count[v * 3 + 2];
        if (mm > 0 && (double)oo / (double)(oo + mm) < 0.05) { m += (unsigned long long)mm; x += (unsigned long long)oo; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { m += __shfl_xor(m, d); x += __shfl_xor(x, d); }
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_x[threadIdx.x >> 6] = x; }
    __syncthreads();
    if (threadIdx.x == 0) {
        m = s_m[0] + s_m[1] + s_m[2] + s_m[3]; x = s_x[0] + s_x[1] + s_x[2] + s_x[3];
        if (m) atomicAdd(&out[0], m);
        if (x) atomicAdd(&out[1], x);
    }
}

constexpr size_t CNT_BYTES = 128 + (size_t)N_SPREAD * SPREAD_WORDS * 8;

// HIP-event timing of a stage on the ctx stream; stop() waits for the stage and reports HIP errors
struct Timer {
    phz_ctx *c; int slot; hipError_t err;
    Timer(phz_ctx *ctx, int s) : c(ctx), slot(s) { err = hipEventRecord(c->ev0, c->stream); }
    int stop() {
        hipError_t e = hipEventRecord(c->ev1, c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(c->ev1);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
        if (err != hipSuccess) e = err;
        if (e != hipSuccess) return phz_fail(c, PHZ_E_HIP, "stage timing / kernel execution", e);
        c->last_ms[slot] = ms; c->total_ms[slot] += ms; c->launches[slot]++;
        return PHZ_OK;
    }
};

int stage_lines(Staging &st, const phz_lines &h, int space, LinesDev *d) {
    d->n = h.n_calls; d->cutoff = h.as_cutoff; d->use_cutoff = h.use_cutoff; d->bam = h.bam_index; d->cut_dev = h.as_cutoff_dev;
    d->var_base = (int32_t)h.var_base; d->qid_base = (uint32_t)h.qid_base; d->line_base = 0;
    if (int s = st.in(h.read_idx, (size_t)h.n_calls, space, &d->read_idx)) return s;
    if (int s = st.in(h.var_idx, (size_t)h.n_calls, space, &d->var_idx)) return s;
    if (int s = st.in(h.code, (size_t)h.n_calls, space, &d->code)) return s;
    if (int s = st.in(h.read_qid, (size_t)h.n_reads, space, &d->read_qid)) return s;
    if (int s = st.in(h.read_as, (size_t)h.n_reads, space, &d->read_as)) return s;
    if (int s = st.in(h.read_has_as, (size_t)h.n_reads, space, &d->read_has_as)) return s;
    if (int s = st.in(h.read_as16, (size_t)h.n_reads, space, &d->read_as16)) return s;
    d->nv_chrom = 0;
    return PHZ_OK;
}

// results and the read-list buffers live in their own buffers (ctx->tally_buf); per-call scratch: the SC_T_* slots of PhzScratch
enum { R_CNT = 0, R_FIRST, R_DIST, R_RANK, R_CLS, R_EA, R_EB, R_CELLS, R_LINKED, R_CTO, R_STATS, R_RLCNT, R_RLSTART, R_RLFILL, R_RLTMP, R_RLLIST, R_RLQID, R_A0, R_A1,
       R_LINEQ, R_SORTK, R_SORTV0, R_SORTV1, R_SORTCNT, R_SPQ, R_SPITEM, R_TILEWB, R_TILEM, R_TILEB, R_QSEEN, R_QDUP, R_RLDIRTY, R_COUNT };

}  // namespace

// k_as_hist is grid-stride with one LDS histogram per block, flushed with global atomics at the end: few, long-running blocks
static unsigned as_hist_blocks(const LinesDev &l) { const unsigned g = nblk((l.n + 15) / 16); return g > 512u ? 512u : (g ? g : 1u); }

// Device image of a shard table for one batched stage: [LinesDev x n][blk0 x (n+1)], blocks per shard from `blocks_of`.  Every
// table of a call gets its own slice of ctx->shard_tab (`slot`), so stages with different block sizes can be in flight together.
template <class F>
static int upload_tab(phz_ctx *ctx, const LinesDev *L, int n, F blocks_of, LinesTab *out, std::vector<uint32_t> *blk0_host, int slot = 0,
                      int n_slots = 1) {
    const size_t one = ((size_t)n * sizeof(LinesDev) + (size_t)(n + 1) * 4 + 63) & ~(size_t)63;
    if (ctx->tab_pending) { PHZ_HIP(ctx, hipEventSynchronize(ctx->tab_ev)); ctx->tab_pending = false; }      // the previous table has left the pinned image
    if (int s = phz_reserve_host(ctx, ctx->h_shard_tab, one * (size_t)n_slots)) return s;
    if (int s = phz_reserve(ctx, ctx->shard_tab, one * (size_t)n_slots)) return s;
    char *h = (char *)ctx->h_shard_tab.p + one * (size_t)slot;
    char *d = (char *)ctx->shard_tab.p + one * (size_t)slot;
    memcpy(h, L, (size_t)n * sizeof(LinesDev));
    uint32_t *b0 = (uint32_t *)(h + (size_t)n * sizeof(LinesDev));
    blk0_host->assign((size_t)n + 1, 0u);
    uint64_t acc = 0;
    for (int i = 0; i < n; i++) {
        b0[i] = (uint32_t)acc; (*blk0_host)[(size_t)i] = (uint32_t)acc;
        acc += L[i].n > 0 ? (uint64_t)blocks_of(L[i]) : 0u;
        if (acc >= (1ull << 31)) return phz_fail(ctx, PHZ_E_ARG, "too many blocks in one batched stage");
    }
    b0[n] = (uint32_t)acc; (*blk0_host)[(size_t)n] = (uint32_t)acc;
    PHZ_HIP(ctx, hipMemcpyAsync(d, h, one, hipMemcpyHostToDevice, ctx->stream));
    if (!ctx->tab_ev) PHZ_HIP(ctx, hipEventCreateWithFlags(&ctx->tab_ev, hipEventDisableTiming));
    PHZ_HIP(ctx, hipEventRecord(ctx->tab_ev, ctx->stream)); ctx->tab_pending = true;
    out->L = (const LinesDev *)d; out->blk0 = (const uint32_t *)(d + (size_t)n * sizeof(LinesDev)); out->n = n;
    return PHZ_OK;
}

// What every AS-histogram entry point enqueues: the shards staged, their table for k_as_hist's grid uploaded, the kernel (none when no shard has a line).
// hist / oor_flag are device pointers: where the histogram and the "AS value outside int16" flag live is the caller's business.
static int enqueue_as_hist(phz_ctx *ctx, Staging &st, const phz_lines *shards, int n_shards, int space, unsigned long long *hist, unsigned int *oor_flag) {
    if (n_shards <= 0) return PHZ_OK;
    std::vector<LinesDev> L((size_t)n_shards);
    for (int i = 0; i < n_shards; i++)
        if (int s = stage_lines(st, shards[i], space, &L[(size_t)i])) return s;
    LinesTab T; std::vector<uint32_t> grids;
    if (int s = upload_tab(ctx, L.data(), n_shards, as_hist_blocks, &T, &grids)) return s;
    if (grids.back() > 0) hipLaunchKernelGGL(k_as_hist, dim3(grids.back()), dim3(256), 0, ctx->stream, T, hist, oor_flag);
    return PHZ_OK;
}

extern "C" int phz_as_histogram(phz_ctx *ctx, const phz_lines *shard, int64_t *hist, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !shard || !hist) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    unsigned long long *dh = nullptr;
    if (space == PHZ_DEVICE) dh = (unsigned long long *)hist;
    else {
        if (int s = phz_reserve(ctx, ctx->scratch[SC_AS_HIST], PHZ_AS_BINS * 8)) return s;
        dh = (unsigned long long *)ctx->scratch[SC_AS_HIST].p;
        PHZ_HIP(ctx, hipMemcpyAsync(dh, hist, PHZ_AS_BINS * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    Timer t(ctx, PHZ_T_ASHIST);
    if (int s = enqueue_as_hist(ctx, st, shard, 1, space, dh, nullptr)) return s;
    PHZ_HIP(ctx, hipGetLastError());
    if (int s = t.stop()) return s;
    if (space == PHZ_HOST) PHZ_HIP(ctx, hipMemcpyAsync(hist, dh, PHZ_AS_BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
    PHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PHZ_OK;
}

// AS histograms of several device-resident shards accumulated into one device histogram, one host wait
extern "C" int phz_as_histogram_batch(phz_ctx *ctx, const phz_lines *shards, int n_shards, int64_t *hist) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || (!shards && n_shards) || !hist || n_shards < 0) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Timer t(ctx, PHZ_T_ASHIST);
    Staging st(ctx);
    DevBuf &flag = ctx->scratch[SC_AS_HIST];          // (the histogram is the caller's: only the out-of-range flag lives here)
    if (n_shards > 0) {
        if (int s2 = phz_reserve(ctx, flag, 64)) return s2;
        PHZ_HIP(ctx, hipMemsetAsync(flag.p, 0, 4, ctx->stream));
    }
    if (int s = enqueue_as_hist(ctx, st, shards, n_shards, PHZ_DEVICE, (unsigned long long *)hist, (unsigned int *)flag.p)) return s;
    PHZ_HIP(ctx, hipGetLastError());
    unsigned int oor = 0;
    if (n_shards > 0) PHZ_HIP(ctx, hipMemcpyAsync(&oor, flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (int s = t.stop()) return s;
    if (oor) return phz_fail(ctx, PHZ_E_UNSUPPORTED, "AS value outside int16");
    return PHZ_OK;
}

// ... and for one rank that needs no all-reduce: the histogram never leaves the device, the host gets its occupied bins
extern "C" int phz_as_histogram_sparse(phz_ctx *ctx, const phz_lines *shards, int n_shards, int cap, int32_t *bins, int64_t *counts, int32_t *n_bins) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || (!shards && n_shards) || n_shards < 0 || cap < 1 || cap > 4096 || !bins || !counts || !n_bins) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Timer t(ctx, PHZ_T_ASHIST);
    Staging st(ctx);
    // SC_AS_HIST: [hist 64 Ki x 8][out-of-range flag, pair count][bins cap x 4][counts cap x 8]; the host image of the tail in h_scalars
    const size_t tail = 16 + (size_t)cap * 12;
    if (int s2 = phz_reserve(ctx, ctx->scratch[SC_AS_HIST], PHZ_AS_BINS * 8 + tail)) return s2;
    if (int s2 = phz_reserve_host(ctx, ctx->h_scalars, tail)) return s2;
    char *d = (char *)ctx->scratch[SC_AS_HIST].p;
    unsigned long long *hist = (unsigned long long *)d;
    unsigned int *flags = (unsigned int *)(d + PHZ_AS_BINS * 8);
    int32_t *d_bins = (int32_t *)(d + PHZ_AS_BINS * 8 + 16);
    unsigned long long *d_counts = (unsigned long long *)(d + PHZ_AS_BINS * 8 + 16 + (size_t)cap * 4);
    PHZ_HIP(ctx, hipMemsetAsync(d, 0, PHZ_AS_BINS * 8 + 16, ctx->stream));
    if (int s = enqueue_as_hist(ctx, st, shards, n_shards, PHZ_DEVICE, hist, flags)) return s;
    hipLaunchKernelGGL(k_hist_compact, dim3(PHZ_AS_BINS / 1024), dim3(1024), 0, ctx->stream, (const unsigned long long *)hist, cap, d_bins, d_counts, (int32_t *)(flags + 1));
    PHZ_HIP(ctx, hipGetLastError());
    PHZ_HIP(ctx, hipMemcpyAsync(ctx->h_scalars.p, flags, tail, hipMemcpyDeviceToHost, ctx->stream));
    if (int s = t.stop()) return s;
    const unsigned int *hf = (const unsigned int *)ctx->h_scalars.p;
    if (hf[0]) return phz_fail(ctx, PHZ_E_UNSUPPORTED, "AS value outside int16");
    *n_bins = (int32_t)hf[1];
    if ((int)hf[1] > cap) return PHZ_E_CAPACITY;
    {   // the pairs arrive workgroup by workgroup in no particular order: into bin order (a few dozen of them)
        const int32_t *hb = (const int32_t *)((const char *)ctx->h_scalars.p + 16);
        const int64_t *hc = (const int64_t *)((const char *)ctx->h_scalars.p + 16 + (size_t)cap * 4);
        std::vector<int> order(hf[1]);
        for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return hb[a] < hb[b]; });
        for (size_t i = 0; i < order.size(); i++) { bins[i] = hb[order[i]]; counts[i] = hc[order[i]]; }
    }
    return PHZ_OK;
}

// the AS column of a shard as the 2-byte plane (phz_lines.read_as16): what a producer that only has the 4-byte column + flag calls once per shard
__global__ __launch_bounds__(256) void k_as16(const int32_t *aln, const uint8_t *has, int64_t n, int16_t *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int a = aln[i];
    out[i] = (has && !has[i]) ? (int16_t)PHZ_AS16_NONE : (int16_t)(a >= PHZ_AS16_RANGE ? PHZ_AS16_RANGE : (a <= -PHZ_AS16_RANGE ? -PHZ_AS16_RANGE : a));
}
extern "C" int phz_as_plane(phz_ctx *ctx, const int32_t *aln, const uint8_t *has_as, int64_t n, int16_t *out) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n < 0 || (n && (!aln || !out))) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    if (n) hipLaunchKernelGGL(k_as16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, aln, has_as, n, out);
    PHZ_HIP(ctx, hipGetLastError());
    return PHZ_OK;          // (no wait: the consumers -- phz_as_cutoff, phz_tally -- run on the same stream)
}

// numpy.percentile(scores, q) (the default "linear" method: numpy/lib/_function_base_impl.py _quantile / _lerp; the reference's call at
// phaser.py:551) over the multiset {bin - 32768 repeated count times}, from the occupied bins in ascending order: the same float64 operations on the
// two neighbouring order statistics (engine.percentile_from_band is the Python twin, pinned against numpy in the tests)
static double percentile_of_bins(const int32_t *bins, const int64_t *counts, int nb, double q) {
    int64_t n = 0;
    for (int i = 0; i < nb; i++) n += counts[i];
    const double quant = q / 100.0;
    const double virt = (double)(n - 1) * quant;
    int64_t prev = (int64_t)floor(virt);
    const double gamma = virt - (double)prev;
    int64_t nxt = prev + 1;
    if (virt >= (double)(n - 1)) prev = nxt = n - 1;
    if (virt < 0) prev = nxt = 0;
    auto value_at = [&](int64_t k) {                 // k-th smallest score (0-based)
        int64_t c = 0;
        for (int i = 0; i < nb; i++) { c += counts[i]; if (c > k) return (int64_t)bins[i] - 32768; }
        return (int64_t)bins[nb - 1] - 32768;
    };
    const int64_t a = value_at(prev), b = value_at(nxt), diff = b - a;
    double out = (double)a + (double)diff * gamma;
    if (gamma >= 0.5) out = (double)b - (double)diff * (1 - gamma);
    return out;
}

// AS histogram of the shards of one BAM + the percentile, in one call and one host wait: *found = 0 when no record carries an alignment score
extern "C" int phz_as_cutoff(phz_ctx *ctx, const phz_lines *shards, int n_shards, double q_percent, double *cutoff, int32_t *found) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !cutoff || !found) return PHZ_E_ARG;
    constexpr int CAP = 4096;
    std::vector<int32_t> bins(CAP); std::vector<int64_t> counts(CAP);
    int32_t nb = 0;
    if (int s = phz_as_histogram_sparse(ctx, shards, n_shards, CAP, bins.data(), counts.data(), &nb)) return s;
    int64_t n = 0;
    for (int i = 0; i < nb; i++) n += counts[i];
    *found = n > 0 ? 1 : 0; *cutoff = 0.0;
    if (n > 0) *cutoff = percentile_of_bins(bins.data(), counts.data(), nb, q_percent);
    return PHZ_OK;
}

// numpy.percentile on the device: one workgroup over the 64 Ki-bin histogram (bin b = AS b - 32768).  Thread t adds up bins [64 t, 64 t + 64), the partial sums are
// scanned by the waves, the two order statistics the linear method interpolates between are found by the threads whose ranges hold them; thread 0 then performs
// percentile_of_bins' float64 operations one by one (contraction off: an fma would round once where numpy rounds twice).
__global__ __launch_bounds__(1024) void k_as_percentile(const unsigned long long *hist, const unsigned int *flags, double quant, double *out) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_incl[1024];
    __shared__ unsigned long long s_wsum[16];
    __shared__ long long s_val[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long mine = 0;
    for (int b = 0; b < 64; b++) mine += hist[tid * 64 + b];
    unsigned long long incl = gs_wave_incl(mine, lane);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    unsigned long long before = 0;
    for (int w = 0; w < wave; w++) before += s_wsum[w];
    incl += before;
    s_incl[tid] = incl;
    __syncthreads();
    const long long n = (long long)s_incl[1023];
    if (n <= 0) { if (tid == 0) { out[0] = 0.0; out[1] = 0.0; out[2] = flags[0] ? 1.0 : 0.0; out[3] = 0.0; } return; }
    const double virt = (double)(n - 1) * quant;
    long long prev = (long long)floor(virt);
    const double gamma = virt - (double)prev;
    long long nxt = prev + 1;
    if (virt >= (double)(n - 1)) prev = nxt = n - 1;
    if (virt < 0) prev = nxt = 0;
    const unsigned long long excl = incl - mine;
    for (int which = 0; which < 2; which++) {
        const unsigned long long k = (unsigned long long)(which ? nxt : prev);
        if (k >= excl && k < incl) {          // the k-th smallest score lies in this thread's bins
            unsigned long long c = excl;
            for (int b = 0; b < 64; b++) { c += hist[tid * 64 + b]; if (c > k) { s_val[which] = (long long)(tid * 64 + b) - 32768; break; } }
        }
    }
    __syncthreads();
    if (tid == 0) {
        const long long a = s_val[0], b = s_val[1], diff = b - a;
        double r = (double)a + (double)diff * gamma;
        if (gamma >= 0.5) r = (double)b - (double)diff * (1 - gamma);
        out[0] = r; out[1] = 1.0; out[2] = flags[0] ? 1.0 : 0.0; out[3] = (double)n;
    }
}

extern "C" int phz_as_cutoff_enqueue(phz_ctx *ctx, const phz_lines *shards, int n_shards, double q_percent, double *dev_out) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || (!shards && n_shards) || n_shards < 0 || !dev_out) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    if (int s2 = phz_reserve(ctx, ctx->scratch[SC_AS_HIST], PHZ_AS_BINS * 8 + 16)) return s2;
    char *d = (char *)ctx->scratch[SC_AS_HIST].p;
    unsigned long long *hist = (unsigned long long *)d;
    unsigned int *flags = (unsigned int *)(d + PHZ_AS_BINS * 8);
    PHZ_HIP(ctx, hipMemsetAsync(d, 0, PHZ_AS_BINS * 8 + 16, ctx->stream));
    if (int s = enqueue_as_hist(ctx, st, shards, n_shards, PHZ_DEVICE, hist, flags)) return s;
    static_assert(PHZ_AS_BINS == 65536, "k_as_percentile: 1024 threads x 64 bins");
    hipLaunchKernelGGL(k_as_percentile, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long *)hist, (const unsigned int *)flags, q_percent / 100.0, dev_out);
    PHZ_HIP(ctx, hipGetLastError());
    return PHZ_OK;
}

namespace {
// What one phz_tally call knows.  Its stage functions are the sections of the pass in stream order, each named after what it enqueues; a host wait is the last thing
// of the section that has one (WAIT in its comment), and what is read back there stays here for the sections after it.
struct TallyPass {
    phz_ctx *ctx; hipStream_t sm; DevBuf *R, *S; Staging st;
    const int64_t nv, n_qid; const int n_shards, n_bams; int64_t total = 0;          // (total: call lines of all shards)
    size_t NV, NQ, TOT = 1, NRL, QWORDS, RLWORDS, NT = 1; std::vector<LinesDev> L;
    // tiles of the per-line stages (k_line and k_tile: TL lines each) and variant blocks of k_colscan (TWT variants each), over the shard table
    LinesTab TT, TC; unsigned grid_t = 0, grid_c = 0;
    const uint8_t *d_a0 = nullptr, *d_a1 = nullptr;
    // typed views of the buffers (reserve_and_clear; tab / used / usedkey: pair_table, which sizes them)
    int32_t *d_cnt, *d_dist, *rl_qid, *tile_wb; unsigned long long *d_first, *d_rank, *counters, *prof = nullptr; uint8_t *d_cls; uint16_t *tile_m;
    uint32_t *line_q, *rl_cnt, *rl_start, *rl_fill, *rl_list, *qcount, *touched, *cnt_t, *base_t, *counters32, *deg, *eoff, *dirty_list, *big_list, *tile_b, *q_seen, *q_dup, *rl_dirty, *sp_q;
    uint64_t *rl_tmp, *items, *sp_item;
    uint32_t *tab = nullptr, *used = nullptr; uint64_t *usedkey = nullptr; uint64_t cap = 0;
    const bool profiling = getenv("PHZ_TALLY_PROFILE") != nullptr;
    // the counter block (see k_pairs) as last read back: at "lines and tiles", then once per attempt of "pair table"
    std::vector<unsigned long long> h_counters = std::vector<unsigned long long>(CNT_BYTES / 8, 0ull);
    int64_t n_kept = 0, n_dirty = 0;          // read at "lines and tiles"
    int64_t n_complete = 0, nt = 0, n_spill = 0;          // item slots of the tiles; QNAMEs whose lines straddle tiles (one group each, built from the spilled lines); spilled lines
    int64_t ne = 0; uint32_t n_big = 0, n_rl = 0;          // read at "pair table": edges, dirty read lists beyond the LDS stage, read-list entries

    TallyPass(phz_ctx *c, int64_t nv_, int64_t n_qid_, int n_shards_, int n_bams_)
        : ctx(c), sm(c->stream), S(c->scratch), st(c), nv(nv_), n_qid(n_qid_), n_shards(n_shards_), n_bams(n_bams_), NV((size_t)(nv_ ? nv_ : 1)), NQ((size_t)(n_qid_ ? n_qid_ : 1)),
          NRL(NV * 2 * (size_t)n_bams_), QWORDS((NQ + 31) / 32 + (size_t)QW / 32), RLWORDS((NRL + 31) / 32), L((size_t)n_shards_) {      // (QWORDS: + the LDS window of k_line, which may reach past the last id)
        if (c->tally_buf.size() < (size_t)R_COUNT) c->tally_buf.resize(R_COUNT);
        R = c->tally_buf.data();
        TT.L = nullptr; TT.blk0 = nullptr; TT.n = 0; TC = TT;
    }
    template <class T> T *res(int slot) const { return (T *)R[slot].p; }
    template <class T> T *scr(int slot) const { return (T *)S[slot].p; }
    unsigned long long spread_sum(int k) const { unsigned long long t = 0; for (int c = 0; c < N_SPREAD; c++) t += h_counters[16 + c * SPREAD_WORDS + k]; return t; }

    // ---- the limits of the key spaces, the shards' arrays and the two allele columns staged, the shard tables of the line tiles and the variant blocks uploaded
    int check_and_stage(const phz_lines *shards, const uint8_t *a0, const uint8_t *a1, int space) {
        if (nv >= (1ll << 28)) return phz_fail(ctx, PHZ_E_ARG, "more than 2^28 variants in one call");
        if (n_qid >= (1ll << 31)) return phz_fail(ctx, PHZ_E_ARG, "more than 2^31 QNAME ids in one call");
        if (2 * nv * n_bams >= (1ll << 31)) return phz_fail(ctx, PHZ_E_ARG, "variants x BAMs exceeds the read-list key space");
        PHZ_HIP(ctx, hipSetDevice(ctx->device));
        for (int b = 0; b < n_shards; b++) {
            if (shards[b].bam_index < 0 || shards[b].bam_index >= n_bams) return phz_fail(ctx, PHZ_E_ARG, "bam_index outside [0, n_bams)");
            if (shards[b].var_base < 0 || shards[b].qid_base < 0) return phz_fail(ctx, PHZ_E_ARG, "negative base");
            if (int s = stage_lines(st, shards[b], space, &L[b])) return s;
            L[b].line_base = total;
            total += L[b].n;
        }
        if (total >= (1ll << 32) - 16) return phz_fail(ctx, PHZ_E_ARG, "more than 2^32 call lines in one call");
        TOT = (size_t)(total ? total : 1);
        // variants of every shard's chromosome: up to the next chromosome's first variant (shards of a chromosome share var_base)
        for (int b = 0; b < n_shards; b++) {
            int64_t end = nv;
            for (int c = 0; c < n_shards; c++)
                if (L[c].var_base > L[b].var_base && L[c].var_base < end) end = L[c].var_base;
            if (L[b].var_base > nv) return phz_fail(ctx, PHZ_E_ARG, "var_base beyond the variant space");
            L[b].nv_chrom = (int32_t)(end - L[b].var_base);
        }
        if (space == PHZ_DEVICE) { d_a0 = a0; d_a1 = a1; }
        else {
            if (int s = reserve_all(ctx, {{R[R_A0], NV}, {R[R_A1], NV}})) return s;
            if (nv) {
                PHZ_HIP(ctx, hipMemcpyAsync(R[R_A0].p, a0, (size_t)nv, hipMemcpyHostToDevice, sm));
                PHZ_HIP(ctx, hipMemcpyAsync(R[R_A1].p, a1, (size_t)nv, hipMemcpyHostToDevice, sm));
            }
            d_a0 = res<const uint8_t>(R_A0); d_a1 = res<const uint8_t>(R_A1);
        }
        if (n_shards > 0) {
            std::vector<uint32_t> gt, gc;
            if (int s2 = upload_tab(ctx, L.data(), n_shards, [](const LinesDev &l) { return (unsigned)((l.n + TL - 1) / TL); }, &TT, &gt, 0, 2)) return s2;
            if (int s2 = upload_tab(ctx, L.data(), n_shards, [](const LinesDev &l) { return (unsigned)((l.nv_chrom + TWT - 1) / TWT); }, &TC, &gc, 1, 2)) return s2;
            grid_t = gt.back(); grid_c = gc.back();
        }
        NT = grid_t ? grid_t : 1;
        return PHZ_OK;
    }
    // ---- every buffer whose size is known before the pass; the typed views
    int reserve_and_clear() {
        if (int s = reserve_all(ctx, {{R[R_CNT], NV * 12}, {R[R_FIRST], NV * 8}, {R[R_DIST], NV * 12}, {R[R_RANK], NV * 8}, {R[R_CLS], TOT}, {R[R_LINEQ], TOT * 4},
                                      {R[R_RLCNT], NRL * 4}, {R[R_RLSTART], (NRL + 1) * 4}, {R[R_RLTMP], TOT * 8}, {R[R_RLLIST], TOT * 4}, {R[R_RLQID], TOT * 4},
                                      {R[R_SPQ], TOT * 4}, {R[R_SPITEM], TOT * 8},
                                      {R[R_TILEWB], NT * 4}, {R[R_TILEM], NT * (TWT * 3) * 2}, {R[R_TILEB], NT * (TWT * 2) * 4},
                                      {R[R_QSEEN], QWORDS * 4}, {R[R_QDUP], QWORDS * 4}, {R[R_RLDIRTY], RLWORDS * 4},
                                      {S[SC_T_TOUCHED], TOT * 4}, {S[SC_T_CNT_T], (TOT + 1) * 4}, {S[SC_T_BASE_T], (TOT + 1) * 4}, {S[SC_T_ITEMS], (2 * TOT + (size_t)(n_shards + 1) * TL) * 8},
                                      {S[SC_T_COUNTERS], CNT_BYTES}, {S[SC_T_DEG], NV * 4}, {S[SC_T_EOFF], (NV + 1) * 4}, {S[SC_T_MISC], std::max(NRL, (size_t)1) * 8 + 64}})) return s;
        // two arrays are persistent and all zero between calls: the spilled-line counter / fill cursor per QNAME (k_group_plan and k_groups return it to
        // zero) and the fill cursor per read list (k_rl_sort_dirty does).  They are cleared only when (re)allocated -- or after a call that failed half way
        const size_t before = ctx->tally_qcount.cap, before_rl = R[R_RLFILL].cap;
        if (int s = reserve_all(ctx, {{ctx->tally_qcount, NQ * 4}, {R[R_RLFILL], NRL * 4}})) return s;
        if (ctx->tally_qcount.cap != before || ctx->tally_dirty) PHZ_HIP(ctx, hipMemsetAsync(ctx->tally_qcount.p, 0, ctx->tally_qcount.cap, sm));
        if (R[R_RLFILL].cap != before_rl || ctx->tally_dirty) PHZ_HIP(ctx, hipMemsetAsync(R[R_RLFILL].p, 0, R[R_RLFILL].cap, sm));
        d_cnt = res<int32_t>(R_CNT); d_dist = res<int32_t>(R_DIST); d_first = res<unsigned long long>(R_FIRST); d_rank = res<unsigned long long>(R_RANK); d_cls = res<uint8_t>(R_CLS);
        line_q = res<uint32_t>(R_LINEQ); rl_cnt = res<uint32_t>(R_RLCNT); rl_start = res<uint32_t>(R_RLSTART); rl_fill = res<uint32_t>(R_RLFILL); rl_list = res<uint32_t>(R_RLLIST);
        rl_tmp = res<uint64_t>(R_RLTMP); rl_qid = res<int32_t>(R_RLQID); sp_q = res<uint32_t>(R_SPQ); sp_item = res<uint64_t>(R_SPITEM);
        tile_wb = res<int32_t>(R_TILEWB); tile_m = res<uint16_t>(R_TILEM); tile_b = res<uint32_t>(R_TILEB); q_seen = res<uint32_t>(R_QSEEN); q_dup = res<uint32_t>(R_QDUP); rl_dirty = res<uint32_t>(R_RLDIRTY);
        qcount = (uint32_t *)ctx->tally_qcount.p; touched = scr<uint32_t>(SC_T_TOUCHED); cnt_t = scr<uint32_t>(SC_T_CNT_T); base_t = scr<uint32_t>(SC_T_BASE_T); items = scr<uint64_t>(SC_T_ITEMS);
        counters = scr<unsigned long long>(SC_T_COUNTERS); counters32 = (uint32_t *)(counters + 8);          // see k_pairs
        deg = scr<uint32_t>(SC_T_DEG); eoff = scr<uint32_t>(SC_T_EOFF); dirty_list = scr<uint32_t>(SC_T_MISC); big_list = dirty_list + NRL;
        return PHZ_OK;
    }
    // ---- the per-call arrays cleared, then the per-line pass, the column scan, the noise sums, the read-list offsets, the per-tile pass.
    // WAIT 0: the counter block (kept lines, far lines, dirty read lists, spilled lines and their QNAMEs)
    int lines_and_tiles() {
        ctx->tally_dirty = true;           // cleared again when the call completes
        const struct { void *p; int value; size_t bytes; } clear[] = {{d_cnt, 0, NV * 12}, {d_dist, 0, NV * 12}, {rl_cnt, 0, NRL * 4}, {d_rank, 0xff, NV * 8}, {counters, 0, CNT_BYTES},
            {d_first, 0xff, NV * 8} /* unsigned max for atomicMin == -1 as int64 ("none") */, {q_seen, 0, QWORDS * 4}, {q_dup, 0, QWORDS * 4}, {rl_dirty, 0, RLWORDS * 4}};
        for (const auto &c : clear) PHZ_HIP(ctx, hipMemsetAsync(c.p, c.value, c.bytes, sm));
        LineOut O;
        O.a0 = d_a0; O.a1 = d_a1; O.line_cls = d_cls; O.line_q = line_q; O.var_count = d_cnt; O.var_first = d_first; O.rl_cnt = rl_cnt;
        O.tile_wb = tile_wb; O.tile_m = tile_m; O.q_seen = q_seen; O.q_dup = q_dup; O.rl_dirty = rl_dirty; O.dirty_list = dirty_list;
        O.counters = counters; O.nb = n_bams; O.prof = nullptr;
        if (profiling) {          // (start, end) cycle stamps per workgroup: k_line's, then k_tile's
            if (int s = phz_reserve(ctx, S[SC_T_PROFILE], (size_t)(2 * grid_t + 2) * 16)) return s;
            O.prof = prof = scr<unsigned long long>(SC_T_PROFILE); PHZ_HIP(ctx, hipMemsetAsync(prof, 0, (size_t)(2 * grid_t + 2) * 16, sm));
        }
        if (grid_t) {
            hipLaunchKernelGGL(k_tile_base, dim3((unsigned)n_shards), dim3(256), 0, sm, TT, tile_wb);
            hipLaunchKernelGGL(k_line, dim3(grid_t), dim3(LINE_TB), 0, sm, TT, O);
            ColScan CS; CS.tile_wb = tile_wb; CS.tile_m = tile_m; CS.tile_b = tile_b; CS.var_count = d_cnt; CS.rl_cnt = rl_cnt; CS.nb = n_bams;
            if (grid_c) hipLaunchKernelGGL(k_colscan, dim3(grid_c), dim3(TWT * CS_PARTS), 0, sm, TC, TT, CS);
        }
        if (nv) hipLaunchKernelGGL(k_noise, dim3(std::min(nblk(nv), 256u)), dim3(256), 0, sm, (const int32_t *)d_cnt, nv, counters + 4);
        if (int s = gscan_excl<uint32_t, uint32_t>(ctx, rl_cnt, rl_start, (int64_t)NRL, S[SC_T_SCAN_TMP])) return s;
        if (grid_t) {
            TileOut TO;
            TO.line_cls = d_cls; TO.line_q = line_q; TO.q_dup = q_dup; TO.qcount = qcount; TO.items = items; TO.sp_q = sp_q; TO.sp_item = sp_item; TO.touched = touched;
            TO.var_rank = d_rank; TO.var_distinct = d_dist; TO.tile_wb = tile_wb; TO.tile_b = tile_b; TO.rl_start = rl_start; TO.rl_dirty = rl_dirty;
            TO.rl_qid = rl_qid; TO.rl_list = rl_list; TO.rl_cursor = rl_fill; TO.rl_tmp = rl_tmp; TO.counters = counters; TO.nb = n_bams; TO.nv = nv;
            TO.prof = profiling ? prof + 2 * (size_t)grid_t : nullptr;
            hipLaunchKernelGGL(k_tile, dim3(grid_t), dim3(TILE_TB), 0, sm, TT, TO);
        }
        PHZ_HIP(ctx, hipGetLastError());
        // (read-backs go to page-locked memory: a copy into a pageable vector is a blocking, staged copy -- PhzMail in phz_internal.h)
        if (int s = phz_reserve_host(ctx, ctx->mail_host, CNT_BYTES + 64)) return s;
        PHZ_HIP(ctx, hipMemcpyAsync(ctx->mail_host.p, counters, CNT_BYTES, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        memcpy(h_counters.data(), ctx->mail_host.p, CNT_BYTES);
        if (h_counters[13]) return phz_fail(ctx, PHZ_E_UNSUPPORTED, "AS value outside int16");          // (reported by the device-side percentile of a BAM: phz_as_cutoff_enqueue)
        n_kept = (int64_t)spread_sum(2); n_dirty = (int64_t)h_counters[11];
        ctx->counters[PHZ_C_FAR_LINES] += (int64_t)h_counters[12]; ctx->counters[PHZ_C_DIRTY_LISTS] += n_dirty;
        if (profiling) { if (int s = profile_report()) return s; }
        n_complete = (int64_t)grid_t * TL; nt = (int64_t)(h_counters[10] >> 32); n_spill = (int64_t)(h_counters[10] & 0xFFFFFFFFull);
        ctx->counters[PHZ_C_SPILL_LINES] += n_spill; ctx->counters[PHZ_C_SPILL_QNAMES] += nt;
        return PHZ_OK;
    }
    // PHZ_TALLY_PROFILE: lifetimes and start times of the workgroups of k_line and k_tile, from their cycle stamps (a blocking copy of its own)
    int profile_report() {
        std::vector<unsigned long long> pr((size_t)grid_t * 4);
        PHZ_HIP(ctx, hipMemcpy(pr.data(), prof, pr.size() * 8, hipMemcpyDeviceToHost));
        for (int which = 0; which < 2 && grid_t; which++) {
            const size_t b0 = which ? grid_t : 0, nb_ = grid_t;
            unsigned long long t0 = ~0ull, t1 = 0; double sum = 0; unsigned long long mx = 0; std::vector<unsigned long long> d;
            for (size_t b = 0; b < nb_; b++) { const unsigned long long a = pr[2 * (b0 + b)], e = pr[2 * (b0 + b) + 1]; t0 = std::min(t0, a); t1 = std::max(t1, e); sum += (double)(e - a); mx = std::max(mx, e - a); d.push_back(e - a); }
            std::sort(d.begin(), d.end());
            // start-time profile: how many workgroups had started by 10 %, 50 %, 90 % of the kernel's span
            size_t s10 = 0, s50 = 0, s90 = 0; const double span = (double)(t1 - t0);
            for (size_t b = 0; b < nb_; b++) { const double st_ = (double)(pr[2 * (b0 + b)] - t0) / span; s10 += st_ <= 0.1; s50 += st_ <= 0.5; s90 += st_ <= 0.9; }
            fprintf(stderr, "[tally profile] %s: %zu workgroups, span %.1f us, lifetime avg %.2f us median %.2f p99 %.2f max %.2f us, sum %.1f ms -> avg %.0f resident; started by 10/50/90%% of the span: %zu %zu %zu\n",
                    which ? "k_tile" : "k_line", nb_, span / 100.0, sum / nb_ / 100.0, d[nb_ / 2] / 100.0, d[nb_ * 99 / 100] / 100.0, mx / 100.0, sum / 1e5, sum / span, s10, s50, s90);
        }
        fprintf(stderr, "[tally profile] far lines %llu, dirty read lists %lld\n", h_counters[12], (long long)n_dirty);
        return PHZ_OK;
    }
    // ---- the groups of the QNAMEs whose lines straddle tiles, built from the spilled lines; then the read lists with far lines into line order (no wait)
    int spilled_groups_and_dirty_lists() {
        if (nt) {
            hipLaunchKernelGGL(k_group_plan, dim3(nblk(nt)), dim3(256), 0, sm, nt, (const uint32_t *)touched, qcount, cnt_t);
            if (int s = gscan_excl<uint32_t, uint32_t>(ctx, cnt_t, base_t, nt, S[SC_T_SCAN_TMP])) return s;
            hipLaunchKernelGGL(k_group_base, dim3(nblk(nt)), dim3(256), 0, sm, nt, (const uint32_t *)touched, (const uint32_t *)base_t, qcount);
            hipLaunchKernelGGL(k_items_spill, dim3(nblk(n_spill)), dim3(256), 0, sm, n_spill, (const uint32_t *)sp_q, (const uint64_t *)sp_item, qcount, items + n_complete);
            GroupOut G; G.qcount = qcount; G.items = items + n_complete; G.cnt_t = cnt_t; G.base_t = base_t; G.touched = touched; G.var_rank = d_rank; G.var_distinct = d_dist;
            G.counters = counters; G.single_bam = n_bams <= 1 ? 1 : 0;     // one BAM: every QNAME's read_vars list is owned by that BAM
            hipLaunchKernelGGL(k_groups, dim3(nblk(nt)), dim3(256), 0, sm, nt, TT, G);
        }
        PHZ_HIP(ctx, hipMemsetAsync(counters32, 0, 16, sm));
        if (n_dirty) hipLaunchKernelGGL(k_rl_sort_dirty, dim3((unsigned)n_dirty), dim3(256), 0, sm, (const uint32_t *)dirty_list, (const uint32_t *)rl_start, (const uint64_t *)rl_tmp, rl_qid, rl_fill,
                                        big_list, counters32);
        return PHZ_OK;
    }
    template <int MODE> void launch_pairs(int64_t m_items) {
        hipLaunchKernelGGL(k_pairs<MODE>, dim3((unsigned)((m_items + PAIR_ITEMS * PAIR_ROUNDS - 1) / (PAIR_ITEMS * PAIR_ROUNDS))), dim3(PAIRS_TB), 0, sm, (const uint64_t *)items, m_items, tab,
                           (uint32_t)(cap - 1), used, usedkey, deg, counters);
    }
    // ---- variant pairs.  The table is the ctx's own buffer (ctx->tally_table: no other entry point writes it), sized from the variant count and left all zero by
    // k_edge_out: it is cleared only when (re)allocated, after a call that failed half way, and for a retry.  A pass that overflows it is redone with a table four times
    // larger (PHZ_C_PAIR_REDOS).  WAIT 1, once per attempt: the counter block (overflow, edges, dirty lists beyond the LDS stage) and the read-list total
    int pair_table() {
        cap = 1 << 16;
        while (cap < 4 * (uint64_t)NV && cap < (1ull << 30)) cap <<= 1;
        if (ctx->tally_table_cap > cap) cap = ctx->tally_table_cap;          // a sample that needed a larger table keeps it (no overflow + redo per call)
        const int64_t m_items = n_complete + n_spill;                // the tiles' slots, then one slot per spilled line
        for (int attempt = 0;; attempt++) {
            DevBuf &table = ctx->tally_table;
            const size_t old_k = table.cap;
            if (int s = reserve_all(ctx, {{table, cap * GE_WORDS * 4}, {S[SC_T_USED], cap * 4}, {S[SC_T_USEDKEY], cap * 8}})) return s;
            tab = (uint32_t *)table.p; used = scr<uint32_t>(SC_T_USED); usedkey = scr<uint64_t>(SC_T_USEDKEY);
            if (table.cap != old_k || ctx->tally_table_dirty || attempt > 0) PHZ_HIP(ctx, hipMemsetAsync(tab, 0, table.cap, sm));
            ctx->tally_table_dirty = true;
            PHZ_HIP(ctx, hipMemsetAsync(counters, 0, 24, sm));              // overflow
            PHZ_HIP(ctx, hipMemsetAsync(counters + 16, 0, CNT_BYTES - 128, sm));      // spread statistics
            PHZ_HIP(ctx, hipMemsetAsync(counters + 7, 0, 8, sm));           // used slots
            PHZ_HIP(ctx, hipMemsetAsync(deg, 0, NV * 4, sm));               // edges per first variant, counted while the slots are claimed
            if (m_items && getenv("PHZ_TALLY_DEBUG")) { launch_pairs<1>(m_items); launch_pairs<2>(m_items); }
            if (m_items) launch_pairs<0>(m_items);
            PHZ_HIP(ctx, hipGetLastError());
            PhzMail mail(ctx);
            const int m0 = mail.add(counters, CNT_BYTES), m1 = mail.add(rl_start + NRL, 4);       // (counters32 is part of the counter block)
            if (int s = mail.send()) return s;
            PHZ_HIP(ctx, hipStreamSynchronize(sm));
            memcpy(h_counters.data(), mail.at<char>(m0), CNT_BYTES);
            n_big = ((const uint32_t *)(mail.at<char>(m0) + 64))[1];
            n_rl = *mail.at<uint32_t>(m1);
            if (h_counters[2] == 0) { ne = (int64_t)h_counters[7]; ctx->tally_table_cap = cap; return PHZ_OK; }
            if (attempt == 4 || cap >= (1ull << 31)) return phz_fail(ctx, PHZ_E_NOMEM, "variant-pair table did not converge");
            ctx->counters[PHZ_C_PAIR_REDOS]++;
            cap <<= 2;
        }
    }
    // ---- the dirty read lists beyond the LDS stage: through the device radix sort, one list at a time.  TWO BLOCKING COPIES (the list of them, the read-list offsets)
    int big_read_lists() {
        if (!n_big) return PHZ_OK;
        std::vector<uint32_t> big(n_big), rs((size_t)NRL + 1);
        PHZ_HIP(ctx, hipMemcpy(big.data(), big_list, big.size() * 4, hipMemcpyDeviceToHost));
        PHZ_HIP(ctx, hipMemcpy(rs.data(), rl_start, rs.size() * 4, hipMemcpyDeviceToHost));
        size_t longest = 0;
        for (uint32_t e : big) longest = std::max(longest, (size_t)(rs[e + 1] - rs[e]));
        if (int s = reserve_all(ctx, {{R[R_SORTK], longest * 8}, {R[R_SORTV0], longest * 4}, {R[R_SORTV1], longest * 4}})) return s;
        const int hi_bit = 32 + bits_for((uint64_t)(total > 1 ? total - 1 : 1));
        for (uint32_t e : big) {
            const int64_t n = (int64_t)rs[e + 1] - rs[e];
            int where = 0;
            if (int s = radix_sort_pairs<uint64_t, uint32_t>(ctx, rl_tmp + rs[e], res<uint64_t>(R_SORTK), res<uint32_t>(R_SORTV0), res<uint32_t>(R_SORTV1), n, 32, hi_bit,
                                                            R[R_SORTCNT], S[SC_T_SCAN_TMP], &where)) return s;
            hipLaunchKernelGGL(k_rl_take_qid, dim3(nblk(n)), dim3(256), 0, sm, (const uint64_t *)(where ? res<uint64_t>(R_SORTK) : rl_tmp + rs[e]), n, rl_qid + rs[e]);
        }
        return PHZ_OK;
    }
    // ---- the used slots into the (a, b)-ordered pair list; every entry of the table read, written out and returned to "empty" (the caller's timer wait follows)
    int edges() {
        const size_t NE = (size_t)(ne ? ne : 1);
        if (int s = reserve_all(ctx, {{R[R_EA], NE * 4}, {R[R_EB], NE * 4}, {R[R_CELLS], NE * 36}, {R[R_LINKED], NE}, {R[R_CTO], NE * 12}, {R[R_STATS], NE * 20},
                                      {S[SC_T_EB], NE * 4}, {S[SC_T_ESLOT], NE * 4}, {S[SC_T_EA], NE * 4}})) return s;
        if (ne > 0) {
            uint32_t *e_a = scr<uint32_t>(SC_T_EA), *e_b = scr<uint32_t>(SC_T_EB), *e_slot = scr<uint32_t>(SC_T_ESLOT);
            if (int s = gscan_excl<uint32_t, uint32_t>(ctx, deg, eoff, nv, S[SC_T_SCAN_TMP])) return s;
            hipLaunchKernelGGL(k_edge_scatter, dim3(nblk(ne)), dim3(256), 0, sm, (const uint32_t *)used, (const uint64_t *)usedkey, ne, (const uint32_t *)eoff, deg, e_a, e_b, e_slot);
            hipLaunchKernelGGL(k_edge_sort_big, dim3(nblk(nv)), dim3(256), 0, sm, nv, (const uint32_t *)eoff, e_b, e_slot);
            hipLaunchKernelGGL(k_edge_out, dim3(nblk(ne)), dim3(256), 0, sm, ne, (const uint32_t *)eoff, (const uint32_t *)e_a, (const uint32_t *)e_b, (const uint32_t *)e_slot, tab,
                               res<int32_t>(R_EA), res<int32_t>(R_EB), res<int32_t>(R_CELLS), res<uint8_t>(R_LINKED), res<int32_t>(R_CTO), res<int32_t>(R_STATS));
        }
        PHZ_HIP(ctx, hipGetLastError());
        return PHZ_OK;
    }
    // ---- the pass is complete: the persistent arrays are clean again, the results become the resident tally of the ctx
    void publish(phz_tally_sizes *sizes) {
        ctx->tally_dirty = false; ctx->tally_table_dirty = false; ctx->tally_gen++;
        auto &T = ctx->tally;
        T.nv = nv; T.nb = n_bams; T.n_lines = total; T.n_kept = n_kept; T.n_edges = ne; T.n_rl = (int64_t)n_rl;
        T.var_count = d_cnt; T.var_distinct = d_dist; T.var_first = (int64_t *)d_first; T.var_rank = (uint64_t *)d_rank; T.line_cls = d_cls;
        T.ea = res<int32_t>(R_EA); T.eb = res<int32_t>(R_EB); T.cells = res<int32_t>(R_CELLS); T.linked = res<uint8_t>(R_LINKED); T.cto = res<int32_t>(R_CTO); T.stats = res<int32_t>(R_STATS);
        T.rl_start = rl_start; T.rl_qid = rl_qid; T.rl_list = rl_list;
        sizes->n_lines = total; sizes->n_kept = T.n_kept; sizes->n_edges = ne; sizes->n_read_list = T.n_rl;
        sizes->n_items = (int64_t)spread_sum(0); sizes->pair_events = (int64_t)spread_sum(1);
        sizes->noise_match = (int64_t)h_counters[4]; sizes->noise_mismatch = (int64_t)h_counters[5];
        ctx->counters[PHZ_C_LINES] += total; ctx->counters[PHZ_C_ITEMS] += sizes->n_items; ctx->counters[PHZ_C_PAIR_EVENTS] += sizes->pair_events; ctx->counters[PHZ_C_EDGES] += ne;
    }
};
}  // namespace

// The sections of a pass; its host waits: after the line / tile stage, per attempt of the pair table (one, unless the table overflowed), the timer's at the end
extern "C" int phz_tally(phz_ctx *ctx, const phz_lines *shards, int n_shards, int64_t nv, const uint8_t *a0, const uint8_t *a1,
                         int64_t n_qid, int n_bams, phz_tally_sizes *sizes, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || (!shards && n_shards) || !sizes || nv < 0 || n_qid < 0 || n_shards < 0 || n_bams < 1) return PHZ_E_ARG;
    memset(sizes, 0, sizeof(*sizes));
    TallyPass P(ctx, nv, n_qid, n_shards, n_bams);
    if (int s = P.check_and_stage(shards, a0, a1, space)) return s;
    if (int s = P.reserve_and_clear()) return s;
    Timer timer(ctx, PHZ_T_TALLY);
    if (int s = P.lines_and_tiles()) return s;                         // wait 0
    if (int s = P.spilled_groups_and_dirty_lists()) return s;
    if (int s = P.pair_table()) return s;                              // wait 1 (per attempt)
    if (int s = P.big_read_lists()) return s;                          // (blocking copies, rare)
    if (int s = P.edges()) return s;
    if (int s = timer.stop()) return s;                                // the timer wait
    P.publish(sizes);
    return PHZ_OK;
}

// copy the results of the last phz_tally into the caller's arrays (NULL members are skipped); one host wait
extern "C" int phz_tally_fetch(phz_ctx *ctx, const phz_tally_out *out, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !out) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    auto &T = ctx->tally;
    const hipMemcpyKind kind = space == PHZ_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    hipStream_t sm = ctx->stream;
    const size_t nv = (size_t)T.nv, ne = (size_t)T.n_edges;
    const struct { void *dst; const void *src; size_t bytes; } parts[] = {
        {out->var_count, T.var_count, nv * 12}, {out->var_first, T.var_first, nv * 8}, {out->var_distinct, T.var_distinct, nv * 12}, {out->var_rank, T.var_rank, nv * 8},
        {out->line_cls, T.line_cls, (size_t)T.n_lines}, {out->edge_a, T.ea, ne * 4}, {out->edge_b, T.eb, ne * 4}, {out->edge_cells, T.cells, ne * 36}, {out->edge_linked, T.linked, ne},
        {out->edge_cto, T.cto, ne * 12}, {out->edge_stats, T.stats, ne * 20}, {out->rl_start, T.rl_start, (nv * 2 * (size_t)T.nb + 1) * 4}, {out->rl_qid, T.rl_qid, (size_t)T.n_rl * 4}};
    for (const auto &c : parts)
        if (c.dst && c.bytes) PHZ_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, kind, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}

// ------------------------------------------------------------------------------------------------ phz_variant_links
// Allele links among a set of variants, from the pair table the tally left in HBM (phaser.py:1928-1949 generate_hap_network_all: |read_set[v][x] & read_set[o][y]| for
// every pair v < o of a block and x, y in {0, 1} -- cells 0, 1, 3, 4 of the pair's nine, the same deduplicated QNAME sets over all BAMs).  Nothing is intersected again:
//   k_links_head    checks the set (strictly ascending, inside [0, nv)) and cuts the (a, b)-sorted edge list to the edges whose a lies in [vars[0], vars[n - 1]]
//   k_links<false>  one thread per edge of that range: both endpoints looked up in the set (bisection), 2 rows per non-zero cell counted
//   gscan_excl      counts -> offsets (and the total)
//   k_links<true>   the same threads write their rows at the offsets: edge order (= (i, j) order: local order is index order), x, y, direct before inferred
// Placement needs no atomics; the output is the same on every run.  One small launch per run that asks for it, untimed.
namespace {
// number of entries of the ascending array w[0, n) below key
__device__ __forceinline__ int64_t links_lower_bound(const int32_t *w, int64_t n, int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((int64_t)w[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
// head[0] / head[1]: the edge range [lo, hi); head[2] != 0: the set is not strictly ascending inside [0, nv) (zeroed by the driver)
__global__ __launch_bounds__(256) void k_links_head(const int32_t *vars, int64_t n, int64_t nv, const int32_t *ea, int64_t ne, long long *head) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) {
        const int32_t v = vars[t];
        if (v < 0 || (int64_t)v >= nv || (t + 1 < n && vars[t + 1] <= v)) head[2] = 1;
    }
    if (t == 0) head[0] = links_lower_bound(ea, ne, (int64_t)vars[0]);
    if (t == 1) head[1] = links_lower_bound(ea, ne, (int64_t)vars[n - 1] + 1);
}
template <bool FILL> __global__ __launch_bounds__(256) void k_links(const int32_t *vars, int64_t n, const int32_t *ea, const int32_t *eb, const int32_t *cells, int64_t e0,
                                                                    int64_t m, uint32_t *count, const unsigned long long *base, phz_link_rec *rows, int64_t rows_cap) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const int64_t e = e0 + t;
    const int32_t a = ea[e], b = eb[e];
    const int64_t i = links_lower_bound(vars, n, a), j = links_lower_bound(vars, n, b);
    const bool member = i < n && vars[i] == a && j < n && vars[j] == b;
    int32_t c[4] = {0, 0, 0, 0};
    if (member) { const int32_t *row = cells + e * 9; c[0] = row[0]; c[1] = row[1]; c[2] = row[3]; c[3] = row[4]; }
    if (!FILL) {
        count[t] = 2u * (uint32_t)((c[0] > 0) + (c[1] > 0) + (c[2] > 0) + (c[3] > 0));
        return;
    }
    int64_t at = (int64_t)base[t];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (c[k] <= 0) continue;
        if (at + 2 > rows_cap) return;                  // (the driver launches this pass only with room for every row)
        const uint8_t x = (uint8_t)(k >> 1), y = (uint8_t)(k & 1);
        phz_link_rec r;
        r.i = (int32_t)i; r.j = (int32_t)j; r.count = c[k]; r.pad = 0;
        r.allele_i = x; r.allele_j = y; r.inferred = 0; rows[at] = r;
        r.allele_i = (uint8_t)(1 - x); r.allele_j = (uint8_t)(1 - y); r.inferred = 1; rows[at + 1] = r;
        at += 2;
    }
}
}  // namespace

// The link rows of ANY strictly ascending set of variants of the resident tally (a haplotype block is only what the command line passes); see phz.h.
// Host waits: one for the edge range and the verdict on the set, one for the row count, one for the rows of a PHZ_HOST caller.
extern "C" int phz_variant_links(phz_ctx *ctx, const int32_t *vars, int64_t n_vars, phz_link_rec *rows, int64_t rows_cap, int64_t *n_rows, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !n_rows || n_vars < 0 || rows_cap < 0 || (n_vars && !vars) || (rows_cap && !rows)) return PHZ_E_ARG;
    *n_rows = 0;
    // ---- what is resident
    auto &T = ctx->tally;
    if (ctx->tally_gen == 0) return phz_fail(ctx, PHZ_E_ARG, "phz_variant_links: no resident tally (phz_tally or phz_tally_import first)");
    if (T.n_edges && (!T.ea || !T.eb || !T.cells)) return phz_fail(ctx, PHZ_E_ARG, "phz_variant_links: the resident tally was imported without edge_cells (the pair cells are what the links are read from)");
    if (space == PHZ_HOST)
        for (int64_t k = 0; k < n_vars; k++)
            if (vars[k] < 0 || vars[k] >= T.nv || (k && vars[k] <= vars[k - 1])) return phz_fail(ctx, PHZ_E_ARG, "phz_variant_links: vars must be strictly ascending inside [0, nv) of the resident tally");
    if (n_vars < 2 && space == PHZ_HOST) return PHZ_OK;          // no pair, no row (a PHZ_DEVICE set is still checked below)
    if (n_vars == 0) return PHZ_OK;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t sm = ctx->stream;
    Staging st(ctx);
    const int32_t *d_vars; phz_link_rec *d_rows;
    if (int s = st.in(vars, (size_t)n_vars, space, &d_vars)) return s;
    if (int s = st.out(rows, (size_t)rows_cap, space, &d_rows)) return s;
    // ---- the set checked on the device, the edge list cut to its range                                      WAIT
    DevBuf *S = ctx->scratch;
    if (int s = phz_reserve(ctx, S[SC_LINK_HEAD], 3 * sizeof(long long))) return s;
    long long *head = (long long *)S[SC_LINK_HEAD].p;
    PHZ_HIP(ctx, hipMemsetAsync(head, 0, 3 * sizeof(long long), sm));
    hipLaunchKernelGGL(k_links_head, dim3(nblk(n_vars)), dim3(256), 0, sm, d_vars, n_vars, T.nv, (const int32_t *)T.ea, T.n_edges, head);
    PHZ_HIP(ctx, hipGetLastError());
    int64_t e0, m;
    {
        PhzMail mail(ctx);
        const int m0 = mail.add(head, 3 * sizeof(long long));
        if (int s = mail.send()) return s;
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        const long long *h = mail.at<long long>(m0);
        if (h[2]) return phz_fail(ctx, PHZ_E_ARG, "phz_variant_links: vars must be strictly ascending inside [0, nv) of the resident tally");
        e0 = h[0]; m = h[1] - h[0];
    }
    if (n_vars < 2 || m <= 0) return PHZ_OK;
    if (e0 < 0 || e0 + m > T.n_edges) return phz_fail(ctx, PHZ_E_ARG, "phz_variant_links: edge range outside the resident list");
    // ---- count, scan                                                                                         WAIT
    if (int s = reserve_all(ctx, {{S[SC_LINK_COUNT], (size_t)m * 4}, {S[SC_LINK_BASE], ((size_t)m + 1) * 8}})) return s;
    uint32_t *count = (uint32_t *)S[SC_LINK_COUNT].p;
    unsigned long long *base = (unsigned long long *)S[SC_LINK_BASE].p;
    hipLaunchKernelGGL(k_links<false>, dim3(nblk(m)), dim3(256), 0, sm, d_vars, n_vars, (const int32_t *)T.ea, (const int32_t *)T.eb, (const int32_t *)T.cells, e0, m, count,
                       (const unsigned long long *)nullptr, (phz_link_rec *)nullptr, (int64_t)0);
    PHZ_HIP(ctx, hipGetLastError());
    if (int s = gscan_excl<uint32_t, unsigned long long>(ctx, count, base, m, S[SC_LINK_SCAN_TMP])) return s;
    int64_t total;
    {
        PhzMail mail(ctx);
        const int m0 = mail.add(base + m, 8);
        if (int s = mail.send()) return s;
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        total = (int64_t)*mail.at<unsigned long long>(m0);
    }
    *n_rows = total;
    if (total > rows_cap) return phz_fail(ctx, PHZ_E_CAPACITY, "phz_variant_links: rows_cap too small (n_rows holds the number of rows)");
    if (total == 0) return PHZ_OK;
    // ---- fill                                                                                                WAIT
    hipLaunchKernelGGL(k_links<true>, dim3(nblk(m)), dim3(256), 0, sm, d_vars, n_vars, (const int32_t *)T.ea, (const int32_t *)T.eb, (const int32_t *)T.cells, e0, m,
                       (uint32_t *)nullptr, (const unsigned long long *)base, d_rows, rows_cap);
    PHZ_HIP(ctx, hipGetLastError());
    if (space == PHZ_HOST) PHZ_HIP(ctx, hipMemcpyAsync(rows, d_rows, (size_t)total * sizeof(phz_link_rec), hipMemcpyDeviceToHost, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}

// ------------------------------------------------------------------------------------------------ phz_read_haplotypes
// Which template votes for which haplotype of which block: per (block, BAM, QNAME id) the number of read-list entries on alleles haplotype A carries and on the
// other allele, over ALL blocks of the caller's table at once, from the read lists the tally left in HBM (rl_list / rl_qid: one entry per kept ref / alt line).
//   k_rh_head      the block offsets checked (ascending, not below 0, not more slots than variants)
//   k_rh_scatter   one thread per block-variant slot: vblk[v] = block ordinal (-1: in no block, -2: in a block but left out of the vote), vside[v] = allele on
//                  haplotype A; the slot's block by bisection of the offsets; a second writer to vblk[v] = a variant in two blocks
//   k_rh_keys      one thread per read-list entry: key = block | BAM | QNAME id | side (bit 0: 0 = the allele haplotype A carries).  The entries are partitioned:
//                  survivors first, in entry order, the dropped ones behind them with a key above every block (in-wave rank from a ballot, the workgroups'
//                  counts through gscan_excl, the same threads fill) -- the number of survivors never visits the host, the sort takes all n_rl keys
//   radix sort     over the significant bits of the key
//   k_rh_runs      heads of full-key runs compacted into a position list (the same count / scan / fill; the scan carries runs and rows in one 64-bit sum); a
//                  head that also starts a new (block, BAM, QNAME id) knows its row
//   k_rh_rows      one thread per run that starts a row: its length and the length of the next run when that one has the same (block, BAM, QNAME id) -- both are
//                  differences of neighbouring list entries, so no thread walks a run whatever its length
// Host waits: one for the verdict on the arguments and the row count, one for the rows.  Every run gives the same records.  Untimed.
namespace {
enum { RH_F_OFF = 0, RH_F_RANGE = 1, RH_F_TWICE = 2, RH_F_HAP = 3 };          // words of the verdict block (zeroed by the driver)
__global__ __launch_bounds__(256) void k_rh_head(const int64_t *blk_off, int64_t n_blocks, int64_t nv, uint32_t *flag) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > n_blocks) return;
    const int64_t o = blk_off[k];
    if (o < 0 || (k < n_blocks && blk_off[k + 1] < o)) flag[RH_F_OFF] = 1;
    if (k == 0 && blk_off[n_blocks] - o > nv) flag[RH_F_TWICE] = 1;          // more slots than variants: some variant is there twice
}
__global__ __launch_bounds__(256) void k_rh_scatter(const int64_t *blk_off, int64_t n_blocks, const int32_t *blk_var, const uint8_t *blk_hap, const uint8_t *var_skip, int64_t nv,
                                                    int32_t *vblk, uint8_t *vside, uint32_t *flag) {
    if (flag[RH_F_OFF] | flag[RH_F_TWICE]) return;          // offsets that say nothing about the slot arrays: those are not read
    const int64_t s = blk_off[0] + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= blk_off[n_blocks]) return;
    int64_t lo = 0, hi = n_blocks;                           // the last block that starts at or before s (empty blocks share their offset with the next one)
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (blk_off[mid] <= s) lo = mid; else hi = mid; }
    const int32_t v = blk_var[s];
    const uint8_t h = blk_hap[s];
    if (v < 0 || (int64_t)v >= nv) { flag[RH_F_RANGE] = 1; return; }
    if (h > 1) { flag[RH_F_HAP] = 1; return; }
    const int32_t mine = var_skip && var_skip[v] ? -2 : (int32_t)lo;
    if (atomicCAS(&vblk[v], -1, mine) != -1) flag[RH_F_TWICE] = 1; else vside[v] = h;
}
// place of a live thread among the live threads of its workgroup of 256 (ballot inside the wave, the four waves' counts in s_w), *total = their number; every
// thread of the workgroup calls it
__device__ __forceinline__ uint32_t rh_wg_rank(bool live, uint32_t *s_w, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(live ? 1 : 0);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; w++) before += s_w[w];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return before + (uint32_t)__popcll(m & below);
}
struct RhKeys {
    const uint32_t *rl_list; const int32_t *rl_qid; int64_t n, nv; uint32_t nb;
    const int32_t *vblk; const uint8_t *vside, *bam_skip; const uint32_t *flag;
    int bam_shift, blk_shift; unsigned long long pad;          // pad: the key of a dropped entry (block field = n_blocks)
};
template <bool FILL> __global__ __launch_bounds__(256) void k_rh_keys(RhKeys a, uint32_t *wg_count, const uint32_t *wg_base, unsigned long long *keys) {
    __shared__ uint32_t s_w[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool live = false;
    unsigned long long key = a.pad;
    if (i < a.n && !(a.flag[RH_F_OFF] | a.flag[RH_F_RANGE] | a.flag[RH_F_TWICE] | a.flag[RH_F_HAP])) {
        const uint32_t e = a.rl_list[i], bam = e % a.nb, va = e / a.nb;
        const int64_t v = (int64_t)(va >> 1);
        const int32_t k = v < a.nv ? a.vblk[v] : -1;
        if (k >= 0 && !(a.bam_skip && a.bam_skip[bam])) {
            live = true;
            key = ((unsigned long long)(uint32_t)k << a.blk_shift) | ((unsigned long long)bam << a.bam_shift) | ((unsigned long long)(uint32_t)a.rl_qid[i] << 1) |
                  (unsigned long long)((va & 1u) != (uint32_t)a.vside[v]);
        }
    }
    uint32_t total;
    const uint32_t rank = rh_wg_rank(live, s_w, &total);
    if (!FILL) { if (threadIdx.x == 0) wg_count[blockIdx.x] = total; return; }
    if (i >= a.n) return;
    const int64_t m = (int64_t)wg_base[gridDim.x], before = (int64_t)wg_base[blockIdx.x] + rank;          // survivors in all / in front of this entry
    keys[live ? before : m + (i - before)] = key;
}
// counts and bases: runs in the high half, rows in the low half of one 64-bit sum (both below 2^30)
template <bool FILL> __global__ __launch_bounds__(256) void k_rh_runs(const unsigned long long *keys, const uint32_t *n_live, unsigned long long *wg_count, const unsigned long long *wg_base,
                                                                      uint32_t *run_pos, int32_t *run_row) {
    __shared__ uint32_t s_run[4], s_row[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < (int64_t)*n_live;
    const unsigned long long key = in ? keys[i] : 0ull, prev = in && i > 0 ? keys[i - 1] : 0ull;
    const bool run_head = in && (i == 0 || key != prev), row_head = in && (i == 0 || (key >> 1) != (prev >> 1));
    uint32_t runs, rows;
    const uint32_t run_rank = rh_wg_rank(run_head, s_run, &runs), row_rank = rh_wg_rank(row_head, s_row, &rows);
    if (!FILL) { if (threadIdx.x == 0) wg_count[blockIdx.x] = ((unsigned long long)runs << 32) | rows; return; }
    if (!run_head) return;
    const unsigned long long base = wg_base[blockIdx.x];
    const uint32_t r = (uint32_t)(base >> 32) + run_rank;
    run_pos[r] = (uint32_t)i;
    run_row[r] = row_head ? (int32_t)((uint32_t)base + row_rank) : -1;
}
__global__ __launch_bounds__(256) void k_rh_rows(const unsigned long long *keys, const uint32_t *n_live, const unsigned long long *totals, const uint32_t *run_pos, const int32_t *run_row,
                                                 int bam_shift, int blk_shift, phz_readhap_rec *rows, int64_t rows_cap) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x, n_runs = (int64_t)(*totals >> 32);
    if (r >= n_runs) return;
    const int64_t row = run_row[r];
    if (row < 0 || row >= rows_cap) return;                  // (the driver launches this kernel only with room for every row)
    const uint32_t m = *n_live, p0 = run_pos[r], p1 = r + 1 < n_runs ? run_pos[r + 1] : m;
    const unsigned long long key = keys[p0];
    int32_t a = 0, b = 0;
    if (key & 1ull) b = (int32_t)(p1 - p0);
    else {
        a = (int32_t)(p1 - p0);
        if (r + 1 < n_runs && (keys[p1] >> 1) == (key >> 1)) b = (int32_t)((r + 2 < n_runs ? run_pos[r + 2] : m) - p1);
    }
    phz_readhap_rec rec;
    rec.block = (int32_t)(key >> blk_shift); rec.bam = (int32_t)((key >> bam_shift) & ((1ull << (blk_shift - bam_shift)) - 1ull)); rec.qid = (int32_t)(uint32_t)(key >> 1);
    rec.a = a; rec.b = b;
    rows[row] = rec;
}
const char *rh_verdict(const uint32_t *f) {
    if (f[RH_F_OFF]) return "phz_read_haplotypes: blk_off must ascend from a value not below 0";
    if (f[RH_F_RANGE]) return "phz_read_haplotypes: a block variant outside [0, nv) of the resident tally";
    if (f[RH_F_HAP]) return "phz_read_haplotypes: blk_hap holds a value above 1";
    if (f[RH_F_TWICE]) return "phz_read_haplotypes: a variant in two blocks (or twice in one)";
    return nullptr;
}
}  // namespace

extern "C" int phz_read_haplotypes(phz_ctx *ctx, int64_t n_blocks, const int64_t *blk_off, const int32_t *blk_var, const uint8_t *blk_hap, const uint8_t *var_skip,
                                   const uint8_t *bam_skip, phz_readhap_rec *rows, int64_t rows_cap, int64_t *n_rows, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !n_rows || n_blocks < 0 || rows_cap < 0 || (n_blocks && !blk_off) || (rows_cap && !rows)) return PHZ_E_ARG;
    *n_rows = 0;
    // ---- what is resident
    auto &T = ctx->tally;
    if (ctx->tally_gen == 0) return phz_fail(ctx, PHZ_E_ARG, "phz_read_haplotypes: no resident tally (phz_tally or phz_tally_import first)");
    if (!T.rl_start || !T.rl_qid || !T.rl_list)
        return phz_fail(ctx, PHZ_E_ARG, "phz_read_haplotypes: the resident tally was imported without its read lists (rl_start, rl_qid and rl_list are what the votes are read from)");
    // ---- arguments a host caller hands over: checked before anything is launched
    const int64_t nv = T.nv, n_rl = T.n_rl;
    int64_t n_slots = nv;                                    // threads of the scatter (a PHZ_DEVICE table has at most one slot per variant, or the head kernel refuses it)
    if (space == PHZ_HOST && n_blocks) {
        uint32_t f[4] = {0, 0, 0, 0};
        for (int64_t k = 0; k <= n_blocks; k++)
            if (blk_off[k] < 0 || (k < n_blocks && blk_off[k + 1] < blk_off[k])) f[RH_F_OFF] = 1;
        if (!f[RH_F_OFF]) {
            n_slots = blk_off[n_blocks] - blk_off[0];
            if (n_slots && (!blk_var || !blk_hap)) return PHZ_E_ARG;
            std::vector<uint8_t> seen((size_t)nv, 0);
            for (int64_t s = blk_off[0]; s < blk_off[n_blocks]; s++) {
                const int32_t v = blk_var[s];
                if (v < 0 || v >= nv) { f[RH_F_RANGE] = 1; continue; }
                if (blk_hap[s] > 1) f[RH_F_HAP] = 1;
                if (seen[(size_t)v]) f[RH_F_TWICE] = 1;
                seen[(size_t)v] = 1;
            }
        }
        if (const char *why = rh_verdict(f)) return phz_fail(ctx, PHZ_E_ARG, why);
    }
    if (n_blocks == 0) return PHZ_OK;
    if (space == PHZ_DEVICE && (!blk_var || !blk_hap)) return PHZ_E_ARG;
    // ---- the key: block | BAM | QNAME id (32 bits as stored) | side
    const int bam_shift = 33, bam_bits = bits_for((uint64_t)(T.nb > 1 ? T.nb - 1 : 1)), blk_shift = bam_shift + bam_bits, blk_bits = bits_for((uint64_t)n_blocks);
    if (blk_shift + blk_bits > 64) return phz_fail(ctx, PHZ_E_UNSUPPORTED, "phz_read_haplotypes: (block, bam, qid, side) does not fit a 64-bit key");
    if (n_rl >= (1ll << 30)) return phz_fail(ctx, PHZ_E_UNSUPPORTED, "phz_read_haplotypes: 2^30 read-list entries or more (the device sort takes fewer)");
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t sm = ctx->stream;
    Staging st(ctx);
    const int64_t *d_off; const int32_t *d_var; const uint8_t *d_hap, *d_vskip, *d_bskip; phz_readhap_rec *d_rows;
    const size_t host_slots = space == PHZ_HOST ? (size_t)(blk_off[0] + n_slots) : 0;          // (the device copy keeps the caller's slot numbers)
    if (int s = st.in(blk_off, (size_t)n_blocks + 1, space, &d_off)) return s;
    if (int s = st.in(blk_var, host_slots, space, &d_var)) return s;
    if (int s = st.in(blk_hap, host_slots, space, &d_hap)) return s;
    if (int s = st.in(var_skip, (size_t)nv, space, &d_vskip)) return s;
    if (int s = st.in(bam_skip, (size_t)T.nb, space, &d_bskip)) return s;
    if (int s = st.out(rows, (size_t)rows_cap, space, &d_rows)) return s;
    // ---- scatter: the block and the side of every variant
    DevBuf *S = ctx->scratch;
    const int64_t nwg = (n_rl + 255) / 256;
    if (int s = reserve_all(ctx, {{S[SC_RH_FLAG], 4 * sizeof(uint32_t)}, {S[SC_RH_VBLK], (size_t)(nv ? nv : 1) * 4}, {S[SC_RH_VSIDE], (size_t)(nv ? nv : 1)},
                                  {S[SC_RH_KEY0], (size_t)(n_rl ? n_rl : 1) * 8}, {S[SC_RH_KEY1], (size_t)(n_rl ? n_rl : 1) * 8}, {S[SC_RH_VAL0], (size_t)(n_rl ? n_rl : 1)},
                                  {S[SC_RH_VAL1], (size_t)(n_rl ? n_rl : 1)}, {S[SC_RH_LIVE_COUNT], (size_t)(nwg ? nwg : 1) * 4}, {S[SC_RH_LIVE_BASE], ((size_t)nwg + 1) * 4},
                                  {S[SC_RH_RUN_COUNT], (size_t)(nwg ? nwg : 1) * 8}, {S[SC_RH_RUN_BASE], ((size_t)nwg + 1) * 8}})) return s;
    uint32_t *flag = (uint32_t *)S[SC_RH_FLAG].p;
    int32_t *vblk = (int32_t *)S[SC_RH_VBLK].p; uint8_t *vside = (uint8_t *)S[SC_RH_VSIDE].p;
    PHZ_HIP(ctx, hipMemsetAsync(flag, 0, 4 * sizeof(uint32_t), sm));
    if (nv) { PHZ_HIP(ctx, hipMemsetAsync(vblk, 0xFF, (size_t)nv * 4, sm)); PHZ_HIP(ctx, hipMemsetAsync(vside, 0, (size_t)nv, sm)); }
    hipLaunchKernelGGL(k_rh_head, dim3(nblk(n_blocks + 1)), dim3(256), 0, sm, d_off, n_blocks, nv, flag);
    if (n_slots) hipLaunchKernelGGL(k_rh_scatter, dim3(nblk(n_slots)), dim3(256), 0, sm, d_off, n_blocks, d_var, d_hap, d_vskip, nv, vblk, vside, flag);
    PHZ_HIP(ctx, hipGetLastError());
    // ---- keys of the surviving entries, sorted; heads of runs, rows counted                                   WAIT
    unsigned long long *keys = (unsigned long long *)S[SC_RH_KEY0].p, *other = (unsigned long long *)S[SC_RH_KEY1].p;
    uint32_t *live_count = (uint32_t *)S[SC_RH_LIVE_COUNT].p, *live_base = (uint32_t *)S[SC_RH_LIVE_BASE].p;
    unsigned long long *run_count = (unsigned long long *)S[SC_RH_RUN_COUNT].p, *run_base = (unsigned long long *)S[SC_RH_RUN_BASE].p;
    uint32_t *run_pos = nullptr; int32_t *run_row = nullptr;
    if (n_rl) {
        RhKeys a;
        a.rl_list = T.rl_list; a.rl_qid = T.rl_qid; a.n = n_rl; a.nv = nv; a.nb = (uint32_t)T.nb; a.vblk = vblk; a.vside = vside; a.bam_skip = d_bskip; a.flag = flag;
        a.bam_shift = bam_shift; a.blk_shift = blk_shift; a.pad = (unsigned long long)n_blocks << blk_shift;
        hipLaunchKernelGGL(k_rh_keys<false>, dim3((unsigned)nwg), dim3(256), 0, sm, a, live_count, (const uint32_t *)nullptr, (unsigned long long *)nullptr);
        PHZ_HIP(ctx, hipGetLastError());
        if (int s = gscan_excl<uint32_t, uint32_t>(ctx, live_count, live_base, nwg, S[SC_RH_SCAN_TMP])) return s;
        hipLaunchKernelGGL(k_rh_keys<true>, dim3((unsigned)nwg), dim3(256), 0, sm, a, (uint32_t *)nullptr, (const uint32_t *)live_base, keys);
        PHZ_HIP(ctx, hipGetLastError());
        const int range[1][2] = {{0, blk_shift + blk_bits}};
        int where = 0;
        if (int s = radix_sort_ranges<unsigned long long, uint8_t>(ctx, keys, other, (uint8_t *)S[SC_RH_VAL0].p, (uint8_t *)S[SC_RH_VAL1].p, n_rl, range, 1, S[SC_RH_SORT_COUNT],
                                                                     S[SC_RH_SCAN_TMP], &where)) return s;
        if (where) std::swap(keys, other);
        run_pos = (uint32_t *)other; run_row = (int32_t *)(run_pos + n_rl);          // the sort's other buffer is free again: 8 bytes per entry, as the two lists need
        hipLaunchKernelGGL(k_rh_runs<false>, dim3((unsigned)nwg), dim3(256), 0, sm, (const unsigned long long *)keys, (const uint32_t *)(live_base + nwg), run_count,
                           (const unsigned long long *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr);
        PHZ_HIP(ctx, hipGetLastError());
        if (int s = gscan_excl<unsigned long long, unsigned long long>(ctx, run_count, run_base, nwg, S[SC_RH_SCAN_TMP])) return s;
        hipLaunchKernelGGL(k_rh_runs<true>, dim3((unsigned)nwg), dim3(256), 0, sm, (const unsigned long long *)keys, (const uint32_t *)(live_base + nwg), (unsigned long long *)nullptr,
                           (const unsigned long long *)run_base, run_pos, run_row);
        PHZ_HIP(ctx, hipGetLastError());
    }
    int64_t n_runs = 0, total = 0;
    {
        PhzMail mail(ctx);
        const int m0 = mail.add(flag, 4 * sizeof(uint32_t)), m1 = n_rl ? mail.add(run_base + nwg, 8) : -1;
        if (int s = mail.send()) return s;
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        if (const char *why = rh_verdict(mail.at<uint32_t>(m0))) return phz_fail(ctx, PHZ_E_ARG, why);
        if (n_rl) { const unsigned long long t = *mail.at<unsigned long long>(m1); n_runs = (int64_t)(t >> 32); total = (int64_t)(t & 0xFFFFFFFFull); }
    }
    *n_rows = total;
    if (total > rows_cap) return phz_fail(ctx, PHZ_E_CAPACITY, "phz_read_haplotypes: rows_cap too small (n_rows holds the number of rows)");
    if (total == 0) return PHZ_OK;
    // ---- one record per row, from the run list                                                               WAIT
    hipLaunchKernelGGL(k_rh_rows, dim3(nblk(n_runs)), dim3(256), 0, sm, (const unsigned long long *)keys, (const uint32_t *)(live_base + nwg), (const unsigned long long *)(run_base + nwg),
                       (const uint32_t *)run_pos, (const int32_t *)run_row, bam_shift, blk_shift, d_rows, rows_cap);
    PHZ_HIP(ctx, hipGetLastError());
    if (space == PHZ_HOST) PHZ_HIP(ctx, hipMemcpyAsync(rows, d_rows, (size_t)total * sizeof(phz_readhap_rec), hipMemcpyDeviceToHost, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}

// edge_a == edge_b == NULL: the edges of the last phz_tally, still resident in HBM (n_edges must match); keep[] lives in `space`
extern "C" int phz_components(phz_ctx *ctx, int64_t nv, int64_t n_edges, const int32_t *edge_a, const int32_t *edge_b,
                              const uint8_t *keep, int32_t *label, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || nv < 0 || n_edges < 0 || (!label && nv)) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    const int32_t *ea, *eb; const uint8_t *kp; int32_t *lab;
    if (!edge_a && !edge_b && n_edges) {
        if (n_edges != ctx->tally.n_edges || nv != ctx->tally.nv) return phz_fail(ctx, PHZ_E_ARG, "no resident edge list of that size");
        ea = ctx->tally.ea; eb = ctx->tally.eb;
    } else {
        if (n_edges && (!edge_a || !edge_b)) return phz_fail(ctx, PHZ_E_ARG, "phz_components: one edge array is NULL");
        if (space == PHZ_HOST)                  // a caller's host arrays: one bad endpoint would write outside parent[]
            for (int64_t i = 0; i < n_edges; i++)
                if (edge_a[i] < 0 || edge_a[i] >= nv || edge_b[i] < 0 || edge_b[i] >= nv)
                    return phz_fail(ctx, PHZ_E_ARG, "phz_components: edge endpoint outside [0, nv)");
        if (int s = st.in(edge_a, (size_t)n_edges, space, &ea)) return s;
        if (int s = st.in(edge_b, (size_t)n_edges, space, &eb)) return s;
    }
    if (int s = st.in(keep, (size_t)n_edges, space, &kp)) return s;
    if (int s = st.out(label, (size_t)nv, space, &lab)) return s;
    if (int s = phz_reserve(ctx, ctx->scratch[SC_UF_PARENT], (size_t)(nv ? nv : 1) * 4)) return s;
    int32_t *parent = (int32_t *)ctx->scratch[SC_UF_PARENT].p;
    Timer t(ctx, PHZ_T_COMPONENTS);
    if (nv) hipLaunchKernelGGL(k_uf_init, dim3(nblk(nv)), dim3(256), 0, ctx->stream, parent, nv);
    if (n_edges) hipLaunchKernelGGL(k_uf_hook, dim3(nblk(n_edges)), dim3(256), 0, ctx->stream, parent, ea, eb, kp, n_edges);
    if (nv) hipLaunchKernelGGL(k_uf_flatten, dim3(nblk(nv)), dim3(256), 0, ctx->stream, parent, lab, nv);
    PHZ_HIP(ctx, hipGetLastError());
    if (int s = t.stop()) return s;
    if (space == PHZ_HOST && nv) PHZ_HIP(ctx, hipMemcpyAsync(label, lab, (size_t)nv * 4, hipMemcpyDeviceToHost, ctx->stream));
    PHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PHZ_OK;
}
