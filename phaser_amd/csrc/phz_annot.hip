// K_annot: the pair loops of phaser_annotate (phaser_annotate/phaser_annotate.py:344-403, :225-247, :426) for every gene of a sample in
// count -> scan -> fill form (include/phz.h, phz_annot_pairs).
//
// A gene with n GW entries and m PG entries has n^2 + m^2 ordered pairs: pair p < n^2 belongs to the first pass (a = p / n, b = p % n), the others
// to the second (q = p - n^2, a = n + q / m, b = n + q % m).  The host driver cuts every pass into TILES of PHZ_ANNOT_TILE consecutive pairs (a tile never
// holds pairs of two genes or of two passes); a workgroup owns a tile, a thread a pair.  k_annot<false> reduces the rows of a tile's pairs (0..8 each) to one
// total per tile, gscan_excl (phz_scan.h) turns the totals of a batch's tiles into bases, k_annot<true> recomputes the pairs, takes a workgroup exclusive scan
// and writes every pair's records at base + local offset: no per-pair value reaches memory and no atomic decides a position, so the records come out in the
// reference's order whatever the schedule.
//
// A pair (:358-401).  interactions(A, B) = the combinations (A[i], B[j], cis if i == j else trans), i-major, of two info rows in one block, without those
// that involve allele 0; it is held as one 64-bit word of four 16-bit items (valid bit, a, b, trans), so list equality is word equality.
//   pass 1: rows of the GW list with read_backed by the ladder of :370-379 against the PG list (taken only when both variants are in the gene's PG list);
//           when the two lists have the same length and differ (-1), the PG list follows with read_backed 1.
//   pass 2: skipped when both variants are in the gene's GW list (the first pass put the pair into outputted_configs, :386) or when an entry is
//           not the first of its variant in the PG list (the pair was added by an earlier iteration, :401); else the PG list with read_backed 1.
// A combination yields a row only if both alleles are in the entries' annotation masks (:426).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "phz.h"
#include "phz_internal.h"
#include "phz_scan.h"

#ifndef PHZ_ANNOT_TILE
#define PHZ_ANNOT_TILE 256          // pairs per tile (at most the 256 threads of a workgroup); the emulation tests shrink it to 8
#endif
static_assert(PHZ_ANNOT_TILE >= 1 && PHZ_ANNOT_TILE <= 256, "a thread owns one pair of its tile");
#ifndef PHZ_ANNOT_GRID
#define PHZ_ANNOT_GRID (1 << 22)    // most tiles per launch: 2^22 workgroups x 256 threads stays below the 2^32 threads a grid dimension may hold
#endif

namespace {

constexpr int THREADS = 256;

struct AnnotArgs {
    const int64_t *entry_off;
    const int32_t *n_gw;
    const int32_t *entry_var;
    const uint16_t *entry_mask;
    const uint8_t *entry_flags;
    const uint8_t *gw_allele, *pg_allele;
    const int32_t *gw_block, *pg_block;
    const int32_t *tile_gene;      // [n_tiles]
    const int64_t *tile_start;     // [n_tiles] first pair of the tile in the gene's pair space
    int64_t t0;                    // first tile of the batch (0 in the count pass)
    int64_t b0;                    // first tile of this launch, relative to t0
    uint32_t *tile_count;          // [n_tiles]
    const uint32_t *tile_base;     // fill: exclusive scan of tile_count[t0 ...], relative to the batch
    uint4 *out;                    // fill: the batch's records
};

// the filtered interaction list of two info rows: item k in bits [16 k, 16 k + 16) = 0x8000 | a | b << 4 | trans << 8
__device__ __forceinline__ uint64_t interactions(const uint8_t *al_a, int32_t blk_a, const uint8_t *al_b, int32_t blk_b) {
    if (blk_a != blk_b) return 0;
    uint64_t key = 0;
    int n = 0;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t x = al_a[i], y = al_b[j];
            if (x != 0 && y != 0) { key |= (uint64_t)(0x8000u | x | (y << 4) | ((uint32_t)(i != j) << 8)) << (16 * n); n++; }
        }
    return key;
}
__device__ __forceinline__ int list_len(uint64_t key) { return (int)((key >> 15) & 1) + (int)((key >> 31) & 1) + (int)((key >> 47) & 1) + (int)((key >> 63) & 1); }
__device__ __forceinline__ int list_rows(uint64_t key, uint32_t mask_a, uint32_t mask_b) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t it = (uint32_t)(key >> (16 * k)) & 0xFFFFu;
        n += (int)((it >> 15) & (mask_a >> (it & 15u)) & (mask_b >> ((it >> 4) & 15u)) & 1u);
    }
    return n;
}

struct Pair {
    int32_t gene, ea, eb;
    uint32_t mask_a, mask_b;
    uint64_t first, second;        // the two lists of the pair in output order (second: the PG list of a conflicting first-pass pair)
    uint32_t first_bits, second_bits;      // bits 9-11 of their records
    int rows;
};

__device__ __forceinline__ Pair pair_of(const AnnotArgs &a, int64_t tile, int tid) {
    Pair P;
    P.rows = 0; P.first = P.second = 0; P.first_bits = P.second_bits = 0; P.mask_a = P.mask_b = 0; P.ea = P.eb = 0;
    const int32_t g = a.tile_gene[tile];
    P.gene = g;
    const int64_t e0 = a.entry_off[g];
    const int64_t n = a.n_gw[g], m = a.entry_off[g + 1] - e0 - n;
    const int64_t start = a.tile_start[tile];
    const bool pass2 = start >= n * n;
    const int64_t end = pass2 ? n * n + m * m : n * n;
    const int64_t p = start + tid;
    if (tid >= PHZ_ANNOT_TILE || p >= end) return P;
    int64_t ea, eb;
    if (!pass2) { ea = e0 + p / n; eb = e0 + p % n; }
    else { const int64_t q = p - n * n; ea = e0 + n + q / m; eb = e0 + n + q % m; }
    P.ea = (int32_t)ea; P.eb = (int32_t)eb;
    const int32_t va = a.entry_var[ea], vb = a.entry_var[eb];
    if (va == vb) return P;
    P.mask_a = a.entry_mask[ea]; P.mask_b = a.entry_mask[eb];
    const uint32_t fa = a.entry_flags[ea], fb = a.entry_flags[eb];
    const bool both = (fa & fb & PHZ_ANNOT_BOTH) != 0;
    if (!pass2) {
        const uint64_t gw = interactions(a.gw_allele + 2 * (int64_t)va, a.gw_block[va], a.gw_allele + 2 * (int64_t)vb, a.gw_block[vb]);
        const uint64_t rb = both ? interactions(a.pg_allele + 2 * (int64_t)va, a.pg_block[va], a.pg_allele + 2 * (int64_t)vb, a.pg_block[vb]) : 0;
        int read_backed = 0;                                        // :370-379
        const bool same_len = list_len(gw) == list_len(rb);
        if (same_len && gw == rb) read_backed = 1;
        if (same_len && gw != rb) read_backed = -1;
        else if (rb == 0) read_backed = 0;
        P.first = gw; P.first_bits = (uint32_t)(read_backed + 1) << 10;
        if (read_backed == -1) { P.second = rb; P.second_bits = (1u << 9) | (2u << 10); }
    } else {
        if (both || !(fa & PHZ_ANNOT_FIRST) || !(fb & PHZ_ANNOT_FIRST)) return P;
        P.first = interactions(a.pg_allele + 2 * (int64_t)va, a.pg_block[va], a.pg_allele + 2 * (int64_t)vb, a.pg_block[vb]);
        P.first_bits = (1u << 9) | (2u << 10);
    }
    P.rows = list_rows(P.first, P.mask_a, P.mask_b) + list_rows(P.second, P.mask_a, P.mask_b);
    return P;
}

__device__ __forceinline__ uint32_t write_list(uint4 *out, uint32_t at, const Pair &P, uint64_t key, uint32_t bits) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t it = (uint32_t)(key >> (16 * k)) & 0xFFFFu;
        if ((it >> 15) & (P.mask_a >> (it & 15u)) & (P.mask_b >> ((it >> 4) & 15u)) & 1u)
            out[at++] = make_uint4((uint32_t)P.gene, (uint32_t)P.ea, (uint32_t)P.eb, (it & 0x1FFu) | bits);
    }
    return at;
}

template <bool FILL> __global__ __launch_bounds__(THREADS) void k_annot(AnnotArgs a) {
    __shared__ uint32_t s_w[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = a.t0 + a.b0 + blockIdx.x;
    const Pair P = pair_of(a, tile, tid);
    const uint32_t c = (uint32_t)P.rows;
    if (!FILL) {
        uint32_t x = c;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
        if (lane == 0) s_w[wave] = x;
        __syncthreads();
        if (tid == 0) a.tile_count[tile] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    } else {
        const uint32_t incl = gs_wave_incl(c, lane);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t at = a.tile_base[a.b0 + blockIdx.x] + incl - c;
        for (int w = 0; w < wave; w++) at += s_w[w];
        if (c) {
            at = write_list(a.out, at, P, P.first, P.first_bits);
            write_list(a.out, at, P, P.second, P.second_bits);
        }
    }
}

}  // namespace

extern "C" int phz_annot_pairs(phz_ctx *ctx, const phz_annot_in *in, int64_t batch_rows, phz_annot_rec *rows, int64_t rows_cap, int64_t *n_rows,
                               int64_t *n_pairs, int32_t *n_batches) {
    PhzEnter phz_guard_(ctx);
    static_assert(sizeof(phz_annot_rec) == sizeof(uint4), "one 16-byte store per record");
    if (!ctx || !in || !n_rows || in->n_genes < 0 || in->n_entries < 0 || in->n_vars < 0 || batch_rows < 0 || batch_rows > (1ll << 30) || rows_cap < 0 ||
        in->n_genes >= (1ll << 31) || in->n_entries >= (1ll << 31))
        return PHZ_E_ARG;
    *n_rows = 0;
    if (n_pairs) *n_pairs = 0;
    if (n_batches) *n_batches = 0;
    if (in->n_genes == 0) return PHZ_OK;
    if (!in->entry_off || !in->n_gw || (in->n_entries && (!in->entry_var || !in->entry_mask || !in->entry_flags)) ||
        (in->n_vars && (!in->gw_allele || !in->pg_allele || !in->gw_block || !in->pg_block)))
        return PHZ_E_ARG;
    if (batch_rows == 0) batch_rows = PHZ_ANNOT_BATCH_ROWS;
    // ---- every index the kernels follow is checked here
    if (in->entry_off[0] != 0 || in->entry_off[in->n_genes] != in->n_entries) return phz_fail(ctx, PHZ_E_ARG, "phz_annot_pairs: entry_off does not span the entries");
    for (int64_t g = 0; g < in->n_genes; g++) {
        const int64_t k = in->entry_off[g + 1] - in->entry_off[g];
        if (k < 0 || in->n_gw[g] < 0 || in->n_gw[g] > k) return phz_fail(ctx, PHZ_E_ARG, "phz_annot_pairs: entry_off / n_gw inconsistent");
    }
    for (int64_t e = 0; e < in->n_entries; e++)
        if (in->entry_var[e] < 0 || in->entry_var[e] >= in->n_vars) return phz_fail(ctx, PHZ_E_ARG, "phz_annot_pairs: entry_var out of range");
    for (int64_t i = 0; i < 2 * in->n_vars; i++)
        if (in->gw_allele[i] > 15 || in->pg_allele[i] > 15) return phz_fail(ctx, PHZ_E_ARG, "phz_annot_pairs: allele index above 15");
    // ---- tiles
    std::vector<int32_t> tile_gene; std::vector<int64_t> tile_start;
    std::vector<int64_t> gene_tile0((size_t)in->n_genes + 1);
    int64_t pairs = 0;
    for (int64_t g = 0; g < in->n_genes; g++) {
        gene_tile0[(size_t)g] = (int64_t)tile_gene.size();
        const int64_t n = in->n_gw[g], m = in->entry_off[g + 1] - in->entry_off[g] - n;
        for (int64_t p = 0; p < n * n; p += PHZ_ANNOT_TILE) { tile_gene.push_back((int32_t)g); tile_start.push_back(p); }
        for (int64_t p = 0; p < m * m; p += PHZ_ANNOT_TILE) { tile_gene.push_back((int32_t)g); tile_start.push_back(n * n + p); }
        pairs += n * n + m * m;
    }
    const int64_t n_tiles = (int64_t)tile_gene.size();
    gene_tile0[(size_t)in->n_genes] = n_tiles;
    if (n_pairs) *n_pairs = pairs;
    if (n_tiles == 0) return PHZ_OK;
    if (n_tiles >= (1ll << 31)) return phz_fail(ctx, PHZ_E_CAPACITY, "phz_annot_pairs: more than 2^31 tiles");
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t sm = ctx->stream;
    Staging st(ctx);
    AnnotArgs a;
    if (int s = st.in(in->entry_off, (size_t)in->n_genes + 1, PHZ_HOST, &a.entry_off)) return s;
    if (int s = st.in(in->n_gw, (size_t)in->n_genes, PHZ_HOST, &a.n_gw)) return s;
    if (int s = st.in(in->entry_var, (size_t)in->n_entries, PHZ_HOST, &a.entry_var)) return s;
    if (int s = st.in(in->entry_mask, (size_t)in->n_entries, PHZ_HOST, &a.entry_mask)) return s;
    if (int s = st.in(in->entry_flags, (size_t)in->n_entries, PHZ_HOST, &a.entry_flags)) return s;
    if (int s = st.in(in->gw_allele, (size_t)in->n_vars * 2, PHZ_HOST, &a.gw_allele)) return s;
    if (int s = st.in(in->pg_allele, (size_t)in->n_vars * 2, PHZ_HOST, &a.pg_allele)) return s;
    if (int s = st.in(in->gw_block, (size_t)in->n_vars, PHZ_HOST, &a.gw_block)) return s;
    if (int s = st.in(in->pg_block, (size_t)in->n_vars, PHZ_HOST, &a.pg_block)) return s;
    if (int s = st.in((const int32_t *)tile_gene.data(), (size_t)n_tiles, PHZ_HOST, &a.tile_gene)) return s;
    if (int s = st.in((const int64_t *)tile_start.data(), (size_t)n_tiles, PHZ_HOST, &a.tile_start)) return s;
    if (int s = phz_reserve(ctx, ctx->scratch[SC_ANNOT_COUNT], (size_t)n_tiles * 4)) return s;
    a.tile_count = (uint32_t *)ctx->scratch[SC_ANNOT_COUNT].p;
    a.tile_base = nullptr; a.out = nullptr; a.t0 = 0; a.b0 = 0;
    double total_ms = 0;
    auto elapsed = [&]() { float ms = 0; (void)hipEventSynchronize(ctx->ev1); (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1); total_ms += ms; };
    auto done = [&]() { ctx->last_ms[PHZ_T_ANNOT] = (float)total_ms; ctx->total_ms[PHZ_T_ANNOT] += total_ms; ctx->launches[PHZ_T_ANNOT]++; };
    // ---- pass 1: rows per tile
    (void)hipEventRecord(ctx->ev0, sm);
    for (a.b0 = 0; a.b0 < n_tiles; a.b0 += PHZ_ANNOT_GRID) {
        hipLaunchKernelGGL(k_annot<false>, dim3((unsigned)std::min<int64_t>(PHZ_ANNOT_GRID, n_tiles - a.b0)), dim3(THREADS), 0, sm, a);
        PHZ_HIP(ctx, hipGetLastError());
    }
    (void)hipEventRecord(ctx->ev1, sm);
    std::vector<uint32_t> count((size_t)n_tiles);
    PHZ_HIP(ctx, hipMemcpyAsync(count.data(), a.tile_count, (size_t)n_tiles * 4, hipMemcpyDeviceToHost, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    elapsed();
    std::vector<int64_t> gene_rows((size_t)in->n_genes, 0);
    int64_t total = 0;
    for (int64_t g = 0; g < in->n_genes; g++) {
        int64_t r = 0;
        for (int64_t t = gene_tile0[(size_t)g]; t < gene_tile0[(size_t)g + 1]; t++) r += count[(size_t)t];
        gene_rows[(size_t)g] = r; total += r;
        if (r > batch_rows) {
            done();
            char msg[160];
            snprintf(msg, sizeof msg, "phz_annot_pairs: gene %lld alone has %lld rows, the batch capacity is %lld", (long long)g, (long long)r, (long long)batch_rows);
            return phz_fail(ctx, PHZ_E_CAPACITY, msg);
        }
    }
    *n_rows = total;
    if (!rows) { done(); return PHZ_OK; }
    if (rows_cap < total) { done(); return phz_fail(ctx, PHZ_E_ARG, "phz_annot_pairs: rows_cap is smaller than the row count"); }
    // ---- pass 2, gene ranges of at most batch_rows records
    int32_t batches = 0;
    int64_t written = 0;
    for (int64_t g0 = 0; g0 < in->n_genes;) {
        int64_t g1 = g0, r = 0;
        while (g1 < in->n_genes && r + gene_rows[(size_t)g1] <= batch_rows) r += gene_rows[(size_t)g1++];
        const int64_t t0 = gene_tile0[(size_t)g0], nt = gene_tile0[(size_t)g1] - t0;
        if (r > 0 && nt > 0) {
            if (int s = phz_reserve(ctx, ctx->scratch[SC_ANNOT_BASE], (size_t)(nt + 1) * 4)) return s;
            if (int s = phz_reserve(ctx, ctx->scratch[SC_ANNOT_OUT], (size_t)r * sizeof(uint4))) return s;
            a.t0 = t0; a.tile_base = (const uint32_t *)ctx->scratch[SC_ANNOT_BASE].p; a.out = (uint4 *)ctx->scratch[SC_ANNOT_OUT].p;
            (void)hipEventRecord(ctx->ev0, sm);
            // (a batch starts at any tile: the scan's input pointer is 16-byte aligned or not as t0 falls, gscan_excl takes either)
            if (int s = gscan_excl<uint32_t, uint32_t>(ctx, a.tile_count + t0, (uint32_t *)ctx->scratch[SC_ANNOT_BASE].p, nt, ctx->scratch[SC_ANNOT_SCAN_TMP])) return s;
            for (a.b0 = 0; a.b0 < nt; a.b0 += PHZ_ANNOT_GRID) {
                hipLaunchKernelGGL(k_annot<true>, dim3((unsigned)std::min<int64_t>(PHZ_ANNOT_GRID, nt - a.b0)), dim3(THREADS), 0, sm, a);
                PHZ_HIP(ctx, hipGetLastError());
            }
            (void)hipEventRecord(ctx->ev1, sm);
            PHZ_HIP(ctx, hipMemcpyAsync(rows + written, a.out, (size_t)r * sizeof(uint4), hipMemcpyDeviceToHost, sm));
            PHZ_HIP(ctx, hipStreamSynchronize(sm));
            elapsed();
            written += r; batches++;
        }
        g0 = g1;
    }
    done();
    if (n_batches) *n_batches = batches;
    return PHZ_OK;
}
