// K_match: the sums of phaser_sample_match (include/phz.h, phz_sample_match; DESIGN.md, "phaser_sample_match and K_match").
// The reference has no such tool.  For every (sample, donor) the log-likelihood of the sample's allele counts under the donor's genotypes, the number of
// the sample's sites the donor is called at, and the number of those at which the class the counts show equals the donor's genotype.
//
// Per entry (site, ref, alt) of a sample, from the inputs alone:
//   total = ref + alt (int64); cap > 0 and total > cap: r = (ref cap + total / 2) / total (floor), a = cap - r; else r = ref, a = alt
//   t_g = fma((double)r, log_ref[g-1], (double)a * log_alt[g-1]) for g = 1, 2, 3: one rounded product and one fused multiply-add, written with fma(), so the
//         compiler's contraction setting cannot change a bit
//   obs = 2 when 1000 min(ref, alt) >= het_permille total (int64), else 1 when ref > alt, else 3
// Per (sample, donor), over the sample's entries in entry order with g = the donor's code at the entry's site: g = 0 adds nothing, otherwise
//   loglik += t_g (one fp64 add, sequentially, from +0.0), n_called += 1, n_match += (g == obs).
// No tree, no atomics: a result depends on its sample's entries and its donor's codes, not on the grid or on what else is in the call.
//
// k_match_pack   one thread per word: the codes of 16 donors at a site as 2 bits each, words[site * W + (d >> 4)], W = ceil(n_donors / 16); donors beyond
//                n_donors are 0.
// k_match        one workgroup of 256 threads per work item (sample, block of 256 donors), grid-stride over at most PHZ_MATCH_GRID workgroups; lane = donor,
//                the three accumulators in registers.  The sample's entries pass through LDS in tiles of PHZ_MATCH_TILE: thread i computes entry i's
//                (site, t_1, t_2, t_3, obs) once; after a barrier every thread walks the tile in order, reading the entry at the same LDS address in all lanes
//                (a broadcast) and its donor's word (the 64 lanes of a wave touch 4 consecutive dwords); a second barrier precedes the next staging, of this
//                work item or of the workgroup's next.  An entry that is out of range (PHZ_DEVICE inputs; host inputs are refused) is staged as "skip".
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "phz.h"
#include "phz_internal.h"

#ifndef PHZ_MATCH_GRID
#define PHZ_MATCH_GRID 8192         // most workgroups of k_match (grid-stride beyond)
#endif
#ifndef PHZ_MATCH_TILE
#define PHZ_MATCH_TILE 256          // entries staged through LDS at a time, 1..256
#endif
static_assert(PHZ_MATCH_TILE >= 1 && PHZ_MATCH_TILE <= 256, "a tile is staged by one thread per entry of a 256-thread workgroup");
static_assert(PHZ_MATCH_GRID >= 1, "at least one workgroup");

namespace {

constexpr int THREADS = 256;
constexpr int TILE = PHZ_MATCH_TILE;
constexpr int BATCH = 8;            // words a thread has in flight before it adds their terms, in entry order

struct MatchArgs {
    int64_t n_sites, n_samples, n_items;          // n_items = n_samples * n_dblk work items
    int32_t n_donors, n_dblk, W;                  // blocks of 256 donors, words per site
    const uint8_t *geno;
    const int64_t *e_off;
    const int32_t *e_site, *e_ref, *e_alt;
    double lr1, lr2, lr3, la1, la2, la3;
    int32_t cap, het_permille;
    uint32_t *words;
    double *loglik;
    int32_t *n_called, *n_match;
};

__global__ __launch_bounds__(THREADS) void k_match_pack(MatchArgs g) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t >= g.n_sites * g.W) return;
    const int64_t site = t / g.W;
    const int32_t d0 = (int32_t)(t % g.W) * 16;
    const uint8_t *row = g.geno + site * g.n_donors;
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 16; k++)
        if (d0 + k < g.n_donors) w |= (uint32_t)(row[d0 + k] & 3u) << (2 * k);
    g.words[t] = w;
}

__global__ __launch_bounds__(THREADS) void k_match(MatchArgs g) {
    __shared__ double s_t1[TILE], s_t2[TILE], s_t3[TILE];
    __shared__ int32_t s_site[TILE], s_obs[TILE];          // site -1: the entry is skipped
    const int tid = (int)threadIdx.x;
    for (int64_t item = blockIdx.x; item < g.n_items; item += gridDim.x) {
        const int64_t s = item / g.n_dblk;
        const int32_t d = (int32_t)(item % g.n_dblk) * THREADS + tid;
        const bool live = d < g.n_donors;
        const uint32_t *col = g.words + (live ? d >> 4 : 0);
        const int shift = (d & 15) * 2;
        double ll = 0.0;
        int32_t nc = 0, nm = 0;
        const int64_t e0 = g.e_off[s], e1 = g.e_off[s + 1];
        for (int64_t base = e0; base < e1; base += TILE) {
            const int n = (int)(e1 - base < TILE ? e1 - base : TILE);
            if (tid < n) {
                const int64_t site = g.e_site[base + tid], ref = g.e_ref[base + tid], alt = g.e_alt[base + tid], total = ref + alt;
                if (site < 0 || site >= g.n_sites || ref < 0 || alt < 0 || total == 0) {
                    s_site[tid] = -1;
                } else {
                    int64_t r = ref, a = alt;
                    if (g.cap > 0 && total > g.cap) { r = (ref * g.cap + total / 2) / total; a = g.cap - r; }
                    s_t1[tid] = fma((double)r, g.lr1, (double)a * g.la1);
                    s_t2[tid] = fma((double)r, g.lr2, (double)a * g.la2);
                    s_t3[tid] = fma((double)r, g.lr3, (double)a * g.la3);
                    const int64_t m = ref < alt ? ref : alt;
                    s_obs[tid] = 1000 * m >= (int64_t)g.het_permille * total ? 2 : (ref > alt ? 1 : 3);
                    s_site[tid] = (int32_t)site;
                }
            }
            __syncthreads();
            for (int i0 = 0; i0 < n; i0 += BATCH) {
                uint32_t code[BATCH];
#pragma unroll
                for (int k = 0; k < BATCH; k++) {
                    const int i = i0 + k;
                    const int32_t site = i < n ? s_site[i] : -1;
                    code[k] = live && site >= 0 ? (col[(int64_t)site * g.W] >> shift) & 3u : 0u;
                }
#pragma unroll
                for (int k = 0; k < BATCH; k++) {
                    if (code[k] == 0) continue;          // a code is non-zero only for i < n
                    const int i = i0 + k;
                    ll += code[k] == 1 ? s_t1[i] : (code[k] == 2 ? s_t2[i] : s_t3[i]);
                    nc++;
                    nm += (int32_t)code[k] == s_obs[i];
                }
            }
            __syncthreads();          // the tile has been walked by every thread: it may be staged again, by this work item or the next
        }
        if (live) {
            const int64_t o = s * g.n_donors + d;
            g.loglik[o] = ll; g.n_called[o] = nc; g.n_match[o] = nm;
        }
    }
}

void record_ms(phz_ctx *ctx, int slot) {
    (void)hipEventSynchronize(ctx->ev1);
    float ms = 0; (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->last_ms[slot] = ms; ctx->total_ms[slot] += ms; ctx->launches[slot]++;
}

}  // namespace

extern "C" int phz_sample_match(phz_ctx *ctx, const phz_match_in *in, double *loglik, int32_t *n_called, int32_t *n_match, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !in || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    if (in->n_sites < 0 || in->n_samples < 0) return PHZ_E_ARG;
    if (in->n_donors < 1) return phz_fail(ctx, PHZ_E_ARG, "phz_sample_match: n_donors must be at least 1");
    if (in->het_permille < 1 || in->het_permille > 500) return phz_fail(ctx, PHZ_E_ARG, "phz_sample_match: het_permille must lie between 1 and 500");
    if (in->cap < 0) return phz_fail(ctx, PHZ_E_ARG, "phz_sample_match: cap must not be negative");
    if (in->n_sites > INT32_MAX) return phz_fail(ctx, PHZ_E_ARG, "phz_sample_match: more than 2^31 - 1 sites");          // e_site is int32
    if (in->n_samples == 0) return PHZ_OK;
    if (!in->e_off || !loglik || !n_called || !n_match || (in->n_sites && !in->geno)) return PHZ_E_ARG;
    int64_t n_entries = 0;          // PHZ_DEVICE: the offsets are the caller's guarantee and nothing is copied, the count is not needed
    if (space == PHZ_HOST) {
        if (in->e_off[0] != 0) return phz_fail(ctx, PHZ_E_ARG, "phz_sample_match: e_off does not start at 0");
        for (int64_t s = 0; s < in->n_samples; s++)
            if (in->e_off[s + 1] < in->e_off[s]) return phz_fail(ctx, PHZ_E_ARG, "phz_sample_match: e_off is not ascending");
        n_entries = in->e_off[in->n_samples];
        if (n_entries && (!in->e_site || !in->e_ref || !in->e_alt)) return PHZ_E_ARG;
        for (int64_t e = 0; e < n_entries; e++)
            if (in->e_site[e] < 0 || in->e_site[e] >= in->n_sites || in->e_ref[e] < 0 || in->e_alt[e] < 0 || (int64_t)in->e_ref[e] + in->e_alt[e] == 0)
                return phz_fail(ctx, PHZ_E_ARG, "phz_sample_match: an entry with a site out of range, a negative count or no read");
    }
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    MatchArgs g;
    g.n_sites = in->n_sites; g.n_samples = in->n_samples; g.n_donors = in->n_donors;
    g.n_dblk = (in->n_donors + THREADS - 1) / THREADS; g.W = (in->n_donors + 15) / 16;
    g.n_items = in->n_samples * g.n_dblk;
    g.lr1 = in->log_ref[0]; g.lr2 = in->log_ref[1]; g.lr3 = in->log_ref[2]; g.la1 = in->log_alt[0]; g.la2 = in->log_alt[1]; g.la3 = in->log_alt[2];
    g.cap = in->cap; g.het_permille = in->het_permille;
    const size_t n_out = (size_t)in->n_samples * (size_t)in->n_donors, n_words = (size_t)in->n_sites * (size_t)g.W;
    if (int s = st.in(in->geno, (size_t)in->n_sites * (size_t)in->n_donors, space, &g.geno)) return s;
    if (int s = st.in(in->e_off, (size_t)in->n_samples + 1, space, &g.e_off)) return s;
    if (int s = st.in(in->e_site, (size_t)n_entries, space, &g.e_site)) return s;
    if (int s = st.in(in->e_ref, (size_t)n_entries, space, &g.e_ref)) return s;
    if (int s = st.in(in->e_alt, (size_t)n_entries, space, &g.e_alt)) return s;
    if (int s = st.out(loglik, n_out, space, &g.loglik)) return s;
    if (int s = st.out(n_called, n_out, space, &g.n_called)) return s;
    if (int s = st.out(n_match, n_out, space, &g.n_match)) return s;
    DevBuf *S = ctx->scratch;
    if (int s = phz_reserve(ctx, S[SC_MATCH_WORDS], (n_words ? n_words : 1) * 4)) return s;
    g.words = (uint32_t *)S[SC_MATCH_WORDS].p;
    hipStream_t sm = ctx->stream;
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_MATCH: the packing and the sums
    if (n_words) hipLaunchKernelGGL(k_match_pack, dim3((unsigned)(((int64_t)n_words + THREADS - 1) / THREADS)), dim3(THREADS), 0, sm, g);
    hipLaunchKernelGGL(k_match, dim3((unsigned)std::min<int64_t>(g.n_items, (int64_t)PHZ_MATCH_GRID)), dim3(THREADS), 0, sm, g);
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    record_ms(ctx, PHZ_T_MATCH);
    if (space == PHZ_HOST) {
        PHZ_HIP(ctx, hipMemcpyAsync(loglik, g.loglik, n_out * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(n_called, g.n_called, n_out * 4, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(n_match, g.n_match, n_out * 4, hipMemcpyDeviceToHost, sm));
    }
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}
