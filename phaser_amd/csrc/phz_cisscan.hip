// K_cisscan: ASE-based cis mapping (phaser_amd/cis_scan.py; include/phz.h, phz_cis_scan).  For every gene, every variant of its window is tested: do the
// heterozygotes of the variant show a larger |aFC| of the gene than its homozygotes?  Everything here is integer work.
//
// A gene's covered samples are given in ascending |aFC| order (order[p] = the sample at sorted position p) with the tie run [run_first[p], run_last[p]] of every
// position.  With H(x) = the number of hom samples at positions < x, the rank-sum count of a (gene, variant) pair is
//     U2 = sum over (het i, hom j) of 2 [|aFC_i| > |aFC_j|] + [|aFC_i| = |aFC_j|] = sum over het positions p of H(run_first[p]) + H(run_last[p] + 1),
// D = U2 - n_het n_hom and T = D^2 / (n_het n_hom (n_het + n_hom + 1)) (3 z^2 of the rank-sum test).  Two T are compared exactly, as rationals, by a 128-bit cross
// product: D^2 <= 2^44 and the denominator < 2^35 at S = 4096.
//
// The walk (one wave, one variant): the lanes take the sorted positions 64 at a time and gather the class of the sample there; two ballots give the chunk's hom
// and het masks, kept in a per-wave LDS table beside the running hom count of the chunk's start, so H(x) is one table read and one popcount.  A second sweep
// adds H(run_first) + H(run_last + 1) over the het positions and a butterfly sums the lanes.
//
// k_cisscan_obs   one wave per (gene, variant) pair, grid-stride: n_het, n_hom, U2 of the observed order.
// k_cisscan_best  one wave per gene: the testable variant with the largest T, the first among equals; its (D^2, denominator) stays on the device for the
//                 permutation pass.
// k_cisscan_perm  one workgroup per (gene, slice of PHZ_CISSCAN_RPS replicates), grid-stride.  Replicate b permutes which sample holds which position: the keys
//                 (w(b, i) << 32 | i), i < n, are sorted by a bitonic network in LDS (padded with all-ones keys to a power of two) and position p is then held
//                 by sample covered[low half of key p]; tie runs stay on positions, genotypes on samples.  The waves split the gene's variants, skip the ones that
//                 are not testable (n_het and n_hom do not change under permutation: both come from the first pass) and keep the largest (D^2, denominator);
//                 thread 0 combines the waves and counts the replicate when its maximum reaches the observed T.  One atomicAdd per slice.
//
// Stream (a contract: tests/cis_scan_restatement.py replays it): w(b, i) is word (b n + i) mod 4 of Philox4x32-10 at counter {lo(q), hi(q), lo(s), hi(s)},
// q = (b n + i) / 4, s = subseq[g], key {lo(seed), hi(seed)}: K_boot's indexing (phz_cisvar.hip).
//
// LDS of k_cisscan_perm at S = 4096: 32 KiB of keys + 8 KiB of samples + 8 x 1,288 B of walk tables + 128 B = 51,392 B, three workgroups per CU
// (profiles/r20/cis_scan_resources.txt).
#include <hip/hip_runtime.h>

#include <vector>

#include "phz.h"
#include "phz_internal.h"

#ifndef PHZ_CISSCAN_GRID
#define PHZ_CISSCAN_GRID 4096       // most workgroups of a launch; the kernels stride over their work beyond it
#endif
#ifndef PHZ_CISSCAN_RPS
#define PHZ_CISSCAN_RPS 8           // replicates of one (gene, slice) work item of k_cisscan_perm
#endif

namespace {

constexpr int MAX_S = PHZ_CISSCAN_MAX_S;
constexpr int MAX_CHUNKS = MAX_S / 64;
constexpr int OBS_WAVES = 4, PERM_WAVES = 8;
constexpr int PERM_THREADS = PERM_WAVES * 64;

typedef unsigned __int128 u128;

struct ScanArgs {
    int64_t n_genes, n_vars, n_pairs;
    int32_t S, min_het, min_hom, n_perm;
    uint64_t seed;
    const uint8_t *cls;
    const int64_t *g_off, *v_lo, *pair_off;
    const uint16_t *covered, *order, *run_first, *run_last;
    const uint64_t *subseq;
    int32_t *n_het, *n_hom, *best_v, *exceed;
    int64_t *u2;
    uint64_t *obs_d2, *obs_den;      // per gene: D^2 and denominator of the best variant
};

struct WalkTab {                     // one wave's tables of the variant it walks
    unsigned long long hom[MAX_CHUNKS], het[MAX_CHUNKS];
    uint32_t pref[MAX_CHUNKS + 1];   // hom samples before the chunk; pref[chunks] = all
};

struct Quad { uint32_t w[4]; };

__device__ __forceinline__ Quad philox4x32_10(uint64_t q, uint64_t s, uint64_t seed) {
    uint32_t c0 = (uint32_t)q, c1 = (uint32_t)(q >> 32), c2 = (uint32_t)s, c3 = (uint32_t)(s >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)m1; c2 = n2; c3 = (uint32_t)m0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Quad o; o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// T = d2 / den of a pair; den > 0 for a testable one
__device__ __forceinline__ uint64_t den_of(uint32_t n1, uint32_t n2) { return (uint64_t)n1 * n2 * ((uint64_t)n1 + n2 + 1); }
__device__ __forceinline__ uint64_t d2_of(uint32_t u2, uint32_t n1, uint32_t n2) {
    const int64_t d = (int64_t)u2 - (int64_t)n1 * (int64_t)n2;
    return (uint64_t)(d * d);
}
__device__ __forceinline__ bool t_greater(uint64_t d2a, uint64_t dena, uint64_t d2b, uint64_t denb) { return (u128)d2a * denb > (u128)d2b * dena; }
__device__ __forceinline__ bool t_at_least(uint64_t d2a, uint64_t dena, uint64_t d2b, uint64_t denb) { return (u128)d2a * denb >= (u128)d2b * dena; }

__device__ __forceinline__ uint32_t hom_before(const WalkTab &t, int x) {
    const int c = x >> 6, r = x & 63;
    return t.pref[c] + (r ? (uint32_t)__popcll(t.hom[c] & ((1ull << r) - 1)) : 0u);
}

// One wave, one variant: samp[p] = the sample at sorted position p (p < n), row = the variant's classes.  -> U2 in every lane; *n_het, *n_hom.
// Indices are clamped (a PHZ_DEVICE caller's arrays are not checked): no read leaves the class row or the tables.
__device__ __forceinline__ uint32_t walk(const uint8_t *row, int S, const uint16_t *samp, const uint16_t *rf, const uint16_t *rl, int n, WalkTab &t, int lane,
                                         uint32_t *n_het, uint32_t *n_hom) {
    const int chunks = (n + 63) >> 6;
    uint32_t H = 0, E = 0;
    for (int c = 0; c < chunks; c++) {
        const int p = c * 64 + lane;
        const int cl = p < n ? row[min((int)samp[p], S - 1)] : 0;
        const unsigned long long hom = __ballot(cl == 2), het = __ballot(cl == 1);
        if (lane == 0) { t.hom[c] = hom; t.het[c] = het; t.pref[c] = H; }
        H += (uint32_t)__popcll(hom); E += (uint32_t)__popcll(het);
    }
    if (lane == 0) t.pref[chunks] = H;
    __builtin_amdgcn_wave_barrier();
    uint32_t acc = 0;
    if (H && E)
        for (int c = 0; c < chunks; c++) {
            const int p = c * 64 + lane;
            if (p < n && ((t.het[c] >> lane) & 1)) acc += hom_before(t, min((int)rf[p], n)) + hom_before(t, min((int)rl[p] + 1, n));
        }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
    __builtin_amdgcn_wave_barrier();                    // the tables are rewritten by the next variant
    *n_het = E; *n_hom = H;
    return acc;
}

__device__ __forceinline__ int64_t gene_of_pair(const int64_t *pair_off, int64_t n_genes, int64_t k) {
    int64_t lo = 0, hi = n_genes;                      // the last g with pair_off[g] <= k
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pair_off[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(OBS_WAVES * 64) void k_cisscan_obs(ScanArgs a) {
    __shared__ WalkTab s_tab[OBS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t k = (int64_t)blockIdx.x * OBS_WAVES + wave; k < a.n_pairs; k += (int64_t)gridDim.x * OBS_WAVES) {
        const int64_t g = gene_of_pair(a.pair_off, a.n_genes, k);
        const int64_t v = a.v_lo[g] + (k - a.pair_off[g]);
        const int64_t o = a.g_off[g];
        const int n = (int)(a.g_off[g + 1] - o);
        uint32_t n1, n2;
        const uint32_t u = walk(a.cls + v * a.S, a.S, a.order + o, a.run_first + o, a.run_last + o, n, s_tab[wave], lane, &n1, &n2);
        if (lane == 0) { a.n_het[k] = (int32_t)n1; a.n_hom[k] = (int32_t)n2; a.u2[k] = (int64_t)u; }
    }
}

__global__ __launch_bounds__(OBS_WAVES * 64) void k_cisscan_best(ScanArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t g = (int64_t)blockIdx.x * OBS_WAVES + wave; g < a.n_genes; g += (int64_t)gridDim.x * OBS_WAVES) {
        const int64_t k0 = a.pair_off[g], nv = a.pair_off[g + 1] - k0;
        uint64_t bd2 = 0, bden = 1;
        int64_t bi = -1;                               // pair position inside the gene
        for (int64_t i = lane; i < nv; i += 64) {
            const uint32_t n1 = (uint32_t)a.n_het[k0 + i], n2 = (uint32_t)a.n_hom[k0 + i];
            if ((int32_t)n1 < a.min_het || (int32_t)n2 < a.min_hom) continue;
            const uint64_t d2 = d2_of((uint32_t)a.u2[k0 + i], n1, n2), den = den_of(n1, n2);
            if (bi < 0 || t_greater(d2, den, bd2, bden)) { bd2 = d2; bden = den; bi = i; }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint64_t od2 = __shfl_xor(bd2, d), oden = __shfl_xor(bden, d);
            const int64_t oi = __shfl_xor(bi, d);
            if (oi >= 0 && (bi < 0 || t_greater(od2, oden, bd2, bden) || (oi < bi && !t_greater(bd2, bden, od2, oden)))) { bd2 = od2; bden = oden; bi = oi; }
        }
        if (lane == 0) {
            a.best_v[g] = bi < 0 ? -1 : (int32_t)(a.v_lo[g] + bi);
            a.obs_d2[g] = bd2; a.obs_den[g] = bden;
        }
    }
}

__global__ __launch_bounds__(PERM_THREADS) void k_cisscan_perm(ScanArgs a, int slices) {
    __shared__ unsigned long long s_key[MAX_S];
    __shared__ uint16_t s_samp[MAX_S];
    __shared__ WalkTab s_tab[PERM_WAVES];
    __shared__ unsigned long long s_wd2[PERM_WAVES], s_wden[PERM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t item = blockIdx.x; item < a.n_genes * slices; item += gridDim.x) {
        const int64_t g = item / slices;
        if (a.best_v[g] < 0) continue;                 // no testable pair: exceed stays 0
        const int b0 = (int)(item % slices) * PHZ_CISSCAN_RPS, b1 = min(a.n_perm, b0 + PHZ_CISSCAN_RPS);
        const int64_t o = a.g_off[g], k0 = a.pair_off[g];
        const int n = (int)(a.g_off[g + 1] - o), nv = (int)(a.pair_off[g + 1] - k0);
        const int64_t v0 = a.v_lo[g];
        const uint64_t sub = a.subseq[g], od2 = a.obs_d2[g], oden = a.obs_den[g];
        int N = 2;
        while (N < n) N <<= 1;
        int count = 0;
        for (int b = b0; b < b1; b++) {
            // ---- keys of the replicate, padded
            const uint64_t base = (uint64_t)b * (uint64_t)n, end = base + (uint64_t)n;
            for (uint64_t q = (base >> 2) + tid; 4 * q < end; q += PERM_THREADS) {
                const Quad w = philox4x32_10(q, sub, a.seed);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint64_t at = 4 * q + i;
                    if (at >= base && at < end) s_key[at - base] = ((unsigned long long)w.w[i] << 32) | (unsigned long long)(at - base);
                }
            }
            for (int i = n + tid; i < N; i += PERM_THREADS) s_key[i] = ~0ull;
            __syncthreads();
            // ---- bitonic sort, ascending.  Compare-exchange t (pairs i, i | j) belongs to thread t mod PERM_THREADS, so the 64 exchanges of a wave's round stay
            // inside one block of 128 keys while j <= 64: those steps need no workgroup barrier, only the wave's own order (63 of the 78 steps at N = 4096)
            const bool wave_has_work = (wave << 6) < (N >> 1);
            for (int k = 2; k <= N; k <<= 1) {
                if ((k >> 1) > 64) __syncthreads();         // the phase before ended in wave-local steps
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < (N >> 1); t += PERM_THREADS) {
                        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), x = i | j;
                        const unsigned long long p = s_key[i], r = s_key[x];
                        if ((p > r) == ((i & k) == 0)) { s_key[i] = r; s_key[x] = p; }
                    }
                    if (j > 64) __syncthreads();
                    else if (wave_has_work) __builtin_amdgcn_wave_barrier();
                }
            }
            __syncthreads();
            for (int p = tid; p < n; p += PERM_THREADS) s_samp[p] = a.covered[o + (int64_t)min((uint32_t)s_key[p], (uint32_t)(n - 1))];
            __syncthreads();
            // ---- the waves split the variants
            uint64_t md2 = 0, mden = 1;
            for (int i = wave; i < nv; i += PERM_WAVES) {
                const uint32_t n1 = (uint32_t)a.n_het[k0 + i], n2 = (uint32_t)a.n_hom[k0 + i];
                if ((int32_t)n1 < a.min_het || (int32_t)n2 < a.min_hom) continue;
                uint32_t e, h;
                const uint32_t u = walk(a.cls + (v0 + i) * a.S, a.S, s_samp, a.run_first + o, a.run_last + o, n, s_tab[wave], lane, &e, &h);
                const uint64_t d2 = d2_of(u, n1, n2), den = den_of(n1, n2);
                if (t_greater(d2, den, md2, mden)) { md2 = d2; mden = den; }
            }
            if (lane == 0) { s_wd2[wave] = md2; s_wden[wave] = mden; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < PERM_WAVES; w++)
                    if (t_greater(s_wd2[w], s_wden[w], md2, mden)) { md2 = s_wd2[w]; mden = s_wden[w]; }
                count += t_at_least(md2, mden, od2, oden);
            }
            // s_key is rewritten before the next barrier, s_wd2 only after it: both were read before this point or by thread 0 alone
        }
        if (tid == 0 && count) atomicAdd(&a.exceed[g], count);
        __syncthreads();
    }
}

int bad(phz_ctx *ctx, const char *what) { return phz_fail(ctx, PHZ_E_ARG, what); }

}  // namespace

extern "C" int phz_cis_scan(phz_ctx *ctx, const phz_cisscan_in *in, int32_t *n_het, int32_t *n_hom, int64_t *u2, int32_t *best_v, int32_t *exceed, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !in || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    if (in->n_genes < 0 || in->n_vars < 0 || in->n_samples < 0) return bad(ctx, "phz_cis_scan: negative size");
    if (in->n_perm < 0) return bad(ctx, "phz_cis_scan: negative n_perm");
    if (in->min_het < 1 || in->min_hom < 1) return bad(ctx, "phz_cis_scan: min_het and min_hom must be at least 1");
    if (in->n_samples > PHZ_CISSCAN_MAX_S) return phz_fail(ctx, PHZ_E_UNSUPPORTED, "phz_cis_scan: more than PHZ_CISSCAN_MAX_S samples");
    if (in->n_genes > 0x7FFFFFFF) return bad(ctx, "phz_cis_scan: more than 2^31 - 1 genes");
    const int64_t G = in->n_genes, V = in->n_vars;
    const int S = in->n_samples;
    if (G == 0) return PHZ_OK;
    if (!in->g_off || !in->v_lo || !in->v_hi || !in->subseq || !best_v || !exceed) return bad(ctx, "phz_cis_scan: a per-gene array is missing");
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t sm = ctx->stream;
    // ---- the per-gene tables are read on the host in either space: they size the outputs
    std::vector<int64_t> h_goff((size_t)G + 1), h_vlo((size_t)G), h_vhi((size_t)G), pair_off((size_t)G + 1);
    const int64_t *goff = in->g_off, *vlo = in->v_lo, *vhi = in->v_hi;
    if (space == PHZ_DEVICE) {
        PHZ_HIP(ctx, hipMemcpyAsync(h_goff.data(), in->g_off, ((size_t)G + 1) * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(h_vlo.data(), in->v_lo, (size_t)G * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(h_vhi.data(), in->v_hi, (size_t)G * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        goff = h_goff.data(); vlo = h_vlo.data(); vhi = h_vhi.data();
    }
    if (goff[0] < 0) return bad(ctx, "phz_cis_scan: offsets not ascending");
    pair_off[0] = 0;
    for (int64_t g = 0; g < G; g++) {
        const int64_t n = goff[g + 1] - goff[g];
        if (n < 0) return bad(ctx, "phz_cis_scan: offsets not ascending");
        if (n > S) return bad(ctx, "phz_cis_scan: a gene holds more samples than n_samples");
        if (vlo[g] < 0 || vhi[g] < vlo[g] || vhi[g] > V) return bad(ctx, "phz_cis_scan: variant range outside [0, n_vars]");
        pair_off[(size_t)g + 1] = pair_off[(size_t)g] + (vhi[g] - vlo[g]);
        if (pair_off[(size_t)g + 1] > 0x7FFFFFFFll) return bad(ctx, "phz_cis_scan: more than 2^31 - 1 pairs");
    }
    const int64_t total = goff[G], n_pairs = pair_off[(size_t)G];
    if (total && (!in->covered || !in->order || !in->run_first || !in->run_last)) return bad(ctx, "phz_cis_scan: a per-position array is missing");
    if (n_pairs && (!in->cls || !n_het || !n_hom || !u2)) return bad(ctx, "phz_cis_scan: a per-pair array is missing");
    if (space == PHZ_HOST) {
        for (int64_t i = 0; i < V * (int64_t)S; i++)
            if (in->cls[i] > 2) return bad(ctx, "phz_cis_scan: a class above 2");
        for (int64_t g = 0; g < G; g++) {
            const int64_t o = goff[g], n = goff[g + 1] - o;
            const uint16_t *rf = in->run_first + o, *rl = in->run_last + o;
            for (int64_t p = 0; p < n; p++) {
                if (in->covered[o + p] >= S || in->order[o + p] >= S) return bad(ctx, "phz_cis_scan: a sample index >= n_samples");
                const bool ok = rf[p] == p ? ((p == 0 || rl[p - 1] == p - 1) && rl[p] >= p && rl[p] < n)
                                           : (p > 0 && rf[p] == rf[p - 1] && rl[p] == rl[p - 1] && p <= rl[p]);
                if (!ok) return bad(ctx, "phz_cis_scan: run bounds that are not runs");
            }
        }
    }
    // ---- staging
    Staging st(ctx);
    ScanArgs a;
    a.n_genes = G; a.n_vars = V; a.n_pairs = n_pairs; a.S = S; a.min_het = in->min_het; a.min_hom = in->min_hom; a.n_perm = in->n_perm; a.seed = in->seed;
    if (int s = st.in(in->cls, (size_t)V * (size_t)S, space, &a.cls)) return s;
    if (int s = st.in(in->g_off, (size_t)G + 1, space, &a.g_off)) return s;
    if (int s = st.in(in->v_lo, (size_t)G, space, &a.v_lo)) return s;
    if (int s = st.in(in->subseq, (size_t)G, space, &a.subseq)) return s;
    if (int s = st.in(in->covered, (size_t)total, space, &a.covered)) return s;
    if (int s = st.in(in->order, (size_t)total, space, &a.order)) return s;
    if (int s = st.in(in->run_first, (size_t)total, space, &a.run_first)) return s;
    if (int s = st.in(in->run_last, (size_t)total, space, &a.run_last)) return s;
    if (int s = st.in((const int64_t *)pair_off.data(), (size_t)G + 1, PHZ_HOST, &a.pair_off)) return s;
    if (int s = st.out(n_het, (size_t)n_pairs, space, &a.n_het)) return s;
    if (int s = st.out(n_hom, (size_t)n_pairs, space, &a.n_hom)) return s;
    if (int s = st.out(u2, (size_t)n_pairs, space, &a.u2)) return s;
    if (int s = st.out(best_v, (size_t)G, space, &a.best_v)) return s;
    if (int s = st.out(exceed, (size_t)G, space, &a.exceed)) return s;
    void *d = nullptr;
    if (int s = st.slot((size_t)G * 8, &d)) return s;
    a.obs_d2 = (uint64_t *)d;
    if (int s = st.slot((size_t)G * 8, &d)) return s;
    a.obs_den = (uint64_t *)d;
    PHZ_HIP(ctx, hipMemsetAsync(a.exceed, 0, (size_t)G * 4, sm));
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_CISSCAN times the three kernels
    auto grid_of = [](int64_t items) { return (unsigned)(items < PHZ_CISSCAN_GRID ? (items < 1 ? 1 : items) : PHZ_CISSCAN_GRID); };
    if (n_pairs) {
        hipLaunchKernelGGL(k_cisscan_obs, dim3(grid_of((n_pairs + OBS_WAVES - 1) / OBS_WAVES)), dim3(OBS_WAVES * 64), 0, sm, a);
        PHZ_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_cisscan_best, dim3(grid_of((G + OBS_WAVES - 1) / OBS_WAVES)), dim3(OBS_WAVES * 64), 0, sm, a);
    PHZ_HIP(ctx, hipGetLastError());
    if (in->n_perm > 0 && n_pairs) {
        const int slices = (in->n_perm + PHZ_CISSCAN_RPS - 1) / PHZ_CISSCAN_RPS;
        hipLaunchKernelGGL(k_cisscan_perm, dim3(grid_of(G * slices)), dim3(PERM_THREADS), 0, sm, a, slices);
        PHZ_HIP(ctx, hipGetLastError());
    }
    (void)hipEventRecord(ctx->ev1, sm);
    (void)hipEventSynchronize(ctx->ev1);
    float ms = 0; (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->last_ms[PHZ_T_CISSCAN] = ms; ctx->total_ms[PHZ_T_CISSCAN] += ms; ctx->launches[PHZ_T_CISSCAN]++;
    if (space == PHZ_HOST) {
        if (n_pairs) {
            PHZ_HIP(ctx, hipMemcpyAsync(n_het, a.n_het, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, sm));
            PHZ_HIP(ctx, hipMemcpyAsync(n_hom, a.n_hom, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, sm));
            PHZ_HIP(ctx, hipMemcpyAsync(u2, a.u2, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, sm));
        }
        PHZ_HIP(ctx, hipMemcpyAsync(best_v, a.best_v, (size_t)G * 4, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(exceed, a.exceed, (size_t)G * 4, hipMemcpyDeviceToHost, sm));
    }
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}
