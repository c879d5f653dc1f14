// K_boot: the bootstrap confidence intervals of phaser_cis_var (phaser_pop/phaser_cis_var.py:166-171, :202-219) for every group of a run in
// one launch (include/phz.h, phz_bootstrap_medians).  A group is the het or the hom sample set of one (pair row, VCF record); its signed aFC set
// and its |aFC| set share the resamples (every output column is a marginal, so the estimator is unchanged).
//
// Stream (a contract: the tests replay it with numpy): draw j of replicate b is word (b*n + j) mod 4 of Philox4x32-10 at counter
// {lo(q), hi(q), lo(s), hi(s)}, q = (b*n + j) / 4, key {lo(seed), hi(seed)} -- rocrand_device::philox4x32_10_engine(seed, s, b*n + j) -- and
// the drawn sample is (word * n) >> 32.
//
// Layout: a workgroup (8 waves) owns a group at a time (grid-stride over the groups).  The median of a replicate is a function of the
// multiset of drawn RANKS, so each draw only adds one to a per-wave count histogram indexed by the sample's rank, both sets in one 32-bit
// word (signed-set count in the low half, |aFC|-set count in the high half: counts never exceed n < 2^16, so one 32-bit wave scan yields
// both prefix sums).  A wave owns a replicate: 4 draws per lane per Philox call, the histogram in LDS, one wave scan that finds the ranks
// of order statistics (n-1)/2 and n/2 and clears the counters it read.  Rank tables, sorted values and histograms live in LDS for groups
// of up to PHZ_BOOT_LDS_N samples; larger groups read the tables from global memory and count in a per-wave global histogram.
// The replicate medians go to a per-workgroup scratch slice as order-preserving 64-bit keys; a radix select (8 passes of 8 bits, the two
// quantiles of both sets at once) then finds the k-th smallest, and one min pass the (k+1)-th where it differs.
#include <hip/hip_runtime.h>

#include "phz.h"
#include "phz_internal.h"

#ifndef PHZ_BOOT_LDS_N
#define PHZ_BOOT_LDS_N 1024         // largest group kept on chip: 8 waves x n x 4 B of histograms + 12 B per sample of tables (52 KB at 1024)
#endif
#ifndef PHZ_BOOT_GRID
#define PHZ_BOOT_GRID 1024          // most resident workgroups (each holds 2 x bs x 8 B of replicate keys in the scratch)
#endif

namespace {

constexpr int WAVES = 8;
constexpr int THREADS = WAVES * 64;

struct BootArgs {
    int64_t n_groups;
    const int64_t *off;
    const uint64_t *subseq;
    const uint32_t *rank;
    const double *vs, *va;
    uint64_t seed;
    int32_t bs, max_n;
    int32_t k[4];
    uint64_t *keys;        // [gridDim.x][2][bs]
    uint32_t *ghist;       // [gridDim.x][WAVES][max_n], all zero between groups; NULL when every group fits in LDS
    double *order_stats;
    int64_t *sign_counts;
    double *replicates;    // optional
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

// order-preserving key of a double (-0.0 sorts just below +0.0) and back
__device__ __forceinline__ uint64_t key_of(double v) {
    uint64_t b; memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v; memcpy(&v, &b, 8);
    return v;
}

template <bool BIG> __device__ __forceinline__ void wave_sync() {
    if (BIG) __threadfence();              // global histogram: the lanes' atomics are done and this CU's L1 holds no stale line of it
    __builtin_amdgcn_wave_barrier();
}

// every replicate of group g: keys[set * bs + b] = key of the replicate median, res = this wave's 4-word LDS mailbox
template <bool BIG>
__device__ __forceinline__ void replicates(const BootArgs &a, int64_t g, int n, const uint32_t *rank, const double *vs, const double *va, uint32_t *hist,
                           uint64_t *keys, uint32_t *res, unsigned long long *sign) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t s = a.subseq[g];
    const uint32_t m1 = (uint32_t)(n - 1) >> 1, m2 = (uint32_t)n >> 1;      // 0-based order statistics of the median
    const int chunk = (n + 63) >> 6;
    const int lo = min(n, lane * chunk), hi = min(n, lo + chunk);
    unsigned long long pos_s = 0, neg_s = 0, pos_a = 0, neg_a = 0;
    for (int64_t b = wave; b < a.bs; b += WAVES) {
        const uint64_t base = (uint64_t)b * (uint64_t)n, end = base + (uint64_t)n;
        for (uint64_t q = (base >> 2) + lane; 4 * q < end; q += 64) {
            const Quad w = philox4x32_10(q, s, a.seed);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint64_t o = 4 * q + i;
                if (o < base || o >= end) continue;
                const uint32_t p = (uint32_t)(((uint64_t)w.w[i] * (uint32_t)n) >> 32);
                const uint32_t r = rank[p];
                atomicAdd(&hist[r & 0xFFFFu], 1u);
                atomicAdd(&hist[r >> 16], 0x10000u);
            }
        }
        wave_sync<BIG>();
        uint32_t loc = 0;
        for (int r = lo; r < hi; r++) loc += hist[r];
        uint32_t inc = loc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        uint32_t cum = inc - loc;
        for (int r = lo; r < hi; r++) {
            const uint32_t h = hist[r];
            hist[r] = 0;
            const uint32_t nc = cum + h;
            const uint32_t cl = cum & 0xFFFFu, nl = nc & 0xFFFFu, ch = cum >> 16, nh = nc >> 16;
            if (cl <= m1 && m1 < nl) res[0] = (uint32_t)r;
            if (cl <= m2 && m2 < nl) res[1] = (uint32_t)r;
            if (ch <= m1 && m1 < nh) res[2] = (uint32_t)r;
            if (ch <= m2 && m2 < nh) res[3] = (uint32_t)r;
            cum = nc;
        }
        wave_sync<BIG>();
        if (lane == 0) {
            // numpy.median: the mean of the middle element(s), i.e. v or (a + b) / 2 in fp64
            const double ms = (n & 1) ? vs[res[0]] : (vs[res[0]] + vs[res[1]]) / 2.0;
            const double ma = (n & 1) ? va[res[2]] : (va[res[2]] + va[res[3]]) / 2.0;
            keys[b] = key_of(ms);
            keys[a.bs + b] = key_of(ma);
            pos_s += ms > 0; neg_s += ms < 0; pos_a += ma > 0; neg_a += ma < 0;
            if (a.replicates) {
                a.replicates[(2 * g) * (int64_t)a.bs + b] = ms;
                a.replicates[(2 * g + 1) * (int64_t)a.bs + b] = ma;
            }
        }
        __builtin_amdgcn_wave_barrier();              // res is rewritten by the next replicate
    }
    if (lane == 0) {
        atomicAdd(&sign[0], pos_s); atomicAdd(&sign[1], neg_s); atomicAdd(&sign[2], pos_a); atomicAdd(&sign[3], neg_a);
    }
}

__global__ __launch_bounds__(THREADS) void k_boot(BootArgs a) {
    __shared__ uint32_t s_hist[WAVES * PHZ_BOOT_LDS_N];
    __shared__ uint32_t s_rank[PHZ_BOOT_LDS_N];
    __shared__ double s_vs[PHZ_BOOT_LDS_N], s_va[PHZ_BOOT_LDS_N];
    __shared__ uint32_t s_sel[4 * 256];
    __shared__ unsigned long long s_prefix[4], s_min[4], s_sign[4];
    __shared__ uint32_t s_k[4], s_cnt[4];
    __shared__ uint32_t s_res[WAVES * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < WAVES * PHZ_BOOT_LDS_N; i += THREADS) s_hist[i] = 0;
    uint64_t *keys = a.keys + (size_t)blockIdx.x * 2 * (size_t)a.bs;
    for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        const int64_t o = a.off[g];
        const int n = (int)(a.off[g + 1] - o);
        if (n <= 0) {                                 // an empty set: no CI (the reference's NaN row), nothing drawn
            if (tid < 8) a.order_stats[8 * g + tid] = __builtin_nan("");
            if (tid < 4) a.sign_counts[4 * g + tid] = 0;
            continue;
        }
        if (tid < 4) s_sign[tid] = 0;
        if (n <= PHZ_BOOT_LDS_N) {
            for (int i = tid; i < n; i += THREADS) { s_rank[i] = a.rank[o + i]; s_vs[i] = a.vs[o + i]; s_va[i] = a.va[o + i]; }
            __syncthreads();
            replicates<false>(a, g, n, s_rank, s_vs, s_va, s_hist + wave * PHZ_BOOT_LDS_N, keys, s_res + 4 * wave, s_sign);
        } else {
            __syncthreads();
            replicates<true>(a, g, n, a.rank + o, a.vs + o, a.va + o, a.ghist + ((size_t)blockIdx.x * WAVES + wave) * (size_t)a.max_n, keys,
                             s_res + 4 * wave, s_sign);
        }
        __threadfence();                              // the keys are in L2 and no wave of this CU reads a stale L1 line of them
        // ---- radix select: target t = set * 2 + j finds the k[2 j]-th smallest key of set `set`
        if (tid < 4) { s_prefix[tid] = 0; s_k[tid] = (uint32_t)a.k[2 * (tid & 1)]; s_min[tid] = ~0ull; }
        __syncthreads();
        for (int d = 7; d >= 0; d--) {
            const int shift = 8 * d;
            const uint64_t himask = d == 7 ? 0 : (~0ull << (shift + 8));
            for (int i = tid; i < 4 * 256; i += THREADS) s_sel[i] = 0;
            __syncthreads();
            const uint64_t p0 = s_prefix[0], p1 = s_prefix[1], p2 = s_prefix[2], p3 = s_prefix[3];
            for (int64_t b = tid; b < a.bs; b += THREADS) {
                const uint64_t ks = keys[b], ka = keys[a.bs + b];
                if (((ks ^ p0) & himask) == 0) atomicAdd(&s_sel[0 * 256 + ((ks >> shift) & 255)], 1u);
                if (((ks ^ p1) & himask) == 0) atomicAdd(&s_sel[1 * 256 + ((ks >> shift) & 255)], 1u);
                if (((ka ^ p2) & himask) == 0) atomicAdd(&s_sel[2 * 256 + ((ka >> shift) & 255)], 1u);
                if (((ka ^ p3) & himask) == 0) atomicAdd(&s_sel[3 * 256 + ((ka >> shift) & 255)], 1u);
            }
            __syncthreads();
            if (wave < 4) {
                const int t = wave;
                uint32_t h[4], loc = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) { h[j] = s_sel[t * 256 + 4 * lane + j]; loc += h[j]; }
                const uint32_t k = s_k[t];
                uint32_t inc = loc;
#pragma unroll
                for (int dd = 1; dd < 64; dd <<= 1) {
                    const uint32_t x = __shfl_up(inc, dd);
                    if (lane >= dd) inc += x;
                }
                uint32_t cum = inc - loc;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (cum <= k && k < cum + h[j]) {
                        s_prefix[t] |= (unsigned long long)(4 * lane + j) << shift;
                        s_k[t] = k - cum;
                        s_cnt[t] = h[j];
                    }
                    cum += h[j];
                }
            }
            __syncthreads();
        }
        // ---- the (k+1)-th: the same key unless the k-th is the last of its run of equal keys, then the smallest larger key
        bool need[4];
        bool any = false;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            need[t] = a.k[2 * (t & 1) + 1] != a.k[2 * (t & 1)] && s_k[t] + 1 >= s_cnt[t];
            any = any || need[t];
        }
        if (any) {
            for (int64_t b = tid; b < a.bs; b += THREADS) {
                const uint64_t ks = keys[b], ka = keys[a.bs + b];
                if (need[0] && ks > s_prefix[0]) atomicMin(&s_min[0], (unsigned long long)ks);
                if (need[1] && ks > s_prefix[1]) atomicMin(&s_min[1], (unsigned long long)ks);
                if (need[2] && ka > s_prefix[2]) atomicMin(&s_min[2], (unsigned long long)ka);
                if (need[3] && ka > s_prefix[3]) atomicMin(&s_min[3], (unsigned long long)ka);
            }
            __syncthreads();
        }
        if (tid < 4) {
            const int t = tid, set = t >> 1, j = t & 1;
            const uint64_t x = s_prefix[t], y = need[t] ? s_min[t] : x;
            a.order_stats[8 * g + 4 * set + 2 * j] = value_of(x);
            a.order_stats[8 * g + 4 * set + 2 * j + 1] = value_of(y);
            a.sign_counts[4 * g + t] = (int64_t)s_sign[t];
        }
        __syncthreads();                              // the tables, s_sign and the keys are reused by the next group
    }
}

}  // namespace

extern "C" int phz_bootstrap_medians(phz_ctx *ctx, const phz_boot_in *in, double *order_stats, int64_t *sign_counts, double *replicates, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !in || in->n_groups < 0 || in->bs < 1 || in->max_n < 0 || in->max_n > 65535 || (space != PHZ_HOST && space != PHZ_DEVICE))
        return PHZ_E_ARG;
    for (int i = 0; i < 4; i++)
        if (in->k[i] < 0 || in->k[i] >= in->bs) return phz_fail(ctx, PHZ_E_ARG, "phz_bootstrap_medians: order statistic out of range");
    if ((in->k[1] != in->k[0] && in->k[1] != in->k[0] + 1) || (in->k[3] != in->k[2] && in->k[3] != in->k[2] + 1))
        return phz_fail(ctx, PHZ_E_ARG, "phz_bootstrap_medians: k[1] / k[3] must equal k[0] / k[2] or follow it");
    if (in->n_groups == 0) return PHZ_OK;
    if (!in->off || !in->subseq || !order_stats || !sign_counts) return PHZ_E_ARG;
    int64_t total = 0;
    if (space == PHZ_HOST) {
        for (int64_t g = 0; g < in->n_groups; g++) {
            const int64_t n = in->off[g + 1] - in->off[g];
            if (in->off[g] < 0 || n < 0 || n > in->max_n) return phz_fail(ctx, PHZ_E_ARG, "phz_bootstrap_medians: group offsets / max_n inconsistent");
        }
        total = in->off[in->n_groups];
    }
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    BootArgs a;
    a.n_groups = in->n_groups; a.seed = in->seed; a.bs = in->bs; a.max_n = in->max_n;
    for (int i = 0; i < 4; i++) a.k[i] = in->k[i];
    if (int s = st.in(in->off, (size_t)in->n_groups + 1, space, &a.off)) return s;
    if (int s = st.in(in->subseq, (size_t)in->n_groups, space, &a.subseq)) return s;
    if (int s = st.in(in->rank, (size_t)total, space, &a.rank)) return s;
    if (int s = st.in(in->sorted_s, (size_t)total, space, &a.vs)) return s;
    if (int s = st.in(in->sorted_a, (size_t)total, space, &a.va)) return s;
    if (int s = st.out(order_stats, (size_t)in->n_groups * 8, space, &a.order_stats)) return s;
    if (int s = st.out(sign_counts, (size_t)in->n_groups * 4, space, &a.sign_counts)) return s;
    a.replicates = nullptr;
    if (replicates)
        if (int s = st.out(replicates, (size_t)in->n_groups * 2 * (size_t)in->bs, space, &a.replicates)) return s;
    const int grid = (int)(in->n_groups < PHZ_BOOT_GRID ? in->n_groups : PHZ_BOOT_GRID);
    if (int s = phz_reserve(ctx, ctx->boot_keys, (size_t)grid * 2 * (size_t)in->bs * 8)) return s;
    a.keys = (uint64_t *)ctx->boot_keys.p;
    a.ghist = nullptr;
    hipStream_t sm = ctx->stream;
    const size_t ghist_bytes = (size_t)grid * WAVES * (size_t)in->max_n * 4;
    if (in->max_n > PHZ_BOOT_LDS_N) {
        if (int s = phz_reserve(ctx, ctx->boot_hist, ghist_bytes)) return s;
        a.ghist = (uint32_t *)ctx->boot_hist.p;
    }
    if (a.ghist) PHZ_HIP(ctx, hipMemsetAsync(a.ghist, 0, ghist_bytes, sm));
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_BOOT times the kernel alone
    hipLaunchKernelGGL(k_boot, dim3((unsigned)grid), dim3(THREADS), 0, sm, a);
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    (void)hipEventSynchronize(ctx->ev1);
    float ms = 0; (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->last_ms[PHZ_T_BOOT] = ms; ctx->total_ms[PHZ_T_BOOT] += ms; ctx->launches[PHZ_T_BOOT]++;
    if (space == PHZ_HOST) {
        PHZ_HIP(ctx, hipMemcpyAsync(order_stats, a.order_stats, (size_t)in->n_groups * 64, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(sign_counts, a.sign_counts, (size_t)in->n_groups * 32, hipMemcpyDeviceToHost, sm));
        if (replicates)
            PHZ_HIP(ctx, hipMemcpyAsync(replicates, a.replicates, (size_t)in->n_groups * 16 * (size_t)in->bs, hipMemcpyDeviceToHost, sm));
    }
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}
