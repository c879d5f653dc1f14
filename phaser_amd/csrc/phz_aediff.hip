// K_fisher and K_cmh: the statistics of phaser_ae_diff (include/phz.h, phz_fisher_test and phz_cmh_test; DESIGN.md, "phaser_ae_diff, K_fisher and K_cmh").
// The reference has no such tool; the contracts restate R's fisher.test (two-sided) per cell and R's mantelhaen.test (2 x 2 x K, the samples as strata) per
// gene, for the cells [[a1, b1], [a2, b2]] of two conditions.  Everything in fp64.
//
// K_fisher: n1 = a1 + b1, n2 = a2 + b2, m = a1 + a2, N = n1 + n2, k = a1; the support is [lo, hi] = [max(0, m - n2), min(n1, m)],
//   log pmf(x) = [lgamma(n1+1) + lgamma(n2+1) + lgamma(m+1) + lgamma(N-m+1) - lgamma(N+1)] - lgamma(x+1) - lgamma(n1-x+1) - lgamma(m-x+1) - lgamma(n2-m+x+1)
//   pmf(x+1) / pmf(x) = (n1 - x)(m - x) / ((x + 1)(n2 - m + x + 1))
// P = min(1, sum of pmf(i) over all i of the support with pmf(i) <= pmf(k) (1 + 1e-7)).  The pmf is unimodal with a mode at M = floor((n1+1)(m+1) / (N+2)),
// taken in 64-bit integers.  The near tail runs outward from k, away from M.  The far tail runs outward from j, the index next to M on the other side of it
// with log pmf(j) <= log pmf(k) + log1p(1e-7), found by bisection of the log pmf (monotone on either side of M); no such index, no far tail.  Each tail is
// summed by the ratio recurrence until a term falls below 1e-18 of the running sum.  pmf(k) that underflows: 0.  lo == hi: 1.
// The limit of the rule: an exact tie pmf(j) == pmf(k) is told from lgamma's rounding by the relative 1e-7 alone, which holds while the error of a log pmf,
// about 4 E(N) with E(N) = 2^-52 (N + 1) ln(N + 2), stays below 1e-7: up to N of about 6 * 10^6.  Where the pmf is symmetric -- n1 == n2 (mirror m - k) or
// 2 m == N (mirror n1 - k) -- the tie is exact by construction and j is the mirror of k, without a search, at every N (k its own mirror: 1).
// Two tiers by N against PHZ_FISHER_WAVE_N, as K_bbtest's (the header's default, 2^31 - 1, leaves every cell to the lane tier: the wave tier did not pay in
// the A/B of DESIGN.md and runs in builds that set the macro):
//   lane tier   one lane per cell, grid-stride over at most PHZ_AETEST_GRID workgroups.
//   wave tier   the cells above the threshold are compacted into a list (gscan_excl) and taken one wave per cell.  Plan and search run in every lane alike; in
//               a tail lane L of round r owns the PHZ_FISHER_WAVE_B consecutive indices that start (r 64 + L) PHZ_FISHER_WAVE_B from the tail's start, begins
//               at its own lgamma pmf and recurs through them; the lane sums are combined by a fixed xor butterfly (the same bits in every lane) and the tail
//               ends with the first round that adds less than 1e-18 of the sum.
// The tiers do not agree bit for bit; each is held to the same tolerance (tests/test_ae_diff.py).  Within a tier the bits depend on the inputs alone.
//
// K_cmh: one wave per gene (row), lanes stride over the samples.  A stratum is a cell tested under K_fisher's rule with N >= 2.  A lane adds its strata in
// sample order, the lane sums are combined by __shfl_xor from 32 down to 1: the shape of every sum is fixed by n_cols alone.  Per stratum, with the integer
// products taken exactly in int64 (they are below 2^62):
//   D += (a1 N - n1 m) / N        V += n1 n2 * m (N - m) / (N^2 (N - 1))        R += a1 b2 / N        S += b1 a2 / N
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "phz.h"
#include "phz_internal.h"
#include "phz_scan.h"

#ifndef PHZ_AETEST_GRID
#define PHZ_AETEST_GRID 2048        // most workgroups of a kernel here (grid-stride beyond), as in phz_aetest.hip
#endif
#ifndef PHZ_FISHER_WAVE_B
#define PHZ_FISHER_WAVE_B 8         // consecutive tail indices per lane and round of the wave tier
#endif

namespace {

constexpr int THREADS = 256;
constexpr bool WAVE_TIER = PHZ_FISHER_WAVE_N < INT32_MAX;          // INT32_MAX: no cell can lie above it, the list and the wave kernel are not launched

// ------------------------------------------------------------------------------------------------ K_fisher
struct FisherArgs {
    int64_t n_cells;
    const int32_t *a1, *b1, *a2, *b2;
    double log_tol;               // log1p(1e-7)
    int32_t min_cov;
    double *pvalue;
    uint32_t *flag, *pos, *list;  // 1 = wave tier; exclusive scan of flag, pos[n_cells] = cells of the wave tier; their indices
};

struct FiCell {
    double n1, n2, m, base;       // base = lgamma(n1+1) + lgamma(n2+1) + lgamma(m+1) + lgamma(N-m+1) - lgamma(N+1)
    int32_t k, lo, hi, mode;
    bool symmetric; int32_t mirror;
};

// a tested cell's four counts -> the cell; false: not tested
__device__ __forceinline__ bool fi_load(const FisherArgs &g, int64_t t, FiCell *q, int64_t *N_out) {
    const int32_t a1 = g.a1[t], b1 = g.b1[t], a2 = g.a2[t], b2 = g.b2[t];
    if (a1 < 0 || b1 < 0 || a2 < 0 || b2 < 0) return false;
    const int64_t least = g.min_cov > 1 ? g.min_cov : 1;
    const int64_t n1 = (int64_t)a1 + b1, n2 = (int64_t)a2 + b2, m = (int64_t)a1 + a2, N = n1 + n2;          // N fits in int32: checked on the host for PHZ_HOST, the caller's guarantee for PHZ_DEVICE
    if (n1 < least || n2 < least) return false;
    q->n1 = (double)n1; q->n2 = (double)n2; q->m = (double)m;
    q->k = a1; q->lo = (int32_t)(m > n2 ? m - n2 : 0); q->hi = (int32_t)(n1 < m ? n1 : m);
    int64_t mode = (n1 + 1) * (m + 1) / (N + 2);
    q->mode = (int32_t)(mode < q->lo ? q->lo : (mode > q->hi ? q->hi : mode));
    q->symmetric = n1 == n2 || 2 * m == N;
    q->mirror = (int32_t)(n1 == n2 ? m - a1 : n1 - a1);
    *N_out = N;
    return true;
}
__device__ __forceinline__ void fi_base(FiCell *q) {
    const double N = q->n1 + q->n2;
    q->base = lgamma(q->n1 + 1.0) + lgamma(q->n2 + 1.0) + lgamma(q->m + 1.0) + lgamma(N - q->m + 1.0) - lgamma(N + 1.0);
}
__device__ __forceinline__ double fi_lp(const FiCell &q, double x) {
    return q.base - lgamma(x + 1.0) - lgamma(q.n1 - x + 1.0) - lgamma(q.m - x + 1.0) - lgamma(q.n2 - q.m + x + 1.0);
}
// pmf(x + 1) = pmf(x) * fi_step_up(x), pmf(x - 1) = pmf(x) * fi_step_down(x)
__device__ __forceinline__ double fi_step_up(const FiCell &q, double x) { return (q.n1 - x) * (q.m - x) / ((x + 1.0) * (q.n2 - q.m + x + 1.0)); }
__device__ __forceinline__ double fi_step_down(const FiCell &q, double x) { return x * (q.n2 - q.m + x) / ((q.n1 - x + 1.0) * (q.m - x + 1.0)); }

// The far tail's start index (-1: none) and whether the near tail runs down from k (the far tail then runs up from the index).  -2: k is its own mirror.
__device__ __forceinline__ int32_t fi_far(const FiCell &q, double thr, bool *near_down) {
    if (q.symmetric) {
        *near_down = q.k < q.mirror;
        return q.mirror == q.k ? -2 : q.mirror;
    }
    int32_t lo, hi;
    if (q.k < q.mode) {
        // the smallest i in [mode, hi] with pmf(i) <= pmf(k) (1 + 1e-7): the pmf does not rise on that range
        *near_down = true;
        lo = q.mode; hi = q.hi;
        if (fi_lp(q, (double)hi) > thr) return -1;
        while (lo < hi) { const int32_t mid = lo + (hi - lo) / 2; if (fi_lp(q, (double)mid) <= thr) hi = mid; else lo = mid + 1; }
        return lo;
    }
    // the largest i in [lo, mode] below k with pmf(i) <= pmf(k) (1 + 1e-7): the pmf does not fall on that range
    *near_down = false;
    lo = q.lo; hi = q.mode < q.k ? q.mode : q.k - 1;
    if (hi < lo || fi_lp(q, (double)lo) > thr) return -1;
    while (lo < hi) { const int32_t mid = lo + (hi - lo + 1) / 2; if (fi_lp(q, (double)mid) <= thr) lo = mid; else hi = mid - 1; }
    return lo;
}

__device__ __forceinline__ double fi_tail_down(const FiCell &q, int32_t start, double term) {
    double sum = term;
    for (int32_t i = start; i > q.lo && term > 1e-18 * sum; i--) { term *= fi_step_down(q, (double)i); sum += term; }
    return sum;
}
__device__ __forceinline__ double fi_tail_up(const FiCell &q, int32_t start, double term) {
    double sum = term;
    for (int32_t i = start; i < q.hi && term > 1e-18 * sum; i++) { term *= fi_step_up(q, (double)i); sum += term; }
    return sum;
}

__device__ __forceinline__ double fi_two_sided_lane(const FiCell &q, double log_tol) {
    if (q.lo == q.hi) return 1.0;
    const double lk = fi_lp(q, (double)q.k), pk = exp(lk);
    if (pk == 0.0) return 0.0;
    bool near_down = false;
    const int32_t far = fi_far(q, lk + log_tol, &near_down);
    if (far == -2) return 1.0;
    double P = near_down ? fi_tail_down(q, q.k, pk) : fi_tail_up(q, q.k, pk);
    if (far >= 0) {
        const double pf = q.symmetric ? pk : exp(fi_lp(q, (double)far));
        P += near_down ? fi_tail_up(q, far, pf) : fi_tail_down(q, far, pf);
    }
    return P < 1.0 ? P : 1.0;
}

__device__ __forceinline__ double fi_wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}
// dir = -1: pmf(start) + pmf(start - 1) + ... + pmf(lo); dir = +1: ... + pmf(hi).  Called by all 64 lanes with the same arguments; the same bits return in each.
__device__ __forceinline__ double fi_tail_wave(const FiCell &q, int32_t start, int dir, int lane) {
    double total = 0.0;
    const int64_t room = dir < 0 ? (int64_t)start - q.lo : (int64_t)q.hi - start;          // indices beyond the start
    for (int64_t first = 0; first <= room; first += 64 * PHZ_FISHER_WAVE_B) {
        const int64_t off = first + (int64_t)lane * PHZ_FISHER_WAVE_B;
        double sum = 0.0;
        if (off <= room) {
            const int64_t left = room - off;          // indices of the tail beyond this lane's first
            const int steps = (int)(left < PHZ_FISHER_WAVE_B - 1 ? left : PHZ_FISHER_WAVE_B - 1);
            double i = (double)start + (double)dir * (double)off;
            double term = exp(fi_lp(q, i));
            sum = term;
            for (int s = 0; s < steps; s++) {
                term *= dir < 0 ? fi_step_down(q, i) : fi_step_up(q, i);
                i += (double)dir;
                sum += term;
            }
        }
        const double round = fi_wave_sum(sum);
        total += round;
        if (!(round > 1e-18 * total)) break;
    }
    return total;
}

__global__ __launch_bounds__(THREADS) void k_fisher_lane(FisherArgs g) {
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < g.n_cells; t += (int64_t)gridDim.x * THREADS) {
        FiCell q;
        int64_t N;
        double p = __builtin_nan("");
        uint32_t wave = 0;
        if (fi_load(g, t, &q, &N)) {
            if (WAVE_TIER && N > (int64_t)PHZ_FISHER_WAVE_N) wave = 1;
            else { fi_base(&q); p = fi_two_sided_lane(q, g.log_tol); }
        }
        if (WAVE_TIER) g.flag[t] = wave;
        g.pvalue[t] = p;
    }
}

__global__ __launch_bounds__(THREADS) void k_fisher_list(FisherArgs g) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t < g.n_cells && g.flag[t]) g.list[g.pos[t]] = (uint32_t)t;
}

__global__ __launch_bounds__(THREADS) void k_fisher_wave(FisherArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t count = g.pos[g.n_cells], n_waves = (int64_t)gridDim.x * (THREADS / 64);
    for (int64_t w = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); w < count; w += n_waves) {
        const int64_t t = g.list[w];
        FiCell q;
        int64_t N;
        (void)fi_load(g, t, &q, &N);          // a listed cell is a tested one
        fi_base(&q);
        double P = 1.0;
        if (q.lo < q.hi) {                    // every branch below is the same in all lanes
            const double lk = fi_lp(q, (double)q.k);
            if (exp(lk) == 0.0) {
                P = 0.0;
            } else {
                bool near_down = false;
                const int32_t far = fi_far(q, lk + g.log_tol, &near_down);
                if (far != -2) {
                    P = fi_tail_wave(q, q.k, near_down ? -1 : +1, lane);
                    if (far >= 0) P += fi_tail_wave(q, far, near_down ? +1 : -1, lane);
                    P = P < 1.0 ? P : 1.0;
                }
            }
        }
        if (lane == 0) g.pvalue[t] = P;
    }
}

// ------------------------------------------------------------------------------------------------ K_cmh
struct CmhArgs {
    int64_t n_rows, n_cols;
    const int32_t *a1, *b1, *a2, *b2;
    int32_t min_cov, min_samples, correct;
    double *stat, *pvalue, *log2_or;
    int32_t *n_strata;
};

__global__ __launch_bounds__(THREADS) void k_cmh(CmhArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * (THREADS / 64);
    const int64_t least = g.min_cov > 1 ? g.min_cov : 1;
    for (int64_t r = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); r < g.n_rows; r += n_waves) {
        double D = 0.0, V = 0.0, R = 0.0, S = 0.0;
        int32_t cnt = 0;
        for (int64_t c = lane; c < g.n_cols; c += 64) {
            const int64_t t = r * g.n_cols + c;
            const int64_t a1 = g.a1[t], b1 = g.b1[t], a2 = g.a2[t], b2 = g.b2[t];
            if (a1 < 0 || b1 < 0 || a2 < 0 || b2 < 0) continue;
            const int64_t n1 = a1 + b1, n2 = a2 + b2, m = a1 + a2, N = n1 + n2;          // N fits in int32, as in K_fisher
            if (n1 < least || n2 < least || N < 2) continue;
            const double Nd = (double)N;
            D += (double)(a1 * N - n1 * m) / Nd;
            V += (double)(n1 * n2) * (double)(m * (N - m)) / (Nd * Nd * (Nd - 1.0));
            R += (double)(a1 * b2) / Nd;
            S += (double)(b1 * a2) / Nd;
            cnt++;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            D += __shfl_xor(D, d); V += __shfl_xor(V, d); R += __shfl_xor(R, d); S += __shfl_xor(S, d); cnt += __shfl_xor(cnt, d);
        }
        if (lane != 0) continue;
        const double nan = __builtin_nan("");
        double stat = nan, p = nan;
        if (cnt >= (g.min_samples > 1 ? g.min_samples : 1) && V != 0.0) {
            const double ad = fabs(D), y = g.correct != 0 && ad >= 0.5 ? 0.5 : 0.0, e = ad - y;
            stat = e * e / V;
            p = erfc(sqrt(stat / 2.0));
        }
        // log2(R / S) with gene_ae's conventions: S = 0 < R: +inf, R = 0 < S: -inf, both 0: NaN
        const double inf = __builtin_inf();
        const double lor = S == 0.0 ? (R == 0.0 ? nan : inf) : (R == 0.0 ? -inf : log2(R / S));
        g.stat[r] = stat; g.pvalue[r] = p; g.log2_or[r] = lor; g.n_strata[r] = cnt;
    }
}

void record_ms(phz_ctx *ctx, int slot) {
    (void)hipEventSynchronize(ctx->ev1);
    float ms = 0; (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->last_ms[slot] = ms; ctx->total_ms[slot] += ms; ctx->launches[slot]++;
}

// the argument errors both entry points share; n_cells is set when they pass
int check_matrices(phz_ctx *ctx, const char *who, int64_t n_rows, int64_t n_cols, const int32_t *a1, const int32_t *b1, const int32_t *a2, const int32_t *b2, int space,
                   int64_t *n_cells) {
    char msg[160];
    if (n_cols && n_rows > (int64_t)INT32_MAX / n_cols) { snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 cells", who); return phz_fail(ctx, PHZ_E_ARG, msg); }
    *n_cells = n_rows * n_cols;
    if (*n_cells && (!a1 || !b1 || !a2 || !b2)) return PHZ_E_ARG;
    if (space == PHZ_HOST)
        for (int64_t t = 0; t < *n_cells; t++)
            if (a1[t] >= 0 && b1[t] >= 0 && a2[t] >= 0 && b2[t] >= 0 && (int64_t)a1[t] + b1[t] + a2[t] + b2[t] > INT32_MAX) {
                snprintf(msg, sizeof msg, "%s: a1 + b1 + a2 + b2 does not fit in int32", who); return phz_fail(ctx, PHZ_E_ARG, msg);
            }
    return PHZ_OK;
}

}  // namespace

extern "C" int phz_fisher_test(phz_ctx *ctx, int64_t n_rows, int64_t n_cols, const int32_t *a1, const int32_t *b1, const int32_t *a2, const int32_t *b2, int32_t min_cov,
                               double *pvalue, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_rows < 0 || n_cols < 0 || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    int64_t n = 0;
    if (int s = check_matrices(ctx, "phz_fisher_test", n_rows, n_cols, a1, b1, a2, b2, space, &n)) return s;
    if (n == 0) return PHZ_OK;
    if (!pvalue) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    FisherArgs g;
    g.n_cells = n; g.log_tol = log1p(1e-7); g.min_cov = min_cov; g.flag = g.pos = g.list = nullptr;
    if (int s = st.in(a1, (size_t)n, space, &g.a1)) return s;
    if (int s = st.in(b1, (size_t)n, space, &g.b1)) return s;
    if (int s = st.in(a2, (size_t)n, space, &g.a2)) return s;
    if (int s = st.in(b2, (size_t)n, space, &g.b2)) return s;
    if (int s = st.out(pvalue, (size_t)n, space, &g.pvalue)) return s;
    DevBuf *S = ctx->scratch;
    if (WAVE_TIER) {
        if (int s = reserve_all(ctx, {{S[SC_FISHER_FLAG], (size_t)n * 4}, {S[SC_FISHER_POS], ((size_t)n + 1) * 4}, {S[SC_FISHER_LIST], (size_t)n * 4}})) return s;
        g.flag = (uint32_t *)S[SC_FISHER_FLAG].p; g.pos = (uint32_t *)S[SC_FISHER_POS].p; g.list = (uint32_t *)S[SC_FISHER_LIST].p;
    }
    hipStream_t sm = ctx->stream;
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_FISHER: lane tier, compaction, wave tier
    hipLaunchKernelGGL(k_fisher_lane, dim3((unsigned)std::min<int64_t>(nblk(n), (int64_t)PHZ_AETEST_GRID)), dim3(THREADS), 0, sm, g);
    if (WAVE_TIER) {
        if (int s = gscan_excl<uint32_t, uint32_t>(ctx, g.flag, g.pos, n, S[SC_FISHER_SCAN_TMP])) return s;
        hipLaunchKernelGGL(k_fisher_list, dim3(nblk(n)), dim3(THREADS), 0, sm, g);
        // the number of listed cells is known to the device alone: a wave per listed cell at most, the rest of the grid returns at once
        hipLaunchKernelGGL(k_fisher_wave, dim3((unsigned)std::min<int64_t>((n + THREADS / 64 - 1) / (THREADS / 64), (int64_t)PHZ_AETEST_GRID)), dim3(THREADS), 0, sm, g);
    }
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    record_ms(ctx, PHZ_T_FISHER);
    if (space == PHZ_HOST) PHZ_HIP(ctx, hipMemcpyAsync(pvalue, g.pvalue, (size_t)n * 8, hipMemcpyDeviceToHost, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}

extern "C" int phz_cmh_test(phz_ctx *ctx, int64_t n_rows, int64_t n_cols, const int32_t *a1, const int32_t *b1, const int32_t *a2, const int32_t *b2, int32_t min_cov,
                            int32_t min_samples, int32_t correct, double *stat, double *pvalue, double *log2_or, int32_t *n_strata, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_rows < 0 || n_cols < 0 || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    int64_t n = 0;
    if (int s = check_matrices(ctx, "phz_cmh_test", n_rows, n_cols, a1, b1, a2, b2, space, &n)) return s;
    if (n_rows == 0) return PHZ_OK;
    if (!stat || !pvalue || !log2_or || !n_strata) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    CmhArgs g;
    g.n_rows = n_rows; g.n_cols = n_cols; g.min_cov = min_cov; g.min_samples = min_samples; g.correct = correct;
    if (int s = st.in(a1, (size_t)n, space, &g.a1)) return s;
    if (int s = st.in(b1, (size_t)n, space, &g.b1)) return s;
    if (int s = st.in(a2, (size_t)n, space, &g.a2)) return s;
    if (int s = st.in(b2, (size_t)n, space, &g.b2)) return s;
    if (int s = st.out(stat, (size_t)n_rows, space, &g.stat)) return s;
    if (int s = st.out(pvalue, (size_t)n_rows, space, &g.pvalue)) return s;
    if (int s = st.out(log2_or, (size_t)n_rows, space, &g.log2_or)) return s;
    if (int s = st.out(n_strata, (size_t)n_rows, space, &g.n_strata)) return s;
    hipStream_t sm = ctx->stream;
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_CMH times the kernel alone
    hipLaunchKernelGGL(k_cmh, dim3((unsigned)std::min<int64_t>((n_rows + THREADS / 64 - 1) / (THREADS / 64), (int64_t)PHZ_AETEST_GRID)), dim3(THREADS), 0, sm, g);
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    record_ms(ctx, PHZ_T_CMH);
    if (space == PHZ_HOST) {
        PHZ_HIP(ctx, hipMemcpyAsync(stat, g.stat, (size_t)n_rows * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(pvalue, g.pvalue, (size_t)n_rows * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(log2_or, g.log2_or, (size_t)n_rows * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(n_strata, g.n_strata, (size_t)n_rows * 4, hipMemcpyDeviceToHost, sm));
    }
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}
