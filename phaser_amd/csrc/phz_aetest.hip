// K_binom and K_bh: the statistics of phaser_ae_test (include/phz.h, phz_binom_test and phz_bh_adjust).  The reference has no such tool; the contracts
// restate scipy.stats.binomtest(k, n, p0, alternative="two-sided") and scipy.stats.false_discovery_control(p, method="bh") ("phaser_ae_test,
// K_binom and K_bh").
//
// K_binom: one lane per test, grid-stride over at most PHZ_AETEST_GRID workgroups.  Everything in fp64.  A lane takes log pmf(k) through lgamma, finds the
// far-side index j by binary search on the log pmf (monotone on either side of the mode) against log pmf(k) + log1p(1e-7), and sums each tail outward from its
// start index by the pmf recurrence until a term falls below 1e-18 of the running sum: O(sqrt(n)) iterations per tail.  The loops diverge inside a wave (n
// differs from cell to cell); no balancing scheme, see DESIGN.md.
//
// K_bh: the tested (non-NaN) cells of the row-major matrix are compacted in cell order (one scan), sorted by p-value (a non-negative double orders as its
// 64 bits; 62 of them are significant for p <= 1) and then stably by column, both with radix_sort_pairs.  A workgroup then owns a column at a time and
// walks its segment from the top rank down in tiles of 256: p * (m / s) per cell, a prefix minimum along the tile, the running minimum carried from tile to
// tile, min(1, .) scattered back to the cell.  Minima are exact, so the result does not depend on how the tiles cut the segment; tied p-values get the same
// q whatever order the sort leaves them in.
#include <hip/hip_runtime.h>
#include <math.h>

#include "phz.h"
#include "phz_internal.h"
#include "phz_sort.h"

#ifndef PHZ_AETEST_GRID
#define PHZ_AETEST_GRID 2048        // most workgroups of k_binom and k_bh_walk (grid-stride beyond)
#endif

namespace {

constexpr int THREADS = 256;

// ------------------------------------------------------------------------------------------------ K_binom
struct BinomArgs {
    int64_t n_tests;
    const int32_t *a, *b;
    double p0, log_p, log_q, odds, log_tol;      // log(p0), log1p(-p0), p0 / (1 - p0), log1p(1e-7): taken once on the host
    int32_t min_cov;
    double *pvalue;
};

__device__ __forceinline__ double log_pmf(const BinomArgs &g, double n, double lg_n1, double i) {
    return lg_n1 - lgamma(i + 1.0) - lgamma(n - i + 1.0) + i * g.log_p + (n - i) * g.log_q;
}
// pmf(start) + pmf(start - 1) + ... : pmf(i - 1) = pmf(i) * i / ((n - i + 1) * odds)
__device__ __forceinline__ double tail_down(double n, int32_t start, double term, double odds) {
    double sum = term;
    for (int32_t i = start; i > 0 && term > 1e-18 * sum; i--) {
        term *= (double)i / ((n - (double)i + 1.0) * odds);
        sum += term;
    }
    return sum;
}
// pmf(start) + pmf(start + 1) + ... : pmf(i + 1) = pmf(i) * (n - i) * odds / (i + 1)
__device__ __forceinline__ double tail_up(double n, int32_t n_int, int32_t start, double term, double odds) {
    double sum = term;
    for (int32_t i = start; i < n_int && term > 1e-18 * sum; i++) {
        term *= (n - (double)i) * odds / ((double)i + 1.0);
        sum += term;
    }
    return sum;
}

__device__ __forceinline__ double binom_two_sided(const BinomArgs &g, int32_t k, int32_t n_int) {
    const double n = (double)n_int, mean = g.p0 * n;
    if ((double)k == mean) return 1.0;
    const double lg_n1 = lgamma(n + 1.0);
    const double lk = log_pmf(g, n, lg_n1, (double)k);
    const double thr = lk + g.log_tol;
    const double pk = exp(lk);
    double P;
    if ((double)k < mean) {
        // j = smallest i in [ceil(mean), n] with pmf(i) <= pmf(k) (1 + 1e-7): the pmf does not rise on that range
        int32_t lo = (int32_t)ceil(mean), hi = n_int;
        P = tail_down(n, k, pk, g.odds);
        if (lo <= hi && log_pmf(g, n, lg_n1, (double)hi) <= thr) {
            while (lo < hi) {
                const int32_t mid = lo + (hi - lo) / 2;
                if (log_pmf(g, n, lg_n1, (double)mid) <= thr) hi = mid; else lo = mid + 1;
            }
            P += tail_up(n, n_int, lo, exp(log_pmf(g, n, lg_n1, (double)lo)), g.odds);
        }
    } else {
        // j = largest i in [0, floor(mean)] with pmf(i) <= pmf(k) (1 + 1e-7): the pmf does not fall on that range
        int32_t lo = 0, hi = (int32_t)floor(mean);
        P = tail_up(n, n_int, k, pk, g.odds);
        if (log_pmf(g, n, lg_n1, 0.0) <= thr) {
            while (lo < hi) {
                const int32_t mid = lo + (hi - lo + 1) / 2;
                if (log_pmf(g, n, lg_n1, (double)mid) <= thr) lo = mid; else hi = mid - 1;
            }
            P += tail_down(n, lo, exp(log_pmf(g, n, lg_n1, (double)lo)), g.odds);
        }
    }
    return P < 1.0 ? P : 1.0;
}

__global__ __launch_bounds__(THREADS) void k_binom(BinomArgs g) {
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < g.n_tests; t += (int64_t)gridDim.x * THREADS) {
        const int32_t a = g.a[t], b = g.b[t];
        double p = __builtin_nan("");
        if (a >= 0 && b >= 0) {
            const int32_t n = a + b;          // fits: checked on the host for PHZ_HOST, the caller's guarantee for PHZ_DEVICE
            if (n >= (g.min_cov > 1 ? g.min_cov : 1)) p = binom_two_sided(g, a, n);
        }
        g.pvalue[t] = p;
    }
}

// ------------------------------------------------------------------------------------------------ K_bh
struct Tested { template <class T> __device__ static __forceinline__ T f(T x) { return x == x ? (T)1 : (T)0; } };

// tested cells per column: thread = column (consecutive lanes read consecutive cells), blockIdx.y = a chunk of rows
__global__ __launch_bounds__(THREADS) void k_bh_count(const double *p, int64_t n_rows, int64_t n_cols, int64_t rows_per_chunk, uint32_t *col_count) {
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= n_cols) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk, r1 = r0 + rows_per_chunk < n_rows ? r0 + rows_per_chunk : n_rows;
    uint32_t cnt = 0;
    for (int64_t r = r0; r < r1; r++) { const double v = p[r * n_cols + c]; cnt += v == v ? 1u : 0u; }
    if (cnt) atomicAdd(&col_count[c], cnt);
}

// cell i: tested -> (bits of p, i) at its place among the tested cells; not tested -> q = NaN
__global__ __launch_bounds__(THREADS) void k_bh_compact(const double *p, int64_t n, const uint32_t *pos, uint64_t *key, uint32_t *cell, double *q) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const double v = p[i];
    if (v == v) {
        uint64_t bits; memcpy(&bits, &v, 8);
        key[pos[i]] = bits; cell[pos[i]] = (uint32_t)i;
    } else {
        q[i] = __builtin_nan("");
    }
}

__global__ __launch_bounds__(THREADS) void k_bh_colkey(const uint32_t *cell, int64_t m, uint32_t n_cols, uint32_t *ckey) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < m) ckey[i] = cell[i] % n_cols;
}

// column c: cells cell[off[c] .. off[c + 1]) in ascending p; rank s (1-based) gets min(1, min over ranks >= s of p * (m / s))
__global__ __launch_bounds__(THREADS) void k_bh_walk(const double *p, const uint32_t *cell, const uint32_t *off, int64_t n_cols, double *q, int64_t *n_tested) {
    __shared__ double s_w[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = __builtin_inf();
    for (int64_t c = blockIdx.x; c < n_cols; c += gridDim.x) {
        const int64_t lo = off[c], hi = off[c + 1];
        const double m = (double)(hi - lo);
        if (tid == 0) n_tested[c] = hi - lo;
        double carry = inf;                          // minimum over the ranks above this tile (the same in every thread)
        for (int64_t top = hi; top > lo; top -= THREADS) {
            const int64_t i = top - 1 - tid;         // thread 0 holds the tile's top rank
            const bool valid = i >= lo;
            const uint32_t ce = valid ? cell[i] : 0u;
            double x = valid ? p[ce] * (m / (double)(i - lo + 1)) : inf;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d); if (lane >= d) x = y < x ? y : x; }
            if (lane == 63) s_w[wave] = x;
            __syncthreads();
            double before = carry;
            for (int w = 0; w < THREADS / 64; w++) {
                const double y = s_w[w];
                if (w < wave) before = y < before ? y : before;
                carry = y < carry ? y : carry;
            }
            x = before < x ? before : x;
            if (valid) q[ce] = x < 1.0 ? x : 1.0;
            __syncthreads();                         // s_w is rewritten by the next tile
        }
    }
}

void record_ms(phz_ctx *ctx, int slot) {
    (void)hipEventSynchronize(ctx->ev1);
    float ms = 0; (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->last_ms[slot] = ms; ctx->total_ms[slot] += ms; ctx->launches[slot]++;
}

}  // namespace

extern "C" int phz_binom_test(phz_ctx *ctx, int64_t n_tests, const int32_t *a, const int32_t *b, double p0, int32_t min_cov, double *pvalue, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_tests < 0 || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    if (!(p0 > 0.0 && p0 < 1.0)) return phz_fail(ctx, PHZ_E_ARG, "phz_binom_test: p0 must lie strictly between 0 and 1");
    if (n_tests == 0) return PHZ_OK;
    if (!a || !b || !pvalue) return PHZ_E_ARG;
    if (space == PHZ_HOST)
        for (int64_t t = 0; t < n_tests; t++)
            if (a[t] >= 0 && b[t] >= 0 && (int64_t)a[t] + (int64_t)b[t] > INT32_MAX) return phz_fail(ctx, PHZ_E_ARG, "phz_binom_test: a + b does not fit in int32");
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    BinomArgs g;
    g.n_tests = n_tests; g.p0 = p0; g.log_p = log(p0); g.log_q = log1p(-p0); g.odds = p0 / (1.0 - p0); g.log_tol = log1p(1e-7); g.min_cov = min_cov;
    if (int s = st.in(a, (size_t)n_tests, space, &g.a)) return s;
    if (int s = st.in(b, (size_t)n_tests, space, &g.b)) return s;
    if (int s = st.out(pvalue, (size_t)n_tests, space, &g.pvalue)) return s;
    hipStream_t sm = ctx->stream;
    const unsigned grid = (unsigned)std::min<int64_t>((n_tests + THREADS - 1) / THREADS, (int64_t)PHZ_AETEST_GRID);
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_BINOM times the kernel alone
    hipLaunchKernelGGL(k_binom, dim3(grid), dim3(THREADS), 0, sm, g);
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    record_ms(ctx, PHZ_T_BINOM);
    if (space == PHZ_HOST) PHZ_HIP(ctx, hipMemcpyAsync(pvalue, g.pvalue, (size_t)n_tests * 8, hipMemcpyDeviceToHost, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}

extern "C" int phz_bh_adjust(phz_ctx *ctx, int64_t n_rows, int64_t n_cols, const double *pvalue, double *qvalue, int64_t *n_tested, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_rows < 0 || n_cols < 0 || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    if (n_cols == 0) return PHZ_OK;
    if (!n_tested || (n_rows && (!pvalue || !qvalue))) return PHZ_E_ARG;
    if (n_rows > (int64_t)INT32_MAX / n_cols) return phz_fail(ctx, PHZ_E_ARG, "phz_bh_adjust: more than 2^31 - 1 cells");
    const int64_t n = n_rows * n_cols;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    const double *p = nullptr; double *q = nullptr; int64_t *nt = nullptr;
    if (int s = st.in(pvalue, (size_t)n, space, &p)) return s;
    if (int s = st.out(qvalue, (size_t)n, space, &q)) return s;
    if (int s = st.out(n_tested, (size_t)n_cols, space, &nt)) return s;
    DevBuf *S = ctx->scratch;
    if (int s = reserve_all(ctx, {{S[SC_BH_POS], ((size_t)n + 1) * 4}, {S[SC_BH_COL_COUNT], (size_t)n_cols * 4}, {S[SC_BH_COL_OFF], ((size_t)n_cols + 1) * 4}})) return s;
    uint32_t *pos = (uint32_t *)S[SC_BH_POS].p, *col_count = (uint32_t *)S[SC_BH_COL_COUNT].p, *col_off = (uint32_t *)S[SC_BH_COL_OFF].p;
    hipStream_t sm = ctx->stream;
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_BH: count, compaction, both sorts and the walk
    PHZ_HIP(ctx, hipMemsetAsync(col_count, 0, (size_t)n_cols * 4, sm));
    const int64_t rows_per_chunk = std::max<int64_t>(64, (n_rows + 32767) / 32768);          // at most 32,768 chunks: grid.y
    if (n) hipLaunchKernelGGL(k_bh_count, dim3(nblk(n_cols), (unsigned)((n_rows + rows_per_chunk - 1) / rows_per_chunk)), dim3(THREADS), 0, sm, p, n_rows, n_cols, rows_per_chunk, col_count);
    if (int s = gscan_excl<uint32_t, uint32_t>(ctx, col_count, col_off, n_cols, S[SC_BH_SCAN_TMP])) return s;
    if (n) {
        // the number of tested cells is known to the device alone: the buffers are sized for all n, the sorts run over the m tested ones
        if (int s = gscan_excl<double, uint32_t, Tested>(ctx, p, pos, n, S[SC_BH_SCAN_TMP])) return s;
        PhzMail mail(ctx);
        const int slot = mail.add(pos + n, 4);
        if (int s = mail.send()) return s;
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        const int64_t m = (int64_t)*mail.at<uint32_t>(slot);
        const size_t cap = (size_t)(m ? m : 1);
        if (int s = reserve_all(ctx, {{S[SC_BH_KEY0], cap * 8}, {S[SC_BH_KEY1], cap * 8}, {S[SC_BH_CELL0], cap * 4}, {S[SC_BH_CELL1], cap * 4},
                                      {S[SC_BH_CKEY0], cap * 4}, {S[SC_BH_CKEY1], cap * 4}})) return s;
        uint64_t *key[2] = {(uint64_t *)S[SC_BH_KEY0].p, (uint64_t *)S[SC_BH_KEY1].p};
        uint32_t *cell[2] = {(uint32_t *)S[SC_BH_CELL0].p, (uint32_t *)S[SC_BH_CELL1].p};
        uint32_t *ckey[2] = {(uint32_t *)S[SC_BH_CKEY0].p, (uint32_t *)S[SC_BH_CKEY1].p};
        hipLaunchKernelGGL(k_bh_compact, dim3(nblk(n)), dim3(THREADS), 0, sm, p, n, (const uint32_t *)pos, key[0], cell[0], q);
        int w = 0;
        // p <= 1.0 = 0x3FF0...: bits 62 and 63 are clear
        if (int s = radix_sort_pairs<uint64_t, uint32_t>(ctx, key[0], key[1], cell[0], cell[1], m, 0, 62, S[SC_BH_SORT_COUNT], S[SC_BH_SCAN_TMP], &w)) return s;
        uint32_t *by_p = cell[w], *spare = cell[w ^ 1];
        if (m && n_cols > 1) {
            hipLaunchKernelGGL(k_bh_colkey, dim3(nblk(m)), dim3(THREADS), 0, sm, (const uint32_t *)by_p, m, (uint32_t)n_cols, ckey[0]);
            int w2 = 0;
            if (int s = radix_sort_pairs<uint32_t, uint32_t>(ctx, ckey[0], ckey[1], by_p, spare, m, 0, bits_for((uint64_t)n_cols - 1), S[SC_BH_SORT_COUNT], S[SC_BH_SCAN_TMP], &w2))
                return s;
            if (w2) by_p = spare;
        }
        const unsigned grid = (unsigned)std::min<int64_t>(n_cols, (int64_t)PHZ_AETEST_GRID);
        hipLaunchKernelGGL(k_bh_walk, dim3(grid), dim3(THREADS), 0, sm, p, (const uint32_t *)by_p, (const uint32_t *)col_off, n_cols, q, nt);
    } else {
        PHZ_HIP(ctx, hipMemsetAsync(nt, 0, (size_t)n_cols * 8, sm));
    }
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    record_ms(ctx, PHZ_T_BH);
    if (space == PHZ_HOST) {
        if (n) PHZ_HIP(ctx, hipMemcpyAsync(qvalue, q, (size_t)n * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(n_tested, nt, (size_t)n_cols * 8, hipMemcpyDeviceToHost, sm));
    }
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}
