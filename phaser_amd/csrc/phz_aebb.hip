// K_bbfit and K_bbtest: the overdispersed statistics of phaser_ae_test (include/phz.h, phz_betabinom_fit and phz_betabinom_test; DESIGN.md, "K_bbfit and
// K_bbtest").  The null is a beta-binomial with mean p0 and overdispersion rho: alpha = p0 (1 - rho) / rho, beta = (1 - p0)(1 - rho) / rho,
//   log pmf(i) = [lgamma(n+1) - lgamma(i+1) - lgamma(n-i+1)] + [lgamma(i+alpha) + lgamma(n-i+beta) - lgamma(n+alpha+beta)] + [lgamma(alpha+beta) - lgamma(alpha) - lgamma(beta)]
// with PHZ_BB_RHO_MIN <= rho <= m / (1 + m), m = min(p0, 1 - p0): alpha, beta >= 1, the ratio pmf(i+1) / pmf(i) = (n-i)(i+alpha) / ((i+1)(n-i-1+beta)) does not
// increase with i, the pmf is unimodal.  Everything in fp64.
//
// K_bbfit: per column the rho that maximises the summed log pmf of its tested cells, by R = 4 rounds of G = 64 candidates equally spaced in ln rho.  Per round
// two launches and no host wait:
//   k_bbfit_eval   one wave per (chunk of 256 rows, block of 64 columns), lane = column: consecutive lanes read consecutive cells.  A tile of 8 rows is loaded
//                  once -- k, n - k and the first bracket above, which no candidate changes -- into the lane's own column of an LDS array (read by that lane
//                  alone: no barrier), then every candidate walks the tile; the 64 running sums of a lane live in LDS as well.  The third bracket comes from
//                  the candidate table.  The sums of the chunk go to partial[chunk][column][candidate].
//   k_bbfit_pick   one wave per column, lane = candidate: adds the partials in chunk order, takes the first candidate with the largest sum by a fixed
//                  butterfly, and writes the next round's candidate table (x, alpha, beta and the third bracket: once per candidate) or, after the last
//                  round, the result.
// The chunks are cut by the row count alone and added in their order, so the bits of rho and loglik do not depend on the grid, the memory space or the run.
//
// K_bbtest: P = min(1, sum of pmf(i) over all i in [0, n] with pmf(i) <= pmf(k) (1 + 1e-7)).  The pmf is unimodal, so the set is [0, jl] and [jr, n]: the mode
// comes from the ratio, jl and jr from binary searches of the log pmf on either side of it against log pmf(k) + log1p(1e-7), on the side of k as well (pmf values
// within 1e-7 of pmf(k) between k and the mode belong to the set).  jl >= jr: 1.  Two tiers by n against PHZ_BB_WAVE_N:
//   lane tier   one lane per cell; each tail is summed outward from its start index by the ratio recurrence until a term falls below 1e-18 of the running sum.
//               The tails are O(n) terms long where rho is large.
//   wave tier   the cells above the threshold are compacted into a list (gscan_excl) and taken one wave per cell.  Mode and searches run in every lane alike;
//               in a tail lane L of round r owns the PHZ_BB_WAVE_B consecutive indices that start (r 64 + L) PHZ_BB_WAVE_B from the tail's start, begins at
//               its own lgamma pmf and recurs through them; the lane sums are combined by a fixed xor butterfly (every lane holds the same bits after it) and
//               the tail ends with the first round that adds less than 1e-18 of the sum.
// The tiers do not agree bit for bit; each is held to the same tolerance (tests/test_ae_betabinom.py).
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "phz.h"
#include "phz_internal.h"
#include "phz_scan.h"

#ifndef PHZ_AETEST_GRID
#define PHZ_AETEST_GRID 2048        // most workgroups of a kernel here (grid-stride beyond), as in phz_aetest.hip
#endif
#ifndef PHZ_BB_WAVE_N
#define PHZ_BB_WAVE_N 8192          // cells with n above this take the wave tier (A/B of 512, 2048, 8192, 32768 and no wave tier at scale: DESIGN.md)
#endif
#ifndef PHZ_BB_WAVE_B
#define PHZ_BB_WAVE_B 16            // consecutive tail indices per lane and round of the wave tier
#endif

namespace {

constexpr int THREADS = 256;
constexpr int BB_G = PHZ_BB_FIT_CANDIDATES, BB_R = PHZ_BB_FIT_ROUNDS;
constexpr int FIT_TILE = 8;           // rows of a tile of k_bbfit_eval
constexpr int FIT_CHUNK = 256;        // rows of a chunk: the shape of the reduction tree, fixed
static_assert(BB_G == 64, "a lane of k_bbfit_pick is a candidate");

__device__ __host__ __forceinline__ double bb_rho_max(double p0) { const double m = p0 < 1.0 - p0 ? p0 : 1.0 - p0; return m / (1.0 + m); }

// ------------------------------------------------------------------------------------------------ K_bbfit
// candidate table: [4][BB_G][n_cols] doubles -- x = ln rho, alpha, beta, lgamma(alpha+beta) - lgamma(alpha) - lgamma(beta)
struct FitArgs {
    int64_t n_rows, n_cols, n_chunks, n_colblk;
    const int32_t *a, *b;
    double p0;
    int32_t min_cov;
    double *cand;
    double *partial;            // [n_chunks][n_cols][BB_G]
    uint32_t *used;             // [n_chunks][n_cols]
    double *rho_out, *loglik_out;
    int64_t *n_used_out;
};

// candidate g of the bracket [lo, hi] of column c
__device__ __forceinline__ void bb_candidate(const FitArgs &a, int64_t c, int g, double lo, double hi) {
    const double x = g == BB_G - 1 ? hi : lo + (hi - lo) * ((double)g / (double)(BB_G - 1));
    double rho = exp(x);
    const double top = bb_rho_max(a.p0);
    rho = rho < PHZ_BB_RHO_MIN ? PHZ_BB_RHO_MIN : (rho > top ? top : rho);          // exp(log(.)) may step an ulp outside the domain
    const double s = (1.0 - rho) / rho, al = a.p0 * s, be = (1.0 - a.p0) * s;
    const int64_t plane = (int64_t)BB_G * a.n_cols, at = (int64_t)g * a.n_cols + c;
    a.cand[at] = x; a.cand[plane + at] = al; a.cand[2 * plane + at] = be; a.cand[3 * plane + at] = lgamma(al + be) - lgamma(al) - lgamma(be);
}

__global__ __launch_bounds__(THREADS) void k_bbfit_init(FitArgs a) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.n_cols * BB_G) return;
    bb_candidate(a, i % a.n_cols, (int)(i / a.n_cols), log(PHZ_BB_RHO_MIN), log(bb_rho_max(a.p0)));
}

__global__ __launch_bounds__(64) void k_bbfit_eval(FitArgs a) {
    // every lane reads and writes its own column of these arrays alone: no barrier
    __shared__ int32_t s_k[FIT_TILE][64], s_m[FIT_TILE][64];
    __shared__ double s_c0[FIT_TILE][64];
    __shared__ double s_acc[BB_G][64];
    const int lane = threadIdx.x;
    const int32_t least = a.min_cov > 1 ? a.min_cov : 1;
    const int64_t plane = (int64_t)BB_G * a.n_cols, n_items = a.n_chunks * a.n_colblk;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t chunk = item / a.n_colblk, c = (item % a.n_colblk) * 64 + lane;
        if (c >= a.n_cols) continue;
        for (int g = 0; g < BB_G; g++) s_acc[g][lane] = 0.0;
        uint32_t used = 0;
        const int64_t r0 = chunk * FIT_CHUNK, r1 = r0 + FIT_CHUNK < a.n_rows ? r0 + FIT_CHUNK : a.n_rows;
        for (int64_t rt = r0; rt < r1; rt += FIT_TILE) {
            const int nt = (int)(r1 - rt < FIT_TILE ? r1 - rt : FIT_TILE);
            int live = 0;
            for (int j = 0; j < nt; j++) {
                const int32_t x = a.a[(rt + j) * a.n_cols + c], y = a.b[(rt + j) * a.n_cols + c];
                const bool tested = x >= 0 && y >= 0 && x + y >= least;          // x + y fits: checked on the host for PHZ_HOST, the caller's guarantee for PHZ_DEVICE
                s_k[j][lane] = tested ? x : -1; s_m[j][lane] = y;
                if (tested) {
                    s_c0[j][lane] = lgamma((double)x + (double)y + 1.0) - lgamma((double)x + 1.0) - lgamma((double)y + 1.0);
                    live++;
                }
            }
            if (!live) continue;
            used += (uint32_t)live;
            for (int g = 0; g < BB_G; g++) {
                const int64_t at = (int64_t)g * a.n_cols + c;
                const double al = a.cand[plane + at], be = a.cand[2 * plane + at], cc = a.cand[3 * plane + at], ab = al + be;
                double acc = s_acc[g][lane];
                for (int j = 0; j < nt; j++) {
                    if (s_k[j][lane] < 0) continue;
                    const double k = (double)s_k[j][lane], m = (double)s_m[j][lane];
                    acc += (lgamma(k + al) + lgamma(m + be) - lgamma(k + m + ab) + cc) + s_c0[j][lane];
                }
                s_acc[g][lane] = acc;
            }
        }
        double *out = a.partial + (chunk * a.n_cols + c) * BB_G;
        for (int g = 0; g < BB_G; g++) out[g] = s_acc[g][lane];
        a.used[chunk * a.n_cols + c] = used;
    }
}

__global__ __launch_bounds__(64) void k_bbfit_pick(FitArgs a, int last) {
    const int lane = threadIdx.x;
    for (int64_t c = blockIdx.x; c < a.n_cols; c += gridDim.x) {
        double ll = 0.0;
        int64_t used = 0;
        for (int64_t ch = 0; ch < a.n_chunks; ch++) { ll += a.partial[(ch * a.n_cols + c) * BB_G + lane]; used += a.used[ch * a.n_cols + c]; }
        // the first candidate with the largest sum: every lane ends with the same pair
        double best = ll; int idx = lane;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double ov = __shfl_xor(best, d); const int oi = __shfl_xor(idx, d);
            if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
        }
        const double x = a.cand[(int64_t)idx * a.n_cols + c];
        if (last) {
            if (lane == 0) {
                const double top = bb_rho_max(a.p0);
                double rho = exp(x);
                rho = rho < PHZ_BB_RHO_MIN ? PHZ_BB_RHO_MIN : (rho > top ? top : rho);
                a.rho_out[c] = used ? rho : __builtin_nan(""); a.loglik_out[c] = used ? best : __builtin_nan(""); a.n_used_out[c] = used;
            }
        } else {
            const double lo = a.cand[(int64_t)(idx > 0 ? idx - 1 : 0) * a.n_cols + c], hi = a.cand[(int64_t)(idx < BB_G - 1 ? idx + 1 : BB_G - 1) * a.n_cols + c];
            // Every lane must have read the old table before any lane overwrites it.  On the hardware that order is no barrier's doing: the column belongs to
            // this one wave, its lanes execute one instruction stream, and the stores below need lo and hi, so the loads above have returned for all lanes
            // before the first store issues.  The ballot adds nothing there; it is the rendezvous that the host emulation's fibres need (one fibre per lane).
            (void)__ballot(1);
            bb_candidate(a, c, lane, lo, hi);
        }
    }
}

// ------------------------------------------------------------------------------------------------ K_bbtest
struct TestArgs {
    int64_t n_cells, n_cols;
    const int32_t *a, *b;
    const double *rho;
    double p0, log_tol;           // log1p(1e-7)
    int32_t min_cov;
    double *par;                  // [3][n_cols]: alpha (NaN: the column is not tested), beta, lgamma(alpha+beta) - lgamma(alpha) - lgamma(beta)
    double *pvalue;
    uint32_t *flag, *pos, *list;  // 1 = wave tier; exclusive scan of flag, pos[n_cells] = cells of the wave tier; their indices
};

__global__ __launch_bounds__(THREADS) void k_bbtest_colpar(TestArgs g) {
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= g.n_cols) return;
    const double rho = g.rho[c];
    double al = __builtin_nan(""), be = al, cc = al;
    if (rho >= PHZ_BB_RHO_MIN && rho <= bb_rho_max(g.p0)) {          // false for NaN; outside the domain (PHZ_DEVICE callers alone): not tested either
        const double s = (1.0 - rho) / rho;
        al = g.p0 * s; be = (1.0 - g.p0) * s; cc = lgamma(al + be) - lgamma(al) - lgamma(be);
    }
    g.par[c] = al; g.par[g.n_cols + c] = be; g.par[2 * g.n_cols + c] = cc;
}

struct BbCell {
    double n, alpha, beta, base;          // base = lgamma(n+1) - lgamma(n+alpha+beta) + the column's bracket
    int32_t n_int;
};
__device__ __forceinline__ BbCell bb_cell(const TestArgs &g, int64_t t, int32_t n_int) {
    const int64_t c = t % g.n_cols;
    BbCell q;
    q.n_int = n_int; q.n = (double)n_int; q.alpha = g.par[c]; q.beta = g.par[g.n_cols + c];
    q.base = lgamma(q.n + 1.0) - lgamma(q.n + (q.alpha + q.beta)) + g.par[2 * g.n_cols + c];
    return q;
}
__device__ __forceinline__ double bb_lp(const BbCell &q, double i) {
    return q.base - lgamma(i + 1.0) - lgamma(q.n - i + 1.0) + lgamma(i + q.alpha) + lgamma(q.n - i + q.beta);
}
// pmf(i+1) / pmf(i) = bb_up(i) / bb_dn(i)
__device__ __forceinline__ double bb_up(const BbCell &q, double i) { return (q.n - i) * (i + q.alpha); }
__device__ __forceinline__ double bb_dn(const BbCell &q, double i) { return (i + 1.0) * (q.n - i - 1.0 + q.beta); }

// an index m with pmf(i+1) >= pmf(i) for i < m and pmf(i+1) <= pmf(i) for i >= m: the ratio is >= 1 exactly for i <= (n (alpha-1) + 1 - beta) / (alpha + beta - 2);
// the quotient places m, the ratio itself settles it
__device__ __forceinline__ int32_t bb_mode(const BbCell &q) {
    const double den = q.alpha + q.beta - 2.0;
    const double t = den > 0.0 ? (q.n * (q.alpha - 1.0) + 1.0 - q.beta) / den : 0.5 * q.n;
    int32_t m = t < 0.0 ? 0 : (t >= q.n ? q.n_int : (int32_t)t + 1);
    if (m > q.n_int) m = q.n_int;
    while (m < q.n_int && bb_up(q, (double)m) > bb_dn(q, (double)m)) m++;
    while (m > 0 && bb_up(q, (double)m - 1.0) < bb_dn(q, (double)m - 1.0)) m--;
    return m;
}

// jl = the largest i <= mode with log pmf(i) <= thr (-1: none), jr = the smallest i >= mode with log pmf(i) <= thr (n + 1: none)
__device__ __forceinline__ void bb_bounds(const BbCell &q, int32_t k, int32_t mode, double thr, int32_t *jl, int32_t *jr) {
    int32_t lo, hi;
    // left of the mode the pmf does not fall with i
    lo = k <= mode ? k : 0; hi = mode;
    if (k <= mode || bb_lp(q, 0.0) <= thr) {
        while (lo < hi) { const int32_t mid = lo + (hi - lo + 1) / 2; if (bb_lp(q, (double)mid) <= thr) lo = mid; else hi = mid - 1; }
        *jl = lo;
    } else {
        *jl = -1;
    }
    // right of it the pmf does not rise
    lo = mode; hi = k >= mode ? k : q.n_int;
    if (k >= mode || bb_lp(q, q.n) <= thr) {
        while (lo < hi) { const int32_t mid = lo + (hi - lo) / 2; if (bb_lp(q, (double)mid) <= thr) hi = mid; else lo = mid + 1; }
        *jr = lo;
    } else {
        *jr = q.n_int + 1;
    }
}

// pmf(start) + pmf(start - 1) + ... : pmf(i - 1) = pmf(i) * i (n - i + beta) / ((n - i + 1)(i - 1 + alpha))
__device__ __forceinline__ double bb_step_down(const BbCell &q, double i) { return i * (q.n - i + q.beta) / ((q.n - i + 1.0) * (i - 1.0 + q.alpha)); }
// pmf(start) + pmf(start + 1) + ... : pmf(i + 1) = pmf(i) * (n - i)(i + alpha) / ((i + 1)(n - i - 1 + beta))
__device__ __forceinline__ double bb_step_up(const BbCell &q, double i) { return bb_up(q, i) / bb_dn(q, i); }

__device__ __forceinline__ double bb_tail_down(const BbCell &q, int32_t start, double term) {
    double sum = term;
    for (int32_t i = start; i > 0 && term > 1e-18 * sum; i--) { term *= bb_step_down(q, (double)i); sum += term; }
    return sum;
}
__device__ __forceinline__ double bb_tail_up(const BbCell &q, int32_t start, double term) {
    double sum = term;
    for (int32_t i = start; i < q.n_int && term > 1e-18 * sum; i++) { term *= bb_step_up(q, (double)i); sum += term; }
    return sum;
}

__device__ __forceinline__ double bb_two_sided_lane(const BbCell &q, int32_t k, double log_tol) {
    const int32_t mode = bb_mode(q);
    const double lk = bb_lp(q, (double)k);
    int32_t jl, jr;
    bb_bounds(q, k, mode, lk + log_tol, &jl, &jr);
    if (jl >= jr) return 1.0;
    double P = 0.0;
    if (jl >= 0) P += bb_tail_down(q, jl, exp(jl == k ? lk : bb_lp(q, (double)jl)));
    if (jr <= q.n_int) P += bb_tail_up(q, jr, exp(jr == k ? lk : bb_lp(q, (double)jr)));
    return P < 1.0 ? P : 1.0;
}

__device__ __forceinline__ double bb_wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}
// dir = -1: pmf(start) + pmf(start - 1) + ... + pmf(0); dir = +1: ... + pmf(n).  Called by all 64 lanes with the same arguments; the same bits return in each.
__device__ __forceinline__ double bb_tail_wave(const BbCell &q, int32_t start, int dir, int lane) {
    double total = 0.0;
    const int64_t room = dir < 0 ? (int64_t)start : (int64_t)q.n_int - start;          // indices beyond the start
    for (int64_t first = 0; first <= room; first += 64 * PHZ_BB_WAVE_B) {
        const int64_t off = first + (int64_t)lane * PHZ_BB_WAVE_B;
        double sum = 0.0;
        if (off <= room) {
            const int64_t left = room - off;          // indices of the tail beyond this lane's first
            const int steps = (int)(left < PHZ_BB_WAVE_B - 1 ? left : PHZ_BB_WAVE_B - 1);
            double i = (double)start + (double)dir * (double)off;
            double term = exp(bb_lp(q, i));
            sum = term;
            for (int s = 0; s < steps; s++) {
                term *= dir < 0 ? bb_step_down(q, i) : bb_step_up(q, i);
                i += (double)dir;
                sum += term;
            }
        }
        const double round = bb_wave_sum(sum);
        total += round;
        if (!(round > 1e-18 * total)) break;
    }
    return total;
}

__device__ __forceinline__ bool bb_tested(const TestArgs &g, int64_t t, int32_t *k, int32_t *n) {
    const int32_t a = g.a[t], b = g.b[t];
    if (a < 0 || b < 0) return false;
    *k = a; *n = a + b;          // fits: checked on the host for PHZ_HOST, the caller's guarantee for PHZ_DEVICE
    if (*n < (g.min_cov > 1 ? g.min_cov : 1)) return false;
    const double al = g.par[t % g.n_cols];
    return al == al;
}

__global__ __launch_bounds__(THREADS) void k_bbtest_lane(TestArgs g) {
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < g.n_cells; t += (int64_t)gridDim.x * THREADS) {
        int32_t k, n;
        double p = __builtin_nan("");
        uint32_t wave = 0;
        if (bb_tested(g, t, &k, &n)) {
            if (n > PHZ_BB_WAVE_N) wave = 1;
            else p = bb_two_sided_lane(bb_cell(g, t, n), k, g.log_tol);
        }
        g.flag[t] = wave; g.pvalue[t] = p;
    }
}

__global__ __launch_bounds__(THREADS) void k_bbtest_list(TestArgs g) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t < g.n_cells && g.flag[t]) g.list[g.pos[t]] = (uint32_t)t;
}

__global__ __launch_bounds__(THREADS) void k_bbtest_wave(TestArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t count = g.pos[g.n_cells], n_waves = (int64_t)gridDim.x * (THREADS / 64);
    for (int64_t w = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); w < count; w += n_waves) {
        const int64_t t = g.list[w];
        const int32_t k = g.a[t], n = k + g.b[t];
        const BbCell q = bb_cell(g, t, n);
        const int32_t mode = bb_mode(q);
        const double lk = bb_lp(q, (double)k);
        int32_t jl, jr;
        bb_bounds(q, k, mode, lk + g.log_tol, &jl, &jr);
        double P = 1.0;
        if (jl < jr) {          // the same in every lane
            P = 0.0;
            if (jl >= 0) P += bb_tail_wave(q, jl, -1, lane);
            if (jr <= n) P += bb_tail_wave(q, jr, +1, lane);
            P = P < 1.0 ? P : 1.0;
        }
        if (lane == 0) g.pvalue[t] = P;
    }
}

void record_ms(phz_ctx *ctx, int slot) {
    (void)hipEventSynchronize(ctx->ev1);
    float ms = 0; (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->last_ms[slot] = ms; ctx->total_ms[slot] += ms; ctx->launches[slot]++;
}

// the argument errors both entry points share; n_cells is set when they pass
int check_matrix(phz_ctx *ctx, const char *who, int64_t n_rows, int64_t n_cols, const int32_t *a, const int32_t *b, double p0, int space, int64_t *n_cells) {
    char msg[160];
    if (!(p0 > 0.0 && p0 < 1.0)) { snprintf(msg, sizeof msg, "%s: p0 must lie strictly between 0 and 1", who); return phz_fail(ctx, PHZ_E_ARG, msg); }
    if (n_cols && n_rows > (int64_t)INT32_MAX / n_cols) { snprintf(msg, sizeof msg, "%s: more than 2^31 - 1 cells", who); return phz_fail(ctx, PHZ_E_ARG, msg); }
    *n_cells = n_rows * n_cols;
    if (*n_cells && (!a || !b)) return PHZ_E_ARG;
    if (space == PHZ_HOST)
        for (int64_t t = 0; t < *n_cells; t++)
            if (a[t] >= 0 && b[t] >= 0 && (int64_t)a[t] + (int64_t)b[t] > INT32_MAX) { snprintf(msg, sizeof msg, "%s: a + b does not fit in int32", who); return phz_fail(ctx, PHZ_E_ARG, msg); }
    return PHZ_OK;
}

}  // namespace

extern "C" int phz_betabinom_fit(phz_ctx *ctx, int64_t n_rows, int64_t n_cols, const int32_t *a, const int32_t *b, double p0, int32_t min_cov, double *rho_out,
                                 double *loglik_out, int64_t *n_used_out, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_rows < 0 || n_cols < 0 || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    int64_t n = 0;
    if (int s = check_matrix(ctx, "phz_betabinom_fit", n_rows, n_cols, a, b, p0, space, &n)) return s;
    if (n_cols == 0) return PHZ_OK;
    if (!rho_out || !loglik_out || !n_used_out) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    FitArgs g;
    g.n_rows = n_rows; g.n_cols = n_cols; g.n_chunks = (n_rows + FIT_CHUNK - 1) / FIT_CHUNK; g.n_colblk = (n_cols + 63) / 64; g.p0 = p0; g.min_cov = min_cov;
    if (int s = st.in(a, (size_t)n, space, &g.a)) return s;
    if (int s = st.in(b, (size_t)n, space, &g.b)) return s;
    if (int s = st.out(rho_out, (size_t)n_cols, space, &g.rho_out)) return s;
    if (int s = st.out(loglik_out, (size_t)n_cols, space, &g.loglik_out)) return s;
    if (int s = st.out(n_used_out, (size_t)n_cols, space, &g.n_used_out)) return s;
    DevBuf *S = ctx->scratch;
    const size_t per_chunk = (size_t)n_cols * (size_t)(g.n_chunks ? g.n_chunks : 1);
    if (int s = reserve_all(ctx, {{S[SC_BB_CAND], (size_t)n_cols * BB_G * 4 * 8}, {S[SC_BB_PARTIAL], per_chunk * BB_G * 8}, {S[SC_BB_USED], per_chunk * 4}})) return s;
    g.cand = (double *)S[SC_BB_CAND].p; g.partial = (double *)S[SC_BB_PARTIAL].p; g.used = (uint32_t *)S[SC_BB_USED].p;
    hipStream_t sm = ctx->stream;
    const int64_t n_items = g.n_chunks * g.n_colblk;
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_BBFIT: the candidate table and the launches of all rounds
    hipLaunchKernelGGL(k_bbfit_init, dim3(nblk(n_cols * BB_G)), dim3(THREADS), 0, sm, g);
    for (int round = 0; round < BB_R; round++) {          // no host wait between the rounds
        if (n_items) hipLaunchKernelGGL(k_bbfit_eval, dim3((unsigned)std::min<int64_t>(n_items, (int64_t)PHZ_AETEST_GRID)), dim3(64), 0, sm, g);
        hipLaunchKernelGGL(k_bbfit_pick, dim3((unsigned)std::min<int64_t>(n_cols, (int64_t)PHZ_AETEST_GRID)), dim3(64), 0, sm, g, round == BB_R - 1 ? 1 : 0);
    }
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    record_ms(ctx, PHZ_T_BBFIT);
    if (space == PHZ_HOST) {
        PHZ_HIP(ctx, hipMemcpyAsync(rho_out, g.rho_out, (size_t)n_cols * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(loglik_out, g.loglik_out, (size_t)n_cols * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(n_used_out, g.n_used_out, (size_t)n_cols * 8, hipMemcpyDeviceToHost, sm));
    }
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}

extern "C" int phz_betabinom_test(phz_ctx *ctx, int64_t n_rows, int64_t n_cols, const int32_t *a, const int32_t *b, double p0, const double *rho, int32_t min_cov,
                                  double *pvalue, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_rows < 0 || n_cols < 0 || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    int64_t n = 0;
    if (int s = check_matrix(ctx, "phz_betabinom_test", n_rows, n_cols, a, b, p0, space, &n)) return s;
    if (n_cols && !rho) return PHZ_E_ARG;
    if (space == PHZ_HOST)
        for (int64_t c = 0; c < n_cols; c++)
            if (rho[c] == rho[c] && !(rho[c] >= PHZ_BB_RHO_MIN && rho[c] <= bb_rho_max(p0)))
                return phz_fail(ctx, PHZ_E_ARG, "phz_betabinom_test: rho must lie in [1e-6, m / (1 + m)], m = min of p0 and 1 - p0");
    if (n == 0) return PHZ_OK;
    if (!pvalue) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    TestArgs g;
    g.n_cells = n; g.n_cols = n_cols; g.p0 = p0; g.log_tol = log1p(1e-7); g.min_cov = min_cov;
    if (int s = st.in(a, (size_t)n, space, &g.a)) return s;
    if (int s = st.in(b, (size_t)n, space, &g.b)) return s;
    if (int s = st.in(rho, (size_t)n_cols, space, &g.rho)) return s;
    if (int s = st.out(pvalue, (size_t)n, space, &g.pvalue)) return s;
    DevBuf *S = ctx->scratch;
    if (int s = reserve_all(ctx, {{S[SC_BB_COLPAR], (size_t)n_cols * 3 * 8}, {S[SC_BB_FLAG], (size_t)n * 4}, {S[SC_BB_POS], ((size_t)n + 1) * 4}, {S[SC_BB_LIST], (size_t)n * 4}})) return s;
    g.par = (double *)S[SC_BB_COLPAR].p; g.flag = (uint32_t *)S[SC_BB_FLAG].p; g.pos = (uint32_t *)S[SC_BB_POS].p; g.list = (uint32_t *)S[SC_BB_LIST].p;
    hipStream_t sm = ctx->stream;
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_BBTEST: column parameters, lane tier, compaction, wave tier
    hipLaunchKernelGGL(k_bbtest_colpar, dim3(nblk(n_cols)), dim3(THREADS), 0, sm, g);
    hipLaunchKernelGGL(k_bbtest_lane, dim3((unsigned)std::min<int64_t>(nblk(n), (int64_t)PHZ_AETEST_GRID)), dim3(THREADS), 0, sm, g);
    if (int s = gscan_excl<uint32_t, uint32_t>(ctx, g.flag, g.pos, n, S[SC_BB_SCAN_TMP])) return s;
    hipLaunchKernelGGL(k_bbtest_list, dim3(nblk(n)), dim3(THREADS), 0, sm, g);
    // the number of listed cells is known to the device alone: a wave per listed cell at most, the rest of the grid returns at once
    hipLaunchKernelGGL(k_bbtest_wave, dim3((unsigned)std::min<int64_t>((n + THREADS / 64 - 1) / (THREADS / 64), (int64_t)PHZ_AETEST_GRID)), dim3(THREADS), 0, sm, g);
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    record_ms(ctx, PHZ_T_BBTEST);
    if (space == PHZ_HOST) PHZ_HIP(ctx, hipMemcpyAsync(pvalue, g.pvalue, (size_t)n * 8, hipMemcpyDeviceToHost, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}
