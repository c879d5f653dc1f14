// K_blnfit and K_blntest: the population statistics of phaser_ae_outlier (include/phz.h, phz_bln_fit and phz_bln_test; DESIGN.md, "K_blnfit and K_blntest").
// The model is a logit-normal mixture of binomials: with mu0 = logit(p0), x ~ N(mu0, s^2) and k | x ~ Binomial(n, sigma(x)),
//   pmf(k; n, s) = C(n, k) * integral of sigma(x)^k (1 - sigma(x))^(n-k) phi((x - mu0) / s) / s dx,      PHZ_BLN_S_MIN <= s <= PHZ_BLN_S_MAX.
// Everything in fp64.
//
// The integrals.  Every integrand here is log-concave in x.  A safeguarded Newton iteration finds the mode xm of its log h, the curvature there gives the
// width wl = 1 / sqrt(-h''(xm)), and a Gauss-Hermite rule of PHZ_BLN_Q nodes t_i (weights folded with exp(t_i^2) into v_i, phz_bln_nodes.h) is laid over it:
//   integral of exp(h) = exp(h(xm)) sqrt(2) wl * sum of v_i exp(h(xm + sqrt(2) wl t_i) - h(xm)).
// The centre and the width only place the rule: Newton stops at a step of 1e-5 widths.
//   pmf      h = k log sigma + (n - k) log(1 - sigma) - (x - mu0)^2 / 2 s^2, Newton from mu0.
//   tails    lower = P(X <= k); the upper tail is the lower tail of (n - k, -mu0); k = n gives lower = 1.  Three tiers:
//     sum      n <= PHZ_BLN_SUM_N: the pmf summed over the tail.
//     form A   integral of BinCDF(k; n, sigma(x)) phi((x - mu0) / s) / s.  d/dx BinCDF = -g, g(x) = (n - k) C(n, k) sigma^(k+1) (1 - sigma)^(n-k) the density of
//              logit Beta(k + 1, n - k), which gives Newton its derivatives.  log BinCDF at a node: K_binom's outward ratio recurrence from k down where
//              k <= n sigma, from k + 1 up with the complement taken where it is above (k = 0 is the closed form (1 - sigma)^n: the recurrence has no term).
//     form B   the same tail integrated by parts: integral of Phi((x - mu0) / s) g(x); log Phi through erfc, beyond u = 25 through the asymptotic series.
//     Each form fails where its cumulative factor is a step across the density factor: with w = 1 / sqrt((n + 1) pm (1 - pm)), pm = (k + 1) / (n + 1),
//     form A is taken when w > s and form B otherwise.
//   two-sided  the tail on the side of k (lower when k <= n p0) first; when it is at most 0.5 the other is at least 0.5 (they add up to 1 + pmf(k)) and is
//     not taken.
//
// K_blnfit: one wave per row, lane = candidate.  A pre-pass counts the row's tested cells and adds their log C(n, k), lane L taking the columns L, L + 64, ...;
// a fixed xor butterfly combines the lanes.  Then the four rounds run in this one launch: every lane walks the row's cells in ascending column order (all lanes
// read the same cell: the load is uniform) and keeps the running sum of its candidate in a register; the first candidate with the largest sum is picked by
// a fixed xor butterfly and the next bracket is read from the neighbours' lanes.  No partials table, no atomics: the bits depend on the inputs alone.
//
// K_blntest: one lane per cell, grid-stride over at most PHZ_AETEST_GRID workgroups.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "phz.h"
#include "phz_internal.h"

#ifndef PHZ_AETEST_GRID
#define PHZ_AETEST_GRID 2048        // most workgroups of a kernel here (grid-stride beyond), as in phz_aetest.hip
#endif
#ifndef PHZ_BLN_Q
#define PHZ_BLN_Q 32                // nodes of the Gauss-Hermite rule (phz_bln_nodes.h holds 16, 24, 32, 48 and 64)
#endif
#ifndef PHZ_BLN_SUM_N
#define PHZ_BLN_SUM_N 64            // cells with n up to this sum the pmf over the tail; above, the tail is one integral
#endif

namespace {

#include "phz_bln_nodes.h"

constexpr int THREADS = 256;
constexpr int BLN_G = PHZ_BLN_FIT_CANDIDATES, BLN_R = PHZ_BLN_FIT_ROUNDS;
static_assert(BLN_G == 64, "a lane of k_blnfit is a candidate");
constexpr double BLN_SQRT2 = 1.4142135623730951, BLN_INV_SQRT_PI = 0.56418958354775629, BLN_INV_SQRT_2PI = 0.3989422804014327;
constexpr int BLN_NEWTON = 60;      // Newton steps at most (a bisection step where Newton leaves the bracket)

// sigma(x), 1 - sigma(x), their logs and their product, from one exp and one log1p
struct BlnSig { double p, q, lp, lq, pq; };
__device__ __forceinline__ BlnSig bln_sig(double x) {
    const double e = exp(-fabs(x)), d = 1.0 / (1.0 + e), sp = log1p(e);
    BlnSig r;
    r.p = x >= 0.0 ? d : e * d; r.q = x >= 0.0 ? e * d : d;
    r.lp = (x < 0.0 ? x : 0.0) - sp; r.lq = (x > 0.0 ? -x : 0.0) - sp;
    r.pq = e * d * d;
    return r;
}

// A functor F gives F.at(x, &d1, &d2) = h(x), with d1 = h'(x) and d2 = -h''(x) > 0.
// -> the mode of h by Newton from x0, *d2_out = -h'' there, *h_out = h there
template <class F> __device__ __forceinline__ double bln_mode(const F &f, double x0, double tol, double *h_out, double *d2_out) {
    double x = x0, lo = -INFINITY, hi = INFINITY, d1, d2, h = 0.0;
    for (int it = 0; it < BLN_NEWTON; it++) {
        h = f.at(x, &d1, &d2);
        if (d1 > 0.0) lo = x; else hi = x;
        const double dx = d1 / d2;
        if (fabs(dx) * sqrt(d2) < tol || it == BLN_NEWTON - 1) break;          // h, d2 stay those of x: the rule is laid there
        double xn = x + dx;
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);          // the step went beyond the far end of the bracket, which is finite then, as the near one is
        if (!(xn > lo && xn < hi)) break;                         // no double between the ends
        x = xn;
    }
    *h_out = h; *d2_out = d2;
    return x;
}

// -> log of the integral of exp(h) over the line
template <class F> __device__ __forceinline__ double bln_log_integral(const F &f, double x0, double tol) {
    double h0, d2, u1, u2;
    const double xm = bln_mode(f, x0, tol, &h0, &d2);
    const double wl = 1.0 / sqrt(d2), step = BLN_SQRT2 * wl;
    double acc = 0.0;
    for (int i = 0; i < PHZ_BLN_Q; i++) acc += BLN_V[i] * exp(f.at(xm + step * BLN_T[i], &u1, &u2) - h0);
    return h0 + log(step * acc);
}

// h = ka log sigma + kb log(1 - sigma) - (x - mu0)^2 / 2 s^2 - log(s sqrt(2 pi))
struct BlnPmf {
    double ka, kb, mu0, is2, lnorm;
    __device__ __forceinline__ double at(double x, double *d1, double *d2) const {
        const BlnSig g = bln_sig(x);
        const double n = ka + kb, dx = x - mu0;
        *d1 = ka - n * g.p - dx * is2; *d2 = n * g.pq + is2;
        return ka * g.lp + kb * g.lq - 0.5 * dx * dx * is2 + lnorm;
    }
};
// log of pmf / C(n, k)
__device__ __forceinline__ double bln_log_mix(double ka, double kb, double mu0, double s) {
    BlnPmf f; f.ka = ka; f.kb = kb; f.mu0 = mu0; f.is2 = 1.0 / (s * s); f.lnorm = -log(s) + log(BLN_INV_SQRT_2PI);
    return bln_log_integral(f, mu0, 1e-5);
}
__device__ __forceinline__ double bln_lchoose(double k, double m) { return lgamma(k + m + 1.0) - lgamma(k + 1.0) - lgamma(m + 1.0); }

// log Phi(z) and lambda = phi(z) / Phi(z)
__device__ __forceinline__ double bln_log_phi(double z, double *lambda) {
    if (z >= 0.0) {
        const double t = 0.5 * erfc(z * 0.70710678118654752), P = 1.0 - t;
        *lambda = BLN_INV_SQRT_2PI * exp(-0.5 * z * z) / P;
        return log1p(-t);
    }
    const double u = -z * 0.70710678118654752;
    if (u < 25.0) {
        const double P = 0.5 * erfc(u);
        *lambda = BLN_INV_SQRT_2PI * exp(-u * u) / P;
        return log(P);
    }
    // erfc(u) exp(u^2) = (1 / (u sqrt(pi))) (1 - 1/(2u^2) + 3/(4u^4) - 15/(8u^6) + 105/(16u^8) - 945/(32u^10) + 10395/(64u^12)): below 3e-15 of it at u = 25
    const double v = 1.0 / (u * u);
    const double ex = BLN_INV_SQRT_PI / u * (1.0 + v * (-0.5 + v * (0.75 + v * (-1.875 + v * (6.5625 + v * (-29.53125 + v * 162.421875))))));
    *lambda = 2.0 * BLN_INV_SQRT_2PI / ex;
    return log(0.5 * ex) - u * u;
}

// form A: h = log BinCDF(k; n, sigma(x)) - (x - mu0)^2 / 2 s^2 - log(s sqrt(2 pi)), k < n
struct BlnFormA {
    double k, n, lc, mu0, is2, lnorm;          // lc = log C(n, k)
    __device__ __forceinline__ double at(double x, double *d1, double *d2) const {
        const BlnSig g = bln_sig(x);
        const double lpk = lc + k * g.lp + (n - k) * g.lq, dx = x - mu0;          // log pmf(k) of Binomial(n, sigma)
        double lF, hz;                                                            // log BinCDF and g / BinCDF
        if (k <= n * g.p) {
            // pmf(i - 1) / pmf(i) = i q / ((n - i + 1) p), below 1 here
            const double r = g.q / g.p;
            double term = 1.0, sum = 1.0;
            for (double i = k; i > 0.0 && term > 1e-17 * sum; i -= 1.0) { term *= i * r / (n - i + 1.0); sum += term; }
            lF = lpk + log(sum); hz = (n - k) * g.p / sum;
        } else {
            // the complement: pmf(i + 1) / pmf(i) = (n - i) p / ((i + 1) q), below 1 here
            const double r = g.p / g.q;
            double term = (n - k) * r / (k + 1.0), sum = term;
            for (double i = k + 1.0; i < n && term > 1e-17 * sum; i += 1.0) { term *= (n - i) * r / (i + 1.0); sum += term; }
            const double pk = exp(lpk), S = pk * sum;
            lF = log1p(-S); hz = (n - k) * g.p * pk / (1.0 - S);
        }
        const double c = hz * (k + 1.0 - (n + 1.0) * g.p + hz);          // -(log BinCDF)'': not negative
        *d1 = -hz - dx * is2; *d2 = (c > 0.0 ? c : 0.0) + is2;
        return lF - 0.5 * dx * dx * is2 + lnorm;
    }
};
// form B: h = log Phi((x - mu0) / s) + log g(x)
struct BlnFormB {
    double k1, m, lk, mu0, is;          // k1 = k + 1, m = n - k, lk = log((n - k) C(n, k))
    __device__ __forceinline__ double at(double x, double *d1, double *d2) const {
        const BlnSig g = bln_sig(x);
        const double z = (x - mu0) * is;
        double lam;
        const double lphi = bln_log_phi(z, &lam);
        const double c = lam * (z + lam);          // -(log Phi)'': not negative
        *d1 = lam * is + k1 - (k1 + m) * g.p; *d2 = (c > 0.0 ? c : 0.0) * is * is + (k1 + m) * g.pq;
        return lk + lphi + k1 * g.lp + m * g.lq;
    }
};

// P(X <= k) of the mixture centred at mu0 by one integral (n above PHZ_BLN_SUM_N)
__device__ __forceinline__ double bln_lower_integral(double k, double n, double mu0, double s) {
    if (k >= n) return 1.0;
    const double pm = (k + 1.0) / (n + 1.0), w = 1.0 / sqrt((n + 1.0) * pm * (1.0 - pm)), lc = bln_lchoose(k, n - k);
    double lt;
    if (w > s) {
        BlnFormA f; f.k = k; f.n = n; f.lc = lc; f.mu0 = mu0; f.is2 = 1.0 / (s * s); f.lnorm = -log(s) + log(BLN_INV_SQRT_2PI);
        lt = bln_log_integral(f, mu0, 1e-4);
    } else {
        BlnFormB f; f.k1 = k + 1.0; f.m = n - k; f.lk = lc + log(n - k); f.mu0 = mu0; f.is = 1.0 / s;
        lt = bln_log_integral(f, log(pm / (1.0 - pm)), 1e-5);
    }
    const double t = exp(lt);
    return t < 1.0 ? t : 1.0;
}
// P(X <= k) by the sum of the pmf (n up to PHZ_BLN_SUM_N)
__device__ __forceinline__ double bln_lower_sum(int32_t k, int32_t n, double mu0, double s) {
    if (k >= n) return 1.0;
    double t = 0.0;
    for (int32_t i = 0; i <= k; i++) t += exp(bln_lchoose((double)i, (double)(n - i)) + bln_log_mix((double)i, (double)(n - i), mu0, s));
    return t < 1.0 ? t : 1.0;
}
__device__ __forceinline__ double bln_lower(int32_t k, int32_t n, double mu0, double s) {
    return n <= PHZ_BLN_SUM_N ? bln_lower_sum(k, n, mu0, s) : bln_lower_integral((double)k, (double)n, mu0, s);
}
__device__ __forceinline__ double bln_two_sided(int32_t k, int32_t n, double p0, double mu0, double s) {
    const bool low_first = (double)k <= (double)n * p0;
    double t1 = 0.0;
    for (int pass = 0; pass < 2; pass++) {          // one copy of the tail code: the second pass is rare
        const bool low = (pass == 0) == low_first;
        const double t = bln_lower(low ? k : n - k, n, low ? mu0 : -mu0, s);
        if (pass == 0) {
            if (t <= 0.5) return 2.0 * t;          // the other tail is 1 + pmf(k) - t >= 0.5
            t1 = t;
        } else if (t < t1) {
            t1 = t;
        }
    }
    return t1 < 0.5 ? 2.0 * t1 : 1.0;
}

__device__ __forceinline__ double bln_clip_s(double s) { return s < PHZ_BLN_S_MIN ? PHZ_BLN_S_MIN : (s > PHZ_BLN_S_MAX ? PHZ_BLN_S_MAX : s); }

// ------------------------------------------------------------------------------------------------ K_blnfit
struct FitArgs {
    int64_t n_rows, n_cols;
    const int32_t *a, *b;
    double mu0;
    int32_t min_cov, min_samples;
    double *s_out, *loglik_out, *loglik_min_out;
    int64_t *n_used_out;
};

__global__ __launch_bounds__(64) void k_blnfit(FitArgs g) {
    const int lane = threadIdx.x;
    const int32_t least = g.min_cov > 1 ? g.min_cov : 1;
    for (int64_t row = blockIdx.x; row < g.n_rows; row += gridDim.x) {
        const int32_t *ra = g.a + row * g.n_cols, *rb = g.b + row * g.n_cols;
        // the tested cells and the sum of their log C(n, k): lane L takes the columns L, L + 64, ...; every lane ends with the same bits
        int used = 0;          // at most 2^31 - 1 cells
        double lcs = 0.0;
        for (int64_t c = lane; c < g.n_cols; c += 64) {
            const int32_t x = ra[c], y = rb[c];
            if (x >= 0 && y >= 0 && x + y >= least) { used++; lcs += bln_lchoose((double)x, (double)y); }          // x + y fits: checked on the host for PHZ_HOST, the caller's guarantee for PHZ_DEVICE
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { used += __shfl_xor(used, d); lcs += __shfl_xor(lcs, d); }
        if (used < g.min_samples) {
            if (lane == 0) { g.s_out[row] = g.loglik_out[row] = g.loglik_min_out[row] = __builtin_nan(""); g.n_used_out[row] = used; }
            continue;
        }
        double lo = log(PHZ_BLN_S_MIN), hi = log(PHZ_BLN_S_MAX), ll_min = 0.0;
        for (int round = 0; round < BLN_R; round++) {
            const double x = lane == BLN_G - 1 ? hi : lo + (hi - lo) * ((double)lane / (double)(BLN_G - 1));
            const double s = bln_clip_s(exp(x));          // exp(log(.)) may step an ulp outside the domain
            double ll = 0.0;
            for (int64_t c = 0; c < g.n_cols; c++) {
                const int32_t ka = ra[c], kb = rb[c];
                if (ka >= 0 && kb >= 0 && ka + kb >= least) ll += bln_log_mix((double)ka, (double)kb, g.mu0, s);
            }
            if (round == 0) ll_min = __shfl(ll, 0);
            // the first candidate with the largest sum: every lane ends with the same pair
            double best = ll; int idx = lane;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const double ov = __shfl_xor(best, d); const int oi = __shfl_xor(idx, d);
                if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
            }
            const double xb = __shfl(x, idx), xl = __shfl(x, idx > 0 ? idx - 1 : 0), xh = __shfl(x, idx < BLN_G - 1 ? idx + 1 : BLN_G - 1);
            if (round == BLN_R - 1) {
                if (lane == 0) { g.s_out[row] = bln_clip_s(exp(xb)); g.loglik_out[row] = best + lcs; g.loglik_min_out[row] = ll_min + lcs; g.n_used_out[row] = used; }
            } else {
                lo = xl; hi = xh;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ K_blntest
struct TestArgs {
    int64_t n_cells, n_rows, n_cols;
    const int32_t *a, *b;
    const double *s;
    double p0, mu0;
    int32_t min_cov;
    double *rowpar;               // [n_rows]: s, NaN where the row is not tested
    double *pvalue;
};

__global__ __launch_bounds__(THREADS) void k_blntest_rowpar(TestArgs g) {
    const int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (r >= g.n_rows) return;
    const double s = g.s[r];
    g.rowpar[r] = s >= PHZ_BLN_S_MIN && s <= PHZ_BLN_S_MAX ? s : __builtin_nan("");          // false for NaN; outside the domain (PHZ_DEVICE callers alone): not tested either
}

__global__ __launch_bounds__(THREADS) void k_blntest(TestArgs g) {
    const int32_t least = g.min_cov > 1 ? g.min_cov : 1;
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < g.n_cells; t += (int64_t)gridDim.x * THREADS) {
        const int32_t a = g.a[t], b = g.b[t];
        double p = __builtin_nan("");
        if (a >= 0 && b >= 0 && a + b >= least) {          // a + b fits: checked on the host for PHZ_HOST, the caller's guarantee for PHZ_DEVICE
            const double s = g.rowpar[t / g.n_cols];
            if (s == s) p = bln_two_sided(a, a + b, g.p0, g.mu0, s);
        }
        g.pvalue[t] = p;
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

extern "C" int phz_bln_fit(phz_ctx *ctx, int64_t n_rows, int64_t n_cols, const int32_t *a, const int32_t *b, double p0, int32_t min_cov, int32_t min_samples,
                           double *s_out, double *loglik_out, double *loglik_min_out, int64_t *n_used_out, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_rows < 0 || n_cols < 0 || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    if (min_samples < 1) return phz_fail(ctx, PHZ_E_ARG, "phz_bln_fit: min_samples must be at least 1");
    int64_t n = 0;
    if (int s = check_matrix(ctx, "phz_bln_fit", n_rows, n_cols, a, b, p0, space, &n)) return s;
    if (n_rows == 0) return PHZ_OK;
    if (!s_out || !loglik_out || !loglik_min_out || !n_used_out) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    FitArgs g;
    g.n_rows = n_rows; g.n_cols = n_cols; g.mu0 = log(p0) - log1p(-p0); g.min_cov = min_cov; g.min_samples = min_samples;
    if (int s = st.in(a, (size_t)n, space, &g.a)) return s;
    if (int s = st.in(b, (size_t)n, space, &g.b)) return s;
    if (int s = st.out(s_out, (size_t)n_rows, space, &g.s_out)) return s;
    if (int s = st.out(loglik_out, (size_t)n_rows, space, &g.loglik_out)) return s;
    if (int s = st.out(loglik_min_out, (size_t)n_rows, space, &g.loglik_min_out)) return s;
    if (int s = st.out(n_used_out, (size_t)n_rows, space, &g.n_used_out)) return s;
    hipStream_t sm = ctx->stream;
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_BLNFIT: the one launch
    hipLaunchKernelGGL(k_blnfit, dim3((unsigned)std::min<int64_t>(n_rows, (int64_t)PHZ_AETEST_GRID)), dim3(64), 0, sm, g);
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    record_ms(ctx, PHZ_T_BLNFIT);
    if (space == PHZ_HOST) {
        PHZ_HIP(ctx, hipMemcpyAsync(s_out, g.s_out, (size_t)n_rows * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(loglik_out, g.loglik_out, (size_t)n_rows * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(loglik_min_out, g.loglik_min_out, (size_t)n_rows * 8, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipMemcpyAsync(n_used_out, g.n_used_out, (size_t)n_rows * 8, hipMemcpyDeviceToHost, sm));
    }
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}

extern "C" int phz_bln_test(phz_ctx *ctx, int64_t n_rows, int64_t n_cols, const int32_t *a, const int32_t *b, double p0, const double *s, int32_t min_cov,
                            double *pvalue, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_rows < 0 || n_cols < 0 || (space != PHZ_HOST && space != PHZ_DEVICE)) return PHZ_E_ARG;
    int64_t n = 0;
    if (int st = check_matrix(ctx, "phz_bln_test", n_rows, n_cols, a, b, p0, space, &n)) return st;
    if (n_rows && !s) return PHZ_E_ARG;
    if (space == PHZ_HOST)
        for (int64_t r = 0; r < n_rows; r++)
            if (s[r] == s[r] && !(s[r] >= PHZ_BLN_S_MIN && s[r] <= PHZ_BLN_S_MAX)) return phz_fail(ctx, PHZ_E_ARG, "phz_bln_test: s must lie in [1e-3, 2]");
    if (n == 0) return PHZ_OK;
    if (!pvalue) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    Staging st(ctx);
    TestArgs g;
    g.n_cells = n; g.n_rows = n_rows; g.n_cols = n_cols; g.p0 = p0; g.mu0 = log(p0) - log1p(-p0); g.min_cov = min_cov;
    if (int e = st.in(a, (size_t)n, space, &g.a)) return e;
    if (int e = st.in(b, (size_t)n, space, &g.b)) return e;
    if (int e = st.in(s, (size_t)n_rows, space, &g.s)) return e;
    if (int e = st.out(pvalue, (size_t)n, space, &g.pvalue)) return e;
    DevBuf *S = ctx->scratch;
    if (int e = reserve_all(ctx, {{S[SC_BLN_ROWPAR], (size_t)n_rows * 8}})) return e;
    g.rowpar = (double *)S[SC_BLN_ROWPAR].p;
    hipStream_t sm = ctx->stream;
    (void)hipEventRecord(ctx->ev0, sm);                 // PHZ_T_BLNTEST: the row parameters and the cells
    hipLaunchKernelGGL(k_blntest_rowpar, dim3(nblk(n_rows)), dim3(THREADS), 0, sm, g);
    hipLaunchKernelGGL(k_blntest, dim3((unsigned)std::min<int64_t>(nblk(n), (int64_t)PHZ_AETEST_GRID)), dim3(THREADS), 0, sm, g);
    PHZ_HIP(ctx, hipGetLastError());
    (void)hipEventRecord(ctx->ev1, sm);
    record_ms(ctx, PHZ_T_BLNTEST);
    if (space == PHZ_HOST) PHZ_HIP(ctx, hipMemcpyAsync(pvalue, g.pvalue, (size_t)n * 8, hipMemcpyDeviceToHost, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}
