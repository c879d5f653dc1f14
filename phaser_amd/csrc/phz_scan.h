// Device-wide exclusive scan written for this library (no rocPRIM / hipCUB): gscan_excl, TI -> TO with an optional transform of the input on load.  One launch
// (decoupled look-back) for 32-bit sums below 4 Mi elements, three launches from there on and for 64-bit sums.  Every device scan of the library goes through it, except those of phz_bamdev.hip (see there).
// Header-only: every translation unit that needs it gets its own copy of the kernels.  The per-ctx state of the one-launch path (phz_ctx::scan_state, scan_epoch,
// scan_ticket_base) is shared by all of them: gscan_excl launches on ctx->stream and expects the calling host thread to be the only one inside the ctx (PhzEnter).
// Tested directly by tests/test_scan.py (phz_selftest_scan, against a host cumulative sum; emulation and GPU).
#pragma once
#include "phz_internal.h"

namespace {

// ------------------------------------------------------------------------------------------------ exclusive scan TI -> TO
// out[i] = sum(in[0..i)), out[n] = total.  Three passes: chunk sums, one-block scan of the sums, chunk-local scan + base.
constexpr int GS_ITEMS = 16, GS_CHUNK = GS_ITEMS * 256;

// optional transform of the input on load (a scan over f(in[i]) without materialising f(in)): default = the values themselves
struct GsIdentity { template <class T> __device__ static __forceinline__ T f(T x) { return x; } };

template <class T> __device__ __forceinline__ T gs_wave_incl(T x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T y = __shfl_up(x, d); if (lane >= d) x += y; }
    return x;
}

template <class TI, class TO, class F = GsIdentity> __global__ __launch_bounds__(256) void k_gs_reduce(const TI *in, int64_t n, TO *partial) {
    __shared__ TO s[4];
    const int64_t base = (int64_t)blockIdx.x * GS_CHUNK;
    TO x = 0;
#pragma unroll
    for (int k = 0; k < GS_ITEMS; k++) { const int64_t i = base + k * 256 + threadIdx.x; if (i < n) x += (TO)F::f(in[i]); }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

template <class TO> __global__ __launch_bounds__(1024) void k_gs_partials(TO *partial, int64_t nb, TO *total) {
    __shared__ TO s_w[16];
    __shared__ TO s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
        const int64_t i = b0 + tid;
        const TO v = i < nb ? partial[i] : (TO)0;
        const TO x = gs_wave_incl(v, lane);
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        TO before = s_carry;
        for (int w2 = 0; w2 < wave; w2++) before += s_w[w2];
        if (i < nb) partial[i] = before + x - v;
        __syncthreads();
        if (tid == 1023) s_carry = before + x;
        __syncthreads();
    }
    if (tid == 0) *total = s_carry;
}

// A workgroup's chunk of GS_CHUNK elements as GS_ROWS rows of 256 x 4: thread t holds elements (row * 256 + t) * 4 .. + 3 of every row, so a wave
// reads / writes 1 KB of consecutive memory per instruction (16 consecutive elements per thread made every access instruction touch 64 cache lines:
// the 18.8 M-element scan of a genome's read-label widths ran at 0.9 TB/s).  Exclusive prefix of the chunk with ONE barrier: wave scans of the four
// row sums, the waves' totals of every row in LDS.
constexpr int GS_ROWS = GS_ITEMS / 4;
template <class TI, class TO, class F = GsIdentity> __device__ __forceinline__ void gs_load_rows(const TI *in, int64_t n, int64_t chunk0, int tid, TO v[GS_ROWS][4]) {
#pragma unroll
    for (int r = 0; r < GS_ROWS; r++) {
        const int64_t i = chunk0 + ((int64_t)r * 256 + tid) * 4;
        if (sizeof(TI) == 4 && i + 3 < n && ((reinterpret_cast<uintptr_t>(in) & 15u) == 0)) {
            const uint4 x = *reinterpret_cast<const uint4 *>(in + i);
            v[r][0] = (TO)F::f((TI)x.x); v[r][1] = (TO)F::f((TI)x.y); v[r][2] = (TO)F::f((TI)x.z); v[r][3] = (TO)F::f((TI)x.w);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[r][j] = i + j < n ? (TO)F::f(in[i + j]) : (TO)0;
        }
    }
}
// -> exclusive prefix (inside the chunk) of the first element of every row of this thread; *chunk_sum = sum of the chunk.  s_w: [GS_ROWS][4] in LDS
template <class TO> __device__ __forceinline__ void gs_chunk_scan(const TO v[GS_ROWS][4], int tid, TO (*s_w)[4], TO base[GS_ROWS], TO *chunk_sum) {
    const int lane = tid & 63, wave = tid >> 6;
    TO rs[GS_ROWS], incl[GS_ROWS];
#pragma unroll
    for (int r = 0; r < GS_ROWS; r++) {
        rs[r] = v[r][0] + v[r][1] + v[r][2] + v[r][3];
        incl[r] = gs_wave_incl(rs[r], lane);
        if (lane == 63) s_w[r][wave] = incl[r];
    }
    __syncthreads();
    TO carry = 0;
#pragma unroll
    for (int r = 0; r < GS_ROWS; r++) {
        TO before = carry;
        for (int w2 = 0; w2 < wave; w2++) before += s_w[r][w2];
        base[r] = before + incl[r] - rs[r];
        carry += s_w[r][0] + s_w[r][1] + s_w[r][2] + s_w[r][3];
    }
    *chunk_sum = carry;
}
template <class TO> __device__ __forceinline__ void gs_store_rows(TO *out, int64_t n, int64_t chunk0, int tid, const TO v[GS_ROWS][4], const TO base[GS_ROWS], TO offset) {
#pragma unroll
    for (int r = 0; r < GS_ROWS; r++) {
        const int64_t i = chunk0 + ((int64_t)r * 256 + tid) * 4;
        TO run = offset + base[r];
        TO o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { o[j] = run; run += v[r][j]; }
        if (sizeof(TO) == 4 && i + 3 < n && ((reinterpret_cast<uintptr_t>(out) & 15u) == 0)) {
            *reinterpret_cast<uint4 *>(out + i) = make_uint4((uint32_t)o[0], (uint32_t)o[1], (uint32_t)o[2], (uint32_t)o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) if (i + j < n) out[i + j] = o[j];
        }
        if (i <= n - 1 && n - 1 < i + 4) out[n] = run;      // the thread holding the last element also holds the total (elements beyond n read as 0)
    }
}

template <class TI, class TO, class F = GsIdentity> __global__ __launch_bounds__(256) void k_gs_apply(const TI *in, TO *out, int64_t n, const TO *partial) {
    __shared__ TO s_w[GS_ROWS][4];
    const int tid = threadIdx.x;
    const int64_t chunk0 = (int64_t)blockIdx.x * GS_CHUNK;
    TO v[GS_ROWS][4], base[GS_ROWS], sum;
    gs_load_rows<TI, TO, F>(in, n, chunk0, tid, v);
    gs_chunk_scan<TO>(v, tid, s_w, base, &sum);
    gs_store_rows<TO>(out, n, chunk0, tid, v, base, partial[blockIdx.x]);
}

// ---- the same scan in ONE launch for 32-bit sums (decoupled look-back): tiles take tickets in start order, publish their sum, and the
// first wave of a tile looks back over its predecessors' status words (64 at a time) until it meets one that already knows its prefix.
// A status word = epoch:30 | state:2 | value:32, written and read as one 64-bit access; words of older scans carry an older epoch and
// read as "not there yet", so nothing is cleared between scans.
constexpr unsigned GS_AGG = 1u, GS_PREFIX = 2u;
__device__ __forceinline__ unsigned long long gs_word(uint32_t epoch, unsigned state, uint32_t value) {
    return ((unsigned long long)epoch << 34) | ((unsigned long long)state << 32) | value;
}
template <class TI, class F = GsIdentity> __global__ __launch_bounds__(256) void k_gs_lookback(const TI *in, uint32_t *out, int64_t n, unsigned long long *status, uint32_t *ticket,
                                                                          uint32_t ticket_base, uint32_t epoch) {
    __shared__ uint32_t s_w[GS_ROWS][4];
    __shared__ uint32_t s_tile, s_prefix;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_tile = atomicAdd(ticket, 1u) - ticket_base;
    __syncthreads();
    const uint32_t tile = s_tile;
    const int64_t chunk0 = (int64_t)tile * GS_CHUNK;
    uint32_t v[GS_ROWS][4], base[GS_ROWS], block_sum;
    gs_load_rows<TI, uint32_t, F>(in, n, chunk0, tid, v);
    gs_chunk_scan<uint32_t>(v, tid, s_w, base, &block_sum);
    if (wave == 0) {
        if (lane == 0) __hip_atomic_store(&status[tile], gs_word(epoch, tile == 0 ? GS_PREFIX : GS_AGG, block_sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t excl = 0;
        if (tile > 0) {
            int64_t j = (int64_t)tile - 1;
            for (;;) {
                const int64_t idx = j - lane;
                const unsigned long long w = idx >= 0 ? __hip_atomic_load(&status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : gs_word(epoch, GS_PREFIX, 0u);
                const unsigned state = (uint32_t)(w >> 34) == epoch ? (unsigned)(w >> 32) & 3u : 0u;
                // usable: every word from the nearest predecessor up to the first one that holds a prefix
                const unsigned long long have = __ballot(state != 0u), pref = __ballot(state == GS_PREFIX);
                const unsigned long long upto = pref ? ((pref & (~pref + 1ull)) << 1) - 1ull : ~0ull;        // lanes 0 .. first prefix lane
                if ((have & upto) != upto) { __builtin_amdgcn_s_sleep(1); continue; }                  // a predecessor in that stretch has not published yet
                uint32_t x = ((upto >> lane) & 1ull) ? (uint32_t)w : 0u;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
                excl += x;
                if (pref) break;
                j -= 64;
            }
            if (lane == 0) __hip_atomic_store(&status[tile], gs_word(epoch, GS_PREFIX, excl + block_sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) s_prefix = excl;
    }
    __syncthreads();
    gs_store_rows<uint32_t>(out, n, chunk0, tid, v, base, s_prefix);
}

// force_three_launch: the three-launch passes also where the one-launch scan would be taken (the tests run both; no product caller sets it)
template <class TI, class TO, class F = GsIdentity> int gscan_excl(phz_ctx *ctx, const TI *in, TO *out /* [n + 1] */, int64_t n, DevBuf &tmp, bool force_three_launch = false) {
    hipStream_t sm = ctx->stream;
    if (n <= 0) { PHZ_HIP(ctx, hipMemsetAsync(out, 0, sizeof(TO), sm)); return PHZ_OK; }
    const int64_t nb = (n + GS_CHUNK - 1) / GS_CHUNK;
    // (beyond a few million elements the prefix front of the look-back -- 64 tiles per round trip -- is slower than two streaming passes:
    //  18.8 M elements took 161 us in one launch)
    if (sizeof(TO) == 4 && n < (int64_t)(4 << 20) && !force_three_launch) {
      if constexpr (sizeof(TO) == 4) {
        const size_t before = ctx->scan_state.cap;
        if (int s = phz_reserve(ctx, ctx->scan_state, 64 + (size_t)nb * 8)) return s;
        if (ctx->scan_state.cap != before || ctx->scan_epoch >= (1u << 30) - 2u) {
            PHZ_HIP(ctx, hipMemsetAsync(ctx->scan_state.p, 0, ctx->scan_state.cap, sm));
            ctx->scan_epoch = 0; ctx->scan_ticket_base = 0;
        }
        const uint32_t epoch = ++ctx->scan_epoch;
        hipLaunchKernelGGL((k_gs_lookback<TI, F>), dim3((unsigned)nb), dim3(256), 0, sm, in, (uint32_t *)out, n, (unsigned long long *)((char *)ctx->scan_state.p + 64),
                           (uint32_t *)ctx->scan_state.p, ctx->scan_ticket_base, epoch);
        ctx->scan_ticket_base += (uint32_t)nb;
        PHZ_HIP(ctx, hipGetLastError());
        (void)tmp;
        return PHZ_OK;
      }
    }
    {
        if (int s = phz_reserve(ctx, tmp, (size_t)nb * sizeof(TO) + 16)) return s;
        TO *partial = (TO *)tmp.p;
        hipLaunchKernelGGL((k_gs_reduce<TI, TO, F>), dim3((unsigned)nb), dim3(256), 0, sm, in, n, partial);
        hipLaunchKernelGGL((k_gs_partials<TO>), dim3(1), dim3(1024), 0, sm, partial, nb, out + n);
        hipLaunchKernelGGL((k_gs_apply<TI, TO, F>), dim3((unsigned)nb), dim3(256), 0, sm, in, out, n, (const TO *)partial);
        PHZ_HIP(ctx, hipGetLastError());
        return PHZ_OK;
    }
}

}  // namespace
