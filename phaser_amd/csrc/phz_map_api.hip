// Host side of the mapper entry points of the C ABI (include/phz.h): argument checks and staging for PHZ_HOST callers around the
// launchers of phz_map.hip.
#include "phz_internal.h"

static int check_variants(phz_ctx *ctx, const phz_variants *v, int space) {
    // SNP-only fast path: reject indel mode up front (host-visible arrays only)
    if (space == PHZ_HOST && v->ref_len)
        for (int64_t i = 0; i < v->n; i++)
            if (v->ref_len[i] != 1) return phz_fail(ctx, PHZ_E_UNSUPPORTED, "variants with ref_len != 1 (indel mode) are not supported by K_map yet");
    return PHZ_OK;
}

extern "C" int phz_map_reads_batch(phz_ctx *ctx, int n_shards, const phz_reads *reads, const phz_variants *vars, int baseq,
                                   const phz_calls *out, int64_t *n_calls) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_shards < 0 || (n_shards && (!reads || !vars || !out || !n_calls))) return PHZ_E_ARG;
    for (int i = 0; i < n_shards; i++)
        if (reads[i].n_reads < 0 || vars[i].n < 0 || out[i].cap < 0) return phz_fail(ctx, PHZ_E_ARG, "negative size");
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    return phz_launch_map_batch(ctx, n_shards, reads, vars, baseq, out, n_calls);
}

extern "C" int phz_map_reads(phz_ctx *ctx, const phz_reads *reads, const phz_variants *vars, int baseq,
                             phz_calls *out, int64_t *n_calls, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !reads || !vars || !out || !n_calls) return PHZ_E_ARG;
    if (reads->n_reads < 0 || vars->n < 0 || out->cap < 0) return phz_fail(ctx, PHZ_E_ARG, "negative size");
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    if (int s = check_variants(ctx, vars, space)) return s;
    if (space == PHZ_DEVICE) return phz_launch_map(ctx, *reads, *vars, baseq, *out, n_calls);
    if (space != PHZ_HOST) return phz_fail(ctx, PHZ_E_ARG, "bad memory space");

    // device copies of the caller's arrays and outputs: slots of the ctx's staging pool, as for every other PHZ_HOST entry point
    Staging st(ctx);
    const size_t n = (size_t)reads->n_reads, cap = (size_t)out->cap;
    phz_reads dr = *reads;
    phz_variants dv = *vars;
    phz_calls dc = *out;
    dr.bq = nullptr; dv.ref_len = nullptr; dc.aux0 = nullptr; dc.aux1 = nullptr;
    if (int s = st.in(reads->pos, n, space, &dr.pos)) return s;
    if (int s = st.in(reads->cigar_off, n + 1, space, &dr.cigar_off)) return s;
    if (int s = st.in(reads->cigar, (size_t)reads->n_ops, space, &dr.cigar)) return s;
    if (int s = st.in(reads->seq_off, n + 1, space, &dr.seq_off)) return s;
    if (int s = st.in(reads->seq2, (size_t)reads->n_seq_bytes, space, &dr.seq2)) return s;
    if (int s = st.in(reads->qual, (size_t)reads->n_seq_bytes * 4, space, &dr.qual)) return s;
    if (int s = st.in(vars->pos, (size_t)vars->n, space, &dv.pos)) return s;
    if (int s = st.out(out->read_idx, cap, space, &dc.read_idx)) return s;
    if (int s = st.out(out->var_idx, cap, space, &dc.var_idx)) return s;
    if (int s = st.out(out->code, cap, space, &dc.code)) return s;
    if (out->aux0 && out->aux1) {          // both planes or none
        if (int s = st.out(out->aux0, cap, space, &dc.aux0)) return s;
        if (int s = st.out(out->aux1, cap, space, &dc.aux1)) return s;
    }
    const int status = phz_launch_map(ctx, dr, dv, baseq, dc, n_calls);
    if (status != PHZ_OK && status != PHZ_E_CAPACITY) return status;
    const size_t m = (size_t)(*n_calls < out->cap ? *n_calls : out->cap);          // PHZ_E_CAPACITY: the first `cap` calls
    if (m) {
        PHZ_HIP(ctx, hipMemcpyAsync(out->read_idx, dc.read_idx, m * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHZ_HIP(ctx, hipMemcpyAsync(out->var_idx, dc.var_idx, m * 4, hipMemcpyDeviceToHost, ctx->stream));
        PHZ_HIP(ctx, hipMemcpyAsync(out->code, dc.code, m, hipMemcpyDeviceToHost, ctx->stream));
        if (dc.aux0) {
            PHZ_HIP(ctx, hipMemcpyAsync(out->aux0, dc.aux0, m * 4, hipMemcpyDeviceToHost, ctx->stream));
            PHZ_HIP(ctx, hipMemcpyAsync(out->aux1, dc.aux1, m * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    PHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return status;
}
