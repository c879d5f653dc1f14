// --output_haplotag_bam: the records of an input BAM that passed the run's filters, written out again with the haplotype their template votes for (HP:C, PS:I).
// Two entry points over data that is already in HBM ("--output_haplotag_bam, K_tagpick and K_tagwrite"):
//
//   phz_haplotag_pick      K_tagpick: the join.  One tag word per template of one BAM from the records of phz_read_haplotypes.
//     k_tagpick_max   one lane per row: the row is checked, and a row of this BAM in a phased block puts (a + b) << 32 | (0xFFFFFFFF - block) into the template's
//                     slot of a zeroed table with a 64-bit atomicMax -- the largest total wins, the smallest block index among equal totals.  Max does not depend
//                     on the order of the lanes: every run gives the same table.
//     k_tagpick_write one lane per row: the row whose key IS the table's writes the tag word, (block + 1) << 2 | hp, with a plain store (one such row per slot:
//                     the rows of phz_read_haplotypes hold every (block, bam, qid) once).  hp = 1 (a > b), 2 (b > a), 0 (a == b: the winning block tied; the
//                     template does not fall through to its next block).
//
//   phz_bamdev_haplotag    the record rewrite, on an open handle of the device BAM path (the inflated stream and the offset of every kept record: phz_bamdev.K.off).
//     k_tagsize       one lane per kept record of the reference: block_size, the tag word of its template, and a walk over its aux fields (the walker shape of
//                     aux_as_dev in phz_bamdev.hip) that refuses a record which already carries HP or PS, or whose aux chain does not end at block_size;
//                     output bytes of the record = 4 + block_size (+ 11 when tagged)
//     gscan_excl      uint32 -> uint64: where every record starts in the output
//     k_tagwrite      one wave per record, the lanes striding over its bytes; block_size raised by 11 and HP:C, PS:I appended on a tagged record
// Every read of the stream stays inside [record, record + 4 + block_size), which k_hop validated against the stream's end when the handle was opened.
// Neither the source nor the destination of the copy is aligned to anything (records are packed back to back, and 11 is odd), so the copy moves ONE BYTE PER LANE:
// the 64 lanes of a wave read 64 consecutive bytes and write 64 consecutive bytes, a cache line's worth per instruction on either side whatever the alignment.  A
// wider access would need a funnel shift on one side and byte-wise heads and tails on both.  Measured once at whole-genome size (tools/haplotag_scale.py,
// profiles/r25/haplotag_scale.txt): the fill calls of 59 M records, 11.2 GB, took 34 ms in all, next to 21 s of deflate on the host -- this copy is not what a user waits for.
// Plain vector stores only.
//
// Tested in tests/test_gpu_haplotag.py against the plain Python restatement of tests/haplotag_restatement.py.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "phz.h"
#include "phz_internal.h"
#include "phz_bamdev_internal.h"
#include "phz_scan.h"

namespace {

// ------------------------------------------------------------------------------------------------ K_tagpick
enum { TP_F_BLOCK = 0, TP_F_CHROM = 1, TP_F_QID = 2, TP_F_COUNT = 3 };          // words of the verdict block (zeroed by the driver)

struct TagPick {
    const phz_readhap_rec *rows; int64_t n_rows, n_blocks, n_phased; int32_t bam;
    const int32_t *blk_chrom; int32_t n_chroms; const int64_t *tmpl_base; int64_t n_templates;
};

// the slot of a row in the joint template space; -1: the row does not vote (another BAM, a block that is not phased).  A row that cannot be placed sets its flag
__device__ __forceinline__ int64_t tagpick_slot(const TagPick &a, const phz_readhap_rec &r, uint32_t *flag) {
    if (r.block < 0 || (int64_t)r.block >= a.n_blocks) { flag[TP_F_BLOCK] = 1; return -1; }
    const int32_t c = a.blk_chrom[r.block];
    if (c < 0 || c >= a.n_chroms) { flag[TP_F_CHROM] = 1; return -1; }
    const int64_t base = a.tmpl_base[c], slot = base + (int64_t)r.qid;
    if (r.qid < 0 || slot >= a.tmpl_base[c + 1] || slot < 0 || slot >= a.n_templates) { flag[TP_F_QID] = 1; return -1; }
    if (r.a < 0 || r.b < 0) { flag[TP_F_COUNT] = 1; return -1; }
    if (r.bam != a.bam || (int64_t)r.block >= a.n_phased) return -1;
    return slot;
}
__device__ __forceinline__ unsigned long long tagpick_key(const phz_readhap_rec &r) {
    return ((unsigned long long)((uint32_t)r.a + (uint32_t)r.b) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)r.block);
}

__global__ __launch_bounds__(256) void k_tagpick_max(TagPick a, unsigned long long *best, uint32_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rows) return;
    const phz_readhap_rec r = a.rows[i];
    const int64_t slot = tagpick_slot(a, r, flag);
    if (slot >= 0) atomicMax(&best[slot], tagpick_key(r));
}

__global__ __launch_bounds__(256) void k_tagpick_write(TagPick a, const unsigned long long *best, uint32_t *flag, uint32_t *tag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_rows) return;
    if (flag[TP_F_BLOCK] | flag[TP_F_CHROM] | flag[TP_F_QID] | flag[TP_F_COUNT]) return;          // refused rows: no tag is written (the first pass has finished: same stream)
    const phz_readhap_rec r = a.rows[i];
    const int64_t slot = tagpick_slot(a, r, flag);
    if (slot < 0 || best[slot] != tagpick_key(r)) return;
    tag[slot] = (((uint32_t)r.block + 1u) << 2) | (r.a > r.b ? 1u : r.b > r.a ? 2u : 0u);
}

const char *tagpick_verdict(const uint32_t *f) {
    if (f[TP_F_BLOCK]) return "phz_haplotag_pick: a row whose block is outside [0, n_blocks)";
    if (f[TP_F_CHROM]) return "phz_haplotag_pick: blk_chrom holds a value outside [0, n_chroms)";
    if (f[TP_F_QID]) return "phz_haplotag_pick: a row whose qid is outside the template ids of its chromosome (tmpl_base)";
    if (f[TP_F_COUNT]) return "phz_haplotag_pick: a row with a negative count";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------ K_tagsize, K_tagwrite
// the aux fields [p, e) of a record: 0 = a clean chain that ends exactly at e without HP or PS, 1 = it carries HP or PS, 2 = it does not end at e (an unknown type,
// a string without its NUL, a field that runs past e)
__device__ int aux_tag_check(const uint8_t *p, const uint8_t *e) {
    bool carries = false;
    while (p < e) {
        if (p + 3 > e) return 2;
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
        p += 3;
        uint64_t sz = 0;
        switch (ty) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'Z': case 'H': { const uint8_t *q = p; while (q < e && *q) q++; if (q >= e) return 2; sz = (uint64_t)(q - p) + 1; break; }
            case 'B': {
                if (p + 5 > e) return 2;
                const uint8_t sub = p[0];
                const uint32_t cnt = ld32(p + 1);
                uint64_t es = 0;
                switch (sub) { case 'c': case 'C': es = 1; break; case 's': case 'S': es = 2; break; case 'i': case 'I': case 'f': es = 4; break; default: return 2; }
                sz = 5 + es * (uint64_t)cnt;
                break;
            }
            default: return 2;
        }
        if (sz > (uint64_t)(e - p)) return 2;
        if ((t0 == 'H' && t1 == 'P') || (t0 == 'P' && t1 == 'S')) carries = true;
        p += sz;
    }
    return carries ? 1 : 0;
}

enum { TW_BAD = 0, TW_TAGGED = 1, TW_ARG = 2, TW_WORDS = 3 };          // 64-bit words of the head block: first refused record (offset << 1 | kind; all ones = none), tagged records, bad argument

struct TagWrite {
    const uint8_t *d; const uint64_t *off; int64_t n;          // the stream, the kept records of the reference
    const int32_t *qid; const uint32_t *tag; int64_t n_tag; const uint32_t *blk_ps; int64_t n_blocks;
};

// the tag word of kept record i when it is a usable one, else 0 with the argument flag set
__device__ __forceinline__ uint32_t tagwrite_word(const TagWrite &a, int64_t i, unsigned long long *head) {
    const int32_t q = a.qid[i];
    if (q < 0 || (int64_t)q >= a.n_tag) { head[TW_ARG] = 1; return 0; }
    const uint32_t t = a.tag[q];
    if (t && ((t >> 2) == 0 || (int64_t)(t >> 2) > a.n_blocks || (t & 3u) == 3u)) { head[TW_ARG] = 1; return 0; }
    return t;
}

__global__ __launch_bounds__(256) void k_tagsize(TagWrite a, uint32_t *len, unsigned long long *head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool tagged = false;
    if (i < a.n) {
        const uint8_t *r = a.d + a.off[i];
        const uint32_t bs = ld32(r - 4);          // (k_hop: 32 <= block_size, the fixed fields + name + CIGAR + bases + qualities fit in it, the record ends inside the stream)
        const uint32_t l_rn = r[8], n_cig = ld16(r + 12);
        const int32_t l_seq = ldi32(r + 16);
        const uint64_t fixed = 32 + (uint64_t)l_rn + 4 * (uint64_t)n_cig + ((uint64_t)(l_seq > 0 ? l_seq : 0) + 1) / 2 + (uint64_t)(l_seq > 0 ? l_seq : 0);
        const int kind = fixed > (uint64_t)bs ? 2 : aux_tag_check(r + fixed, r + bs);
        if (kind) atomicMin(&head[TW_BAD], ((unsigned long long)(a.off[i] - 4) << 1) | (unsigned long long)(kind - 1));
        tagged = (tagwrite_word(a, i, head) & 3u) != 0;
        len[i] = 4u + bs + (tagged ? 11u : 0u);
    }
    const unsigned long long m = __ballot(tagged ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&head[TW_TAGGED], (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void k_tagwrite(TagWrite a, const unsigned long long *out_off, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);          // one wave per record
    if (i >= a.n) return;
    const uint8_t *src = a.d + a.off[i] - 4;
    const uint32_t bs = ld32(src);
    const uint32_t t = a.tag[a.qid[i]];          // (k_tagsize has checked qid and the word; this kernel is launched only when it found nothing)
    const bool tagged = (t & 3u) != 0;
    uint8_t *dst = out + out_off[i];
    const uint32_t end = 4u + bs, new_bs = bs + (tagged ? 11u : 0u);
    if (lane < 4) dst[lane] = (uint8_t)(new_bs >> (8 * lane));
    for (uint32_t k = 4u + (uint32_t)lane; k < end; k += 64) dst[k] = src[k];
    if (tagged && lane < 11) {
        const uint32_t ps = a.blk_ps[(t >> 2) - 1];
        uint8_t v;
        switch (lane) {
            case 0: v = 'H'; break; case 1: v = 'P'; break; case 2: v = 'C'; break; case 3: v = (uint8_t)(t & 3u); break;
            case 4: v = 'P'; break; case 5: v = 'S'; break; case 6: v = 'I'; break;
            default: v = (uint8_t)(ps >> (8 * (lane - 7))); break;
        }
        dst[end + lane] = v;
    }
}

}  // namespace

extern "C" int phz_haplotag_pick(phz_ctx *ctx, const phz_readhap_rec *rows, int64_t n_rows, int64_t n_blocks, int64_t n_phased, int32_t bam, const int32_t *blk_chrom,
                                 int32_t n_chroms, const int64_t *tmpl_base, int64_t n_templates, uint32_t *tag, int space) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || n_rows < 0 || n_blocks < 0 || n_phased < 0 || n_phased > n_blocks || n_chroms < 0 || n_templates < 0 || (n_templates && !tag) ||
        (n_rows && (!rows || !blk_chrom || !tmpl_base))) return PHZ_E_ARG;
    if (n_rows && n_templates == 0) return phz_fail(ctx, PHZ_E_ARG, "phz_haplotag_pick: a row whose qid is outside the template ids of its chromosome (there are no templates)");
    if (n_blocks >= (1ll << 30)) return phz_fail(ctx, PHZ_E_ARG, "phz_haplotag_pick: 2^30 blocks or more (the tag word keeps block + 1 in 30 bits)");
    // ---- arguments a host caller hands over: checked before anything is launched
    if (space == PHZ_HOST && n_rows) {
        uint32_t f[4] = {0, 0, 0, 0};
        for (int64_t i = 0; i < n_rows; i++) {
            const phz_readhap_rec &r = rows[i];
            if (r.block < 0 || r.block >= n_blocks) { f[TP_F_BLOCK] = 1; continue; }
            const int32_t c = blk_chrom[r.block];
            if (c < 0 || c >= n_chroms) { f[TP_F_CHROM] = 1; continue; }
            const int64_t slot = tmpl_base[c] + (int64_t)r.qid;
            if (r.qid < 0 || slot >= tmpl_base[c + 1] || slot < 0 || slot >= n_templates) f[TP_F_QID] = 1;
            if (r.a < 0 || r.b < 0) f[TP_F_COUNT] = 1;
        }
        if (const char *why = tagpick_verdict(f)) return phz_fail(ctx, PHZ_E_ARG, why);
    }
    if (n_templates == 0) return PHZ_OK;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t sm = ctx->stream;
    Staging st(ctx);
    TagPick a;
    a.n_rows = n_rows; a.n_blocks = n_blocks; a.n_phased = n_phased; a.bam = bam; a.n_chroms = n_chroms; a.n_templates = n_templates;
    uint32_t *d_tag;
    if (int s = st.in(rows, (size_t)n_rows, space, &a.rows)) return s;
    if (int s = st.in(blk_chrom, (size_t)(n_rows ? n_blocks : 0), space, &a.blk_chrom)) return s;
    if (int s = st.in(tmpl_base, (size_t)(n_rows ? n_chroms + 1 : 0), space, &a.tmpl_base)) return s;
    if (int s = st.out(tag, (size_t)n_templates, space, &d_tag)) return s;
    PHZ_HIP(ctx, hipMemsetAsync(d_tag, 0, (size_t)n_templates * 4, sm));
    if (n_rows) {
        DevBuf *S = ctx->scratch;
        if (int s = reserve_all(ctx, {{S[SC_TAG_FLAG], 4 * sizeof(uint32_t)}, {S[SC_TAG_BEST], (size_t)n_templates * 8}})) return s;
        uint32_t *flag = (uint32_t *)S[SC_TAG_FLAG].p;
        unsigned long long *best = (unsigned long long *)S[SC_TAG_BEST].p;
        PHZ_HIP(ctx, hipMemsetAsync(flag, 0, 4 * sizeof(uint32_t), sm));
        PHZ_HIP(ctx, hipMemsetAsync(best, 0, (size_t)n_templates * 8, sm));
        hipLaunchKernelGGL(k_tagpick_max, dim3(nblk(n_rows)), dim3(256), 0, sm, a, best, flag);
        hipLaunchKernelGGL(k_tagpick_write, dim3(nblk(n_rows)), dim3(256), 0, sm, a, (const unsigned long long *)best, flag, d_tag);
        PHZ_HIP(ctx, hipGetLastError());
        PhzMail mail(ctx);
        const int m0 = mail.add(flag, 4 * sizeof(uint32_t));
        if (int s = mail.send()) return s;
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        if (const char *why = tagpick_verdict(mail.at<uint32_t>(m0))) return phz_fail(ctx, PHZ_E_ARG, why);
    }
    if (space == PHZ_HOST) PHZ_HIP(ctx, hipMemcpyAsync(tag, d_tag, (size_t)n_templates * 4, hipMemcpyDeviceToHost, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}

extern "C" int phz_bamdev_haplotag(phz_bamdev *h, int ref, const int32_t *qid, const uint32_t *tag, int64_t n_tag, const uint32_t *blk_ps, int64_t n_blocks, uint8_t *out,
                                   int64_t out_cap, int64_t *out_bytes, int64_t *n_tagged) {
    if (!h || !h->ctx) return PHZ_E_ARG;
    phz_ctx *ctx = h->ctx;
    PhzEnter phz_guard_(ctx);
    if (!out_bytes || !n_tagged || ref < 0 || (size_t)ref >= h->refs.size() || n_tag < 0 || n_blocks < 0 || out_cap < 0)
        return phz_fail(ctx, PHZ_E_ARG, "phz_bamdev_haplotag: a NULL result pointer, a reference the file does not have, or a negative size");
    *out_bytes = 0; *n_tagged = 0;
    const int64_t i0 = h->ref_begin[(size_t)ref], n = h->ref_begin[(size_t)ref + 1] - i0;
    if (n <= 0) return PHZ_OK;
    if (!qid || (n_tag && !tag) || (n_blocks && !blk_ps)) return phz_fail(ctx, PHZ_E_ARG, "phz_bamdev_haplotag: qid, tag or blk_ps is NULL");
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t sm = ctx->stream;
    DevBuf *S = ctx->scratch;
    if (int s = reserve_all(ctx, {{S[SC_TAGW_HEAD], TW_WORDS * 8}, {S[SC_TAGW_LEN], (size_t)n * 4}, {S[SC_TAGW_OFF], ((size_t)n + 1) * 8}})) return s;
    unsigned long long *head = (unsigned long long *)S[SC_TAGW_HEAD].p, *out_off = (unsigned long long *)S[SC_TAGW_OFF].p;
    uint32_t *len = (uint32_t *)S[SC_TAGW_LEN].p;
    TagWrite a;
    a.d = (const uint8_t *)h->d_stream; a.off = h->K.off + i0; a.n = n; a.qid = qid; a.tag = tag; a.n_tag = n_tag; a.blk_ps = blk_ps; a.n_blocks = n_blocks;
    // ---- sizes, their scan, the verdict                                                                      WAIT
    PHZ_HIP(ctx, hipMemsetAsync(head, 0xFF, 8, sm));
    PHZ_HIP(ctx, hipMemsetAsync(head + 1, 0, (TW_WORDS - 1) * 8, sm));
    hipLaunchKernelGGL(k_tagsize, dim3(nblk(n)), dim3(256), 0, sm, a, len, head);
    PHZ_HIP(ctx, hipGetLastError());
    if (int s = gscan_excl<uint32_t, unsigned long long>(ctx, len, out_off, n, S[SC_TAGW_SCAN_TMP])) return s;
    PhzMail mail(ctx);
    const int m0 = mail.add(head, TW_WORDS * 8), m1 = mail.add(out_off + n, 8);
    if (int s = mail.send()) return s;
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    const unsigned long long *hw = mail.at<unsigned long long>(m0);
    if (hw[TW_ARG]) return phz_fail(ctx, PHZ_E_ARG, "phz_bamdev_haplotag: a qid outside [0, n_tag), or a tag word that names no block of blk_ps");
    if (hw[TW_BAD] != ~0ull) {
        char msg[200];
        snprintf(msg, sizeof msg, (hw[TW_BAD] & 1ull) ? "phz_bamdev_haplotag: the aux fields of the record at offset %llu of the inflated stream do not end at its block_size"
                                                        : "phz_bamdev_haplotag: the record at offset %llu of the inflated stream already carries HP or PS (nothing is stripped)",
                 hw[TW_BAD] >> 1);
        return phz_fail(ctx, PHZ_E_UNSUPPORTED, msg);
    }
    const int64_t total = (int64_t)*mail.at<unsigned long long>(m1);
    *out_bytes = total; *n_tagged = (int64_t)hw[TW_TAGGED];
    if (!out || out_cap < total) return phz_fail(ctx, PHZ_E_CAPACITY, "phz_bamdev_haplotag: out_cap too small (out_bytes holds the number of bytes)");
    // ---- the records                                                                                         WAIT
    hipLaunchKernelGGL(k_tagwrite, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, sm, a, (const unsigned long long *)out_off, out);
    PHZ_HIP(ctx, hipGetLastError());
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}
