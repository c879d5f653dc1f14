// Device-side BAM path (SURVEY.md 8(f) next-1 on the GPU): from the BGZF members of a coordinate-sorted BAM in a file to the
// structure-of-arrays shards K_map reads, without the records ever visiting the host.  Replaces, like phz_bam.cpp, what phASER gets
// from `samtools view -h BAM 'chr': | samtools view -Sh [-F 0x400] [-f 2] -q MAPQ -` (phaser/phaser.py:1346, :505-513) plus the
// mapper's per-record text parsing (phaser/read_variant_map.py:27-64) -- same filters, same packed arrays (tests compare the two
// paths array by array).
//
//   host   member table + header + chromosome ranges (phz_bam_plan_file: a few probe members inflated with zlib)
//   H2D    the compressed members that hold wanted records
//   K_inflate (phz_inflate.hip)  one lane per BGZF member
//   k_seg_start   the stream is cut into ~256 KB segments; the first record boundary of each is GUESSED by a plausibility chain
//   k_hop<0>      one lane per segment hops its record chain: filters, kept-record count, sortedness; every guess is VERIFIED
//                 (segment k must end exactly where segment k+1 starts -- the same proof the host's parallel hop uses)
//   scan + k_hop<1>   kept-record list (offset, reference, op count, bases, name length)
//   scans + k_pack    one lane per kept record writes its slots of the shard arrays (normalised CIGAR, 2-bit bases, quals, AS)
// Anything the device path cannot prove (a member that is not valid DEFLATE, a boundary that does not verify, an unsorted file,
// 32-bit offsets exceeded) returns PHZ_E_UNSUPPORTED and the caller uses the host path.  Reference boundaries that the plan cannot prove are not among
// them: phz_bam_plan_file then answers the whole record stream as one piece, and the reference mask selects the records here.
//
// Tested in tests/test_gpu_bamdev.py (K_inflate against zlib; shards against the host decoder under every filter, on odd records, long reads, damaged
// members and corrupt streams; the chunked multi-stream pipeline) and in tests/test_gpu_bam_boundaries.py (k_seg_start, k_hop<0> and counting_hop on
// files with PLANTED fake record chains under chosen segment guesses, against the sequential Python reader: one repair per pass for fakes at
// consecutive guesses, 7 in a row converge and 8 decline, fakes out of coordinate order are never taken, a dead-end fake chain behind an unclean
// segment does not fail the file, a record longer than two segments leaves empty segments; members that start on a fake, whole file and restricted, the one-piece plan included).
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "phz.h"
#include "phz_internal.h"
#include "phz_bamdev_internal.h"      // struct phz_bamdev, KeptOut, ld16 / ld32 / ldi32

namespace {

// ------------------------------------------------------------------------------------------------ exclusive scan (uint32), this unit's own
// out[i] = sum(in[0..i)), out[n] = total.  Three passes at every size: chunk sums, one-block scan of the sums, chunk-local scan + base (16 consecutive elements
// per thread).  The older scan of the library, kept HERE only: with gscan_excl of phz_scan.h in its place the medians of bam_path.seconds and of
// bam_path.copy_plus_inflate_ms lay above the spread of this build's four runs (profiles/r13/scan_swap_bench.txt), and the margin had been set beforehand.
constexpr int SCAN_ITEMS = 16, SCAN_CHUNK = SCAN_ITEMS * 256;

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if (lane >= d) x += y; }
    return x;
}

__global__ __launch_bounds__(256) void k_scan_reduce(const uint32_t *in, int64_t n, uint32_t *partial) {
    __shared__ uint32_t s[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK;
    uint32_t x = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { const int64_t i = base + k * 256 + threadIdx.x; if (i < n) x += in[i]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__global__ __launch_bounds__(1024) void k_scan_partials(uint32_t *partial, int64_t nb, uint32_t *total) {
    __shared__ uint32_t s_w[16];
    __shared__ uint32_t s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
        const int64_t i = b0 + tid;
        const uint32_t v = i < nb ? partial[i] : 0;
        const uint32_t x = wave_incl_scan(v, lane);
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        uint32_t before = s_carry;
        for (int w2 = 0; w2 < wave; w2++) before += s_w[w2];
        if (i < nb) partial[i] = before + x - v;
        __syncthreads();
        if (tid == 1023) s_carry = before + x;
        __syncthreads();
    }
    if (tid == 0) *total = s_carry;
}

__global__ __launch_bounds__(256) void k_scan_apply(const uint32_t *in, uint32_t *out, int64_t n, const uint32_t *partial) {
    __shared__ uint32_t s_v[SCAN_CHUNK + SCAN_CHUNK / 16];      // padded: item i at i + i/16 (thread t's 16 items: no bank conflicts)
    __shared__ uint32_t s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        const int j = k * 256 + tid;
        const int64_t i = base + j;
        s_v[j + (j >> 4)] = i < n ? in[i] : 0;
    }
    __syncthreads();
    uint32_t loc[SCAN_ITEMS];
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { loc[k] = s_v[tid * 17 + k]; sum += loc[k]; }
    const uint32_t incl = wave_incl_scan(sum, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t run = partial[blockIdx.x] + incl - sum;
    for (int w2 = 0; w2 < wave; w2++) run += s_w[w2];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { s_v[tid * 17 + k] = run; run += loc[k]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        const int j = k * 256 + tid;
        const int64_t i = base + j;
        if (i < n) out[i] = s_v[j + (j >> 4)];
    }
}

int scan_excl(phz_ctx *ctx, const uint32_t *in, uint32_t *out /* [n + 1] */, int64_t n, DevBuf &tmp) {
    hipStream_t sm = ctx->stream;
    if (n <= 0) { PHZ_HIP(ctx, hipMemsetAsync(out, 0, 4, sm)); return PHZ_OK; }
    const int64_t nb = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (int s = phz_reserve(ctx, tmp, (size_t)nb * 4 + 16)) return s;
    uint32_t *partial = (uint32_t *)tmp.p;
    hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)nb), dim3(256), 0, sm, in, n, partial);
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(1024), 0, sm, partial, nb, out + n);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(256), 0, sm, in, out, n, (const uint32_t *)partial);
    PHZ_HIP(ctx, hipGetLastError());
    return PHZ_OK;
}

struct Seg { uint64_t guess, end; uint32_t exact, piece; };     // end = end of the segment's piece

struct Filters {
    int min_mapq, flag_required, flag_forbidden;
    double isize_cutoff;
    const uint8_t *ref_mask;      // [n_ref] device, 1 = wanted
    int n_ref;
};

// can offset p of d[0, n) start a record?  -> offset of the next record, 0 when it cannot (same test as the host's record_at);
// *key = the record's coordinate-sort key (k_seg_start wants the keys of a chain in order, which the host's guesses do not ask)
__device__ uint64_t plausible(const uint8_t *d, uint64_t n, uint64_t p, int n_ref, uint64_t *key) {
    if (p + 36 > n) return 0;
    const int32_t bs = ldi32(d + p);
    if (bs < 32 || bs > (1 << 24) || p + 4 + (uint64_t)bs > n) return 0;
    const uint8_t *r = d + p + 4;
    const int32_t ref = ldi32(r), pos0 = ldi32(r + 4), l_seq = ldi32(r + 16), nref = ldi32(r + 20);
    const uint32_t l_rn = r[8], n_cig = ld16(r + 12), flag = ld16(r + 14);
    // a QNAME has at least one character (SAM: [!-?A-~]{1,254}; an empty name would make every zero byte a candidate), FLAG has 12
    // defined bits, mate position >= -1
    if (ref < -1 || ref >= n_ref || nref < -1 || nref >= n_ref || pos0 < -1 || l_seq < 0 || l_rn < 2 || flag >= 4096 || ldi32(r + 24) < -1) return 0;
    const uint64_t need = 32 + (uint64_t)l_rn + 4 * (uint64_t)n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
    if (need > (uint64_t)bs) return 0;
    if (r[32 + l_rn - 1] != 0) return 0;
    for (uint32_t k = 0; k + 1 < l_rn; k++) if (r[32 + k] < 33 || r[32 + k] > 126) return 0;
    *key = ((uint64_t)(ref < 0 ? 0x7fffffff : ref) << 32) | (uint32_t)(pos0 + 1);      // coordinate-sort key (unmapped last)
    return p + 4 + (uint64_t)bs;
}

__global__ __launch_bounds__(64) void k_seg_start(const uint8_t *d, const Seg *segs, int64_t nseg, int n_ref, uint64_t *start) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= nseg) return;
    const Seg s = segs[k];
    if (s.exact) { start[k] = s.guess; return; }
    const uint64_t limit = s.guess + (32u << 20) < s.end ? s.guess + (32u << 20) : s.end;
    uint64_t found = s.end;
    for (uint64_t p = s.guess; p < limit; p++) {
        uint64_t q = p, prev_key = 0; int ok = 0;
        while (ok < 12) {
            uint64_t key;
            const uint64_t nx = plausible(d, s.end, q, n_ref, &key);
            if (!nx || key < prev_key) break;              // the records of a chain are in coordinate order, too
            prev_key = key;
            ok++; q = nx;
            if (q + 4 > s.end) { ok = 12; break; }
        }
        if (ok >= 12) { found = p; break; }
    }
    start[k] = found;
}

// number of ops of a record's normalised op list (see norm_ops in phz_bam.cpp / soa.pack_sam); out != nullptr: write them
__device__ int norm_ops_dev(const uint8_t *cig, int n_cig, int nb, uint32_t *out) {
    int n = 0;
    long long read_pos = 0;
    for (int i = 0; i < n_cig; i++) {
        const uint32_t c = ld32(cig + 4 * i);
        const uint32_t op = c & 15, len = c >> 4;
        if (op == 0 || op == 7 || op == 8) {
            const long long lo = read_pos < nb ? read_pos : nb, hi = read_pos + (long long)len < nb ? read_pos + (long long)len : nb;
            const uint32_t avail = (uint32_t)(hi > lo ? hi - lo : 0);
            if (avail == len) { if (out) out[n] = c; n++; }
            else {
                if (avail) { if (out) out[n] = (avail << 4) | op; n++; }
                if (out) out[n] = ((len - avail) << 4) | 9u;
                n++;
            }
            read_pos += len;
        } else if (op == 1) {
            const long long lo = read_pos < nb ? read_pos : nb, hi = read_pos + (long long)len < nb ? read_pos + (long long)len : nb;
            const uint32_t avail = (uint32_t)(hi > lo ? hi - lo : 0);
            if (out) out[n] = (avail << 4) | 1u;
            n++;
            read_pos += len;
        } else if (op == 4) {
            if (out) out[n] = c;
            n++;
            read_pos += len;
        } else if (op == 2 || op == 3) {
            if (out) out[n] = c;
            n++;
        }                                  // H, P and anything else leave no trace (as in the host packer)
    }
    return n;
}

struct SegOut {                 // per segment, written by the counting hop
    uint32_t kept;
    uint32_t flags;             // 1 corrupt chain, 2 boundary mismatch, 4 unsorted inside the segment
    int32_t first_ref, first_pos, last_ref, last_pos;      // of the kept records (first_ref = -2 when none)
    uint64_t end_pos;                                      // where the chain arrived (>= the segment's stop)
    uint64_t sq_sum, qn_sum, op_sum;                       // 64-bit sums of base groups, name bytes and 2 x CIGAR ops (upper bound of the
                                                           // normalised op count) over the kept records: the scans below are 32-bit
};

template <int WRITE>
__global__ __launch_bounds__(64) void k_hop(const uint8_t *d, const Seg *segs, int64_t nseg, const uint64_t *start, Filters F, SegOut *so,
                                            const uint32_t *kept_base, KeptOut K) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= nseg) return;
    const Seg s = segs[k];
    const uint64_t n = s.end;
    uint64_t p = start[k];
    const uint64_t stop = (k + 1 < nseg && segs[k + 1].piece == s.piece) ? start[k + 1] : s.end;
    uint32_t kept = 0, flags = 0;
    uint64_t sq_sum = 0, qn_sum = 0, op_sum = 0;
    int32_t first_ref = -2, first_pos = 0, last_ref = -2, last_pos = 0;
    uint64_t w = WRITE ? kept_base[k] : 0;
    while (p < stop) {
        if (p + 36 > n) { flags |= 1; break; }
        const int32_t bs = ldi32(d + p);
        if (bs < 32 || (uint64_t)bs > n - p - 4) { flags |= 1; break; }
        const uint8_t *r = d + p + 4;
        const int32_t ref = ldi32(r);
        const uint32_t l_rn = r[8], mapq = r[9], n_cig = ld16(r + 12), flag = ld16(r + 14);
        const int32_t l_seq = ldi32(r + 16), tlen = ldi32(r + 28);
        if (l_seq < 0 || l_rn < 1 || 32 + (uint64_t)l_rn + 4 * (uint64_t)n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > (uint64_t)bs) { flags |= 1; break; }
        bool keep = ref >= 0 && ref < F.n_ref && F.ref_mask[ref] && (int)mapq >= F.min_mapq && ((int)flag & F.flag_required) == F.flag_required &&
                    ((int)flag & F.flag_forbidden) == 0;
        if (keep && F.isize_cutoff != 0) { const double tl = tlen < 0 ? -(double)tlen : (double)tlen; keep = tl <= F.isize_cutoff; }
        if (keep) {
            const int32_t pos0 = ldi32(r + 4);
            if (last_ref != -2 && (ref < last_ref || (ref == last_ref && pos0 < last_pos))) flags |= 4;
            if (first_ref == -2) { first_ref = ref; first_pos = pos0; }
            last_ref = ref; last_pos = pos0;
            if (!WRITE) {
                const uint8_t *qual0 = r + 32 + l_rn + 4 * (uint64_t)n_cig + ((uint64_t)l_seq + 1) / 2;
                const uint32_t nb0 = l_seq <= 0 ? 1u : (qual0[0] == 0xFF ? 1u : (uint32_t)l_seq);
                sq_sum += (nb0 + 3) / 4; qn_sum += l_rn - 1; op_sum += 2 * (uint64_t)n_cig;
            }
            if (WRITE) {
                const uint8_t *cig = r + 32 + l_rn;
                const uint8_t *qual = cig + 4 * (uint64_t)n_cig + ((uint64_t)l_seq + 1) / 2;
                uint32_t nb;
                if (l_seq <= 0) nb = 1; else nb = qual[0] == 0xFF ? 1u : (uint32_t)l_seq;
                K.off[w] = p + 4; K.ref[w] = ref; K.nops[w] = (uint32_t)norm_ops_dev(cig, (int)n_cig, (int)nb, nullptr);
                K.sq[w] = (nb + 3) / 4; K.nb[w] = nb; K.lqn[w] = l_rn - 1;
                w++;
            }
            kept++;
        }
        p += 4 + (uint64_t)bs;
    }
    if (!(flags & 1) && p != stop) flags |= 2;
    if (!WRITE) { SegOut o; o.kept = kept; o.flags = flags; o.first_ref = first_ref; o.first_pos = first_pos; o.last_ref = last_ref; o.last_pos = last_pos;
                  o.sq_sum = sq_sum; o.qn_sum = qn_sum; o.op_sum = op_sum; o.end_pos = p; so[k] = o; }
}

__global__ void k_seg_kept(const SegOut *so, int64_t nseg, uint32_t *kept) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nseg) kept[k] = so[k].kept;
}

// ref_begin[r] = first kept record with reference >= r (the list is grouped by reference: the file is coordinate-sorted)
__global__ void k_ref_bounds(const int32_t *ref, int64_t n, int n_ref, int64_t *ref_begin) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_ref) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (ref[m] < r) lo = m + 1; else hi = m; }
    ref_begin[r] = lo;
}

struct DevShard {               // device pointers of one reference's output arrays (caller-allocated)
    int32_t *pos; uint32_t *cigar_off, *cigar, *seq_off; uint8_t *seq2, *qual; int32_t *aln; uint8_t *has_as; uint32_t *qname_off; char *qnames;
};

// value of the last AS tag among the aux fields [p, e); false when absent (same walk as aux_as in phz_bam.cpp)
__device__ bool aux_as_dev(const uint8_t *p, const uint8_t *e, int32_t *out) {
    bool found = false;
    while (p + 3 <= e) {
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
        p += 3;
        uint64_t sz = 0;
        switch (ty) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'Z': case 'H': { const uint8_t *q = p; while (q < e && *q) q++; if (q >= e) return found; sz = (uint64_t)(q - p) + 1; break; }
            case 'B': {
                if (p + 5 > e) return found;
                const uint8_t sub = p[0];
                const uint32_t cnt = ld32(p + 1);
                uint64_t es = 0;
                switch (sub) { case 'c': case 'C': es = 1; break; case 's': case 'S': es = 2; break; case 'i': case 'I': case 'f': es = 4; break; default: return found; }
                sz = 5 + es * (uint64_t)cnt;
                break;
            }
            default: return found;
        }
        if (sz > (uint64_t)(e - p)) return found;
        if (t0 == 'A' && t1 == 'S' && ty != 'A' && ty != 'f' && ty != 'Z' && ty != 'H' && ty != 'B') {
            int32_t v = 0;
            switch (ty) {
                case 'c': v = (int8_t)p[0]; break;
                case 'C': v = p[0]; break;
                case 's': v = (int16_t)ld16(p); break;
                case 'S': v = (int32_t)ld16(p); break;
                case 'i': v = ldi32(p); break;
                case 'I': v = (int32_t)ld32(p); break;
            }
            *out = v; found = true;
        }
        p += sz;
    }
    return found;
}

// l_seq of the record at r (phase B needs it for the offset of the qualities)
__device__ __forceinline__ uint32_t nb_seq_len(const uint8_t *r) { const int32_t l = ldi32(r + 16); return l > 0 ? (uint32_t)l : 0u; }

__constant__ int8_t c_code_of[16] = {-2, 0, 1, -2, 2, -2, -2, -2, 3, -2, -2, -2, -2, -1, -2, -1};   // =ACMGRSVTWYHKDBN

// One wave per 64 kept records.  Phase A, lane = record: the scalar columns, the normalised CIGAR and the AS tag (a few dependent
// loads per lane).  Phase B, lane = byte: the wave walks its 64 records and moves each one's name, bases and qualities with
// coalesced accesses -- a lane reading its own record byte by byte pulls a whole cache line per byte through L2 (the first version
// of this kernel did, and was bound by exactly that: 0.21 s for 59M records).
__global__ __launch_bounds__(256) void k_pack(const uint8_t *d, KeptOut K, int64_t n_kept, const int64_t *ref_begin, const uint32_t *co,
                                              const uint32_t *so, const uint32_t *qo, const DevShard *shards) {
    __shared__ const uint8_t *s_src[256];
    __shared__ char *s_qn[256];
    __shared__ uint8_t *s_o2[256], *s_oq[256];
    __shared__ uint32_t s_meta[256];           // l_rn | n_cig << 8 | star << 24 (SEQ '*')
    __shared__ uint32_t s_nb[256];
    const int tid = threadIdx.x, lane = tid & 63, wbase = tid & ~63;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const bool live = i < n_kept;
    if (live) {
        const int ref = K.ref[i];
        const int64_t b = ref_begin[ref], e = ref_begin[ref + 1];
        const int64_t k = i - b;
        const DevShard S = shards[ref];
        const uint32_t c0 = co[i] - co[b], s0 = so[i] - so[b], q0 = qo[i] - qo[b];
        const uint8_t *r = d + K.off[i];
        const uint32_t l_rn = r[8], n_cig = ld16(r + 12);
        const int32_t l_seq = ldi32(r + 16);
        const int32_t bs = ldi32(r - 4);
        const uint32_t nb = K.nb[i];
        S.pos[k] = ldi32(r + 4) + 1;
        S.cigar_off[k] = c0; S.seq_off[k] = s0; S.qname_off[k] = q0;
        if (i + 1 == e) { S.cigar_off[k + 1] = co[e] - co[b]; S.seq_off[k + 1] = so[e] - so[b]; S.qname_off[k + 1] = qo[e] - qo[b]; }
        const uint8_t *cig = r + 32 + l_rn;
        norm_ops_dev(cig, (int)n_cig, (int)nb, S.cigar + c0);
        const uint8_t *ql = cig + 4 * (uint64_t)n_cig + ((uint64_t)(l_seq > 0 ? l_seq : 0) + 1) / 2;
        int32_t as = 0;
        const bool has = aux_as_dev(ql + (l_seq > 0 ? l_seq : 0), r + bs, &as);
        S.aln[k] = has ? as : 0; S.has_as[k] = has ? 1 : 0;
        s_src[tid] = r; s_qn[tid] = S.qnames + q0; s_o2[tid] = S.seq2 + s0; s_oq[tid] = S.qual + (uint64_t)s0 * 4;
        s_meta[tid] = l_rn | (n_cig << 8) | (l_seq <= 0 ? 1u << 24 : 0u);
        s_nb[tid] = nb;
    } else {
        s_nb[tid] = 0; s_meta[tid] = 0;
    }
    __syncthreads();
    for (int j = 0; j < 64; j++) {
        const uint32_t nb = s_nb[wbase + j];
        if (nb == 0) continue;                 // record beyond the end of the list
        const uint32_t meta = s_meta[wbase + j];
        const uint32_t l_rn = meta & 0xFF, n_cig = (meta >> 8) & 0xFFFF;
        const uint8_t *r = s_src[wbase + j];
        char *qn = s_qn[wbase + j];
        for (uint32_t t = lane; t + 1 < l_rn; t += 64) qn[t] = (char)r[32 + t];
        uint8_t *o2 = s_o2[wbase + j], *oq = s_oq[wbase + j];
        if (meta >> 24) {                      // SEQ '*' QUAL '*': one IUPAC-other character with phred 9
            if (lane < 4) oq[lane] = lane == 0 ? (uint8_t)(9 | 0x80) : 0;
            if (lane == 0) o2[0] = 1;
            continue;
        }
        const uint8_t *sq = r + 32 + l_rn + 4 * (uint64_t)n_cig;
        const uint8_t *ql = sq + ((uint64_t)nb_seq_len(r) + 1) / 2;
        const bool noq = ql[0] == 0xFF;
        const uint32_t padded = ((nb + 3) / 4) * 4;
        for (uint32_t jb = lane; jb < ((padded + 63) & ~63u); jb += 64) {
            uint32_t code2 = 0; uint8_t q = 0;
            if (jb < nb) {
                const uint8_t by = sq[jb >> 1];
                const uint8_t nib = (jb & 1) ? (by & 15) : (by >> 4);
                const int c = c_code_of[nib];
                q = noq ? 9 : (ql[jb] > 127 ? 127 : ql[jb]);
                if (c >= 0) code2 = (uint32_t)c; else { code2 = c == -1 ? 0u : 1u; q |= 0x80; }
            }
            uint32_t v = code2 << (2 * (jb & 3));
            v |= __shfl_xor(v, 1); v |= __shfl_xor(v, 2);
            if (jb < padded) {
                oq[jb] = q;
                if ((jb & 3) == 0) o2[jb >> 2] = (uint8_t)v;
            }
        }
    }
}

// ---- QNAME interning on the device: ids in first-appearance order (what a sequential dictionary would hand out; mates and
// repeated templates share an id), continuing the numbering of the BAMs seen before.  The names of the ids handed out so far live
// in a device-side store (blob + offsets, id order).  Per call: an open-addressing table keyed by a 64-bit hash of the name, equality
// decided by comparing the name bytes; a slot belongs to one name for good.  Slot values: an OLD id (< 2^31), or 2^31 | record index
// of a name that is new in this call -- that value converges to the smallest record index of the name.
constexpr uint32_t NEWBIT = 0x80000000u, EMPTY = 0xFFFFFFFFu;
__device__ __forceinline__ uint64_t name_hash(const char *p, uint32_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t i = 0; i < n; i++) { h ^= (uint8_t)p[i]; h *= 0x100000001b3ull; }
    h ^= h >> 29; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 32;
    return h;
}
__device__ __forceinline__ bool bytes_eq(const char *pa, uint32_t la, const char *pb, uint32_t lb) {
    if (la != lb) return false;
    for (uint32_t i = 0; i < la; i++) if (pa[i] != pb[i]) return false;
    return true;
}
// the names already in the store claim their slots (they are distinct: no comparisons)
__global__ __launch_bounds__(256) void k_intern_old(const char *store, const uint32_t *store_off, int64_t n_old, uint32_t *table, uint32_t mask) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n_old) return;
    uint32_t s = (uint32_t)name_hash(store + store_off[id], store_off[id + 1] - store_off[id]) & mask;
    while (atomicCAS(&table[s], EMPTY, (uint32_t)id) != EMPTY) s = (s + 1) & mask;
}
__global__ __launch_bounds__(256) void k_intern_insert(const char *blob, const uint32_t *off, int64_t n, const char *store, const uint32_t *store_off,
                                                       uint32_t *table, uint32_t mask, uint32_t *slot_of) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const char *nm = blob + off[i];
    const uint32_t ln = off[i + 1] - off[i];
    const uint32_t mine = NEWBIT | (uint32_t)i;
    uint32_t s = (uint32_t)name_hash(nm, ln) & mask;
    for (;;) {
        uint32_t cur = table[s];
        if (cur == EMPTY) {
            cur = atomicCAS(&table[s], EMPTY, mine);
            if (cur == EMPTY) break;                             // claimed for this name
        }
        if (cur & NEWBIT) {                                      // a name that is new in this call: compare with that record's name
            const uint32_t j = cur & ~NEWBIT;
            if (j == (uint32_t)i || bytes_eq(nm, ln, blob + off[j], off[j + 1] - off[j])) { atomicMin(&table[s], mine); break; }
        } else if (bytes_eq(nm, ln, store + store_off[cur], store_off[cur + 1] - store_off[cur])) break;      // a name of an earlier BAM
        s = (s + 1) & mask;
    }
    slot_of[i] = s;
}
__global__ __launch_bounds__(256) void k_intern_first(const uint32_t *table, const uint32_t *slot_of, int64_t n, uint32_t *first) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) first[i] = table[slot_of[i]] == (NEWBIT | (uint32_t)i) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_intern_assign(const uint32_t *table, const uint32_t *slot_of, const uint32_t *first, const uint32_t *rank, int64_t n,
                                                       int32_t base, int32_t *qid, int32_t *first_idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = table[slot_of[i]];
    qid[i] = (v & NEWBIT) ? base + (int32_t)rank[v & ~NEWBIT] : (int32_t)v;
    if (first[i]) first_idx[rank[i]] = (int32_t)i;
}
// the names of the new ids appended to a store: name k = blob[off[first_idx[k]] ..), written at dst_off[k]
__global__ __launch_bounds__(256) void k_names_gather(const char *blob, const uint32_t *off, const int32_t *first_idx, int64_t m, const uint32_t *dst_off, char *dst) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const int32_t i = first_idx[k];
    const char *src = blob + off[i];
    const uint32_t ln = off[i + 1] - off[i];
    char *d = dst + dst_off[k];
    for (uint32_t t = 0; t < ln; t++) d[t] = src[t];
}
__global__ void k_add_u32(uint32_t *a, int64_t n, uint32_t x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] += x;
}
__global__ __launch_bounds__(256) void k_names_len(const uint32_t *off, const int32_t *first_idx, int64_t m, uint32_t *len) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < m) { const int32_t i = first_idx[k]; len[k] = off[i + 1] - off[i]; }
}

}  // namespace

// The two big buffers of a device BAM read are kept in the ctx between calls (the larger one wins a slot): take / give back.  keep = BamKnobs::keep_buffers
static void *bam_take(DevBuf *slot, size_t bytes, size_t *cap, bool keep) {
    if (slot && slot->p && slot->cap >= bytes) { void *p = slot->p; *cap = slot->cap; slot->p = nullptr; slot->cap = 0; return p; }
    // a fresh buffer gets ~3 % + 64 MB of head room: the BAMs of one sample differ by fractions of a percent, and a buffer cut to the byte sent every slightly larger
    // file to a new 15 GB hipMalloc (0.2-0.7 s each time on this runtime: profiles/r06/cli_4bam_full_before.txt, 'device buffers 684 ms' at the third of four BAMs)
    void *p = nullptr;
    const size_t roomy = bytes + bytes / 32 + ((size_t)64 << 20);
    if (keep && hipMalloc(&p, roomy) == hipSuccess) { *cap = roomy; return p; }
    (void)hipGetLastError();
    p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    *cap = bytes;
    return p;
}
static void bam_give_back(DevBuf *slot, void *p, size_t cap, bool keep) {
    if (!p) return;
    if (slot && keep && cap > slot->cap) { if (slot->p) (void)hipFree(slot->p); slot->p = p; slot->cap = cap; return; }
    (void)hipFree(p);
}

// (struct phz_bamdev: phz_bamdev_internal.h)
phz_bamdev::~phz_bamdev() {
    if (d_stream) bam_give_back(ctx ? &ctx->bam_stream : nullptr, d_stream, d_stream_cap, keep_buffers);
    if (d_work) bam_give_back(ctx ? &ctx->bam_work : nullptr, d_work, d_work_cap, keep_buffers);
}

namespace {

// The switches of one phz_bamdev_open, read once at its top (tests change them between calls on one ctx): nothing below this struct calls getenv
struct BamKnobs {
    static constexpr int NCOPY_MAX = 16;
    bool timing;                 // PHZ_TIMING: the [phz timing] lines
    bool force_nomem;            // PHZ_BAMDEV_FORCE_NOMEM=1 (tests): the out-of-memory exit without exhausting a GPU
    bool crc;                    // PHZ_BAM_CRC=0 skips the check of every member's output against the CRC32 of its trailer
    bool keep_buffers;           // PHZ_BAM_KEEP_BUFFERS=0 turns the ctx's cache of the big buffers off
    bool many_queues;            // GPU_MAX_HW_QUEUES >= 16 (PHZ_HW_QUEUES_LATE: the variable was set after the runtime had started, so it does not count)
    int ncopy;                   // PHZ_BAM_NCOPY = 1..16: host threads (and streams) that read the file and send it over
    int inflate_streams;         // PHZ_BAM_INFLATE_STREAMS = 1..8
    uint64_t chunk_bytes;        // PHZ_BAM_CHUNK_MB: compressed bytes per K_inflate launch
    uint64_t limit;              // PHZ_BAMDEV_LIMIT: the 32-bit limit of a call's byte sums (tests lower it to exercise the caller's split)
    uint64_t slice_min;          // PHZ_BAM_SLICE_MIN_KB (65536): a chunk of at least this many bytes goes over in ncopy slices
    uint64_t stage_bytes;        // PHZ_BAM_STAGE_KB (8192): one page-locked staging buffer; a multiple of 4 KB, at least 4.  Tests lower these two so that a small
                                 // file goes through the threaded staging copy and reuses its buffers
    static long long num(const char *name, long long dflt) { const char *e = getenv(name); return e ? atoll(e) : dflt; }
    // K_inflate launches of consecutive chunks overlap only when their streams sit on different HARDWARE queues: the runtime spreads a process's streams over
    // GPU_MAX_HW_QUEUES of them (default 4) and this call alone has eight copy streams -- a copy stream that shares the queue of a running K_inflate waits
    // behind it, which serialised everything (profiles/r05/bam_device_sweep_streams.txt: 12 chunks on 4 streams 0.69 s with 4 queues, 0.30 s with 16).  With
    // >= 16 queues (the package asks for them before the runtime starts, phaser_amd/__init__.py): 3 streams x 1,280 MB chunks, file -> shards 0.24 s; a host
    // application that keeps the runtime's default gets ONE launch per 4 GB (0.27 s; 0.32 s with the old 1,280 MB chunks on one stream).
    // A launch lasts as long as its slowest member (60-100 ms) however few it holds, and the chip holds 262,000 members at once: big chunks.
    BamKnobs() {
        timing = getenv("PHZ_TIMING") != nullptr;
        force_nomem = getenv("PHZ_BAMDEV_FORCE_NOMEM") != nullptr;
        crc = num("PHZ_BAM_CRC", 1) != 0;
        keep_buffers = num("PHZ_BAM_KEEP_BUFFERS", 1) != 0;
        many_queues = num("GPU_MAX_HW_QUEUES", 0) >= 16 && getenv("PHZ_HW_QUEUES_LATE") == nullptr;
        const long long nc = num("PHZ_BAM_NCOPY", 8), ns = num("PHZ_BAM_INFLATE_STREAMS", 0), mb = num("PHZ_BAM_CHUNK_MB", 0);
        ncopy = nc >= 1 && nc <= NCOPY_MAX ? (int)nc : 8;
        inflate_streams = ns >= 1 && ns <= 8 ? (int)ns : (many_queues ? 3 : 1);
        chunk_bytes = (uint64_t)(mb > 0 ? mb : (many_queues ? 1280 : 4096)) << 20;
        limit = (uint64_t)num("PHZ_BAMDEV_LIMIT", (1ll << 32) - 16);
        const long long sl = num("PHZ_BAM_SLICE_MIN_KB", 65536), sk = num("PHZ_BAM_STAGE_KB", 8192);
        slice_min = (uint64_t)(sl > 0 ? sl : 65536) << 10;
        stage_bytes = (uint64_t)((sk < 4 ? 4 : sk) & ~3ll) << 10;
    }
};

// ---- What the plan and the chunk size decide, computed on the host before anything touches the device.
// Compressed side: one contiguous file range per run of members (a gap of more than 64 KB starts a new run), the runs back to back in d_comp, 16-byte aligned.
// Inflated side: the needed members back to back in file order (mem[i].dst = where member i's output starts in the device stream).
struct BamChunk { size_t first, count; uint64_t a, b; size_t run; };      // members [first, first + count) of one K_inflate launch, their file range [a, b), its run
struct BamLayout {
    static constexpr uint64_t SEG = 256u << 10;
    const PhzBamPlan *plan = nullptr;
    std::vector<std::pair<uint64_t, uint64_t>> runs;          // file ranges [a, b)
    std::vector<uint64_t> run_dev;                            // their offsets in the device buffer
    std::vector<phz_bgzf_member> mem;                         // device member table: src = offset in d_comp, dst = offset in the inflated stream
    std::vector<uint32_t> crcs;                               // the trailers' CRC32s, member order
    uint64_t comp_bytes = 0, out_bytes = 0;
    std::vector<BamChunk> chunks;
    std::vector<Seg> segs;                                    // the inflated stream's pieces cut every SEG bytes (exact = the piece's own start: a known boundary)

    void build(const PhzBamPlan &p, uint64_t chunk_bytes) {
        plan = &p;
        const auto &M = p.members;
        uint64_t run_a = 0, run_b = 0;
        for (size_t i = 0; i < M.size(); i++) {
            const uint64_t a = M[i].src, b = M[i].src + M[i].csize;
            if (i == 0 || a > run_b + 65536) {
                if (i) runs.emplace_back(run_a, run_b);
                run_a = a; run_b = b;
            } else run_b = b;
        }
        runs.emplace_back(run_a, run_b);
        for (auto &r : runs) { run_dev.push_back(comp_bytes); comp_bytes += (r.second - r.first + 15) & ~(uint64_t)15; }
        mem.resize(M.size()); crcs.resize(M.size());
        for (size_t i = 0, ri = 0; i < M.size(); i++) {
            while (ri + 1 < runs.size() && M[i].src >= runs[ri].second) ri++;
            mem[i].src = run_dev[ri] + (M[i].src - runs[ri].first);
            mem[i].csize = M[i].csize; mem[i].isize = M[i].isize; mem[i].dst = out_bytes;
            crcs[i] = M[i].crc;
            out_bytes += M[i].isize;
        }
        // chunks: members of one run, up to chunk_bytes of file (a chunk's first member may reach twice that)
        for (size_t i0 = 0, ri = 0; i0 < M.size();) {
            while (ri + 1 < runs.size() && M[i0].src >= runs[ri].second) ri++;
            size_t i1 = i0;
            const uint64_t a = M[i0].src;
            uint64_t bnd = a;
            while (i1 < M.size() && M[i1].src < runs[ri].second && M[i1].src + M[i1].csize - a <= chunk_bytes + (i1 == i0 ? chunk_bytes : 0)) {
                bnd = M[i1].src + M[i1].csize; i1++;
            }
            if (i1 == i0) { bnd = M[i0].src + M[i0].csize; i1 = i0 + 1; }
            chunks.push_back({i0, i1 - i0, a, bnd, ri});
            i0 = i1;
        }
        for (size_t pi = 0; pi < p.pieces.size(); pi++) {
            const uint64_t a = dev_of(p.pieces[pi].first), b = a + (p.pieces[pi].second - p.pieces[pi].first);
            for (uint64_t g = a; g < b; g += SEG) segs.push_back({g, b, g == a ? 1u : 0u, (uint32_t)pi});
        }
    }
    uint64_t dev_of(uint64_t u) const {                       // global inflated offset -> device stream offset
        const auto &M = plan->members;
        size_t lo = 0, hi = M.size();
        while (lo < hi) { const size_t m = (lo + hi) >> 1; if (M[m].dst + M[m].isize <= u) lo = m + 1; else hi = m; }
        if (lo >= M.size()) return out_bytes;                 // u == end of the last member
        return mem[lo].dst + (u - M[lo].dst);
    }
    uint64_t comp_at(const BamChunk &c) const { return run_dev[c.run] + (c.a - runs[c.run].first); }      // where the chunk's bytes go in d_comp
};

// ---- the two allocations the driver carves into parts, every part 256-byte aligned: byte offsets computed once, typed pointers handed out
static size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }
template <class T> static T *bam_part(void *p, size_t off) { return (T *)((char *)p + off); }
// BamOpen::d_seg: [Seg x nseg][start x (nseg + 1)][SegOut x nseg][kept x (nseg + 2)][kbase x (nseg + 2)][reference mask x n_ref]
struct SegCarve {
    size_t off_start = 0, off_so = 0, off_kept = 0, off_kbase = 0, off_mask = 0, bytes = 0;
    SegCarve() {}
    SegCarve(int64_t nseg, int n_ref) {
        off_start = al256((size_t)nseg * sizeof(Seg)); off_so = off_start + al256((size_t)(nseg + 1) * 8); off_kept = off_so + al256((size_t)nseg * sizeof(SegOut));
        off_kbase = off_kept + al256((size_t)(nseg + 2) * 4); off_mask = off_kbase + al256((size_t)(nseg + 2) * 4); bytes = off_mask + al256((size_t)n_ref);
    }
    Seg *segs(void *p) const { return bam_part<Seg>(p, 0); }
    uint64_t *start(void *p) const { return bam_part<uint64_t>(p, off_start); }
    SegOut *so(void *p) const { return bam_part<SegOut>(p, off_so); }
    uint32_t *kept(void *p) const { return bam_part<uint32_t>(p, off_kept); }
    uint32_t *kbase(void *p) const { return bam_part<uint32_t>(p, off_kbase); }
    uint8_t *mask(void *p) const { return bam_part<uint8_t>(p, off_mask); }
};
// phz_bamdev::d_work: [KeptOut.off x n][KeptOut.ref, nops, sq, nb, lqn x (n + 1)][co, so, qo x (n + 1)][ref_begin x (n_ref + 2)], n = kept records (at least 1)
struct KeptCarve {
    size_t a8, a4, rb;
    KeptCarve(int64_t nk, int n_ref) : a8(al256((size_t)(nk ? nk : 1) * 8)), a4(al256(((size_t)(nk ? nk : 1) + 1) * 4)), rb(al256((size_t)(n_ref + 2) * 8)) {}
    size_t bytes() const { return a8 + 8 * a4 + rb; }
    template <class T> T *word(void *p, int k) const { return bam_part<T>(p, a8 + (size_t)k * a4); }          // the k-th of the eight 4-byte arrays
    void point(phz_bamdev *h) const {
        void *p = h->d_work;
        h->K.off = bam_part<uint64_t>(p, 0);
        h->K.ref = word<int32_t>(p, 0); h->K.nops = word<uint32_t>(p, 1); h->K.sq = word<uint32_t>(p, 2); h->K.nb = word<uint32_t>(p, 3); h->K.lqn = word<uint32_t>(p, 4);
        h->co = word<uint32_t>(p, 5); h->so = word<uint32_t>(p, 6); h->qo = word<uint32_t>(p, 7);
        h->d_ref_begin = bam_part<int64_t>(p, a8 + 8 * a4);
    }
};

// What one phz_bamdev_open knows and OWNS: the plan, the handle until success hands it to the caller, the compressed copy and the member table, the copy and
// inflate streams, the staging events, the file descriptor, the segment allocation.  Its functions are the stages of the call in stream order (run()).
// THE RULE of its clean-up: no buffer goes back to the ctx cache or to the runtime while work that touches it can still be queued.  So the destructor, which
// every exit goes through, releases in ONE order: the inflate streams, then the copy streams (each waited for, then destroyed), the events, the file
// descriptor; on a failing exit a wait for the ctx stream (the hop or a scan may still be queued on the handle's buffers); only then d_comp back to the cache,
// d_mem and d_seg freed, the plan released and the handle, unless it was handed over, deleted (its two buffers return to the cache).  A successful call has
// released each of these at its old place in the sequence already (the drop_* functions release once), and pays nothing here.
struct BamOpen {
    using Clock = std::chrono::steady_clock;
    phz_ctx *const ctx; const char *const path; const char *const *const ref_names; const int n_names; const phz_bam_filters *const f; phz_bamdev **const out;
    const BamKnobs knobs;
    const hipStream_t sm; const hipEvent_t e0, e1;
    int status = PHZ_OK;
    // owned (see above)
    PhzBamPlan plan; phz_bamdev *h = nullptr;
    void *d_comp = nullptr; size_t d_comp_cap = 0; void *d_mem = nullptr, *d_seg = nullptr;
    hipStream_t cs[BamKnobs::NCOPY_MAX] = {}; std::vector<hipStream_t> is; hipEvent_t stage_ev[BamKnobs::NCOPY_MAX * 2] = {}; int fd = -1;
    // what a stage leaves for the next ones
    BamLayout L; int n_ref = 0;
    int *d_status = nullptr; bool stage_ok = false; int n_is = 1, n_launch = 0, n_slices = 0; long long n_rounds = 0;
    SegCarve seg; int64_t nseg = 0; unsigned gseg = 0; Filters F{}; std::vector<uint8_t> mask; std::vector<SegOut> hso; uint32_t total_kept = 0;
    Clock::time_point t_lap = Clock::now(), t_h2d0; double h2d_ms = 0; float inflate_ms = 0;

    BamOpen(phz_ctx *c, const char *path_, const char *const *ref_names_, int n_names_, const phz_bam_filters *f_, phz_bamdev **out_)
        : ctx(c), path(path_), ref_names(ref_names_), n_names(n_names_), f(f_), out(out_), sm(c->stream), e0(c->ev0), e1(c->ev1) {}
    ~BamOpen() {
        drop_inflate_streams(); drop_copy_streams(); drop_staging();
        if (status != PHZ_OK) (void)hipStreamSynchronize(sm);
        drop_compressed(); drop_segments();
        phz_bam_plan_release(&plan);
        delete h;
        // Every allocation failure of the device path is PHZ_E_NOMEM (the caller then decodes the file on the host; earlier BAMs' shards stay resident, so HBM can
        // legitimately be short here), and the runtime's sticky last-error is cleared so that the next kernel-launch check of this ctx does not report a stale
        // out-of-memory
        if (status == PHZ_E_NOMEM) (void)hipGetLastError();
    }
    void drop_inflate_streams() { for (auto &s : is) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); s = nullptr; } }
    void drop_copy_streams() { for (auto &c : cs) if (c) { (void)hipStreamSynchronize(c); (void)hipStreamDestroy(c); c = nullptr; } }
    void drop_staging() { for (auto &e : stage_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } if (fd >= 0) { ::close(fd); fd = -1; } }
    void drop_compressed() { bam_give_back(&ctx->bam_comp, d_comp, d_comp_cap, knobs.keep_buffers); d_comp = nullptr; if (d_mem) { (void)hipFree(d_mem); d_mem = nullptr; } }
    void drop_segments() { if (d_seg) { (void)hipFree(d_seg); d_seg = nullptr; } }

    int fail(int code, const char *what) { if (what) ctx->err = what; status = code; return code; }      // every failing exit: the destructor does the rest
    int hand_over() { *out = h; h = nullptr; return PHZ_OK; }
    void lap(const char *what) {
        if (!knobs.timing) return;
        const auto now = Clock::now();
        fprintf(stderr, "[phz timing]     bam device: %-40s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_lap).count());
        t_lap = now;
    }

    int run() {
        if (int st = make_plan()) return st;
        if (plan.members.empty() || plan.pieces.empty()) return hand_over();         // no wanted record in the file: a handle without records
        if (hipSetDevice(ctx->device) != hipSuccess) return fail(PHZ_E_HIP, nullptr);
        L.build(plan, knobs.chunk_bytes);
        if (int st = device_buffers()) return st;
        if (int st = upload_tables()) return st;
        if (int st = copy_and_inflate()) return st;
        if (L.segs.empty()) return hand_over();
        if (int st = segments()) return st;
        if (int st = counting_hop()) return st;
        if (int st = host_checks()) return st;
        if (int st = kept_list()) return st;
        if (int st = read_backs()) return st;
        return hand_over();
    }

    // ---- 1. plan (host: member table, header, chromosome ranges) and the handle
    int make_plan() {
        if (int st = phz_bam_plan_file(path, ref_names, n_names, &plan)) return fail(st, nullptr);
        lap("plan (member table, header, chromosome ranges)");
        h = new phz_bamdev();
        h->ctx = ctx; h->keep_buffers = knobs.keep_buffers;
        h->refs = plan.refs;
        n_ref = (int)plan.refs.size();
        h->ref_begin.assign((size_t)n_ref + 1, 0);
        h->h_co.assign((size_t)n_ref + 1, 0); h->h_so.assign((size_t)n_ref + 1, 0); h->h_qo.assign((size_t)n_ref + 1, 0);
        return PHZ_OK;
    }
    // ---- 3. device buffers: compressed copy, member table + the trailers' CRC32s behind it, inflated stream.  Short of memory: the kept buffers (too small for
    // this file) go back to the runtime, then one more try
    int device_buffers() {
        bool got = false;
        for (int attempt = 0; attempt < 2 && !knobs.force_nomem && !got; attempt++) {
            d_comp = bam_take(&ctx->bam_comp, L.comp_bytes + 64, &d_comp_cap, knobs.keep_buffers);
            if (d_comp && hipMalloc(&d_mem, L.mem.size() * sizeof(phz_bgzf_member) + L.mem.size() * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); d_mem = nullptr; }
            if (d_comp && d_mem) h->d_stream = bam_take(&ctx->bam_stream, L.out_bytes + 64, &h->d_stream_cap, knobs.keep_buffers);
            got = d_comp && d_mem && h->d_stream;
            if (!got) {
                if (d_comp) { (void)hipFree(d_comp); d_comp = nullptr; }
                if (d_mem) { (void)hipFree(d_mem); d_mem = nullptr; }
                if (h->d_stream) { (void)hipFree(h->d_stream); h->d_stream = nullptr; }
                for (DevBuf *b : {&ctx->bam_comp, &ctx->bam_stream, &ctx->bam_work}) if (b->p) { (void)hipFree(b->p); *b = DevBuf(); }
            }
        }
        if (!got) return fail(PHZ_E_NOMEM, "device BAM buffers");
        lap("device buffers");
        return PHZ_OK;
    }
    uint32_t *d_crc() const { return (uint32_t *)((char *)d_mem + L.mem.size() * sizeof(phz_bgzf_member)); }
    // ---- 4. upload of the member table, the CRC32s and the cleared status word on the ctx stream.  (The wall-clock figure of the summary line starts here, and
    // the copy streams are made here: ncopy of them, one per host thread of copy_chunk)
    int upload_tables() {
        t_h2d0 = Clock::now();
        for (int t = 0; t < knobs.ncopy; t++) if (hipStreamCreateWithFlags(&cs[t], hipStreamNonBlocking) != hipSuccess) cs[t] = nullptr;
        if (phz_reserve(ctx, ctx->scalars, 64) != PHZ_OK ||
            phz_reserve(ctx, ctx->scratch[SC_INFLATE_LENS], L.mem.size() * (size_t)phz_inflate_scratch_bytes_per_member()) != PHZ_OK) return fail(PHZ_E_NOMEM, nullptr);
        d_status = (int *)ctx->scalars.p;
        (void)hipMemsetAsync(d_status, 0, 4, sm);
        (void)hipMemcpyAsync(d_mem, L.mem.data(), L.mem.size() * sizeof(phz_bgzf_member), hipMemcpyHostToDevice, sm);
        // every member's output is checked against the CRC32 of its trailer after it has been inflated (htslib does, so the reference's `samtools view` stops on a
        // damaged file that is still valid DEFLATE)
        if (knobs.crc) (void)hipMemcpyAsync(d_crc(), L.crcs.data(), L.crcs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, sm);
        (void)hipEventRecord(e0, sm);
        return PHZ_OK;
    }
    // ---- 5. copy + inflate pipeline.  H2D and K_inflate overlapped: the members go over chunk by chunk on the copy streams, and each chunk's members are inflated
    // as soon as its bytes have arrived -- on n_is streams in turn, so that a chunk's members start while the previous launches are still running (BamKnobs) and the
    // copy of chunk c + 1 runs while chunk c inflates.  Then the verdict on the status word.
    int copy_and_inflate() {
        if (int st = reserve_staging()) return st;
        start_inflate_streams();
        for (const BamChunk &c : L.chunks) {
            if (int st = copy_chunk(c)) return st;
            hipStream_t si = n_is > 1 ? is[(size_t)(n_launch % n_is)] : sm;
            int st = phz_inflate_launch(ctx, (const uint8_t *)d_comp, (const phz_bgzf_member *)d_mem, (int64_t)c.first, (int64_t)c.count, (uint8_t *)h->d_stream,
                                        (uint8_t *)ctx->scratch[SC_INFLATE_LENS].p, d_status, si);
            if (st == PHZ_OK && knobs.crc) st = phz_crc_launch(ctx, (const phz_bgzf_member *)d_mem, (int64_t)c.first, (int64_t)c.count, (const uint8_t *)h->d_stream, d_crc(), d_status, si);
            n_launch++;
            if (st != PHZ_OK) return fail(st, nullptr);
        }
        return verdict();
    }
    // page-locked staging: ncopy threads x 2 buffers, kept in the ctx for the next BAM of the sample, one event per buffer; without it the mapped file
    int reserve_staging() {
        fd = ::open(path, O_RDONLY);
        stage_ok = fd >= 0 && phz_reserve_host(ctx, ctx->h_bam_stage, (size_t)knobs.ncopy * 2 * knobs.stage_bytes) == PHZ_OK;
        if (!stage_ok) {
            (void)hipGetLastError();
            if (!phz_bam_plan_map(&plan)) return fail(PHZ_E_NOMEM, nullptr);          // no page-locked staging and no mapping either
        }
        for (int t = 0; t < knobs.ncopy * 2; t++) if (stage_ok && hipEventCreateWithFlags(&stage_ev[t], hipEventDisableTiming) != hipSuccess) stage_ev[t] = nullptr;
        return PHZ_OK;
    }
    void start_inflate_streams() {
        n_is = knobs.inflate_streams;
        is.assign((size_t)n_is, nullptr);
        if (n_is == 1) return;
        (void)hipStreamSynchronize(sm);                  // the member table and the cleared status word are on the device before any other stream reads them
        bool all = true;
        for (auto &s : is) if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { s = nullptr; all = false; }
        if (!all) { drop_inflate_streams(); n_is = 1; }          // one stream could not be made: every stream that was goes away again, the chunks take the ctx stream
    }
    // The chunk goes over in ncopy slices, each read by its own host thread with pread() into page-locked staging buffers of its own (two per thread, in turn: a
    // buffer is refilled once the event of its last copy has passed) and sent on its own stream.  Copying out of the mapped file instead -- pageable memory, staged
    // by the runtime at ~13 GB/s per thread -- also populated a page-table entry for every page of the file: 0.16 s of munmap afterwards for a 3.8 GB BAM, on top
    // of 0.34 s for the copy; it is what remains when the staging memory cannot be reserved.  Returns when the chunk is on the device.
    int copy_chunk(const BamChunk &c) {
        char *dst = (char *)d_comp + L.comp_at(c), *stage = (char *)ctx->h_bam_stage.p;
        const uint64_t a = c.a, len = c.b - c.a, SB = knobs.stage_bytes;
        const int nsl = (cs[0] && stage_ok && len >= knobs.slice_min) ? knobs.ncopy : 1;
        std::vector<std::thread> th;
        std::vector<int> thst((size_t)nsl, PHZ_OK), rounds((size_t)nsl, 0);
        for (int t = 0; t < nsl; t++)
            th.emplace_back([&, t] {
                (void)hipSetDevice(ctx->device);
                const uint64_t lo = (len * (uint64_t)t / (uint64_t)nsl) & ~(uint64_t)4095, hi = t + 1 == nsl ? len : ((len * (uint64_t)(t + 1) / (uint64_t)nsl) & ~(uint64_t)4095);
                hipStream_t s2 = cs[t] ? cs[t] : sm;
                if (!stage_ok) {
                    if (hipMemcpyAsync(dst + lo, plan.file + a + lo, hi - lo, hipMemcpyHostToDevice, s2) != hipSuccess) thst[(size_t)t] = PHZ_E_HIP;
                    (void)hipStreamSynchronize(s2);
                    return;
                }
                int which = 0;
                for (uint64_t o = lo; o < hi; o += SB, which ^= 1) {
                    const uint64_t m = hi - o < SB ? hi - o : SB;
                    char *sb = stage + ((size_t)t * 2 + (size_t)which) * SB;
                    const hipEvent_t ev = stage_ev[(size_t)t * 2 + (size_t)which];
                    if (ev && hipEventSynchronize(ev) != hipSuccess) { thst[(size_t)t] = PHZ_E_HIP; return; }
                    uint64_t got = 0;
                    while (got < m) {
                        const ssize_t r = pread(fd, sb + got, (size_t)(m - got), (off_t)(a + o + got));
                        if (r <= 0) { thst[(size_t)t] = PHZ_E_ARG; return; }
                        got += (uint64_t)r;
                    }
                    if (hipMemcpyAsync(dst + o, sb, m, hipMemcpyHostToDevice, s2) != hipSuccess) { thst[(size_t)t] = PHZ_E_HIP; return; }
                    if (ev) (void)hipEventRecord(ev, s2);
                    else (void)hipStreamSynchronize(s2);
                    rounds[(size_t)t]++;
                }
                (void)hipStreamSynchronize(s2);                   // the slice is on the device (and the staging buffers are free again)
            });
        for (auto &x : th) x.join();
        n_slices += nsl;
        for (int r : rounds) n_rounds += r;
        for (int v : thst) if (v != PHZ_OK) return fail(v, nullptr);
        return PHZ_OK;
    }
    int verdict() {
        drop_inflate_streams();
        (void)hipEventRecord(e1, sm);
        int bad = 0;
        (void)hipMemcpyAsync(&bad, d_status, 4, hipMemcpyDeviceToHost, sm);
        (void)hipStreamSynchronize(sm);
        drop_copy_streams(); drop_staging();
        h2d_ms = std::chrono::duration<double, std::milli>(Clock::now() - t_h2d0).count();
        (void)hipEventElapsedTime(&inflate_ms, e0, e1);
        ctx->last_ms[PHZ_T_INFLATE] = inflate_ms; ctx->total_ms[PHZ_T_INFLATE] += inflate_ms; ctx->launches[PHZ_T_INFLATE]++;
        drop_compressed();
        if (bad) return fail(PHZ_E_UNSUPPORTED, bad == 7 ? "a BGZF member does not give the CRC32 of its trailer" : "a BGZF member is not valid DEFLATE");
        lap("H2D + K_inflate (+ free of the compressed copy)");
        phz_bam_plan_release(&plan);         // closes the file (nothing was mapped unless the fallback copied out of a mapping)
        lap("release of the plan");
        return PHZ_OK;
    }
    // ---- 6. segments: the list, the mask of the wanted references and the filters on the device, the guessed first boundary of every segment
    int segments() {
        nseg = (int64_t)L.segs.size(); gseg = (unsigned)((nseg + 63) / 64);
        seg = SegCarve(nseg, n_ref);
        if (hipMalloc(&d_seg, seg.bytes) != hipSuccess) { d_seg = nullptr; return fail(PHZ_E_NOMEM, "device BAM segments"); }
        mask.assign((size_t)n_ref, ref_names ? 0 : 1);
        if (ref_names) for (int i = 0; i < n_ref; i++) for (int k = 0; k < n_names; k++) if (h->refs[(size_t)i].first == ref_names[k]) mask[(size_t)i] = 1;
        if (hipMemcpyAsync(seg.segs(d_seg), L.segs.data(), (size_t)nseg * sizeof(Seg), hipMemcpyHostToDevice, sm) != hipSuccess ||
            hipMemcpyAsync(seg.mask(d_seg), mask.data(), (size_t)n_ref, hipMemcpyHostToDevice, sm) != hipSuccess) return fail(PHZ_E_HIP, "hipMemcpyAsync");
        F.min_mapq = f->min_mapq; F.flag_required = f->flag_required; F.flag_forbidden = f->flag_forbidden; F.isize_cutoff = f->isize_cutoff;
        F.ref_mask = seg.mask(d_seg); F.n_ref = n_ref;
        (void)hipEventRecord(e0, sm);
        hipLaunchKernelGGL(k_seg_start, dim3(gseg), dim3(64), 0, sm, (const uint8_t *)h->d_stream, (const Seg *)seg.segs(d_seg), nseg, n_ref, seg.start(d_seg));
        return PHZ_OK;
    }
    // ---- 7. The counting hop, repeated while a guessed boundary turns out to be a fake (a byte pattern inside a record that passes the plausibility chain):
    // segment k's chain is the truth when its own start is, so where it ARRIVES becomes the start of segment k + 1, and the hop runs again.  Every boundary is
    // verified in the end, or the file goes to the host path.  Then the kept counts of the segments, scanned.
    int counting_hop() {
        const uint8_t *d = (const uint8_t *)h->d_stream;
        const Seg *dsegs = seg.segs(d_seg); uint64_t *dstart = seg.start(d_seg); SegOut *dso = seg.so(d_seg);
        const auto &segs = L.segs;
        hso.resize((size_t)nseg);
        for (int pass = 0;; pass++) {
            hipLaunchKernelGGL(k_hop<0>, dim3(gseg), dim3(64), 0, sm, d, dsegs, nseg, (const uint64_t *)dstart, F, dso, (const uint32_t *)nullptr, KeptOut{});
            if (hipMemcpyAsync(hso.data(), dso, (size_t)nseg * sizeof(SegOut), hipMemcpyDeviceToHost, sm) != hipSuccess || hipStreamSynchronize(sm) != hipSuccess)
                return fail(PHZ_E_HIP, "segment read-back");
            int repaired = 0;
            bool prev_clean = true;
            for (int64_t k = 0; k < nseg; k++) {
                const SegOut &o = hso[(size_t)k];
                const bool last_of_piece = !(k + 1 < nseg && segs[(size_t)k + 1].piece == segs[(size_t)k].piece);
                if ((o.flags & 1) && prev_clean) return fail(PHZ_E_ARG, "truncated or corrupt BAM record");
                if ((o.flags & 2) && prev_clean) {
                    if (last_of_piece) return fail(PHZ_E_ARG, "truncated or corrupt BAM record");      // ran past the end of the piece
                    if (hipMemcpyAsync(dstart + k + 1, &hso[(size_t)k].end_pos, 8, hipMemcpyHostToDevice, sm) != hipSuccess) return fail(PHZ_E_HIP, "boundary repair");
                    repaired++;
                }
                prev_clean = (o.flags & 3) == 0;
            }
            if (!repaired) {
                bool any = false;
                for (auto &o : hso) if (o.flags & 3) any = true;
                if (!any) break;
            }
            if (knobs.timing) fprintf(stderr, "[phz timing]     bam device: %d guessed record boundaries were fakes, repaired from the preceding chain (pass %d)\n", repaired, pass);
            if (pass == 7) return fail(PHZ_E_UNSUPPORTED, "record boundaries did not converge");
            if (hipStreamSynchronize(sm) != hipSuccess) return fail(PHZ_E_HIP, "boundary repair");
        }
        hipLaunchKernelGGL(k_seg_kept, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, sm, (const SegOut *)dso, nseg, seg.kept(d_seg));
        if (int s2 = scan_excl(ctx, seg.kept(d_seg), seg.kbase(d_seg), nseg, ctx->scratch[SC_BAM_SCAN_TMP])) return fail(s2, nullptr);
        if (hipMemcpyAsync(&total_kept, seg.kbase(d_seg) + nseg, 4, hipMemcpyDeviceToHost, sm) != hipSuccess || hipStreamSynchronize(sm) != hipSuccess)
            return fail(PHZ_E_HIP, "segment read-back");
        return PHZ_OK;
    }
    // ---- 8. host checks: records sorted (inside segments and across them); 64-bit totals within the 32-bit scans
    int host_checks() {
        int32_t lr = -2, lp = 0;
        uint64_t sum = 0, sq = 0, qn = 0, ops = 0;
        for (const SegOut &o : hso) {
            if (o.flags & 4) return fail(PHZ_E_UNSUPPORTED, "BAM is not coordinate-sorted");
            if (o.first_ref != -2) {
                if (lr != -2 && (o.first_ref < lr || (o.first_ref == lr && o.first_pos < lp))) return fail(PHZ_E_UNSUPPORTED, "BAM is not coordinate-sorted");
                lr = o.last_ref; lp = o.last_pos;
            }
            sum += o.kept; sq += o.sq_sum; qn += o.qn_sum; ops += o.op_sum;
        }
        if (sum >= (1ull << 31) || sq >= knobs.limit || qn >= knobs.limit || ops >= knobs.limit)
            return fail(PHZ_E_UNSUPPORTED, "call exceeds the 32-bit offsets of the device path");
        lap("segments + counting hop");
        return PHZ_OK;
    }
    // ---- 9. kept-record list (the writing hop), the three prefix sums over it, the first record of every reference
    int kept_list() {
        const int64_t nk = h->n_kept = (int64_t)total_kept;
        const KeptCarve work(nk, n_ref);
        h->d_work = bam_take(&ctx->bam_work, work.bytes(), &h->d_work_cap, knobs.keep_buffers);          // (kept between BAMs like the two stream buffers: this ~1 GB hipMalloc took 0.38 s now and then)
        if (!h->d_work) return fail(PHZ_E_NOMEM, "device BAM record list");
        work.point(h);
        if (nk > 0) {
            hipLaunchKernelGGL(k_hop<1>, dim3(gseg), dim3(64), 0, sm, (const uint8_t *)h->d_stream, (const Seg *)seg.segs(d_seg), nseg, (const uint64_t *)seg.start(d_seg), F,
                               seg.so(d_seg), (const uint32_t *)seg.kbase(d_seg), h->K);
            if (int s2 = scan_excl(ctx, h->K.nops, h->co, nk, ctx->scratch[SC_BAM_SCAN_TMP])) return fail(s2, nullptr);
            if (int s2 = scan_excl(ctx, h->K.sq, h->so, nk, ctx->scratch[SC_BAM_SCAN_TMP])) return fail(s2, nullptr);
            if (int s2 = scan_excl(ctx, h->K.lqn, h->qo, nk, ctx->scratch[SC_BAM_SCAN_TMP])) return fail(s2, nullptr);
        } else {
            (void)hipMemsetAsync(h->co, 0, 4, sm); (void)hipMemsetAsync(h->so, 0, 4, sm); (void)hipMemsetAsync(h->qo, 0, 4, sm);
        }
        hipLaunchKernelGGL(k_ref_bounds, dim3((unsigned)((n_ref + 1 + 63) / 64)), dim3(64), 0, sm, (const int32_t *)h->K.ref, nk, n_ref, h->d_ref_begin);
        (void)hipEventRecord(e1, sm);
        return PHZ_OK;
    }
    // ---- 10. read-backs (reference bounds, then the three offsets at every bound: what phz_bamdev_sizes_of answers from) and the timing
    int read_backs() {
        if (hipMemcpyAsync(h->ref_begin.data(), h->d_ref_begin, (size_t)(n_ref + 1) * 8, hipMemcpyDeviceToHost, sm) != hipSuccess || hipStreamSynchronize(sm) != hipSuccess)
            return fail(PHZ_E_HIP, "reference bounds read-back");
        // totals must fit the 32-bit offsets of the scans: 64-bit sums of the per-segment kept counts are fine, the byte sums are
        // checked through the per-reference values (a wrapped scan makes a reference's span negative or absurd)
        for (int r = 0; r <= n_ref; r++) {
            const int64_t i = h->ref_begin[(size_t)r];
            (void)hipMemcpyAsync(&h->h_co[(size_t)r], h->co + i, 4, hipMemcpyDeviceToHost, sm);
            (void)hipMemcpyAsync(&h->h_so[(size_t)r], h->so + i, 4, hipMemcpyDeviceToHost, sm);
            (void)hipMemcpyAsync(&h->h_qo[(size_t)r], h->qo + i, 4, hipMemcpyDeviceToHost, sm);
        }
        if (hipStreamSynchronize(sm) != hipSuccess) return fail(PHZ_E_HIP, "offset read-back");
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        ctx->last_ms[PHZ_T_BAMPACK] = ms; ctx->total_ms[PHZ_T_BAMPACK] += ms; ctx->launches[PHZ_T_BAMPACK]++;
        drop_segments();
        lap("kept-record list + scans");
        if (knobs.timing)
            fprintf(stderr, "[phz timing]     bam device: H2D of %.1f MB overlapped with K_inflate (%.1f MB out): %.1f ms wall, first launch to last %.1f ms; boundaries + hop + scans %.1f ms, %lld records kept; "
                            "%d chunks, %d copy slices, %lld staging rounds\n",
                    L.comp_bytes / 1e6, L.out_bytes / 1e6, h2d_ms, inflate_ms, ms, (long long)h->n_kept, n_launch, n_slices, n_rounds);
        return PHZ_OK;
    }
};

}  // namespace

extern "C" {

int phz_bamdev_open(phz_ctx *ctx, const char *path, const char *const *ref_names, int n_names, const phz_bam_filters *f, phz_bamdev **out) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !path || !f || !out) return PHZ_E_ARG;
    *out = nullptr;
    BamOpen call(ctx, path, ref_names, n_names, f, out);
    return call.run();
}

int phz_bamdev_close(phz_bamdev *h) { delete h; return PHZ_OK; }
int phz_bamdev_n_ref(const phz_bamdev *h) { return (int)h->refs.size(); }
const char *phz_bamdev_ref_name(const phz_bamdev *h, int i) { return (i < 0 || (size_t)i >= h->refs.size()) ? nullptr : h->refs[(size_t)i].first.c_str(); }
int64_t phz_bamdev_ref_length(const phz_bamdev *h, int i) { return (i < 0 || (size_t)i >= h->refs.size()) ? -1 : (int64_t)h->refs[(size_t)i].second; }

int phz_bamdev_sizes_of(const phz_bamdev *h, int ref, phz_bamdev_sizes *out) {
    if (!h || !out || ref < 0 || (size_t)ref >= h->refs.size()) return PHZ_E_ARG;
    const size_t r = (size_t)ref;
    out->n_reads = h->ref_begin[r + 1] - h->ref_begin[r];
    out->n_ops = (int64_t)(uint32_t)(h->h_co[r + 1] - h->h_co[r]);
    out->n_seq_bytes = (int64_t)(uint32_t)(h->h_so[r + 1] - h->h_so[r]);
    out->n_qname_bytes = (int64_t)(uint32_t)(h->h_qo[r + 1] - h->h_qo[r]);
    return PHZ_OK;
}

// Fill the caller's (device) arrays of every reference: dst[r] is used for reference r when it holds records, ignored otherwise.
int phz_bamdev_pack(phz_bamdev *h, const phz_dev_shard *dst, int n_dst) {
    if (!h || !dst || n_dst != (int)h->refs.size()) return PHZ_E_ARG;
    phz_ctx *ctx = h->ctx;
    PhzEnter phz_guard_(ctx);
    if (h->n_kept == 0) return PHZ_OK;
    static_assert(sizeof(phz_dev_shard) == sizeof(DevShard), "shard pointer table layout");
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t sm = ctx->stream;
    if (int s = phz_reserve(ctx, ctx->shard_tab, (size_t)n_dst * sizeof(DevShard))) return s;
    PHZ_HIP(ctx, hipMemcpyAsync(ctx->shard_tab.p, dst, (size_t)n_dst * sizeof(DevShard), hipMemcpyHostToDevice, sm));
    PHZ_HIP(ctx, hipEventRecord(ctx->ev0, sm));
    hipLaunchKernelGGL(k_pack, dim3((unsigned)((h->n_kept + 255) / 256)), dim3(256), 0, sm, (const uint8_t *)h->d_stream, h->K, h->n_kept,
                       (const int64_t *)h->d_ref_begin, (const uint32_t *)h->co, (const uint32_t *)h->so, (const uint32_t *)h->qo,
                       (const DevShard *)ctx->shard_tab.p);
    PHZ_HIP(ctx, hipGetLastError());
    PHZ_HIP(ctx, hipEventRecord(ctx->ev1, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    float ms = 0;
    PHZ_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->last_ms[PHZ_T_BAMPACK] = ms; ctx->total_ms[PHZ_T_BAMPACK] += ms; ctx->launches[PHZ_T_BAMPACK]++;
    if (getenv("PHZ_TIMING")) fprintf(stderr, "[phz timing]     bam device: k_pack %.1f ms for %lld records\n", ms, (long long)h->n_kept);
    return PHZ_OK;
}

// QNAME ids of one shard on the device, continuing a numbering: the store holds the names of ids [0, n_old) in id order
// (store_off[n_old + 1]; NULL / 0 for an empty store).  qid[i] = the id of record i's name (an old id, or n_old + the number of new
// names that first appear before it does) -- exactly what phz_intern assigns.  first_idx[0, *n_new) = record of the first occurrence
// of every new name, in id order.
int phz_intern_device(phz_ctx *ctx, const char *qnames, const uint32_t *qname_off, int64_t n, const char *store, const uint32_t *store_off,
                      int64_t n_old, int32_t *qid, int32_t *first_idx, int64_t *n_new) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || !n_new || n < 0 || n_old < 0 || (n > 0 && (!qnames || !qname_off || !qid || !first_idx)) || (n_old > 0 && (!store || !store_off)))
        return PHZ_E_ARG;
    *n_new = 0;
    if (n == 0) return PHZ_OK;
    if (n + n_old >= (1ll << 31) - 16) return PHZ_E_UNSUPPORTED;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t sm = ctx->stream;
    uint64_t cap = 1024;
    while (cap < 2 * (uint64_t)(n + n_old)) cap <<= 1;
    DevBuf *S = ctx->scratch;
    if (int s = phz_reserve(ctx, S[SC_INTERN_TABLE], cap * 4)) return s;
    if (int s = phz_reserve(ctx, S[SC_INTERN_SLOT_OF], (size_t)n * 4)) return s;
    if (int s = phz_reserve(ctx, S[SC_INTERN_FIRST], (size_t)n * 4)) return s;
    if (int s = phz_reserve(ctx, S[SC_INTERN_RANK], ((size_t)n + 1) * 4)) return s;
    uint32_t *table = (uint32_t *)S[SC_INTERN_TABLE].p, *slot_of = (uint32_t *)S[SC_INTERN_SLOT_OF].p, *first = (uint32_t *)S[SC_INTERN_FIRST].p, *rank = (uint32_t *)S[SC_INTERN_RANK].p;
    PHZ_HIP(ctx, hipMemsetAsync(table, 0xff, cap * 4, sm));
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (n_old > 0) hipLaunchKernelGGL(k_intern_old, dim3((unsigned)((n_old + 255) / 256)), dim3(256), 0, sm, store, store_off, n_old, table, (uint32_t)(cap - 1));
    hipLaunchKernelGGL(k_intern_insert, dim3(grid), dim3(256), 0, sm, qnames, qname_off, n, store, store_off, table, (uint32_t)(cap - 1), slot_of);
    hipLaunchKernelGGL(k_intern_first, dim3(grid), dim3(256), 0, sm, (const uint32_t *)table, (const uint32_t *)slot_of, n, first);
    if (int s = scan_excl(ctx, first, rank, n, S[SC_BAM_SCAN_TMP])) return s;
    hipLaunchKernelGGL(k_intern_assign, dim3(grid), dim3(256), 0, sm, (const uint32_t *)table, (const uint32_t *)slot_of, (const uint32_t *)first,
                       (const uint32_t *)rank, n, (int32_t)n_old, qid, first_idx);
    PHZ_HIP(ctx, hipGetLastError());
    uint32_t total = 0;
    PHZ_HIP(ctx, hipMemcpyAsync(&total, rank + n, 4, hipMemcpyDeviceToHost, sm));
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    *n_new = (int64_t)total;
    return PHZ_OK;
}

// Appends the names of new ids to a store: step 1 (dst == NULL): dst_off[0 .. m] = exclusive prefix sums of their lengths starting at
// `base_bytes`, *total_bytes = the store's size afterwards; step 2 (dst = the store blob, at least *total_bytes long): copies the bytes.
int phz_names_append_device(phz_ctx *ctx, const char *qnames, const uint32_t *qname_off, const int32_t *first_idx, int64_t m, uint32_t base_bytes,
                            uint32_t *dst_off, char *dst, int64_t *total_bytes) {
    PhzEnter phz_guard_(ctx);
    if (!ctx || m < 0 || !total_bytes || (m > 0 && (!qnames || !qname_off || !first_idx || !dst_off))) return PHZ_E_ARG;
    PHZ_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t sm = ctx->stream;
    if (m == 0) { *total_bytes = base_bytes; return PHZ_OK; }
    const unsigned grid = (unsigned)((m + 255) / 256);
    if (!dst) {
        DevBuf *S = ctx->scratch;
        if (int s = phz_reserve(ctx, S[SC_NAMES_LEN], (size_t)m * 4)) return s;
        if (int s = phz_reserve(ctx, S[SC_NAMES_PRE], ((size_t)m + 1) * 4)) return s;
        uint32_t *len = (uint32_t *)S[SC_NAMES_LEN].p, *pre = (uint32_t *)S[SC_NAMES_PRE].p;
        hipLaunchKernelGGL(k_names_len, dim3(grid), dim3(256), 0, sm, qname_off, first_idx, m, len);
        if (int s = scan_excl(ctx, len, pre, m, S[SC_BAM_SCAN_TMP])) return s;
        uint32_t total = 0;
        PHZ_HIP(ctx, hipMemcpyAsync(&total, pre + m, 4, hipMemcpyDeviceToHost, sm));
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        if ((uint64_t)total + base_bytes >= (1ull << 32) - 16) return PHZ_E_UNSUPPORTED;
        // dst_off = pre + base_bytes (one more tiny pass keeps the scan generic)
        PHZ_HIP(ctx, hipMemcpyAsync(dst_off, pre, ((size_t)m + 1) * 4, hipMemcpyDeviceToDevice, sm));
        if (base_bytes) {
            hipLaunchKernelGGL(k_add_u32, dim3((unsigned)((m + 1 + 255) / 256)), dim3(256), 0, sm, dst_off, m + 1, base_bytes);
            PHZ_HIP(ctx, hipGetLastError());
        }
        PHZ_HIP(ctx, hipStreamSynchronize(sm));
        *total_bytes = (int64_t)total + base_bytes;
        return PHZ_OK;
    }
    hipLaunchKernelGGL(k_names_gather, dim3(grid), dim3(256), 0, sm, qnames, qname_off, first_idx, m, (const uint32_t *)dst_off, dst);
    PHZ_HIP(ctx, hipGetLastError());
    PHZ_HIP(ctx, hipStreamSynchronize(sm));
    return PHZ_OK;
}

}  // extern "C"
