// Internal declarations shared by the HIP translation units of libphz.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "phz.h"

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

// Names of the per-call scratch slots ctx->scratch[...], grouped by the entry points that use them.  THE RULE: a slot holds nothing that must survive the
// return of the entry point that wrote it -- every entry point reserves and fills what it reads, which is why owners may (and do) share a number.  Whatever
// has to outlive a call has a ctx member of its own (tally_qcount, tally_table, tally_buf, ...).
enum PhzScratch {
    // AS histograms (phz_as_histogram / _batch / _sparse, phz_as_cutoff_enqueue): histogram + flags + occupied bins
    SC_AS_HIST = 0,
    // phz_tally (slots 1 and 7 are not used by it: 7 held the variant-pair table, now ctx->tally_table)
    SC_T_TOUCHED = 2, SC_T_CNT_T = 3, SC_T_BASE_T = 4, SC_T_ITEMS = 5, SC_T_COUNTERS = 6, SC_T_USEDKEY = 8, SC_T_DEG = 9, SC_T_EOFF = 10, SC_T_EB = 11, SC_T_ESLOT = 12,
    SC_T_SCAN_TMP = 13, SC_T_USED = 14, SC_T_MISC = 15, SC_T_EA = 19, SC_T_PROFILE = 20,
    // phz_components
    SC_UF_PARENT = 16,
    // K_map (phz_map_reads / _batch): per-tile totals, packed staging slots, first overflow slot per tile, PHZ_MAP_DBG cycle counts
    SC_MAP_TILE_TOTAL = 17, SC_MAP_STAGE = 18, SC_MAP_TILE_OVF = 19, SC_MAP_PROFILE = 21,
    // K_map_general (phz_map_reads_general)
    SC_GEN_N_CALLS = 0, SC_GEN_TILE_SUMS = 1, SC_GEN_CALL_BASE = 2, SC_GEN_TEXT_BASE = 3, SC_GEN_WINDOW = 4, SC_GEN_DESC = 5, SC_GEN_SCAN_TMP = 6, SC_GEN_WORKLIST = 7,
    SC_GEN_WORKLIST_N = 8, SC_GEN_SIDE = 9,
    // device BAM path (phz_bamdev.hip): scan temporary of the decode, QNAME interning (hash table, slot / first flag / rank per record), name lengths + offsets
    SC_BAM_SCAN_TMP = 6, SC_INTERN_TABLE = 7, SC_INTERN_SLOT_OF = 8, SC_INTERN_FIRST = 9, SC_INTERN_RANK = 10, SC_NAMES_LEN = 8, SC_NAMES_PRE = 9,
    // K_inflate: code lengths + cold table part per member
    SC_INFLATE_LENS = 11,
    // K_annot (phz_annot_pairs): rows per tile, their exclusive scan, the scan's temporary, the records of one batch
    SC_ANNOT_COUNT = 0, SC_ANNOT_BASE = 1, SC_ANNOT_SCAN_TMP = 2, SC_ANNOT_OUT = 3,
    // phz_variant_links: rows per edge of the range, their exclusive scan, the scan's temporary, edge range + verdict on the set
    SC_LINK_COUNT = 0, SC_LINK_BASE = 1, SC_LINK_SCAN_TMP = 2, SC_LINK_HEAD = 3,
    // phz_read_haplotypes: verdict on the block table, block + side per variant, the two key buffers of the sort (the free one then holds the run list) and its
    // value bytes, survivors per workgroup + scan, (runs, rows) per workgroup + scan, the sort's digit table, the scans' temporary
    SC_RH_FLAG = 0, SC_RH_VBLK = 1, SC_RH_VSIDE = 2, SC_RH_KEY0 = 3, SC_RH_KEY1 = 4, SC_RH_VAL0 = 5, SC_RH_VAL1 = 6, SC_RH_LIVE_COUNT = 7, SC_RH_LIVE_BASE = 8,
    SC_RH_RUN_COUNT = 9, SC_RH_RUN_BASE = 10, SC_RH_SORT_COUNT = 11, SC_RH_SCAN_TMP = 12,
    // K_bh (phz_bh_adjust): place of every cell among the tested ones, tested cells per column + their scan, the two (p bits, cell) buffers of the sort by p, the
    // two column-key buffers of the sort by column, the sorts' digit table, the scans' temporary
    SC_BH_POS = 0, SC_BH_COL_COUNT = 1, SC_BH_COL_OFF = 2, SC_BH_KEY0 = 3, SC_BH_KEY1 = 4, SC_BH_CELL0 = 5, SC_BH_CELL1 = 6, SC_BH_CKEY0 = 7, SC_BH_CKEY1 = 8,
    SC_BH_SORT_COUNT = 9, SC_BH_SCAN_TMP = 10,
    // K_bbfit (phz_betabinom_fit): candidate table, per-chunk sums of every (column, candidate), per-chunk tested cells of every column
    SC_BB_CAND = 0, SC_BB_PARTIAL = 1, SC_BB_USED = 2,
    // K_bbtest (phz_betabinom_test): per-column parameters, wave-tier flag of every cell, its exclusive scan, the listed cells, the scan's temporary
    SC_BB_COLPAR = 3, SC_BB_FLAG = 4, SC_BB_POS = 5, SC_BB_LIST = 6, SC_BB_SCAN_TMP = 7,
    // K_blntest (phz_bln_test): 1 / s per row, NaN where the row is not tested (K_blnfit keeps everything in registers)
    SC_BLN_ROWPAR = 0,
    // K_fisher (phz_fisher_test): wave-tier flag of every cell, its exclusive scan, the listed cells, the scan's temporary (K_cmh keeps everything in registers)
    SC_FISHER_FLAG = 0, SC_FISHER_POS = 1, SC_FISHER_LIST = 2, SC_FISHER_SCAN_TMP = 3,
    // K_match (phz_sample_match): the genotype codes packed 2 bits per donor (the sums stay in registers)
    SC_MATCH_WORDS = 0,
    // K_tagpick (phz_haplotag_pick): verdict on the rows, best (a + b, block) key per template
    SC_TAG_FLAG = 0, SC_TAG_BEST = 1,
    // K_tagsize / K_tagwrite (phz_bamdev_haplotag): verdict + tagged count, output bytes per kept record, their 64-bit exclusive scan, the scan's temporary
    SC_TAGW_HEAD = 0, SC_TAGW_LEN = 1, SC_TAGW_OFF = 2, SC_TAGW_SCAN_TMP = 3,
    SC_COUNT = 24
};

struct phz_ctx {
    // Every public entry point that works on a ctx holds this lock for the whole call (PhzEnter): two threads that share a ctx are
    // serialised, never interleaved inside its stream / scratch / error string.  Recursive because entry points call each other.
    std::recursive_mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;      // device -> host copies that run beside the kernels of `stream` (phz_rowsdev_run's copy-as-written), created on first use
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    // timing
    float last_ms[PHZ_T_COUNT] = {0};
    double total_ms[PHZ_T_COUNT] = {0};
    int64_t launches[PHZ_T_COUNT] = {0};
    int64_t counters[PHZ_C_COUNT] = {0};     // work counters accumulated by phz_tally (phz_get_counter)
    // scratch
    DevBuf scalars;
    DevBuf h_scalars;                  // pinned host mirror of `scalars` (hipHostMalloc); its users (phz_as_histogram_sparse, K_map) wait for the stream before they return: no copy is ever pending on it
    DevBuf h_bam_stage;                // page-locked staging of the device BAM path (phz_bamdev.hip)
    DevBuf bam_comp, bam_stream, bam_work;       // the device BAM path's big buffers (compressed members, inflated stream, kept-record list) kept between BAMs: a fresh hipMalloc of ~19 GB
                                       // took 1.1-1.5 s every few calls (profiles/r05/cli_4bam_full.txt); given back to the runtime when an allocation fails
                                       // and by phz_ctx_destroy; PHZ_BAM_KEEP_BUFFERS=0 turns the cache off
    DevBuf mail_dev, mail_host;        // PhzMail: gathered small read-backs (device block, page-locked host image)
    // shard table of a batched stage (device / pinned host image) and the last upload of the image: written and read by upload_tab (phz_tally.hip) ALONE, which waits for
    // tab_ev before it overwrites or reallocates the image (a stage that returns without a host wait -- phz_as_cutoff_enqueue -- leaves its copy queued)
    DevBuf shard_tab, h_shard_tab;
    hipEvent_t tab_ev = nullptr; bool tab_pending = false;
    // generic per-call scratch slots (PhzScratch), grown on demand and reused across calls
    DevBuf scratch[SC_COUNT];
    // device copies of PHZ_HOST callers' arrays (Staging): slot k of a call reuses stage_pool[k], grown on demand, so the
    // steady state allocates nothing
    std::vector<DevBuf> stage_pool;
    std::vector<DevBuf> tally_buf;     // result + read-list buffers of phz_tally
    std::vector<DevBuf> import_buf;    // arrays adopted by phz_tally_import
    std::vector<DevBuf> resident_vars; // phz_load_variants: slot s = {pos, ref_len} of one chromosome's het-variant table at [2 s], [2 s + 1]
    bool tally_dirty = false, tally_table_dirty = true;     // per-QNAME counters / variant-pair table not known to be clean
    // single-pass scan (phz_scan.h): ticket counter + one status word per tile, valid for the current epoch only (never cleared between scans)
    DevBuf scan_state; uint32_t scan_epoch = 0, scan_ticket_base = 0;
    uint64_t tally_gen = 0;            // bumped by every phz_tally / phz_tally_import: stamps what later stages prepared for "the resident tally"
    uint64_t tally_table_cap = 0;      // slots of the variant-pair table that the last phz_tally needed
    DevBuf boot_keys, boot_hist;       // K_boot: replicate medians per resident block, histograms of groups too large for LDS
    DevBuf tally_qcount;               // lines per QNAME: all zero between phz_tally calls (never shared with other stages)
    DevBuf tally_table;                // variant-pair hash table of phz_tally: all zero between calls (k_edge_out leaves it so), never shared with other stages
    // results of the last phz_tally, resident in HBM until the next one (phz_tally_fetch / phz_components read them)
    struct {
        int64_t nv = 0, n_lines = 0, n_kept = 0, n_edges = 0, n_rl = 0;
        int nb = 0;
        int32_t *var_count = nullptr, *var_distinct = nullptr, *ea = nullptr, *eb = nullptr, *cells = nullptr, *cto = nullptr, *stats = nullptr, *rl_qid = nullptr;
        int64_t *var_first = nullptr;
        uint64_t *var_rank = nullptr;
        uint32_t *rl_start = nullptr, *rl_list = nullptr;
        uint8_t *linked = nullptr, *line_cls = nullptr;
    } tally;
    // what K_map keeps between submissions (phz_map.hip alone reads and writes it; the layouts of tab and desc: MapTab, MapDesc there)
    struct {
        DevBuf tab;                    // device: shard table, per-shard call bases, overflow-area record
        DevBuf tab_host;               // pinned image of `tab`.  K_map waits for its stream before it returns, so no copy out of it is ever pending: no event
        std::vector<char> tab_image; void *tab_dev = nullptr;      // the table last uploaded to tab (a repeated submission skips the copy)
        long long ovf_image[5] = {0, 0, 0, 0, 0};      // the overflow-area record last uploaded (+ where): likewise
        hipEvent_t ev[2] = {nullptr, nullptr};         // around the k_map launch of an attempt
        DevBuf tile_w0, desc;          // per-tile window words; tile prefix + chunk sums of the two-level scan
        int tile_reads = 0;
        int slot_cap = 0;              // calls per tile slot of the staging area
        int64_t ovf_cap = 0;           // calls the overflow area behind the slots holds (grown to what the densest submission needed)
    } map;
};

// Small values a stage reads back before it can go on (counts, sizes, flags: a few words each, scattered over device buffers) travel as ONE block:
// a tiny kernel gathers them into ctx->mail_dev and one asynchronous copy brings the block to PAGE-LOCKED host memory.  (A hipMemcpyAsync to a pageable
// destination -- a stack variable, a std::vector -- is not asynchronous at all: the call waits for the stream and stages the bytes, 20-30 us each; a stage
// that read ten values back paid that ten times over, measured as 150-250 us of idle GPU per host wait in the phasing pass.)
struct PhzMail {
    static constexpr int MAX = 16;
    phz_ctx *ctx;
    const void *src[MAX]; uint32_t bytes[MAX], off[MAX];
    int n = 0; uint32_t total = 0; bool overflow = false;
    explicit PhzMail(phz_ctx *c) : ctx(c) {}
    int add(const void *dev, size_t nbytes) {          // -> slot; the value is at<T>(slot) after send() + a host wait on the ctx stream
        if (n >= MAX) { overflow = true; return -1; }          // (send() then fails: nobody reads at<T>(-1))
        src[n] = dev; bytes[n] = (uint32_t)nbytes; off[n] = total;
        total += ((uint32_t)nbytes + 7u) & ~7u;
        return n++;
    }
    int send();
    template <class T> const T *at(int slot) const { return (const T *)((const char *)ctx->mail_host.p + off[slot]); }
};

struct PhzEnter {
    std::unique_lock<std::recursive_mutex> lk;
    explicit PhzEnter(phz_ctx *ctx) { if (ctx) lk = std::unique_lock<std::recursive_mutex>(ctx->mu); }
};

int phz_fail(phz_ctx *ctx, int status, const char *what, hipError_t e = hipSuccess);
int phz_reserve(phz_ctx *ctx, DevBuf &b, size_t bytes);
int phz_reserve_host(phz_ctx *ctx, DevBuf &b, size_t bytes);      // pinned host memory
// reserve a list of (buffer, bytes); the first failure ends it
struct Rsv { DevBuf &b; size_t bytes; };
inline int reserve_all(phz_ctx *ctx, std::initializer_list<Rsv> list) {
    for (const Rsv &r : list) if (int s = phz_reserve(ctx, r.b, r.bytes)) return s;
    return PHZ_OK;
}
inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }          // workgroups of 256 threads over n items

#define PHZ_HIP(ctx, call)                                                      \
    do {                                                                        \
        hipError_t _e = (call);                                                 \
        if (_e != hipSuccess) return phz_fail((ctx), PHZ_E_HIP, #call, _e);     \
    } while (0)

// launchers implemented in the kernel translation units (device pointers only)
int phz_launch_map(phz_ctx *ctx, const phz_reads &r, const phz_variants &v, int baseq, const phz_calls &out,
                   int64_t *n_calls);
int phz_launch_map_batch(phz_ctx *ctx, int n, const phz_reads *r, const phz_variants *v, int baseq, const phz_calls *out,
                         int64_t *n_calls);

// Scoped staging of host arrays for PHZ_HOST callers: the k-th array of a call lives in ctx->stage_pool[k] (kept across
// calls, grown on demand -- no allocation in the steady state).
struct Staging {
    phz_ctx *ctx;
    size_t next = 0;
    explicit Staging(phz_ctx *c) : ctx(c) {}
    int slot(size_t bytes, void **d) {
        if (next >= ctx->stage_pool.size()) ctx->stage_pool.resize(next + 1);
        DevBuf &b = ctx->stage_pool[next++];
        if (int s = phz_reserve(ctx, b, bytes ? bytes : 1)) return s;
        *d = b.p;
        return PHZ_OK;
    }
    // returns a device pointer holding `count` items copied from host pointer src (or src itself in device space)
    template <class T> int in(const T *src, size_t count, int space, const T **dst) {
        if (space == PHZ_DEVICE || src == nullptr) { *dst = src; return PHZ_OK; }
        void *d = nullptr;
        const size_t bytes = count * sizeof(T);
        if (int s = slot(bytes, &d)) return s;
        if (bytes) { hipError_t e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream); if (e != hipSuccess) return phz_fail(ctx, PHZ_E_HIP, "H2D", e); }
        *dst = (const T *)d;
        return PHZ_OK;
    }
    // device buffer for an output of `count` elements; host pointer remembered by the caller for the copy back
    template <class T> int out(T *host, size_t count, int space, T **dev) {
        if (space == PHZ_DEVICE) { *dev = host; return PHZ_OK; }
        void *d = nullptr;
        if (int s = slot(count * sizeof(T), &d)) return s;
        *dev = (T *)d;
        return PHZ_OK;
    }
};

// ---- plan of a (chromosome-restricted) BAM read, shared by the host decode and the device decode (phz_bam.cpp)
struct PhzBamPlan {
    std::vector<std::pair<std::string, int32_t>> refs;
    std::vector<uint8_t> head;                             // inflated bytes from the file start; the header ends at first_record
    size_t first_record = 0;
    std::vector<std::pair<uint64_t, uint64_t>> pieces;     // [u0, u1) of the inflated stream (global offsets), cut at record boundaries
    struct Mem { uint64_t src; uint32_t csize, isize; uint64_t dst; uint32_t crc; };          // crc: the CRC32 field of the member's trailer
    std::vector<Mem> members;                              // members that overlap a piece, file order; dst = global inflated offset
    const uint8_t *file = nullptr; size_t file_size = 0;   // the mapped file: NULL until phz_bam_plan_map (valid until phz_bam_plan_release)
    void *owner = nullptr;
};
int phz_bam_plan_file(const char *path, const char *const *ref_names, int n_names, PhzBamPlan *out);
const uint8_t *phz_bam_plan_map(PhzBamPlan *p);          // maps the file on first use (the plan itself reads it with pread)
void phz_bam_plan_release(PhzBamPlan *p);

// K_inflate launcher for callers that pipeline it with their own copies (phz_inflate.hip)
int phz_inflate_launch(phz_ctx *ctx, const uint8_t *comp, const phz_bgzf_member *members, int64_t first, int64_t count, uint8_t *out,
                       uint8_t *lens_scratch, int *d_status, hipStream_t s);
int phz_inflate_scratch_bytes_per_member();
// CRC-32 check of the same members' output against the trailers' values (want: device array, one per member of the table), status code 7 into d_status
int phz_crc_launch(phz_ctx *ctx, const phz_bgzf_member *members, int64_t first, int64_t count, const uint8_t *out, const uint32_t *want, int *d_status, hipStream_t s);

