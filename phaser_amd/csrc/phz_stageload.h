// The staging loads of a K_map tile (phz_map.hip) through bounds-checked buffer loads: the descriptor lengths are plain C++, compiled by hipcc for the
// device and by any host compiler for the unit test (tests/test_stage_load.py); the descriptor and the load are device code.
//
// A tile stages five slices -- pos, seq_off and cigar_off of its records, its het-SNP window, its packed CIGAR words.  Each gets ONE descriptor per tile,
// built from wave-uniform values only: base = the slice's first word, num_records = the slice's bytes.  The hardware then answers 0 for a lane whose word
// lies past the slice, so the load needs neither an exec-mask guard (`j < nr`, `j < cnt_w`, `tid < wlen`, `idx < nv`) nor a 64-bit address per lane: the
// lane's part is a 32-bit byte offset.  Per-tile bases keep every offset small (a tile's slices are a few KB) whatever the shard's size.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PHZ_SL_FN __host__ __device__ __forceinline__
#else
#define PHZ_SL_FN inline
#endif

// records of the tile that starts at record r0 < n of a shard of n records: min(n - r0, tile)
PHZ_SL_FN int stage_tile_records(int64_t n, int64_t r0, int tile) { const int64_t rest = n - r0; return rest < tile ? (int)rest : tile; }
// words of the cigar_off slice: one per record and the offset that ends the last one (lanes past the tile read index nr: stage_coff_index)
PHZ_SL_FN uint32_t stage_coff_words(int nr) { return (uint32_t)nr + 1u; }
PHZ_SL_FN uint32_t stage_coff_index(int j, int nr) { return (uint32_t)(j < nr ? j : nr); }
// het-SNP window of staged length wlen that starts at table entry w0 of nv: the entries that exist, clamp(min(wlen, nv - w0), 0, wlen); everything
// beyond them is INT_MAX padding (window_lower_bound probes it without a bounds test)
PHZ_SL_FN uint32_t stage_window_words(int wlen, int nv, int w0) {
    const int64_t rest = (int64_t)nv - (int64_t)w0;
    const int64_t m = rest < (int64_t)wlen ? rest : (int64_t)wlen;
    return m > 0 ? (uint32_t)m : 0u;
}
// packed CIGAR words of the tile that LDS holds: min(words of the tile, cap)
PHZ_SL_FN uint32_t stage_cigar_words(uint32_t words, uint32_t cap) { return words < cap ? words : cap; }

#if defined(__HIPCC__)
// descriptor over `words` 32-bit words at `base` (both wave-uniform); raw buffer, no stride: an offset with offset + 4 > 4 * words loads 0
#define PHZ_STAGE_RSRC(base, words) __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(static_cast<const void *>(base)), (short)0, (int)((uint32_t)(words) * 4u), 0x00020000)
// word `index` of the slice (0 past its end)
#define PHZ_STAGE_WORD(rsrc, index) ((uint32_t)__builtin_amdgcn_raw_buffer_load_b32((rsrc), (int)((uint32_t)(index) * 4u), 0, 0))
#endif
