// The narrow staging record of K_map (phz_map.hip): plain C++, compiled by hipcc for the device and by any host compiler for the unit test
// (tests/test_stage_pack.py).
//
// A call that nobody asks the text planes of is (record of the tile, variant of the shard, allele code).  While a tile has at most 256 records and every
// shard's het-SNP table at most 2^20 entries, that is ONE 32-bit word,
//   var[0:20) | rec[20:28) | code[28:32),
// stored once by k_map's flush and loaded once by k_compact: 4 bytes per call each way where the general record (stage_put: 8 bytes and two side planes)
// also carries the read offset of the base and the inserted-text flags, which only the text planes read.
// The host chooses the form per submission (stage_narrow_form): there is no per-call escape.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PHZ_SP_FN __host__ __device__ __forceinline__
#else
#define PHZ_SP_FN inline
#endif

constexpr int STAGE4_VAR_BITS = 20, STAGE4_REC_BITS = 8, STAGE4_CODE_BITS = 4;
constexpr int64_t STAGE4_MAX_NV = (int64_t)1 << STAGE4_VAR_BITS;          // variant indices 0 .. 2^20 - 1
constexpr int STAGE4_MAX_TILE_READS = 1 << STAGE4_REC_BITS;              // records 0 .. 255 of a tile

PHZ_SP_FN uint32_t stage4_pack(uint32_t var, uint32_t rec, uint32_t code) { return var | (rec << STAGE4_VAR_BITS) | (code << (STAGE4_VAR_BITS + STAGE4_REC_BITS)); }
PHZ_SP_FN uint32_t stage4_var(uint32_t w) { return w & ((1u << STAGE4_VAR_BITS) - 1u); }
PHZ_SP_FN uint32_t stage4_rec(uint32_t w) { return (w >> STAGE4_VAR_BITS) & ((1u << STAGE4_REC_BITS) - 1u); }
PHZ_SP_FN uint32_t stage4_code(uint32_t w) { return w >> (STAGE4_VAR_BITS + STAGE4_REC_BITS); }

// the host's choice for one submission: no shard wants the text planes, a tile's record number fits 8 bits, every live shard's variant index fits 20, and
// nobody forces the general form (PHZ_MAP_WIDE_STAGE=1)
PHZ_SP_FN bool stage_narrow_form(bool text_planes, int tile_reads, int64_t max_nv, bool force_wide) {
    return !force_wide && !text_planes && tile_reads <= STAGE4_MAX_TILE_READS && max_nv <= STAGE4_MAX_NV;
}
