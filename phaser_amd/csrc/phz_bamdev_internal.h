// The open handle of the device BAM path (phz_bamdev.hip), shared with the units that read the inflated stream and the kept-record list it keeps in HBM
// (phz_haplotag.hip).  Not part of the C ABI.
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "phz_internal.h"

// little-endian fields of a BAM record at any alignment
static __device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static __device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static __device__ __forceinline__ int32_t ldi32(const uint8_t *p) { return (int32_t)ld32(p); }

struct KeptOut {                // kept-record list (structure of arrays); off = offset of the record's refID field in the stream (its block_size sits 4 bytes in front)
    uint64_t *off; int32_t *ref; uint32_t *nops, *sq, *nb, *lqn;
};

struct phz_bamdev {
    phz_ctx *ctx = nullptr;
    bool keep_buffers = true;           // BamKnobs::keep_buffers of the call that opened the handle
    std::vector<std::pair<std::string, int32_t>> refs;
    void *d_stream = nullptr;           // inflated bytes of the needed members
    size_t d_stream_cap = 0;            // its size (the buffer goes back to the ctx's cache when the handle is closed)
    void *d_work = nullptr;             // kept-record list + offsets (one allocation)
    size_t d_work_cap = 0;
    KeptOut K{};
    int64_t n_kept = 0;
    uint32_t *co = nullptr, *so = nullptr, *qo = nullptr;      // exclusive prefix sums over the kept list ([n_kept + 1] each)
    int64_t *d_ref_begin = nullptr;
    std::vector<int64_t> ref_begin;     // host copy [n_ref + 1]
    std::vector<uint32_t> h_co, h_so, h_qo;     // values at the reference boundaries
    std::string err;
    ~phz_bamdev();                      // (phz_bamdev.hip: the two buffers go back to the ctx's cache)
};
