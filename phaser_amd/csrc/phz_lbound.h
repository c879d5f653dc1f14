// Lower bound over a tile's staged het-SNP window (K_map, phz_map.hip): plain C++, compiled by hipcc for the device and by any host compiler for
// the unit test (tests/test_window_search.py).
//
// window_lower_bound<D>(w, key) = number of entries of w below key, for a sorted window of at most 2^D entries that is PADDED WITH INT_MAX UP TO
// 2^D ENTRIES: D halving steps from 2^(D-1) down to 1 and one closing probe, fully unrolled, no bounds test (probes reach index 2^D - 1 at most).
//
// A step is written so that gfx950 needs five issue slots for it (LDS read with an immediate offset, its wait, subtract, shift, and-or) and nothing
// on the scalar unit:
//   * the cursor is a BYTE offset: the probe address is base + cursor + constant, the constant goes into the instruction's offset field, and no
//     index-to-bytes shift is left per probe;
//   * the step is taken through the sign bit of an UNSIGNED difference, cursor += ((uint32_t)v - (uint32_t)key) >> 31 times the step, instead of
//     compare + select: a vector compare writes VCC, the select that reads it must wait out a hazard (an s_nop per probe), and the signed form
//     (uint32_t)(v - key) >> 31 is folded back into exactly that pair by the compiler.
// The sign bit equals v < key only while the difference cannot wrap: 0 <= key and 0 <= w[i] <= INT_MAX.  Positions are never negative;
// window_clamp_key() maps the negative keys the callers can produce (the "no record" sentinel INT_MIN, a wrapped position sum) to 0, whose lower
// bound is what the compare form gave for them: 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PHZ_LB_FN __device__ __forceinline__
#else
#define PHZ_LB_FN inline
#endif

PHZ_LB_FN int window_clamp_key(int key) { return key > 0 ? key : 0; }

// cursor (bytes) after the probe of entry cursor / 4 + S - 1 with step S entries
template <int S>
PHZ_LB_FN uint32_t window_lb_step(const int32_t *w, uint32_t key, uint32_t cur) {
    const uint32_t v = (uint32_t) * reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(w) + cur + 4u * (uint32_t)(S - 1));
    return cur + ((v - key) >> 31) * (4u * (uint32_t)S);
}

template <int S>
struct WindowLbChain {
    static PHZ_LB_FN uint32_t run(const int32_t *w, uint32_t key, uint32_t cur) { return WindowLbChain<S / 2>::run(w, key, window_lb_step<S>(w, key, cur)); }
};
template <>
struct WindowLbChain<0> {
    static PHZ_LB_FN uint32_t run(const int32_t *, uint32_t, uint32_t cur) { return cur; }
};

// key >= 0 (window_clamp_key); w sorted, 0 <= w[i], padded with INT_MAX up to 2^D entries
template <int D>
PHZ_LB_FN int window_lower_bound(const int32_t *w, int key) {
    static_assert(D >= 0 && D <= 10, "window_lower_bound: 2^D entries, D up to 10");
    const uint32_t k = (uint32_t)window_clamp_key(key);
    uint32_t cur = WindowLbChain<((1 << D) >> 1)>::run(w, k, 0u);      // steps 2^(D-1) .. 1
    cur = window_lb_step<1>(w, k, cur);                                 // closing probe
    return (int)(cur >> 2);
}
