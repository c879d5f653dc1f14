// TEST INFRASTRUCTURE ONLY (tests/test_window_search.py): window_lower_bound<D> of phaser_amd/csrc/phz_lbound.h -- the search K_map runs over a
// tile's staged het-SNP window -- compiled for the host and compared with std::lower_bound: every depth D, every window length 0 .. 2^D (padded
// with INT_MAX up to 2^D entries, as the kernel pads its LDS window), several window shapes, and every key the kernel's callers can produce.
#include "phz_lbound.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <vector>

static long long n_checked = 0;

template <int D>
static bool check_key(const std::vector<int32_t> &w, int n, int key, int shape) {
    const int want = key < 0 ? 0 : (int)(std::lower_bound(w.begin(), w.begin() + n, key) - w.begin());
    const int got = window_lower_bound<D>(w.data(), key);
    n_checked++;
    if (got == want) return true;
    std::printf("MISMATCH D=%d shape=%d wlen=%d key=%d: got %d, std::lower_bound %d\n", D, shape, n, key, got, want);
    return false;
}

// shapes: 0 = starts at entry 0, gaps of 2 and 4 (strictly increasing); 1 = one run of consecutive positions from 1; 2 = near 2,000,000,000;
//         3 = pairs of equal positions (a multi-allelic site listed twice); 4 = the largest positions an int holds below the padding value
static int32_t entry(int shape, int i, int n) {
    switch (shape) {
    case 0: return 3 * i - (i % 2);          // 0, 2, 6, 8, 12, ...
    case 1: return 1 + i;
    case 2: return 2000000000 + 3 * i;
    case 3: return 100 + 5 * (i / 2);
    default: return INT_MAX - 1 - (n - 1 - i);
    }
}

template <int D>
static bool check_depth() {
    constexpr int CAP = 1 << D;
    for (int shape = 0; shape < 5; shape++) {
        for (int n = 0; n <= CAP; n++) {
            std::vector<int32_t> w((size_t)CAP, INT_MAX);          // the padding: INT_MAX up to 2^D entries
            for (int i = 0; i < n; i++) w[(size_t)i] = entry(shape, i, n);
            if (!std::is_sorted(w.begin(), w.begin() + n) || (n > 0 && w[0] < 0)) { std::printf("bad test window: shape %d wlen %d\n", shape, n); return false; }
            const int fixed[] = {0, INT_MAX, -1, INT_MIN, (int)0x80000000 /* the bracket's "no single-run record in this wave" */, 1, INT_MAX - 1, -2000000000};
            for (int key : fixed) if (!check_key<D>(w, n, key, shape)) return false;
            for (int i = 0; i < n; i++) {
                const int e = w[(size_t)i];
                if (!check_key<D>(w, n, e, shape)) return false;
                if (!check_key<D>(w, n, e - 1, shape)) return false;          // -1 under an entry 0: a negative key
                if (e < INT_MAX && !check_key<D>(w, n, e + 1, shape)) return false;
            }
        }
    }
    return true;
}

int main() {
    const bool ok = check_depth<0>() && check_depth<1>() && check_depth<2>() && check_depth<3>() && check_depth<4>() && check_depth<5>() && check_depth<6>() &&
                    check_depth<7>() && check_depth<8>() && check_depth<9>();
    if (!ok) return 1;
    std::printf("ok %lld\n", n_checked);
    return 0;
}
