// Unit test of phaser_amd/csrc/phz_leanwalk.h on the CPU (driven by tests/test_lean_walk.py): the per-op step of K_map's lean walker, walked over a
// sorted window with std::lower_bound in place of the kernel's LDS search, against a direct restatement of walk_read<0>'s position rule.
//   * a record the lean walker keeps must yield walk_read<0>'s candidate list: (window index, read offset, inserted-text word, ordinal);
//   * a record it poisons must be one of the restated causes, and every restated cause must poison; only the verdict is compared then;
//   * LEAN_NEUTRAL appended 1..3 times changes neither the list nor the verdict.
// Prints one line per counter and "ok <records walked>" as the last line; any mismatch prints the record and exits 1.
#include "phz_leanwalk.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

enum : uint32_t { M = 0, I = 1, D = 2, N = 3, S = 4, H = 5, P = 6, EQ = 7, X = 8, G = 9 };
const char OPCH[] = "MIDNSHP=XG";

struct Cand {
    int var; uint32_t x0, x1; int ord;
    bool operator==(const Cand &o) const { return var == o.var && x0 == o.x0 && x1 == o.x1 && ord == o.ord; }
};
typedef std::vector<uint32_t> Cigar;
typedef std::vector<int> Window;

uint32_t word(uint32_t op, uint32_t len) { return (len << 4) | op; }

// ---- walk_read<0> of phz_map.hip, restated: one cursor over the window, segment-relative insertion keys looked up by a scan of the segment
std::vector<Cand> ref_walk(const Cigar &c, int pos, const Window &win) {
    std::vector<Cand> out;
    const size_t nv = win.size(), nc = c.size();
    size_t i = std::lower_bound(win.begin(), win.end(), pos) - win.begin();
    if (i >= nv) return out;
    int cnt = 0, gpos = 0, rpos = 0, seg_start = 0, plen = 0, seg_rpos = 0;
    size_t seg_op = 0;
    for (size_t k = 0; k < nc; k++) {
        const int len = (int)(c[k] >> 4); const uint32_t op = c[k] & 15;
        if (op == M || op == EQ || op == X || op == D) {
            const int lo = pos + seg_start + plen, hi = lo + len;
            while (i < nv && win[i] < lo) i++;
            while (i < nv && win[i] < hi) {
                const int vp = win[i];
                const int p = vp - pos - seg_start;
                const int rb = rpos + (p - plen);
                int ioff = 0, ilen = 0;
                if (nc > 1) {
                    int g2 = seg_start, r2 = seg_rpos;
                    for (size_t k2 = seg_op; k2 < nc; k2++) {
                        const int l2 = (int)(c[k2] >> 4); const uint32_t o2 = c[k2] & 15;
                        if (o2 == N) break;
                        if (o2 == M || o2 == EQ || o2 == X) { g2 += l2; r2 += l2; }
                        else if (o2 == D || o2 == G) g2 += l2;
                        else if (o2 == I) { if (g2 - 1 == p) { ioff = r2; ilen = l2; } r2 += l2; }
                        else if (o2 == S) r2 += l2;
                    }
                }
                const int nchars = (op != D) + ilen;
                if (nchars > 0) {
                    const uint32_t x0 = op != D ? (uint32_t)rb : 0xFFFFFFFFu;
                    const uint32_t x1 = ilen > 0 ? (((uint32_t)ioff << 12) | (uint32_t)(ilen > 4095 ? 4095 : ilen)) : 0u;
                    out.push_back(Cand{(int)i, x0, x1, cnt});
                    cnt++;
                }
                i++;
            }
            plen += len; gpos += len;
            if (op != D) rpos += len;
        } else if (op == I || op == S) {
            rpos += len;
        } else if (op == N) {
            gpos += len; seg_start = gpos; plen = 0; seg_op = k + 1; seg_rpos = rpos;
        } else if (op == G) {
            gpos += len;
        }
    }
    return out;
}

// ---- the causes for which the lean walker leaves a record to the general one, restated
enum : uint32_t { C_G = 1, C_THIRD = 2, C_AFTER_I = 4, C_AFTER_S = 8, C_AFTER_H = 16, C_AFTER_P = 32, C_AFTER_G = 64, C_AFTER_EMPTY = 128, C_COVER = 256, C_N = 9 };
const char *CAUSE_NAME[C_N] = {"G", "third_insertion", "ins_after_I", "ins_after_S", "ins_after_H", "ins_after_P", "ins_after_G", "ins_after_empty", "beyond_cover"};

uint32_t causes(const Cigar &c, int pos, long long cover) {
    uint32_t out = 0, prev = S, prev_len = 1; int nins = 0; long long g = 0;          // the first op counts as following a soft clip
    for (uint32_t w : c) {
        const uint32_t op = w & 15, len = w >> 4;
        if (op == I) {
            if (prev == I) out |= C_AFTER_I;
            if (prev == S) out |= C_AFTER_S;
            if (prev == H) out |= C_AFTER_H;
            if (prev == P) out |= C_AFTER_P;
            if (prev == G) out |= C_AFTER_G;
            if (prev_len == 0) out |= C_AFTER_EMPTY;
            if (nins == 2) out |= C_THIRD;
            nins++;
        }
        if (op == G) out |= C_G;
        if ((op == M || op == EQ || op == X || op == D) && pos + g + (long long)len > cover) out |= C_COVER;
        if (op == M || op == D || op == N || op == EQ || op == X || op == G) g += len;
        prev = op; prev_len = len;
    }
    return out;
}

// ---- the kernel's loop around lean_step, with std::lower_bound for the LDS search
bool lean_walk(const Cigar &c, int pos, const Window &win, long long cover, std::vector<Cand> &out) {
    out.clear();
    LeanWalk s; lean_init(s);
    const size_t n = c.size(), nv = win.size();
    for (size_t u = 0; u < n; u++) {
        const LeanOp o = lean_step(s, c[u], pos, cover);
        if (!o.search) continue;
        size_t i = std::lower_bound(win.begin(), win.end(), o.lo) - win.begin();
        while (i < nv && win[i] < o.hi) {
            const int vp = win[i];
            const uint32_t x1 = s.seg_start == 0 ? lean_ins_ahead(o, vp, u + 1 < n ? c[u + 1] : LEAN_NEUTRAL) : lean_ins_carried(s, vp, pos);
            const int nchars = (int)(o.mlike & 1u) + (int)(x1 & LEAN_INS_MAX);
            if (nchars > 0) {
                out.push_back(Cand{(int)i, o.mlike ? o.rbase + (uint32_t)(vp - o.lo) : 0xFFFFFFFFu, x1, s.cnt});
                s.cnt++;
            }
            i++;
        }
    }
    return s.bad == 0;
}

// het SNPs on the first and the last base of every aligned run, one before and one behind each of its boundaries
Window boundary_window(const Cigar &c, int pos) {
    Window w;
    long long g = 0;
    for (uint32_t x : c) {
        const uint32_t op = x & 15; const long long len = x >> 4;
        if ((op == M || op == EQ || op == X || op == D) && len > 0)
            for (long long p : {pos + g - 1, pos + g, pos + g + len - 1, pos + g + len})
                if (p >= 0 && p < 0x7fffffffll) w.push_back((int)p);
        if (op == M || op == D || op == N || op == EQ || op == X || op == G) g += len;
    }
    std::sort(w.begin(), w.end());
    w.erase(std::unique(w.begin(), w.end()), w.end());
    return w;
}

long long n_walked = 0, n_clean = 0, n_poisoned = 0, n_cands = 0, by_cause[C_N], clean_ins_first = 0, clean_ins_later = 0, n_neutral = 0;

void fail(const char *what, const Cigar &c, const Window &win) {
    printf("MISMATCH %s: ", what);
    for (uint32_t w : c) printf("%u%c ", w >> 4, OPCH[w & 15]);
    printf("| window:");
    for (int v : win) printf(" %d", v);
    printf("\n");
    exit(1);
}

void check(const Cigar &c, int pos, bool with_neutral) {
    const long long cover = (long long)pos + 65536;
    const uint32_t why = causes(c, pos, cover);
    const Window wins[2] = {boundary_window(c, pos), Window()};
    std::vector<Cand> got, got2;
    for (int wi = 0; wi < 2; wi++) {
        const Window &win = wins[wi];
        const bool kept = lean_walk(c, pos, win, cover, got);
        n_walked++;
        if (kept != (why == 0)) fail(kept ? "kept a record that one of the causes should poison" : "poisoned a record without a cause", c, win);
        if (kept) {
            if (!(got == ref_walk(c, pos, win))) fail("candidate list differs from walk_read<0>", c, win);
            n_cands += (long long)got.size();
        }
        if (wi == 0) {
            if (kept) {
                n_clean++;
                // inserted text on a candidate of the first segment / of a later one: the candidate's position lies before / behind the first N
                long long g = 0, first_n = -1;
                for (uint32_t x : c) { if ((x & 15) == N) { first_n = g; break; } if ((1u << (x & 15)) & LEAN_T_REF) g += x >> 4; }
                bool a = false, b = false;
                for (const Cand &k : got) if (k.x1) { if (first_n < 0 || win[k.var] - pos < first_n) a = true; else b = true; }
                clean_ins_first += a; clean_ins_later += b;
            } else {
                n_poisoned++;
                for (int k = 0; k < (int)C_N; k++) by_cause[k] += (why >> k) & 1;
            }
        }
        if (with_neutral) {
            Cigar c2 = c;
            for (int k = 1; k <= 3; k++) {
                c2.push_back(LEAN_NEUTRAL);
                const bool kept2 = lean_walk(c2, pos, win, cover, got2);
                n_neutral++;
                if (kept2 != kept || (kept && !(got2 == got))) fail("the neutral word changed the walk", c2, win);
            }
        }
    }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 33) % n);
}

const uint32_t LENS[4] = {0, 1, 2, 7};
const uint32_t N_LONG = 70000;          // an N that puts a later run past cover

}  // namespace

int main() {
    const int pos = 1000;
    // every word: ten ops x four lengths, and the long N
    std::vector<uint32_t> words;
    for (uint32_t op = 0; op < 10; op++) for (uint32_t l : LENS) words.push_back(word(op, l));
    words.push_back(word(N, N_LONG));
    const size_t W = words.size();
    // 1..3 ops: every sequence of words
    for (int n = 1; n <= 3; n++) {
        std::vector<size_t> ix(n, 0);
        for (;;) {
            Cigar c(n);
            for (int k = 0; k < n; k++) c[k] = words[ix[k]];
            check(c, pos, true);
            int k = n - 1;
            while (k >= 0 && ++ix[k] == W) ix[k--] = 0;
            if (k < 0) break;
        }
    }
    // 4..5 ops: every sequence of ops; six seeded draws of the lengths for each (all combinations would be 41^5 records)
    for (int n = 4; n <= 5; n++) {
        int total = 1; for (int k = 0; k < n; k++) total *= 10;
        for (int code = 0; code < total; code++) {
            for (int draw = 0; draw < 6; draw++) {
                Cigar c(n);
                int x = code;
                for (int k = 0; k < n; k++) {
                    const uint32_t op = (uint32_t)(x % 10); x /= 10;
                    const uint32_t pick = rnd(op == N ? 5 : 4);
                    c[k] = word(op, pick == 4 ? N_LONG : LENS[pick]);
                }
                check(c, pos, draw == 0);
            }
        }
    }
    // 6..12 ops, seeded, at most four insertions; M-heavy so that records survive to their later segments
    for (int t = 0; t < 200000; t++) {
        const int n = 6 + (int)rnd(7);
        Cigar c(n);
        int ins = 0;
        for (int k = 0; k < n; k++) {
            uint32_t op;
            const uint32_t r = rnd(100);
            if (r < 40) op = M; else if (r < 55) op = I; else if (r < 67) op = N; else if (r < 77) op = D; else if (r < 97) op = (uint32_t)(S + rnd(5)); else op = G;
            if (op == I && ++ins > 4) op = M;
            const uint32_t lr = rnd(20);
            const uint32_t len = lr == 0 ? 0 : (op == N && lr == 1 ? N_LONG : LENS[1 + rnd(3)]);
            c[k] = word(op, len);
        }
        check(c, pos, (t & 7) == 0);
    }
    for (int k = 0; k < (int)C_N; k++) printf("cause %s %lld\n", CAUSE_NAME[k], by_cause[k]);
    printf("clean %lld\npoisoned %lld\ncandidates %lld\nclean_ins_first %lld\nclean_ins_later %lld\nneutral %lld\n", n_clean, n_poisoned, n_cands, clean_ins_first,
           clean_ins_later, n_neutral);
    printf("ok %lld\n", n_walked);
    return 0;
}
