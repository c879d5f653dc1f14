// Output rows of phaser_annotate (phaser_annotate/phaser_annotate.py:405-456 build_interaction_result, :220-222) from K_annot's records, threaded.
// Everything a row says about one side -- variant id, rsid, allele, allele frequency, CADD phred and effect -- depends only on (entry, allele), so the
// caller prepares that text once per annotated (entry, allele) slot and a row is four copies: gene + name of side a, side a, side b, configuration.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "phz.h"

extern "C" int phz_annot_rows(const phz_annot_rec *rec, int64_t n_rows, int64_t n_entries, const int32_t *slot_of, int64_t n_slots, const char *head,
                              const int64_t *head_off, const char *side, const int64_t *side_off, int32_t threads, char **out, int64_t *out_len) {
    if (n_rows < 0 || n_entries < 0 || n_slots < 0 || !out || !out_len || (n_rows && (!rec || !slot_of || !head || !head_off || !side || !side_off)))
        return PHZ_E_ARG;
    *out = nullptr; *out_len = 0;
    static const char *const tail[8] = {"\tcis\t-1\n", "\ttrans\t-1\n", "\tcis\t0\n", "\ttrans\t0\n", "\tcis\t1\n", "\ttrans\t1\n", "\tcis\t2\n", "\ttrans\t2\n"};
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(threads, 64), n_rows / 4096 + 1));
    std::vector<int64_t> part((size_t)nt + 1, 0);
    std::vector<int> bad((size_t)nt, 0);
    auto slots = [&](const phz_annot_rec &r, int64_t *sa, int64_t *sb) {
        if (r.entry_a < 0 || r.entry_a >= n_entries || r.entry_b < 0 || r.entry_b >= n_entries) return false;
        *sa = slot_of[(int64_t)r.entry_a * 16 + (r.bits & 15u)]; *sb = slot_of[(int64_t)r.entry_b * 16 + ((r.bits >> 4) & 15u)];
        return *sa >= 0 && *sa < n_slots && *sb >= 0 && *sb < n_slots;
    };
    auto range = [&](int t, int64_t *lo, int64_t *hi) { *lo = n_rows * t / nt; *hi = n_rows * (t + 1) / nt; };
    auto measure = [&](int t) {
        int64_t lo, hi, bytes = 0; range(t, &lo, &hi);
        for (int64_t i = lo; i < hi; i++) {
            int64_t sa, sb;
            if (!slots(rec[i], &sa, &sb)) { bad[(size_t)t] = 1; return; }
            bytes += (head_off[sa + 1] - head_off[sa]) + 1 + (side_off[sa + 1] - side_off[sa]) + 1 + (side_off[sb + 1] - side_off[sb]) +
                     (int64_t)strlen(tail[(rec[i].bits >> 8 & 1u) | ((rec[i].bits >> 10 & 3u) << 1)]);
        }
        part[(size_t)t + 1] = bytes;
    };
    {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++) th.emplace_back(measure, t);
        for (auto &x : th) x.join();
    }
    for (int t = 0; t < nt; t++) { if (bad[(size_t)t]) return PHZ_E_ARG; part[(size_t)t + 1] += part[(size_t)t]; }
    const int64_t total = part[(size_t)nt];
    char *buf = (char *)malloc((size_t)total + 1);
    if (!buf) return PHZ_E_NOMEM;
    auto fill = [&](int t) {
        int64_t lo, hi; range(t, &lo, &hi);
        char *p = buf + part[(size_t)t];
        auto put = [&](const char *s, int64_t n) { memcpy(p, s, (size_t)n); p += n; };
        for (int64_t i = lo; i < hi; i++) {
            int64_t sa = 0, sb = 0;
            (void)slots(rec[i], &sa, &sb);
            put(head + head_off[sa], head_off[sa + 1] - head_off[sa]); *p++ = '\t';
            put(side + side_off[sa], side_off[sa + 1] - side_off[sa]); *p++ = '\t';
            put(side + side_off[sb], side_off[sb + 1] - side_off[sb]);
            const char *tl = tail[(rec[i].bits >> 8 & 1u) | ((rec[i].bits >> 10 & 3u) << 1)];
            put(tl, (int64_t)strlen(tl));
        }
    };
    {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++) th.emplace_back(fill, t);
        for (auto &x : th) x.join();
    }
    buf[total] = 0;
    *out = buf; *out_len = total;
    return PHZ_OK;
}
