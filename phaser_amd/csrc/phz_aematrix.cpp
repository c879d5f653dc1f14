// Host side of phaser_ae_test (include/phz.h): the parser of a gene x sample aCount|bCount matrix and the writer of the p-value / q-value matrices,
// both with host threads.  No device work here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "phz.h"

namespace {

struct Line { int64_t lo, hi; };          // [lo, hi) without the line end (\n, or \r\n, or trailing \r's)

// every non-empty line of the text
std::vector<Line> split_lines(const char *text, int64_t len) {
    std::vector<Line> lines;
    int64_t p = 0;
    while (p < len) {
        const char *nl = (const char *)memchr(text + p, '\n', (size_t)(len - p));
        const int64_t end = nl ? nl - text : len;
        int64_t hi = end;
        while (hi > p && text[hi - 1] == '\r') hi--;
        if (hi > p) lines.push_back({p, hi});
        p = end + 1;
    }
    return lines;
}

// <digits> in [s, e) -> value, or -1 (empty, another character, beyond int32)
int64_t parse_count(const char *s, const char *e) {
    if (s == e) return -1;
    int64_t v = 0;
    for (; s < e; s++) {
        if (*s < '0' || *s > '9') return -1;
        v = v * 10 + (*s - '0');
        if (v > INT32_MAX) return -1;
    }
    return v;
}

template <class F> void run_threads(int nt, F f) {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back(f, t);
    for (auto &x : th) x.join();
}

int thread_count(int32_t threads, int64_t n_rows) { return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int32_t>(threads, 64), n_rows / 256 + 1)); }

}  // namespace

extern "C" int phz_aematrix_parse(const char *text, int64_t len, int32_t threads, int64_t *n_rows, int64_t *n_cols, int64_t *header_len, int32_t *a, int32_t *b,
                                  int64_t *lead_off, int32_t *lead_len) {
    if (!text || len < 0 || !n_rows || !n_cols || !header_len) return PHZ_E_ARG;
    const std::vector<Line> lines = split_lines(text, len);
    if (lines.empty()) return PHZ_E_ARG;
    const Line head = lines[0];
    int64_t fields = 1;
    for (int64_t i = head.lo; i < head.hi; i++) fields += text[i] == '\t';
    const int64_t R = (int64_t)lines.size() - 1, C = std::max<int64_t>(0, fields - 4);
    *n_rows = R; *n_cols = C; *header_len = head.hi - head.lo;
    if (!a) return PHZ_OK;
    if (!b || !lead_off || !lead_len) return PHZ_E_ARG;
    const int nt = thread_count(threads, R);
    std::vector<int> bad((size_t)nt, 0);
    run_threads(nt, [&](int t) {
        for (int64_t r = R * t / nt; r < R * (t + 1) / nt; r++) {
            const Line ln = lines[(size_t)r + 1];
            const char *p = text + ln.lo, *end = text + ln.hi;
            // the four leading columns
            const char *q = p;
            int tabs = 0;
            while (q < end && !(*q == '\t' && ++tabs == 4)) q++;
            if (q - p > INT32_MAX) { bad[(size_t)t] = 1; return; }
            lead_off[r] = ln.lo; lead_len[r] = (int32_t)(q - p);
            int32_t *ra = a + r * C, *rb = b + r * C;
            for (int64_t c = 0; c < C; c++) {
                int32_t va = -1, vb = -1;
                if (q < end) {                       // q is the tab in front of cell c
                    const char *s = q + 1;
                    const char *e = (const char *)memchr(s, '\t', (size_t)(end - s));
                    if (!e) e = end;
                    const char *bar = (const char *)memchr(s, '|', (size_t)(e - s));
                    if (bar) {
                        const int64_t x = parse_count(s, bar), y = parse_count(bar + 1, e);
                        if (x >= 0 && y >= 0 && x + y <= INT32_MAX) { va = (int32_t)x; vb = (int32_t)y; }
                    }
                    q = e;
                }
                ra[c] = va; rb[c] = vb;
            }
        }
    });
    for (int x : bad) if (x) return PHZ_E_ARG;
    return PHZ_OK;
}

extern "C" int phz_aetest_rows(const char *text, const int64_t *lead_off, const int32_t *lead_len, int64_t n_rows, int64_t n_cols, const double *value, int32_t threads,
                               char **out, int64_t *out_len) {
    if (n_rows < 0 || n_cols < 0 || !out || !out_len || (n_rows && (!text || !lead_off || !lead_len || (n_cols && !value)))) return PHZ_E_ARG;
    *out = nullptr; *out_len = 0;
    const int nt = thread_count(threads, n_rows);
    std::vector<std::vector<char>> part((size_t)nt);
    run_threads(nt, [&](int t) {
        std::vector<char> &o = part[(size_t)t];
        const int64_t lo = n_rows * t / nt, hi = n_rows * (t + 1) / nt;
        o.reserve((size_t)((hi - lo) * (n_cols * 9 + 48)));
        char num[40];
        for (int64_t r = lo; r < hi; r++) {
            o.insert(o.end(), text + lead_off[r], text + lead_off[r] + lead_len[r]);
            const double *v = value + r * n_cols;
            for (int64_t c = 0; c < n_cols; c++) {
                o.push_back('\t');
                if (v[c] != v[c]) { o.push_back('N'); o.push_back('A'); continue; }
                const int k = snprintf(num, sizeof num, "%.6g", v[c]);
                o.insert(o.end(), num, num + k);
            }
            o.push_back('\n');
        }
    });
    int64_t total = 0;
    for (const auto &o : part) total += (int64_t)o.size();
    char *buf = (char *)malloc((size_t)total + 1);
    if (!buf) return PHZ_E_NOMEM;
    int64_t at = 0;
    for (const auto &o : part) { if (!o.empty()) memcpy(buf + at, o.data(), o.size()); at += (int64_t)o.size(); }
    buf[total] = 0;
    *out = buf; *out_len = total;
    return PHZ_OK;
}
