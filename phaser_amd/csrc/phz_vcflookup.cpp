// VCF lookup of phaser_cis_var (phaser_pop/phaser_cis_var.py:276-284, vcf_reader.retrieve_variant): every record of a bgzipped VCF at the given
// (CHROM, 1-based POS) keys -- what pysam's fetch(chr, pos-1, pos) plus the `POS == pos` filter return -- reduced to the fields the tool reads:
// CHROM, POS, ID, REF, ALT, the index of GT in FORMAT and the GT subfield of each mapped sample.
//
// With <path>.tbi: the index gives, per key, the chunks of its UCSC bins that end past the linear-index bound of the key's 16 kb window; the chunks
// of all keys are merged into disjoint spans of virtual offsets, each span's BGZF members are read and inflated on a worker thread, and only the
// span's lines are scanned.  Without an index: the whole file is inflated (phz_bgzf_read) and scanned.  Both paths report the same lines in file order.
//
// phz_tabix_lines (phaser_annotate's CADD table and allele-frequency VCF) is the same lookup with another reduction of a matching line: a caller-chosen
// list of columns instead of the VCF fields, and no header line to find.
//
// phz_vcf_region_classes (phaser_cis_scan) asks by region instead of by position: the regions of a contig are merged into disjoint intervals, the index path
// collects the chunks of every interval's bins, and a matching line is reduced to its five leading fields, the GT index and one class character per sample
// (class_code: cis_var's _classify).  A record inside several of the caller's regions is reported once, since the lines are scanned once, in file order.
//
// phz_vcf_site_genotypes (phaser_sample_match) is phz_vcf_lookup with the GT texts reduced to one genotype code per sample (geno_code).
#include <fcntl.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "phz.h"

namespace {

struct Key {
    std::string chrom; int64_t pos;
    bool operator==(const Key &o) const { return pos == o.pos && chrom == o.chrom; }
};
struct KeyHash { size_t operator()(const Key &k) const { return std::hash<std::string>()(k.chrom) * 1000003u ^ std::hash<int64_t>()(k.pos); } };

struct Ctx {
    std::unordered_map<Key, int64_t, KeyHash> keys;
    std::vector<int32_t> scol;             // VCF column of each mapped sample, -1 = absent from the header
    const int32_t *cols = nullptr;         // phz_tabix_lines: the columns to report (-1 = the last one) instead of the VCF fields
    int32_t n_cols = 0;
    // phz_vcf_region_classes: records inside a region instead of records at a key; per contig the merged [lo, hi] intervals (1-based, inclusive), ascending
    const int64_t *hi = nullptr;
    std::unordered_map<std::string, std::vector<std::pair<int64_t, int64_t>>> regions;
    bool geno = false;                     // phz_vcf_site_genotypes: records at a key, one genotype code per sample instead of the GT texts
};

// phaser_amd.cis_var's _classify and its phased test on one GT text -> '0' + class (+ 4: the "1" of a het is the second field)
char class_code(std::string_view gt) {
    if (gt.find('|') == std::string_view::npos) return '0';
    const size_t zeros = (size_t)std::count(gt.begin(), gt.end(), '0'), ones = (size_t)std::count(gt.begin(), gt.end(), '1');
    if (zeros && ones) {
        int idx = 0;
        for (size_t a = 0;; idx++) {
            const size_t b = gt.find('|', a);
            if (gt.substr(a, b == std::string_view::npos ? std::string_view::npos : b - a) == "1") return idx == 0 ? '1' : (idx == 1 ? '5' : '0');
            if (b == std::string_view::npos) return '0';              // e.g. 0|10
            a = b + 1;
        }
    }
    return (zeros == 2 || ones == 2) ? '2' : '0';
}

// phaser_amd.sample_match's genotype of one GT text -> '0' + code: two alleles split by '/' or '|'; "0" and "0": 1, one "0" and one "1": 2, "1" and "1": 3;
// everything else (".", "./.", one allele, three, an allele of 2 or more): 0
char geno_code(std::string_view gt) {
    const size_t sep = gt.find_first_of("/|");
    if (sep == std::string_view::npos) return '0';
    const std::string_view x = gt.substr(0, sep), y = gt.substr(sep + 1);
    if ((x != "0" && x != "1") || (y != "0" && y != "1")) return '0';
    return (char)('1' + (x == "1") + (y == "1"));
}

// the GT subfield (index gi of FORMAT) of sample column text v; false: the column has fewer subfields
bool gt_subfield(std::string_view v, int gi, std::string_view *gt) {
    size_t a = 0; int idx = 0;
    while (idx < gi && a != std::string_view::npos) { a = v.find(':', a); if (a != std::string_view::npos) a++; idx++; }
    if (a == std::string_view::npos) return false;
    const size_t b = v.find(':', a);
    *gt = v.substr(a, b == std::string_view::npos ? std::string_view::npos : b - a);
    return true;
}

// one record line -> output line "key\tCHROM\tPOS\tID\tREF\tALT\tgi\tGT...\n" (GT of a column the line lacks: "\x01")
void emit(const Ctx &C, int64_t key, std::string_view line, std::string &out) {
    std::vector<std::string_view> f;
    size_t i = 0;
    while (true) {
        size_t j = line.find('\t', i);
        if (j == std::string_view::npos) { f.push_back(line.substr(i)); break; }
        f.push_back(line.substr(i, j - i)); i = j + 1;
    }
    if (!C.hi) out += std::to_string(key);
    if (C.cols) {
        for (int32_t k = 0; k < C.n_cols; k++) {
            const int64_t c = C.cols[k] < 0 ? (int64_t)f.size() - 1 : C.cols[k];
            out += '\t';
            if (c >= 0 && (size_t)c < f.size()) out.append(f[(size_t)c]);
        }
        out += '\n';
        return;
    }
    for (int k = 0; k < 5; k++) { if (k || !C.hi) out += '\t'; if ((size_t)k < f.size()) out.append(f[(size_t)k]); }
    int gi = -1;
    if (f.size() > 8) {
        std::string_view fmt = f[8];
        int idx = 0; size_t a = 0;
        while (true) {
            size_t b = fmt.find(':', a);
            std::string_view sub = fmt.substr(a, b == std::string_view::npos ? std::string_view::npos : b - a);
            if (sub == "GT") { gi = idx; break; }
            if (b == std::string_view::npos) break;
            a = b + 1; idx++;
        }
    }
    out += '\t'; out += std::to_string(gi);
    if (C.hi || C.geno) out += '\t';
    for (int32_t c : C.scol) {
        if (C.geno) {                                                // one genotype character per sample
            std::string_view gt;
            out += gi >= 0 && c >= 0 && (size_t)c < f.size() && gt_subfield(f[(size_t)c], gi, &gt) ? geno_code(gt) : '0';
            continue;
        }
        if (C.hi) {                                                  // one class character per sample
            char code = '0';
            if (gi >= 0 && c >= 0 && (size_t)c < f.size()) {
                std::string_view v = f[(size_t)c];
                size_t a = 0; int idx = 0;
                while (idx < gi && a != std::string_view::npos) { a = v.find(':', a); if (a != std::string_view::npos) a++; idx++; }
                if (a != std::string_view::npos) {
                    const size_t b = v.find(':', a);
                    code = class_code(v.substr(a, b == std::string_view::npos ? std::string_view::npos : b - a));
                }
            }
            out += code;
            continue;
        }
        out += '\t';
        if (c < 0 || (size_t)c >= f.size()) { out += '\x01'; continue; }
        if (gi < 0) continue;
        std::string_view v = f[(size_t)c];
        size_t a = 0; int idx = 0;
        while (idx < gi && a != std::string_view::npos) { a = v.find(':', a); if (a != std::string_view::npos) a++; idx++; }
        if (a == std::string_view::npos) continue;                  // fewer subfields than FORMAT: an empty GT
        size_t b = v.find(':', a);
        out.append(v.substr(a, b == std::string_view::npos ? std::string_view::npos : b - a));
    }
    out += '\n';
}

// scan lines [p, e) of inflated text; a line whose (CHROM, POS) is a key is emitted
void scan(const Ctx &C, const char *p, const char *e, std::string &out, std::vector<std::string> *contigs) {
    std::string last_contig;
    std::string chrom_s, pos_s;
    while (p < e) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
        const char *le = nl ? nl : e;
        std::string_view line(p, (size_t)(le - p));
        if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
        if (!line.empty() && line[0] != '#') {
            size_t t1 = line.find('\t');
            if (t1 != std::string_view::npos) {
                size_t t2 = line.find('\t', t1 + 1);
                std::string_view chrom = line.substr(0, t1), ps = line.substr(t1 + 1, (t2 == std::string_view::npos ? line.size() : t2) - t1 - 1);
                if (contigs && chrom != last_contig) {
                    last_contig.assign(chrom);
                    if (std::find(contigs->begin(), contigs->end(), last_contig) == contigs->end()) contigs->push_back(last_contig);
                }
                pos_s.assign(ps);
                char *endp = nullptr;
                const long long pos = strtoll(pos_s.c_str(), &endp, 10);
                if (!pos_s.empty() && endp && *endp == 0) {
                    chrom_s.assign(chrom);
                    if (C.hi) {
                        auto rg = C.regions.find(chrom_s);
                        if (rg != C.regions.end()) {
                            const auto &iv = rg->second;              // the last interval that starts at or before pos
                            auto u = std::upper_bound(iv.begin(), iv.end(), std::make_pair((int64_t)pos, INT64_MAX));
                            if (u != iv.begin() && (u - 1)->second >= pos) emit(C, 0, line, out);
                        }
                    } else {
                        auto it = C.keys.find(Key{chrom_s, pos});
                        if (it != C.keys.end()) emit(C, it->second, line, out);
                    }
                }
            }
        }
        p = le + 1;
    }
}

// the BGZF member at file offset `off` into m: its size and inflated size (false at EOF / a malformed header)
bool member_at(int fd, uint64_t off, uint32_t *bsize, uint32_t *isize, std::vector<uint8_t> &m) {
    uint8_t h[18];
    if (pread(fd, h, 18, (off_t)off) != 18 || h[0] != 31 || h[1] != 139) return false;
    const uint16_t xlen = (uint16_t)(h[10] | (h[11] << 8));
    std::vector<uint8_t> x(xlen);
    if (pread(fd, x.data(), xlen, (off_t)(off + 12)) != (ssize_t)xlen) return false;
    uint32_t bs = 0;
    for (size_t k = 0; k + 4 <= xlen;) {
        const uint16_t slen = (uint16_t)(x[k + 2] | (x[k + 3] << 8));
        if (x[k] == 66 && x[k + 1] == 67 && slen == 2 && k + 6 <= xlen) bs = (uint32_t)(x[k + 4] | (x[k + 5] << 8)) + 1;
        k += 4 + (size_t)slen;
    }
    if (bs < 12u + xlen + 8u) return false;
    m.resize(bs);
    if (pread(fd, m.data(), bs, (off_t)off) != (ssize_t)bs) return false;
    *bsize = bs;
    memcpy(isize, m.data() + bs - 4, 4);
    return true;
}

bool inflate_member(const std::vector<uint8_t> &m, uint32_t isize, std::string &dst) {
    const size_t h = 12 + (size_t)(uint16_t)(m[10] | (m[11] << 8));
    const size_t at = dst.size();
    dst.resize(at + isize);
    if (!isize) return true;
    z_stream zs; memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = (Bytef *)m.data() + h; zs.avail_in = (uInt)(m.size() - h - 8);
    zs.next_out = (Bytef *)&dst[at]; zs.avail_out = isize;
    const int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    return rc == Z_STREAM_END && zs.avail_out == 0;
}

void reg2bins(int64_t beg, int64_t end, std::vector<uint32_t> &bins) {
    bins.clear(); --end;
    bins.push_back(0);
    const int shifts[5] = {26, 23, 20, 17, 14}; const uint32_t base[5] = {1, 9, 73, 585, 4681};
    for (int l = 0; l < 5; l++)
        for (int64_t b = beg >> shifts[l]; b <= end >> shifts[l]; b++) bins.push_back(base[l] + (uint32_t)b);
}

struct TbiRef { std::unordered_map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins; std::vector<uint64_t> ioff; };

bool read_tbi(const std::string &path, std::vector<std::string> &names, std::vector<TbiRef> &refs) {
    gzFile g = gzopen(path.c_str(), "rb");
    if (!g) return false;
    std::string d; char b[1 << 16]; int n;
    while ((n = gzread(g, b, sizeof b)) > 0) d.append(b, (size_t)n);
    gzclose(g);
    auto i32 = [&](size_t p) { int32_t v; memcpy(&v, d.data() + p, 4); return v; };
    if (d.size() < 36 || d.compare(0, 4, "TBI\x01", 4) != 0) return false;
    const int32_t n_ref = i32(4), l_nm = i32(32);
    size_t p = 36;
    if (n_ref < 0 || l_nm < 0 || p + (size_t)l_nm > d.size()) return false;
    for (size_t a = p; a < p + (size_t)l_nm;) {
        size_t z = d.find('\0', a);
        if (z == std::string::npos) return false;
        names.push_back(d.substr(a, z - a)); a = z + 1;
    }
    p += (size_t)l_nm;
    refs.resize((size_t)n_ref);
    for (int r = 0; r < n_ref; r++) {
        if (p + 4 > d.size()) return false;
        const int32_t n_bin = i32(p); p += 4;
        for (int k = 0; k < n_bin; k++) {
            if (p + 8 > d.size()) return false;
            uint32_t bin; memcpy(&bin, d.data() + p, 4);
            const int32_t nc = i32(p + 4); p += 8;
            if (nc < 0 || p + 16 * (size_t)nc > d.size()) return false;
            auto &v = refs[(size_t)r].bins[bin];
            for (int c = 0; c < nc; c++) { uint64_t cb, ce; memcpy(&cb, d.data() + p, 8); memcpy(&ce, d.data() + p + 8, 8); v.emplace_back(cb, ce); p += 16; }
        }
        if (p + 4 > d.size()) return false;
        const int32_t n_intv = i32(p); p += 4;
        if (n_intv < 0 || p + 8 * (size_t)n_intv > d.size()) return false;
        refs[(size_t)r].ioff.resize((size_t)n_intv);
        if (n_intv) memcpy(refs[(size_t)r].ioff.data(), d.data() + p, 8 * (size_t)n_intv);
        p += 8 * (size_t)n_intv;
    }
    return (int)names.size() == n_ref;
}

char *to_malloc(const std::string &s) {
    char *p = (char *)malloc(s.size() + 1);
    if (p) { memcpy(p, s.data(), s.size()); p[s.size()] = 0; }
    return p;
}

// the lookup both entry points share; C.cols set: column mode, no header line is looked for
int lookup(Ctx &C, const char *path, int64_t n_keys, const char *const *contig, const int64_t *pos, int32_t n_samples, const char *const *samples,
           int use_index, int threads, char **out, int64_t *out_len, char **contigs_out, int64_t *contigs_len) {
    if (!path || n_keys < 0 || !out || !out_len || !contigs_out || !contigs_len || (n_keys && (!contig || !pos))) return PHZ_E_ARG;
    *out = nullptr; *out_len = 0; *contigs_out = nullptr; *contigs_len = 0;
    const bool want_header = C.cols == nullptr;
    if (C.hi) {
        for (int64_t k = 0; k < n_keys; k++)
            if (C.hi[k] >= pos[k]) C.regions[contig[k]].emplace_back(pos[k], C.hi[k]);
        for (auto &r : C.regions) {
            auto &iv = r.second;
            std::sort(iv.begin(), iv.end());
            size_t m = 0;
            for (size_t i = 1; i < iv.size(); i++) {
                if (iv[i].first <= iv[m].second + 1) iv[m].second = std::max(iv[m].second, iv[i].second);
                else iv[++m] = iv[i];
            }
            iv.resize(m + 1);
        }
    } else {
        for (int64_t k = 0; k < n_keys; k++) C.keys.emplace(Key{contig[k], pos[k]}, k);
    }
    const int nt = std::max(1, std::min(threads, 64));
    std::vector<std::string> contigs;
    std::string result;
    const std::string tbi = std::string(path) + ".tbi";
    std::vector<std::string> names; std::vector<TbiRef> refs;
    const bool indexed = use_index && access(tbi.c_str(), R_OK) == 0 && read_tbi(tbi, names, refs);
    // ---- header: the #CHROM line (the index path inflates members from the file start until the line is complete)
    std::string head;
    char *whole_p = nullptr; int64_t whole_n = 0;
    if (indexed && want_header) {
        int fd = open(path, O_RDONLY);
        if (fd < 0) return PHZ_E_ARG;
        uint64_t off = 0; std::vector<uint8_t> m; std::string txt;
        while (true) {
            uint32_t bs, is;
            if (!member_at(fd, off, &bs, &is, m)) break;
            if (!inflate_member(m, is, txt)) { close(fd); return PHZ_E_UNSUPPORTED; }
            off += bs;
            size_t a = txt.find("#CHROM");
            if (a != std::string::npos && txt.find('\n', a) != std::string::npos) { head = txt.substr(a, txt.find('\n', a) - a); break; }
            if (!is) break;
        }
        close(fd);
    } else if (!indexed) {
        if (int st = phz_bgzf_read(path, nt, &whole_p, &whole_n)) return st;
        std::string_view w(whole_p, (size_t)whole_n);
        const size_t a = want_header ? w.find("#CHROM") : std::string_view::npos;
        if (a != std::string_view::npos) head = std::string(w.substr(a, w.find('\n', a) - a));
    }
    if (!head.empty() && head.back() == '\r') head.pop_back();
    {
        std::vector<std::string> cols;
        for (size_t a = 0;;) {
            size_t b = head.find('\t', a);
            cols.push_back(head.substr(a, b == std::string::npos ? std::string::npos : b - a));
            if (b == std::string::npos) break;
            a = b + 1;
        }
        for (int s = 0; s < n_samples; s++) {
            int32_t c = -1;
            for (size_t j = 9; j < cols.size(); j++) if (cols[j] == samples[s]) c = (int32_t)j;      // a repeated name: the last column
            C.scol.push_back(c);
        }
    }
    if (!indexed) {
        scan(C, whole_p, whole_p + whole_n, result, &contigs);
        phz_buf_free(whole_p);
    } else {
        contigs = names;
        std::unordered_map<std::string, int> rid;
        for (size_t r = 0; r < names.size(); r++) rid.emplace(names[r], (int)r);
        std::vector<std::pair<uint64_t, uint64_t>> ch;
        std::vector<uint32_t> bins;
        for (int64_t k = 0; k < n_keys; k++) {
            auto it = rid.find(contig[k]);
            if (it == rid.end() || (C.hi ? C.hi[k] < pos[k] || C.hi[k] < 1 : pos[k] < 1)) continue;
            const TbiRef &R = refs[(size_t)it->second];
            const int64_t top = (int64_t)1 << 29;                     // the index's coordinate space
            const int64_t beg = std::min(top - 1, std::max<int64_t>(pos[k], 1) - 1), end = C.hi ? std::min(top, std::max(C.hi[k], beg + 1)) : pos[k];
            const size_t w = (size_t)(beg >> 14);
            const uint64_t min_off = R.ioff.empty() ? 0 : (w < R.ioff.size() ? R.ioff[w] : R.ioff.back());
            reg2bins(beg, end, bins);
            for (uint32_t b : bins) {
                auto f = R.bins.find(b);
                if (f == R.bins.end()) continue;
                for (auto &c : f->second) if (c.second > min_off) ch.emplace_back(std::max(c.first, min_off), c.second);
            }
        }
        std::sort(ch.begin(), ch.end());
        std::vector<std::pair<uint64_t, uint64_t>> span;           // disjoint, in file order
        for (auto &c : ch) {
            if (!span.empty() && c.first <= span.back().second) span.back().second = std::max(span.back().second, c.second);
            else span.push_back(c);
        }
        std::vector<std::string> part(span.size());
        std::atomic<size_t> next{0}; std::atomic<int> bad{0};
        auto work = [&]() {
            int fd = open(path, O_RDONLY);
            if (fd < 0) { bad = 1; return; }
            std::vector<uint8_t> m; std::string txt;
            for (size_t s; (s = next++) < span.size();) {
                const uint64_t c0 = span[s].first >> 16, c1 = span[s].second >> 16;
                const size_t u0 = (size_t)(span[s].first & 0xFFFF), u1 = (size_t)(span[s].second & 0xFFFF);
                txt.clear();
                uint64_t off = c0; size_t last_start = 0;
                bool ok = true;
                while (true) {
                    uint32_t bs, is;
                    if (!member_at(fd, off, &bs, &is, m)) { ok = false; break; }
                    last_start = txt.size();
                    if (!inflate_member(m, is, txt)) { ok = false; break; }
                    if (off >= c1) break;
                    off += bs;
                }
                const size_t e = last_start + u1;
                if (!ok || off != c1 || u0 > e || e > txt.size()) { bad = 1; continue; }
                scan(C, txt.data() + u0, txt.data() + e, part[s], nullptr);
            }
            close(fd);
        };
        std::vector<std::thread> th;
        const int nw = (int)std::min<size_t>((size_t)nt, std::max<size_t>(1, span.size()));
        for (int t = 0; t < nw; t++) th.emplace_back(work);
        for (auto &t : th) t.join();
        if (bad) return PHZ_E_UNSUPPORTED;
        for (auto &p : part) result += p;
    }
    std::string cs;
    for (auto &c : contigs) { cs += c; cs += '\n'; }
    *out = to_malloc(result); *contigs_out = to_malloc(cs);
    if (!*out || !*contigs_out) { free(*out); free(*contigs_out); *out = *contigs_out = nullptr; return PHZ_E_NOMEM; }
    *out_len = (int64_t)result.size(); *contigs_len = (int64_t)cs.size();
    return PHZ_OK;
}

}  // namespace

extern "C" int phz_vcf_lookup(const char *path, int64_t n_keys, const char *const *contig, const int64_t *pos, int32_t n_samples,
                              const char *const *samples, int use_index, int threads, char **out, int64_t *out_len, char **contigs_out,
                              int64_t *contigs_len) {
    if (n_samples < 0 || (n_samples && !samples)) return PHZ_E_ARG;
    Ctx C;
    return lookup(C, path, n_keys, contig, pos, n_samples, samples, use_index, threads, out, out_len, contigs_out, contigs_len);
}

extern "C" int phz_vcf_site_genotypes(const char *path, int64_t n_keys, const char *const *contig, const int64_t *pos, int32_t n_samples,
                                      const char *const *samples, int use_index, int threads, char **out, int64_t *out_len, char **contigs_out,
                                      int64_t *contigs_len) {
    if (n_samples < 0 || (n_samples && !samples)) return PHZ_E_ARG;
    Ctx C;
    C.geno = true;
    return lookup(C, path, n_keys, contig, pos, n_samples, samples, use_index, threads, out, out_len, contigs_out, contigs_len);
}

extern "C" int phz_tabix_lines(const char *path, int64_t n_keys, const char *const *contig, const int64_t *pos, int32_t n_cols, const int32_t *cols,
                               int use_index, int threads, char **out, int64_t *out_len, char **contigs_out, int64_t *contigs_len) {
    if (n_cols < 1 || !cols) return PHZ_E_ARG;
    Ctx C;
    C.cols = cols; C.n_cols = n_cols;
    return lookup(C, path, n_keys, contig, pos, 0, nullptr, use_index, threads, out, out_len, contigs_out, contigs_len);
}

extern "C" int phz_vcf_region_classes(const char *path, int64_t n_regions, const char *const *contig, const int64_t *lo, const int64_t *hi, int32_t n_samples,
                                      const char *const *samples, int use_index, int threads, char **out, int64_t *out_len, char **contigs_out,
                                      int64_t *contigs_len) {
    if (n_samples < 0 || (n_samples && !samples) || (n_regions && !hi)) return PHZ_E_ARG;
    static const int64_t none = 0;
    Ctx C;
    C.hi = n_regions ? hi : &none;
    return lookup(C, path, n_regions, contig, lo, n_samples, samples, use_index, threads, out, out_len, contigs_out, contigs_len);
}
