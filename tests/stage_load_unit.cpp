// Host-side unit test of phaser_amd/csrc/phz_stageload.h (the lengths of a K_map tile's staging descriptors): every length against the guards the
// loads had before -- a lane's word is inside the descriptor exactly when the old test let the lane load, and the index it loads is the old one.
#include "phz_stageload.h"
#include <stdio.h>

static long long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const int TILE = 256;
    // records of a tile and the cigar_off slice: shards of 1 .. 3 tiles and a bit, every tile of them
    for (int64_t n = 1; n <= 3 * TILE + 2; n++) {
        for (int64_t r0 = 0; r0 < n; r0 += TILE) {
            const int nr = stage_tile_records(n, r0, TILE);
            CHECK(nr >= 1 && nr <= TILE && r0 + nr <= n && (nr == TILE || r0 + nr == n));
            CHECK(r0 + (int64_t)stage_coff_words(nr) <= n + 1);            // the slice lies inside the shard's cigar_off array of n + 1 words
            for (int j = 0; j < TILE; j++) {
                const uint32_t idx = stage_coff_index(j, nr);
                CHECK(idx < stage_coff_words(nr));                         // always inside the slice: a lane past the tile gets a real word, not the 0 of a miss
                CHECK(j < nr ? idx == (uint32_t)j : r0 + idx == r0 + nr);  // a record's own offset; past the tile, the offset that ends the tile's last record
            }
        }
    }
    // the window: entry j is loaded exactly when j < wlen and w0 + j < nv
    const int nvs[] = {0, 1, 7, 8, 9, 130, 511, 512, 513, 100000, 0x7fffffff};
    const int wlens[] = {0, 1, 8, 9, 127, 128, 129, 511, 512};
    for (int nv : nvs) {
        for (int wlen : wlens) {
            for (int back = -3; back <= 520; back++) {
                const long long w0l = (long long)nv - back;                // window starts `back` entries before the table's end (negative: never produced, still clamped)
                if (w0l < 0 || w0l > 0x7fffffff) continue;
                const int w0 = (int)w0l;
                const uint32_t live = stage_window_words(wlen, nv, w0);
                CHECK(live <= (uint32_t)wlen);
                for (int j = 0; j < 520; j += (j < 10 || j > 500 ? 1 : 7)) {
                    const bool old_guard = j < wlen && (long long)w0 + j < (long long)nv;
                    CHECK(((uint32_t)j < live) == old_guard);
                }
            }
        }
    }
    // the CIGAR words: min(words of the tile, the LDS cap)
    const uint32_t cap = 640;
    const uint32_t words[] = {0, 1, 256, 383, 384, 385, 639, 640, 641, 799, 100000, 0xffffffffu};
    for (uint32_t w : words) {
        const uint32_t c = stage_cigar_words(w, cap);
        CHECK(c <= cap && c <= w && (c == w || c == cap));
    }
    printf("ok %lld\n", checks);
    return 0;
}
