// Host unit test of phaser_amd/csrc/phz_stagepack.h (built and run by tests/test_stage_pack.py): the 4-byte staging word of K_map round-trips every field
// at its limits, fields do not bleed into each other, and the host predicate chooses the narrow form exactly inside its three limits.
#include "phz_stagepack.h"
#include <stdio.h>

static long long checks = 0;
static int fail(const char *what, unsigned a, unsigned b, unsigned c) {
    printf("FAIL %s var %u rec %u code %u\n", what, a, b, c);
    return 1;
}

int main() {
    static_assert(STAGE4_VAR_BITS + STAGE4_REC_BITS + STAGE4_CODE_BITS == 32, "the word is 32 bits");
    const uint32_t vars[] = {0u, 1u, 2u, 0x7FFFFu, 0x80000u, 0xAAAAAu, 0x55555u, 0xFFFFEu, 0xFFFFFu};          // 0 .. 2^20 - 1
    const uint32_t recs[] = {0u, 1u, 127u, 128u, 0xAAu, 0x55u, 254u, 255u};
    for (uint32_t var : vars)
        for (uint32_t rec : recs)
            for (uint32_t code = 0; code < 16; code++) {        // the kernels emit 0 .. 3 (a base) and 4 (text); all sixteen values of the field are checked
                const uint32_t w = stage4_pack(var, rec, code);
                if (stage4_var(w) != var) return fail("var", var, rec, code);
                if (stage4_rec(w) != rec) return fail("rec", var, rec, code);
                if (stage4_code(w) != code) return fail("code", var, rec, code);
                checks += 3;
            }
    // every record number of a tile and every single bit of the variant field, exhaustively
    for (uint32_t rec = 0; rec < 256; rec++)
        for (int b = 0; b <= STAGE4_VAR_BITS; b++) {
            const uint32_t var = b == STAGE4_VAR_BITS ? 0u : 1u << b;
            const uint32_t w = stage4_pack(var, rec, 4u);
            if (stage4_var(w) != var || stage4_rec(w) != rec || stage4_code(w) != 4u) return fail("bits", var, rec, 4u);
            checks++;
        }
    if (stage4_pack(0xFFFFFu, 255u, 15u) != 0xFFFFFFFFu || stage4_pack(0u, 0u, 0u) != 0u) return fail("extremes", 0, 0, 0);
    if (stage4_pack(1u, 0u, 0u) != 1u || stage4_pack(0u, 1u, 0u) != (1u << 20) || stage4_pack(0u, 0u, 1u) != (1u << 28)) return fail("layout", 0, 0, 0);
    checks += 5;

    // the host's choice: narrow iff no text planes, tile_reads <= 256, every table <= 2^20 entries, not forced wide
    struct { bool text; int tile_reads; int64_t nv; bool force; bool want; } cases[] = {
        {false, 256, 1, false, true},
        {false, 256, (int64_t)1 << 20, false, true},
        {false, 256, ((int64_t)1 << 20) + 1, false, false},
        {false, 256, 0x7fffffff, false, false},
        {false, 255, 1000, false, true},
        {false, 257, 1000, false, false},
        {false, 512, 1000, false, false},
        {true, 256, 1000, false, false},
        {false, 256, 1000, true, false},
        {true, 512, ((int64_t)1 << 20) + 1, true, false},
        {false, 1, 0, false, true},
    };
    for (const auto &c : cases) {
        if (stage_narrow_form(c.text, c.tile_reads, c.nv, c.force) != c.want) {
            printf("FAIL predicate text %d tile_reads %d nv %lld force %d\n", (int)c.text, c.tile_reads, (long long)c.nv, (int)c.force);
            return 1;
        }
        checks++;
    }
    printf("ok %lld\n", checks);
    return 0;
}
