// TEST INFRASTRUCTURE ONLY: PhzMail (phaser_amd/csrc/phz_internal.h) driven directly, for tests/test_emu_mail.py.  Compiled by g++ against the
// host-side HIP emulation and linked to libphz_emu.so; no entry point of the library queues a caller-chosen number of values.
#include "phz_internal.h"

extern "C" int mail_unit_queue(phz_ctx *ctx, int n_values, uint32_t *back) {
    static uint32_t word[PhzMail::MAX + 4];
    for (int i = 0; i < PhzMail::MAX + 4; i++) word[i] = 1000u + (uint32_t)i;
    PhzMail mail(ctx);
    int slot[PhzMail::MAX + 4];
    for (int i = 0; i < n_values && i < PhzMail::MAX + 4; i++) slot[i] = mail.add(&word[i], 4);
    if (int s = mail.send()) return s;
    PHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n_values; i++) back[i] = *mail.at<uint32_t>(slot[i]);
    return PHZ_OK;
}
