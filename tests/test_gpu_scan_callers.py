"""Entry points that scan, on the MI355X, where the existing tests do not reach: phz_intern_device / phz_names_append_device beyond 64 scan tiles with sums that
differ from tile to tile, and one ctx used in turn by the interner, K_tally, K_map_general, the interner again and K_tally again (K_tally and K_map_general
share the look-back status words of gscan_excl, phaser_amd/csrc/phz_scan.h; the interner's scans are phz_bamdev.hip's own).  Every expected value is worked out
here with a dict and numpy.cumsum; all comparisons are exact.  (K_annot's scan over a batch of more than one chunk is in tests/test_annotate.py.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 4096                       # elements per scan tile, in phz_scan.h and in phz_bamdev.hip's own scan
OVER_64_TILES = 65 * TILE + 7
BASE_BYTES = 13
ALPHABET = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789:/_", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def names_case(n):
    """-> (n record names of 1 to 12 bytes drawn with repeats from about n / 3 distinct ones, 1,000 distinct store names of which half recur among the records);
    computed once, never changed"""
    rng = np.random.default_rng(1000 + n % 9973)
    want = max(1, n // 3)
    pool = {}
    while len(pool) < want:
        raw = ALPHABET[rng.integers(0, len(ALPHABET), (want, 12))]
        for row, k in zip(raw, rng.integers(1, 13, want).tolist()):
            pool.setdefault(row[:k].tobytes(), None)
            if len(pool) == want:
                break
    pool = list(pool)
    names = tuple(pool[int(i)] for i in rng.integers(0, len(pool), n))
    recurring = [pool[int(i)] for i in rng.choice(len(pool), size=min(500, len(pool)), replace=False)]
    absent = [b"#%d" % i for i in range(1000 - len(recurring))]             # '#' is not in the alphabet
    old = recurring + absent
    old = tuple(old[int(i)] for i in rng.permutation(len(old)))
    return names, old


def expected(names, old):
    """what phz_intern assigns: an old name keeps its id, a new one gets n_old + its rank of first appearance"""
    ids = {nm: i for i, nm in enumerate(old)}
    assert len(ids) == len(old)
    qid, first = [], []
    for i, nm in enumerate(names):
        k = ids.get(nm)
        if k is None:
            k = ids[nm] = len(old) + len(first)
            first.append(i)
        qid.append(k)
    lens = np.array([len(names[i]) for i in first], dtype=np.int64)
    dst_off = BASE_BYTES + np.concatenate([[0], np.cumsum(lens)])
    return {"qid": np.array(qid, np.int32), "first_idx": np.array(first, np.int32), "n_new": len(first), "dst_off": dst_off, "total_bytes": int(dst_off[-1]),
            "bytes": np.frombuffer(b"".join(names[i] for i in first), dtype=np.uint8)}


def pack(names):
    blob = np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int32)
    return torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda()


def device(ctx, names, old):
    """phz_intern_device, then both steps of phz_names_append_device -> the same keys as expected()"""
    p = lambda t: C.c_void_p(t.data_ptr())
    n = len(names)
    qn, qo = pack(names)
    st, so = pack(old) if old else (None, None)
    qid = torch.full((n,), -7, dtype=torch.int32, device="cuda"); first = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    n_new = C.c_int64(-1)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.phz_intern_device(ctx.h, p(qn), p(qo), n, p(st) if old else None, p(so) if old else None, len(old), p(qid), p(first), C.byref(n_new)))
    m = int(n_new.value)
    got = {"qid": qid.cpu().numpy(), "first_idx": first[:m].cpu().numpy(), "n_new": m}
    dst_off = torch.full((m + 2,), -7, dtype=torch.int32, device="cuda")
    total = C.c_int64(-1)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.phz_names_append_device(ctx.h, p(qn), p(qo), p(first), m, BASE_BYTES, p(dst_off), None, C.byref(total)))
    got["total_bytes"] = int(total.value)
    blob = torch.full((got["total_bytes"] + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx.lib.phz_names_append_device(ctx.h, p(qn), p(qo), p(first), m, BASE_BYTES, p(dst_off), p(blob), C.byref(total)))
    off = dst_off.cpu().numpy()
    blob = blob.cpu().numpy()
    assert off[m + 1] == -7 and np.all(blob[:BASE_BYTES] == 0xEE) and np.all(blob[got["total_bytes"]:] == 0xEE), "wrote outside dst_off[0 .. m] / the new names' bytes"
    got["dst_off"] = off[:m + 1].astype(np.int64) if m else np.array([BASE_BYTES], np.int64)
    got["bytes"] = blob[BASE_BYTES:got["total_bytes"]]
    return got


def check_intern(ctx, names, old, what):
    want, got = expected(names, old), device(ctx, names, old)
    for k in ("n_new", "total_bytes"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("qid", "first_idx", "dst_off", "bytes"):
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, (what, k, "first of %d differences at" % bad.size, int(bad[0]), "got", int(got[k][bad[0]]), "want", int(want[k][bad[0]]))
    return want


@pytest.mark.parametrize("with_store", [False, True], ids=["empty_store", "store_of_1000"])
@pytest.mark.parametrize("n", [1, 4097, OVER_64_TILES])
def test_interning_and_name_store_match_a_dict(n, with_store):
    """one tile, two tiles, more than 64 tiles: `first` holds 0 / 1 flags and the lengths are 1 .. 12, so the tile sums differ from tile to tile and a tile that
    took a predecessor's sum for another's gives a wrong id or offset"""
    from phaser_amd.mapper import Mapper
    names, old = names_case(n)
    ctx = Mapper(0).ctx
    want = check_intern(ctx, names, old if with_store else (), (n, with_store))
    if n > 64 * TILE:
        flags = np.zeros(n, np.int64); flags[want["first_idx"]] = 1          # what the interner scans
        assert len(set(np.add.reduceat(flags, np.arange(0, n, TILE)).tolist())) > 8
    if with_store:
        assert 0 < (want["qid"] < len(old)).sum() < n or n == 1          # old names do recur among the records, new ones appear too
    ctx.close()


from test_gpu_pipeline import small_tally          # noqa: E402,F401  (the fixture tally of test_tally_after_another_stage_on_the_same_ctx)


def test_one_ctx_many_owners_of_the_status_words(small_tally, oracle_build):
    """interner (65 tiles), K_tally, K_map_general, the interner again on other sums, K_tally again -- all on ONE ctx, whose scratch they share and whose
    look-back status words, epoch and ticket base K_tally and K_map_general share: each result is the expected one, and the tally does not redo its pair pass"""
    import indel_inputs as ii
    from phaser_amd import _lib
    from phaser_amd.mapper import Mapper
    from test_emu_tally import run_tally
    from test_gpu_mapper_general import check_calls
    from test_gpu_pipeline import _map_indel_reads
    saved, chroms, nb, want = small_tally
    names, old = names_case(OVER_64_TILES)
    mapper = Mapper(0)
    ctx = mapper.ctx

    def tally(what):
        got, sz = run_tally(ctx, saved, chroms, nb)
        NV = want["nv"]
        assert np.array_equal(got["var_count"].reshape(NV, 3), want["var_count"]), what
        assert np.array_equal(got["var_first"], want["var_first"]), what
        assert np.array_equal(got["var_distinct"].reshape(NV, 3), want["var_distinct"]), what
        assert np.array_equal(got["var_rank"], want["var_rank"]), what
        assert np.array_equal(got["ea"], want["ea"]) and np.array_equal(got["eb"], want["eb"]), what
        assert np.array_equal(got["linked"], want["linked"]), what
        assert np.array_equal(got["cto"].reshape(-1, 3), want["cto"]), what
        assert np.array_equal(got["stats"].reshape(5, -1), want["stats"]), what
        assert np.array_equal(got["rl_start"], want["rl_start"]) and np.array_equal(got["rl_qid"], want["rl_qid"]), what
        assert (int(sz.noise_match), int(sz.noise_mismatch)) == want["noise"] and int(sz.n_kept) == want["n_kept"], what

    check_intern(ctx, names, old, "first interning")
    tally("first tally")
    redos = ctx.counter(_lib.PHZ_C_PAIR_REDOS)
    rb, vt = ii.inputs("main")
    check_calls(_map_indel_reads(mapper), ii.expected(oracle_build, rb, vt, 10), "K_map_general between the interners")
    k = len(names) // 3 + 1
    check_intern(ctx, names[k:] + names[:k], old, "second interning, names rolled")
    tally("second tally")
    assert ctx.counter(_lib.PHZ_C_PAIR_REDOS) == redos
    ctx.close()
