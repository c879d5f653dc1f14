"""phaser_cis_var on the GPU (phaser_amd/cis_var.py + K_boot, phaser_amd/csrc/phz_cisvar.hip).

CPU tests: the numpy replay of the Philox stream against rocRAND's own engine; K_boot under the host emulation (on-chip and
forced-large paths) against the replay, bit for bit; the whole CLI with the replay in place of the launch against an independent
pandas restatement of the reference's measure_effect + to_csv; the stream's replicate medians against numpy.random.choice's in
distribution; the 16-bit packing at n = 32,768 and 65,535 and the refusal of 65,536.  GPU tests: the product kernel against the replay
-- also in launches whose workgroups serve several groups in a row, at the 16-bit limits, on a reused context and in PHZ_DEVICE space --
and a GTEx-shaped synthetic run for determinism."""
import gzip
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

HIPEMU = os.path.join(REPO, "tests", "hipemu")
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
EMU_DIR = os.path.join(HIPEMU, "_build", "cisvar")


# ------------------------------------------------------------------------------------------------ the stream, replayed in numpy
M32 = np.uint64(0xFFFFFFFF)


def philox(q, s, seed):
    q = np.asarray(q, dtype=np.uint64)
    c0 = q & M32; c1 = q >> np.uint64(32)
    c2 = np.full_like(q, np.uint64(s) & M32); c3 = np.full_like(q, np.uint64(s) >> np.uint64(32))
    k0 = np.uint64(seed) & M32; k1 = np.uint64(seed) >> np.uint64(32)
    for _ in range(10):
        m0 = np.uint64(0xD2511F53) * c0; m1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (m1 >> np.uint64(32)) ^ c1 ^ k0, m1 & M32, (m0 >> np.uint64(32)) ^ c3 ^ k1, m0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32; k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def stream_words(seed, s, offset, count):
    """words offset .. offset+count-1 of rocrand_device::philox4x32_10_engine(seed, s, 0)"""
    q0 = int(offset) // 4; q1 = (int(offset) + count - 1) // 4
    W = philox(np.arange(q0, q1 + 1, dtype=np.uint64), s, seed).reshape(-1)
    return W[int(offset) - 4 * q0:int(offset) - 4 * q0 + count]


def replicate_medians(values, seed, s, bs):
    values = np.asarray(values, dtype=np.float64)
    n = len(values)
    w = stream_words(seed, s, 0, bs * n).astype(np.uint64)
    P = ((w * np.uint64(n)) >> np.uint64(32)).astype(np.int64).reshape(bs, n)
    return np.median(values[P], axis=1), np.median(np.abs(values)[P], axis=1)


def replay_bootstrap(bi, want_replicates=False):
    """what phz_bootstrap_medians returns, from the replay"""
    G = bi.n_groups
    os_ = np.full((G, 2, 4), np.nan); sc = np.zeros((G, 2, 2), dtype=np.int64); reps = np.zeros((G, 2, bi.bs))
    for g in range(G):
        v = bi.values[bi.off[g]:bi.off[g + 1]]
        if not len(v):
            continue
        for k, r in enumerate(replicate_medians(v, bi.seed, int(bi.subseq[g]), bi.bs)):
            reps[g, k] = r
            srt = np.sort(r)
            os_[g, k] = srt[bi.k]
            sc[g, k] = [(r > 0).sum(), (r < 0).sum()]
    return os_, sc, (reps if want_replicates else None)


def test_stream_replay_matches_rocrand():
    hipcc = shutil.which("hipcc")
    if not hipcc or not os.path.exists("/opt/rocm/include/rocrand/rocrand_philox4x32_10.h"):
        pytest.skip("hipcc / rocRAND headers not present")
    os.makedirs(EMU_DIR, exist_ok=True)
    src = os.path.join(EMU_DIR, "philox_ref.cpp"); exe = os.path.join(EMU_DIR, "philox_ref")
    with open(src, "w") as f:
        f.write("#include <rocrand/rocrand_philox4x32_10.h>\n#include <cstdio>\n#include <cstdlib>\n"
                "int main(int c, char **v) {\n"
                "  rocrand_device::philox4x32_10_engine e(strtoull(v[1], 0, 10), strtoull(v[2], 0, 10), strtoull(v[3], 0, 10));\n"
                "  for (int i = 0, n = atoi(v[4]); i < n; i++) printf(\"%u\\n\", e());\n  return 0;\n}\n")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", src, "-o", exe])
    cases = [(0, 0, 0), (0, 1, 3), (12345, 7 << 16, 5), (2 ** 64 - 1, 2 ** 40 + 3, 2 ** 32 - 6), (99, 2 ** 63 + 5, 2 ** 34 + 2),
             (7, 3, 4 * (2 ** 32 - 1) - 3), (42, (1234 << 16) + 2 * 3 + 1, 10_000 * 671 - 9)]
    for seed, s, off in cases:
        want = [int(x) for x in subprocess.check_output([exe, str(seed), str(s), str(off), "40"], text=True).split()]
        assert stream_words(seed, s, off, 40).tolist() == want, (seed, s, off)


# ------------------------------------------------------------------------------------------------ K_boot under the emulation
def _emu_lib(lds_n=None):
    import ctypes as C
    from phaser_amd import _lib
    os.makedirs(EMU_DIR, exist_ok=True)
    tag = "" if lds_n is None else "_n%d" % lds_n
    lib = os.path.join(EMU_DIR, "libphz_cisvar%s.so" % tag)
    srcs = [os.path.join(CSRC, "phz_api.hip"), os.path.join(CSRC, "phz_cisvar.hip"), os.path.join(HIPEMU, "hipemu.cpp")]
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(REPO, "include", "phz.h"), os.path.join(HIPEMU, "hipemu.h")]
    newest = max(os.path.getmtime(p) for p in srcs + hdrs)
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        import fcntl
        with open(os.path.join(EMU_DIR, ".lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            flags = ["-O1", "-std=c++17", "-fPIC", "-I" + os.path.join(HIPEMU, "include"), "-I" + os.path.join(REPO, "include"), "-I" + CSRC]
            defs = [] if lds_n is None else ["-DPHZ_BOOT_LDS_N=%d" % lds_n, "-DPHZ_BOOT_GRID=3"]
            objs = []
            for src in srcs:
                obj = os.path.join(EMU_DIR, os.path.basename(src) + tag + ".o"); objs.append(obj)
                lang = [] if src.endswith(".cpp") else ["-x", "c++"]
                subprocess.check_call(["g++"] + flags + defs + lang + ["-c", src, "-o", obj])
            subprocess.check_call(["g++", "-shared", "-fPIC"] + objs + ["-o", lib + ".tmp", "-lpthread"])
            os.replace(lib + ".tmp", lib)
    L = C.CDLL(lib)
    for name in ("phz_ctx_create", "phz_ctx_destroy", "phz_last_error", "phz_bootstrap_medians"):
        res, args = _lib.SYMBOLS[name]
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


def _emu_ctx(L):
    import ctypes as C
    h = C.c_void_p()
    assert L.phz_ctx_create(0, C.byref(h)) == 0
    return h


def _groups(rng, sizes, ties=True, zeros=True):
    vals = []
    for n in sizes:
        v = rng.normal(0, 1.5, n)
        if ties and n > 2:
            v[rng.integers(0, n, n // 3)] = v[0]
        if zeros and n > 3:
            v[1] = 0.0; v[2] = -0.0
        vals.append(v)
    off = np.zeros(len(sizes) + 1, dtype=np.int64); np.cumsum(sizes, out=off[1:])
    return (np.concatenate(vals) if vals else np.zeros(0)), off


def _same(a, b):
    """bit-equal, except that a zero may carry either sign (the signed-zero rule)"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    z = (a == 0) & (b == 0)
    return np.array_equal(np.where(z, 0.0, a).view(np.uint64), np.where(z, 0.0, b).view(np.uint64)) or \
        (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(z | np.isnan(a), 0.0, a), np.where(z | np.isnan(b), 0.0, b)))


@pytest.mark.parametrize("lds_n", [None, 8])
def test_kboot_emulated_matches_replay(lds_n):
    from phaser_amd import _lib, cis_var
    _lib.build()
    L = _emu_lib(lds_n)
    h = _emu_ctx(L)
    rng = np.random.default_rng(3 if lds_n is None else 4)
    try:
        for bs, sizes in ((1, [1, 5, 12]), (2, [3, 0, 9]), (3, [2, 17]), (41, [1, 2, 3, 7, 8, 31, 0, 70]), (10000, [7]), (10001, [6])):
            vals, off = _groups(rng, sizes)
            sub = rng.integers(0, 2 ** 40, len(sizes), dtype=np.uint64)
            bi = cis_var.BootInput(vals, off, sub, int(rng.integers(0, 2 ** 63)), bs)
            got_os, got_sc, got_reps = cis_var.bootstrap_gpu(L, h, bi, want_replicates=True)
            want_os, want_sc, want_reps = replay_bootstrap(bi, want_replicates=True)
            for g, n in enumerate(sizes):
                if n == 0:
                    assert np.isnan(got_os[g]).all() and (got_sc[g] == 0).all()
                    continue
                assert _same(got_reps[g], want_reps[g]), (bs, n)
                assert _same(got_os[g], want_os[g]), (bs, n)
                assert np.array_equal(got_sc[g], want_sc[g]), (bs, n)
                for k in range(2):                               # the host's lerp of the order statistics = numpy.percentile itself
                    lo = cis_var.lerp(got_os[g, k, 0], got_os[g, k, 1], bi.gamma_lo)
                    hi = cis_var.lerp(got_os[g, k, 2], got_os[g, k, 3], bi.gamma_hi)
                    assert _same(lo, np.percentile(want_reps[g, k], 2.5)) and _same(hi, np.percentile(want_reps[g, k], 97.5)), (bs, n, k)
    finally:
        L.phz_ctx_destroy(h)


def _assert_boot_equals_replay(got, bi, what, reps=True):
    """order statistics, sign counts and (reps) every replicate of every group of a launch against the numpy replay"""
    got_os, got_sc, got_reps = got
    want_os, want_sc, want_reps = replay_bootstrap(bi, want_replicates=reps)
    sizes = np.diff(bi.off)
    for g, n in enumerate(sizes.tolist()):
        if n == 0:
            assert np.isnan(got_os[g]).all() and (got_sc[g] == 0).all(), (what, g)
            continue
        if reps:
            assert _same(got_reps[g], want_reps[g]), (what, g, n)
        assert _same(got_os[g], want_os[g]), (what, g, n, got_os[g].tolist(), want_os[g].tolist())
        assert np.array_equal(got_sc[g], want_sc[g]), (what, g, n, got_sc[g].tolist(), want_sc[g].tolist())


# sizes 0 .. 129 of 40 groups at bs 41: with the lds_n = 8 build (grid 3) every workgroup serves 13 or 14 groups one after the other,
# on-chip and global ones mixed
MIXED_40 = [129, 0, 1, 64, 2, 8, 9, 127, 3, 65, 0, 7, 128, 1, 63, 5, 100, 4, 0, 33, 8, 9, 2, 129, 1, 17, 66, 0, 3, 126, 7, 8, 90, 1, 2, 64, 11, 0, 129, 6]
PACKING_CASES = [(3, [65535]), (2, [65534, 3, 65535]), (41, MIXED_40), (2, [32768])]


@pytest.mark.parametrize("lds_n", [None, 8])
@pytest.mark.parametrize("case", range(len(PACKING_CASES)))
def test_kboot_emulated_16bit_packing_and_workgroup_reuse(lds_n, case):
    """The two 16-bit halves of a histogram word and of a rank at their limits -- bit 15 alone (n = 32,768), n = 65,535 -- and workgroups
    that serve many groups in a row, against the replay bit for bit."""
    from phaser_amd import _lib, cis_var
    _lib.build()
    L = _emu_lib(lds_n)
    h = _emu_ctx(L)
    bs, sizes = PACKING_CASES[case]
    rng = np.random.default_rng(50 + case)
    try:
        vals, off = _groups(rng, sizes)
        bi = cis_var.BootInput(vals, off, rng.integers(0, 2 ** 40, len(sizes), dtype=np.uint64), int(rng.integers(0, 2 ** 63)), bs)
        _assert_boot_equals_replay(cis_var.bootstrap_gpu(L, h, bi, want_replicates=True), bi, (lds_n, bs))
    finally:
        L.phz_ctx_destroy(h)


@pytest.mark.parametrize("lds_n", [None, 8])
def test_kboot_group_of_65536_samples_is_refused(lds_n):
    import ctypes as C
    from phaser_amd import _lib, cis_var
    _lib.build()
    rng = np.random.default_rng(60)
    with pytest.raises(cis_var.FatalError):
        cis_var.BootInput(rng.normal(size=65536 + 3), np.array([0, 3, 65539], dtype=np.int64), np.zeros(2, np.uint64), 1, 3)
    # the same group handed to the library in a phz_boot_in filled by hand: one more than the 16-bit halves can count
    bi = cis_var.BootInput(rng.normal(size=65535), np.array([0, 65535], dtype=np.int64), np.zeros(1, np.uint64), 1, 3)
    n = 65536
    off = np.array([0, n], dtype=np.int64); sub = np.zeros(1, np.uint64)
    rank = np.arange(n, dtype=np.uint32); rank |= rank << np.uint32(16)
    v = np.sort(rng.normal(size=n)); va = np.sort(np.abs(v))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    L = _emu_lib(lds_n)
    h = _emu_ctx(L)
    try:
        s = bi.struct()
        s.off = vp(off); s.subseq = vp(sub); s.rank = vp(rank); s.sorted_s = vp(v); s.sorted_a = vp(va); s.max_n = n
        os_ = np.full((1, 2, 4), -5.0); sc = np.full((1, 2, 2), -5, dtype=np.int64)
        assert L.phz_bootstrap_medians(h, C.byref(s), vp(os_), vp(sc), None, _lib.PHZ_HOST) == _lib.PHZ_E_ARG
        assert np.all(os_ == -5.0) and np.all(sc == -5)
        got = cis_var.bootstrap_gpu(L, h, bi)                    # the context is still usable, at the limit itself
        assert not np.isnan(got[0]).any()
    finally:
        L.phz_ctx_destroy(h)


def test_quantile_positions_match_numpy_percentile():
    from phaser_amd import cis_var
    rng = np.random.default_rng(5)
    for bs in (1, 2, 3, 4, 41, 200, 10000, 10001):
        x = rng.normal(size=bs)
        x[rng.integers(0, bs, bs // 4)] = x[0]
        s = np.sort(x)
        for q in (2.5, 97.5):
            p, n, t = cis_var.quantile_positions(bs, q)
            assert _same(cis_var.lerp(s[p], s[n], t), np.percentile(x, q)), (bs, q)


def test_ranksums_restatement_matches_scipy():
    stats = pytest.importorskip("scipy.stats")
    from phaser_amd import cis_var
    rng = np.random.default_rng(6)
    xs, ys = [], []
    for r in range(60):
        n1, n2 = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        xs.append(np.abs(np.round(rng.normal(size=n1), 1))); ys.append(np.abs(np.round(rng.normal(size=n2), 1)))
    xr = np.repeat(np.arange(60), [len(x) for x in xs]); yr = np.repeat(np.arange(60), [len(y) for y in ys])
    got = cis_var.ranksums_p(np.concatenate(xs), xr, np.concatenate(ys), yr, 60)
    import warnings
    for r in range(60):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = stats.ranksums(xs[r], ys[r]).pvalue
        assert _same(got[r], want), r


@pytest.mark.parametrize("n", [7, 8, 31])
def test_stream_medians_distribution_matches_numpy_choice(n):
    """Two-sample KS of 200k replicate medians: the Philox stream vs numpy.random.choice (seeded), alpha = 0.01."""
    rng = np.random.default_rng(n)
    v = np.round(rng.normal(size=n), 1)             # ties
    B = 200_000
    ours = replicate_medians(v, 11, (5 << 16) + 1, B)[0]
    theirs = np.median(v[np.random.default_rng(12).integers(0, n, (B, n))], axis=1)
    grid = np.union1d(ours, theirs)
    d = np.max(np.abs(np.searchsorted(np.sort(ours), grid, side="right") / B - np.searchsorted(np.sort(theirs), grid, side="right") / B))
    assert d < 1.628 * math.sqrt(2.0 / B), d


# ------------------------------------------------------------------------------------------------ end to end: restatement of the reference
def restate_reference(bed_text, vcf_text, pairs_text, map_text, pc=1, min_cov=8, chrom="", bs=10000, ignore_v=0, seed=0):
    """An independent pandas restatement of phaser_cis_var.py's measure_effect + to_csv, with bootstrap_ci's resamples taken
    from the documented stream (record order for several records, map-file order for the samples)."""
    pd = pytest.importorskip("pandas")
    from scipy.stats import ranksums
    import io
    import warnings
    smap = pd.read_csv(io.StringIO(map_text), sep="\t", index_col=False, dtype=str)
    dmap = dict(zip(smap["vcf_sample"], smap["bed_sample"]))
    pairs = pd.read_csv(io.StringIO(pairs_text), sep="\t", index_col=False, dtype={"var_contig": str, "var_id": str, "gene_id": str,
                                                                                     "var_ref": str, "var_alt": str}, keep_default_na=False)
    if ignore_v == 1:
        pairs["gene_id"] = [x.split(".")[0] for x in pairs["gene_id"]]
    if chrom:
        pairs = pairs[pairs.var_contig == chrom]
    lines = []
    genes = set(pairs["gene_id"])
    for l in bed_text.split("\n"):
        l = l.rstrip()
        if not l:
            continue
        c = l.split("\t")
        if l.startswith("#"):
            lines.append(l); continue
        if chrom and c[0] != chrom:
            continue
        if c[3] in genes:
            lines.append(l)
    bed = pd.read_csv(io.StringIO("\n".join(lines)), sep="\t", dtype=str, keep_default_na=False)
    bed.index = [x.split(".")[0] for x in bed["name"]] if ignore_v == 1 else list(bed["name"])
    if len(bed.index) == 0:
        return None
    vl = [l for l in vcf_text.split("\n") if l and not l.startswith("##")]
    cols = vl[0].lstrip("#").split("\t")
    recs = [dict(zip(cols, l.split("\t"))) for l in vl[1:]]
    out = []
    for xi, row in pairs.iterrows():
        if row["gene_id"] not in bed.index:
            continue
        rp = bed.loc[row["gene_id"]]
        ordinal = -1
        for rec in recs:
            if rec["CHROM"] != row["var_contig"] or int(rec["POS"]) != int(row["var_pos"]):
                continue
            ordinal += 1
            if not ((row["var_ref"] != "" and row["var_alt"] != "" and rec["REF"] == row["var_ref"] and rec["ALT"] == row["var_alt"])
                    or rec["ID"] == row["var_id"]):
                continue
            gi = rec["FORMAT"].split(":").index("GT")
            afcs = [[], []]; cnt = [[[], []], [[], []]]; ids = [[], []]
            for xs in dmap:
                if xs in rec and dmap[xs] in bed.columns:
                    cell = rp[dmap[xs]]
                    if cell == "":
                        continue
                    gt = rec[xs].split(":")[gi]
                    if "|" not in gt:
                        continue
                    c = list(map(float, cell.split("|")))
                    if sum(c) < min_cov:
                        continue
                    afc = math.log(float(c[0] + pc) / float(c[1] + pc), 2)
                    if "0" in gt and "1" in gt:
                        if "1" not in gt.split("|"):
                            continue
                        ai = gt.split("|").index("1")
                        if ai == 1:
                            afc *= -1
                        afcs[0].append(afc); ids[0].append(xs); cnt[0][0].append(int(c[int(not ai)])); cnt[0][1].append(int(c[ai]))
                    elif gt.count("0") == 2 or gt.count("1") == 2:
                        afcs[1].append(afc); ids[1].append(xs); cnt[1][0].append(int(c[0])); cnt[1][1].append(int(c[1]))
            cis = []
            for k in range(2):
                if afcs[k]:
                    s = (int(xi) << 16) + ordinal * 2 + k
                    rs, ra = replicate_medians(afcs[k], seed, s, bs)
                    for reps, vals, with_p in ((rs, afcs[k], k == 0), (ra, list(map(abs, afcs[k])), False)):
                        ci = [np.percentile(reps, 2.5), np.median(vals), np.percentile(reps, 97.5)]
                        if with_p:
                            ci.append(float(min(sum(int(x > 0) for x in reps), sum(int(x < 0) for x in reps))) / float(bs) * 2)
                        cis.append(ci)
                else:
                    cis.append([float("nan")] * (4 if k == 0 else 3)); cis.append([float("nan")] * 3)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                p = ranksums(list(map(abs, afcs[0])), list(map(abs, afcs[1])))[1] if afcs[0] and afcs[1] else float("nan")
            j = lambda x: ",".join(map(str, x))
            out.append([rp["name"], row["var_id"], row["var_contig"], int(row["var_pos"]), len(afcs[0]), len(afcs[1]), p] + cis[0] + cis[1] + cis[2] +
                       cis[3] + [j(afcs[0]), j(afcs[1]), j(cnt[0][0]), j(cnt[0][1]), j(cnt[1][0]), j(cnt[1][1]), j(ids[0]), j(ids[1])])
    from phaser_amd.cis_var import COLUMNS
    return pd.DataFrame(out, columns=COLUMNS).to_csv(sep="\t", index=False)


def _float_cols():
    from phaser_amd.cis_var import COLUMNS
    return {i for i, c in enumerate(COLUMNS) if c in ("het_hom_pvalue",) or c.endswith(("_lower", "_upper", "_afc", "_pval"))}


def assert_same_table(got, want):
    """bytes, except that the median / CI / p fields are compared as floats (a zero may carry either sign)"""
    gl, wl = got.split("\n"), want.split("\n")
    assert len(gl) == len(wl), (len(gl), len(wl))
    fc = _float_cols()
    for a, b in zip(gl, wl):
        fa, fb = a.split("\t"), b.split("\t")
        assert len(fa) == len(fb), (a, b)
        for i, (x, y) in enumerate(zip(fa, fb)):
            if x == y:
                continue
            assert i in fc and x and y and float(x) == float(y) == 0.0, (i, x, y, a, b)


def make_fixture(tmp, seed=1, n_samples=24, n_genes=12, extra=True, matrix="plain", tbi=False, versioned=True):
    """A small world: a phased VCF covering every GT class, a gene x sample matrix, pairs with every matching rule."""
    from phaser_amd import vcfout
    rng = np.random.default_rng(seed)
    samples = ["S%02d" % i for i in range(n_samples)]
    gts = ["0|1", "1|0", "0|0", "1|1", "0/1", "./.", "1|2", "0|10"]
    recs = []          # (chrom, pos, id, ref, alt, gts)
    pos = 1000
    for v in range(30):
        pos += int(rng.integers(5, 50))
        chrom = "chr1" if v < 20 else "chr2"
        if v == 20:
            pos = 500
        g = [gts[int(rng.integers(0, len(gts)))] for _ in samples]
        if v in (10, 11):                      # empty groups: no phased sample at all / no het
            g = ["0/1" if v == 10 else "0|0"] * len(samples)
        recs.append((chrom, pos, "rs%d" % v, "A", "G" if v % 7 else "G,T", g))
        if v in (3, 22):                       # two records at one position
            recs.append((chrom, pos, "rs%db" % v, "A", "C", [gts[int(rng.integers(0, 4))] for _ in samples]))
    vcf = ["##fileformat=VCFv4.2", "#" + "\t".join(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples)]
    for c, p, i, r, a, g in recs:
        fmt = "GT:DP" if p % 2 else "DP:GT"
        cells = [("%s:7" % x) if fmt == "GT:DP" else ("7:%s" % x) for x in g]
        vcf.append("\t".join([c, str(p), i, r, a, ".", "PASS", ".", fmt] + cells))
    vcf_text = "\n".join(vcf) + "\n"
    vpath = os.path.join(tmp, "x.vcf.gz")
    assert vcfout.write_bgzf(vpath, vcf_text, 2, index="vcf" if tbi else None) and os.path.exists(vpath + ".tbi") == tbi
    genes = [("ENSG%05d.%d" % (i, i % 3 + 1)) if versioned else ("ENSG%05d" % i) for i in range(n_genes)]
    bed = ["\t".join(["#contig", "start", "stop", "name"] + ["B" + s for s in samples])]
    for gi, gname in enumerate(genes):
        cells = []
        for si in range(n_samples):
            a, b = int(rng.integers(0, 14)), int(rng.integers(0, 14))
            if (gi, si) == (1, 2):
                cells.append("")                           # empty cell of a mapped sample
            elif si == 3:
                cells.append("4|4")                         # afc 0.0 -> -0.0 on the alt haplotype
            elif si == 4:
                cells.append("5|3")                         # total 8: the min_cov boundary
            elif si == 5:
                cells.append("4|3")
            else:
                cells.append("%d|%d" % (a + 1, b + 1))
        bed.append("\t".join(["chr1" if gi < 8 else "chr2", str(100 * gi), str(100 * gi + 50), gname] + cells))
    bed_text = "\n".join(bed) + "\n"
    if matrix == "plain":
        bpath = os.path.join(tmp, "m.bed")
        open(bpath, "w").write(bed_text)
    elif matrix == "gzip":
        bpath = os.path.join(tmp, "m.bed.gz")
        with gzip.open(bpath, "wt") as f:
            f.write(bed_text)
    else:
        bpath = os.path.join(tmp, "m.gw_phased.bed.gz")
        vcfout.write_bgzf(bpath, bed_text, 2)
    smap = ["vcf_sample\tbed_sample"] + ["%s\tB%s" % (s, s) for s in samples if s != "S07"] + ["S07\tBS07", "S99\tBS99"]
    pairs = ["gene_id\tvar_id\tvar_contig\tvar_pos\tvar_ref\tvar_alt"]
    for k, (c, p, i, r, a, g) in enumerate(recs):
        gname = genes[k % n_genes]
        if k % 5 == 1:
            pairs.append("\t".join([gname, i, c, str(p), "", a]))           # empty var_ref: ID only
        elif k % 5 == 2:
            pairs.append("\t".join([gname, i, c, str(p), "C", "T"]))        # REF/ALT mismatch, ID match
        elif k % 5 == 3:
            pairs.append("\t".join([gname, "nomatch", c, str(p), r, a]))    # REF/ALT match (a multi-allelic ALT too)
        else:
            pairs.append("\t".join([gname, i, c, str(p), r, a]))
    if extra:
        pairs.append("\t".join(["ENSG99999.1", "rsX", "chr1", "1001", "A", "G"]))        # gene absent
        pairs.append("\t".join([genes[0], "rsY", "chr1", "999999", "A", "G"]))           # no record
    open(os.path.join(tmp, "pairs.txt"), "w").write("\n".join(pairs) + "\n")
    open(os.path.join(tmp, "map.txt"), "w").write("\n".join(smap) + "\n")
    return {"bed": bpath, "bed_text": bed_text, "vcf": vpath, "vcf_text": vcf_text, "pairs": os.path.join(tmp, "pairs.txt"),
            "pairs_text": "\n".join(pairs) + "\n", "map": os.path.join(tmp, "map.txt"), "map_text": "\n".join(smap) + "\n"}


def _replay_hook(bi):
    return replay_bootstrap(bi)[:2]


E2E = [dict(), dict(pc=0, min_cov=9), dict(chrom="chr2"), dict(ignore_v=1), dict(min_cov=8, bs=33, seed=5)]


@pytest.mark.parametrize("matrix,tbi", [("plain", False), ("gzip", True), ("bgzf", False)])
@pytest.mark.parametrize("opt", range(len(E2E)))
def test_cis_var_host_stages_match_restatement(tmp_path, matrix, tbi, opt):
    pytest.importorskip("pandas"); pytest.importorskip("scipy")
    from phaser_amd import _lib, cis_var
    _lib.build()
    kw = dict(E2E[opt]); kw.setdefault("bs", 64)
    fx = make_fixture(str(tmp_path), seed=opt + 1, matrix=matrix, tbi=tbi, versioned=opt != 3 or matrix != "plain")
    want = restate_reference(fx["bed_text"], fx["vcf_text"], fx["pairs_text"], fx["map_text"], **kw)
    got = cis_var.cis_var(cis_var.read_text(fx["bed"]), fx["vcf"], fx["pairs_text"], fx["map_text"], threads=2, _bootstrap=_replay_hook, **kw)
    if want is None:
        assert got is None
        return
    assert got is not None
    assert got.count("\n") > 1 or opt == 3
    assert_same_table(got, want)


def test_cis_var_pc0_zero_count_is_fatal(tmp_path):
    from phaser_amd import _lib, cis_var
    _lib.build()
    fx = make_fixture(str(tmp_path))
    bed = fx["bed_text"].replace("\t4|4\t", "\t0|8\t")
    with pytest.raises(cis_var.FatalError):
        cis_var.cis_var(bed, fx["vcf"], fx["pairs_text"], fx["map_text"], pc=0, bs=8, _bootstrap=_replay_hook)


def test_cis_var_duplicate_gene_is_fatal_and_empty_matrix_prints_error(tmp_path):
    from phaser_amd import _lib, cis_var
    _lib.build()
    fx = make_fixture(str(tmp_path))
    lines = fx["bed_text"].split("\n")
    with pytest.raises(cis_var.FatalError):
        cis_var.cis_var("\n".join(lines[:2] + lines[1:]), fx["vcf"], fx["pairs_text"], fx["map_text"], bs=8, _bootstrap=_replay_hook)
    logs = []
    assert cis_var.cis_var(lines[0] + "\n", fx["vcf"], fx["pairs_text"], fx["map_text"], bs=8, log=logs.append, _bootstrap=_replay_hook) is None
    assert cis_var.NO_DATA in logs


def test_cis_var_seed_changes_only_the_resampled_columns(tmp_path):
    from phaser_amd import _lib, cis_var
    _lib.build()
    fx = make_fixture(str(tmp_path))
    a = cis_var.cis_var(fx["bed_text"], fx["vcf"], fx["pairs_text"], fx["map_text"], bs=50, seed=1, _bootstrap=_replay_hook)
    b = cis_var.cis_var(fx["bed_text"], fx["vcf"], fx["pairs_text"], fx["map_text"], bs=50, seed=2, _bootstrap=_replay_hook)
    c = cis_var.cis_var(fx["bed_text"], fx["vcf"], fx["pairs_text"], fx["map_text"], bs=50, seed=1, threads=4, _bootstrap=_replay_hook)
    assert a == c and a != b
    cols = cis_var.COLUMNS
    keep = [i for i, k in enumerate(cols) if not k.endswith(("_lower", "_upper", "_pval"))]
    pick = lambda t: [[r.split("\t")[i] for i in keep] for r in t.split("\n") if r]
    assert pick(a) == pick(b)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_kboot_gpu_matches_replay():
    from phaser_amd import _lib, cis_var
    ctx = _lib.Context(0)
    rng = np.random.default_rng(9)
    for bs, sizes in ((1, [1, 4]), (3, [2, 9, 0]), (41, [1, 2, 3, 7, 8, 31, 64, 65, 300]), (10000, [7, 8, 670, 1024, 1025]), (10001, [6, 333]),
                      (50000, [5000])):
        vals, off = _groups(rng, sizes)
        sub = rng.integers(0, 2 ** 40, len(sizes), dtype=np.uint64)
        bi = cis_var.BootInput(vals, off, sub, int(rng.integers(0, 2 ** 63)), bs)
        got_os, got_sc, got_reps = cis_var.bootstrap_gpu(ctx.lib, ctx.h, bi, want_replicates=True)
        for g, n in enumerate(sizes):
            if n == 0:
                assert np.isnan(got_os[g]).all()
                continue
            v = bi.values[bi.off[g]:bi.off[g + 1]]
            for k, r in enumerate(replicate_medians(v, bi.seed, int(bi.subseq[g]), bs)):
                assert _same(got_reps[g, k], r), (bs, n, k)
                assert _same(got_os[g, k], np.sort(r)[bi.k]), (bs, n, k)
                assert got_sc[g, k].tolist() == [(r > 0).sum(), (r < 0).sum()], (bs, n, k)


# ---- workgroups that serve several groups of one launch (grid-stride over PHZ_BOOT_GRID = 1024 workgroups), the 16-bit limits, a reused context, PHZ_DEVICE
BOOT_GRID = 1024            # PHZ_BOOT_GRID of the product build
BOOT_LDS_N = 1024           # PHZ_BOOT_LDS_N: larger groups count in the global histogram
REUSE_SIZES = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1500]
# what workgroup w meets in a row (groups w, w + 1024, w + 2048), planted on workgroups 0 .. 15 and again on 200 .. 215
REUSE_PLANTED = [(64, 1025, 63), (1024, 1500, 1023), (1500, 1025, 1024), (1500, 1025, 1500), (0, 129, 0), (0, 1500, 3), (1500, 1, 1025), (1025, 1, 1),
                 (1024, 1, 64), (1025, 0, 1500), (3, 1500, 2), (1500, 2, 1500), (1, 1025, 0), (128, 1500, 127), (1500, 1500, 1025), (65, 0, 1)]


def _reuse_sizes(rng, n_groups=2500):
    sizes = rng.choice(REUSE_SIZES, size=n_groups)
    for base in (0, 200):
        for i, seq in enumerate(REUSE_PLANTED):
            sizes[[base + i, base + i + BOOT_GRID, base + i + 2 * BOOT_GRID]] = seq
    # the sequences the launch must contain somewhere, checked on the sizes themselves
    rows = [tuple(int(sizes[g]) for g in range(w, n_groups, BOOT_GRID)) for w in range(BOOT_GRID)]
    assert min(len(r) for r in rows) == 2 and max(len(r) for r in rows) == 3
    big = lambda n: n > BOOT_LDS_N
    chip = lambda n: 0 < n <= BOOT_LDS_N
    pairs = [(a, b) for r in rows for a, b in zip(r, r[1:])]
    assert any(len(r) == 3 and chip(r[0]) and big(r[1]) and chip(r[2]) for r in rows)          # on-chip -> global -> on-chip
    assert any(big(a) and big(b) and b < a for a, b in pairs)                                  # global -> global with a smaller n
    assert any(a == 0 and chip(b) for a, b in pairs) and any(a == 0 and big(b) for a, b in pairs)      # non-empty right after empty
    assert any(big(a) and b == 1 for a, b in pairs) and any(a == BOOT_LDS_N and b == 1 for a, b in pairs)      # large n, then n = 1
    return sizes.tolist()


def _reuse_subset(sizes):
    """the groups compared at bs 10,000: every group of the planted workgroups 0 .. 15 (48 groups, every path change above)"""
    return sorted(w + r * BOOT_GRID for w in range(len(REUSE_PLANTED)) for r in range(3))


def _sub_input(bi, pick):
    from phaser_amd import cis_var
    return cis_var.BootInput(np.concatenate([bi.values[bi.off[g]:bi.off[g + 1]] for g in pick]),
                             np.concatenate([[0], np.cumsum([bi.off[g + 1] - bi.off[g] for g in pick])]), bi.subseq[pick], bi.seed, bi.bs)


@pytest.mark.gpu
def test_kboot_gpu_reused_workgroups_match_replay_bs41():
    """2,500 groups in one launch: every workgroup serves two or three groups and carries its LDS tables, its keys slice and its global
    histogram slice from one to the next.  Every group of the launch against the replay."""
    import time
    from phaser_amd import _lib, cis_var
    ctx = _lib.Context(0)
    rng = np.random.default_rng(21)
    sizes = _reuse_sizes(rng)
    vals, off = _groups(rng, sizes)
    bi = cis_var.BootInput(vals, off, rng.integers(0, 2 ** 40, len(sizes), dtype=np.uint64), int(rng.integers(0, 2 ** 63)), 41)
    got = cis_var.bootstrap_gpu(ctx.lib, ctx.h, bi, want_replicates=True)
    t0 = time.time()
    _assert_boot_equals_replay(got, bi, "bs 41")
    print("replay of %d groups (%d samples) at bs 41: %.1f s" % (len(sizes), int(off[-1]), time.time() - t0))


@pytest.mark.gpu
def test_kboot_gpu_reused_workgroups_match_replay_bs10000():
    """The same launch shape at the product's bs: 48 groups (the three of each planted workgroup) against the replay."""
    import time
    from phaser_amd import _lib, cis_var
    ctx = _lib.Context(0)
    rng = np.random.default_rng(22)
    sizes = _reuse_sizes(rng)
    vals, off = _groups(rng, sizes)
    bi = cis_var.BootInput(vals, off, rng.integers(0, 2 ** 40, len(sizes), dtype=np.uint64), int(rng.integers(0, 2 ** 63)), 10000)
    got_os, got_sc, got_reps = cis_var.bootstrap_gpu(ctx.lib, ctx.h, bi, want_replicates=True)
    pick = _reuse_subset(sizes)
    sub = _sub_input(bi, pick)
    t0 = time.time()
    _assert_boot_equals_replay((got_os[pick], got_sc[pick], got_reps[pick]), sub, "bs 10000")
    print("replay of %d groups (%d samples) at bs 10000: %.1f s" % (len(pick), int(sub.off[-1]), time.time() - t0))
    empty = np.diff(off) == 0                                     # every other group: the cheap invariants
    assert np.isnan(got_os[empty]).all() and not np.isnan(got_os[~empty]).any()
    assert np.all(got_sc.sum(axis=2) <= 10000) and np.all(got_sc[empty] == 0)
    assert np.all(got_os[~empty][:, :, 0] <= got_os[~empty][:, :, 3])


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[65535], [32768, 5, 65535, 32767]])
def test_kboot_gpu_16bit_limits_match_replay(sizes):
    from phaser_amd import _lib, cis_var
    ctx = _lib.Context(0)
    rng = np.random.default_rng(23 + len(sizes))
    vals, off = _groups(rng, sizes)
    bi = cis_var.BootInput(vals, off, rng.integers(0, 2 ** 40, len(sizes), dtype=np.uint64), int(rng.integers(0, 2 ** 63)), 3)
    _assert_boot_equals_replay(cis_var.bootstrap_gpu(ctx.lib, ctx.h, bi, want_replicates=True), bi, sizes)


@pytest.mark.gpu
def test_kboot_gpu_one_context_through_changing_reservations():
    """(max_n 5000, bs 500), (max_n 40, bs 41), (max_n 1500, bs 10001) on one context: the keys and histogram reservations and the
    [grid][2][bs] layout change from call to call."""
    from phaser_amd import _lib, cis_var
    ctx = _lib.Context(0)
    rng = np.random.default_rng(24)
    for bs, sizes in ((500, [5000, 70, 1025, 3]), (41, [40, 1, 17, 0, 40]), (10001, [1500, 8, 1030])):
        vals, off = _groups(rng, sizes)
        bi = cis_var.BootInput(vals, off, rng.integers(0, 2 ** 40, len(sizes), dtype=np.uint64), int(rng.integers(0, 2 ** 63)), bs)
        assert bi.max_n == sizes[0]
        _assert_boot_equals_replay(cis_var.bootstrap_gpu(ctx.lib, ctx.h, bi, want_replicates=True), bi, (bs, sizes))


def _bootstrap_device_space(ctx, bi, want_replicates):
    """phz_bootstrap_medians with every input and output as a device tensor (PHZ_DEVICE)"""
    import ctypes as C
    import torch
    from phaser_amd import _lib
    dev = torch.device("cuda", ctx.device)
    up = lambda a, dt: torch.from_numpy(a.view(dt)).to(dev)
    t = {"off": up(bi.off, np.int64), "subseq": up(bi.subseq, np.int64), "rank": up(bi.rank, np.int32), "vs": up(bi.sorted_s, np.float64),
         "va": up(bi.sorted_a, np.float64)}
    G = bi.n_groups
    os_ = torch.full((G, 2, 4), -5.0, dtype=torch.float64, device=dev); sc = torch.full((G, 2, 2), -5, dtype=torch.int64, device=dev)
    reps = torch.full((G, 2, bi.bs), -5.0, dtype=torch.float64, device=dev) if want_replicates else None
    s = bi.struct()
    p = lambda x: C.c_void_p(x.data_ptr())
    s.off = p(t["off"]); s.subseq = p(t["subseq"]); s.rank = p(t["rank"]); s.sorted_s = p(t["vs"]); s.sorted_a = p(t["va"])
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.phz_bootstrap_medians(ctx.h, C.byref(s), p(os_), p(sc), p(reps) if want_replicates else None, _lib.PHZ_DEVICE))
    return os_.cpu().numpy(), sc.cpu().numpy(), (reps.cpu().numpy() if want_replicates else None)


@pytest.mark.gpu
@pytest.mark.parametrize("want_replicates", [True, False])
def test_kboot_gpu_device_space_equals_host_space_and_replay(want_replicates):
    from phaser_amd import _lib, cis_var
    ctx = _lib.Context(0)
    rng = np.random.default_rng(25)
    sizes = [7, 0, 1024, 1025, 1, 300, 2000, 64, 0, 1500, 2]
    vals, off = _groups(rng, sizes)
    bi = cis_var.BootInput(vals, off, rng.integers(0, 2 ** 40, len(sizes), dtype=np.uint64), int(rng.integers(0, 2 ** 63)), 200)
    host = cis_var.bootstrap_gpu(ctx.lib, ctx.h, bi, want_replicates=want_replicates)
    dev = _bootstrap_device_space(ctx, bi, want_replicates)
    assert _same(dev[0], host[0]) and np.array_equal(dev[1], host[1])
    if want_replicates:
        live = np.diff(off) > 0                                   # the replicates of an empty group are not written
        assert _same(dev[2][live], host[2][live])
    _assert_boot_equals_replay(dev, bi, "PHZ_DEVICE", reps=want_replicates)


@pytest.mark.gpu
@pytest.mark.parametrize("matrix,tbi", [("bgzf", True), ("plain", False)])
def test_cis_var_gpu_matches_restatement(tmp_path, matrix, tbi):
    pytest.importorskip("pandas"); pytest.importorskip("scipy")
    from phaser_amd import cis_var
    fx = make_fixture(str(tmp_path), matrix=matrix, tbi=tbi)
    want = restate_reference(fx["bed_text"], fx["vcf_text"], fx["pairs_text"], fx["map_text"], bs=500, seed=3)
    got = cis_var.cis_var(cis_var.read_text(fx["bed"]), fx["vcf"], fx["pairs_text"], fx["map_text"], bs=500, seed=3)
    assert_same_table(got, want)


@pytest.mark.gpu
def test_cis_var_gpu_gtex_shaped_is_deterministic(tmp_path):
    """2,000 pairs x 670 samples at bs 10,000: 64 random groups equal the replay, launched on their own and as part of the launch of all
    4,000 groups; two CLI runs and --t 1 / --t 16 give the same bytes."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import cis_var_scale
    from phaser_amd import _lib, cis_var
    paths = cis_var_scale.make_inputs(str(tmp_path), seed=7, n_pairs=2000, n_samples=670, n_records=12000, n_genes=2500)
    outs = []
    for t in (1, 16, 16):
        o = os.path.join(str(tmp_path), "out_%d_%d.txt" % (t, len(outs)))
        r = subprocess.run([sys.executable, "-m", "phaser_amd.cis_var", "--bed", paths["bed"], "--vcf", paths["vcf"], "--pairs", paths["pairs"],
                            "--map", paths["map"], "--o", o, "--t", str(t), "--seed", "11"], cwd=REPO, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(open(o, "rb").read())
    assert outs[0] == outs[1] == outs[2]
    # 64 random groups of that run against the replay
    captured = {}

    def capture(bi):
        captured["bi"] = bi
        return np.full((bi.n_groups, 2, 4), np.nan), np.zeros((bi.n_groups, 2, 2), np.int64)
    cis_var.cis_var(cis_var.read_text(paths["bed"]), paths["vcf"], open(paths["pairs"]).read(), open(paths["map"]).read(), seed=11, _bootstrap=capture)
    bi = captured["bi"]
    rng = np.random.default_rng(1)
    pick = np.sort(rng.choice(bi.n_groups, size=min(64, bi.n_groups), replace=False))
    sub = cis_var.BootInput(np.concatenate([bi.values[bi.off[g]:bi.off[g + 1]] for g in pick]),
                            np.concatenate([[0], np.cumsum([bi.off[g + 1] - bi.off[g] for g in pick])]), bi.subseq[pick], bi.seed, bi.bs)
    ctx = _lib.Context(0)
    got_os, got_sc, _ = cis_var.bootstrap_gpu(ctx.lib, ctx.h, sub)
    want_os, want_sc, _ = replay_bootstrap(sub)
    assert _same(got_os, want_os) and np.array_equal(got_sc, want_sc)
    # ... and the same 64 groups taken from the launch of the whole run, the one in which a workgroup serves several groups in a row
    assert bi.n_groups > 2 * BOOT_GRID
    full_os, full_sc, _ = cis_var.bootstrap_gpu(ctx.lib, ctx.h, bi, want_replicates=False)
    assert _same(full_os[pick], want_os) and np.array_equal(full_sc[pick], want_sc)


# ------------------------------------------------------------------------------------------------ VCF lookup: index path = whole-file scan = an independent reader
def _lookup_vcf(tmp, seed, n_rec=3000, n_samples=40):
    from phaser_amd import vcfout
    rng = np.random.default_rng(seed)
    samples = ["s%d" % i for i in range(n_samples)]
    lines = ["##fileformat=VCFv4.2", "#" + "\t".join(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples)]
    keys = []
    for c in ("1", "2", "X"):
        pos = np.cumsum(rng.integers(1, 9000, n_rec)) + 1
        for k, p in enumerate(pos.tolist()):
            g = ["%s|%s:%d" % (rng.integers(0, 2), rng.integers(0, 2), rng.integers(0, 50)) for _ in samples]
            lines.append("\t".join([c, str(p), "id%s_%d" % (c, k), "ACGT"[k % 4], "G", ".", "PASS", ".", "GT:DP"] + g))
            if k % 41 == 3:                                   # a second record at the position
                lines.append("\t".join([c, str(p), "id%s_%db" % (c, k), "A", "T", ".", "PASS", ".", "DP:GT"] + ["9:1|0"] * n_samples))
            keys.append((c, p))
    path = os.path.join(tmp, "q.vcf.gz")
    assert vcfout.write_bgzf(path, "\n".join(lines) + "\n", 4, index="vcf")
    q = [keys[int(i)] for i in rng.integers(0, len(keys), 400)] + [(c, p + 1) for c, p in keys[:30:3]] + [("7", 100), ("1", 1)]
    return path, sorted(set(q)), samples


@pytest.mark.parametrize("seed", [1, 2])
def test_vcf_lookup_index_equals_scan_equals_independent_reader(tmp_path, seed):
    from phaser_amd import _lib, cis_var
    from test_tabix import Tbi, _vcf_span
    _lib.build()
    path, q, samples = _lookup_vcf(str(tmp_path), seed)
    assert os.path.exists(path + ".tbi")
    pick = samples[::3] + ["absent"]
    by_index, contigs_i = cis_var.vcf_records(path, q, pick, threads=4, use_index=True)
    by_scan, contigs_s = cis_var.vcf_records(path, q, pick, threads=3, use_index=False)
    assert by_index == by_scan and sum(len(v) for v in by_index.values()) > 300
    assert contigs_i == contigs_s == {"1", "2", "X"}
    t = Tbi(path)
    cols = [l for l in t.text.decode().split("\n") if l.startswith("#CHROM")][0].lstrip("#").split("\t")
    for c, p in q:
        want = []
        if c.encode() in t.names:
            want = [l for l in t.query(c, p - 1, p, _vcf_span) if int(l.split("\t")[1]) == p]
        got = by_index.get((c, p), [])
        assert sorted(r[2] for r in got) == sorted(l.split("\t")[2] for l in want), (c, p)
        for r in got:                                     # the GT subfields of the named samples
            line = [l for l in want if l.split("\t")[2] == r[2]][0].split("\t")
            gi = line[8].split(":").index("GT")
            assert r[5] == str(gi)
            assert r[6:] == [line[cols.index(s)].split(":")[gi] for s in samples[::3]] + ["\x01"]


def test_cis_var_contig_absent_from_vcf_gives_no_row_and_a_log_line(tmp_path):
    from phaser_amd import _lib, cis_var
    _lib.build()
    fx = make_fixture(str(tmp_path), tbi=True)
    gene = fx["bed_text"].split("\n")[1].split("\t")[3]
    pairs = fx["pairs_text"] + "\t".join([gene, "rsZ", "chr9", "1200", "A", "G"]) + "\n"
    logs = []
    got = cis_var.cis_var(fx["bed_text"], fx["vcf"], pairs, fx["map_text"], bs=16, log=logs.append, _bootstrap=_replay_hook)
    base = cis_var.cis_var(fx["bed_text"], fx["vcf"], fx["pairs_text"], fx["map_text"], bs=16, _bootstrap=_replay_hook)
    assert got == base and "chr9" not in got
    assert any("1 pair(s) name a contig that the VCF does not hold" in l for l in logs)


def test_cis_var_on_reference_written_expression_matrix(tmp_path):
    """the population flow: tests/golden/expr_matrix's gw_phased matrix (written by the reference's phaser_expr_matrix) + a generated
    phased VCF -> cis_var, against the restatement"""
    pytest.importorskip("pandas"); pytest.importorskip("scipy")
    from conftest import GOLD
    from phaser_amd import _lib, cis_var, vcfout
    _lib.build()
    mpath = os.path.join(GOLD, "expr_matrix", "out.sorted.gw_phased.bed.gz")
    bed_text = cis_var.read_text(mpath)
    head = bed_text.split("\n")[0].split("\t")
    rows = [l.split("\t") for l in bed_text.split("\n")[1:] if l]
    bed_samples = head[4:]
    rng = np.random.default_rng(8)
    vcf_samples = ["V_" + s for s in bed_samples]
    lines = ["##fileformat=VCFv4.2", "#" + "\t".join(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + vcf_samples)]
    pairs = ["gene_id\tvar_id\tvar_contig\tvar_pos\tvar_ref\tvar_alt"]
    recs = []
    for k, r in enumerate(rows):
        p = int(r[1]) + 10 + k
        recs.append((r[0], p, "rs%d" % k))
    recs.sort(key=lambda x: (x[0], x[1]))
    for c, p, i in recs:
        g = [["0|1", "1|0", "0|0", "1|1", "0/1"][int(rng.integers(0, 5))] for _ in vcf_samples]
        lines.append("\t".join([c, str(p), i, "A", "G", ".", "PASS", ".", "GT:AD"] + [x + ":3,4" for x in g]))
    for k, (c, p, i) in enumerate(recs):
        pairs.append("\t".join([rows[int(rng.integers(0, len(rows)))][3], i, c, str(p), "A", "G"]))
    vpath = os.path.join(str(tmp_path), "v.vcf.gz")
    vcf_text = "\n".join(lines) + "\n"
    vcfout.write_bgzf(vpath, vcf_text, 2, index="vcf")
    map_text = "vcf_sample\tbed_sample\n" + "".join("%s\t%s\n" % (v, b) for v, b in zip(vcf_samples, bed_samples))
    pairs_text = "\n".join(pairs) + "\n"
    for kw in (dict(min_cov=8), dict(min_cov=0, pc=1)):
        want = restate_reference(bed_text, vcf_text, pairs_text, map_text, bs=40, seed=2, **kw)
        got = cis_var.cis_var(bed_text, vpath, pairs_text, map_text, bs=40, seed=2, _bootstrap=_replay_hook, **kw)
        assert got.count("\n") == len(recs) + 1
        assert_same_table(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [7, 8, 31])
def test_kboot_gpu_medians_distribution_matches_numpy_choice(n):
    """Two-sample KS of 200k replicate medians returned by the product kernel vs numpy.random.choice (seeded), alpha = 0.01."""
    from phaser_amd import _lib, cis_var
    ctx = _lib.Context(0)
    rng = np.random.default_rng(n)
    v = np.round(rng.normal(size=n), 1)
    B = 200_000
    bi = cis_var.BootInput(v, np.array([0, n], dtype=np.int64), np.array([(5 << 16) + 1], dtype=np.uint64), 11, B)
    ours = cis_var.bootstrap_gpu(ctx.lib, ctx.h, bi, want_replicates=True)[2][0, 0]
    theirs = np.median(v[np.random.default_rng(12).integers(0, n, (B, n))], axis=1)
    grid = np.union1d(ours, theirs)
    d = np.max(np.abs(np.searchsorted(np.sort(ours), grid, side="right") / B - np.searchsorted(np.sort(theirs), grid, side="right") / B))
    assert d < 1.628 * math.sqrt(2.0 / B), d
