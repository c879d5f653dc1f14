"""k_edge_local / k_phase_pair / k_phase_general (phz_rowsdev.hip, entry point phz_phase_components) at their limits: the designed
components of tests/phase_inputs.py, under the host-side emulation and on the product build on an MI355X, against the native host
routine phz_phase_block.  Every comparison is exact (n_sub, sub_of, and alle_of wherever sub_of >= 0); there is no tolerance anywhere.

Three tiers.  oracle/phasing_oracle.py (the Python restatement of phase_v3) pins phz_phase_block here on every designed case whose
longest fragment that needs the search over configurations (a fragment no flood fill settles) has at most ORACLE_MAX_SEARCH = 14
variants and whose component has at most ORACLE_MAX_N variants: the restatement scores 2^len strings pair by pair and took, on one core,
0.10 s at 12 variants, 0.23 s at 13, 0.54 s at 14 and 1.5 s at 15, so 14 is the last length that stays under a second; its split is a
Python loop over positions x pairs, about two seconds for each of the three 256-variant cases around 2,048 pairs (they are run) and minutes
at 4,100 variants (that one case is not).  Longer cases rest on phz_phase_block alone, which searches by plain brute force with no dynamic
programme and so is independent of the device's shortcut.  phz_phase_block in turn pins the kernels.

Before any kernel runs, the test_*_designs_hold_what_they_promise tests, one per family of cases, check against the host routine and the
restatement's own split that every case is what its name says: size (counted from the pairs, and against the sizes written out in
NAMED_SIZES), pair count, spans, a failing whole-component flood, one fragment or the intended cuts, fragments that their own flood settles,
the intended refusal; each asserts that the branches its family was designed for are reached, and prints its rows of the table
name, n, E, D, blocks (-s).  The emulated test runs the 22-variant brute-force cases too (2^21 configurations each: under half a second per case).

The two refusals are batches of their own: a component that cannot be split to max_block_size (the device's own verdict, counters[2])
and a fragment of 31 variants (handed to the host inside the call, refused by best_free); phz_phase_components returns
PHZ_E_UNSUPPORTED for both, as phz_phase_block does."""
import ctypes as C
import functools

import numpy as np
import pytest

import phase_inputs as pi
from helpers import EmuContext, emu_library
from test_emu_phase import SEED_LISTS, assert_list_matches, batch_phase, random_list
from test_phase_block import _native_phase, _oracle_inputs, _oracle_phase

ORACLE_MAX_SEARCH = 14
ORACLE_MAX_N = 300                       # the restatement's split is a Python loop over positions x pairs: minutes at 4,100 variants
PHZ_E_UNSUPPORTED = -4


@functools.lru_cache(maxsize=None)
def product_lib():
    from phaser_amd import _lib
    return _lib.load()


def host_run(case):
    """phz_phase_block of the product library -> (status, sub_of, alle_of, n_sub)"""
    lib = product_lib()
    n, edges = case.n, case.edges
    ei = np.asarray([e[0] for e in edges], dtype=np.int32); ej = np.asarray([e[1] for e in edges], dtype=np.int32)
    ek = np.asarray([e[2] for e in edges], dtype=np.int8)
    first = np.zeros(n + 1, dtype=np.int32); ln = np.zeros(n + 1, dtype=np.int32); cfg = np.zeros(n + 1, dtype=np.uint8); ns = C.c_int32(0)
    st = lib.phz_phase_block(n, len(edges), ei.ctypes.data, ej.ctypes.data, ek.ctypes.data, case.mbs, first.ctypes.data, ln.ctypes.data, cfg.ctypes.data, C.byref(ns))
    if st != 0:
        return st, None, None, 0
    sub = np.full(n, -1, dtype=np.int16); al = np.zeros(n, dtype=np.uint8)
    w = 0; k2 = 0
    for k in range(ns.value):
        if ln[k] <= 0:
            continue
        for t in range(int(ln[k])):
            sub[first[k] + t] = k2; al[first[k] + t] = 1 if cfg[w] == ord("1") else 0; w += 1
        k2 += 1
    sub.setflags(write=False); al.setflags(write=False)
    return st, sub, al, k2


@functools.lru_cache(maxsize=None)
def reference():
    """name -> (status, sub_of, alle_of, n_sub) of the host routine for every designed case and shape: computed once, read-only"""
    return {c.name: host_run(c) for c in pi.accepted_cases() + pi.refused_cases() + pi.many_shapes()}


def flood_reaches(n, edges, lo=0, hi=None):
    """allele nodes in the component of (variant lo, allele 0) over the pairs inside [lo, hi): resolve_phase accepts the whole component
    (a fragment) iff this equals n (hi - lo)"""
    hi = n if hi is None else hi
    edges = [e for e in edges if lo <= min(e[0], e[1]) and max(e[0], e[1]) < hi]
    parent = list(range(2 * n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]; x = parent[x]
        return x
    for i, j, k in edges:
        if k >= 0:
            for a in (0, 1):
                parent[find(2 * i + a)] = find(2 * j + (a ^ k))
    return sum(find(x) == find(2 * lo) for x in range(2 * n))


@functools.lru_cache(maxsize=None)
def oracle_split(name):
    """the restatement's own split of an accepted case whose flood fails -> (fragment bounds, longest fragment left to the search)"""
    case = {c.name: c for c in pi.accepted_cases()}[name]
    ph, names, vc, ac = _oracle_inputs(case.n, case.edges, case.mbs)
    frags = ph.weak_split(names, vc, case.n if case.mbs == 0 else case.mbs)
    bounds = [0]; search = 0
    for f in frags:
        bounds.append(bounds[-1] + len(f))
        if len(frags) == 1 or ph.component_of_first(f, ac, True) is None:
            search = max(search, len(f))
    return tuple(bounds), search


def needs_search(case):
    """longest fragment the restatement would search configuration by configuration (0: a flood settles everything)"""
    if flood_reaches(case.n, case.edges) == case.n:
        return 0
    return oracle_split(case.name)[1]


# ------------------------------------------------------------------------------------------------ the case list
# Sizes the issue names, written out here and not taken from the generator: name (or its start) -> (variants, pairs or None)
SPLIT_SIZES = ((63, 61), (64, 62), (65, 63), (128, 63), (128, 65), (129, 127), (200, 64), (200, 128), (255, 127), (255, 191), (256, 192), (256, 254))
NAMED_SIZES = {"table_n256_E2047": (256, 2047), "table_n256_E2048": (256, 2048), "table_n256_E2049": (256, 2049), "table_n257_mbs15_break192": (257, None),
               "table_n4100_mbs15_break2050": (4100, None), "host_len23_D11_unique_mbs": (23, None), "host_len31_D11_unique_mbs": (31, None),
               "split_n100_mbs0_fragments_40_36_24": (100, None), "split_n100_mbs0_clean_fragments_40_36_24": (100, None),
               "split_n100_mbs0_clean_fragments_33_32_35": (100, None), "pair_two_variants_cfg0": (2, 1), "pair_two_variants_cfg1": (2, 1),
               "pair_two_variants_cfgm1": (2, 1), "pair_tree_17_variants_16_pairs": (17, 16), "pair_tree_18_variants_17_pairs": (18, 17),
               "pair_9_variants_16_pairs_conflict": (9, 16), "refuse_split_n6_mbs1": (6, None)}
NAMED_SIZES.update({"split_n%d_mbs%d_break%d" % (n, mbs, brk): (n, None) for mbs in (15, 8) for n, brk in SPLIT_SIZES})
for _n in (8, 15, 22):
    NAMED_SIZES.update({"dp_len%d_D%d_" % (_n, D): (_n, None) for D in (0, 1, 5, 6, 7, 10) if D < _n})
NAMED_SIZES.update({"brute_len%d_D%d_" % nd: (nd[0], None) for nd in ((3, 2), (3, 0), (7, 3), (7, 6), (7, 5), (12, 11), (18, 11), (18, 17), (22, 11), (22, 21))})
NAMED_SIZES["dp_len12_D10_"] = (12, None)


def check_row(c):
    """what every case promises: its size (counted from the pairs themselves), pair count, largest span, whether the whole-component flood
    fails, acceptance by the host routine.  Prints the case's row of the table -> (n_sub, sub_of, blocks as (first, length)), None if refused"""
    st, sub, al, ns = reference()[c.name]
    lo = [min(i, j) for i, j, k in c.edges]; hi = [max(i, j) for i, j, k in c.edges]
    assert all(a < b and k in (0, 1, -1) for a, b, (i, j, k) in zip(lo, hi, c.edges)), c.name
    assert (len(set(lo) | set(hi)), min(lo), max(hi)) == (c.n, 0, c.n - 1), c.name            # a connected component: every variant is in some pair
    assert (len(c.edges), len(set(zip(lo, hi))), max(b - a for a, b in zip(lo, hi))) == (c.E, c.E, c.span), c.name
    named = [size for key, size in NAMED_SIZES.items() if c.name == key or (key.endswith("_") or key.endswith("_mbs")) and c.name.startswith(key)]
    assert len(named) <= 1 and all(c.n == n and E in (None, c.E) for n, E in named), (c.name, named)
    assert (flood_reaches(c.n, c.edges) != c.n) == c.flood_fails, c.name
    D = c.D if c.D is not None else "-"
    if c.refused:
        assert st == PHZ_E_UNSUPPORTED, c.name
        print("%-44s %5d %6d %4s refused (%s)" % (c.name, c.n, c.E, D, c.refused))
        return None
    assert st == 0, (c.name, st)                                    # every other case is accepted by the host routine
    blocks = [(int(np.flatnonzero(sub == b)[0]), int((sub == b).sum())) for b in range(ns)]
    print("%-44s %5d %6d %4s %s" % (c.name, c.n, c.E, D, " ".join("%d+%d" % b for b in blocks[:6]) + (" ..." if ns > 6 else "") if ns else "none"))
    return ns, sub, blocks


def check_host_path(c, reached):
    if c.host_path:
        assert c.n > pi.PH_NMAX or c.E > pi.PH_EMAX or c.name.startswith(("host_", "split_n100_mbs0_fragments")), c.name
        reached.add("host_path_" + ("n" if c.n > pi.PH_NMAX else "E" if c.E > pi.PH_EMAX else "fragment"))
    else:
        assert c.n <= pi.PH_NMAX and c.E <= pi.PH_EMAX, c.name


@functools.lru_cache(maxsize=None)
def survey_single():
    """one fragment of n variants whose farthest verdict spans D -> the branches reached"""
    reached = set()
    print("\n%-44s %5s %6s %4s %s" % ("name", "n", "E", "D", "blocks"))
    for c in pi.single_cases() + (pi.fragment_of_31(),):
        assert max([abs(i - j) for i, j, k in c.edges if k >= 0], default=0) == c.D, c.name
        assert c.mbs == 0 or c.mbs >= c.n
        want = "host" if c.n > pi.PH_BRUTE_MAX else ("dp" if c.n >= pi.PH_DP_MINLEN and c.D <= pi.PH_DP_MAXD else "brute")
        assert c.search == want and c.name.startswith("%s_len%d_D%d_" % (want, c.n, c.D)), c.name
        row = check_row(c)
        if row is None:
            assert c.refused == "fragment" and c.n > pi.BEST_FREE_MAX, c.name
            reached.add("refused_fragment")
            continue
        ns, sub, blocks = row
        one = ns == 1 and bool((sub == 0).all()); none = ns == 0 and bool((sub == -1).all())
        assert {"one": one, "none": none, "either": one or none}[c.blocks], (c.name, blocks)
        if c.n > 3:
            assert oracle_split(c.name)[0] == (0, c.n), c.name      # left as one fragment
        reached.add("%s_len%d_D%d_%s" % (c.search, c.n, c.D, "one" if one else "none"))
        check_host_path(c, reached)
    return frozenset(reached)


@functools.lru_cache(maxsize=None)
def survey_pair():
    reached = set()
    for c in pi.pair_cases():
        ns, sub, blocks = check_row(c)
        assert c.blocks is not None and c.D is None and not c.cuts
        one = ns == 1 and bool((sub == 0).all())
        assert {"one": one, "none": ns == 0, "either": True}[c.blocks], (c.name, blocks)
        check_host_path(c, reached)
        reached.add(c.name)
    by = {c.name: c for c in pi.pair_cases()}
    assert all(k == 1 for i, j, k in by["pair_clean_all_opposite"].edges) and not by["pair_clean_all_opposite"].flood_fails
    assert not by["pair_tree_17_variants_16_pairs"].flood_fails and not by["pair_tree_18_variants_17_pairs"].flood_fails
    assert by["pair_9_variants_16_pairs_conflict"].flood_fails
    return frozenset(reached)


def check_cuts(c, reached):
    """the restatement's own split holds the intended cuts and none of the blocked positions; the host's first block ends at the intended break"""
    ns, sub, blocks = check_row(c)
    if c.n <= ORACLE_MAX_N:
        bounds = oracle_split(c.name)[0]
        assert set(c.cuts) <= set(bounds) and not set(c.blocked) & set(bounds), (c.name, bounds)
        if c.blocked:                                               # the levels above 1 were visited: some cut is not a level-1 position
            assert set(bounds) - set(c.cuts) - {0, c.n}, c.name
        if c.mbs == 0:
            assert bounds == (0,) + c.cuts + (c.n,), c.name
        for b in c.blocked:
            reached.add("blocked_%d_by_%s" % (b, "left" if b - 1 in c.cuts else "right"))
        reached.update("cut_%d" % p for p in c.cuts)
        if c.clean_fragments:                                       # every fragment settled by its own flood: nothing for the host, nothing for the search
            assert not c.host_path and c.mbs == 0 and bool((sub >= 0).all()), (c.name, blocks)
            for lo, hi in zip(bounds, bounds[1:]):
                assert flood_reaches(c.n, c.edges, lo, hi) == hi - lo, (c.name, lo, hi)
                reached.add("%s_flood_len%d" % ("lds" if hi - lo > 32 else "mask", hi - lo))
    if c.first_break is not None:                                   # the host's first block is [0, first_break): a block boundary at the intended cut
        assert blocks and blocks[0] == (0, c.first_break), (c.name, blocks[:3])
        reached.add("break_%d_mbs%d" % (c.first_break, c.mbs))
    check_host_path(c, reached)


@functools.lru_cache(maxsize=None)
def survey_split():
    reached = set()
    for c in pi.split_cases():
        assert c.cuts and c.D is None and c.flood_fails, c.name
        check_cuts(c, reached)
    return frozenset(reached)


@functools.lru_cache(maxsize=None)
def survey_table():
    reached = set()
    for c in pi.table_cases():
        assert c.host_path == (c.n > pi.PH_NMAX or c.E > pi.PH_EMAX) and c.flood_fails, c.name
        check_cuts(c, reached)
        reached.add(c.name)
    return frozenset(reached)


def test_single_fragment_designs_hold_what_they_promise():
    reached = survey_single()
    want = {"refused_fragment", "host_path_fragment"}
    for n in (8, 15, 22):
        want |= {"dp_len%d_D0_none" % n, "dp_len%d_D1_none" % n}
        for D in (5, 6, 7, 10):
            if D < n:
                want |= {"dp_len%d_D%d_one" % (n, D), "dp_len%d_D%d_none" % (n, D)}
    want |= {"brute_len3_D2_none", "brute_len3_D0_none", "brute_len7_D3_one", "brute_len7_D3_none", "brute_len7_D6_one", "brute_len7_D6_none"}
    want |= {"brute_len7_D5_one", "dp_len8_D5_one", "dp_len12_D10_one", "brute_len12_D11_one", "brute_len22_D11_one", "host_len23_D11_one"}
    for n, D in ((12, 11), (18, 11), (18, 17), (22, 11), (22, 21)):
        want |= {"brute_len%d_D%d_one" % (n, D), "brute_len%d_D%d_none" % (n, D)}
    assert want <= reached, sorted(want - reached)
    assert sum(c.search == "brute" and c.n >= 20 for c in pi.single_cases()) <= 10


def test_pair_kernel_designs_hold_what_they_promise():
    assert {"pair_two_variants_cfg0", "pair_two_variants_cfg1", "pair_two_variants_cfgm1", "pair_tree_17_variants_16_pairs", "pair_tree_18_variants_17_pairs",
            "pair_9_variants_16_pairs_conflict", "pair_clean_all_opposite"} <= survey_pair()


def test_split_designs_hold_what_they_promise():
    reached = survey_split()
    want = {"break_%d_mbs%d" % (b, mbs) for mbs in (15, 8) for b in (61, 62, 63, 64, 65, 127, 128, 191, 192, 254)}
    want |= {"blocked_64_by_left", "blocked_128_by_left", "blocked_192_by_left", "blocked_63_by_right", "blocked_64_by_right", "blocked_127_by_right", "blocked_191_by_right"}
    want |= {"cut_40", "cut_76", "cut_33", "cut_65", "host_path_fragment"}
    want |= {"lds_flood_len40", "lds_flood_len36", "lds_flood_len33", "lds_flood_len35", "mask_flood_len32", "mask_flood_len24"}
    assert want <= reached, sorted(want - reached)
    assert {"split_n%d_mbs%d_break%d" % (n, mbs, brk) for mbs in (15, 8) for n, brk in SPLIT_SIZES} <= {c.name for c in pi.split_cases()}


def test_table_limit_designs_hold_what_they_promise():
    want = {"table_n256_E2047", "table_n256_E2048", "table_n256_E2049", "table_n257_mbs15_break192", "table_n4100_mbs15_break2050", "host_path_n", "host_path_E"}
    assert want <= survey_table(), sorted(want - survey_table())


def test_refusal_and_many_component_designs_hold_what_they_promise():
    c = pi.unsplittable()
    assert check_row(c) is None and c.refused == "split" and (c.n, c.mbs) == (6, 1)
    # the 20,000-component list: more than the grid's first batches, every shape complex (no shape is settled by k_phase_pair's flood)
    shapes = pi.many_shapes(); order = pi.many_order()
    assert len(order) == pi.N_MANY > pi.PH_GRID * pi.PH_BATCH and set(order) == set(range(len(shapes))) and len(shapes) == 50
    for s in shapes:
        assert check_row(s) is not None and 3 <= s.n <= 6 and s.flood_fails, s.name


def test_case_names_are_distinct():
    cases = pi.accepted_cases() + pi.refused_cases() + pi.many_shapes()
    assert len({c.name for c in cases}) == len(cases)


@pytest.mark.parametrize("group", ["single", "pair", "split", "table"])
def test_host_routine_matches_the_restatement_on_designed_cases(group):
    """long-range pairs, thinned splits, the pair kernel's shapes: phz_phase_block against oracle/phasing_oracle.py"""
    cases = {"single": pi.single_cases(), "pair": pi.pair_cases(), "split": pi.split_cases(), "table": pi.table_cases()}[group]
    ran = 0
    for c in cases:
        if c.n > ORACLE_MAX_N or needs_search(c) > ORACLE_MAX_SEARCH:
            continue
        want = _oracle_phase(c.n, c.edges, c.mbs)                    # a case that makes the restatement raise is a badly designed case
        got = [b for b in _native_phase(product_lib(), c.n, c.edges, c.mbs) if b]
        assert got == want, c.name
        ran += 1
    assert ran >= {"single": 20, "pair": 7, "split": 14, "table": 4}[group], ran


# ------------------------------------------------------------------------------------------------ the kernels
def case_lists(reverse):
    """{max_block_size: (components, host results)} over every accepted case"""
    ref = reference()
    out = {}
    for mbs, cases in sorted(pi.lists_by_block_size().items()):
        cases = cases[::-1] if reverse else cases
        out[mbs] = ([(c.n, list(c.edges)) for c in cases], [ref[c.name][1:] for c in cases], [c.name for c in cases])
    return out


def phase_raw(ctx, comps, mbs):
    """phz_phase_components without the status check -> (status, last error text)"""
    cs = np.zeros(len(comps) + 1, dtype=np.uint32); es = np.zeros(len(comps) + 1, dtype=np.uint32)
    for c, (n, edges) in enumerate(comps):
        cs[c + 1] = cs[c] + n; es[c + 1] = es[c] + len(edges)
    pi_ = np.asarray([e[0] for n, ed in comps for e in ed], dtype=np.int32); pj = np.asarray([e[1] for n, ed in comps for e in ed], dtype=np.int32)
    pk = np.asarray([e[2] for n, ed in comps for e in ed], dtype=np.int8)
    sub = np.zeros(int(cs[-1]), dtype=np.int32); al = np.zeros(int(cs[-1]), dtype=np.uint8); ns = np.zeros(len(comps), dtype=np.uint32)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    st = ctx.lib.phz_phase_components(ctx.h, len(comps), vp(cs), vp(es), vp(pi_), vp(pj), vp(pk), mbs, vp(sub), vp(al), vp(ns))
    return st, (ctx.lib.phz_last_error(ctx.h) or b"").decode()


def check_designed_lists(ctx, orders=(False, True)):
    """every accepted case, one call per max_block_size, in the list's order and in reverse (other cstart / estart offsets, other neighbours in the ticket order)"""
    bad = []
    for reverse in orders:
        for mbs, (comps, want, names) in case_lists(reverse).items():
            cs, sub, al, ns = batch_phase(ctx, comps, mbs)
            for c, (name, (wsub, wal, wns)) in enumerate(zip(names, want)):
                lo, hi = int(cs[c]), int(cs[c + 1])
                live = wsub >= 0
                if int(ns[c]) != wns or not np.array_equal(sub[lo:hi], wsub) or not np.array_equal(al[lo:hi][live], wal[live]):
                    bad.append(name + (" (reverse order)" if reverse else ""))
    assert not bad, "differ from phz_phase_block: %s" % bad


def check_refusals(ctx):
    """each refusal in a batch of its own: PHZ_E_UNSUPPORTED, the message names the cause, and the context goes on working"""
    ref = reference()
    normal = [c for c in pi.pair_cases() + pi.single_cases()[:12]]
    for case, text in ((pi.unsplittable(), "cannot be split"), (pi.fragment_of_31(), "on the host")):
        assert ref[case.name][0] == PHZ_E_UNSUPPORTED
        st, msg = phase_raw(ctx, [(case.n, list(case.edges))], case.mbs)
        assert st == PHZ_E_UNSUPPORTED and text in msg, (case.name, st, msg)
        for mbs in (15, 0):
            sel = [c for c in normal if c.mbs == mbs]
            assert len(sel) >= 5
            assert_list_matches(ctx, [(c.n, list(c.edges)) for c in sel], [ref[c.name][1:] for c in sel], mbs)


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_emulated_kernels_match_host_routine_on_designed_cases(order):
    check_designed_lists(EmuContext(emu_library()), orders=(order == "reverse",))


def test_emulated_kernels_refuse_what_the_host_routine_refuses():
    check_refusals(EmuContext(emu_library()))


@pytest.fixture(scope="module")
def gpu_ctx():
    from phaser_amd import _lib
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_product_kernels_match_host_routine_on_designed_cases(gpu_ctx):
    check_designed_lists(gpu_ctx)


@pytest.mark.gpu
def test_product_kernels_take_further_ticket_batches_and_reset_them(gpu_ctx):
    """20,000 complex components on a grid of 4,096 waves taking 4 tickets at a time; twice on one context (ticket word and counters start from zero
    again).  The second call takes the list in reverse: should it get the first call's buffers back and its waves find the tickets used up, what is
    left in those buffers is the first call's answer, which differs from the reversed list's almost everywhere."""
    ref = reference()
    shapes = pi.many_shapes()
    order = pi.many_order()
    assert sum(shapes[a].n != shapes[b].n for a, b in zip(order, order[::-1])) > pi.N_MANY // 2
    for order in (order, order[::-1]):
        assert_list_matches(gpu_ctx, [(shapes[s].n, list(shapes[s].edges)) for s in order], [ref[shapes[s].name][1:] for s in order], 15)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,mbs", SEED_LISTS)
def test_product_kernels_match_host_routine_on_random_components(gpu_ctx, seed, mbs):
    comps, want = random_list(product_lib(), seed, mbs)
    split = assert_list_matches(gpu_ctx, comps, want, mbs)
    assert len(comps) > 100 and split > 10


@pytest.mark.gpu
def test_product_kernels_refuse_what_the_host_routine_refuses(gpu_ctx):
    check_refusals(gpu_ctx)
