"""Designed inputs for K_genes (k_gene_items / phz_gene_counts, phaser_amd/csrc/phz_genes.hip) and a reference that shares nothing with it.

A *run* is what one haplotypic_counts row holds for one haplotype: for each variant, in the row's order, a position and the list of read
labels (strings) seen at it.  A *pair* is (run, feature); the wanted number is how many different labels the variants inside the feature
carry -- `expected_counts`, a set union over the label lists, which never looks at lab_prev (variant_feature_reads of the reference's
script: the test of its line 194, the set of its lines 204-217).

`encode` turns a Case into the arrays phz_gene_work points at: lab_pos / lab_prev from the label lists with a dictionary, the way
phz_hc_parse writes them, and one (lo, n, run, pair, hap) item for every piece a run is cut into.  Plain Python and numpy; no GPU, no ctypes.
"""
import numpy as np


def expected_counts(feature, run):
    """distinct labels of the run's variants with fb <= pos - 1 <= fe (the feature's end is inclusive)"""
    fb, fe = feature
    return len(set().union(*[labels for pos, labels in run if fb <= pos - 1 <= fe]))


def encode_run(run):
    """lab_pos, lab_prev (run-relative index of the label's previous occurrence, -1 = none) of one run"""
    pos = []; prev = []; last = {}
    for p, labels in run:
        for lab in labels:
            prev.append(last.get(lab, -1)); last[lab] = len(pos); pos.append(p)
    return pos, prev


class Case:
    """One launch.  runs: [(hap, run)]; pairs: [(fb, fe)]; work: [(pair, run index, item sizes or None = one item)], at most one entry
    per (pair, haplotype), the sizes adding up to the run's label count."""

    def __init__(self, name, runs, pairs, work, seed=1):
        self.name = name; self.runs = runs; self.pairs = pairs; self.work = work; self.seed = seed

    def n_labels(self, r):
        return sum(len(labels) for _, labels in self.runs[r][1])


class Encoded:
    pass


def encode(case):
    """arrays of a phz_gene_work for `case` (items in shuffled order) + the expected (n_pairs, 2) counts"""
    E = Encoded()
    E.name = case.name
    pos = [[], []]; prev = [[], []]; start = []
    for hap, run in case.runs:
        p, q = encode_run(run)
        start.append(len(pos[hap])); pos[hap] += p; prev[hap] += q
    E.lab_pos = [np.asarray(pos[h], dtype=np.int32) for h in (0, 1)]
    E.lab_prev = [np.asarray(prev[h], dtype=np.int32) for h in (0, 1)]
    E.n_pairs = len(case.pairs)
    E.pair_begin = np.asarray([p[0] for p in case.pairs], dtype=np.int32)
    E.pair_end = np.asarray([p[1] for p in case.pairs], dtype=np.int32)
    E.expected = np.zeros((E.n_pairs, 2), dtype=np.int32)
    items = []; seen = set()
    for pair, r, sizes in case.work:
        hap, run = case.runs[r]
        assert (pair, hap) not in seen, "one run per pair and haplotype"
        seen.add((pair, hap))
        total = case.n_labels(r)
        sizes = [total] if sizes is None else list(sizes)
        assert sum(sizes) == total and min(sizes) >= 0, (case.name, sizes, total)
        lo = start[r]
        for n in sizes:
            items.append((lo, n, start[r], pair, hap)); lo += n
        E.expected[pair, hap] = expected_counts(case.pairs[pair], run)
    order = np.random.default_rng(case.seed).permutation(len(items))
    items = [items[i] for i in order]
    col = lambda k, dt: np.asarray([it[k] for it in items], dtype=dt)
    E.item_lo = col(0, np.int64); E.item_n = col(1, np.int32); E.item_run = col(2, np.int64); E.item_pair = col(3, np.int32); E.item_hap = col(4, np.uint8)
    E.n_items = len(items)
    return E


def cut(total, sizes):
    """the given item sizes while they fit, then the rest"""
    out = []
    for s in sizes:
        if s > total - sum(out):
            break
        out.append(s)
    if total - sum(out):
        out.append(total - sum(out))
    return out


# ------------------------------------------------------------------------------------------------------------------ the named designs
BOUNDS_F = (100, 200)
BOUNDS_X = [99, 100, 101, 199, 200, 201]


def bounds():
    """Aims at `if (x < fb || x > fe) continue;` and at the same test of y inside the chain walk: variants on, one before and one after
    either feature end; features with fb == fe, fb > fe (counts 0), covering nothing and covering everything.  Every variant has a label of
    its own, so each count names the variants that were taken; the label "s" sits in every variant, so that its earlier occurrences lie
    exactly on fb and fe (ascending run: the one on fb; descending run: the one on fe)."""
    fb, fe = BOUNDS_F
    up = [(x + 1, ["v%d" % x, "s"]) for x in BOUNDS_X]
    down = up[::-1]
    pairs = [(fb, fe), (fb, fb), (fe, fe), (fe, fb), (300, 400), (0, 1000), (fb + 1, fe - 1), (fb - 1, fe + 1), (fe + 1, fe + 1), (fb - 1, fb - 1),
             (fb - 1, fb), (fe, fe + 1)]
    work = [(p, 0, None) for p in range(len(pairs))] + [(p, 1, None) for p in range(len(pairs))]
    return [Case("bounds", [(0, up), (1, down)], pairs, work)]


WALK_F = (100, 200)


def walk_on():
    """Aims at the chain loop `for (q = lab_prev[p]; q >= 0; q = lab_prev[run + q])`: it must walk on past an occurrence outside the
    feature ("ioi": inside, outside, inside -- the last one is NOT counted), count a last occurrence whose earlier ones are all outside
    ("ooi"), take the first of two inside ("oii"), follow a chain of 63 steps to its end, and treat a label repeated inside one variant's
    list as one read ("rep5")."""
    IN = [111, 121, 131, 141]; OUT = [51, 301, 311]
    run = [(IN[0], ["ioi", "a0"]), (OUT[0], ["ioi", "oii", "a1"]), (IN[1], ["ioi", "oii", "a2"]), (IN[2], ["oii", "rep5", "rep5", "a3", "rep5", "rep5", "rep5"]),
           (OUT[1], ["ooi", "a4"]), (OUT[2], ["ooi", "a5"]), (IN[3], ["ooi", "a6"])]
    long = [(1001 + v, ["all", "u%d" % v]) for v in range(64)]
    pairs = [WALK_F, (0, 1000), (300, 320), (50, 50), (1000, 1000), (1063, 1063), (1031, 1031), (1000, 1063)]
    work = [(p, 0, None) for p in range(4)] + [(p, 1, None) for p in range(4, 8)]
    return [Case("walk_on", [(0, run), (1, long)], pairs, work)]


def any_order():
    """Aims at the header's claim "any subset of the row's variants, in any order": nothing in the kernel may assume ascending positions.
    One run descends, one is shuffled and holds two variants with the same position; the features take the low end, the high end, the
    middle, the shared position alone."""
    rng = np.random.default_rng(11)
    positions = [900, 800, 700, 600, 500, 400, 300]
    lab = lambda: ["r%d" % x for x in rng.integers(0, 12, int(rng.integers(3, 9))).tolist()]
    down = [(p, lab()) for p in positions]
    shuffled = [(p, lab()) for p in (500, 900, 300, 500, 700, 400, 800)]
    pairs = [(299, 499), (699, 899), (399, 699), (499, 499), (0, 2000), (899, 899), (299, 299)]
    work = [(p, 0, None) for p in range(len(pairs))] + [(p, 1, None) for p in range(len(pairs))]
    return [Case("any_order", [(0, down), (1, shuffled)], pairs, work)]


SLICE_SIZES = [1, 63, 64, 65, 127, 128, 129, 4095]


def slices():
    """Aims at `lab_prev[run + q]` / `lab_pos[run + q]` against `p = lo + i`: a chain that starts in one item and ends in labels of another,
    so run and lo differ; at the lane loop `for (i = lane; i < n; i += 64)` on item sizes around the wave width; and at n = 0.  One run of
    about 9,000 labels per haplotype (40 variants, reads drawn from 600) cut three ways; all three launches must give the same counts.
    In front of them a launch of six labels in two items: "x" sits inside, outside, inside the feature, and its last occurrence lies in
    the second item, so the second step of its chain is `lab_prev[run + 3]` -- with lo in place of run it would read the next run."""
    rng = np.random.default_rng(12)
    pos = np.sort(rng.choice(np.arange(1000, 9000), 40, replace=False)).tolist()

    def run():
        return [(p, ["%d" % x for x in rng.integers(0, 600, int(rng.integers(180, 270))).tolist()]) for p in pos]
    two_steps = [(10, ["x", "p", "q"]), (50, ["x", "r"]), (20, ["x"])]
    runs = [(0, [(77, ["lead"])]), (0, two_steps), (0, run()), (1, run())]     # short runs in front: run start and array start differ
    pairs = [(0, 20000), (pos[5] - 1, pos[25] - 1), (pos[10] - 1, pos[10] - 1), (pos[30], 20000), (pos[39] - 1, pos[39] - 1), (10, 20), (9, 19)]
    cases = [Case("slices/two_steps", runs, pairs, [(6, 1, [3, 3])], seed=13)]
    for name, how in (("slices/4096", lambda t: cut(t, [4096] * 8)), ("slices/sizes", lambda t: cut(t, SLICE_SIZES)),
                      ("slices/zero", lambda t: cut(t, [4096] * 8)[:1] + [0] + cut(t, [4096] * 8)[1:] + [0])):
        c = Case(name, runs, pairs, [], seed=13)
        c.work = [(p, r, how(c.n_labels(r))) for p in range(6) for r in (2, 3)]
        cases.append(c)
    return cases


WAVE_TAIL_N = [1, 2, 3, 4, 5, 7, 8, 1021]


def wave_tail():
    """Aims at `it = blockIdx.x * 4 + (threadIdx.x >> 6); if (it >= n_items) return;` and at the clearing of the counts: item counts that
    leave 3, 2, 1 or 0 waves of the last workgroup idle, one item per (pair, haplotype), and pairs that own no item at all, which must
    read [0, 0] in an output that was full of -7."""
    cases = []
    for N in WAVE_TAIL_N:
        rng = np.random.default_rng(100 + N)
        n_pairs = N // 2 + 3
        empty = {1, n_pairs - 1}
        slots = [(p, h) for p in range(n_pairs) if p not in empty for h in (0, 1)]
        slots = [slots[i] for i in rng.permutation(len(slots))[:N]]
        runs = []; work = []
        for k, (p, h) in enumerate(slots):
            a = ["x%d" % j for j in range(k % 5 + 1)]
            runs.append((h, [(10, a), (20, a[:k % 3] + ["y"]), (30, ["z"] * (k % 2))]))
            work.append((p, k, None))
        pairs = [[(9, 19), (9, 9), (0, 50), (19, 29)][p % 4] for p in range(n_pairs)]
        cases.append(Case("wave_tail/%d" % N, runs, pairs, work, seed=N))
    return cases


def haps():
    """Aims at `hap ? pos_b : pos_a`, `hap ? prev_b : prev_a` and `counts[2 * pair + hap]`: the two label arrays differ in length and
    content, pair 0 has items with the same (lo, n, run) numbers in both arrays and different answers, pair 1 has items for haplotype 0
    only, pair 2 for haplotype 1 only.  Pair 3 takes the variant at 20 alone: read with the other haplotype's positions, either run gives
    another count (a: 2 reads, 4 with b's positions; b: 3 reads, 1 with a's)."""
    a0 = [(10, ["1", "2", "3"]), (20, ["1", "4"])]                       # 5 labels, 4 reads
    b0 = [(10, ["7"]), (20, ["8", "9", "7", "7"])]                       # 5 labels, 3 reads; positions 10,20,20,20,20 against a0's 10,10,10,20,20
    a1 = [(10, ["5", "6"]), (20, ["5", "6", "9", "10"]), (30, ["11"])]
    b1 = [(10, ["1", "2", "3", "4"]), (30, ["1", "2"])]
    pairs = [(0, 100), (0, 100), (0, 100), (19, 19)]
    work = [(0, 0, None), (0, 1, None), (1, 2, [3, 4]), (2, 3, [6]), (3, 0, [2, 3]), (3, 1, [1, 4])]
    return [Case("haps", [(0, a0), (1, b0), (0, a1), (1, b1)], pairs, work)]


def one_counter():
    """Aims at `atomicAdd(&counts[2 * pair + hap], cnt)`: 3,000 items of 1 to 3 labels that all add into one counter."""
    rng = np.random.default_rng(14)
    sizes = rng.integers(1, 4, 3000).tolist()
    total = sum(sizes)
    per = total // 30 + 1
    reads = rng.integers(0, 2500, total).tolist()
    run = [(100 + 10 * v, ["%d" % x for x in reads[v * per:(v + 1) * per]]) for v in range(30) if reads[v * per:(v + 1) * per]]
    pairs = [(0, 10), (99, 500), (0, 10)]
    return [Case("one_counter", [(1, run)], pairs, [(1, 0, sizes)], seed=15)]


RANDOM_SIZES = [1, 63, 64, 65, 100, 4096]


def random(ones_cap=None):
    """No line in particular: 30 rows of 2 to 11 variants, 0 to 199 labels per variant from 1 to 299 reads, 4 features per row on or
    beside variant positions, item sizes drawn from RANDOM_SIZES.  ones_cap bounds how many items of one label the design holds (the
    host emulation spends a wave of fibers on each)."""
    rng = np.random.default_rng(16)
    runs = []; pairs = []; work = []
    ones = 0
    for row in range(30):
        nv = int(rng.integers(2, 12))
        pos = rng.choice(np.arange(100, 400), nv, replace=False).tolist()
        nreads = int(rng.integers(1, 300))
        for hap in (0, 1):
            runs.append((hap, [(p, ["%d" % x for x in rng.integers(0, nreads, int(rng.integers(0, 200))).tolist()]) for p in pos]))
        for f in range(4):
            a, b = sorted(int(x) - 1 + int(rng.integers(-1, 2)) for x in rng.choice(pos, 2))
            pairs.append((a, b))
            for hap in (0, 1):
                r = 2 * row + hap
                left = sum(len(labels) for _, labels in runs[r][1]); sizes = []
                while left:
                    s = int(rng.choice(RANDOM_SIZES))
                    if s == 1 and ones_cap is not None and ones >= ones_cap:
                        continue
                    ones += s == 1
                    sizes.append(min(s, left)); left -= sizes[-1]
                work.append((len(pairs) - 1, r, sizes or None))
    return [Case("random", runs, pairs, work, seed=17)]


DESIGNS = {"bounds": bounds, "walk_on": walk_on, "any_order": any_order, "slices": slices, "wave_tail": wave_tail, "haps": haps,
           "one_counter": one_counter, "random": random}
