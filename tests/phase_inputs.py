"""Designed connected components for the block-phasing kernels (k_edge_local / k_phase_pair / k_phase_general, phz_rowsdev.hip) -- test
side, plain Python, no GPU, deterministic.

A case is (name, n, edges, max_block_size) plus what its design promises (tests/test_phase_limits.py checks every promise against the
host routine and the Python restatement before any kernel sees the case).  edges are (i, j, cfg): local variant indices, cfg 0 same
configuration / 1 opposite / -1 tie.

The building block is a component whose whole-component flood fails and which is still left as ONE fragment: pairs (i, i + 1) and
(i, i + 2) for every i, so that every cut position is spanned by at least two pairs (split_by_weak cuts only where the number of spanning
pairs equals the level, starting at 1, and stops after the first level when nothing is longer than max_block_size), chosen longer pairs
(i, i + D), and one contradictory verdict; max_block_size is 0 or >= n.  The search then sees a fragment of n variants whose farthest
pair with a verdict spans D: the dynamic programme for n >= 8 and D <= 10, brute force otherwise.  A pair whose verdict is a tie counts
for the split and not for D, which is how D = 0 and D = 1 fragments hold together.

Why the outcome of a single-fragment design is known in advance.  Fix variant 0's allele; a configuration is the truth with a set S of
variants flipped; with m pairs carrying a verdict of which one contradicts the truth, the truth satisfies m - 1, a set S that separates
the contradicting pair satisfies m - cut(S) and any other S satisfies m - 1 - cut(S), cut(S) = consistent pairs leaving S.
  "unique": the consistent pairs hold (i, i + 1) and (i, i + 2) throughout (one of them less when D = 2), every cut has two pairs or more
            -> the truth alone reaches m - 1 -> one block of n variants.
  "tie":    variant 0 keeps one consistent pair, (0, 1), and one contradicting pair, (0, D); (0, 2) is a tie -> the truth and the truth
            with variant 0 flipped both reach m - 1, nothing reaches m -> all '-' -> no block.
  D = 1:    verdicts only on (i, i + 1) form a forest: never a contradiction, the flood fails only when the forest is disconnected, and
            then the two sides flip independently -> always a tie.  A unique winner does not exist at D = 1 (nor at n = 3, where a
            contradicting triangle leaves three configurations with two pairs each).
  D = 0:    every verdict a tie, every score 0 -> no block.
  "noisy":  several contradictions; one block of n or none, whatever the host routine says.

Split designs start from every pair up to distance 3 (six pairs span an interior cut) and thin the pairs around chosen positions down
to a chosen level; the one position whose spanning pairs are all ties is where the stitching finds no winner for the first time, so the
host's first block ends exactly there (after that first break the reference's start index is assigned, not advanced, and nothing
further is promised about block boundaries -- only that all tiers agree)."""
import dataclasses
import functools
import random
from typing import List, Optional, Tuple

PH_NMAX, PH_EMAX, PH_BRUTE_MAX, PH_DP_MAXD, PH_DP_MINLEN = 256, 2048, 22, 10, 8      # the kernel's limits (phz_rowsdev.hip)
PH_GRID, PH_BATCH = 4096, 4
BEST_FREE_MAX = 30                                                                   # phz_rows.cpp: best_free refuses beyond


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    n: int
    edges: Tuple[Tuple[int, int, int], ...]
    mbs: int
    E: int                                   # promised number of pairs
    span: int                                # promised largest |i - j| over all pairs, ties included
    D: Optional[int] = None                  # single-fragment designs: farthest pair WITH a verdict (what the search sees)
    search: Optional[str] = None             # "dp" / "brute" / "host" (fragment longer than PH_BRUTE_MAX: handed over inside the call)
    blocks: Optional[str] = None             # "one" (one block of n variants) / "none" / "either"
    flood_fails: bool = True                 # the whole-component flood of resolve_phase does not accept
    cuts: Tuple[int, ...] = ()               # positions that must be fragment boundaries
    blocked: Tuple[int, ...] = ()            # positions that must NOT be
    first_break: Optional[int] = None        # the host's first block is exactly [0, first_break)
    host_path: bool = False                  # beyond the kernel's tables: comes back from the host inside the call
    clean_fragments: bool = False            # every fragment is settled by its own flood: nothing of the component reaches the host or the search
    refused: Optional[str] = None            # "split" / "fragment": the host routine returns PHZ_E_UNSUPPORTED

    def __iter__(self):                      # (name, n, edges, max_block_size)
        return iter((self.name, self.n, self.edges, self.mbs))


def _rng(*key):
    return random.Random("phase_inputs/" + "/".join(str(k) for k in key))


def _emit(rng, n, pairs, truth):
    """pairs: {(i, j): 'ok' | 'flip' | 'tie'} -> shuffled edge list with random orientation, verdicts from the truth"""
    edges = []
    for (i, j), what in sorted(pairs.items()):
        assert 0 <= i < j < n
        k = -1 if what == "tie" else (truth[i] ^ truth[j]) ^ (1 if what == "flip" else 0)
        edges.append((j, i, k) if rng.random() < 0.5 else (i, j, k))
    rng.shuffle(edges)
    return tuple(edges)


# ------------------------------------------------------------------------------------------------ one fragment of n variants
def single(n, D, mode, mbs):
    assert mode in ("unique", "tie", "noisy") and 0 <= D < n
    rng = _rng("single", n, D, mode)
    truth = [rng.randint(0, 1) for _ in range(n)]
    pairs = {}
    for i in range(n - 1):
        pairs[(i, i + 1)] = "ok" if D >= 1 else "tie"
    for i in range(n - 2):
        pairs[(i, i + 2)] = "ok" if D >= 2 else "tie"
    if D == 0:
        blocks = "none"
    elif D == 1:
        assert mode == "tie"
        pairs[(n // 2, n // 2 + 1)] = "tie"                      # disconnects the forest: the flood stops there
        blocks = "none"
    else:
        for d in range(3, D):                                    # a few pairs at every distance below D, none at variant 0
            for i in {1 + (7 * d) % (n - d - 1), 1 + (11 * d + 3) % (n - d - 1)}:
                pairs[(i, i + d)] = "ok"
        if mode == "tie":
            pairs[(0, 2)] = "tie"
            pairs[(0, D)] = "flip"
            blocks = "none"
        else:
            far = list(range(1, n - D, 3)) or [0]
            for i in far:
                pairs[(i, i + D)] = "ok"
            a = far[len(far) // 2]
            if D == 2:
                a = n // 2 - 1
            pairs[(a, a + D)] = "flip"
            blocks = "one" if n > 3 else "none"
            if mode == "noisy":
                keys = sorted(pairs)
                for k in rng.sample(keys, max(2, len(keys) // 6)):
                    pairs[k] = "flip"
                pairs[(0, D)] = "ok"                             # keeps D what the name says
                blocks = "either"
    if n > PH_BRUTE_MAX:
        search = "host"
    else:
        search = "dp" if n >= PH_DP_MINLEN and D <= PH_DP_MAXD else "brute"
    refused = "fragment" if n > BEST_FREE_MAX else None
    return Case("%s_len%d_D%d_%s_mbs%d" % (search, n, D, mode, mbs), n, _emit(rng, n, pairs, truth), mbs, E=len(pairs), span=max(2, D) if n > 2 else 1,
                D=D, search=search, blocks=None if refused else blocks, host_path=search == "host", refused=refused)


@functools.lru_cache(maxsize=None)
def single_cases() -> Tuple[Case, ...]:
    out = []
    alt = [0]

    def add(n, D, mode):
        alt[0] += 1
        out.append(single(n, D, mode, 0 if alt[0] % 2 else 40))              # max_block_size 0 and >= n in turn
    for n in (8, 15, 22):                                                    # dynamic programme: 2 / 32 / 64 / 128 / 1024 states
        add(n, 0, "tie")
        add(n, 1, "tie")
        for D in (5, 6, 7, 10):
            if D < n:
                for mode in ("unique", "tie", "noisy"):
                    add(n, D, mode)
    add(3, 2, "unique"); add(3, 0, "tie")                                    # brute force (n = 3: the contradicting triangle, a tie)
    for D in (3, 6):
        for mode in ("unique", "tie", "noisy"):
            add(7, D, mode)
    add(7, 5, "unique")                                                      # thresholds: 7 / 8 variants at D = 5 (8: above),
    add(12, 10, "unique"); add(12, 10, "tie")                                # D = 10 / 11 at 12 variants,
    for n, D in ((12, 11), (18, 11), (18, 17), (22, 11), (22, 21)):
        add(n, D, "unique"); add(n, D, "tie")
    add(18, 13, "noisy")
    add(23, 11, "unique")                                                    # 22 / 23 variants at D = 11: 23 goes to the host inside the call
    return tuple(out)


def fragment_of_31() -> Case:
    """past best_free's own limit of 30: the kernel hands it over, the host routine refuses it"""
    return single(31, 11, "unique", 0)


# ------------------------------------------------------------------------------------------------ k_phase_pair
@functools.lru_cache(maxsize=None)
def pair_cases() -> Tuple[Case, ...]:
    out = []
    for k in (0, 1, -1):
        out.append(Case("pair_two_variants_cfg%s" % ("m1" if k < 0 else k), 2, ((0, 1, k),) if k else ((1, 0, k),), 15, E=1, span=1,
                        flood_fails=k < 0, blocks="none" if k < 0 else "one"))

    def tree(name, n):
        rng = _rng(name)
        truth = [rng.randint(0, 1) for _ in range(n)]
        pairs = {(rng.randrange(max(0, i - 5), i), i): "ok" for i in range(1, n - 1)}
        pairs[(0, n - 1)] = "ok"
        return Case(name, n, _emit(rng, n, pairs, truth), 15, E=n - 1, span=n - 1, flood_fails=False, blocks="one")
    out.append(tree("pair_tree_17_variants_16_pairs", 17))                   # accepted by the per-thread flood (pairs <= 16)
    out.append(tree("pair_tree_18_variants_17_pairs", 18))                   # clean, one pair too many: k_phase_general's reached == n branch
    rng = _rng("pair_9_16")
    truth = [rng.randint(0, 1) for _ in range(9)]
    pairs = {(i, i + 1): "ok" for i in range(8)}
    pairs.update({(i, i + 2): "ok" for i in range(7)})
    pairs[(0, 8)] = "flip"
    out.append(Case("pair_9_variants_16_pairs_conflict", 9, _emit(rng, 9, pairs, truth), 15, E=16, span=8, blocks="either"))
    out.append(Case("pair_clean_all_opposite", 10, tuple((i + 1, i, 1) if i % 2 else (i, i + 1, 1) for i in range(9)), 15, E=9, span=1,
                    flood_fails=False, blocks="one"))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ split over a wide component
def _thin(pairs, p, level):
    """leave `level` pairs spanning the cut before variant p: the pair (p - 1, p) and the first level - 1 others"""
    over = sorted(q for q in pairs if q[0] < p <= q[1] and q != (p - 1, p))
    assert len(over) >= level - 1, (p, level, over)
    for q in over[level - 1:]:
        del pairs[q]


def split(n, mbs, brk, level2=(), same=(), name=None, conflicts=6):
    """every pair up to distance 3, thinned to one spanning pair at `brk`, at every 11th position on both sides of it (one of them left out on each
    side that has room: a stretch of 22 keeps the levels above 1 in play) and at the positions `same`; thinned to two at `level2`.  The pair over
    `brk` is a tie; verdicts behind it carry `conflicts` contradictions, the ones before it none."""
    rng = _rng("split", n, mbs, brk, name)
    truth = [rng.randint(0, 1) for _ in range(n)]
    pairs = {(i, i + d): "ok" for d in (1, 2, 3) for i in range(n - d)}
    ones = {brk} | set(same)
    left = [p for p in range(brk - 11, 1, -11)]
    right = [p for p in range(brk + 11, n - 1, 11)]
    for side in (left, right):
        if len(side) >= 3:
            del side[1]
    ones |= set(left) | set(right)
    for p in sorted(ones):
        assert 2 <= p <= n - 2 and all(abs(p - q) > 3 or p == q or q in same or p in same for q in ones), (p, sorted(ones))
        _thin(pairs, p, 1)
    for p in level2:
        _thin(pairs, p, 2)
    pairs[(brk - 1, brk)] = "tie"
    behind = sorted(q for q in pairs if q[0] >= brk + 1)
    for q in rng.sample(behind, min(conflicts, len(behind))):
        pairs[q] = "flip"
    blocked = tuple(sorted(set(level2) | {q for q in same}))
    return Case(name or "split_n%d_mbs%d_break%d" % (n, mbs, brk), n, _emit(rng, n, pairs, truth), mbs, E=len(pairs), span=3,
                cuts=tuple(sorted(ones - set(same))), blocked=blocked, first_break=brk, host_path=n > PH_NMAX)


SPLIT_DESIGNS = (          # n, first break, positions thinned to level 2 (blocked by a cut to their right or left), level-1 positions blocked by their left neighbour
    (63, 61, (), ()),            # n - 2, the last candidate
    (64, 62, (), ()),
    (65, 63, (), ()),            # n - 2 = bit 63 of word 0
    (128, 63, (), (64,)),        # 63 and 64 at the same level: 63 is cut, 64 (bit 0 of word 1) is blocked by is_cut(q - 1) across the words
    (128, 65, (64,), ()),        # 65 cut at level 1, 64 at level 2 blocked by is_cut(q + 1) inside word 1
    (129, 127, (), ()),          # n - 2 = bit 63 of word 1
    (200, 64, (63,), ()),        # 64 cut at level 1; 63 at level 2 is blocked by is_cut(q + 1) across the words
    (200, 128, (127,), ()),      # the same at the second boundary
    (255, 127, (), (128,)),
    (255, 191, (), (192,)),      # third boundary, same level on both sides
    (256, 192, (191,), ()),      # third boundary, is_cut(q + 1) across the words
    (256, 254, (), ()),          # n - 2 at the largest n the tables take: lane 63's fourth position of the running sum
)


@functools.lru_cache(maxsize=None)
def split_cases() -> Tuple[Case, ...]:
    out = [split(n, mbs, brk, l2, same) for mbs in (15, 8) for n, brk, l2, same in SPLIT_DESIGNS]
    out.append(fragments_over_32())
    out.append(clean_fragments(100, (40, 76)))                               # fragments of 40, 36 and 24 variants
    out.append(clean_fragments(100, (33, 65)))                               # 33, 32 and 35: both sides of the 32 variants the bit-mask flood takes
    return tuple(out)


def fragments_over_32() -> Case:
    """max_block_size 0 on 100 variants: only level 1 is cut, at 40 and 76.  Fragments of 40 and 36 variants, clean, take flood(base, base + len)
    (not the bit-mask flood for up to 32 variants); the fragment of 24 carries a contradiction, is longer than PH_BRUTE_MAX and goes to the host:
    the handover of an unresolved fragment -- the host then phases the WHOLE component again, so what the device made of the fragments of 40
    and 36 is not what comes back (clean_fragments() is where that is compared)."""
    n = 100
    rng = _rng("fragments_over_32")
    truth = [rng.randint(0, 1) for _ in range(n)]
    pairs = {(i, i + d): "ok" for d in (1, 2, 3) for i in range(n - d)}
    for p in (40, 76):
        _thin(pairs, p, 1)
    pairs[(85, 88)] = "flip"
    return Case("split_n100_mbs0_fragments_40_36_24", n, _emit(rng, n, pairs, truth), 0, E=len(pairs), span=3, cuts=(40, 76), host_path=True)


def clean_fragments(n, cuts) -> Case:
    """max_block_size 0, no contradiction anywhere: one pair spans each of `cuts` and that pair is a tie, so the whole-component flood stops at
    the first cut, level 1 cuts exactly there, and every fragment is settled by its own flood -- over 32 variants by flood(base, base + len)
    and marks_to_string, up to 32 by the bit-mask flood.  Nothing goes to the host or to the search: the fragments' configurations and their
    stitching (no joint configuration wins over a tie, so the first block ends at the first cut) are the device's own."""
    rng = _rng("clean_fragments", n, *cuts)
    truth = [rng.randint(0, 1) for _ in range(n)]
    pairs = {(i, i + d): "ok" for d in (1, 2, 3) for i in range(n - d)}
    for p in cuts:
        _thin(pairs, p, 1)
        pairs[(p - 1, p)] = "tie"
    lens = [b - a for a, b in zip((0,) + tuple(cuts), tuple(cuts) + (n,))]
    return Case("split_n%d_mbs0_clean_fragments_%s" % (n, "_".join(str(x) for x in lens)), n, _emit(rng, n, pairs, truth), 0, E=len(pairs), span=3,
                cuts=tuple(cuts), first_break=cuts[0], clean_fragments=True)


# ------------------------------------------------------------------------------------------------ table limits
def dense(n, E, mbs=15):
    """n variants, pairs at distances 1 to 9 with all of distance 1 kept and others dropped down to E; a contradiction every 37 pairs"""
    rng = _rng("dense", n, E)
    truth = [rng.randint(0, 1) for _ in range(n)]
    far = [(i, i + d) for d in range(2, 10) for i in range(n - d)]
    drop = (n - 1) + len(far) - E
    assert 0 <= drop <= len(far) // 4
    dropped = set(rng.sample(far, drop))
    pairs = {(i, i + 1): "ok" for i in range(n - 1)}
    for t, q in enumerate(q for q in far if q not in dropped):
        pairs[q] = "flip" if t % 37 == 5 else "ok"
    return Case("table_n%d_E%d" % (n, E), n, _emit(rng, n, pairs, truth), mbs, E=E, span=9, host_path=n > PH_NMAX or E > PH_EMAX)


@functools.lru_cache(maxsize=None)
def table_cases() -> Tuple[Case, ...]:
    out = [dense(256, E) for E in (2047, 2048, 2049)]                        # the last pair counts whose list fits s_i / s_j / s_k
    out.append(split(257, 15, 192, (191,), (), name="table_n257_mbs15_break192"))      # (255 and 256 variants: among the split designs)
    out.append(split(4100, 15, 2050, (), (), name="table_n4100_mbs15_break2050", conflicts=40))     # past the 12-bit fields of eloc
    return tuple(out)


# ------------------------------------------------------------------------------------------------ refusal
def unsplittable() -> Case:
    """six variants with a contradiction and max_block_size 1: the levels run out before every fragment is down to one variant"""
    rng = _rng("unsplittable")
    truth = [rng.randint(0, 1) for _ in range(6)]
    pairs = {(i, i + 1): "ok" for i in range(5)}
    pairs.update({(i, i + 2): "ok" for i in range(4)})
    pairs[(1, 4)] = "flip"
    return Case("refuse_split_n6_mbs1", 6, _emit(rng, 6, pairs, truth), 1, E=10, span=3, refused="split")


# ------------------------------------------------------------------------------------------------ many components
N_MANY = 20000
assert N_MANY > PH_GRID * PH_BATCH                                            # some wave must come back for a second batch of tickets


@functools.lru_cache(maxsize=None)
def many_shapes() -> Tuple[Case, ...]:
    """50 distinct components of 3 to 6 variants, every pair present, the triangle (0, 1, 2) contradicting: none is settled by k_phase_pair"""
    out = []
    for s in range(50):
        n = 3 if s < 2 else 4 + s % 3
        rng = _rng("many", s)
        k01, k12 = (s & 1, s & 1) if s < 2 else (rng.randint(0, 1), rng.randint(0, 1))
        edges = []
        for i in range(n):
            for j in range(i + 1, n):
                k = rng.choice([0, 0, 1, 1, -1])
                if j <= 2:
                    k = {(0, 1): k01, (1, 2): k12, (0, 2): k01 ^ k12 ^ 1}[(i, j)]
                edges.append((j, i, k) if rng.random() < 0.5 else (i, j, k))
        rng.shuffle(edges)
        out.append(Case("many_shape%02d" % s, n, tuple(edges), 15, E=n * (n - 1) // 2, span=n - 1, blocks=None))
    assert len({(c.n, c.edges) for c in out}) == len(out)
    return tuple(out)


def many_order() -> List[int]:
    """shape index of each of the N_MANY components: a seeded shuffle of the cycle, so that neighbours in the ticket order differ in size"""
    order = [t % 50 for t in range(N_MANY)]
    _rng("many_order").shuffle(order)
    return order


# ------------------------------------------------------------------------------------------------ lists
def accepted_cases() -> Tuple[Case, ...]:
    """every designed case the host routine accepts (the 20,000-component list is built from many_shapes() / many_order())"""
    return single_cases() + pair_cases() + split_cases() + table_cases()


def refused_cases() -> Tuple[Case, ...]:
    return (unsplittable(), fragment_of_31())


def lists_by_block_size():
    """accepted cases grouped by max_block_size (one phz_phase_components call takes one): {mbs: [Case, ...]}"""
    out = {}
    for c in accepted_cases():
        out.setdefault(c.mbs, []).append(c)
    return out
