"""Seeded inputs for the tests of vdjx_tree_sankoff: the builders of tests/tree_nj_cases.py, tests/tree_mp_cases.py (caterpillar starts,
mixed_random) and tests/tree_spr_cases.py (the handmade start).  A case is tree_mp_cases' dict -- tree_nj_cases' plus "start" and
"max_rounds" -- plus "cost" (a 4 x 4 matrix), "search" and "plain" (which path of the model computes it: None for the model's own choice by
size, False where the plain path would take minutes).

The shapes are the smallest at which the kernels can go wrong.  The bound cases are cut to two constants of vdjx_sankoff.hip, read from
the file by kernel_constant: SK_PICK_T (k_sk_pick's threads: more candidates than that and a thread reads a second key) and SK_FILL_WAVES
(the scorer's grid is as high as fills that many waves and no higher than the most column tiles of a searched lineage: below that, a wave
walks several tiles in turn).  A case named unit_<x> is tree_mp_cases' case <x> under the unit matrix."""
import functools

import numpy as np

from tests import tree_mp_cases as MK
from tests import tree_nj_cases as K
from tests import tree_spr_cases as SK

with_caterpillars, plain = MK.with_caterpillars, MK.plain

UNIT = [[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]]
TSTV = [[0, 2, 1, 2], [2, 0, 2, 1], [1, 2, 0, 2], [2, 1, 2, 0]]             # transitions A <-> G, C <-> T 1, transversions 2
ASYM = [[0, 5, 2, 7], [4, 0, 6, 1], [3, 5, 0, 6], [7, 2, 5, 0]]
BIG = [[0, 65535, 65535, 65535], [65535, 0, 65535, 65535], [65535, 1, 0, 65535], [65535, 65535, 65535, 0]]      # one cell of 1: G over C
MATRICES = {"UNIT": UNIT, "TSTV": TSTV, "ASYM": ASYM, "BIG": BIG}
UNIT_SHARED = ("m1", "m2", "m3", "m4_nj", "m4_cat", "m5_nj", "m5_cat", "w1", "w65", "cat20", "random_wild", "random_12", "identical", "mixed_random",
               "one_round")                                  # cases of tree_mp_cases.gpu_cases run under UNIT


def kernel_constant(name):
    """a #define of vdjer_amd/csrc/vdjx_sankoff.hip as an int"""
    return K.kernel_constant("vdjx_sankoff.hip", name)


def members_for_candidates(count):
    """the smallest lineage with at least `count` candidates: 2 (m - 3) of them"""
    return (count + 1) // 2 + 3


def stride_tiles_raw(seed=71):
    """300 lineages of 6 .. 8 members with windows of 450 .. 600 columns (8 .. 10 column tiles), interleaved: about 2,400 candidates, so
    the scorer's grid is SK_FILL_WAVES / 2,400 = 7 waves high -- below the tiles of every lineage: a wave takes a second tile"""
    rng = np.random.default_rng(seed)
    lin = [(K.random_windows(int(rng.integers(6, 9)), int(rng.integers(450, 601)), rng, wild=0.03, per_member=0.2), None) for _ in range(300)]
    return K.assemble(lin, rng, loose=20, shuffle=True)


def big_raw(seed=72, m=340):
    """340 unrelated random members over 513 columns (200 stay below 2^32 in all): under BIG a column costs far more than 2^16 and the lineage more than 2^32"""
    rng = np.random.default_rng(seed)
    return K.assemble([(K.random_windows(m, 513, rng, wild=0.01, per_member=1.0), None)], rng)


def scorer_grid(case):
    """MK.scorer_grid under this file's SK_FILL_WAVES: (n_cand, tiles of every searched lineage, grid_y)"""
    fill = kernel_constant("SK_FILL_WAVES")
    ws = MK.lineage_windows(case)
    searched = [key for key in sorted(ws) if len(ws[key]) > 3]
    n_cand = sum(2 * (len(ws[key]) - 3) for key in searched)
    tiles = [(len(ws[key][0]) + 63) // 64 for key in searched]
    return n_cand, tiles, (min(max(tiles), (fill + n_cand - 1) // n_cand) if n_cand else 1)


def gpu_cases():
    """name -> builder of every case test_gpu_tree_sankoff.py runs; test_tree_sankoff_cpu.py checks that each reaches the edge it is named
    for"""
    pick = members_for_candidates(kernel_constant("SK_PICK_T"))
    under = lambda cost, f, **kw: (lambda: dict(f(), cost=cost, **kw))
    out = {f"m{m}": under(ASYM, lambda m=m: plain(K.infinite_sites(m, 100 + m))) for m in (1, 2, 3)}
    out.update({
        "m4_nj": under(TSTV, lambda: plain(K.random_case(4, 30, 31))),
        "m4_cat": under(ASYM, lambda: with_caterpillars(K.infinite_sites(4, 104))),
        "m5_nj": under(ASYM, lambda: plain(K.random_case(5, 40, 32))),
        "m5_cat": under(TSTV, lambda: with_caterpillars(K.infinite_sites(5, 105))),
        "small_wild_cat": under(ASYM, lambda: with_caterpillars(K.assemble(
            [(K.random_windows(m, 25, np.random.default_rng(80 + m), wild=0.3), None) for m in (1, 2, 3, 4, 5)], np.random.default_rng(80)))),
        "w1": under(ASYM, lambda: with_caterpillars(K.random_case(6, 1, 33))),
        "w64": under(TSTV, lambda: with_caterpillars(K.infinite_sites(12, 34, w=64))),
        "w65": under(ASYM, lambda: with_caterpillars(K.infinite_sites(12, 35, w=65))),
        "w513": under(TSTV, lambda: with_caterpillars(K.infinite_sites(20, 16, w=513))),
        "cat20": under(ASYM, lambda: with_caterpillars(K.infinite_sites(20, 5))),
        "cat20_tstv": under(TSTV, lambda: with_caterpillars(K.infinite_sites(20, 5))),
        "random_wild": under(TSTV, lambda: plain(K.random_case(40, 100, 18, wild=0.1))),
        "random_wild_asym": under(ASYM, lambda: plain(K.random_case(40, 100, 18, wild=0.1))),
        "random_12": under(TSTV, lambda: plain(K.random_case(12, 60, 3))),
        "identical": under(ASYM, lambda: plain(K.identical(7, 19))),
        "identical_cat": under(TSTV, lambda: with_caterpillars(K.identical(7, 19))),
        "many_small": under(ASYM, lambda: plain(K.many_small(300, 20, loose=30))),
        "mixed": under(ASYM, lambda: dict(with_caterpillars(K.mixed(21)), max_rounds=12)),      # (the caterpillars of 20 and 65 are cut)
        "mixed_random": under(TSTV, lambda: plain(MK.mixed_random(22))),
        "handmade": under(ASYM, SK.handmade),
        "one_round": under(TSTV, lambda: dict(with_caterpillars(K.mixed(21)), max_rounds=1)),
        "no_search": under(ASYM, lambda: with_caterpillars(K.random_case(40, 100, 18, wild=0.1)), search=False),
        # k_sk_pick: as many candidates as threads, and two more; k_sk_score: a wave over several column tiles
        "pick_bound": under(TSTV, lambda: dict(with_caterpillars(K.infinite_sites(pick, 73)), max_rounds=1)),
        "pick_bound_plus1": under(TSTV, lambda: dict(with_caterpillars(K.infinite_sites(pick + 1, 74)), max_rounds=1)),
        "stride_tiles": under(ASYM, lambda: plain(stride_tiles_raw()), plain=False),
        "big": under(BIG, lambda: dict(plain(big_raw()), max_rounds=1)),
    })
    mp = MK.gpu_cases()
    out.update({f"unit_{name}": under(UNIT, mp[name]) for name in UNIT_SHARED})
    return {k: (lambda f=f: dict({"max_rounds": 0, "search": True, "plain": None}, **f())) for k, f in out.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    return gpu_cases()[name]()


@functools.lru_cache(maxsize=None)
def want(name, knob=1 << 26):
    """the model's result of a case, computed once for all the tests of a run: nothing but info["batches"] moves with the knob, so another
    knob's result is the first one's with the batches counted again"""
    from tests import tree_mp_model as M
    from tests import tree_sankoff_model as S
    c = case(name)
    if knob != 1 << 26:
        base = want(name)
        return dict(base, info=dict(base["info"], batches=M.batches_under([m for m in K.sizes_of(c) if m > 1], knob)))
    return S.tree_sankoff(c["contigs"], c["clone"], c["anchor"], c["prio"], cost=c["cost"], start=c["start"], search_=c["search"],
                          max_rounds=c["max_rounds"], plain=c["plain"])
