"""Seeded inputs for the tests of vdjx_tree_sankoff_spr: the builders of tests/tree_nj_cases.py, tests/tree_mp_cases.py (caterpillar starts,
mixed_random), tests/tree_spr_cases.py (the handmade start, the displaced clade) and the matrices of tests/tree_sankoff_cases.py, by import
only.  A case is tree_spr_cases' dict -- tree_nj_cases' plus "start" and "max_rounds" -- plus "cost" (a 4 x 4 matrix).

The model's numpy search costs about (2m)^2 small array operations per round of a lineage of m members, so the cases above about 40 members
carry a max_rounds of 1 .. 3.  The bound cases are cut to constants of vdjx_sankoff_spr.hip, read from the file by kernel_constant:
SKSP_LDS_MEMBERS_8 and VDJX_SKSP_LDS_MEMBERS (the slab in LDS in one of two geometries up to them, in the workspace beyond the second),
SKSP_SLAB_WGS (the workgroups of the workspace path: more prunes than that and a workgroup takes a second one) and SKSP_PICK_T
(k_sksp_pick's threads: more keys than that and a thread reads a second one)."""
import functools

import numpy as np

from tests import tree_mp_cases as MK
from tests import tree_nj_cases as K
from tests import tree_sankoff_cases as KC
from tests import tree_spr_cases as SC

with_caterpillars, plain = MK.with_caterpillars, MK.plain
MATRICES = KC.MATRICES
UNIT, TSTV, ASYM, BIG = (MATRICES[k] for k in ("UNIT", "TSTV", "ASYM", "BIG"))
SEVENS = [[0 if s == t else 7 for t in range(4)] for s in range(4)]                  # all twelve costs 7: 7 x vdjx_tree_spr's count
GEOMETRY = SC.GEOMETRY
SPR_SHARED = tuple(k for k in sorted(SC.gpu_cases()) if not k.startswith("lds_bound") and k not in ("slab_stride", "many_small"))


def kernel_constant(name):
    """a #define of vdjer_amd/csrc/vdjx_sankoff_spr.hip as an int"""
    return K.kernel_constant("vdjx_sankoff_spr.hip", name)


def big_raw(seed=91, m=44, w=4000):
    """44 unrelated random members over 4,000 columns (24 stay at 2.6e9): under BIG the lineage costs more than 2^32"""
    rng = np.random.default_rng(seed)
    return K.assemble([(K.random_windows(m, w, rng, wild=0.01, per_member=1.0), None)], rng)


def gpu_cases():
    """name -> builder of every case test_gpu_tree_sankoff_spr.py runs; test_tree_sankoff_spr_cpu.py checks that each reaches the edge it
    is named for"""
    small, bound = kernel_constant("SKSP_LDS_MEMBERS_8"), kernel_constant("VDJX_SKSP_LDS_MEMBERS")
    under = lambda cost, f, **kw: (lambda: dict(f(), cost=cost, **kw))
    out = {f"m{m}": under(ASYM, lambda m=m: plain(K.infinite_sites(m, 100 + m))) for m in (1, 2, 3)}
    out.update({
        "m4_nj": under(TSTV, lambda: plain(K.random_case(4, 30, 31))),
        "m4_cat": under(ASYM, lambda: with_caterpillars(K.infinite_sites(4, 104))),
        "m5_nj": under(ASYM, lambda: plain(K.random_case(5, 40, 32))),
        "m5_cat": under(TSTV, lambda: with_caterpillars(K.infinite_sites(5, 105))),
        "handmade": under(TSTV, SC.handmade),
        "cat20": under(ASYM, lambda: with_caterpillars(K.infinite_sites(20, 5))),
        "cat20_unit": under(UNIT, lambda: with_caterpillars(K.infinite_sites(20, 5))),
        "random_wild": under(TSTV, lambda: plain(K.random_case(40, 100, 18, wild=0.1))),
        "random_wild_unit": under(UNIT, lambda: plain(K.random_case(40, 100, 18, wild=0.1))),
        "identical": under(ASYM, lambda: plain(K.identical(7, 19))),
        "identical_cat": under(TSTV, lambda: with_caterpillars(K.identical(7, 19))),
        "w1": under(ASYM, lambda: with_caterpillars(K.random_case(6, 1, 33))),
        "w64": under(TSTV, lambda: with_caterpillars(K.infinite_sites(12, 34, w=64))),
        "w65": under(ASYM, lambda: with_caterpillars(K.infinite_sites(12, 35, w=65))),
        "w513": under(TSTV, lambda: with_caterpillars(K.infinite_sites(20, 16, w=513))),
        "mixed": under(ASYM, lambda: dict(with_caterpillars(K.mixed(21)), max_rounds=12)),      # (the caterpillars of 20 and 65 are cut)
        "mixed_random": under(TSTV, lambda: plain(MK.mixed_random(22))),
        # k_sksp_score on both sides of either LDS bound; beyond the second more prunes than workgroups, and k_sksp_pick with more keys than
        # threads
        "lds8_bound": under(ASYM, lambda: with_caterpillars(K.random_case(small, 70, 60, wild=0.05))),
        "lds8_bound_plus1": under(TSTV, lambda: with_caterpillars(K.random_case(small + 1, 70, 61, wild=0.05))),
        "lds_bound": under(ASYM, lambda: dict(with_caterpillars(K.random_case(bound, 90, 62, wild=0.05)), max_rounds=2)),
        "lds_bound_plus1": under(BIG, lambda: dict(with_caterpillars(K.random_case(bound + 1, 90, 63, wild=0.05)), max_rounds=2)),
        "slab_stride": under(ASYM, lambda: dict(SC.displaced(140, 64, kernel_constant("SKSP_PICK_T"))[0], max_rounds=1)),
        "big": under(BIG, lambda: dict(plain(big_raw()), max_rounds=1)),
    })
    out.update({f"random_12_{name.lower()}": under(cost, lambda: plain(K.random_case(12, 60, 3))) for name, cost in MATRICES.items()})
    return {k: (lambda f=f: dict({"max_rounds": 0}, **f())) for k, f in out.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    return gpu_cases()[name]()


@functools.lru_cache(maxsize=None)
def want(name, knob=1 << 26):
    """the model's result of a case, computed once for all the tests of a run: nothing but info["batches"] moves with the knob, so another
    knob's result is the first one's with the batches counted again"""
    from tests import tree_mp_model as M
    from tests import tree_sankoff_spr_model as X
    c = case(name)
    if knob != 1 << 26:
        base = want(name)
        return dict(base, info=dict(base["info"], batches=M.batches_under([m for m in K.sizes_of(c) if m > 1], knob)))
    return X.tree_sankoff_spr(c["contigs"], c["clone"], c["anchor"], c["prio"], cost=c["cost"], start=c["start"], max_rounds=c["max_rounds"])
