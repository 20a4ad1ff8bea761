"""Seeded inputs for the tests of vdjx_tree_spr: the builders of tests/tree_nj_cases.py and tests/tree_mp_cases.py (caterpillar starts,
mixed_random).  A case is tree_mp_cases' dict: tree_nj_cases' plus "start" (int32[nodes] parents in output slots, or None for
vdjx_tree_nj's tree) and "max_rounds".

The model's numpy search costs about (2m)^2 small array operations per round of a lineage of m members, so the cases above about 65
members carry a max_rounds of 1 .. 3.  The bound cases are cut to three constants of vdjx_spr.hip, read from the file by kernel_constant:
VDJX_SPR_LDS_MEMBERS (the slab in LDS up to it, in the workspace beyond), SPR_SLAB_WGS (the workgroups of the workspace path: more prunes
than that and a workgroup takes a second one) and SPR_PICK_T (k_spr_pick's threads: more keys than that and a thread reads a second one)."""
import functools

from tests import tree_mp_cases as MK
from tests import tree_nj_cases as K

with_caterpillars, plain, mixed_random, root_of, start_slots, caterpillar = (MK.with_caterpillars, MK.plain, MK.mixed_random, MK.root_of,
                                                                             MK.start_slots, MK.caterpillar)
GEOMETRY = ("g_root", "x_root", "c_leaf", "c_inferred", "y_leaf", "y_inferred")      # tree_spr_model.geometry's words


def kernel_constant(name):
    """a #define of vdjer_amd/csrc/vdjx_spr.hip as an int"""
    return K.kernel_constant("vdjx_spr.hip", name)


def handmade():
    """six members from a start written out by hand -- neither a caterpillar nor vdjx_tree_nj's tree: with r the root and l0 .. l4 the other
    leaves ascending, 6 = (7, 8) under r, 7 = (l0, l1), 8 = (l2, 9), 9 = (l3, l4)"""
    case = K.random_case(6, 50, 67)
    root = root_of(case, list(range(6)))
    l = [v for v in range(6) if v != root]
    local = [-1] * 10
    for v, p in [(6, root), (7, 6), (8, 6), (l[0], 7), (l[1], 7), (l[2], 8), (9, 8), (l[3], 9), (l[4], 9)]:
        local[v] = p
    return dict(case, start=start_slots(case, {0: local}))


def displaced(m, seed, lowest):
    """an infinite-sites lineage of m members started from its generator's own tree, rooted at the root member, with one clade out of
    place: the inferred node c >= lowest of smallest id with 3 .. 10 leaves is pruned and regrafted on the edge farthest from it (most
    edges between; the smallest id among those).  The first move of the search prunes that c again: a key past `lowest`"""
    from tests import tree_mp_model as M
    from tests import tree_spr_model as S
    case = K.infinite_sites(m, seed)
    adj, root = case["gen"][0]["adj"], root_of(case, list(range(m)))
    parent, stack = [-1] * (2 * m - 2), [root]
    while stack:
        v = stack.pop()
        for u in adj[v]:
            if u != parent[v]:
                parent[u] = v
                stack.append(u)
    kids = M.tree_of_parents(m, root, parent)
    leaves = lambda v: sum(1 for u in S.subtree(m, kids, v) if u < m)
    c = next(v for v in range(max(lowest, m), 2 * m - 2) if v != kids[root][0] and 3 <= leaves(v) <= 10)
    dist, stack = {parent[c]: 0}, [parent[c]]
    while stack:
        v = stack.pop()
        for u in adj[v]:
            if u not in dist:
                dist[u] = dist[v] + 1
                stack.append(u)
    ys = S.regrafts(m, root, parent, kids, c)
    y = min(ys, key=lambda v: (-dist[v], v))
    S.apply(parent, kids, c, y)
    return dict(case, start=start_slots(case, {0: parent})), c


def gpu_cases():
    """name -> builder of every case test_gpu_tree_spr.py runs; test_tree_spr_cpu.py checks that each reaches the edge it is named for"""
    bound = kernel_constant("VDJX_SPR_LDS_MEMBERS")
    out = {f"m{m}": (lambda m=m: plain(K.infinite_sites(m, 100 + m))) for m in (1, 2, 3)}
    out.update({
        "m4_nj": lambda: plain(K.random_case(4, 30, 31)),
        "m4_cat": lambda: with_caterpillars(K.infinite_sites(4, 104)),
        "m5_nj": lambda: plain(K.random_case(5, 40, 32)),
        "m5_cat": lambda: with_caterpillars(K.infinite_sites(5, 105)),
        "cat20": lambda: with_caterpillars(K.infinite_sites(20, 5)),
        "random_wild": lambda: plain(K.random_case(40, 100, 18, wild=0.1)),
        "random_wild_cat": lambda: with_caterpillars(K.random_case(40, 100, 18, wild=0.1)),
        "random_12": lambda: plain(K.random_case(12, 60, 3)),
        "random_12_cat": lambda: with_caterpillars(K.random_case(12, 60, 3)),
        "identical": lambda: plain(K.identical(7, 19)),
        "identical_cat": lambda: with_caterpillars(K.identical(7, 19)),
        "w1": lambda: with_caterpillars(K.random_case(6, 1, 33)),
        "w64": lambda: with_caterpillars(K.infinite_sites(12, 34, w=64)),
        "w65": lambda: with_caterpillars(K.infinite_sites(12, 35, w=65)),
        "w513": lambda: with_caterpillars(K.infinite_sites(20, 16, w=513)),
        "mixed": lambda: with_caterpillars(K.mixed(21)),
        "mixed_random": lambda: plain(mixed_random(22)),
        "many_small": lambda: plain(K.many_small(3000, 20)),
        "one_round": lambda: dict(with_caterpillars(K.mixed(21)), max_rounds=1),
        "handmade": handmade,
        # k_spr_score on both sides of the LDS bound; beyond it more prunes than workgroups, and k_spr_pick with more keys than threads
        "lds_bound": lambda: dict(with_caterpillars(K.random_case(bound, 90, 62, wild=0.05)), max_rounds=2),
        "lds_bound_plus1": lambda: dict(with_caterpillars(K.random_case(bound + 1, 90, 63, wild=0.05)), max_rounds=2),
        "slab_stride": lambda: dict(displaced(140, 64, kernel_constant("SPR_PICK_T"))[0], max_rounds=3),
    })
    return {k: (lambda f=f: dict({"max_rounds": 0}, **f())) for k, f in out.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    return gpu_cases()[name]()


@functools.lru_cache(maxsize=None)
def want(name, knob=1 << 26):
    """the model's result of a case, computed once for all the tests of a run: nothing but info["batches"] moves with the knob, so another
    knob's result is the first one's with the batches counted again"""
    from tests import tree_mp_model as M
    from tests import tree_spr_model as S
    c = case(name)
    if knob != 1 << 26:
        base = want(name)
        return dict(base, info=dict(base["info"], batches=M.batches_under([m for m in K.sizes_of(c) if m > 1], knob)))
    return S.tree_spr(c["contigs"], c["clone"], c["anchor"], c["prio"], start=c["start"], max_rounds=c["max_rounds"])
