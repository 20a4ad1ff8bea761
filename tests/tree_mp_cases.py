"""Seeded inputs for the tests of vdjx_tree_mp: the builders of tests/tree_nj_cases.py, and caterpillar start trees.  A case is
tree_nj_cases' dict plus "start" (int32[nodes] parents in output slots, or None for vdjx_tree_nj's tree) and "max_rounds".

caterpillar(m, root): the leaves other than the root, ascending, are l_0 .. l_(m-2); inferred node m + j has the children l_j and
m + j + 1, the last inferred node l_(m-3) and l_(m-2); the root's child is m.  Far from any good tree: the search has a long way to go,
and its paths to the root are as long as the lineage."""
import numpy as np

from tests import tree_nj_cases as K
from tests.tree_model import members_of

header_constant = K.header_constant


def caterpillar(m, root):
    """local parents of the 2m - 2 nodes (m >= 3); the root's is -1"""
    leaves = [v for v in range(m) if v != root]
    parent = [-1] * (2 * m - 2)
    for j in range(m - 2):
        parent[leaves[j]] = m + j
        parent[m + j] = m + j - 1 if j else root
    parent[leaves[m - 2]] = 2 * m - 3
    return parent


def root_of(case, members):
    return min(range(len(members)), key=lambda p: (int(case["prio"][members[p]]), members[p]))


def start_slots(case, local_parents):
    """local_parents: lineage key -> the local parents of its nodes -> int32[nodes] in output slots (-1 elsewhere)"""
    groups = members_of(case["clone"])
    n = len(case["contigs"])
    nodes = n + sum(max(0, len(v) - 2) for v in groups.values())
    out = np.full(nodes, -1, np.int32)
    slot0 = n
    for key in sorted(groups):
        members, m = groups[key], len(groups[key])
        slot = lambda v: members[v] if v < m else slot0 + v - m
        if key in local_parents:
            for v, p in enumerate(local_parents[key]):
                out[slot(v)] = slot(p) if p >= 0 else -1
        slot0 += max(0, m - 2)
    return out


def with_caterpillars(case):
    """every lineage of three and more members starts as a caterpillar; a lineage of two as its one edge"""
    groups = members_of(case["clone"])
    local = {}
    for key, members in groups.items():
        m, root = len(members), root_of(case, members)
        local[key] = caterpillar(m, root) if m >= 3 else ([-1] if m == 1 else [-1 if v == root else root for v in range(2)])
    return dict(case, start=start_slots(case, local))


def plain(case, max_rounds=0):
    return dict(case, start=None, max_rounds=max_rounds)


def mixed_random(seed):
    """lineages of K.MIXED_SIZES members with non-additive windows, interleaved: they finish in different rounds"""
    rng = np.random.default_rng(seed)
    return K.assemble([(K.random_windows(m, 60 + 7 * i, rng, wild=0.05, per_member=0.2), None) for i, m in enumerate(K.MIXED_SIZES)], rng, loose=5, shuffle=True)


def gpu_cases():
    """name -> builder of every case test_gpu_tree_mp.py runs; test_tree_mp_cpu.py checks that each reaches the edge it is named for"""
    bound = header_constant("VDJX_NJ_LDS_MEMBERS")
    out = {f"m{m}": (lambda m=m: plain(K.infinite_sites(m, 100 + m))) for m in (1, 2, 3)}
    out.update({
        "m4_nj": lambda: plain(K.random_case(4, 30, 31)),
        "m4_cat": lambda: with_caterpillars(K.infinite_sites(4, 104)),
        "m5_nj": lambda: plain(K.random_case(5, 40, 32)),
        "m5_cat": lambda: with_caterpillars(K.infinite_sites(5, 105)),
        "w1": lambda: with_caterpillars(K.random_case(6, 1, 33)),
        "w64": lambda: with_caterpillars(K.infinite_sites(12, 34, w=64)),
        "w65": lambda: with_caterpillars(K.infinite_sites(12, 35, w=65)),
        "w513": lambda: with_caterpillars(K.infinite_sites(20, 16, w=513)),
        "cat20": lambda: with_caterpillars(K.infinite_sites(20, 5)),
        "cat130": lambda: with_caterpillars(K.infinite_sites(130, 36)),
        "lds_bound": lambda: plain(K.infinite_sites(bound, 11)),
        "lds_bound_plus1": lambda: plain(K.infinite_sites(bound + 1, 12)),
        "random_wild": lambda: plain(K.random_case(40, 100, 18, wild=0.1)),
        "random_12": lambda: plain(K.random_case(12, 60, 3)),
        "identical": lambda: plain(K.identical(7, 19)),
        "identical_cat": lambda: with_caterpillars(K.identical(7, 19)),
        "many_small": lambda: plain(K.many_small(3000, 20)),
        "mixed": lambda: with_caterpillars(K.mixed(21)),
        "mixed_random": lambda: plain(mixed_random(22)),
        "one_round": lambda: dict(with_caterpillars(K.mixed(21)), max_rounds=1),
    })
    return {k: (lambda f=f: dict({"max_rounds": 0}, **f())) for k, f in out.items()}
