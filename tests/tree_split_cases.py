"""Seeded inputs for the tests of vdjx_tree_split_support: the builders of tests/tree_nj_cases.py and tests/tree_mp_cases.py, a scored tree
from one of the models, a replicate count and a seed.  A case is tree_nj_cases' dict plus "parent" (int32[nodes] in output slots),
"replicates" and "seed".  No case has a lineage of more than 129 members or more than 16 replicates.

The root of a lineage is its member of smallest (prio, index): with_root gives one member priority 0 and the others 1, so the root's
local id is the case's choice -- 0, m - 1 or the middle.  tests/test_tree_split_cpu.py checks with the model that every case reaches what
it is named for."""
import functools

import numpy as np

from tests import tree_mp_cases as MK
from tests import tree_mp_model as MP
from tests import tree_nj_cases as K
from tests import tree_nj_model as N
from tests.tree_model import members_of

SPLIT_KNOB = 2500                                           # a VDJX_NJ_CELLS that cuts a replicate of `mixed` between its lineages


def with_root(case, where):
    """where: "first", "last" or "middle" -- the local id of every lineage's root"""
    prio = np.ones(len(case["contigs"]), np.uint32)
    for members in members_of(case["clone"]).values():
        prio[members[{"first": 0, "last": len(members) - 1, "middle": len(members) // 2}[where]]] = 0
    return dict(case, prio=prio)


def scored_nj(case):
    return N.tree_nj(case["contigs"], case["clone"], case["anchor"], case["prio"], ancestors=False)["parent"]


def scored_mp(case):
    return MP.tree_mp(case["contigs"], case["clone"], case["anchor"], case["prio"], ancestors=False)["parent"]


def scored_caterpillar(case):
    return MK.with_caterpillars(case)["start"]


def make(case, tree, replicates, seed):
    return dict(case, parent=np.asarray(tree(case), np.int32), replicates=replicates, seed=seed)


def n_column(m, w, seed):
    """random windows in which one column is N in every member and another in one member alone"""
    rng = np.random.default_rng(seed)
    ws = [list(s) for s in K.random_windows(m, w, rng, per_member=0.2)]
    for s in ws:
        s[w // 2] = "N"
    ws[1][3] = "N"
    return K.assemble([(["".join(s) for s in ws], None)], rng)


def several(sizes, seed, w=40):
    """one lineage per size, random windows of w .. w + 7 * count columns, interleaved, with loose items"""
    rng = np.random.default_rng(seed)
    return K.assemble([(K.random_windows(m, w + 7 * i, rng, wild=0.03, per_member=0.2), None) for i, m in enumerate(sizes)], rng, loose=3, shuffle=True)


WIDE = 1100                                                 # about 550 kept columns: more than 16 packed words, the matrix kernel's chunked path


def gpu_cases():
    """name -> builder of every case test_gpu_tree_split.py runs"""
    out = {
        # the sizes: no scored node up to three members, one at four; 63 / 64 / 65 the LDS and the global join, one and two words per clade
        "small_sizes": lambda: make(with_root(several([1, 2, 3, 4, 5], 51), "first"), scored_nj, 8, 1),
        "m63_first": lambda: make(with_root(K.random_case(63, 120, 52, wild=0.03), "first"), scored_nj, 4, 2),
        "m64_last": lambda: make(with_root(K.random_case(64, 120, 53, wild=0.03), "last"), scored_nj, 4, 3),
        "m65_middle": lambda: make(with_root(K.random_case(65, 120, 54, wild=0.03), "middle"), scored_nj, 4, 4),
        "m128_last": lambda: make(with_root(K.infinite_sites(128, 55), "last"), scored_nj, 3, 5),
        "m129_last": lambda: make(with_root(K.infinite_sites(129, 56), "last"), scored_nj, 3, 6),
        "m129_first": lambda: make(with_root(K.random_case(129, 200, 57), "first"), scored_nj, 2, 7),
        # the trees that are scored
        "caterpillar": lambda: make(with_root(K.infinite_sites(12, 58), "middle"), scored_caterpillar, 16, 8),
        "caterpillar_70": lambda: make(with_root(K.infinite_sites(70, 59), "last"), scored_caterpillar, 3, 9),
        "mp_tree": lambda: make(MK.mixed_random(22), scored_mp, 6, 10),
        "infinite_sites_20": lambda: make(with_root(K.infinite_sites(20, 60), "middle"), scored_nj, 16, 11),
        # the windows' contents
        "identical": lambda: make(K.identical(7, 19), scored_nj, 4, 12),
        "n_column": lambda: make(with_root(n_column(9, 40, 61), "last"), scored_nj, 8, 13),
        # one replicate; several batches (test_gpu_tree_split.py runs `mixed` under three knobs)
        "one_replicate": lambda: make(K.infinite_sites(10, 62), scored_nj, 1, 14),
        "mixed": lambda: make(K.mixed(21), scored_nj, 5, 15),
        f"w{WIDE}": lambda: make(with_root(K.random_case(6, WIDE, 63, wild=0.02), "middle"), scored_nj, 3, 16),
    }
    for i, w in enumerate((1, 3, 31, 32, 33, 64, 65, 513)):
        out[f"w{w}"] = lambda w=w, i=i: make(with_root(K.random_case(6, w, 70 + i), ("first", "last", "middle")[i % 3]), scored_nj, 8, 20 + i)
    return out


def last_word_pair(m=67):
    """two caterpillars over one lineage of m members (65 .. 128: two words per clade) rooted at member 0, whose leaf orders differ in
    the places of the leaves m - 3 and m - 2: every clade is the same but one, and that one differs in the last word only -- {m - 2, m - 1}
    against {m - 3, m - 1} -> (clone, parent_a, parent_b, the slot of the node that is not shared)"""
    assert 67 <= m <= 128
    clone = np.zeros(m, np.int32)

    def tree(order):
        parent = np.full(2 * m - 2, -1, np.int32)
        for j, leaf in enumerate(order[:-1]):
            parent[leaf] = m + j
            parent[m + j] = m + j - 1 if j else 0
        parent[order[-1]] = 2 * m - 3
        return parent

    a = list(range(1, m))
    b = a[:-3] + [a[-2], a[-3], a[-1]]
    return clone, tree(a), tree(b), 2 * m - 3


def bad_trees():
    """a lineage of five from the caterpillar -> (case with "start", {what: int32[nodes] parents that are no tree}): every way
    vdjx_tree_mp refuses a start"""
    case = MK.with_caterpillars(K.infinite_sites(5, 105))
    root = MK.root_of(case, list(range(5)))
    l = [v for v in range(5) if v != root]
    good = MK.caterpillar(5, root)

    def changed(v, x):
        p = list(good)
        p[v] = x
        return p
    cycle = [-1] * 8
    for v, p in [(5, root), (l[0], 5), (l[1], 5), (6, 7), (7, 6), (l[2], 6), (l[3], 7)]:
        cycle[v] = p                                        # every node has the children it should have
    local = {"a parent outside the lineage": changed(l[0], -1), "a root leaf with two children": changed(l[0], root),
             "an inferred node with three children": changed(l[3], 5), "a leaf with children": changed(l[3], l[0]), "a cycle": cycle}
    return case, {what: MK.start_slots(case, {0: p}) for what, p in local.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    return gpu_cases()[name]()


@functools.lru_cache(maxsize=None)
def want(name, knob=1 << 26):
    """the model's result of a case, computed once for all the tests of a run"""
    from tests import tree_split_model as M
    c = case(name)
    return M.split_support(c["contigs"], c["clone"], c["anchor"], c["parent"], c["prio"], c["replicates"], c["seed"], cells_knob=knob)
