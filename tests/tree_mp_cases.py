"""Seeded inputs for the tests of vdjx_tree_mp: the builders of tests/tree_nj_cases.py, and caterpillar start trees.  A case is
tree_nj_cases' dict plus "start" (int32[nodes] parents in output slots, or None for vdjx_tree_nj's tree) and "max_rounds".

caterpillar(m, root): the leaves other than the root, ascending, are l_0 .. l_(m-2); inferred node m + j has the children l_j and
m + j + 1, the last inferred node l_(m-3) and l_(m-2); the root's child is m.  Far from any good tree: the search has a long way to go,
and its paths to the root are as long as the lineage.

The stride and pick cases are cut to two constants of vdjx_mp.hip, read from the file by kernel_constant: scorer_grid restates the
host's formula for k_mp_score's grid, candidate_index the order in which k_mp_pick numbers a lineage's candidates."""
import numpy as np

from tests import tree_nj_cases as K
from tests.tree_model import members_of, windows

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


def kernel_constant(name):
    """a #define of vdjer_amd/csrc/vdjx_mp.hip as an int: the cases below are cut to the scorer's and the picker's constants, and the CPU
    tests recompute from the file what they reach"""
    return K.kernel_constant("vdjx_mp.hip", name)


def stride_all_raw(seed=37):
    """2,100 lineages of 7 members with windows of 130 .. 190 columns (three column tiles each), interleaved: 16,800 candidates, more
    than MP_FILL_WAVES, so the scorer's grid is one wave high and every wave walks all three tiles"""
    rng = np.random.default_rng(seed)
    lin = [(K.random_windows(7, int(rng.integers(130, 191)), rng, wild=0.03, per_member=0.2), None) for _ in range(2100)]
    return K.assemble(lin, rng, loose=50, shuffle=True)


def stride_mixed_raw(seed=38):
    """1,200 lineages of 6 .. 8 members with windows of 20 .. 320 columns (one to five column tiles), interleaved: between MP_FILL_WAVES
    / 2 and MP_FILL_WAVES candidates, so the grid is two waves high -- tiles 0, 2, 4 and tiles 1, 3, and nothing for the second wave of a
    one-tile lineage"""
    rng = np.random.default_rng(seed)
    lin = [(K.random_windows(int(rng.integers(6, 9)), int(rng.integers(20, 321)), rng, wild=0.03, per_member=0.2), None) for _ in range(1200)]
    return K.assemble(lin, rng, loose=50, shuffle=True)


def sample_of(case, count, seed):
    """the case cut down to `count` of its lineages, chosen by seed, and its loose items: keys, member order, anchors and prio as they
    are, so every kept lineage has the tree it has in the whole case (no start: apply with_caterpillars or plain afterwards)"""
    keys = sorted(members_of(case["clone"]))
    rng = np.random.default_rng(seed)
    kept = set(int(keys[i]) for i in rng.permutation(len(keys))[:count]) | {-1}
    idx = [i for i, k in enumerate(case["clone"]) if int(k) in kept]
    return {"contigs": [case["contigs"][i] for i in idx], "clone": case["clone"][idx], "anchor": case["anchor"][idx], "prio": case["prio"][idx], "gen": {}}


def lineage_windows(case):
    """key -> the lineage's windows, for every lineage"""
    return {key: windows(case["contigs"], members, case["anchor"])[0] for key, members in members_of(case["clone"]).items()}


def scorer_grid(case):
    """(n_cand, the column tiles of every searched lineage in key order, grid_y) of k_mp_score for the case in one batch, by the host's
    own formulas: 2 (m - 3) candidates per lineage of four and more, ceil(w / 64) tiles, and a grid as high as fills MP_FILL_WAVES waves
    but no higher than the most tiles of a searched lineage"""
    fill = kernel_constant("MP_FILL_WAVES")
    ws = lineage_windows(case)
    searched = [key for key in sorted(ws) if len(ws[key]) > 3]
    n_cand = sum(2 * (len(ws[key]) - 3) for key in searched)
    tiles = [(len(ws[key][0]) + 63) // 64 for key in searched]
    return n_cand, tiles, (min(max(tiles), (fill + n_cand - 1) // n_cand) if n_cand else 1)


def candidate_index(m, root_kid, v, k):
    """the index k_mp_pick reduces: v's position among the inferred nodes other than the root's child, ascending, times 2, plus k
    (mp_cand_node's inverse)"""
    assert v >= m and v != root_kid
    return 2 * (v - m - (v > root_kid)) + k


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
        # k_mp_score: a wave over several column tiles (grid_y below the most tiles); k_mp_pick: more candidates than threads
        "stride_all": lambda: plain(stride_all_raw()),
        "stride_mixed": lambda: with_caterpillars(stride_mixed_raw()),
        "pick_cat140": lambda: with_caterpillars(K.infinite_sites(140, 39)),
        "pick_random300": lambda: plain(K.random_case(300, 400, 40, wild=0.05)),
        "widths": lambda: plain(K.widths(23)),
    })
    return {k: (lambda f=f: dict({"max_rounds": 0}, **f())) for k, f in out.items()}
