"""The model of vdjx_tree_split_support and vdjx_tree_split_compare (include/vdjx.h) in plain Python: the windows and the joining are
tests/tree_nj_model.py's, the keep rule is tests/tree_support_model.py's.  A clade is a Python frozenset of local leaf ids read off a
ROOTED tree (the leaves below a node), and matching is equality of sets: no bitsets, no signatures, no complementing -- none of the
implementation's shortcuts.  Nothing here is shared with the device code.

What the tests need to know about the implementation's route -- whether a join's clade held the root and had to be complemented, whether
a replicate kept no column of a lineage -- is reported next to the result ("reach") and takes no part in it."""
import numpy as np

from tests import tree_nj_model as N
from tests import tree_support_model as S
from tests.tree_model import distance_matrix, members_of, windows

FIELDS = ["members", "clones", "largest_clone", "replicates", "batches", "units", "scored", "matched", "full", "joins", "cells"]
M64 = (1 << 64) - 1


def root_of(members, prio):
    return min(range(len(members)), key=lambda p: (int(prio[members[p]]) if prio is not None else 0, members[p]))


def clades_of(m, root, parent):
    """local parents of a rooted lineage tree (the root's is -1) -> {inferred node: frozenset of the leaves below it}"""
    below = {v: set() for v in range(m, len(parent))}
    for leaf in range(m):
        v = leaf
        while v != root:
            v = parent[v]
            if v >= m:
                below[v].add(leaf)
    return {v: frozenset(s) for v, s in below.items()}


def scored_nodes(m, root, parent):
    """the inferred nodes other than the root's child, of a lineage of four and more"""
    if m < 4:
        return []
    return [v for v in range(m, 2 * m - 2) if parent[v] != root]


def local_parents(parent, members, slot0):
    """the lineage's nodes of parent[] (output slots) as local ids; -1 for the root; asserts that nothing points outside"""
    m = len(members)
    local = {s: v for v, s in enumerate(members)}
    local.update({slot0 + j: m + j for j in range(max(0, m - 2))})
    out = []
    for v in range(m + max(0, m - 2)):
        p = int(parent[members[v] if v < m else slot0 + v - m])
        out.append(local[p] if p >= 0 else -1)
    return out


def replicate_windows(ws, seed, r):
    at = [q for q in range(len(ws[0])) if S.keeps(seed, r, q)]
    return ["".join(s[q] for q in at) for s in ws], at


def replicate_tree(ws, m, root, seed, r):
    """-> (local parents of replicate r's tree, the join-sense clades that hold the root, the kept positions)"""
    sub, at = replicate_windows(ws, seed, r)
    D = distance_matrix(sub) if at else np.zeros((m, m), np.int32)
    edges = N.nj_edges([[int(x) << N.SHIFT for x in row] for row in D]) if m > 1 else []
    par, _, _, _ = N.orient(m, edges, root)
    flipped = 0                                             # (reach only) joins whose union of children holds the root
    if m >= 4:
        made = {}
        for j in range(m - 3):
            kids = [edges[2 * j][0], edges[2 * j + 1][0]]
            assert edges[2 * j][1] == edges[2 * j + 1][1] == m + j
            made[m + j] = frozenset().union(*[made[c] if c >= m else {c} for c in kids])
            flipped += root in made[m + j]
    return par, flipped, at


def batches_under(sizes, knob):
    count, cells = 0, 0
    for m in sizes:
        if cells and cells + m * m > knob:
            count, cells = count + 1, 0
        cells += m * m
    return count + (cells > 0)


def split_support(contigs, clone, anchor, parent, prio=None, replicates=100, seed=1, cells_knob=1 << 26):
    """-> {"support": int32[nodes], "trees": int32[B, nodes], "info": dict(FIELDS), "reach": dict}"""
    n = len(contigs)
    assert 1 <= replicates <= 1024 and 0 <= seed <= M64
    cs = [c.decode("latin-1") if isinstance(c, (bytes, bytearray)) else c for c in contigs]
    groups = members_of(clone)
    nodes = n + sum(max(0, len(v) - 2) for v in groups.values())
    assert len(parent) == nodes
    support = np.full(nodes, -1, np.int32)
    trees = np.full((replicates, nodes), -1, np.int32)
    info = dict.fromkeys(FIELDS, 0)
    reach = {"flipped": 0, "empty": 0, "per_lineage": {}}
    slot0 = n
    sizes = []
    for key in sorted(groups):
        members = groups[key]
        m = len(members)
        assert m <= N.MAX_MEMBERS
        ws, _ = windows(cs, members, anchor)
        root = root_of(members, prio)
        slot = lambda v: members[v] if v < m else slot0 + v - m
        lp = local_parents(parent, members, slot0)
        assert lp[root] == -1
        mine = clades_of(m, root, lp)
        scored = scored_nodes(m, root, lp)
        assert len(scored) == max(0, m - 3) and len({mine[v] for v in scored}) == len(scored)
        count = {v: 0 for v in scored}
        for r in range(1, replicates + 1):
            par, flipped, at = replicate_tree(ws, m, root, seed, r)
            for v, p in enumerate(par):
                trees[r - 1][slot(v)] = slot(p) if p >= 0 else -1
            if m < 4:
                continue
            theirs = set(clades_of(m, root, par).values())
            for v in scored:
                count[v] += mine[v] in theirs
            reach["flipped"] += flipped
            reach["empty"] += not at
        for v in scored:
            support[slot(v)] = count[v]
        reach["per_lineage"][key] = {"m": m, "root": root, "w": len(ws[0]), "support": [count[v] for v in scored]}
        if m >= 4:
            sizes.append(m)
            info["scored"] += m - 3
        slot0 += max(0, m - 2)
    got = support[support >= 0]
    info.update(members=sum(len(v) for v in groups.values()), clones=len(groups), largest_clone=max([len(v) for v in groups.values()] or [0]),
                replicates=replicates, units=replicates * len(sizes), batches=batches_under(sizes * replicates, cells_knob),
                matched=int(got.sum()), full=int((got == replicates).sum()), joins=replicates * sum(m - 3 for m in sizes),
                cells=replicates * sum(m * m for m in sizes))
    return {"support": support, "trees": trees, "info": info, "reach": reach}


def split_compare(clone, parent_a, parent_b):
    """-> {"shared": int32[nodes], "info": dict(shared, scored, rf)}; a lineage's root in a tree is its member without a parent, and the
    clades of both trees are the sides of their edges that do not hold tree a's root"""
    n = len(clone)
    groups = members_of(clone)
    nodes = n + sum(max(0, len(v) - 2) for v in groups.values())
    assert len(parent_a) == len(parent_b) == nodes
    out = np.full(nodes, -1, np.int32)
    slot0 = n
    for key in sorted(groups):
        members = groups[key]
        m = len(members)
        if m >= 4:
            la, lb = local_parents(parent_a, members, slot0), local_parents(parent_b, members, slot0)
            ra, rb = [[v for v in range(m) if lp[v] < 0] for lp in (la, lb)]
            assert len(ra) == len(rb) == 1
            everyone = frozenset(range(m))
            side = lambda c: everyone - c if ra[0] in c else c
            theirs = {side(c) for v, c in clades_of(m, rb[0], lb).items() if lb[v] != rb[0]}
            for v, c in clades_of(m, ra[0], la).items():
                if la[v] != ra[0]:
                    out[slot0 + v - m] = side(c) in theirs
        slot0 += max(0, m - 2)
    scored, shared = int((out >= 0).sum()), int((out == 1).sum())
    return {"shared": out, "info": {"shared": shared, "scored": scored, "rf": 2 * (scored - shared)}}


def newick_names(names, n, support, replicates):
    """tree_nj_model.node_ids' names with the support labels of annot.tree_nj_newick"""
    return [f"{x}/%.4f" % (int(support[s]) / replicates) if s >= n and support[s] >= 0 else x for s, x in enumerate(names)]
