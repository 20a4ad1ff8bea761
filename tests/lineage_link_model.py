"""The model of vdjx_lineage_link (include/vdjx.h) in plain Python and numpy: complete and average linkage cut at the threshold, agglomerated
naively over WHOLE buckets -- every step looks at every pair of live clusters, O(m^3) -- so that it checks the device's claim that only the
single-linkage components need agglomerating instead of sharing it.  The distances are tests/lineage_model.py's and
tests/lineage_dist_model.py's; nearest and the single-linkage info are theirs too.  Nothing here is shared with the C or HIP code."""
import numpy as np

from tests import lineage_dist_model as LM
from tests import lineage_model as M

LINKAGE = ("single", "complete", "average")
MAX_M = 4096                                                 # members of a single-linkage component under complete or average linkage
CELLS = 1 << 26                                              # VDJX_LINK_CELLS' default
LINK_FIELDS = ["components", "largest_component", "merges", "clones_single", "batches", "cells"]


def agglomerate(D, K, den, linkage):
    """D: int[m, m] of one bucket in the caller's order, K = unit * num * L -> (label[m]: the smallest member (a position in the bucket) of
    every position's final cluster, merges).  The rule: among the eligible pairs of clusters with id(A) < id(B) the smallest under (delta,
    id(A), id(B)) is merged and keeps id(A), until none is eligible"""
    assert linkage in (1, 2)
    m = D.shape[0]
    S = np.array(D, dtype=np.int64)                          # complete: the maximum; average: the sum over the cross pairs
    size = np.ones(m, np.int64)
    label = np.arange(m)
    upper = np.triu(np.ones((m, m), bool), 1)
    merges = 0
    while True:
        live = size > 0
        n = np.outer(size, size) if linkage == 2 else np.ones((m, m), np.int64)
        ok = upper & live[:, None] & live[None, :] & (S <= K * n // den)      # S den <= K n for an integer S; K n < 2^61, where S den may pass 2^63
        if not ok.any():
            return label, merges
        cand = np.argwhere(ok)                               # row-major: (id(A), id(B)) ascending
        if linkage == 1:
            v = S[ok]
            a, b = cand[v == v.min()][0]
        else:
            q = S[ok] / n[ok]                                # a float only narrows the field; the decision is exact below
            near = cand[q <= q.min() * (1 + 1e-9) + 1e-9]
            a, b = min(((int(i), int(j)) for i, j in near),
                       key=lambda p: _Frac(int(S[p]), int(n[p]), p))
        a, b = int(a), int(b)
        new = np.maximum(S[a], S[b]) if linkage == 1 else S[a] + S[b]
        S[a, :] = new
        S[:, a] = new
        size[a] += size[b]
        size[b] = 0
        label[label == b] = a
        merges += 1


class _Frac:
    """S / n compared exactly (S1 n2 against S2 n1 in Python integers), then the pair"""

    def __init__(self, s, n, pair):
        self.s, self.n, self.pair = s, n, pair

    def __lt__(self, o):
        l, r = self.s * o.n, o.s * self.n
        return l < r if l != r else self.pair < o.pair


def batches(sizes, knob=CELLS):
    """whole components, in order, in batches of at most `knob` cells (m * m each); a component of more cells goes alone -> the number"""
    count, cur = 0, 0
    for m in sizes:
        if cur and cur + m * m > knob:
            count, cur = count + 1, 0
        cur += m * m
    return count + (1 if sizes else 0)


def lineage(junctions, group, max_dist=M.DEFAULT, linkage="complete", table=None, symmetry="avg", knob=CELLS):
    """-> (clone int32[n], nearest int32[n], info dict, link dict).  linkage: a name of LINKAGE or 0 .. 2"""
    linkage = LINKAGE.index(linkage) if isinstance(linkage, str) else int(linkage)
    num, den = max_dist
    n = len(junctions)
    js = [j.decode("latin-1") if isinstance(j, (bytes, bytearray)) else j for j in junctions]
    if table is None:
        single, nearest, info = M.lineage(js, group, max_dist)
    else:
        single, nearest, info, _ = LM.lineage(js, group, table, max_dist, symmetry)
    comp = np.bincount(single[single >= 0], minlength=info["clones"]).tolist() if n else []
    comp = [c for c in comp if c >= 2]                       # (single's numbers are in the order of the smallest member)
    link = dict(components=len(comp), largest_component=max(comp or [0]), merges=0, clones_single=info["clones"], batches=0, cells=0)
    if linkage == 0:
        return single, nearest, info, dict.fromkeys(LINK_FIELDS, 0)
    assert max(comp or [0]) <= MAX_M
    link.update(batches=batches(comp, knob), cells=sum(c * c for c in comp))
    buckets = {}
    for i in range(n):
        if int(group[i]) != M.NONE:
            buckets.setdefault((int(group[i]), len(js[i])), []).append(i)
    root = np.full(n, -1, np.int64)
    for (_, L), members in buckets.items():
        sub = [js[i] for i in members]
        D = M.distance_matrix(sub) if table is None else LM.distance_matrix(sub, table, symmetry)[0]
        label, merges = agglomerate(D, (1 if table is None else 2000) * num * L, den, linkage)
        link["merges"] += merges
        for k, i in enumerate(members):
            root[i] = members[int(label[k])]
    clone = np.full(n, -1, np.int32)
    number = {}
    for i in range(n):
        if root[i] < 0:
            continue
        r = int(root[i])
        if r not in number:
            assert r == i
            number[r] = len(number)
        clone[i] = number[r]
    return clone, nearest, dict(info, clones=len(number)), link


def link_line(linkage, info, link):
    """the stderr line of `vdjer --lineage-link complete|average`"""
    return (f"lineage link: {linkage}, {link['components']} components of two and more (largest {link['largest_component']}), {link['merges']} merges, "
            f"{info['clones']} lineages of {link['clones_single']} under single linkage, {link['batches']} batches")
