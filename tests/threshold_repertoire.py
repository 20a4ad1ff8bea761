"""A second seeded repertoire for `vdjer --lineage-threshold`: few V gene / J gene pairs, one junction length, so that the buckets are
large -- in each, lineages of four (a founder and members one, two and three substitutions from it) and unrelated single clones that share
the bucket.  The distances to the nearest neighbour therefore have both modes: 1 .. 3 of 48 bases for the lineages' members, about half the
junction for the singles.  Built from the pieces of tests/families.py (private V and J sequences per clone, designed cores, no 35-mer shared
by two clones); nothing here is stored.

    build()            -> families.Families
    write_ref_dir, pool   tests/families.py's, which take it as they take their own"""
from __future__ import annotations

import functools

import numpy as np

from tests import families as F
from vdjer_amd import synth

SEED = 20261020
PAIRS = [("IGHV3-23", "IGHJ4"), ("IGHV1-18", "IGHJ6"), ("IGHV4-39", "IGHJ5")]
CODONS = 14                                              # junction: 3 + 42 + 3 = 48 bases, every clone
LINEAGES, STEPS, SINGLES = 4, [1, 2, 3], 8               # per pair: four lineages of four, eight singles


@functools.lru_cache(maxsize=None)
def build(seed: int = SEED) -> F.Families:
    rng = np.random.default_rng(seed)
    cl = []

    def clone(vgene, jgene, core, lineage=""):
        k = len(cl)
        cl.append(F.Clone([f"{vgene}*{k + 1:02d}"], [f"{jgene}*{100 + k}"], core, vgene, jgene, lineage))

    for p, (vgene, jgene) in enumerate(PAIRS):
        for t in range(LINEAGES):                            # as families.build's family(): one substitution beside the middle of the core
            f = F._core(rng, CODONS)
            L = len(f)
            free = [q for q in rng.permutation(L).tolist() if not L // 2 - 1 <= q <= L // 2 + 2 and 9 <= q < L - 10]
            for k, d in enumerate([0] + STEPS):
                pos = [L // 2 - 2 + k] + [free.pop() for _ in range(d - 1)] if d else []
                clone(vgene, jgene, F._subst(f, pos, rng), f"pair{p}_lineage{t}")
        for _ in range(SINGLES):
            clone(vgene, jgene, F._core(rng, CODONS))
    n = len(cl)
    v_germ = [F._v_germ(rng) for _ in range(n)]
    j_germ = [F._j_germ(rng) for _ in range(n)]
    clones = [v_germ[k] + c.core + j_germ[k] for k, c in enumerate(cl)]
    rep = synth.Repertoire(v_germ, j_germ, clones, list(range(n)), list(range(n)), np.full(n, 1.0 / n), seed)
    rep.v_anchors = [v[277:293] for v in v_germ]
    rep.j_anchors = [j[8:24] for j in j_germ]
    assert len(set(rep.v_anchors)) == n and len(set(rep.j_anchors)) == n and len({c.junction for c in cl}) == n
    fam = F.Families(rep, cl)
    fam.germline = [rec for k, c in enumerate(cl) for rec in ((c.v_names[0], v_germ[k], 0), (c.j_names[0], j_germ[k][:F.J_RECORD], 0))]
    return fam


def designed_distances(fam):
    """per clone the smallest non-zero Hamming distance to another junction of its (vgene, jgene) pair, and the junctions' length"""
    near = []
    for a in fam.clones:
        ds = [F.hamming(a.junction, b.junction) for b in fam.clones if b is not a and (b.vgene, b.jgene) == (a.vgene, a.jgene)]
        near.append(min(d for d in ds if d > 0))
    return near, [len(c.junction) for c in fam.clones]
