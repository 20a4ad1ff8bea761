"""The cases tests/test_lineage_link_cpu.py and tests/test_gpu_lineage_link.py share: name -> (junctions, group, (num, den), table name or
None, symmetry).  The handmade ones are written with the partitions they must give; the size cases hold one single-linkage component of
exactly the size they are named for (63, 64, 65: the row block of k_link_matrix; 87, 88, 89: LINK_LDS_M, where k_link_merge leaves LDS for
the workspace; 300: more clusters than k_link_merge has threads); the rest vary the arithmetic.  Every model result is computed once."""
import functools

import numpy as np

from tests import lineage_dist_cases as LC
from tests import lineage_link_model as KM
from tests import lineage_model as M

LDS_M = 88                                                   # LINK_LDS_M of vdjx_lineage.hip
SIZES = [63, 64, 65, LDS_M - 1, LDS_M, LDS_M + 1, 300]
RANDOM = 20
LINKAGES = ("complete", "average")

_A20 = "A" * 20
TIE = [_A20, "CC" + _A20[2:], "CCCC" + _A20[4:]]            # d(a, b) = d(b, c) = 2, d(a, c) = 4, linked up to 2
_A25 = "A" * 25
EQUAL = [_A25, "C" + _A25[1:], "ACC" + _A25[3:]]            # d(a, b) = 1, d(a, c) = 2, d(b, c) = 3 at 0.1 of 25: the mean of 2 and 3 is the cut itself

# name -> {linkage: partition as sorted lists of item indices}
HANDMADE = {
    "component_of_2": {"complete": [[0, 1], [2]], "average": [[0, 1], [2]]},
    "tie": {"complete": [[0, 1], [2]], "average": [[0, 1], [2]]},
    "tie_reversed": {"complete": [[0, 1], [2]], "average": [[0, 1], [2]]},      # (items c, b, a: {c, b}, {a} -- the order decides a tie)
    "exact_equality": {"complete": [[0, 1], [2]], "average": [[0, 1, 2]]},
    "identical": {"complete": [list(range(10))], "average": [list(range(10))]},
    "identical_with_n": {"complete": [list(range(10))], "average": [list(range(10))]},
}


def _component(rng, m, L=48, far=5):
    """a family of exactly m around one founder, 1 .. 5 substitutions each (every member within 7 of the founder: one single-linkage
    component at 0.15, with pairs past the cut), and a second family of `far` in the same bucket"""
    founder = LC._rand(rng, L)
    out = [founder]
    while len(out) < m:
        k = int(rng.integers(1, 6))
        out.append(LC._subst(rng, founder, sorted(rng.choice(L, size=k, replace=False).tolist())))
    other = "".join({"A": "C", "C": "G", "G": "T", "T": "A"}[ch] for ch in founder)
    out += [LC._subst(rng, other, sorted(rng.choice(L, size=int(rng.integers(0, 4)), replace=False).tolist())) for _ in range(far)]
    order = rng.permutation(len(out)).tolist()
    return [out[i] for i in order]


def _repertoire(rng):
    """a few buckets of up to ~200 junctions: families of several sizes and depths, loners, a few N"""
    js, grp = [], []
    for g in range(int(rng.integers(2, 5))):
        L = int(rng.choice([12, 30, 33, 45, 64, 70]))
        room = int(rng.integers(20, 200))
        while room > 0:
            m = min(room, int(rng.choice([1, 1, 2, 3, 8, 20, 60])))
            fam = LC._family(rng, LC._rand(rng, L), m, frac=float(rng.choice([0.05, 0.12, 0.25])))
            if rng.integers(0, 4) == 0:
                fam[-1] = fam[-1][:L // 2] + "N" + fam[-1][L // 2 + 1:]
            js += fam
            grp += [g] * m
            room -= m
    order = rng.permutation(len(js)).tolist()
    grp = [grp[i] if rng.integers(0, 25) else M.NONE for i in order]
    return [js[i] for i in order], grp


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(40404)
    out = {}
    out["component_of_2"] = (["ACGTACGTAC", "ACGTACGTAA", "TTTTTTTTTT"], [0, 0, 0], (1000, 10000), None, "avg")
    out["tie"] = (TIE, [0, 0, 0], (1000, 10000), None, "avg")
    out["tie_reversed"] = (TIE[::-1], [0, 0, 0], (1000, 10000), None, "avg")
    out["exact_equality"] = (EQUAL, [0, 0, 0], (1000, 10000), None, "avg")
    out["identical"] = (["ACGTTGCAACGT"] * 10, [3] * 10, (1000, 10000), None, "avg")
    out["identical_with_n"] = (["ACGTTNCAACGT"] * 10, [3] * 10, (1000, 10000), None, "avg")
    fam = LC._family(rng, LC._rand(rng, 30), 12) + [LC._rand(rng, 30)] * 3
    out["num_0"] = (fam + fam[:4], [0] * len(fam) + [0] * 4, (0, 10000), None, "avg")
    out["num_is_den"] = (fam + [LC._rand(rng, 30) for _ in range(5)], [0] * (len(fam) + 5), (7, 7), None, "avg")
    out["chain_40"] = (["C" * i + "A" * (40 - i) for i in range(40)], [0] * 40, (500, 10000), None, "avg")
    a, b = _component(rng, 20, L=36), _component(rng, 17, L=36)
    js, grp = [], []
    for i in range(max(len(a), len(b))):                    # two buckets of one length interleaved, every fifth item takes no part
        for g, fam_ in ((0, a), (1, b)):
            if i < len(fam_):
                js.append(fam_[i])
                grp.append(M.NONE if len(js) % 5 == 0 else g)
    out["none_and_interleaved"] = (js, grp, (1500, 10000), None, "avg")
    for m in SIZES:
        out[f"size_{m}"] = (_component(rng, m), [0] * (m + 5), (1500, 10000), None, "avg")
    js, grp = _repertoire(rng)
    for tab in ("uniform", "realistic", "extreme"):
        out[f"table_{tab}"] = (js, grp, (1500, 10000), tab, "avg")
    out["table_realistic_min"] = (js, grp, (1500, 10000), "realistic", "min")
    out["table_extreme_min"] = (js, grp, (2500, 10000), "extreme", "min")
    out["table_size_89"] = (out["size_89"][0], out["size_89"][1], (1500, 10000), "realistic", "avg")
    for k in range(RANDOM):
        js, grp = _repertoire(rng)
        out[f"random_{k}"] = (js, grp, (int(rng.choice([800, 1500, 2500])), 10000), "realistic" if k % 4 == 3 else None, "avg")
    return out


BATCHED = "random_0"                                         # several components: VDJX_LINK_CELLS splits them


def table_of(tab):
    return None if tab is None else LC.tables()[tab]


@functools.lru_cache(maxsize=None)
def model(name, linkage, knob=KM.CELLS):
    js, grp, md, tab, sym = cases()[name]
    return KM.lineage(js, grp, md, linkage, table_of(tab), sym, knob)


def component_sizes(name):
    """the single-linkage components of two and more of a case, in their order"""
    single = model(name, "single")[0]
    return [int(c) for c in np.bincount(single[single >= 0]) if c >= 2]


def splitting_knob(name):
    """a VDJX_LINK_CELLS that cuts the case's components into several batches and still holds more than one of them somewhere"""
    sizes = component_sizes(name)
    return max(m * m for m in sizes) + min(m * m for m in sizes)
