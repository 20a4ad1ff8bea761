"""The inputs of tests/test_gpu_selection.py and their model results, shared with tests/test_selection_cpu.py (which asserts the margin
conditions of the GPU cases without a GPU).  Everything is seeded and computed once per process."""
from __future__ import annotations

import functools

import numpy as np

from tests import annot_model as A
from tests import selection_model as S
from tests import test_gpu_mutation as TM
from tests.test_gpu_mutation import H, NONE, V0, V1, V2, V3, V4, V5

LEN, CALL = TM.LEN, TM.CALL
PLEN = 2047                                                           # the posterior cases: contigs as long as the longest record
EDGE_P = 905                                                          # a 1-based position of V3: its codon (904 .. 906) is a CDR of its own


def hits(cs, key="v"):
    return TM._hits(cs, key)


# ---- the counts ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def count_cases():
    """test_gpu_mutation.cases() and one more call of 13: hits that reach record positions 1, 2, L - 1 and L, with and without an N, and 300
    bases of the 2,047-base record across its first CDR"""
    rng = np.random.default_rng(3131)
    g = TM.germs()
    out = list(TM.cases())

    def case(name, v=NONE, limit=LEN, edits=()):
        ct = list(TM._rand(rng, LEN))
        if v["gene"] >= 0:
            TM._lay(ct, v, g[v["gene"]])
        for q in edits:
            ct[q] = TM._other(ct[q])
        out.append(dict(name=name, contig="".join(ct), v=v, d=NONE, j=NONE, limit=limit))

    case("whole_v5", v=H(V5, 20, 1, [("M", 60)]), edits=[19, 20, 22, 40, 77, 78])
    case("whole_v1", v=H(V1, 5, 1, [("M", 90)]), edits=[4, 5, 30, 43, 44, 46, 92, 93])
    case("v3_cdr", v=H(V3, 1, 1700, [("M", 300)]), edits=sorted(rng.choice(300, 40, replace=False).tolist()))
    case("v3_cdr_limit", v=H(V3, 1, 1700, [("M", 300)]), limit=131, edits=sorted(rng.choice(300, 40, replace=False).tolist()))
    case("v0_split", v=H(V0, 3, 31, [("M", 20)]), edits=[2 + 3, 2 + 4, 2 + 5, 2 + 6, 2 + 9, 2 + 10])      # germline 31 .. 50, changed at 34 .. 37, 40, 41: the interval 35 .. 40 splits the codons 34 .. 36 and 40 .. 42
    case("v0_indel", v=H(V0, 3, 1, [("M", 34), ("I", 2), ("M", 30), ("D", 3), ("M", 60)]), edits=[10, 36, 40, 41, 70, 100])
    while len(out) % CALL:
        case(f"pad{len(out)}")
    return out


@functools.lru_cache(maxsize=None)
def region_map():
    """int32[11, 4]: intervals that split a codon (V0), run from base 1 to the record's last base (V1), are 0 0 (V2 and the second of
    others), lie across and at the end of the 2,047-base record (V3), and -1 for one V record (V5)"""
    m = np.zeros((11, 4), np.int32)
    m[V0] = (35, 40, 100, 120)
    m[V1] = (1, 90, 0, 0)
    m[V3] = (1800, 1850, 2000, 2047)
    m[V4] = (0, 0, 10, 30)
    m[V5] = -1
    return m


@functools.lru_cache(maxsize=None)
def weights(edge=False):
    """seeded weights up to 2^32 - 1 (uint32[1024, 4]); edge: the 5-mers around the three bases of EDGE_P's codon of V3 weigh 1 for one replacement
    and 0 otherwise"""
    rng = np.random.default_rng(4242)
    w = rng.integers(0, 1 << 32, (1024, 4), dtype=np.uint64).astype(np.uint32)
    w[rng.integers(0, 1024, 40)] = 0xFFFFFFFF
    if edge:
        g = TM.germs()[V3]
        cod = (EDGE_P - 1) // 3
        for p in (3 * cod, 3 * cod + 1, 3 * cod + 2):
            idx = 0
            for ch in g[p - 2:p + 3]:
                idx = 4 * idx + "ACGT".index(ch)
            w[idx] = 0
        p, alt = edge_sites()[0]
        idx = 0
        for ch in g[p - 2:p + 3]:
            idx = 4 * idx + "ACGT".index(ch)
        w[idx, "ACGT".index(alt)] = 1
    return w


@functools.lru_cache(maxsize=None)
def count_model(weighted, mapped):
    cs = count_cases()
    return S.counts([c["contig"] for c in cs], hits(cs), [c["limit"] for c in cs], TM.germs(), region_map() if mapped else None,
                    weights() if weighted else None)


# ---- the posterior --------------------------------------------------------------------------------------------------------------------------
def _sites(rec):
    """the single-base changes of a record by class -> {"R": [(p 0-based, alt)], "S": [...]}, codons without a stop only, one per codon"""
    out = {"R": [], "S": []}
    for cod in range(len(rec) // 3):
        gc = rec[3 * cod:3 * cod + 3]
        if any(ch not in "ACGT" for ch in gc) or A.translate(gc) == "*":
            continue
        for kind in ("R", "S"):
            for b in range(3):
                found = False
                for alt in "ACGT":
                    if alt == gc[b]:
                        continue
                    ma = A.translate(gc[:b] + alt + gc[b + 1:])
                    if ma != "*" and (ma == A.translate(gc)) == (kind == "S"):
                        out[kind].append((3 * cod + b, alt))
                        found = True
                        break
                if found:
                    break
    return out


@functools.lru_cache(maxsize=None)
def edge_sites():
    """two replacements (no stop) at two positions of the V3 codon that is the one-codon CDR -> [(p 0-based, alt)] * 2; the first one is the
    only change the edge weights give any weight"""
    g = TM.germs()[V3]
    cod = (EDGE_P - 1) // 3
    gc = g[3 * cod:3 * cod + 3]
    assert A.translate(gc) != "*"
    out = []
    for b in range(3):
        for alt in "ACGT":
            ma = A.translate(gc[:b] + alt + gc[b + 1:])
            if alt != gc[b] and ma != "*" and ma != A.translate(gc):
                out.append((3 * cod + b, alt))
                break
    assert len(out) >= 2, "no two replacements in the codon of EDGE_P: move it"
    return out[:2]


PGROUPS = 7                                                           # group 0 is empty; 1, 3, 4, 5 and 9 members; four contigs in no group


@functools.lru_cache(maxsize=None)
def posterior_cases(seed=77):
    """26 contigs of 2,047 bases -> (cases, group int32[26]): the most mutated hit (every base differs: n in the thousands), no mutation
    (n = 0), silent changes only (x = 0), replacements only (x = n), the one-codon CDR with two replacements and expected odds of 1 against the
    record's whole silent weight (the peak lies on the grid's edge), a V0 hit whose CDRs lie outside it (exp_r = 0 there), and seeded mixtures"""
    rng = np.random.default_rng(seed)
    g = TM.germs()
    st3, st0 = _sites(g[V3]), _sites(g[V0])
    out = []

    def member(name, gene, length, edits):
        ct = list(TM._rand(rng, PLEN))
        v = H(gene, 1, 1, [("M", length)])
        TM._lay(ct, v, g[gene])
        for p, alt in edits:
            ct[p] = alt
        out.append(dict(name=name, contig="".join(ct), v=v, d=NONE, j=NONE, limit=PLEN))

    def pick(sites, k, avoid=()):
        idx = rng.choice(len(sites), k, replace=False) if k else []
        return [sites[i] for i in idx if sites[i][0] // 3 not in avoid]

    ecod = (EDGE_P - 1) // 3
    member("most", V3, 2047, [(p, TM._other(ch)) for p, ch in enumerate(g[V3])])
    member("none", V3, 2047, [])
    member("silent", V3, 2047, pick(st3["S"], 5, (ecod,)))
    member("replaced", V3, 2047, pick(st3["R"], 7, (ecod,)))
    member("edge", V3, 2047, edge_sites() + pick(st3["S"], 3, (ecod,)))
    member("v0_outside", V0, 90, pick([s for s in st0["R"] if s[0] < 90], 3) + pick([s for s in st0["S"] if s[0] < 90], 2))
    while len(out) < 26:
        member(f"mix{len(out)}", V3, 2047, pick(st3["R"], int(rng.integers(0, 11)), (ecod,)) + pick(st3["S"], int(rng.integers(0, 11)), (ecod,)))
    #        most none silent replaced edge v0_outside, then the mixtures
    group = [1, 2, 2, 2, 3, 3] + [3, 3] + [4] * 5 + [5] * 9 + [-1, -7, -1, -1]
    assert len(group) == len(out) == 26
    return out, np.array(group, np.int32)


@functools.lru_cache(maxsize=None)
def posterior_map():
    m = np.zeros((11, 4), np.int32)
    m[V3] = (EDGE_P - 1, EDGE_P + 1, 0, 0)
    m[V0] = (200, 250, 300, 360)
    m[V5] = -1
    return m


@functools.lru_cache(maxsize=None)
def posterior_counts():
    cs, _ = posterior_cases()
    return S.counts([c["contig"] for c in cs], hits(cs), None, TM.germs(), posterior_map(), weights(True))


@functools.lru_cache(maxsize=None)
def posterior_model(one_group=False):
    """the rows of the posterior call -> [26 + G + 1][2] of selection_model.posterior's dicts; one_group: every contig in group 0 (G = 1)"""
    cs, group = posterior_cases()
    if one_group:
        return S.rows(posterior_counts(), 2, np.zeros(len(cs), np.int32), 1)
    return S.rows(posterior_counts(), 2, group, PGROUPS)
