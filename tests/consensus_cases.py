"""The inputs of tests/test_gpu_consensus.py and their model results, shared with tests/test_consensus_cpu.py (which proves without a GPU that
every case reaches what it is for).  Everything is seeded and computed once per process.  The germlines are tests/test_gpu_mutation.py's: V0
(360 bases), V5 (60) and V3, the record of targeting_cases.HOT_LEN = 2,047 bases."""
from __future__ import annotations

import functools

import numpy as np

from tests import consensus_model as CM
from tests import targeting_cases as TC
from tests import test_gpu_mutation as TM
from tests.test_gpu_mutation import H, V0, V3, V5

LEN = TM.LEN
MOST_COMMON = (0, 1)
FREQS = (CM.DEFAULT, MOST_COMMON)
BIG_VOTERS = 300                                                      # more than one workgroup's 255
assert TC.HOT_LEN == len(TM.germs()[V3]) == 2047 and BIG_VOTERS > CM.SHARE


def hits(cs):
    return TM._hits(cs, "v")


def inputs(cs):
    return [c["contig"] for c in cs], hits(cs), np.array([c["limit"] for c in cs], np.int32), np.array([c["group"] for c in cs], np.int32)


def alt(ch, k=1):
    """the k-th other base after ch"""
    return "ACGT"[("ACGT".index(ch) + k) % 4]


# ---- the edges, one small group each -----------------------------------------------------------------------------------------------------------
P = 40                                                                # the record position (of V0) the column cases are about
PLAIN = H(V0, 5, 1, [("M", 90)])                                      # contig positions 5 .. 94 over record positions 0 .. 89


@functools.lru_cache(maxsize=None)
def edge_cases():
    """[dict(name, what, contig, v, limit, group)]; `what` names the edge, a group per edge.  A contig is its germline along the hit but for
    the characters given per record position"""
    rng = np.random.default_rng(6161)
    g = TM.germs()
    out = []
    groups = {}

    def member(what, v=PLAIN, put=(), limit=LEN, group=None):
        ct = list(TM._rand(rng, LEN))
        TM._lay(ct, v, g[v["gene"]])
        for p, ch in put:
            ct[TC._index(v, p)] = ch
        grp = groups.setdefault(what, 100 + 7 * len(groups)) if group is None else group
        out.append(dict(name=f"{what}{len(out)}", what=what, contig="".join(ct), v=v, limit=limit, group=grp))

    def column(what, symbols, p=P):
        for ch in symbols:
            member(what, put=[(p, ch)] if ch else [])

    g0 = g[V0][P]
    x, y = alt(g0, 1), alt(g0, 2)
    column("thr_3of5", [x, x, x, None, None])                        # 3 * 10000 == 6000 * 5: passes
    column("thr_5of9", [x] * 5 + [None] * 4)                         # 50000 < 54000
    column("thr_5of10", [x] * 5 + [None] * 3 + [y] * 2)              # the largest count, one vote short of 6 of 10
    column("thr_6of10", [x] * 6 + [None] * 2 + [y] * 2)
    column("tie_germ", [x, x, None, None])                           # mostCommon: the germline base
    column("tie_other", [x, x, y, y])                                # mostCommon: N
    # a tie of gap and base without the germline: two voters delete P, two show x
    gap_at = H(V0, 5, 1, [("M", P), ("D", 1), ("M", 40)])
    for _ in range(2):
        member("tie_gap", v=gap_at)
    for _ in range(2):
        member("tie_gap", put=[(P, x)])
    column("n_votes", ["N", "N", None])                              # cover 3, best 1: the germline base under mostCommon, N at 0.6
    column("all_n", ["N", "n", "R"])                                 # best 0
    # a hole: record positions 0 .. 29 and 40 .. 69
    member("hole", v=H(V0, 5, 1, [("M", 30)]))
    member("hole", v=H(V0, 9, 41, [("M", 30)]))
    # a deletion of two won (2 of 3) and lost (1 of 3)
    del2 = H(V0, 5, 1, [("M", 30), ("D", 2), ("M", 40)])
    for v in (del2, del2, PLAIN):
        member("del_won", v=v)
    for v in (del2, PLAIN, PLAIN):
        member("del_lost", v=v)
    # the deletion's vote hangs on the base after it: contig index 34 follows the 30 M bases from index 4
    member("del_at_limit", v=del2, limit=34, group=-1)
    member("del_below_limit", v=del2, limit=35, group=-2)
    # inserted bases: no column, counted below the limit (indices 35, 36)
    ins2 = H(V0, 5, 1, [("M", 31), ("I", 2), ("M", 40)])
    member("ins", v=ins2, group=-1)
    member("ins_cut", v=ins2, limit=36, group=-1)
    # a voter wholly above its limit, alone and beside a sister
    member("above_alone", limit=4, group=-1)
    member("above_sister", limit=0)
    member("above_sister")
    # the record: 2 to 1, and 1 to 1 with the higher index first
    other = H(V5, 20, 1, [("M", 50)])
    for v in (PLAIN, other, PLAIN):
        member("record_2to1", v=v)
    for v in (other, PLAIN):
        member("record_tie", v=v)
    # a consensus of 127 runs from two voters of 64 runs each
    comb = [("M", 1), ("D", 1)] * 32
    member("runs127", v=H(V0, 5, 1, comb))
    member("runs127", v=H(V0, 5, 65, comb))
    # gap columns at either end of the row; a row of gap columns only; a hit of 65 runs (absent) beside a sister
    member("end_gaps", v=H(V0, 5, 11, [("D", 2), ("M", 30), ("D", 3)]), group=-1)
    member("no_base", v=H(V0, 5, 11, [("D", 3)]), group=-1)
    member("truncated", v=H(V0, 5, 1, comb + [("M", 1)]))
    member("truncated")
    return out


def edge(what):
    """the contigs of one edge -> (cases, model at 0.6, model at mostCommon)"""
    cs = [c for c in edge_cases() if c["what"] == what]
    assert cs, what
    ct, v, lim, grp = inputs(cs)
    return cs, CM.consensus(ct, v, TM.germs(), lim, grp, CM.DEFAULT), CM.consensus(ct, v, TM.germs(), lim, grp, MOST_COMMON)


@functools.lru_cache(maxsize=None)
def edge_model(freq=CM.DEFAULT, cells=1 << 24):
    ct, v, lim, grp = inputs(edge_cases())
    return CM.consensus(ct, v, TM.germs(), lim, grp, freq, cells)


@functools.lru_cache(maxsize=None)
def permutation():
    return np.random.default_rng(77).permutation(len(edge_cases()))


# ---- 300 lone contigs (and targeting's groups) -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lone_model(cells=1 << 24):
    ct, v, lim, grp = TC.group_inputs(TC.batch_cases())
    return CM.consensus(ct, v, TM.germs(), lim, grp, CM.DEFAULT, cells)


# ---- one unit of 300 voters over the 2,047-base record -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_cases():
    """BIG_VOTERS contigs of one group over V3, 300 bases each from a seeded start (the first and the last at the record's ends): some
    changes shared by every voter that covers them, some private, a few N and deletions"""
    rng = np.random.default_rng(4242)
    rec = TM.germs()[V3]
    shared = {int(p): alt(rec[int(p)], 1 + int(rng.integers(0, 3))) for p in rng.choice(TC.HOT_LEN, 60, replace=False)}
    out = []
    for k in range(BIG_VOTERS):
        span = 260
        g0 = 0 if k == 0 else TC.HOT_LEN - span if k == 1 else int(rng.integers(0, TC.HOT_LEN - span + 1))
        cut = 20 + int(rng.integers(0, 200))
        ops = [("M", span)] if k % 5 else [("M", cut), ("D", 2), ("M", span - cut - 2)]
        v = H(V3, 1 + int(rng.integers(0, 30)), g0 + 1, ops)
        ct = list(TM._rand(rng, LEN))
        TM._lay(ct, v, rec)
        q, p = v["seq_start"] - 1, g0
        for o, l in ops:
            for t in range(l if o == "M" else 0):
                if p + t in shared:
                    ct[q + t] = shared[p + t]
                elif rng.random() < 0.03:
                    ct[q + t] = "ACGTN"[int(rng.integers(0, 5))]
            q += l * (o != "D")
            p += l
        out.append(dict(name=f"big{k}", what="big", contig="".join(ct), v=v, limit=LEN if k % 7 else 150, group=5))
    return out


@functools.lru_cache(maxsize=None)
def big_model():
    ct, v, lim, grp = inputs(big_cases())
    return CM.consensus(ct, v, TM.germs(), lim, grp, CM.DEFAULT)
