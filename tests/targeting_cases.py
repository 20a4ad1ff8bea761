"""The inputs of tests/test_gpu_targeting.py and their model results, shared with tests/test_targeting_cpu.py (which proves without a GPU
that every case reaches what it is for).  Everything is seeded and computed once per process."""
from __future__ import annotations

import functools

import numpy as np

from tests import annot_model as A
from tests import selection_cases as SC
from tests import targeting_model as T
from tests import test_gpu_mutation as TM
from tests.test_gpu_mutation import H, NONE, V0, V5

LEN = TM.LEN
HOT_LEN = 2047
SINGLES = 300                                                         # single-contig units of the batch case: ten workgroups of k_tgt_count


def hits(cs):
    return TM._hits(cs, "v")


# ---- selection's count cases, every contig a unit of its own ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def count_inputs():
    cs = SC.count_cases()
    return [c["contig"] for c in cs], hits(cs), np.array([c["limit"] for c in cs], np.int32)


@functools.lru_cache(maxsize=None)
def count_model():
    ct, v, lim = count_inputs()
    return T.counts(ct, v, lim, TM.germs())


# ---- groups ------------------------------------------------------------------------------------------------------------------------------------
def _index(v, p):
    """the contig index that carries the 0-based record position p of hit v (inside an M run)"""
    q, g = v["seq_start"] - 1, v["germ_start"] - 1
    for o, l in v["ops"]:
        if o == "M" and g <= p < g + l:
            return q + p - g
        q += l * (o != "D")
        g += l * (o != "I")
    raise AssertionError(p)


def changes(rec, p):
    """the bases that may replace record position p without a stop, the germline codon being none -> [alt]"""
    cod, b = divmod(p, 3)
    gc = rec[3 * cod:3 * cod + 3]
    if len(gc) < 3 or any(ch not in "ACGT" for ch in gc) or A.translate(gc) == "*" or not T.has_5mer(rec, p):
        return []
    return [x for x in "ACGT" if x != gc[b] and A.translate(gc[:b] + x + gc[b + 1:]) != "*"]


def _site(rec, lo, hi, need=1):
    """the first position in lo .. hi - 1 with at least `need` stop-free changes -> (p, [alt])"""
    for p in range(lo, hi):
        if len(changes(rec, p)) >= need:
            return p, changes(rec, p)
    raise AssertionError("no such site: move the window")


GROUP_NAMES = ("shared", "two_records", "indel_sister", "two_alts", "negative")


@functools.lru_cache(maxsize=None)
def group_cases():
    """[dict(name, contig, v, limit, group, what)] of LEN bases; the contigs are their germline except for the named changes.  Group ids are
    neither dense nor ordered"""
    rng = np.random.default_rng(5151)
    g = TM.germs()
    out = []

    def member(what, group, v, edits):
        ct = list(TM._rand(rng, LEN))
        TM._lay(ct, v, g[v["gene"]])
        for p, alt in edits:
            ct[_index(v, p)] = alt
        out.append(dict(name=f"{what}{len(out)}", what=what, contig="".join(ct), v=v, limit=LEN, group=group))

    plain = H(V0, 5, 1, [("M", 90)])
    p1, a1 = _site(g[V0], 12, 80)
    # two members over one record with the same change: once
    member("shared", 40, plain, [(p1, a1[0])])
    member("shared", 40, H(V0, 9, 1, [("M", 90)]), [(p1, a1[0])])
    # the same group over two records, a change in each: twice
    p5, a5 = _site(g[V5], 6, 50)
    member("two_records", 7, plain, [(p1, a1[0])])
    member("two_records", 7, H(V5, 20, 1, [("M", 60)]), [(p5, a5[0])])
    # an insertion after record base 31 splits the codon of positions 30 .. 32: the member's change there is not classifiable, its sister's is
    pi, ai = _site(g[V0], 30, 33)
    member("indel_sister", 2, H(V0, 5, 1, [("M", 31), ("I", 2), ("M", 40)]), [(pi, ai[0])])
    member("indel_sister", 2, plain, [(pi, ai[0])])
    # two members with different new bases at one position: two events over one set of opportunities
    p2, a2 = _site(g[V0], 40, 80, need=2)
    member("two_alts", 3, plain, [(p2, a2[0])])
    member("two_alts", 3, plain, [(p2, a2[1])])
    # negative group ids: units of their own, whatever the id
    member("negative", -1, plain, [(p1, a1[0])])
    member("negative", -1, plain, [(p1, a1[0])])
    member("negative", -5, plain, [(p1, a1[0])])
    return out


def group_inputs(cs=None):
    cs = group_cases() if cs is None else cs
    return [c["contig"] for c in cs], hits(cs), np.array([c["limit"] for c in cs], np.int32), np.array([c["group"] for c in cs], np.int32)


def group_model(what=None, grouped=True):
    """the model over the group cases (what: one kind of them only)"""
    cs = [c for c in group_cases() if what is None or c["what"] == what]
    ct, v, lim, grp = group_inputs(cs)
    return T.counts(ct, v, lim, TM.germs(), grp if grouped else None)


@functools.lru_cache(maxsize=None)
def permutation():
    return np.random.default_rng(99).permutation(len(group_cases()))


# ---- one hot bin -----------------------------------------------------------------------------------------------------------------------------
HOT_RECORDS = [("VA", "A" * HOT_LEN)]
HOT_GROUPS = [0, 0, 0, 1, 1, -1, -1, 2]


@functools.lru_cache(maxsize=None)
def hot_cases():
    """8 contigs over a record of 2,047 A: every position with a 5-mer (2 .. 2044) lands in 5-mer 0.  AAA is K; TAA is a stop, AAG is silent"""
    rng = np.random.default_rng(777)
    v = H(0, 1, 1, [("M", HOT_LEN)])
    out = []
    for k, grp in enumerate(HOT_GROUPS):
        ct = ["A"] * HOT_LEN
        for p in rng.choice(HOT_LEN, 120, replace=False):
            ct[int(p)] = "CGTN"[int(rng.integers(0, 4))]
        out.append(dict(name=f"hot{k}", contig="".join(ct), v=v, limit=HOT_LEN, group=grp))
    return out


@functools.lru_cache(maxsize=None)
def hot_model():
    cs = hot_cases()
    ct, v, lim, grp = group_inputs(cs)
    return T.counts(ct, v, lim, [HOT_RECORDS[0][1]], grp)


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_cases():
    """the group cases and SINGLES contigs in no group, each over 90 bases of V0 or 60 of V5 with a few changes"""
    rng = np.random.default_rng(808)
    g = TM.germs()
    out = list(group_cases())
    for k in range(SINGLES):
        v = H(V0, 1 + int(rng.integers(0, 40)), 1 + int(rng.integers(0, 200)), [("M", 90)]) if k % 3 else H(V5, 3, 1, [("M", 60)])
        ct = list(TM._rand(rng, LEN))
        TM._lay(ct, v, g[v["gene"]])
        for q in rng.choice(60, 4, replace=False):
            ct[v["seq_start"] - 1 + int(q)] = TM._other(ct[v["seq_start"] - 1 + int(q)])
        out.append(dict(name=f"single{k}", what="single", contig="".join(ct), v=v, limit=LEN, group=-1))
    return out


@functools.lru_cache(maxsize=None)
def batch_model():
    ct, v, lim, grp = group_inputs(batch_cases())
    return T.counts(ct, v, lim, TM.germs(), grp)


# ---- the model finish ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def finish_counts():
    """{name: uint64[2, 2, 1024, 4]} for vdjx_targeting_model"""
    rng = np.random.default_rng(2468)
    z = np.zeros((2, 2, 1024, 4), np.uint64)

    def fill(obs_s, opp_s, obs_r=None, opp_r=None):
        c = z.copy()
        c[0, 0], c[1, 0] = obs_s, opp_s
        if obs_r is not None:
            c[0, 1], c[1, 1] = obs_r, opp_r
        for m in range(1024):                                         # (the entries of the centre base stay 0)
            c[:, :, m, m >> 4 & 3] = 0
        return c

    # every level in both tables at the defaults 50 / 500: centre A rich per 5-mer (5), centre C rich per inner 3-mer only (3), centre G
    # rich per centre only (1), centre T empty (0)
    obs = np.zeros((1024, 4), np.uint64)
    opp = np.zeros((1024, 4), np.uint64)
    for m in range(1024):
        c = m >> 4 & 3
        if c == 0:
            obs[m], opp[m] = rng.integers(200, 400, 4), rng.integers(5000, 9000, 4)
        elif c == 1:
            obs[m], opp[m] = rng.integers(10, 14, 4), rng.integers(300, 500, 4)          # 16 x 3 x >= 10 = 480 .. 624: level 3 for some, level 1 for others
        elif c == 2:
            obs[m, (c + 1 + int(rng.integers(0, 3))) % 4], opp[m] = 2, rng.integers(50, 90, 4)      # 16 x 2 = 32 per inner 3-mer, 512 per centre
        else:
            opp[m] = rng.integers(50, 90, 4)
    levels = fill(obs, opp)
    rs = fill(obs // 3, opp // 2, obs, opp)
    # a 5-mer with observed changes and no opportunity under class s (its opportunities are all replacement)
    no_opp = levels.copy()
    no_opp[1, 0, 5] = 0
    no_opp[1, 1, 5] = (9, 9, 9, 9)
    no_opp[1, 1, 5, 5 >> 4 & 3] = 0
    # the minima met exactly, and missed by one: 5-mer 0 (AAAAA) holds 50 changes, 5-mer 1 holds 49; mutability 500 and 499
    exact = z.copy()
    exact[0, 0, 0], exact[1, 0, 0] = (0, 20, 20, 10), (0, 100, 100, 100)
    exact[0, 0, 1], exact[1, 0, 1] = (0, 20, 20, 9), (0, 100, 100, 100)
    exact[0, 0, 512], exact[1, 0, 512] = (0, 200, 200, 100), (0, 1000, 1000, 1000)
    exact[0, 0, 513], exact[1, 0, 513] = (0, 200, 200, 99), (0, 1000, 1000, 1000)
    return dict(levels=levels, rs=rs, zeros=z.copy(), no_opp=no_opp, exact=exact)
