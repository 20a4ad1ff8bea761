"""The cases of vdjx_lineage_model, for tests/test_lineage_dist_cpu.py (which proves that each reaches what it is for) and
tests/test_gpu_lineage_dist.py (which runs them): name -> (junctions, group, (num, den), table name).  Every case runs under both
symmetries.  The tables: uniform (all 1,000), realistic (the model's table of annot.targeting_model's weights over seeded counts) and
extreme (cells of 1 and of 65,535 among seeded ones).  Everything is seeded; every model result is computed once."""
import functools

import numpy as np

from tests import lineage_dist_model as LM
from tests import lineage_model as M
from tests import targeting_cases as TC

SIZES = [1, 2, 63, 64, 65, 129]                                          # row-block and column-tile edges
LENGTHS = [1, 3, 4, 5, 6, 31, 32, 33, 34, 35, 64, 65, 96, 255]           # no 5-mer, the first with one, word edges, the longest
PLACED = [0, 1, 2, -3, -2, -1] + list(range(29, 35)) + list(range(61, 67))   # where the placed substitutions sit (negative: from the end)
PLACED_LENGTHS = [70, 67]                                                 # L - 3 .. L - 1 = 67 .. 69, and 64 .. 66: the end rule inside the third word's first bases
BIG = "bucket_4097"
A, C_ = "A" * 255, "C" * 255                                              # the largest D: every position differs, every 5-mer is AAAAA or CCCCC


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(list(alpha), int(n)))


def _subst(rng, s, positions):
    s = list(s)
    for q in positions:
        s[q] = rng.choice([ch for ch in "ACGT" if ch != s[q]])
    return "".join(s)


def _family(rng, founder, m, frac=0.12):
    L, out = len(founder), [founder]
    while len(out) < m:
        k = int(rng.integers(0, max(1, int(frac * L)) + 1))
        pos = set(rng.choice(L, size=min(k, L), replace=False).tolist())
        if rng.integers(0, 3) == 0:
            pos.add(L - 1)
        out.append(_subst(rng, founder, sorted(pos)))
    return out


def placed_at(L):
    """the placed positions in a junction of L bases, each once"""
    return list(dict.fromkeys(q % L for q in PLACED))


def _index5(s):
    idx = 0
    for ch in s:
        idx = 4 * idx + "ACGT".index(ch)
    return idx


# ---- the tables -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights():
    """{name: uint32[1024, 4]} targeting weights: what the table builder is tested on, the first two also the GPU cases' tables"""
    from vdjer_amd import annot
    rng = np.random.default_rng(8642)
    out = {"uniform": np.ones((1024, 4), np.uint32), "all_equal": np.full((1024, 4), 123456, np.uint32)}
    out["realistic"] = annot.targeting_model(TC.finish_counts()["rs"], "rs", 1, 1)[0]      # every 5-mer on its own level: costs 716 .. 2068
    out["realistic_levels"] = annot.targeting_model(TC.finish_counts()["levels"], "s", 50, 500)[0]
    out["zeros"] = np.zeros((1024, 4), np.uint32)
    one_big = np.ones((1024, 4), np.uint32)
    one_big[_index5("AAGCA"), 3] = 0xFFFFFFFF                             # one cell of 2^32 - 1 among ones: its cost clamps to 1
    out["one_big"] = one_big
    out["seeded"] = rng.integers(0, 1 << 32, (1024, 4), dtype=np.uint64).astype(np.uint32)
    out["seeded_small"] = rng.integers(0, 50, (1024, 4), dtype=np.uint64).astype(np.uint32)
    return out


@functools.lru_cache(maxsize=None)
def tables():
    """{name: uint16[1024, 4]} distance tables of the cases"""
    rng = np.random.default_rng(8643)
    out = {"uniform": LM.distance_table(weights()["uniform"])[0], "realistic": LM.distance_table(weights()["realistic"])[0]}
    ext = rng.integers(1, 65536, (1024, 4)).astype(np.uint16)
    pick = rng.integers(0, 4, (1024, 4))
    ext[pick == 0] = 1
    ext[pick == 1] = 65535
    ext[_index5("AAAAA"), 1] = 65535                                      # A -> C inside AAAAA and C -> A inside CCCCC: the largest D
    ext[_index5("CCCCC"), 0] = 65535
    for m in range(1024):
        ext[m, m >> 4 & 3] = 0
    out["extreme"] = ext
    return out


def _find_pair(rng, table, L, k, want, symmetry="avg", tries=20000):
    """a founder of L bases and a copy with k substitutions whose D satisfies `want`"""
    for _ in range(tries):
        a = _rand(rng, L)
        b = _subst(rng, a, rng.choice(L, size=k, replace=False).tolist())
        if want(LM.distance(a, b, table, symmetry), LM.distance(a, b, table, "min" if symmetry == "avg" else "avg")):
            return a, b
    raise AssertionError("no such pair")


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(30303)
    T = tables()
    out = {}
    for m in SIZES:                                                      # one bucket of m items: two families and a few strangers
        js = (_family(rng, _rand(rng, 45), (m + 1) // 2) + _family(rng, _rand(rng, 45), m // 2))[:m]
        for k in range(0, m, 17):
            js[k] = _rand(rng, 45)
        out[f"size_{m}"] = (js, [3] * m, M.DEFAULT, "realistic")
    for L in LENGTHS:                                                    # 21 items of L bases; some pairs differ in the last base only
        f = _rand(rng, L)
        js = _family(rng, f, 12, 0.2) + _family(rng, _rand(rng, L), 7, 0.2) + [_subst(rng, f, [L - 1]), f]
        out[f"len_{L}"] = (js, [0] * len(js), (2000, 10000), "realistic")
        out[f"len_{L}_extreme"] = (js, [0] * len(js), M.DEFAULT, "extreme")
        out[f"len_{L}_uniform"] = (js, [0] * len(js), (2000, 10000), "uniform")
    for L in PLACED_LENGTHS:                                             # the founder and one copy per placed position, one substitution each
        f = _rand(rng, L)
        js = [f] + [_subst(rng, f, [q]) for q in placed_at(L)]
        for tab in ("realistic", "extreme"):                              # linked when the one mismatch is cheaper than the mean one
            out[f"placed_{L}_{tab}"] = (js, [1] * len(js), (1, L), tab)
    # characters that are not ACGT: g is f with a substitution at 20, h with one at 32 (the first base of the second word); an N or a lower-case
    # letter at the mismatch and one and two bases to either side of it, in the founder's copy and in the variant's
    f = _rand(rng, 40)
    g, h = _subst(rng, f, [20]), _subst(rng, f, [32])
    js = [f, g, h]
    for var, at in ((g, 20), (h, 32)):
        for q in range(at - 2, at + 3):
            for s in (var, f):
                js.append(s[:q] + "N" + s[q + 1:])
                js.append(s[:q] + s[q].lower() + s[q + 1:])
    for tab in ("realistic", "extreme"):
        out[f"not_acgt_{tab}"] = (js, [0] * len(js), (300, 10000), tab)       # D <= 2400: one mean mismatch and a little
    # against Hamming at the default 0.15: at L = 20 Hamming links d <= 3 and the model D <= 6000, at L = 60 d <= 9 and D <= 18000
    a, b = _find_pair(rng, T["realistic"], 20, 3, lambda d, _: d > 6000)
    out["heavier_than_hamming"] = ([a, b], [0, 0], M.DEFAULT, "realistic")
    a, b = _find_pair(rng, T["realistic"], 60, 10, lambda d, _: d <= 18000)
    out["lighter_than_hamming"] = ([a, b], [0, 0], M.DEFAULT, "realistic")
    # avg and min disagree: two pairs and a stranger; avg leaves the first pair apart, min links it
    a, b = _find_pair(rng, T["extreme"], 30, 2, lambda d, other: d > 9000 >= other)
    c, d = _find_pair(rng, T["extreme"], 30, 1, lambda x, other: x <= 9000 and other <= 9000)
    out["symmetry_matters"] = ([a, c, b, _rand(rng, 30), d], [2] * 5, M.DEFAULT, "extreme")
    out["largest_d"] = ([A, C_], [0, 0], (1, 1), "extreme")
    # one bucket of 4,097 random junctions of 45 bases: a chain of 131, each one substitution from the previous, at random rows; exact
    # duplicates in row 0 and the last row (the only column of the last slice of 128) and three more pairs
    m = 4097
    a4 = rng.integers(0, 4, (m, 45))
    js = ["".join("ACGT"[x] for x in row) for row in a4.tolist()]
    at = (1 + rng.choice(m - 2, size=131 + 6, replace=False)).tolist()
    for k in range(1, 131):
        q = k % 45
        s = js[at[k - 1]]
        js[at[k]] = s[:q] + "ACGT"[("ACGT".index(s[q]) + 1) % 4] + s[q + 1:]
    js[m - 1] = js[0]
    for k in range(3):
        js[at[131 + 2 * k]] = js[at[132 + 2 * k]]
    out[BIG] = (js, [11] * m, M.DEFAULT, "realistic")
    # five buckets shuffled together
    js, grp = [], []
    for g_, L, n_ in ((0, 45, 70), (0, 48, 30), (9, 45, 90), (4000000000, 33, 20), (2, 96, 66)):
        fam = _family(rng, _rand(rng, L), n_)
        js += fam
        grp += [g_] * n_
    order = rng.permutation(len(js))
    out["interleaved"] = ([js[i] for i in order], [grp[i] for i in order], M.DEFAULT, "realistic")
    out["interleaved_extreme"] = ([js[i] for i in order], [grp[i] for i in order], M.DEFAULT, "extreme")
    return out


PERMUTED = "interleaved"


@functools.lru_cache(maxsize=None)
def permutation():
    return np.random.default_rng(7).permutation(len(cases()[PERMUTED][0])).tolist()


@functools.lru_cache(maxsize=None)
def model(name, sym):
    js, grp, md, tab = cases()[name]
    return LM.lineage(js, grp, tables()[tab], md, sym)


class _Models:
    """models()[name, symmetry] -> (clone, nearest, info, walked), each computed when first asked for"""

    def __getitem__(self, key):
        return model(*key)


def models():
    return _Models()
