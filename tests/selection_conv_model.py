"""The model of include/vdjx.h's vdjx_selection_convolve and vdjx_selection_compare (`vdjer --selection-combine mean`, `--selection-test`)
restated in numpy: a row's density is the distribution of the mean of its members' independent sigmas -- the members' own posteriors
(tests/selection_model.py) as mass vectors, combined two at a time along a tree that depends only on their number, each combination put
back on the grid by mass-conserving linear binning.  np.longdouble by default; the device's float64 is tested against it within the bound
E that every function here carries along.  Nothing here reads the product."""
from __future__ import annotations

import numpy as np

from tests.selection_model import members, posterior, quantile_margin, tolerance  # noqa: F401  (quantile_margin: for the tests)

T = 4001
LD = np.longdouble
U = 2.0 ** -53


def leaf(m, dtype=LD):
    """member (x, n, exp_r, exp_s), or None for the prior alone -> (mass[T] summing to 1, E)"""
    p = posterior([] if m is None else [m], dtype)
    f = p["pdf"]
    mass = f / f.sum()
    return mass, tolerance(p["A"]) * float(mass.max())


def combine(A, a, B, b):
    """(A, a) (+) (B, b): the distribution of (a sigma_A + b sigma_B) / (a + b), linearly binned -> C[T]"""
    dtype = A.dtype
    den = a + b
    C = np.zeros(T, dtype)
    if a == b:                                                     # num = u + v: np.convolve's index s = num + 4000
        full = np.convolve(A, B)
        C += full[0::2]
        half = full[1::2] / dtype.type(2)
        C[:-1] += half
        C[1:] += half
        return C
    v = np.arange(-2000, 2001, dtype=np.int64)
    for iu in np.flatnonzero(A):
        num = a * (int(iu) - 2000) + b * v
        q = num // den
        rem = num - q * den
        mass = A[iu] * B
        np.add.at(C, q + 2000, mass * ((den - rem).astype(dtype) / dtype.type(den)))
        up = rem > 0                                               # rem = 0: cell q + 1 gets nothing and is not touched
        np.add.at(C, q[up] + 2001, mass[up] * (rem[up].astype(dtype) / dtype.type(den)))
    return C


def split(m):
    """the leaves of the left side of a row of m > 1 leaves: 2^(ceil(log2 m) - 1)"""
    return 1 << ((m - 1).bit_length() - 1)


def tree(leaves):
    """[(mass, E)] in order -> (C, E, combines, depth)"""
    m = len(leaves)
    if m == 1:
        return leaves[0][0], leaves[0][1], 0, 0
    h = split(m)
    A, ea, ca, da = tree(leaves[:h])
    B, eb, cb, db = tree(leaves[h:])
    den = m
    C = combine(A, h, B, m - h)
    return C, den / h * ea + den / (m - h) * eb + 16008 * U * float(C.max()), ca + cb + 1, max(da, db) + 1


def pairs_tree(leaves):
    """the same tree by rounds of adjacent pairs, an odd last entry passed through -> C (for the CPU test of the tree's two descriptions)"""
    ent = [(c, 1) for c, _ in leaves]
    while len(ent) > 1:
        nx = [(combine(ent[i][0], ent[i][1], ent[i + 1][0], ent[i + 1][1]), ent[i][1] + ent[i + 1][1]) for i in range(0, len(ent) - 1, 2)]
        if len(ent) & 1:
            nx.append(ent[-1])
        ent = nx
    return ent[0][0]


def row(ms, dtype=LD):
    """the contributing members [(x, n, exp_r, exp_s)] of a row in a region, in order -> dict like selection_model.posterior's, with mass
    (C / S'), E (the bound per cell of mass), leaves, combines, depth"""
    lv = [leaf(m, dtype) for m in ms] if ms else [leaf(None, dtype)]
    C, E, combines, depth = tree(lv)
    E += 8004 * U * float(C.max())
    sg = (np.arange(T, dtype=dtype) - dtype(2000)) / dtype(100)
    S = C.sum()
    mass = C / S
    cdf = np.cumsum(C) / S
    lower, upper = int(np.argmax(cdf >= dtype(0.025))), int(np.argmax(cdf >= dtype(0.975)))
    return dict(sequences=len(ms), x=sum(m[0] for m in ms), n=sum(m[1] for m in ms), exp_r=sum(m[2] for m in ms), exp_s=sum(m[3] for m in ms),
                sigma=(sg * C).sum() / S, lower=(lower - 2000) / 100.0, upper=(upper - 2000) / 100.0, lower_t=lower, upper_t=upper,
                p_positive=(C[2001:].sum() + C[2000] / 2) / S, pdf=mass / dtype(0.01), mass=mass, cdf=cdf, E=E, leaves=len(lv), combines=combines,
                depth=depth)


def rows(cnt, K, group, G, dtype=LD):
    """every row of vdjx_selection_convolve's out_stat -> [G + 1][K] of row()'s dicts: the groups, then all contigs"""
    n = len(cnt["obs_r"])
    mem = members(dict(cnt, flags=np.zeros(n)), K)
    sets = [[i for i in range(n) if group is not None and int(group[i]) == g] for g in range(G)] + [list(range(n))]
    return [[row([mem[k][i] for i in st if mem[k][i] is not None], dtype) for k in range(K)] for st in sets]


def info(rws, G, K):
    flat = [p for r in rws for p in r]
    return dict(members=sum(p["sequences"] for p in flat), leaves=sum(p["leaves"] for p in flat), combines=sum(p["combines"] for p in flat),
                groups=G, regions=K, rows=(G + 1) * K, levels=max(p["depth"] for p in flat))


# ---- the comparison ------------------------------------------------------------------------------------------------------------------------
def compare(a, b):
    """two densities (any positive scale) -> (p_greater, pvalue): P(sigma_a > sigma_b) + P(equal) / 2, two-sided"""
    a = np.asarray(a, np.float64) / np.asarray(a, np.float64).sum()
    b = np.asarray(b, np.float64) / np.asarray(b, np.float64).sum()
    below = np.concatenate([[0.0], np.cumsum(b)[:-1]])
    pg = float((a * (below + b / 2)).sum())
    return pg, min(1.0, 2 * min(pg, 1 - pg))


def bh(pvalues, skip=None):
    """Benjamini-Hochberg over the rows that are not skipped: ascending by pvalue, ties in row order -> list (None where skipped)"""
    live = [i for i in range(len(pvalues)) if skip is None or not skip[i]]
    order = sorted(live, key=lambda i: (pvalues[i], i))
    out = [None] * len(pvalues)
    run = 1.0
    for j in range(len(order), 0, -1):
        run = min(run, pvalues[order[j - 1]] * len(order) / j)
        out[order[j - 1]] = min(1.0, run)
    return out


TEST_COLUMNS = ["level", "id", "region_a", "region_b", "sigma_a", "sigma_b", "p_greater", "pvalue", "fdr"]


def test_rows(labels, rws):
    """the rows of `vdjer --selection-test`: labels [(level, id)], rws [[fwr, cdr]] of row()'s or posterior()'s dicts -> lists of strings"""
    skip = [r[0]["sequences"] == 0 or r[1]["sequences"] == 0 for r in rws]
    res = [(None, 0.0) if s else compare(r[1]["pdf"], r[0]["pdf"]) for r, s in zip(rws, skip)]
    fdr = bh([p for _, p in res], skip)
    out = []
    for (level, rid), r, s, (pg, pv), f in zip(labels, rws, skip, res, fdr):
        out.append([level, rid, "cdr", "fwr"] + ([""] * 5 if s else ["%.4f" % float(r[1]["sigma"]), "%.4f" % float(r[0]["sigma"]), "%.4f" % pg, "%.4f" % pv,
                                                                       "%.4f" % f]))
    return out


def summary_line(inf, batches, sample):
    return ("selection combine: mean, %d rows, %d densities, %d combinations, %d levels at most, %d batches, sample sigma %s"
            % (inf["rows"], inf["leaves"], inf["combines"], inf["levels"], batches, " ".join("%.4f" % float(p["sigma"]) for p in sample)))
