"""vdjx_quant_boot's model (include/vdjx.h) in float64 numpy, on top of tests/quant_model.py: the draws through annot.quant_boot_draw, the
EM with a multiplicity per placed pair (every replicate's trace of (N, delta) is kept), and the summary of a B x n matrix of replicate
counts in plain Python."""
import math

import numpy as np

from tests import quant_model as Q
from vdjer_amd import annot


def slots(pair):
    """the placed pair ids in ascending order: slot q is ids[q]"""
    return np.unique(np.asarray(pair, np.int64))


def draws(seed, r, Pp):
    """m_r: uint32[Pp], the number of replicate r's Pp draws on every slot"""
    m = np.zeros(Pp, np.int64)
    for i in range(Pp):
        m[annot.quant_boot_draw(seed, r, i, Pp)] += 1
    return m.astype(np.uint32)


def mult_by_id(m, ids, n_pairs):
    """multiplicities per slot -> per pair id (0 for ids without a placement), as out_mult has them"""
    out = np.zeros(n_pairs, np.uint32)
    out[ids] = m
    return out


def _iterate(pair, contig, insert, n_contigs, L, m, order=None):
    """quant_model._iterate with a multiplicity per slot: the same state before the first iteration, then (N, delta) after every
    iteration.  order: a permutation of the placements in which the sums inside pairs and inside contigs are made (None: as given)"""
    pair, contig, insert = (np.asarray(x, np.int64) for x in (pair, contig, insert))
    g, eff_len, unique = Q.frag_weights(pair, insert, L)
    N = np.zeros(n_contigs)
    if pair.size == 0:
        yield eff_len, unique, 0, N
        return
    upair, inv = np.unique(pair, return_inverse=True)
    mm = np.asarray(m, np.float64)[inv]
    placed = np.bincount(contig, minlength=n_contigs) > 0
    N[placed] = upair.size / float(placed.sum())
    yield eff_len, unique, int(upair.size), N
    o = np.arange(pair.size) if order is None else np.asarray(order)
    while True:
        w = N[contig] * g
        s = np.bincount(inv[o], weights=w[o], minlength=upair.size)[inv]
        r = np.where(s > 0, w / np.where(s > 0, s, 1.0), 0.0)
        Nn = np.bincount(contig[o], weights=(mm * r)[o], minlength=n_contigs)
        delta = float(np.max(np.abs(Nn - N) / np.maximum(Nn, 1.0)))
        N = Nn
        yield N, delta


def trace(pair, contig, insert, n_contigs, L, m, iters, order=None):
    """-> (N float64[iters, n_contigs], delta float64[iters]) of one replicate with the multiplicities m (per slot), no stop"""
    steps = _iterate(pair, contig, insert, n_contigs, L, m, order)
    next(steps)
    out = [next(steps) for _ in range(iters)] if np.asarray(pair).size else []
    return np.array([x[0] for x in out]).reshape(len(out), n_contigs), np.array([x[1] for x in out])


def run(pair, contig, insert, n_contigs, L, m, max_iter=10000, tol=1e-5):
    """one replicate under the stop rule -> (N, iterations, converged)"""
    steps = _iterate(pair, contig, insert, n_contigs, L, m)
    _, _, pairs, N = next(steps)
    if pairs == 0:
        return N, 0, True
    for t in range(1, max_iter + 1):
        N, delta = next(steps)
        if delta < tol:
            return N, t, True
    return N, max_iter, False


def boot(pair, contig, insert, n_contigs, L, replicates, seed, max_iter=10000, tol=1e-5):
    """-> (boot float64[B, n], iterations[B], mult uint32[B, Pp] per slot)"""
    Pp = slots(pair).size
    ms = [draws(seed, r, Pp) for r in range(1, replicates + 1)]
    res = [run(pair, contig, insert, n_contigs, L, m, max_iter, tol) for m in ms]
    return np.array([x[0] for x in res]).reshape(replicates, n_contigs), np.array([x[1] for x in res], np.uint32), np.array(ms, np.uint32).reshape(replicates, Pp)


def summary_indices(B):
    """the two order statistics' indices, in integer arithmetic"""
    return 25 * (B - 1) // 1000, -(-975 * (B - 1) // 1000)


def summary(boot_):
    """the summary of include/vdjx.h in plain Python floats -> dict of lists: mean, sd, lower, upper"""
    rows = [[float(x) for x in row] for row in np.asarray(boot_, np.float64)]
    B, n = len(rows), len(rows[0]) if rows else 0
    lo, hi = summary_indices(B)
    out = dict(mean=[], sd=[], lower=[], upper=[])
    for c in range(n):
        s = 0.0
        for r in range(B):
            s += rows[r][c]
        mean = s / B
        e2 = 0.0
        for r in range(B):
            e2 += (rows[r][c] - mean) ** 2
        v = sorted(rows[r][c] for r in range(B))
        out["mean"].append(mean)
        out["sd"].append(math.sqrt(e2 / (B - 1)) if B > 1 else 0.0)
        out["lower"].append(v[lo])
        out["upper"].append(v[hi])
    return out


def one_exact(pair, contig, insert, n_contigs, L, m):
    """iteration 1 of the weighted model in exact rationals (quant_model.quant_one_exact with m_r[pair(a)] on every r_a; m per slot)
    -> (N: list of n_contigs Fractions, degree: dict pair id -> its number of placements)"""
    from fractions import Fraction
    pair = [int(x) for x in pair]
    contig = [int(x) for x in contig]
    insert = [int(x) for x in insert]
    degree = {}
    for p in pair:
        degree[p] = degree.get(p, 0) + 1
    mult = {p: int(x) for p, x in zip(sorted(degree), m)}
    h = [0] * (Q.MAX_INSERT - Q.MIN_INSERT + 1)
    for p, f in zip(pair, insert):
        if degree[p] == 1 and Q.MIN_INSERT <= f <= Q.MAX_INSERT:
            h[f - Q.MIN_INSERT] += 1
    tot = sum(x + 1 for x in h)

    def g(f):
        if not (Q.MIN_INSERT <= f <= Q.MAX_INSERT and f <= L):
            return Fraction(0)
        return Fraction(h[f - Q.MIN_INSERT] + 1, tot) / (L - f + 1)

    N = [Fraction(0)] * n_contigs
    if not pair:
        return N, degree
    start = Fraction(len(degree), len(set(contig)))
    w = [start * g(f) for f in insert]
    total = {}
    for p, x in zip(pair, w):
        total[p] = total.get(p, Fraction(0)) + x
    for p, c, x in zip(pair, contig, w):
        if total[p] > 0:
            N[c] += mult[p] * x / total[p]
    return N, degree
