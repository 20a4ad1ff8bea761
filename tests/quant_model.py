"""vdjx_quant's model (include/vdjx.h) restated in float64 numpy: RSEM's core paired-end EM over (pair, contig, insert) triples, one
triple per placement; quant_trace keeps every iteration, quant_one_exact is its first iteration in exact rationals.  Also the readers the quant tests share: SAM placements and the isoforms.results table of `vdjer --quant`."""
import numpy as np

MIN_INSERT, MAX_INSERT = 50, 400             # quick_map3.c:23-24
HEADER = ["transcript_id", "gene_id", "length", "effective_length", "expected_count", "TPM", "FPKM", "IsoPct"]


def frag_weights(pair, insert, L):
    """(g per placement, eff_len, pairs placed once): P(f) from the inserts of the pairs placed exactly once, add-one smoothed over
    [50, 400]; g(f) = P(f) / (L - f + 1)"""
    pair = np.asarray(pair, np.int64)
    insert = np.asarray(insert, np.int64)
    f = np.arange(MIN_INSERT, MAX_INSERT + 1)
    if pair.size:
        _, inv, deg = np.unique(pair, return_inverse=True, return_counts=True)
        once = (deg[inv] == 1) & (insert >= MIN_INSERT) & (insert <= MAX_INSERT)
        h = np.bincount(insert[once] - MIN_INSERT, minlength=f.size)
    else:
        h = np.zeros(f.size, np.int64)
    P = (h + 1) / float((h + 1).sum())
    span = L - f + 1
    ok = f <= L
    gtab = np.where(ok, P / np.where(ok, span, 1), 0.0)
    eff_len = float((P * span)[ok].sum())
    inwin = (insert >= MIN_INSERT) & (insert <= MAX_INSERT)
    g = np.where(inwin, gtab[np.clip(insert - MIN_INSERT, 0, f.size - 1)], 0.0)
    return g, eff_len, int(h.sum())


def _iterate(pair, contig, insert, n_contigs, L):
    """the model's state before the first iteration (g, eff_len, pairs placed once, placed pairs, N), then (N, delta) after every
    iteration, for as long as the caller goes on asking"""
    pair = np.asarray(pair, np.int64)
    contig = np.asarray(contig, np.int64)
    insert = np.asarray(insert, np.int64)
    g, eff_len, unique = frag_weights(pair, insert, L)
    N = np.zeros(n_contigs)
    if pair.size == 0:
        yield eff_len, unique, 0, N
        return
    upair, inv = np.unique(pair, return_inverse=True)
    placed = np.bincount(contig, minlength=n_contigs) > 0
    N[placed] = upair.size / float(placed.sum())
    yield eff_len, unique, int(upair.size), N
    while True:
        w = N[contig] * g
        s = np.bincount(inv, weights=w, minlength=upair.size)[inv]
        r = np.where(s > 0, w / np.where(s > 0, s, 1.0), 0.0)
        Nn = np.bincount(contig, weights=r, minlength=n_contigs)
        delta = float(np.max(np.abs(Nn - N) / np.maximum(Nn, 1.0)))
        N = Nn
        yield N, delta


def quant(pair, contig, insert, n_contigs, L, max_iter=10000, tol=1e-5):
    """-> (N float64[n_contigs], info) with info as vdjx_quant fills it"""
    steps = _iterate(pair, contig, insert, n_contigs, L)
    eff_len, unique, pairs, N = next(steps)
    info = dict(pairs=pairs, alignments=int(np.asarray(pair).size), unique_pairs=unique, iterations=0, converged=True, eff_len=eff_len)
    if pairs == 0:
        return N, info
    for t in range(1, max_iter + 1):
        N, delta = next(steps)
        info["iterations"] = t
        if delta < tol:
            info["converged"] = True
            return N, info
    info["converged"] = False
    return N, info


def quant_trace(pair, contig, insert, n_contigs, L, iters):
    """-> (N float64[iters, n_contigs], delta float64[iters]): row t - 1 is quant's N after iteration t, delta[t - 1] what its stop rule
    compares with tol then (no stop: all `iters` iterations run)"""
    steps = _iterate(pair, contig, insert, n_contigs, L)
    next(steps)
    out = [next(steps) for _ in range(iters)] if np.asarray(pair).size else []
    return np.array([x[0] for x in out]).reshape(len(out), n_contigs), np.array([x[1] for x in out])


def quant_one_exact(pair, contig, insert, n_contigs, L):
    """iteration 1 of the model in exact rational arithmetic (fractions.Fraction): the histogram of the pairs placed once, P, g, the
    start value, the E and the M step.  -> (N: list of n_contigs Fractions, degree: dict pair id -> its number of placements)"""
    from fractions import Fraction
    pair = [int(x) for x in pair]
    contig = [int(x) for x in contig]
    insert = [int(x) for x in insert]
    degree = {}
    for p in pair:
        degree[p] = degree.get(p, 0) + 1
    h = [0] * (MAX_INSERT - MIN_INSERT + 1)
    for p, f in zip(pair, insert):
        if degree[p] == 1 and MIN_INSERT <= f <= MAX_INSERT:
            h[f - MIN_INSERT] += 1
    tot = sum(x + 1 for x in h)

    def g(f):
        if not (MIN_INSERT <= f <= MAX_INSERT and f <= L):
            return Fraction(0)
        return Fraction(h[f - MIN_INSERT] + 1, tot) / (L - f + 1)

    N = [Fraction(0)] * n_contigs
    if not pair:
        return N, degree
    placed = set(contig)
    start = Fraction(len(degree), len(placed))
    w = [start * g(f) for f in insert]                                   # (every placed contig starts at `start`)
    total = {}
    for p, x in zip(pair, w):
        total[p] = total.get(p, Fraction(0)) + x
    for p, c, x in zip(pair, contig, w):
        if total[p] > 0:
            N[c] += x / total[p]
    return N, degree


def sam_placements(text):
    """(contig ids in @SQ order, contig length, pair names, triples) of SAM text as vdjer writes it: one placement per read-1 line
    (flag 0x40), its contig, TLEN as the insert"""
    ids, L, names = [], None, {}
    trip = []
    index = {}
    for line in text.splitlines():
        if line.startswith("@"):
            if line.startswith("@SQ"):
                f = dict(x.split(":", 1) for x in line.split("\t")[1:])
                index[f["SN"]] = len(ids)
                ids.append(f["SN"])
                L = int(f["LN"])
            continue
        f = line.split("\t", 9)
        if not int(f[1]) & 0x40:
            continue
        p = names.setdefault(f[0], len(names))
        trip.append((p, index[f[2]], abs(int(f[8]))))
    a = np.array(trip, np.int64).reshape(-1, 3)
    return ids, L, list(names), a


def read_table(path):
    rows = [l.rstrip("\n").split("\t") for l in open(path)]
    return rows[0], rows[1:]
