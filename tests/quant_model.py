"""vdjx_quant's model (include/vdjx.h) restated in float64 numpy: RSEM's core paired-end EM over (pair, contig, insert) triples, one
triple per placement.  Also the readers the quant tests share: SAM placements and the isoforms.results table of `vdjer --quant`."""
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


def quant(pair, contig, insert, n_contigs, L, max_iter=10000, tol=1e-5):
    """-> (N float64[n_contigs], info) with info as vdjx_quant fills it"""
    pair = np.asarray(pair, np.int64)
    contig = np.asarray(contig, np.int64)
    insert = np.asarray(insert, np.int64)
    g, eff_len, unique = frag_weights(pair, insert, L)
    info = dict(pairs=0, alignments=int(pair.size), unique_pairs=unique, iterations=0, converged=True, eff_len=eff_len)
    N = np.zeros(n_contigs)
    if pair.size == 0:
        return N, info
    upair, inv = np.unique(pair, return_inverse=True)
    placed = np.bincount(contig, minlength=n_contigs) > 0
    N[placed] = upair.size / float(placed.sum())
    info["pairs"] = int(upair.size)
    for t in range(1, max_iter + 1):
        w = N[contig] * g
        s = np.bincount(inv, weights=w, minlength=upair.size)[inv]
        r = np.where(s > 0, w / np.where(s > 0, s, 1.0), 0.0)
        Nn = np.bincount(contig, weights=r, minlength=n_contigs)
        delta = float(np.max(np.abs(Nn - N) / np.maximum(Nn, 1.0)))
        N = Nn
        info["iterations"] = t
        if delta < tol:
            info["converged"] = True
            return N, info
    info["converged"] = False
    return N, info


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
