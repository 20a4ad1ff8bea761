"""The isotype model of include/vdjx.h (vdjx_constant_load, vdjx_isotype) and the tables of `vdjer --isotypes` / `--clones`, restated in
numpy and plain Python from the reference's post_process/ scripts (call_isotypes.py, collect_vdjer_stats.py, cluster_results.py -- Python 2,
read, not run).  The matrices and the traceback are tests/annot_model.py's: the isotype step is vdjx_annotate's alignment of the contig's
tail.  All integer, so the device is compared bitwise."""
from __future__ import annotations

import numpy as np

from tests import annot_model as A

DEFAULT = dict(match=2, mismatch=3, gap_open=5, gap_extend=2, min_score=48, tail=48)
ISOTYPE_COLUMNS = ["sequence_id", "isotype", "c_call", "c_score", "c_identity", "c_sequence_start", "c_sequence_end", "c_germline_start",
                   "c_germline_end", "c_cigar"]
CLONE_COLUMNS = ["sample", "sequence", "cdr3", "expected_counts", "seq_id", "isotype", "vregion_identity", "aa_cdr3", "vgene", "jgene",
                 "total_count", "cluster"]


# ---- the call ------------------------------------------------------------------------------------------------------------------------
def isotype(contigs, consts, p=DEFAULT):
    """the model of vdjx_isotype: ({field: array} as api.Context.isotype's "c", S int64[n, C])"""
    n, C = len(contigs), len(consts)
    f = {k: np.zeros(n, np.int64) for k in A.FIELDS if k not in ("tied", "runs")}
    f["tied"] = np.full((n, A.TIED), -1, np.int64)
    f["runs"] = np.zeros((n, A.RUNS), np.int64)
    if n == 0:
        return f, np.zeros((0, C), np.int64)
    m = len(contigs[0])
    T = min(p["tail"], m)
    tails = [c[m - T:] for c in contigs]
    uniq = sorted(set(tails))                                              # (equal tails score alike: the matrices are made once)
    at = {t: k for k, t in enumerate(uniq)}
    Su = A.scores(uniq, consts, p) if C else np.zeros((len(uniq), 0), np.int64)
    S = Su[[at[t] for t in tails]]
    done = {}
    for c in range(n):
        best = int(S[c].max()) if C else -1
        f["score"][c] = max(best, 0)
        if best < 0 or best < p["min_score"]:
            f["gene"][c] = -1
            continue
        tied = np.flatnonzero(S[c] == best).tolist()
        f["gene"][c], f["n_tied"][c] = tied[0], len(tied)
        f["tied"][c, :min(A.TIED, len(tied))] = tied[:A.TIED]
        if best > 0:
            key = (tails[c], tied[0])
            if key not in done:
                done[key] = A.traceback(tails[c], consts[tied[0]], p)
            tb = done[key]
            assert tb["score"] == best
            for k in ("germ_start", "germ_end", "matches", "mismatches", "ins", "opens", "n_runs"):
                f[k][c] = tb[k]
            f["seq_start"][c], f["seq_end"][c] = tb["seq_start"] + m - T, tb["seq_end"] + m - T
            f["del"][c] = tb["dele"]
            f["runs"][c] = A.encode_runs(tb["ops"])
    return f, S


# ---- the name rules ------------------------------------------------------------------------------------------------------------------
def gene_of(name):
    return name.split("*")[0]


def _distinct(xs):
    out = []
    for x in xs:
        if x not in out:
            out.append(x)
    return ",".join(out)


def subtypes(names):
    """call_isotypes.py: the first four characters of every gene (IGHG1 -> IGHG), distinct, here in order of first appearance"""
    return _distinct(gene_of(x)[:4] for x in names)


def vq_gene(names):
    """collect_vdjer_stats.py get_vq_gene: the allele and every 'D' dropped, then what lies before a second '-'"""
    out = []
    for x in names:
        g = gene_of(x).replace("D", "")
        parts = g.split("-")
        out.append(parts[0] if len(parts) == 1 else parts[0] + "-" + parts[1])
    return _distinct(out)


def _called(h, c, names):
    if h["gene"][c] < 0:
        return []
    return [names[g] for g in h["tied"][c][:min(A.TIED, h["n_tied"][c])]]


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def isotype_rows(ids, seqs, hit, names):
    """the rows of `vdjer --isotypes` (ISOTYPE_COLUMNS): cells empty where `vdjer --airr` leaves a hit's cells empty"""
    rows = []
    for c, (cid, s) in enumerate(zip(ids, seqs)):
        has = hit["gene"][c] >= 0
        ok = has and hit["score"][c] > 0
        called = _called(hit, c, names)
        ident = ""
        if ok:
            d = hit["matches"][c] + hit["mismatches"][c] + hit["ins"][c] + hit["del"][c]
            ident = "%.4f" % (hit["matches"][c] / d)
        rows.append([cid, subtypes(called), ",".join(called), str(int(hit["score"][c])) if has else "", ident] +
                    [str(int(hit[k][c])) if ok else "" for k in ("seq_start", "seq_end", "germ_start", "germ_end")] + [A.cigar(hit, c, len(s))])
    return rows


def clone_rows(sample, ids, seqs, counts, vj, germ_names, iso=None, const_names=None, total_count=None):
    """the rows of `vdjer --clones` (CLONE_COLUMNS).  vj: annot_model.annotate's hits; iso: isotype()'s hits, or None without --cfa."""
    rows, clusters = [], {}
    hv, hj = vj["v"], vj["j"]
    for c, (cid, s) in enumerate(zip(ids, seqs)):
        cnt = "%.2f" % counts[c]
        junc, p = A.junction_of(cid, s)
        aa = A.translate(junc)
        if not float(cnt) >= 1.0 or hv["gene"][c] < 0 or p < 0 or not aa:
            continue
        d = int(hv["matches"][c] + hv["mismatches"][c] + hv["ins"][c] + hv["del"][c])
        ident = "%.2f" % (100.0 * (int(hv["matches"][c]) / d)) if d else "N/A"
        isot = subtypes(_called(iso, c, const_names)) if iso is not None and iso["gene"][c] >= 0 else "N/A"
        vg = vq_gene(_called(hv, c, germ_names))
        jg = vq_gene(_called(hj, c, germ_names)) if hj["gene"][c] >= 0 else "N/A"
        k = clusters.setdefault((isot, aa, vg, jg), len(clusters) + 1)
        rows.append([sample, s, junc, cnt, cid, isot, ident, aa, vg, jg, str(total_count) if total_count is not None else "N/A", f"cls_{k}"])
    return rows
