"""The selection model of include/vdjx.h (vdjx_selection, `vdjer --selection`) restated in numpy: the observed and expected counts are
integer and come from the columns of tests/mutation_model.py (the device is tested against them bit for bit); the posterior is computed in
np.longdouble with the members in contig order (the device's float64 is tested against it within a derived bound).  Nothing here reads the
product."""
from __future__ import annotations

import numpy as np

from tests import annot_model as A
from tests import mutation_model as M

T = 4001
F_V, F_TRUNC, F_NOREG = 1, 16, 32
COLUMNS = ["level", "id", "region", "sequences", "obs_r", "obs_s", "exp_r", "exp_s", "sigma", "sigma_lower", "sigma_upper", "p_positive"]
LD = np.longdouble


def grid(dtype=np.float64):
    return (np.arange(T, dtype=dtype) - dtype(2000)) / dtype(100)


def region_of(p1, iv):
    """the region of the 1-based record position p1 under the record's four entries (None: no map)"""
    if iv is None:
        return 0
    return int((iv[0] <= p1 <= iv[1]) or (iv[2] <= p1 <= iv[3]))


def counts(contigs, v, limit, germs, cdr=None, weight=None):
    """the model of vdjx_selection's out_counts -> {field: int array [n] or [n, 2] (python ints for the uint64 sums)}"""
    n = len(contigs)
    out = dict(obs_r=np.zeros((n, 2), np.int64), obs_s=np.zeros((n, 2), np.int64), codons=np.zeros((n, 2), np.int64), flags=np.zeros(n, np.int64),
               exp_r=np.zeros((n, 2), object), exp_s=np.zeros((n, 2), object))
    out["exp_r"][:] = 0
    out["exp_s"][:] = 0
    for c in range(n):
        s = contigs[c]
        lim = len(s) if limit is None else int(limit[c])
        cols, flags, _ = M.columns(c, v, None, None)
        if not flags & M.F_V:
            out["flags"][c] = F_TRUNC if flags & M.F_TRUNC else 0
            continue
        gene = int(v["gene"][c])
        iv = None if cdr is None else [int(x) for x in cdr[gene]]
        if iv is not None and iv[0] == -1:
            out["flags"][c] = F_NOREG
            continue
        out["flags"][c] = F_V
        rec = germs[gene]
        where = {g: k for k, (reg, op, p, g) in enumerate(cols) if op == "M"}
        gs, ge = int(v["germ_start"][c]), int(v["germ_end"][c])
        for cod in range(len(rec) // 3):
            gp = [3 * cod + 1, 3 * cod + 2, 3 * cod + 3]
            if gp[0] < gs or gp[2] > ge or any(g not in where for g in gp):
                continue
            ks = [where[g] for g in gp]
            if ks[1] != ks[0] + 1 or ks[2] != ks[1] + 1 or any(cols[k][2] - 1 >= lim for k in ks):
                continue
            gc, cc = "".join(rec[g - 1] for g in gp), "".join(s[cols[k][2] - 1] for k in ks)
            if any(ch not in "ACGT" for ch in gc + cc):
                continue
            out["codons"][c, region_of(gp[0], iv)] += 1
            aa = A.translate(gc)
            for b in range(3):
                reg = region_of(gp[b], iv)
                if cc[b] != gc[b]:
                    ma = A.translate(gc[:b] + cc[b] + gc[b + 1:])
                    if aa != "*" and ma != "*":
                        out["obs_s" if ma == aa else "obs_r"][c, reg] += 1
                if aa == "*":
                    continue
                p = gp[b] - 1
                if weight is not None:
                    five = rec[p - 2:p + 3] if p >= 2 else ""
                    if len(five) != 5 or any(ch not in "ACGT" for ch in five):
                        continue
                    idx = 0
                    for ch in five:
                        idx = 4 * idx + "ACGT".index(ch)
                for alt in "ACGT":
                    if alt == gc[b]:
                        continue
                    ma = A.translate(gc[:b] + alt + gc[b + 1:])
                    if ma == "*":
                        continue
                    w = 1 if weight is None else int(weight[idx][("ACGT").index(alt)])
                    out["exp_s" if ma == aa else "exp_r"][c, reg] += w
    return out


def members(cnt, K):
    """per region k the (x, n, exp_r, exp_s) of every contig, or None where it adds nothing -> [K][n]"""
    n = len(cnt["flags"])
    out = []
    for k in range(K):
        row = []
        for i in range(n):
            ss = sum(int(cnt["obs_s"][i, j]) for j in range(K))
            es = sum(int(cnt["exp_s"][i, j]) for j in range(K))
            x, er = int(cnt["obs_r"][i, k]), int(cnt["exp_r"][i, k])
            row.append((x, x + ss, er, es) if x + ss > 0 and er > 0 and es > 0 else None)
        out.append(row)
    return out


def softplus(z):
    return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))


def posterior(ms, dtype=LD):
    """the posterior of a row in a region from its contributing members [(x, n, exp_r, exp_s)], in order -> dict(sequences, x, n, exp_r, exp_s,
    sigma, lower, upper, p_positive, pdf, cdf, A); A: the size of the row's terms for the tolerance"""
    sg = grid(dtype)
    ell = sg - 2 * softplus(sg)
    acc = np.zeros(T, dtype)
    a_size = 40.0
    for x, n, er, es in ms:
        lo = np.log(dtype(er)) - np.log(dtype(es))
        z = sg + lo
        acc = acc + (dtype(x) * z - dtype(n) * softplus(z))
        a_size += n * (20.0 + abs(float(lo)))
    ell = ell + acc
    f = np.exp(ell - ell.max())
    S = f.sum()
    cdf = np.cumsum(f) / S
    lower, upper = int(np.argmax(cdf >= dtype(0.025))), int(np.argmax(cdf >= dtype(0.975)))
    return dict(sequences=len(ms), x=sum(m[0] for m in ms), n=sum(m[1] for m in ms), exp_r=sum(m[2] for m in ms), exp_s=sum(m[3] for m in ms),
                sigma=(sg * f).sum() / S, lower=(lower - 2000) / 100.0, upper=(upper - 2000) / 100.0, lower_t=lower, upper_t=upper,
                p_positive=(f[2001:].sum() + f[2000] / 2) / S, pdf=f / (dtype(0.01) * S), cdf=cdf, A=a_size)


def rows(cnt, K, group, G, dtype=LD):
    """every row of vdjx_selection's out_stat -> [n + G + 1][K] of posterior()'s dicts: the contigs, the groups, all contigs"""
    n = len(cnt["flags"])
    mem = members(cnt, K)
    sets = [[i] for i in range(n)] + [[i for i in range(n) if group is not None and int(group[i]) == g] for g in range(G)] + [list(range(n))]
    return [[posterior([mem[k][i] for i in st if mem[k][i] is not None], dtype) for k in range(K)] for st in sets]


def tolerance(A_size):
    """|pdf_device - pdf_model| <= 8 * 2^-52 * A * peak: a float64 sum of the row's terms carries about 2^-52 * A per rounding"""
    return 8.0 * 2.0 ** -52 * A_size


def quantile_margin(post):
    """the smallest distance of the model's CDF at the deciding index and the one before it from 0.025 / 0.975"""
    d = []
    for t, q in ((post["lower_t"], 0.025), (post["upper_t"], 0.975)):
        d.append(abs(float(post["cdf"][t]) - q))
        if t > 0:
            d.append(abs(float(post["cdf"][t - 1]) - q))
    return min(d)


def info(cnt, G, K):
    f = np.asarray(cnt["flags"])
    return dict(contigs=len(f), used=int((f & F_V > 0).sum()), no_regions=int((f & F_NOREG > 0).sum()), truncated=int((f & F_TRUNC > 0).sum()),
                groups=G, regions=K)


def table_rows(ids, cnt, K, clone, G, sample):
    """the rows of `vdjer --selection` (lists of strings, COLUMNS): the contigs in order, lin_1 .. lin_G, the sample"""
    st = rows(cnt, K, clone, G)
    names = ["v"] if K == 1 else ["fwr", "cdr"]
    n = len(ids)
    out = []
    labels = [("sequence", cid) for cid in ids] + [("lineage", f"lin_{g + 1}") for g in range(G)] + [("sample", sample)]
    for r, (level, rid) in enumerate(labels):
        if r < n and not int(cnt["flags"][r]) & F_V:
            out.append([level, rid] + [""] * 10)
            continue
        for k in range(K):
            p = st[r][k]
            out.append([level, rid, names[k], str(p["sequences"]), str(p["x"]), str(p["n"] - p["x"]), str(p["exp_r"]), str(p["exp_s"]),
                        "%.4f" % float(p["sigma"]), "%.2f" % p["lower"], "%.2f" % p["upper"], "%.4f" % float(p["p_positive"])])
    return out, st


def summary_line(inf, st, targeting, chunks):
    sample = st[-1]
    return ("selection: %d contigs, %d used, %d without regions, %d lineages, %d regions, targeting %s, sample sigma %s, %d chunks"
            % (inf["contigs"], inf["used"], inf["no_regions"], inf["groups"], inf["regions"], targeting,
               " ".join("%.4f" % float(p["sigma"]) for p in sample), chunks))
