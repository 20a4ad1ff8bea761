"""vdjx_consensus, vdjx_consensus_layout and vdjx_consensus_hits (include/vdjx.h) in plain Python: the units and their record, the votes of a
voter's walk, the decision of a column under the frequency threshold, and the rows as pseudo-contigs with V hits.  Integers only.  The hits are
the field dicts Context.annotate returns (arrays per field), the germlines the records as given to germline_load."""
from __future__ import annotations

import numpy as np

from tests import annot_model as A

SYMS = "ACGTN-"
INFO = ("contigs", "used", "truncated", "off_record", "units", "columns", "votes", "inserted", "undecided", "batches", "large_units")
UNIT = ("group", "gene", "members", "off_record", "lo", "hi", "off")
SHARE = 255                                                           # the voters a workgroup takes: a unit of more is a large unit
DEFAULT = (6000, 10000)


def _hit(v, i):
    return {f: (np.asarray(v[f][i]).tolist() if np.ndim(v[f][i]) else int(v[f][i])) for f in v}


def called(h):
    return h["gene"] >= 0 and h["score"] > 0


def usable(h):
    return called(h) and h["n_runs"] <= A.RUNS


def runs_of(h):
    return [(int(r) & 15, int(r) >> 4) for r in h["runs"][:h["n_runs"]]]


def votes_of(contig, h, limit):
    """[(record position, symbol index)] of one voter, and its inserted bases below the limit"""
    q, p = h["seq_start"] - 1, h["germ_start"] - 1
    out, inserted = [], 0
    for op, L in runs_of(h):
        if op == 0:
            for t in range(L):
                if q + t < limit:
                    ch = contig[q + t]
                    out.append((p + t, SYMS.index(ch) if ch in "ACGT" else 4))
            q += L
            p += L
        elif op == 2:
            if q < limit:
                out.extend((p + t, 5) for t in range(L))
            p += L
        else:
            inserted += max(0, min(L, limit - q))
            q += L
    return out, inserted


def decide(c, germ_ch, num, den):
    """the symbol index of a column with the counts c[6], and (cover, best)"""
    cover = sum(c)
    cand = (0, 1, 2, 3, 5)
    best = max(c[s] for s in cand)
    if cover == 0 or best == 0:
        return 4, cover, best
    top = [s for s in cand if c[s] == best]
    if len(top) == 1:
        sym = top[0]
    else:
        g = SYMS.index(germ_ch) if germ_ch in "ACGT" else -1
        sym = g if g in top else 4
    if best * den < num * cover:
        sym = 4
    return sym, cover, best


def layout(v, n, length, limit=None, group=None):
    """-> (unit per contig, [dict per unit] without lo / hi / off, the voters per unit, truncated, used)"""
    of_group, units, named = {}, [], []
    truncated = used = 0
    for i in range(n):
        h = _hit(v, i)
        if called(h) and not usable(h):
            truncated += 1
        if not usable(h):
            continue
        used += 1
        g = -1 if group is None or int(group[i]) < 0 else int(group[i])
        if g >= 0 and g in of_group:
            u = of_group[g]
        else:
            u = len(units)
            units.append(dict(group=g, contigs=[]))
            if g >= 0:
                of_group[g] = u
        units[u]["contigs"].append((i, h["gene"]))
    unit = [-1] * n
    for u, un in enumerate(units):
        tally = {}
        for _, gene in un["contigs"]:
            tally[gene] = tally.get(gene, 0) + 1
        un["gene"] = min(tally, key=lambda gene: (-tally[gene], gene))
        un["voters"] = [i for i, gene in un["contigs"] if gene == un["gene"]]
        un["members"] = len(un["voters"])
        un["off_record"] = len(un["contigs"]) - un["members"]
        for i in un["voters"]:
            unit[i] = u
    return unit, units, truncated, used


def consensus(contigs, v, germs, limit=None, group=None, min_freq=DEFAULT, cells=1 << 24):
    """-> dict(unit, units {field: list}, cons, germ (list of str), cover, best (list of lists), info)"""
    n = len(contigs)
    length = len(contigs[0]) if n else 0
    num, den = min_freq
    unit, units, truncated, used = layout(v, n, length, limit, group)
    cons, germ, cover, best = [], [], [], []
    inserted = votes = undecided = off = 0
    for un in units:
        table = {}
        for i in un["voters"]:
            vs, ins = votes_of(contigs[i], _hit(v, i), length if limit is None else int(limit[i]))
            inserted += ins
            for p, s in vs:
                table.setdefault(p, [0] * 6)[s] += 1
        lo, hi = (min(table), max(table) + 1) if table else (0, 0)
        rec = germs[un["gene"]]
        row, cv, bs = [], [], []
        for p in range(lo, hi):
            s, c, b = decide(table.get(p, [0] * 6), rec[p], num, den)
            row.append(SYMS[s])
            cv.append(c)
            bs.append(b)
            votes += c
            undecided += s == 4 and c > 0
        un.update(lo=lo, hi=hi, off=off)
        off += hi - lo
        cons.append("".join(row))
        germ.append("".join(ch if ch in "ACGT" else "N" for ch in rec[lo:hi]))
        cover.append(cv)
        best.append(bs)
    batches, held = 0, 0
    for k, un in enumerate(units):
        w = un["hi"] - un["lo"]
        if k == 0 or held + w > cells:
            batches, held = batches + 1, 0
        held += w
    info = dict(contigs=n, used=used, truncated=truncated, off_record=sum(un["off_record"] for un in units), units=len(units), columns=off,
                votes=votes, inserted=inserted, undecided=undecided, batches=batches if off else 0,
                large_units=sum(un["members"] > SHARE for un in units if un["hi"] > un["lo"]))
    return dict(unit=unit, units={f: [un[f] for un in units] for f in UNIT}, cons=cons, germ=germ, cover=cover, best=best, info=info)


def hits(units, cons, germ):
    """vdjx_consensus_hits -> (contigs, [hit dict per unit] with the fields of vdjx_annot_hit)"""
    rows = [c.replace("-", "") for c in cons]
    plen = max([1] + [len(r) for r in rows])
    out = []
    for u, (c, g) in enumerate(zip(cons, germ)):
        h = dict(gene=-1, score=0, n_tied=0, tied=[-1] * A.TIED, seq_start=0, seq_end=0, germ_start=0, germ_end=0, matches=0, mismatches=0, ins=0,
                 opens=0, n_runs=0, runs=[0] * A.RUNS, **{"del": 0})
        core = c.strip("-")
        if core:
            a = len(c) - len(c.lstrip("-"))
            gcore = g[a:a + len(core)]
            runs, k = [], 0
            while k < len(core):
                e = k
                while e < len(core) and (core[e] == "-") == (core[k] == "-"):
                    e += 1
                runs.append((e - k) << 4 | (2 if core[k] == "-" else 0))
                k = e
            m = sum(x == y and x in "ACGT" for x, y in zip(core, gcore))
            nd = core.count("-")
            h.update(gene=int(units["gene"][u]), score=max(1, m), n_tied=1, tied=[int(units["gene"][u])] + [-1] * (A.TIED - 1), seq_start=1,
                     seq_end=len(core) - nd, germ_start=int(units["lo"][u]) + a + 1, germ_end=int(units["lo"][u]) + a + len(core), matches=m,
                     mismatches=len(core) - nd - m, opens=sum(r & 15 == 2 for r in runs), n_runs=len(runs),
                     runs=(runs + [0] * (A.RUNS - len(runs))) if len(runs) <= A.RUNS else [0] * A.RUNS, **{"del": nd})
        out.append(h)
    return [r + "N" * (plen - len(r)) for r in rows], out


COLUMNS = ["clone_id", "sequence_id", "v_call", "members", "off_record", "germline_start", "germline_end", "consensus_alignment", "germline_alignment",
           "min_cover", "undecided", "v_germline_codons", "mu_count_v_r", "mu_count_v_s", "mu_count_v_stop", "mu_count_v_na", "mu_freq_v"]


def unit_ids(ids, res):
    """(clone_id, sequence_id of the first voter) per unit"""
    first = {}
    for i, u in enumerate(res["unit"]):
        if int(u) >= 0:
            first.setdefault(int(u), i)
    return [(f"lin_{int(g) + 1}" if int(g) >= 0 else "", ids[first[u]]) for u, g in enumerate(res["units"]["group"])]


def table_rows(ids, names, res, counts):
    """the rows of `vdjer --consensus` (lists of strings, COLUMNS); res: consensus() with cover; counts: vdjx_mutations' counts of the
    pseudo-contigs of hits() under their hits, J absent ({field: per unit})"""
    out = []
    for u, (clone_id, seq_id) in enumerate(unit_ids(ids, res)):
        un = {f: res["units"][f][u] for f in UNIT}
        cover = [int(x) for x in res["cover"][u]]
        row = [clone_id, seq_id, names[int(un["gene"])], str(int(un["members"])), str(int(un["off_record"])), str(int(un["lo"]) + 1), str(int(un["hi"])),
               res["cons"][u], res["germ"][u], str(min(cover) if cover else 0), str(sum(ch == "N" and c > 0 for ch, c in zip(res["cons"][u], cover)))]
        if int(counts["flags"][u]) & 1:
            cod, r, s = (int(counts[k][u]) for k in ("v_codons", "v_r", "v_s"))
            row += [str(cod), str(r), str(s), str(int(counts["v_stop"][u])), str(int(counts["v_na"][u])), "%.4f" % ((r + s) / (3 * cod)) if cod else ""]
        else:
            row += [""] * 6
        out.append(row)
    return out


def table_text(rows):
    return "".join("\t".join(r) + "\n" for r in [COLUMNS] + rows)


def summary_line(info, largest, num):
    return (f"consensus: {info['contigs']} contigs, {info['used']} used, {info['units']} units (largest {largest}), {info['off_record']} off the unit's record, "
            f"{info['columns']} columns, {info['undecided']} undecided, min share {num // 10000}.{num % 10000:04d}, {info['batches']} batches")
