"""The germline-row and mutation-count model of include/vdjx.h (vdjx_mutations_layout, vdjx_mutations, `vdjer --mutations`) restated in
plain Python, column by column: the device is tested against this, byte for byte and count for count (all integer).  The V / J hits come
from tests/annot_model.py, the D hits from tests/dcall_model.py; nothing here reads the product."""
from __future__ import annotations

import numpy as np

from tests import annot_model as A

RUNS = A.RUNS
COUNTS = ["cols", "v_r", "v_s", "v_stop", "v_na", "v_codons", "j_mis", "flags"]
INFO = ["contigs", "aligned", "cols", "v_r", "v_s", "v_stop", "v_na", "v_codons", "truncated", "clipped"]
COLUMNS = ["sequence_id", "v_call", "j_call", "sequence_alignment", "germline_alignment", "germline_alignment_d_mask", "v_germline_codons",
           "mu_count_v_r", "mu_count_v_s", "mu_count_v_stop", "mu_count_v_na", "mu_freq_v", "mu_count_j"]
F_V, F_J, F_D, F_CLIP, F_TRUNC = 1, 2, 4, 8, 16


def _called(h, c):
    return h is not None and h["gene"][c] >= 0 and h["score"][c] > 0


def _usable(h, c):
    return _called(h, c) and h["n_runs"][c] <= RUNS


def _ops(h, c):
    """the hit's runs as [(op, length)], op in "MID" """
    return [("MID"[int(r) & 15], int(r) >> 4) for r in h["runs"][c][:int(h["n_runs"][c])]]


def _germ_char(ch):
    return ch if ch in "ACGT" else "N"


def _hit_columns(h, c, germ):
    """the columns of a hit by its runs: [(op, contig position 1-based or 0, germline position 1-based or 0)]"""
    out = []
    p, g = int(h["seq_start"][c]), int(h["germ_start"][c])
    for op, L in _ops(h, c):
        for _ in range(L):
            if op == "M":
                out.append(("M", p, g))
                p, g = p + 1, g + 1
            elif op == "I":
                out.append(("I", p, 0))
                p += 1
            else:
                out.append(("D", 0, g))
                g += 1
    return out


def columns(c, v, d, j):
    """contig c's columns from the hits alone -> ([(region, op, contig position, germline position)], flags, truncated hits); region "V",
    "G" (the gap: np1, D's columns, np2) or "J"; op "M", "I", "D" or "N" (a gap column outside the D hit)"""
    trunc = sum(1 for h in (v, d, j) if _called(h, c) and not _usable(h, c))
    flags = F_TRUNC if trunc else 0
    if not _usable(v, c):
        return [], flags, trunc
    flags |= F_V
    cols = [("V",) + x for x in _hit_columns(v, c, None)]
    if not _usable(j, c):
        return cols, flags, trunc
    v_end = int(v["seq_end"][c])
    jc = _hit_columns(j, c, None)
    if int(j["seq_start"][c]) <= v_end:
        flags |= F_CLIP
        first = next((k for k, x in enumerate(jc) if x[1] > v_end), None)
        if first is None:
            return cols, flags, trunc
        jc = jc[first:]
        g1 = jc[0][1] - 1
    else:
        g1 = int(j["seq_start"][c]) - 1
    flags |= F_J
    if _usable(d, c) and int(d["seq_start"][c]) > v_end and int(d["seq_end"][c]) <= g1:
        flags |= F_D
        cols += [("G", "N", p, 0) for p in range(v_end + 1, int(d["seq_start"][c]))]
        cols += [("G",) + x for x in _hit_columns(d, c, None)]
        cols += [("G", "N", p, 0) for p in range(int(d["seq_end"][c]) + 1, g1 + 1)]
    else:
        cols += [("G", "N", p, 0) for p in range(v_end + 1, g1 + 1)]
    cols += [("J",) + x for x in jc]
    return cols, flags, trunc


def layout(v, d, j):
    """vdjx_mutations_layout: uint64[n + 1]"""
    n = len(v["gene"])
    off = np.zeros(n + 1, np.uint64)
    for c in range(n):
        off[c + 1] = off[c] + np.uint64(len(columns(c, v, d, j)[0]))
    return off


def _aa(cod):
    return A.translate(cod)


def mutations(contigs, v, d, j, limit, germs, d_germs):
    """the model of vdjx_mutations -> (rows, counts, info): rows = {"seq", "germ", "mask": list[str]}, counts = {field: int64[n]}, info =
    dict.  germs: the records as given to vdjx_germline_load (v / j genes index them); d_germs: those given to vdjx_dsegment_load"""
    n = len(contigs)
    rows = {"seq": [], "germ": [], "mask": []}
    counts = {k: np.zeros(n, np.int64) for k in COUNTS}
    info = dict.fromkeys(INFO, 0)
    info["contigs"] = n
    for c in range(n):
        s = contigs[c]
        lim = len(s) if limit is None else int(limit[c])
        cols, flags, trunc = columns(c, v, d, j)
        info["truncated"] += trunc
        rec = {"V": germs[int(v["gene"][c])] if flags & F_V else "", "J": germs[int(j["gene"][c])] if flags & F_J else "",
               "G": d_germs[int(d["gene"][c])] if flags & F_D else ""}
        seq = "".join("-" if op == "D" else s[p - 1] for _, op, p, _ in cols)
        germ = "".join("-" if op == "I" else "N" if op == "N" else _germ_char(rec[reg][g - 1]) for reg, op, _, g in cols)
        mask = "".join("N" if reg == "G" else ch for (reg, _, _, _), ch in zip(cols, germ))
        rows["seq"].append(seq)
        rows["germ"].append(germ)
        rows["mask"].append(mask)
        counts["cols"][c], counts["flags"][c] = len(cols), flags
        # V: the germline's codons
        where = {g: k for k, (reg, op, p, g) in enumerate(cols) if reg == "V" and op == "M"}       # germline position -> column
        classified = set()
        if flags & F_V:
            gs, ge = int(v["germ_start"][c]), int(v["germ_end"][c])
            for cod in range(len(rec["V"]) // 3):
                gp = [3 * cod + 1, 3 * cod + 2, 3 * cod + 3]
                if gp[0] < gs or gp[2] > ge or any(g not in where for g in gp):
                    continue
                ks = [where[g] for g in gp]
                if ks[1] != ks[0] + 1 or ks[2] != ks[1] + 1 or any(cols[k][2] - 1 >= lim for k in ks):
                    continue
                gc, cc = "".join(rec["V"][g - 1] for g in gp), "".join(s[cols[k][2] - 1] for k in ks)
                if any(ch not in "ACGT" for ch in gc + cc):
                    continue
                counts["v_codons"][c] += 1
                classified.update(ks)
                for b in range(3):
                    if cc[b] == gc[b]:
                        continue
                    changed = gc[:b] + cc[b] + gc[b + 1:]
                    if _aa(gc) == "*" or _aa(changed) == "*":
                        counts["v_stop"][c] += 1
                    elif _aa(gc) == _aa(changed):
                        counts["v_s"][c] += 1
                    else:
                        counts["v_r"][c] += 1
        for k, (reg, op, p, g) in enumerate(cols):
            if op != "M" or reg == "G":
                continue
            a, b = s[p - 1], rec[reg][g - 1]
            mism = a != b or a not in "ACGT" or b not in "ACGT"
            if reg == "V" and k not in classified and p - 1 < lim and mism:
                counts["v_na"][c] += 1
            if reg == "J" and mism:
                counts["j_mis"][c] += 1
        info["aligned"] += bool(flags & F_V)
        info["clipped"] += bool(flags & F_CLIP)
        for k in ("cols", "v_r", "v_s", "v_stop", "v_na", "v_codons"):
            info[k] += int(counts[k][c])
    return rows, counts, info


def mutation_limit(ids, contigs):
    """vdjer's rule: the junction's 0-based start plus 3 (through the conserved Cys codon); the contig's length when it is not found"""
    out = np.zeros(len(ids), np.int64)
    for c, (cid, s) in enumerate(zip(ids, contigs)):
        p = A.junction_of(cid, s)[1]
        out[c] = min(p + 3, len(s)) if p >= 0 else len(s)
    return out


def table_rows(ids, hits, names, rows, counts, clone=None):
    """the rows of `vdjer --mutations` (lists of strings, COLUMNS [+ clone_id]); clone: int[n] (-1: none) when --lineages is given"""
    out = []
    for c, cid in enumerate(ids):
        def call(h):
            return ",".join(names[g] for g in h["tied"][c][:min(A.TIED, h["n_tied"][c])]) if h["gene"][c] >= 0 else ""
        row = [cid, call(hits["v"]), call(hits["j"])]
        if int(counts["flags"][c]) & F_V:
            cod, r, s = (int(counts[k][c]) for k in ("v_codons", "v_r", "v_s"))
            row += [rows["seq"][c], rows["germ"][c], rows["mask"][c], str(cod), str(r), str(s), str(int(counts["v_stop"][c])),
                    str(int(counts["v_na"][c])), "%.4f" % ((r + s) / (3 * cod)) if cod else "", str(int(counts["j_mis"][c]))]
        else:
            row += [""] * 10
        if clone is not None:
            row.append(f"lin_{int(clone[c]) + 1}" if int(clone[c]) >= 0 else "")
        out.append(row)
    return out


def summary_line(info):
    return ("mutations: %d contigs, %d aligned, %d columns, %d V codons, %d R, %d S, %d stop, %d unclassified, %d J clipped, %d over 64 runs"
            % (info["contigs"], info["aligned"], info["cols"], info["v_codons"], info["v_r"], info["v_s"], info["v_stop"], info["v_na"],
               info["clipped"], info["truncated"]))
