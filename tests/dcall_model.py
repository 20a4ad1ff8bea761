"""The D-call model of include/vdjx.h (vdjx_dsegment_load, vdjx_dcall, `vdjer --airr --d-calls`) restated in numpy and plain Python.  A
window's hit is vdjx_annotate's alignment of the window substring, its coordinates shifted by the window's start: the traceback is
tests/annot_model.py's, the scores are annot_model.scores' computed for windows of unequal length at once (window_scores).  All integer,
so the device is compared bitwise."""
from __future__ import annotations

import numpy as np

from tests import annot_model as A

DEFAULT = dict(match=2, mismatch=3, gap_open=5, gap_extend=2, min_score=22)
WINDOW = 256                                                      # VDJX_DCALL_WINDOW
D_COLUMNS = ["d_score", "d_identity", "d_sequence_start", "d_sequence_end", "d_germline_start", "d_germline_end", "np1", "np1_length", "np2",
             "np2_length"]
AIRR_COLUMNS = A.AIRR_COLUMNS + D_COLUMNS


def _has(h, c):
    return h["gene"][c] >= 0 and h["score"][c] > 0


def d_window(v, j):
    """(start, length) int64 arrays: the bases strictly between a V and a J hit (0-based start v.seq_end, length j.seq_start - 1 -
    v.seq_end); length 0 and start 0 when the hits abut or overlap, when more than 256 bases lie between them, without a V or a J hit"""
    n = len(v["gene"])
    start, length = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for c in range(n):
        if not (_has(v, c) and _has(j, c)):
            continue
        l = int(j["seq_start"][c]) - 1 - int(v["seq_end"][c])
        if 0 < l <= WINDOW:
            start[c], length[c] = int(v["seq_end"][c]), l
    return start, length


def over_window(v, j):
    """how many contigs have more than 256 bases between their V and their J hit (the summary line's count)"""
    return sum(1 for c in range(len(v["gene"])) if _has(v, c) and _has(j, c) and int(j["seq_start"][c]) - 1 - int(v["seq_end"][c]) > WINDOW)


def window_scores(wins, records, p=DEFAULT):
    """S of every (window, record): [n, C] int64, S = annot_model.scores([w], records)[0] for every window w (tests/test_dcall_cpu.py
    checks that), for windows of unequal length in one pass: row by row over the windows, vectorised over windows and record columns.
    The dependency along a row is a running maximum: with Ht = max(0, diagonal + s, F), E[j] = max over k < j of Ht[k] - open - ext -
    (j - 1 - k) ext, because a gap opened from a cell that E itself made never beats extending that gap (open >= 0); H = max(Ht, E).
    Rows past a window's end and columns past a record's end are left out of the maximum, and no cell inside depends on them."""
    n, C = len(wins), len(records)
    S = np.zeros((n, C), np.int64)
    ma, mi, oe, ext = p["match"], p["mismatch"], p["gap_open"] + p["gap_extend"], p["gap_extend"]
    order = sorted((c for c in range(n) if wins[c]), key=lambda c: -len(wins[c]))
    if not order or not C:
        return S
    M = len(wins[order[0]])
    W = np.full((len(order), M), 6, np.int64)
    for k, c in enumerate(order):
        W[k, :len(wins[c])] = A._codes(wins[c], 4)
    wlen = np.array([len(wins[c]) for c in order])
    for idx in ([r for r in range(C) if len(records[r]) <= 64], [r for r in range(C) if len(records[r]) > 64]):      # (less padding)
        if not idx:
            continue
        G = max(len(records[r]) for r in idx)
        Gc = np.full((len(idx), G), 7, np.int64)
        for k, r in enumerate(idx):
            Gc[k, :len(records[r])] = A._codes(records[r], 5)
        glen = np.array([len(records[r]) for r in idx])
        valid = np.arange(1, G + 1)[None, :] <= glen[:, None]                                    # [K, G]
        ramp = np.arange(1, G + 1) * ext
        H = np.zeros((len(order), len(idx), G + 1), np.int64)
        F = np.full((len(order), len(idx), G + 1), A.NEG, np.int64)
        best = np.zeros((len(order), len(idx)), np.int64)
        for i in range(1, M + 1):
            na = int((wlen >= i).sum())                                                           # (the windows are sorted: the first na are still running)
            Hp, Fp = H[:na], F[:na]
            s = np.where(W[:na, i - 1][:, None, None] == Gc[None], ma, -mi)
            f = np.maximum(Fp[:, :, 1:] - ext, Hp[:, :, 1:] - oe)
            ht = np.maximum(np.maximum(Hp[:, :, :-1] + s, 0), f)
            run = np.maximum.accumulate(ht + ramp, axis=2)                                        # max over k <= j of Ht[k] + k ext
            e = np.full_like(ht, A.NEG)
            e[:, :, 1:] = run[:, :, :-1] - oe - ramp[:-1]                                         # E[j], j >= 2: ... - open - ext - (j - 1) ext
            h = np.maximum(ht, e)
            best[:na] = np.maximum(best[:na], np.where(valid[None], h, 0).max(axis=2))
            Hp[:, :, 1:] = h
            Fp[:, :, 1:] = f
        for k, c in enumerate(order):
            S[c, idx] = best[k]
    return S


def dcall(contigs, win_start, win_len, records, p=DEFAULT):
    """the model of vdjx_dcall: ({field: array} as api.Context.dcall's "d", S int64[n, C]); a window's hit is annot_model's traceback of
    the window substring, its coordinates shifted by the window's start"""
    n, C = len(contigs), len(records)
    f = {k: np.zeros(n, np.int64) for k in A.FIELDS if k not in ("tied", "runs")}
    f["tied"] = np.full((n, A.TIED), -1, np.int64)
    f["runs"] = np.zeros((n, A.RUNS), np.int64)
    if n == 0:
        return f, np.zeros((0, C), np.int64)
    wins = [s[int(a):int(a) + int(l)] for s, a, l in zip(contigs, win_start, win_len)]
    assert all(len(w) == int(l) for w, l in zip(wins, win_len))                # (the window lies inside the contig)
    uniq = sorted(set(wins))                                                   # (equal windows score alike)
    at = {w: k for k, w in enumerate(uniq)}
    S = window_scores(uniq, records, p)[[at[w] for w in wins]]
    for c in range(n):
        best = int(S[c].max()) if C else -1
        f["score"][c] = max(best, 0)
        if best < 0 or best < p["min_score"] or not wins[c]:
            f["gene"][c] = -1
            continue
        tied = np.flatnonzero(S[c] == best).tolist()
        f["gene"][c], f["n_tied"][c] = tied[0], len(tied)
        f["tied"][c, :min(A.TIED, len(tied))] = tied[:A.TIED]
        if best > 0:
            tb = A.traceback(wins[c], records[tied[0]], p)
            assert tb["score"] == best
            for k in ("germ_start", "germ_end", "matches", "mismatches", "ins", "opens", "n_runs"):
                f[k][c] = tb[k]
            f["seq_start"][c], f["seq_end"][c] = tb["seq_start"] + int(win_start[c]), tb["seq_end"] + int(win_start[c])
            f["del"][c] = tb["dele"]
            f["runs"][c] = A.encode_runs(tb["ops"])
    return f, S


def airr_rows(ids, seqs, hits, names, d, d_names, counts=None):
    """the rows of `vdjer --airr --d-calls` (AIRR_COLUMNS [+ expected_count]): annot_model.airr_rows' with d_call and d_cigar filled and
    the ten columns after j_germline_end.  hits: the V / J hits; d: dcall()'s hits of the d_window windows; d_names: the D set's names"""
    rows = []
    hv, hj = hits["v"], hits["j"]
    for c, row in enumerate(A.airr_rows(ids, seqs, hits, names, counts)):
        s = seqs[c]
        called, ok = d["gene"][c] >= 0, _has(d, c)
        row[5] = ",".join(d_names[g] for g in d["tied"][c][:min(A.TIED, d["n_tied"][c])]) if called else ""
        row[16] = A.cigar(d, c, len(s))
        ident = ""
        if ok:
            ident = "%.4f" % (d["matches"][c] / (d["matches"][c] + d["mismatches"][c] + d["ins"][c] + d["del"][c]))
        cells = [str(int(d["score"][c])) if called else "", ident] + [str(int(d[k][c])) if ok else "" for k in ("seq_start", "seq_end", "germ_start", "germ_end")]
        if _has(hv, c) and _has(hj, c):
            v_end, j_at = int(hv["seq_end"][c]), int(hj["seq_start"][c]) - 1       # (0-based: the gap is s[v_end:j_at])
            np1 = s[v_end:int(d["seq_start"][c]) - 1] if ok else s[v_end:max(j_at, v_end)]
            np2 = s[int(d["seq_end"][c]):j_at] if ok else ""
            cells += [np1, str(len(np1)), np2, str(len(np2))]
        else:
            cells += ["", "", "", ""]
        at = len(A.AIRR_COLUMNS)
        rows.append(row[:at] + cells + row[at:])
    return rows
