"""The contig-annotation model of include/vdjx.h (vdjx_germline_load, vdjx_annotate, `vdjer --airr`) restated in numpy and plain Python:
the device is tested against this, field for field (all integer, so bitwise)."""
from __future__ import annotations

import numpy as np

DEFAULT = dict(match=2, mismatch=3, gap_open=5, gap_extend=2, min_v_score=40, min_j_score=20)
NEG = -(1 << 40)
TIED = 8
RUNS = 64
FIELDS = ["gene", "score", "n_tied", "tied", "seq_start", "seq_end", "germ_start", "germ_end", "matches", "mismatches", "ins", "del",
          "opens", "n_runs", "runs"]
AIRR_COLUMNS = ["sequence_id", "sequence", "rev_comp", "productive", "v_call", "d_call", "j_call", "sequence_alignment", "germline_alignment",
                "junction", "junction_aa", "cdr3", "cdr3_aa", "vj_in_frame", "stop_codon", "v_cigar", "d_cigar", "j_cigar",
                "v_score", "v_identity", "v_sequence_start", "v_sequence_end", "v_germline_start", "v_germline_end",
                "j_score", "j_identity", "j_sequence_start", "j_sequence_end", "j_germline_start", "j_germline_end"]


# ---- germline records ----------------------------------------------------------------------------------------------------------------
def parse_name(header):
    tok = header.split()[0] if header.split() else ""
    return tok.split("|")[1] if "|" in tok else tok


def parse_class(name):
    if len(name) >= 4 and ((name[:2] == "IG" and name[2] in "HKL") or (name[:2] == "TR" and name[2] in "ABDG")):
        return name[3]
    return name[:1]


def clean(seq):
    return "".join(c for c in seq.upper() if c not in ". \t\r\n")


# ---- scoring -------------------------------------------------------------------------------------------------------------------------
def _codes(s, other):
    a = np.frombuffer(s.encode(), np.uint8)
    out = np.full(a.shape, other, np.int64)
    for k, ch in enumerate(b"ACGT"):
        out[a == ch] = k
    return out


def scores(contigs, germs, p=DEFAULT):
    """S of every (contig, germline): [n, K] int64.  Gotoh by anti-diagonals, vectorised over all pairs (germlines padded at their 3'
    end: a padded column never feeds a real one)."""
    n, K = len(contigs), len(germs)
    if n == 0 or K == 0:
        return np.zeros((n, K), np.int64)
    m = len(contigs[0])
    G = max(len(g) for g in germs)
    C = np.stack([_codes(c, 4) for c in contigs])                          # [n, m]
    Gc = np.full((K, G + 1), 5, np.int64)
    for k, g in enumerate(germs):
        Gc[k, 1:len(g) + 1] = _codes(g, 5)
    glen = np.array([len(g) for g in germs])
    ma, mi, oe, ext = p["match"], p["mismatch"], p["gap_open"] + p["gap_extend"], p["gap_extend"]
    # diagonal buffers indexed by i (0..m): H of d-1 and d-2, E and F of d-1
    H1 = np.zeros((n, K, m + 1), np.int64)
    H2 = np.zeros((n, K, m + 1), np.int64)
    E1 = np.full((n, K, m + 1), NEG, np.int64)
    F1 = np.full((n, K, m + 1), NEG, np.int64)
    S = np.zeros((n, K), np.int64)
    for d in range(2, m + G + 1):
        lo, hi = max(1, d - G), min(m, d - 1)
        if lo > hi:
            continue
        i = np.arange(lo, hi + 1)
        j = d - i
        H0 = np.zeros_like(H1)
        E0 = np.full_like(E1, NEG)
        F0 = np.full_like(F1, NEG)
        diag = np.where((i > 1) & (j > 1), H2[:, :, i - 1], 0)
        hl = np.where(j > 1, H1[:, :, i], 0)
        el = np.where(j > 1, E1[:, :, i], NEG)
        hu = np.where(i > 1, H1[:, :, i - 1], 0)
        fu = np.where(i > 1, F1[:, :, i - 1], NEG)
        s = np.where(C[:, None, i - 1] == Gc[None, :, j], ma, -mi)
        e = np.maximum(el - ext, hl - oe)
        f = np.maximum(fu - ext, hu - oe)
        h = np.maximum(np.maximum(diag + s, 0), np.maximum(e, f))
        H0[:, :, i], E0[:, :, i], F0[:, :, i] = h, e, f
        valid = j[None, :] <= glen[:, None]                                   # [K, cells]
        S = np.maximum(S, np.where(valid[None], h, 0).max(axis=2))
        H2, H1, E1, F1 = H1, H0, E0, F0
    return S


def matrices(contig, germ, p=DEFAULT):
    """the full H, E, F of one pair, [m + 1, g + 1] (plain loops)"""
    m, g = len(contig), len(germ)
    ma, mi, op, ext = p["match"], p["mismatch"], p["gap_open"], p["gap_extend"]
    H = [[0] * (g + 1) for _ in range(m + 1)]
    E = [[NEG] * (g + 1) for _ in range(m + 1)]
    F = [[NEG] * (g + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        a = contig[i - 1]
        for j in range(1, g + 1):
            s = ma if (a == germ[j - 1] and a in "ACGT") else -mi
            E[i][j] = max(E[i][j - 1] - ext, H[i][j - 1] - op - ext)
            F[i][j] = max(F[i - 1][j] - ext, H[i - 1][j] - op - ext)
            H[i][j] = max(0, H[i - 1][j - 1] + s, E[i][j], F[i][j])
    return H, E, F


def traceback(contig, germ, p=DEFAULT):
    """the alignment of one pair by the rules of include/vdjx.h -> dict of vdjx_annot_hit's alignment fields"""
    H, E, F = matrices(contig, germ, p)
    m, g = len(contig), len(germ)
    S = max(max(r) for r in H)
    out = dict(score=S, seq_start=0, seq_end=0, germ_start=0, germ_end=0, matches=0, mismatches=0, ins=0, dele=0, opens=0, n_runs=0, ops=[])
    if S == 0:
        return out
    ie, je = next((i, j) for i in range(1, m + 1) for j in range(1, g + 1) if H[i][j] == S)
    ma, mi, oe, ext = p["match"], p["mismatch"], p["gap_open"] + p["gap_extend"], p["gap_extend"]
    i, j, st, ops = ie, je, "H", []
    while True:
        if st == "H":
            if i == 0 or j == 0 or H[i][j] == 0:
                break
            s = ma if (contig[i - 1] == germ[j - 1] and contig[i - 1] in "ACGT") else -mi
            if H[i][j] == H[i - 1][j - 1] + s:
                ops.append("M")
                out["matches" if s > 0 else "mismatches"] += 1
                i, j = i - 1, j - 1
            elif H[i][j] == E[i][j]:
                st = "E"
            else:
                st = "F"
        elif st == "E":
            ops.append("D")
            out["dele"] += 1
            if E[i][j] == H[i][j - 1] - oe:
                out["opens"] += 1
                st = "H"
            j -= 1
        else:
            ops.append("I")
            out["ins"] += 1
            if F[i][j] == H[i - 1][j] - oe:
                out["opens"] += 1
                st = "H"
            i -= 1
    ops.reverse()
    runs = []
    for o in ops:
        if runs and runs[-1][1] == o:
            runs[-1][0] += 1
        else:
            runs.append([1, o])
    out.update(seq_start=i + 1, seq_end=ie, germ_start=j + 1, germ_end=je, n_runs=len(runs), ops=runs, score=S)
    return out


def trace_fast(contig, germ, p=DEFAULT):
    """traceback()'s dict, computed by anti-diagonals in numpy (int64, E and F unclamped) with a direction byte per cell instead of the
    three matrices: bits 0-1 where H came from (0 stop, 1 diagonal, 2 E, 3 F, in that order of preference), bit 2 E opened here, bit 3
    F opened here.  For pairs whose matrices plain Python cannot hold (4,095 x 2,047: about 1.5 s)."""
    m, g = len(contig), len(germ)
    ma, mi, oe, ext = p["match"], p["mismatch"], p["gap_open"] + p["gap_extend"], p["gap_extend"]
    out = dict(score=0, seq_start=0, seq_end=0, germ_start=0, germ_end=0, matches=0, mismatches=0, ins=0, dele=0, opens=0, n_runs=0, ops=[])
    if m == 0 or g == 0:
        return out
    cc, gc = _codes(contig, 4), _codes(germ, 5)
    dirs = np.zeros(m * g, np.uint8)                                          # cell (i, j) at (i - 1) * g + (j - 1)
    # diagonals indexed by i (0 .. m): H of d-1 and d-2, E and F of d-1; an entry a diagonal does not write is a border cell (0, -inf)
    H1, H2 = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)
    E1, F1 = np.full(m + 1, NEG, np.int64), np.full(m + 1, NEG, np.int64)
    S, end = 0, -1
    for d in range(2, m + g + 1):
        lo, hi = max(1, d - g), min(m, d - 1)
        i = np.arange(lo, hi + 1)
        j = d - i
        s = np.where(cc[i - 1] == gc[j - 1], ma, -mi)
        eo, fo = H1[lo:hi + 1] - oe, H1[lo - 1:hi] - oe
        e = np.maximum(E1[lo:hi + 1] - ext, eo)
        f = np.maximum(F1[lo - 1:hi] - ext, fo)
        dg = H2[lo - 1:hi] + s
        h = np.maximum(np.maximum(dg, 0), np.maximum(e, f))
        src = np.where(h == 0, 0, np.where(h == dg, 1, np.where(h == e, 2, 3)))
        at = (i - 1) * g + (j - 1)
        dirs[at] = src | np.where(e == eo, 4, 0) | np.where(f == fo, 8, 0)
        top = int(h.max())
        if top > S:
            S, end = top, -1
        if top == S and S > 0:
            first = int(at[h == S].min())
            end = first if end < 0 else min(end, first)
        H0, E0, F0 = np.zeros(m + 1, np.int64), np.full(m + 1, NEG, np.int64), np.full(m + 1, NEG, np.int64)
        H0[lo:hi + 1], E0[lo:hi + 1], F0[lo:hi + 1] = h, e, f
        H2, H1, E1, F1 = H1, H0, E0, F0
    if S == 0:
        return out
    ie, je = end // g + 1, end % g + 1
    i, j, st, ops = ie, je, "H", []
    while True:
        dv = int(dirs[(i - 1) * g + (j - 1)]) if i > 0 and j > 0 else 0
        if st == "H":
            if dv & 3 == 0:
                break
            if dv & 3 == 1:
                ops.append("M")
                out["matches" if cc[i - 1] == gc[j - 1] else "mismatches"] += 1
                i, j = i - 1, j - 1
            else:
                st = "E" if dv & 3 == 2 else "F"
        elif st == "E":
            ops.append("D")
            out["dele"] += 1
            if dv & 4:
                out["opens"] += 1
                st = "H"
            j -= 1
        else:
            ops.append("I")
            out["ins"] += 1
            if dv & 8:
                out["opens"] += 1
                st = "H"
            i -= 1
    ops.reverse()
    runs = []
    for o in ops:
        if runs and runs[-1][1] == o:
            runs[-1][0] += 1
        else:
            runs.append([1, o])
    out.update(seq_start=i + 1, seq_end=ie, germ_start=j + 1, germ_end=je, n_runs=len(runs), ops=runs, score=S)
    return out


def encode_runs(runs):
    code = {"M": 0, "I": 1, "D": 2}
    r = [(l << 4) | code[o] for l, o in runs] if len(runs) <= RUNS else []
    return r + [0] * (RUNS - len(r))


def _scores_by_length(contigs, germs, p):
    """scores(), the records taken in groups of similar length (each longer than half the group's longest), so that a short record is
    not padded to the longest one's columns"""
    S = np.zeros((len(contigs), len(germs)), np.int64)
    left = sorted(range(len(germs)), key=lambda k: -len(germs[k]))
    while left:
        grp = [k for k in left if 2 * len(germs[k]) > len(germs[left[0]])]
        S[:, grp] = scores(contigs, [germs[k] for k in grp], p)
        left = left[len(grp):]
    return S


def annotate(contigs, germs, classes, p=DEFAULT, fast=False):
    """the model of vdjx_annotate: {"v": {field: array}, "j": {...}} as api.Context.annotate returns them.  fast: the primary hits by
    trace_fast, and every distinct contig computed once (for long contigs against long records)"""
    if fast:
        first = {}
        order = [first.setdefault(c, len(first)) for c in contigs]
        if len(first) < len(contigs):
            h = annotate(list(first), germs, classes, p, fast=True)
            return {key: {f: v[order] for f, v in h[key].items()} for key in h}
    n = len(contigs)
    out = {}
    for cls, key, mn in (("V", "v", p["min_v_score"]), ("J", "j", p["min_j_score"])):
        idx = [r for r, c in enumerate(classes) if c == cls]
        S = (_scores_by_length if fast else scores)(contigs, [germs[r] for r in idx], p) if idx else np.zeros((n, 0), np.int64)
        f = {k: np.zeros(n, np.int64) for k in FIELDS if k not in ("tied", "runs")}
        f["tied"] = np.full((n, TIED), -1, np.int64)
        f["runs"] = np.zeros((n, RUNS), np.int64)
        for c in range(n):
            best = int(S[c].max()) if idx else -1
            f["score"][c] = max(best, 0)
            if best < 0 or best < mn:
                f["gene"][c] = -1
                continue
            tied = [idx[k] for k in np.flatnonzero(S[c] == best)]
            f["gene"][c], f["n_tied"][c] = tied[0], len(tied)
            f["tied"][c, :min(TIED, len(tied))] = tied[:TIED]
            if best > 0:
                tb = (trace_fast if fast else traceback)(contigs[c], germs[tied[0]], p)
                assert tb["score"] == best
                for k in ("seq_start", "seq_end", "germ_start", "germ_end", "matches", "mismatches", "ins", "opens", "n_runs"):
                    f[k][c] = tb[k]
                f["del"][c] = tb["dele"]
                f["runs"][c] = encode_runs(tb["ops"])
        out[key] = f
    return out


# ---- junction-derived fields and the AIRR row ---------------------------------------------------------------------------------------
_B = "TCAG"
_AA = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"


def translate(s):
    out = []
    for q in range(0, len(s) - len(s) % 3, 3):
        cod = s[q:q + 3]
        out.append(_AA[16 * _B.index(cod[0]) + 4 * _B.index(cod[1]) + _B.index(cod[2])] if all(ch in _B for ch in cod) else "X")
    return "".join(out)


def junction_of(cid, seq):
    """(junction, its 0-based start in seq or -1)"""
    parts = cid.split("_", 2)
    if len(parts) < 3 or not parts[2]:
        return "", -1
    p = seq.find(parts[2])
    return (parts[2], p) if p >= 0 else ("", -1)


def cigar(h, c, m):
    if h["gene"][c] < 0 or h["score"][c] <= 0 or h["n_runs"][c] > RUNS:
        return ""
    out = ""
    if h["seq_start"][c] > 1:
        out += f"{h['seq_start'][c] - 1}S"
    if h["germ_start"][c] > 1:
        out += f"{h['germ_start'][c] - 1}N"
    for r in h["runs"][c][:h["n_runs"][c]]:
        out += f"{int(r) >> 4}{'MID'[int(r) & 15]}"
    if h["seq_end"][c] < m:
        out += f"{m - h['seq_end'][c]}S"
    return out


def airr_rows(ids, seqs, hits, names, counts=None):
    """the AIRR rows of `vdjer --airr` (lists of strings, AIRR_COLUMNS [+ expected_count])"""
    rows = []
    hv, hj = hits["v"], hits["j"]
    for c, (cid, s) in enumerate(zip(ids, seqs)):
        m = len(s)
        junc, p = junction_of(cid, s)
        hasv, hasj = hv["gene"][c] >= 0 and hv["score"][c] > 0, hj["gene"][c] >= 0 and hj["score"][c] > 0
        inframe = bool(p >= 0 and hasv and len(junc) % 3 == 0 and (p - (hv["seq_start"][c] - 1) + (hv["germ_start"][c] - 1)) % 3 == 0)
        stop = False
        if p >= 0 and hasv and hasj:
            lo, hi = hv["seq_start"][c] - 1, hj["seq_end"][c] - 1
            q = p % 3
            while q + 2 <= hi:
                if q >= lo and translate(s[q:q + 3]) == "*":
                    stop = True
                    break
                q += 3
        prod = hasv and hasj and inframe and not stop

        def call(h):
            return ",".join(names[g] for g in h["tied"][c][:min(TIED, h["n_tied"][c])]) if h["gene"][c] >= 0 else ""

        def num(h, f, ok):
            return str(int(h[f][c])) if ok else ""

        def ident(h, ok):
            if not ok:
                return ""
            d = h["matches"][c] + h["mismatches"][c] + h["ins"][c] + h["del"][c]
            return "%.4f" % (h["matches"][c] / d)

        cdr3 = junc[3:-3] if len(junc) >= 6 else ""
        row = [cid, s, "F", "T" if prod else "F", call(hv), "", call(hj), "", "", junc, translate(junc), cdr3, translate(cdr3),
               "T" if inframe else "F", "T" if stop else "F", cigar(hv, c, m), "", cigar(hj, c, m)]
        for h, ok in ((hv, hasv), (hj, hasj)):
            row += [num(h, "score", h["gene"][c] >= 0), ident(h, ok)] + [num(h, f, ok) for f in ("seq_start", "seq_end", "germ_start", "germ_end")]
        if counts is not None:
            row.append("%.2f" % counts[c])
        rows.append(row)
    return rows


def read_table(path):
    lines = open(path).read().splitlines()
    return lines[0].split("\t"), [l.split("\t") for l in lines[1:]]
