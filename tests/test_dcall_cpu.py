"""The D-call model of include/vdjx.h (vdjx_dcall) on hand-checked cases, the window rule of `vdjer --airr --d-calls` (the model's and
vdjer_amd/annot.py's), the figures behind the default min_score, the table rows, the ABI mirror and the command line up to where a GPU
would be needed.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np

from tests import annot_model as A
from tests import dcall_model as D
from tests.test_isotype_cpu import EXE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D0 = "GGTATAGCAGCAGCTGGTAC"
D1 = "TTGACTACGGTGACTAC"


def _rand(rng, n):
    return "".join(rng.choice(list("ACGT"), int(n)))


def _one(window, records, p=D.DEFAULT, before="TTTTTTTTTT", after="TTTTTTTTTT"):
    """the hit of one window that lies between `before` and `after` in its contig"""
    h, S = D.dcall([before + window + after], [len(before)], [len(window)], records, p)
    return {k: (v[0].tolist() if v.ndim > 1 else int(v[0])) for k, v in h.items()}, S[0].tolist()


# ---- hand-checked calls ----------------------------------------------------------------------------------------------------------------
def test_exact_cut_is_called_in_contig_coordinates():
    # D0[3:17] (14 bases) between CCC and CCC: neither flank extends the match (D0 has T on both sides of the cut)
    h, S = _one("CCC" + D0[3:17] + "CCC", [D0, D1])
    assert (h["gene"], h["score"], h["n_tied"], h["tied"]) == (0, 28, 1, [0] + [-1] * 7)
    assert (h["seq_start"], h["seq_end"], h["germ_start"], h["germ_end"]) == (14, 27, 4, 17)          # (window start 10 + 3, 1-based)
    assert (h["matches"], h["mismatches"], h["ins"], h["del"], h["opens"], h["n_runs"]) == (14, 0, 0, 0, 0, 1)
    assert h["runs"][0] == 14 << 4 and not any(h["runs"][1:])
    assert S[0] == 28 and S[1] < 22


def test_cut_with_a_substitution():
    cut = D0[3:10] + "T" + D0[11:17]                               # (C -> T in the middle: 13 matches and a mismatch, 26 - 3)
    h, S = _one("CCC" + cut + "CCC", [D0, D1])
    assert (h["gene"], h["score"], h["matches"], h["mismatches"], h["opens"]) == (0, 23, 13, 1, 0)
    assert (h["seq_start"], h["seq_end"], h["germ_start"], h["germ_end"], h["n_runs"], h["runs"][0]) == (14, 27, 4, 17, 1, 14 << 4)


def test_tie_between_two_identical_records():
    h, S = _one("CCC" + D0[3:17] + "CCC", [D0, D1, D0])
    assert (h["gene"], h["score"], h["n_tied"], h["tied"][:3]) == (0, 28, 2, [0, 2, -1])
    assert S[0] == S[2] == 28


def test_empty_window_and_score_below_the_minimum():
    h, S = _one("", [D0, D1])
    assert (h["gene"], h["score"], h["n_tied"], h["tied"], h["seq_start"], h["n_runs"]) == (-1, 0, 0, [-1] * 8, 0, 0) and S == [0, 0]
    # even with min_score 0 an empty window is no call
    h, _ = _one("", [D0, D1], dict(D.DEFAULT, min_score=0))
    assert (h["gene"], h["n_tied"]) == (-1, 0)
    # ten matched bases: S = 20 < 22 -- no call, the score all the same; with min_score 20 it is one
    win = "CCCCC" + D0[3:13] + "AAAAA"
    h, S = _one(win, [D0, D1])
    assert (h["gene"], h["score"], h["n_tied"], h["tied"], h["seq_start"], h["seq_end"], h["n_runs"]) == (-1, 20, 0, [-1] * 8, 0, 0, 0) and S[0] == 20
    h, _ = _one(win, [D0, D1], dict(D.DEFAULT, min_score=20))
    assert (h["gene"], h["score"], h["seq_start"], h["seq_end"]) == (0, 20, 16, 25)
    # no record at all: no call, score 0
    h, S = _one(win, [])
    assert (h["gene"], h["score"], h["n_tied"]) == (-1, 0, 0) and S == []


def test_bases_outside_the_window_do_not_count():
    # the whole of D0 lies in the contig, but the window holds only its first 12 bases
    h, S = _one(D0[:12], [D0], before="ACACACACAC", after=D0[12:] + "ACAC")
    assert (h["score"], h["seq_start"], h["seq_end"], h["germ_start"], h["germ_end"]) == (24, 11, 22, 1, 12)
    whole, _ = _one(D0, [D0])
    assert whole["score"] == 40


def test_window_scores_are_annot_models_scores_of_the_substring():
    """window_scores (all windows in one pass, row by row) against annot_model.scores of every window on its own (by anti-diagonals)"""
    rng = np.random.default_rng(11)
    recs = [_rand(rng, k) for k in (1, 2, 11, 37, 64, 65, 150)] + ["ACGTNACGTACGTAC", "A" * 40, "ACACACACACACACACACAC"]
    recs.append(recs[3])
    wins = [_rand(rng, m) for m in (1, 2, 3, 37, 64, 65, 90)] + ["", "ACGTNNACGTACGTACGT", recs[4][5:50], recs[6][20:70] + "T" + recs[6][70:100],
                                                                   recs[6][:30] + recs[6][36:80], "A" * 30, "ACACACACTTACACACACAC"]
    for p in (D.DEFAULT, dict(match=15, mismatch=31, gap_open=31, gap_extend=31), dict(match=1, mismatch=1, gap_open=0, gap_extend=1),
              dict(match=3, mismatch=0, gap_open=0, gap_extend=0), dict(match=5, mismatch=4, gap_open=1, gap_extend=3)):
        S = D.window_scores(wins, recs, p)
        for c, w in enumerate(wins):
            want = A.scores([w], recs, p)[0] if w else np.zeros(len(recs), np.int64)
            assert S[c].tolist() == want.tolist(), (p, c, w)
    assert D.window_scores([], recs).shape == (0, len(recs)) and D.window_scores(wins, []).shape == (len(wins), 0)


# ---- the window rule -------------------------------------------------------------------------------------------------------------------
def _hits(rows):
    """{field: array} of (gene, score, seq_start, seq_end) rows"""
    a = np.array(rows, np.int64)
    return dict(gene=a[:, 0], score=a[:, 1], seq_start=a[:, 2], seq_end=a[:, 3])


def test_d_window_cases():
    from vdjer_amd import annot
    #            normal             abutting           overlapping        257 between         256 between        no V call          no J call          J at score 0
    v = _hits([(3, 500, 1, 300), (3, 500, 1, 300), (3, 500, 1, 300), (3, 500, 1, 300), (3, 500, 1, 300), (-1, 12, 0, 0), (3, 500, 1, 300), (3, 500, 1, 300)])
    j = _hits([(9, 80, 321, 360), (9, 80, 301, 340), (9, 80, 295, 330), (9, 80, 558, 600), (9, 80, 557, 600), (9, 80, 321, 360), (-1, 7, 0, 0), (9, 0, 0, 0)])
    start, length = D.d_window(v, j)
    assert start.tolist() == [300, 0, 0, 0, 300, 0, 0, 0] and length.tolist() == [20, 0, 0, 0, 256, 0, 0, 0]
    assert D.over_window(v, j) == 1
    s2, l2 = annot.d_window(v, j)
    assert s2.dtype == np.int32 and l2.dtype == np.int32 and s2.tolist() == start.tolist() and l2.tolist() == length.tolist()
    assert annot.DCALL_WINDOW == D.WINDOW == 256
    e = _hits(np.zeros((0, 4)))
    assert [x.shape for x in annot.d_window(e, e)] == [(0,), (0,)]


# ---- the figures behind min_score 22 (include/vdjx.h quotes them) --------------------------------------------------------------------
def test_min_score_figures():
    rng = np.random.default_rng(7)
    recs = [_rand(rng, rng.integers(11, 38)) for _ in range(34)]
    reach = {}
    for m in (24, 45, 64):
        S = A.scores([_rand(rng, m) for _ in range(400)], recs, D.DEFAULT).max(axis=1)
        reach[m] = (float((S >= 20).mean()), float((S >= 22).mean()), int(S.max()))
    print("random windows (reach 20, reach 22, highest S):", reach)
    rng = np.random.default_rng([7, 1])                            # (a stream of its own: seed 7 again would draw the records' own bases)
    wins, src = [], []
    for _ in range(200):
        r = int(rng.integers(0, 34))
        k = min(int(rng.integers(11, 17)), len(recs[r]))
        o = int(rng.integers(0, len(recs[r]) - k + 1))
        at = int(rng.integers(0, 45 - k + 1))
        w = _rand(rng, 45)
        wins.append(w[:at] + recs[r][o:o + k] + w[at + k:])
        src.append(r)
    h, S = D.dcall(wins, [0] * 200, [45] * 200, recs)
    primary = sum(int(h["gene"][c]) == src[c] for c in range(200))
    print("planted cuts: lowest S", int(S.max(axis=1).min()), "primary for its record", primary, "of 200")
    assert reach[45][1] <= 0.02, reach
    for c in range(200):
        assert S[c, src[c]] >= 22 and h["gene"][c] >= 0 and src[c] in h["tied"][c][:min(8, h["n_tied"][c])].tolist(), (c, wins[c], recs[src[c]])


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def _table_case():
    rng = np.random.default_rng(23)
    V, J = _rand(rng, 60), _rand(rng, 30)
    names = ["IGHV1*01", "IGHJ1*01"]
    d_names, d_recs = ["IGHD1*01", "IGHD2*01", "IGHD1*02"], [D0, D1, D0]
    n1, n2 = "CCCAC", "CCAC"
    body = [V + n1 + D0[3:17] + n2 + J,                             # a D call, tied between IGHD1*01 and IGHD1*02
            V + "CCCACACCACCAC" + J,                                # no D call
            V + n1 + D0[3:17] + n2 + "CACACACACACCCACACACACACACACACC",       # no J hit
            V + J]                                                  # the hits abut
    m = max(len(b) for b in body) + 5
    seqs = [(b + "CA" * m)[:m] for b in body]
    ids = [f"vjf_{c}_x" for c in range(len(seqs))]
    hits = A.annotate(seqs, [V, J], ["V", "J"])
    ws, wl = D.d_window(hits["v"], hits["j"])
    d, _ = D.dcall(seqs, ws, wl, d_recs)
    return ids, seqs, hits, names, d, d_names, (ws, wl), (n1, n2)


def test_airr_rows_with_d_calls():
    ids, seqs, hits, names, d, d_names, (ws, wl), (n1, n2) = _table_case()
    assert ws.tolist() == [60, 60, 0, 0] and wl.tolist() == [23, 13, 0, 0]
    rows = D.airr_rows(ids, seqs, hits, names, d, d_names)
    col = {k: i for i, k in enumerate(D.AIRR_COLUMNS)}
    assert D.AIRR_COLUMNS[:30] == A.AIRR_COLUMNS and D.AIRR_COLUMNS[30:] == D.D_COLUMNS and all(len(r) == 40 for r in rows)
    base = A.airr_rows(ids, seqs, hits, names)
    for r, b in zip(rows, base):                                    # (every other cell is --airr's)
        assert [x for i, x in enumerate(r[:30]) if i not in (5, 16)] == [x for i, x in enumerate(b) if i not in (5, 16)]
    r = rows[0]
    assert r[col["d_call"]] == "IGHD1*01,IGHD1*02" and r[col["d_cigar"]] == f"65S3N14M{len(seqs[0]) - 79}S"
    assert r[30:] == ["28", "1.0000", "66", "79", "4", "17", n1, "5", n2, "4"]
    r = rows[1]
    assert r[col["d_call"]] == "" and r[col["d_cigar"]] == "" and r[30:36] == [""] * 6 and r[36:] == ["CCCACACCACCAC", "13", "", "0"]
    r = rows[2]
    assert r[col["j_call"]] == "" and r[col["d_call"]] == "" and r[30:] == [""] * 10
    r = rows[3]
    assert r[col["v_call"]] and r[col["j_call"]] and r[30:] == [""] * 6 + ["", "0", "", "0"]
    # expected_count stays last
    rows = D.airr_rows(ids, seqs, hits, names, d, d_names, counts=[1.5, 0.0, 2.25, 7.0])
    assert [r[-1] for r in rows] == ["1.50", "0.00", "2.25", "7.00"] and all(len(r) == 41 for r in rows) and rows[0][30:40] == ["28", "1.0000", "66", "79", "4", "17", n1, "5", n2, "4"]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_exports():
    from vdjer_amd import _lib
    assert ctypes.sizeof(_lib.DcallParams) == 20
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    assert re.search(r"\bint vdjx_dsegment_load\(vdjx_ctx\*", header) and re.search(r"\bint vdjx_dcall\(vdjx_ctx\*", header)
    assert "vdjx_dcall_params;   /* 20 bytes */" in header and re.search(r"#define VDJX_DCALL_WINDOW 256\b", header)
    for s in ("vdjx_dsegment_load", "vdjx_dcall"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)


# ---- the command line, up to where a GPU would be needed ----------------------------------------------------------------------------
def test_cli_d_calls_needs_airr(tmp_path):
    for extra in (["--d-calls"], ["--d-calls", "--quant", "q.tsv"], ["--quant", "q.tsv", "--d-calls"]):
        r = _run(tmp_path, extra)
        assert r.returncode != 0 and "--d-calls" in r.stderr and "--airr" in r.stderr and "ELAPSED_SECS" not in r.stderr, (extra, r.stderr[-500:])
        assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
        assert not (tmp_path / "q.tsv").exists()


def test_cli_usage_names_d_calls(tmp_path):
    r = subprocess.run([EXE, "--help", "x"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--d-calls" in r.stderr
