"""CPU checks of the contig-annotation model (tests/annot_model.py, the restatement vdjx_annotate is tested against), of the germline
record parser of vdjer_amd/annot.py and of the ctypes mirror of vdjx_annot_hit."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import annot_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scalar(a, b, p=A.DEFAULT):
    """plain row-major Gotoh, the score only"""
    ma, mi, op, ext = p["match"], p["mismatch"], p["gap_open"], p["gap_extend"]
    g = len(b)
    Hp, Ep = [0] * (g + 1), [A.NEG] * (g + 1)
    Fp = [A.NEG] * (g + 1)
    best = 0
    for i in range(1, len(a) + 1):
        H, E, F = [0] * (g + 1), [A.NEG] * (g + 1), [A.NEG] * (g + 1)
        for j in range(1, g + 1):
            s = ma if a[i - 1] == b[j - 1] and a[i - 1] in "ACGT" else -mi
            E[j] = max(E[j - 1] - ext, H[j - 1] - op - ext)
            F[j] = max(Fp[j] - ext, Hp[j] - op - ext)
            H[j] = max(0, Hp[j - 1] + s, E[j], F[j])
            best = max(best, H[j])
        Hp, Ep, Fp = H, E, F
    return best


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(list(alpha), n))


@pytest.mark.parametrize("p", [A.DEFAULT, dict(match=1, mismatch=1, gap_open=0, gap_extend=1, min_v_score=5, min_j_score=5)])
def test_model_scores_match_scalar_gotoh(p):
    rng = np.random.default_rng(3)
    contigs = [_rand(rng, 23, "ACGTN") for _ in range(4)]
    germs = [_rand(rng, int(rng.integers(1, 30)), "ACGTN") for _ in range(9)]
    germs += [contigs[0][3:15], contigs[1][:10] + "A" + contigs[1][12:20]]        # (real local hits)
    S = A.scores(contigs, germs, p)
    for c in range(len(contigs)):
        for k in range(len(germs)):
            assert S[c, k] == _scalar(contigs[c], germs[k], p), (c, k)
    # the traceback's counts recompute the score
    for c in range(len(contigs)):
        for k in range(len(germs)):
            tb = A.traceback(contigs[c], germs[k], p)
            if S[c, k] == 0:
                assert tb["n_runs"] == 0
                continue
            assert p["match"] * tb["matches"] - p["mismatch"] * tb["mismatches"] - p["gap_open"] * tb["opens"] - \
                p["gap_extend"] * (tb["ins"] + tb["dele"]) == S[c, k]
            assert tb["seq_end"] - tb["seq_start"] + 1 == tb["matches"] + tb["mismatches"] + tb["ins"]
            assert tb["germ_end"] - tb["germ_start"] + 1 == tb["matches"] + tb["mismatches"] + tb["dele"]


def _one(contig, germ, p=A.DEFAULT):
    return A.traceback(contig, germ, p)


def test_hand_cases():
    g = "ACGTTGCAAGGCTTACCGATGCATGCAAGT"                      # 30 bases
    t = _one("TT" + g + "GG", g)
    assert (t["score"], t["seq_start"], t["seq_end"], t["germ_start"], t["germ_end"]) == (60, 3, 32, 1, 30)
    assert t["ops"] == [[30, "M"]] and t["mismatches"] == 0 and t["opens"] == 0
    mm = g[:15] + ("A" if g[15] != "A" else "C") + g[16:]
    t = _one(mm, g)
    assert t["score"] == 29 * 2 - 3 and t["mismatches"] == 1 and t["ops"] == [[30, "M"]]
    ins = g[:15] + "T" + g[15:]                               # one I
    t = _one(ins, g)
    assert t["score"] == 60 - 7 and t["ins"] == 1 and t["dele"] == 0 and t["opens"] == 1 and t["ops"] == [[15, "M"], [1, "I"], [15, "M"]]
    dele = g[:15] + g[16:]                                    # one D
    t = _one(dele, g)
    assert t["score"] == 58 - 7 and t["dele"] == 1 and t["ops"] == [[15, "M"], [1, "D"], [14, "M"]]
    # one gap of 4 (5 + 8 = 13) against two of 2 (2 x 9 = 18): the long gap wins
    gl = "ACGTTGCAAGGCTTACCGATGCATGCAAGTCCATGAGT"
    t = _one(gl[:15] + gl[19:], gl)
    assert t["dele"] == 4 and t["opens"] == 1 and t["score"] == 2 * (len(gl) - 4) - 13
    # N bases never match, not even each other
    assert _one("NNNN", "NNNN")["score"] == 0 and A.scores(["NNNN"], ["NNNN"])[0, 0] == 0
    assert _one("ACNT", "ACNT")["score"] == 4
    # the end cell is the first cell in row-major order holding S: two equal copies of the germline in the contig, the first is taken
    t = _one(g[:12] + "TTTTT" + g[:12], g[:12])
    assert (t["seq_start"], t["seq_end"]) == (1, 12)
    # ... and within a row the smallest j: a germline holding the contig twice
    t = _one(g[:12], g[:12] + "AAAAA" + g[:12])
    assert (t["germ_start"], t["germ_end"]) == (1, 12)


def test_calls_ties_and_threshold():
    rng = np.random.default_rng(11)
    v = _rand(rng, 40)
    j = _rand(rng, 20)
    contig = _rand(rng, 5) + v + _rand(rng, 10) + j + _rand(rng, 5)
    germs = [_rand(rng, 40), v, _rand(rng, 20), j, v, _rand(rng, 30), j[:12]]
    classes = ["V", "V", "J", "J", "V", "D", "J"]
    h = A.annotate([contig], germs, classes)
    assert h["v"]["gene"][0] == 1 and h["v"]["n_tied"][0] == 2 and h["v"]["tied"][0].tolist()[:3] == [1, 4, -1]
    assert h["v"]["score"][0] == 80 and h["v"]["seq_start"][0] == 6 and h["v"]["germ_start"][0] == 1
    assert h["j"]["gene"][0] == 3 and h["j"]["n_tied"][0] == 1 and h["j"]["score"][0] == 40
    # below the thresholds: no call, the score stays
    p = dict(A.DEFAULT, min_v_score=81, min_j_score=41)
    h = A.annotate([contig], germs, classes, p)
    assert h["v"]["gene"][0] == -1 and h["v"]["score"][0] == 80 and h["v"]["n_tied"][0] == 0 and h["v"]["seq_start"][0] == 0
    assert h["j"]["gene"][0] == -1 and h["j"]["score"][0] == 40
    # more than 8 ties: n_tied counts them all, tied lists the first 8
    h = A.annotate([contig], [v] * 11 + [j], ["V"] * 11 + ["J"])
    assert h["v"]["n_tied"][0] == 11 and h["v"]["tied"][0].tolist() == list(range(8))


def test_name_and_class_parsing():
    from vdjer_amd import annot as P
    cases = [("IGHV1-2*02", "IGHV1-2*02", "V"), ("V7", "V7", "V"), ("J2 some text", "J2", "J"),
             ("X12345|IGHV3-23*01|Homo sapiens|F|V-REGION|", "IGHV3-23*01", "V"), ("M99|IGKJ1*01|Homo", "IGKJ1*01", "J"),
             ("TRBD1*01", "TRBD1*01", "D"), ("IGHD2-2*01", "IGHD2-2*01", "D"), ("IGHM*01", "IGHM*01", "M"), ("D3", "D3", "D"),
             ("TRAV1-1*01", "TRAV1-1*01", "V"), ("IG", "IG", "I")]
    for head, name, cls in cases:
        for f in (P, A):
            assert f.parse_name(head) == name, (f, head)
            assert f.parse_class(name) == cls, (f, name)
    assert P.clean_seq("acg.t..N n\n") == A.clean("acg.t..N n\n") == "ACGTNN"
    assert P.parse_record("X|IGHV1*01|x", "ca.g")[1:] == ("V", "CAG")


def test_translation_and_productive():
    assert A.translate("TGTGCGAGATGG") == "CARW"
    assert A.translate("TAATAGTGA") == "***" and A.translate("ANG") == "X" and A.translate("TGTG") == "C"
    v = "ATGGCT" + "CCAGGA" * 16 + "TGT"                       # 102 bases: V (codon 1 at its first base), Cys at its end
    j = "TGGGGCCAAGGGACC"
    junc = "TGT" + "GCGAGA" + "TGG"
    contig = "GG" + v[:-3] + junc + j[3:] + "A"
    cid = "vjf_0_" + junc
    hits = A.annotate([contig], [v, j], ["V", "J"], dict(A.DEFAULT, min_j_score=10))
    row = A.airr_rows([cid], [contig], hits, ["V0", "J0"])[0]
    r = dict(zip(A.AIRR_COLUMNS, row))
    assert r["v_call"] == "V0" and r["j_call"] == "J0" and r["junction"] == junc and r["junction_aa"] == "CARW"
    assert r["cdr3"] == "GCGAGA" and r["cdr3_aa"] == "AR" and r["vj_in_frame"] == "T" and r["stop_codon"] == "F" and r["productive"] == "T"
    assert r["v_sequence_start"] == "3" and r["v_cigar"].startswith("2S") and r["rev_comp"] == "F" and r["d_call"] == ""
    assert r["v_identity"] == "1.0000"
    # out of frame: one base more in the junction region
    c2 = "GG" + v[:-3] + "TGTAGCGAGATGG" + j[3:] + "A"
    h2 = A.annotate([c2], [v, j], ["V", "J"], dict(A.DEFAULT, min_j_score=10))
    r2 = dict(zip(A.AIRR_COLUMNS, A.airr_rows(["vjf_1_TGTAGCGAGATGG"], [c2], h2, ["V0", "J0"])[0]))
    assert r2["vj_in_frame"] == "F" and r2["productive"] == "F"
    # a stop codon in frame between V start and J end
    c3 = "GG" + v[:-3] + "TGTTAGAGATGG" + j[3:] + "A"
    h3 = A.annotate([c3], [v, j], ["V", "J"], dict(A.DEFAULT, min_j_score=10))
    r3 = dict(zip(A.AIRR_COLUMNS, A.airr_rows(["vjf_2_TGTTAGAGATGG"], [c3], h3, ["V0", "J0"])[0]))
    assert r3["stop_codon"] == "T" and r3["productive"] == "F" and r3["junction_aa"] == "C*RW"
    # a junction that is not in the contig: empty fields, not productive
    r4 = dict(zip(A.AIRR_COLUMNS, A.airr_rows(["vjf_3_TTTTTTTTT"], [contig], hits, ["V0", "J0"])[0]))
    assert r4["junction"] == "" and r4["vj_in_frame"] == "F" and r4["productive"] == "F"
    assert A.junction_of("contig7", contig) == ("", -1)


def test_annot_struct_sizes_match_header():
    from vdjer_amd import _lib, api
    assert ctypes.sizeof(_lib.AnnotParams) == 24
    assert ctypes.sizeof(_lib.AnnotHit) == 340 == api.Context.ANNOT_HIT.itemsize
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    assert re.search(r"#define VDJX_ANNOT_TIED 8\b", header) and re.search(r"#define VDJX_ANNOT_RUNS 64\b", header)
    assert "/* 340 bytes */" in header
    for s in ("vdjx_germline_load", "vdjx_annotate"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)
