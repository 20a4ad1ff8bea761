"""CPU checks of the contig-annotation model (tests/annot_model.py, the restatement vdjx_annotate is tested against), of the germline
record parser of vdjer_amd/annot.py and of the ctypes mirror of vdjx_annot_hit."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import annot_limit_cases as L
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


# ---- trace_fast: the single-pair model by anti-diagonals, equal to traceback() on every field -----------------------------------------
PARAM_SETS = [A.DEFAULT, dict(match=1, mismatch=1, gap_open=0, gap_extend=1, min_v_score=10, min_j_score=5),
              dict(match=15, mismatch=31, gap_open=31, gap_extend=31, min_v_score=0, min_j_score=0),
              dict(match=3, mismatch=2, gap_open=2, gap_extend=1, min_v_score=40, min_j_score=20), dict(A.DEFAULT, gap_open=0)]


def _fast_equals_plain(a, b, p, what=None):
    x, y = A.traceback(a, b, p), A.trace_fast(a, b, p)
    assert x == y, (what, a, b, p, x, y)
    return x


@pytest.mark.parametrize("k", range(len(PARAM_SETS)))
def test_trace_fast_equals_traceback_random_pairs(k):
    """240 seeded pairs of 1 .. 120 bases per parameter set (the five of test_gpu_annot._api_checks; DEFAULT is two of them, so
    gap_open = 0 with DEFAULT's other costs stands in): unrelated pairs, a mutated copy of the other, N and lower-case bases"""
    p = PARAM_SETS[k]
    rng = np.random.default_rng(100 + k)
    zero = hit = 0
    for q in range(240):
        a = _rand(rng, int(rng.integers(1, 121)), "ACGTN" if q % 5 == 0 else "ACGT")
        if q % 3 == 0:
            b = _rand(rng, int(rng.integers(1, 121)))
        else:                                                                   # (a piece of a with substitutions and indels)
            lo = int(rng.integers(0, len(a)))
            b = list(a[lo:lo + int(rng.integers(1, 121))])
            for _ in range(int(rng.integers(0, 6))):
                at, op = int(rng.integers(0, len(b))), int(rng.integers(0, 3))
                if op == 0:
                    b[at] = "ACGT"[int(rng.integers(0, 4))]
                elif op == 1 and len(b) > 1:
                    del b[at]
                else:
                    b.insert(at, "ACGT"[int(rng.integers(0, 4))])
            b = "".join(b)[:120]
        if q % 7 == 0:
            a = a[:len(a) // 2] + a[len(a) // 2:].lower()                       # (a lower-case base matches nothing)
        if q % 11 == 0:
            b = b[:len(b) // 2] + "N" + b[len(b) // 2 + 1:]
        t = _fast_equals_plain(a, b, p, q)
        zero += t["score"] == 0
        hit += t["n_runs"] > 1
    assert hit > 20, hit


def test_trace_fast_equals_traceback_ties_and_zero():
    """S = 0; cells that two or three sources reach with the same value; several cells that hold S"""
    for p in PARAM_SETS:
        for a, b in (("AAAA", "CCCC"), ("NNNN", "NNNN"), ("acgt", "ACGT"), ("A", "C"), ("N", "A")):
            assert _fast_equals_plain(a, b, p)["score"] == 0
    # match = mismatch = extend = 1, open = 0: a gap of one costs what a mismatch costs, so diagonal, E and F tie all over
    flat = PARAM_SETS[1]
    rng = np.random.default_rng(77)
    for _ in range(60):
        a, b = _rand(rng, int(rng.integers(2, 40)), "AC"), _rand(rng, int(rng.integers(2, 40)), "AC")
        _fast_equals_plain(a, b, flat)
    # handmade: a cell whose diagonal, E and F all give H (1 - 1 = 2 - 2 ... ) -- count them in the plain matrices
    three = two = 0
    for _ in range(60):
        a, b = _rand(rng, 12, "AC"), _rand(rng, 12, "AC")
        H, E, F = A.matrices(a, b, flat)
        for i in range(1, 13):
            for j in range(1, 13):
                s = 1 if a[i - 1] == b[j - 1] else -1
                srcs = [H[i - 1][j - 1] + s, E[i][j], F[i][j]]
                if H[i][j] > 0:
                    n = sum(x == H[i][j] for x in srcs)
                    three += n == 3
                    two += n == 2
    assert three > 0 and two > 0, (three, two)
    # several cells hold S: a repeat in the contig, in the record, in both; the first in row-major order is the end
    g = "ACGTTGCAAGGC"
    for a, b in ((g + "TTTTT" + g, g), (g, g + "AAAAA" + g), (g + "T" * 20 + g, g + "A" * 20 + g), ("ACACACACAC", "ACACAC"), ("AAAAAAAA", "AAA")):
        for p in PARAM_SETS:
            t = _fast_equals_plain(a, b, p)
            H = A.matrices(a, b, p)[0]
            assert sum(x == t["score"] for r in H for x in r) > 1, (a, b)
    t = A.trace_fast(g + "TTTTT" + g, g)
    assert (t["seq_start"], t["seq_end"]) == (1, 12)


def test_trace_fast_more_than_64_runs():
    """the case of test_gpu_annot._api_checks: n_runs exact, the run list dropped by encode_runs, the same through annotate(fast=True)"""
    rng = np.random.default_rng(9)
    g = _rand(rng, 900)
    cont = "".join(g[q:q + 6] + ("" if (q // 6) % 2 else "T") for q in range(0, 900, 6))[:700]
    p = dict(A.DEFAULT, gap_open=0, gap_extend=1)
    t = _fast_equals_plain(cont, g, p)
    assert t["n_runs"] > 64 and not any(A.encode_runs(t["ops"]))
    slow, fast = A.annotate([cont, cont], [g, g[:50]], ["V", "J"], p), A.annotate([cont, cont], [g, g[:50]], ["V", "J"], p, fast=True)
    for cls in ("v", "j"):
        for f in A.FIELDS:
            assert np.array_equal(slow[cls][f], fast[cls][f]), (cls, f)
    assert fast["v"]["n_runs"][0] == t["n_runs"] and not fast["v"]["runs"].any()


def test_annotate_fast_equals_plain_on_a_random_case():
    from tests.test_gpu_annot import _random_case
    contigs, recs, germs, classes = _random_case(3, 64, n=5)
    slow, fast = A.annotate(contigs, germs, classes), A.annotate(contigs + contigs[:2], germs, classes, fast=True)
    for cls in ("v", "j"):
        for f in A.FIELDS:
            assert np.array_equal(slow[cls][f], fast[cls][f][:5]) and np.array_equal(fast[cls][f][5:], fast[cls][f][:2]), (cls, f)


# ---- the limit cases (tests/annot_limit_cases.py): each one's condition, from the inputs and the model alone ---------------------------
def _vlens(c):
    return [len(g) for g, cl in zip(c["germs"], c["classes"]) if cl == "V"]


def test_packing_rules_restated():
    assert L.chunk_sizes([2047] * 32) == [31, 1] and L.chunk_sizes([2047] * 5 + [2046] + [2047] * 26) == [32]
    assert L.chunk_sizes([65534]) == [1] and L.chunk_sizes([10, 20, 30], recs=2) == [2, 1] and L.chunk_sizes([]) == []
    assert L.chunk_sizes([2047] * 32, cols=65537) == [32]
    h = dict(v=dict(gene=[0] * 33, score=[5] * 33), j=dict(gene=[-1, 1], score=[9, 0]))
    assert L.trace_launch_sizes(h, 4095, ["A" * 2047, "A"]) == [32, 1]
    assert 32 * 4095 * 2047 == 268238880 <= L.DIR_BYTES == 268435456 < 33 * 4095 * 2047
    assert L.trace_launch_sizes(dict(v=dict(gene=[-1], score=[0]), j=dict(gene=[], score=[])), 10, ["A"]) == []


def test_limit_case_long_pair():
    c = L.long_pair()
    assert c["m"] == 4095 and len(c["contigs"]) == 6 and [len(c["germs"][k]) for k in (L.VA, L.VB)] == [2047, 2047]
    assert c["germs"][L.VA] != c["germs"][L.VB] and c["germs"][5] == c["germs"][2] and c["params"] == [A.DEFAULT, dict(A.DEFAULT, gap_open=0)]
    assert all(30 <= len(g) <= 60 for g, cl in zip(c["germs"], c["classes"]) if cl == "J")
    for k in range(2):
        h = L.model("long_pair", k)
        v, j = h["v"], h["j"]
        assert v["gene"].tolist() == [L.VA, L.VA, L.VB, L.VB, L.VA, L.VB], (k, v["gene"])
        assert (v["germ_end"] - v["germ_start"] >= 1400).all() and (v["n_runs"] <= 64).all() and (v["n_runs"] > 1).all(), (k, v["n_runs"])
        assert (v["ins"] > 0).any() and (v["del"] > 0).any()
        assert v["seq_end"][5] == 4095 and v["seq_start"][4] == 1 and (j["gene"] >= 0).all()
        assert (j["seq_start"][:5] > v["seq_end"][:5]).all() and j["seq_end"][5] < v["seq_start"][5]


def test_limit_case_ceiling():
    c = L.ceiling()
    assert c["params"][0] == dict(match=15, mismatch=31, gap_open=31, gap_extend=31, min_v_score=0, min_j_score=0)
    v = L.model("ceiling")["v"]
    s = v["score"].tolist()
    assert s[0] == 30705 == 15 * 2047 and v["matches"][0] == 2047 and v["n_runs"][0] == 1 and v["runs"][0][0] == 2047 << 4
    assert all(0 < 30705 - x <= 200 for x in s[1:]) and len(set(s)) == 4, s
    assert v["mismatches"][1] == 1 and v["del"][2] == 1 and v["germ_end"][3] == 2046 and (v["gene"] == 1).all()


def test_limit_case_column_chunks():
    a, b = L.column_chunks("A"), L.column_chunks("B")
    la, lb = _vlens(a), _vlens(b)
    assert la[:32] == [2047] * 32 and len(la) == 35 and lb[5] == 2046 and [x for k, x in enumerate(lb) if k != 5] == [x for k, x in enumerate(la) if k != 5]
    assert sum(x + 1 for x in la[:32]) + 1 == 65537 and sum(x + 1 for x in lb[:32]) + 1 == 65536
    assert L.chunk_sizes(la) == [31, 4] and L.n_chunks(a["germs"], a["classes"]) == 3
    assert L.chunk_sizes(lb) == [32, 3] and L.n_chunks(b["germs"], b["classes"]) == 3
    # the long records alone: the class is 65,537 and 65,536 columns, two chunks and one
    al, bl = L.column_chunks("A", False), L.column_chunks("B", False)
    assert L.chunk_sizes(_vlens(al)) == [31, 1] and L.n_chunks(al["germs"], al["classes"]) == 3
    assert L.chunk_sizes(_vlens(bl)) == [32] and L.n_chunks(bl["germs"], bl["classes"]) == 2
    # VDJX_ANNOT_PAIRS = 100: at most 25 records per chunk, and a launch that ends between two contig groups of a chunk
    assert L.chunk_sizes(la, recs=25) == [25, 10] and L.n_chunks(a["germs"], a["classes"], recs=25) == 3
    assert L.score_launches(9, a["germs"], a["classes"], 100) == 4
    assert len(a["contigs"]) == 9 and all(len(x) == 70 for x in a["contigs"])
    for which, cut in (("A", 31), ("B", 32)):
        v = L.model("column_chunks_" + which)["v"]
        assert v["n_tied"][0] == 11 and v["tied"][0].tolist() == L.TIED_IN[:8] and v["score"][0] == 140
        assert sum(r < cut for r in L.TIED_IN) in (7, 8) and sum(r >= cut for r in L.TIED_IN) >= 3
        assert v["n_tied"][1] == 2 and v["tied"][1].tolist()[:2] == L.TWICE_IN and L.TWICE_IN[0] < 25 and L.TWICE_IN[1] >= cut
        assert v["gene"][2] == L.AFTER_IN >= cut and v["gene"][3] == L.BEFORE_IN < 25 and v["n_tied"][2] == v["n_tied"][3] == 1
        assert v["n_tied"][4] == 11 and 0 < v["score"][4] < 140 and v["del"][5] == 1
    assert L.model("column_chunks_A_long")["v"]["n_tied"][0] == 8 and L.model("column_chunks_B_long")["v"]["n_tied"][1] == 1


def test_limit_case_trace_launches():
    c = L.trace_launches()
    assert len(c["contigs"]) == 34 and c["m"] == 4095 and len(set(c["contigs"])) == 7
    assert all(c["contigs"][q] == c["contigs"][q % 4] for q in range(31)) and len(set(c["contigs"][:4] + c["contigs"][31:])) == 7
    assert all(c["contigs"][q] != c["contigs"][q + 1] for q in range(33))
    h = L.model("trace_launches")
    v, j = h["v"], h["j"]
    assert set(v["gene"].tolist()) == {L.VA, L.VB} and (v["gene"][:-1] != v["gene"][1:]).all() and (j["gene"] >= 0).all() and (j["score"] > 0).all()
    sizes = L.trace_launch_sizes(h, 4095, c["germs"])
    assert len(sizes) >= 2 and sizes[0] == 32 and sum(sizes) == 68, sizes       # (V alignments 0 .. 31 | 32, 33 and the J's)
    # the parts taken from long_pair's model are what annotate gives for this case's own contigs
    own = A.annotate(c["contigs"][2:3], c["germs"], c["classes"], c["params"][0], fast=True)
    for cls in ("v", "j"):
        for f in A.FIELDS:
            assert np.array_equal(own[cls][f][0], h[cls][f][2]) and np.array_equal(h[cls][f][2], h[cls][f][30]), (cls, f)
