"""CPU checks of the isotype model (tests/isotype_model.py, the restatement vdjx_isotype and `vdjer --isotypes` / `--clones` are tested
against), of the name rules of vdjer_amd/annot.py, of the ctypes mirror, and of what the command line decides before any GPU work."""
import ctypes
import os
import re
import subprocess

import numpy as np

from tests import annot_model as A
from tests import isotype_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vdjer_amd", "vdjer")


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(list(alpha), int(n)))


def _other(ch):
    return "A" if ch != "A" else "C"


def test_hand_checked_calls():
    rng = np.random.default_rng(5)
    consts = [_rand(rng, 300), _rand(rng, 500), _rand(rng, 200)]
    m, T, r, o = 120, 48, 1, 137
    body = _rand(rng, m - T)
    # a tail copied from record r at offset o: 2T, exact coordinates
    h, S = M.isotype([body + consts[r][o:o + T]], consts)
    assert S.shape == (1, 3) and S[0, r] == 2 * T and h["gene"][0] == r and h["score"][0] == 2 * T and h["n_tied"][0] == 1
    assert (h["seq_start"][0], h["seq_end"][0], h["germ_start"][0], h["germ_end"][0]) == (m - T + 1, m, o + 1, o + T)
    assert h["matches"][0] == T and h["n_runs"][0] == 1 and h["runs"][0][0] == (T << 4)
    assert h["tied"][0].tolist() == [r] + [-1] * 7
    # one interior substitution: 2(T - 1) - 3
    tail = consts[r][o:o + T]
    tail = tail[:20] + _other(tail[20]) + tail[21:]
    h, S = M.isotype([body + tail], consts)
    assert h["score"][0] == 2 * (T - 1) - 3 and h["mismatches"][0] == 1 and h["matches"][0] == T - 1 and h["gene"][0] == r
    # a duplicated record: n_tied 2; more than 8 ties: all counted, the first 8 listed
    h, S = M.isotype([body + consts[r][o:o + T]], consts + [consts[r]])
    assert h["n_tied"][0] == 2 and h["tied"][0].tolist()[:3] == [1, 3, -1] and h["gene"][0] == 1
    h, S = M.isotype([body + consts[r][o:o + T]], [consts[0]] + [consts[r]] * 11)
    assert h["n_tied"][0] == 11 and h["tied"][0].tolist() == list(range(1, 9)) and S[0].tolist() == [S[0, 0]] + [96] * 11
    # below min_score: no call, the score stays
    h, S = M.isotype([body + consts[r][o:o + T]], consts, dict(M.DEFAULT, min_score=97))
    assert h["gene"][0] == -1 and h["score"][0] == 96 and h["n_tied"][0] == 0 and h["seq_start"][0] == 0 and h["tied"][0].tolist() == [-1] * 8
    # only the tail is looked at: a copy of record 0 upstream of it does not count
    h, S = M.isotype([consts[0][:m - T] + consts[r][o:o + T]], consts)
    assert h["gene"][0] == r and S[0, 0] < 48
    # len < tail: the whole contig is the tail; C = 0: no call, score 0
    short = consts[2][50:80]
    h, S = M.isotype([short], consts, dict(M.DEFAULT, min_score=30))
    assert h["score"][0] == 60 and (h["seq_start"][0], h["seq_end"][0], h["germ_start"][0]) == (1, 30, 51)
    h, S = M.isotype([short], [])
    assert S.shape == (1, 0) and h["gene"][0] == -1 and h["score"][0] == 0 and h["n_tied"][0] == 0
    h, S = M.isotype([], consts)
    assert S.shape == (0, 3) and h["gene"].shape == (0,)
    # the score matrix is the scalar Gotoh score of the tail
    contigs = [_rand(rng, 70, "ACGTN") for _ in range(3)]
    h, S = M.isotype(contigs, consts[:2], dict(M.DEFAULT, tail=20))
    for c in range(3):
        for k in range(2):
            assert S[c, k] == max(max(row) for row in A.matrices(contigs[c][-20:], consts[k], M.DEFAULT)[0])


def test_min_score_48_separates_noise_from_tails():
    """the figures the default rests on: random 48-mers against 9 random records of 1,000 bases stay below 48; a true tail with three
    substitutions is far above it"""
    rng = np.random.default_rng(48)
    consts = [_rand(rng, 1000) for _ in range(9)]
    S = A.scores([_rand(rng, 48) for _ in range(60)], consts, M.DEFAULT)
    assert S.max() < 48
    t = list(consts[4][500:548])
    for q in (5, 20, 40):
        t[q] = _other(t[q])
    assert A.scores(["".join(t)], consts, M.DEFAULT)[0, 4] == 2 * 45 - 3 * 3 == 81


def test_name_rules():
    from vdjer_amd import annot as P
    for f in (P, M):
        assert f.gene_of("IGHG1*01") == "IGHG1" and f.gene_of("IGHM") == "IGHM"
        assert f.subtypes(["IGHG1*01", "IGHG2*02", "IGHA1*01"]) == "IGHG,IGHA"
        assert f.subtypes(["IGHM*01"]) == "IGHM" and f.subtypes([]) == "" and f.subtypes(["IGHA2*01", "IGHG4*01", "IGHA1*01"]) == "IGHA,IGHG"
        assert f.vq_gene(["IGHV3-30-5*01"]) == "IGHV3-30"
        assert f.vq_gene(["IGHV1-69D*01", "IGHV1-69*01"]) == "IGHV1-69"
        assert f.vq_gene(["IGKV1D-39*01"]) == "IGKV1-39"
        assert f.vq_gene(["IGHV4-34*01", "IGHV1-2*02"]) == "IGHV4-34,IGHV1-2"
        assert f.vq_gene(["V7"]) == "V7" and f.vq_gene(["IGHJ4*02"]) == "IGHJ4" and f.vq_gene([]) == ""
    rng = np.random.default_rng(2)
    parts = ["IGHV", "IGKV", "D", "-", "-", "1", "30", "69", "*01", "*", "G"]
    for _ in range(300):
        names = ["".join(rng.choice(parts, int(rng.integers(1, 6)))) for _ in range(int(rng.integers(0, 5)))]
        assert P.vq_gene(names) == M.vq_gene(names) and P.subtypes(names) == M.subtypes(names), names


def _clone_case():
    v = "ATGGCT" + "CCAGGA" * 16 + "TGT"
    j = "TGGGGCCAAGGGACC"
    junc = "TGT" + "GCGAGA" + "TGG"
    rng = np.random.default_rng(8)
    consts = [_rand(rng, 200), _rand(rng, 200)]
    consts.append(consts[1][:150] + _other(consts[1][150]) + consts[1][151:])
    cnames = ["IGHM*01", "IGHG1*01", "IGHG2*01"]
    base = "GG" + v[:-3] + junc + j[3:]
    contigs = [base + consts[0][10:70], base + consts[1][20:80], base + consts[1][20:80], base + _rand(rng, 60), base + consts[0][10:70],
               base + consts[1][120:180]]
    ids = [f"vjf_{k}_{junc}" for k in range(5)] + ["vjf_5_TTTTTTTTTTTT"]
    p = dict(A.DEFAULT, min_j_score=10)
    vj = A.annotate(contigs, [v, j], ["V", "J"], p)
    iso, S = M.isotype(contigs, consts)
    return ids, contigs, vj, iso, cnames, junc


def test_clone_rows():
    ids, contigs, vj, iso, cnames, junc = _clone_case()
    gn = ["IGHV3-30-5*01", "IGHJ4*02"]
    counts = [3.0, 0.996, 0.994, 7.25, 2.0, 9.0]
    rows = M.clone_rows("s1", ids, contigs, counts, vj, gn, iso, cnames, total_count=1234)
    # 0.996 prints as 1.00 and is in; 0.994 prints as 0.99 and is out; contig 5's junction is not in it: no row
    assert [r[4] for r in rows] == ids[:2] + ids[3:5]
    assert [r[3] for r in rows] == ["3.00", "1.00", "7.25", "2.00"]
    r0 = dict(zip(M.CLONE_COLUMNS, rows[0]))
    assert r0 == dict(sample="s1", sequence=contigs[0], cdr3=junc, expected_counts="3.00", seq_id=ids[0], isotype="IGHM",
                      vregion_identity="100.00", aa_cdr3="CARW", vgene="IGHV3-30", jgene="IGHJ4", total_count="1234", cluster="cls_1")
    # IGHG1 and IGHG2 tie on contig 1 (the copy lies before the point mutation): one subtype; contig 3 has a random tail: N/A
    assert iso["n_tied"][1] == 2 and rows[1][5] == "IGHG" and rows[2][5] == "N/A"
    # clusters count from 1 in order of first appearance; contig 4 joins contig 0's
    assert [r[11] for r in rows] == ["cls_1", "cls_2", "cls_3", "cls_1"]
    # past the mutation only IGHG1 holds the best score, by one mismatch
    assert iso["n_tied"][5] == 1 and iso["gene"][5] == 1
    # no --cfa: every isotype N/A, total_count N/A; no J call: jgene N/A
    rows = M.clone_rows("s1", ids, contigs, counts, vj, gn)
    assert {r[5] for r in rows} == {"N/A"} and {r[10] for r in rows} == {"N/A"} and [r[11] for r in rows] == ["cls_1"] * 4
    vj["j"]["gene"][0] = -1
    assert M.clone_rows("s1", ids, contigs, counts, vj, gn)[0][9] == "N/A"
    # no V call: no row
    vj["v"]["gene"][0] = -1
    assert [r[4] for r in M.clone_rows("s1", ids, contigs, counts, vj, gn)] == [ids[1]] + ids[3:5]
    assert M.clone_rows("s1", [], [], [], A.annotate([], [], []), []) == []


def test_isotype_rows():
    ids, contigs, vj, iso, cnames, junc = _clone_case()
    rows = M.isotype_rows(ids, contigs, iso, cnames)
    m = len(contigs[0])
    assert rows[0] == [ids[0], "IGHM", "IGHM*01", "96", "1.0000", str(m - 47), str(m), "23", "70", f"{m - 48}S22N48M"]
    assert rows[1][1:3] == ["IGHG", "IGHG1*01,IGHG2*01"]
    assert rows[3][1:] == [""] * 9                                    # (no call: every cell empty, as --airr leaves a hit's cells)
    assert all(len(r) == len(M.ISOTYPE_COLUMNS) for r in rows)


def test_abi_mirror_and_exports():
    from vdjer_amd import _lib
    assert ctypes.sizeof(_lib.IsotypeParams) == 24
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    assert re.search(r"\bint vdjx_constant_load\(vdjx_ctx\*", header) and re.search(r"\bint vdjx_isotype\(vdjx_ctx\*", header)
    assert "vdjx_isotype_params;   /* 24 bytes */" in header
    for s in ("vdjx_constant_load", "vdjx_isotype"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)


# ---- the command line, up to where a GPU would be needed ----------------------------------------------------------------------------
def _cli_inputs(d):
    open(os.path.join(d, "reads.txt"), "w").write("P r1 1 0 ACGTACGTAC IIIIIIIIII\nP r1 2 1 ACGTACGTAC IIIIIIIIII\n")
    os.makedirs(os.path.join(d, "ref"), exist_ok=True)
    for fn in ("v_index", "j_index"):
        open(os.path.join(d, "ref", fn), "w").write("1\t0\n")
    open(os.path.join(d, "ref", "v_region.fa"), "w").write(">v\nACGT\n")
    open(os.path.join(d, "c.fa"), "w").write(">IGHM*01\nACGTACGTACGTACGTACGT\n")


def _run(tmp_path, extra, **env):
    assert os.path.exists(EXE), "build it: make -C vdjer_amd/csrc/host"
    _cli_inputs(str(tmp_path))
    return subprocess.run([EXE, "--in", "reads.txt", "--chain", "IGH", "--ref-dir", "ref", "--ins", "175"] + extra, cwd=tmp_path,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=dict(os.environ, **env))


def test_cli_isotypes_needs_cfa(tmp_path):
    r = _run(tmp_path, ["--isotypes", "i.tsv"])
    assert r.returncode != 0 and "--cfa" in r.stderr and "ELAPSED_SECS" not in r.stderr
    assert not (tmp_path / "i.tsv").exists()


def test_cli_clones_refuses_sharded_runs_before_any_gpu_work(tmp_path):
    r = _run(tmp_path, ["--clones", "c.tsv", "--cfa", "c.fa"], VDJX_FORCE_MGPU="1")
    assert r.returncode != 0 and "--clones runs on one GPU only" in r.stderr and "ELAPSED_SECS" not in r.stderr
    assert not (tmp_path / "c.tsv").exists()
    r = _run(tmp_path, ["--clones", "c.tsv", "--gpus", "2"])
    assert r.returncode != 0 and "--clones" in r.stderr and "ELAPSED_SECS" not in r.stderr and not (tmp_path / "c.tsv").exists()


def test_cli_total_count_must_be_a_whole_number(tmp_path):
    for bad in ("12x", "-3", "1.5", ""):
        r = _run(tmp_path, ["--clones", "c.tsv", "--total-count", bad], VDJX_FORCE_MGPU="1")
        assert r.returncode != 0 and "--total-count" in r.stderr and "--clones runs on one GPU only" not in r.stderr, bad
        assert not (tmp_path / "c.tsv").exists()


def test_cli_unreadable_cfa_is_an_error(tmp_path):
    r = _run(tmp_path, ["--isotypes", "i.tsv", "--cfa", "missing.fa"])
    assert r.returncode != 0 and "missing.fa" in r.stderr and "ELAPSED_SECS" not in r.stderr and not (tmp_path / "i.tsv").exists()


def test_cli_usage_names_the_flags(tmp_path):
    r = subprocess.run([EXE, "--help", "x"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    for flag in ("--cfa", "--isotypes", "--clones", "--total-count", "--sample"):
        assert flag in r.stderr, flag
