"""The selection model of include/vdjx.h (vdjx_selection) on its own, without a GPU: the posterior against its closed form, the prior
alone, the region sums against tests/mutation_model.py, the two file readers of vdjer_amd/annot.py on every malformed shape, the ABI
mirror, `vdjer --selection`'s refusals up to where a GPU would be needed, and the margin conditions of the GPU cases
(tests/selection_cases.py), so that a case that cannot be compared for equality shows here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import mutation_model as M
from tests import selection_cases as SC
from tests import selection_model as S
from tests import test_gpu_mutation as TM
from tests.test_isotype_cpu import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the posterior -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x,n", [(3, 10), (1, 2), (20, 50), (1, 40)])
def test_closed_form_with_even_odds(x, n):
    """odds 1 : 1, one member: the density of sigma is the Beta(x + 1, n - x + 1) density of pi = 1 / (1 + e^-sigma) times pi (1 - pi).
    (x >= 1 and n - x >= 1: the mass beyond +-20 is below e^-40.)  Measured here, float64 against the analytic density: 2.1e-15, 8.9e-16,
    5.5e-14 and 1.7e-14 of the peak for the four cases; the bound 1e-12 holds."""
    sg = S.grid()
    logpi, log1m = -S.softplus(-sg), -S.softplus(sg)
    want = np.exp((x + 1) * logpi + (n - x + 1) * log1m - (math.lgamma(x + 1) + math.lgamma(n - x + 1) - math.lgamma(n + 2)))
    for dtype in (np.float64, S.LD):
        got = S.posterior([(x, n, 1, 1)], dtype)
        dev = float(np.abs(got["pdf"].astype(np.float64) - want).max() / want.max())
        print(f"closed form x={x} n={n} {dtype.__name__}: {dev:.3g} of the peak")
        assert dev <= 1e-12
        assert abs(float(got["p_positive"]) - float(np.sum(want[2001:]) + want[2000] / 2) * 0.01) < 1e-12
    assert (got["sequences"], got["x"], got["n"], got["exp_r"], got["exp_s"]) == (1, x, n, 1, 1)


def test_prior_alone():
    p = S.posterior([])
    assert abs(float(p["sigma"])) < 1e-15 and abs(float(p["p_positive"]) - 0.5) < 1e-15 and p["sequences"] == 0
    # cdf_t holds the cell of t: about F(sigma_t + 0.005) of the logistic F.  F(-3.655) = 0.02520 >= 0.025 > F(-3.665) = 0.02496; F(3.665) = 0.97504 >= 0.975
    assert (p["lower"], p["upper"]) == (-3.66, 3.66)
    assert S.tolerance(p["A"]) == 8 * 2.0 ** -52 * 40


def test_a_wrong_formula_misses_by_far_more_than_the_tolerance():
    good = S.posterior([(3, 10, 5, 7), (0, 4, 9, 2)])
    bad = S.posterior([(3, 10, 7, 5), (0, 4, 9, 2)])
    assert float(np.abs(good["pdf"] - bad["pdf"]).max() / good["pdf"].max()) > 1e-3 > 1e6 * S.tolerance(good["A"])


# ---- the counts ----------------------------------------------------------------------------------------------------------------------------
def test_region_sums_are_the_mutation_counts():
    cs = SC.count_cases()
    ct, v = [c["contig"] for c in cs], SC.hits(cs)
    lim = [c["limit"] for c in cs]
    none = SC.hits(cs, "j")
    none["gene"][:] = -1
    _, want, _ = M.mutations(ct, v, None, none, lim, TM.germs(), [])
    for weighted in (False, True):
        for mapped in (False, True):
            got = SC.count_model(weighted, mapped)
            take = (np.asarray(got["flags"]) & S.F_V) > 0
            assert take.sum() > 40 and ((np.asarray(got["flags"]) & S.F_NOREG) > 0).sum() == (2 if mapped else 0)       # ("ends" and "whole_v5": the V record without regions)
            for f, g in (("obs_r", "v_r"), ("obs_s", "v_s"), ("codons", "v_codons")):
                assert np.array_equal(got[f].sum(axis=1)[take], want[g][take]), (weighted, mapped, f)
                assert not got[f][~take].any() and (mapped or not got[f][:, 1].any())
    # what the cases are there for
    at = {c["name"]: k for k, c in enumerate(cs)}
    plain, w, wm = SC.count_model(False, False), SC.count_model(True, False), SC.count_model(True, True)
    assert int(plain["codons"][at["end2047"], 0]) > 64 and max(int(x) for x in w["exp_r"][:, 0]) > 1 << 32
    k = at["whole_v5"]                                               # positions 1, 2, L - 1 and L have no 5-mer: 56 of 60 positions weigh
    assert int(plain["exp_r"][k, 0] + plain["exp_s"][k, 0]) > int(SC.count_model(False, False)["exp_r"][at["ends"], 0])
    assert int(plain["flags"][at["runs65_v"]]) == S.F_TRUNC and int(plain["flags"][at["cols1"]]) == S.F_V and int(plain["codons"][at["cols1"]].sum()) == 0
    k = at["v0_split"]
    assert wm["codons"][k].tolist() == [4, 2] and wm["obs_r"][k].sum() + wm["obs_s"][k].sum() > 0 and all(int(x) > 0 for x in wm["exp_r"][k])
    assert int(wm["flags"][at["whole_v5"]]) == S.F_NOREG and int(wm["codons"][at["whole_v1"], 0]) == 0 < int(wm["codons"][at["whole_v1"], 1])
    lim_k, full_k = at["v3_cdr_limit"], at["v3_cdr"]
    assert 0 < int(wm["codons"][lim_k].sum()) < int(wm["codons"][full_k].sum()) and int(wm["codons"][full_k, 1]) > 0
    # a uniform model weighs every position, a 5-mer model drops those next to the N and the record's ends
    u = SC.count_model(False, True)
    k = at["germ_N"]
    assert int(u["codons"][k].sum()) > 0


def test_the_5mer_context_by_hand():
    germs = ["GCAGCAGCAGCA"]                                         # Ala x 4: every third-base change is silent, every other a replacement
    v = SC.hits([dict(v=TM.H(0, 1, 1, [("M", 12)]))])
    w = np.zeros((1024, 4), np.uint32)
    idx = lambda five: int("".join(str("ACGT".index(ch)) for ch in five), 4)
    w[idx("GCAGC")] = (0, 7, 11, 13)                                 # centre A (a third base): silent, 7 + 11 + 13
    w[idx("CAGCA")] = (100, 200, 0, 400)                             # centre G (a first base): replacement, 100 + 200 + 400
    w[idx("AGCAG")] = (1000, 0, 2000, 4000)                          # centre C (a second base): replacement
    got = S.counts(["GCAGCAGCAGCA"], v, None, germs, None, w)
    # positions 3 .. 10 (1-based) have a 5-mer: A at 3, 6, 9; G at 4, 7, 10; C at 5, 8
    assert int(got["exp_s"][0, 0]) == 3 * 31 and int(got["exp_r"][0, 0]) == 3 * 700 + 2 * 7000 and got["codons"][0].tolist() == [4, 0]
    uni = S.counts(["GCAGCAGCAGCA"], v, None, germs, None, None)
    assert int(uni["exp_s"][0, 0]) == 4 * 3 and int(uni["exp_r"][0, 0]) == 8 * 3
    m = S.members(uni, 1)
    assert m == [[None]]                                             # no mutation: n = 0, the contig adds nothing


# ---- the margin conditions of the GPU cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_group", [False, True])
def test_margins_of_the_gpu_posterior_cases(one_group):
    """the quantiles are compared for equality on the GPU: in every row the model's CDF at the deciding index and the one before it lies
    further than 4001 x tolerance from 0.025 / 0.975; and the cases hold what they are there for"""
    rows = SC.posterior_model(one_group)
    cs, group = SC.posterior_cases()
    for r, row in enumerate(rows):
        for k, p in enumerate(row):
            assert S.quantile_margin(p) > S.T * S.tolerance(p["A"]), (r, k, S.quantile_margin(p), S.tolerance(p["A"]))
    if one_group:
        assert len(rows) == 26 + 2 and rows[26][0]["sequences"] == rows[27][0]["sequences"] > 20
        return
    cnt = SC.posterior_counts()
    at = {c["name"]: k for k, c in enumerate(cs)}
    assert len(rows) == 26 + SC.PGROUPS + 1
    assert [int((group == g).sum()) for g in range(SC.PGROUPS)] == [0, 1, 3, 4, 5, 9, 0] and int((group < 0).sum()) == 4
    assert rows[at["most"]][0]["n"] > 1000 and rows[at["none"]][0]["sequences"] == 0
    assert rows[at["silent"]][0]["x"] == 0 < rows[at["silent"]][0]["n"] and rows[at["replaced"]][0]["x"] == rows[at["replaced"]][0]["n"] == 7
    e = rows[at["edge"]][1]
    assert (e["x"], e["exp_r"]) == (2, 1) and e["exp_s"] > 1 << 36 and int(np.argmax(e["pdf"])) == S.T - 1 and e["upper"] > 19.9
    k = at["v0_outside"]
    assert int(cnt["exp_r"][k, 1]) == 0 and rows[k][1]["sequences"] == 0 and rows[k][0]["sequences"] == 1
    assert rows[26][0]["sequences"] == 0 and rows[26 + 6][1]["sequences"] == 0        # the empty groups: the prior alone
    assert rows[-1][0]["sequences"] >= 20


# ---- the readers ---------------------------------------------------------------------------------------------------------------------------
def _targeting_lines(w=None):
    out = []
    for idx in range(1024):
        five = "".join("ACGT"[idx >> s & 3] for s in (8, 6, 4, 2, 0))
        out.append(five + "\t" + "\t".join(str(int(x)) for x in (w[idx] if w is not None else (idx, 1, 2, 3))))
    return out


def test_read_targeting(tmp_path):
    from vdjer_amd import annot
    w = SC.weights()
    p = tmp_path / "t.tsv"
    p.write_text("# HH_S5F x 10^6\n\n" + "\n".join(reversed(_targeting_lines(w))) + "\n")
    got = annot.read_targeting(str(p))
    assert got.dtype == np.uint32 and np.array_equal(got, w) and int(w.max()) == 0xFFFFFFFF
    good = _targeting_lines()
    for what, lines in (("1023 lines", good[:-1]), ("twice", good + [good[5]]), ("four fields", good[:7] + ["AAACT 1 2 3"] + good[8:]),
                        ("six fields", good[:7] + ["AAACT 1 2 3 4 5"] + good[8:]), ("a 4-mer", good[:7] + ["AACT 1 2 3 4"] + good[8:]),
                        ("an N", good[:7] + ["AANCT 1 2 3 4"] + good[8:]), ("lower case", good[:7] + ["aaact 1 2 3 4"] + good[8:]),
                        ("2^32", good[:7] + ["AAACT 1 2 3 4294967296"] + good[8:]), ("a sign", good[:7] + ["AAACT 1 2 -3 4"] + good[8:]),
                        ("a fraction", good[:7] + ["AAACT 1 2 3.5 4"] + good[8:]), ("empty file", [])):
        p.write_text("\n".join(lines) + "\n")
        with pytest.raises(ValueError, match="line 8|line 1025|5-mers"):
            annot.read_targeting(str(p))
    with pytest.raises(OSError):
        annot.read_targeting(str(tmp_path / "none.tsv"))


def test_read_v_regions(tmp_path):
    from vdjer_amd import annot
    names = ["IGHV1-1*01", "IGHD1-1*01", "IGHV2-2*01", "IGHV1-1*01", "IGHJ1*01"]
    p = tmp_path / "r.tsv"
    p.write_text("# name cdr1 cdr2\nIGHV1-1*01\t76\t99\t151\t174\n\nIGHV9-9*01 1 2 0 0\nIGHJ1*01  0 0   0 0\n")
    miss = []
    got = annot.read_v_regions(str(p), names, miss)
    assert got.dtype == np.int32 and got.tolist() == [[76, 99, 151, 174], [-1] * 4, [-1] * 4, [76, 99, 151, 174], [0] * 4] and miss == ["IGHV9-9*01"]
    for bad in ("IGHV1-1*01 1 2 3", "IGHV1-1*01 1 2 3 4 5", "IGHV1-1*01 5 4 0 0", "IGHV1-1*01 0 4 0 0", "IGHV1-1*01 1 2 3 x", "IGHV1-1*01 1 2 -3 4",
                "IGHV1-1*01 1 2 3 2147483648", "IGHV1-1*01 1 2 3 4\nIGHV1-1*01 1 2 3 4".replace("\n", "\n", 1)):
        p.write_text("# x\n" + ("\n" if "\n" not in bad else "") + bad + "\n")
        with pytest.raises(ValueError, match="line 3"):
            annot.read_v_regions(str(p), names)
    with pytest.raises(OSError):
        annot.read_v_regions(str(tmp_path / "none.tsv"), names)
    assert annot.selection_grid().shape == (S.T,) and np.array_equal(annot.selection_grid(), S.grid())


# ---- the ABI mirror ------------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_exports():
    from vdjer_amd import _lib, api
    assert ctypes.sizeof(_lib.SelInfo) == 48 and api.Context.SEL_COUNTS.itemsize == 64 and api.Context.SEL_STAT.itemsize == 72
    assert [f for f, _ in _lib.SelInfo._fields_] == list(api.Context.SEL_INFO_FIELDS)
    assert "vdjx_selection" in _lib.SYMBOLS and hasattr(_lib.lib(), "vdjx_selection") and callable(api.Context.selection)
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    assert re.search(r"#define VDJX_SEL_GRID %d\b" % S.T, header)
    for word in ("BAYESIAN_FITTED", "convolution", "IMGT numbering", "N-averaged", "representative per clone", "J segment", "two groups"):
        assert word in header, word
    source = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_select.hip")).read()
    assert re.search(r'vdjx_env_num\("VDJX_SEL_CHUNK", 1024, 1, 65536\)', source)


# ---- the command line, up to where a GPU would be needed -----------------------------------------------------------------------------------
def _refused(r, tmp_path):
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr, r.stderr[-500:]
    assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
    assert not (tmp_path / "s.tsv").exists()


def test_cli_options_need_selection(tmp_path):
    (tmp_path / "x.tsv").write_text("junk junk\n")                    # (not read: the flag is refused first)
    for flag, what in (("--v-regions", "region map"), ("--targeting", "targeting model")):
        r = _run(tmp_path, [flag, "x.tsv"])
        _refused(r, tmp_path)
        assert flag in r.stderr and what in r.stderr and "it needs --selection <file>" in r.stderr and "line 1" not in r.stderr, r.stderr[-500:]


def test_cli_refuses_unreadable_and_malformed_files(tmp_path):
    good = _targeting_lines()
    cases = [("--targeting", "none.tsv", None, "--targeting: cannot read none.tsv"),
             ("--v-regions", "none.tsv", None, "--v-regions: cannot read none.tsv"),
             ("--targeting", "t.tsv", good[:-1], "holds 1023 5-mers"),
             ("--targeting", "t.tsv", good[:3] + ["AAAAT 1 2 3"] + good[4:], "t.tsv line 4: expected"),
             ("--targeting", "t.tsv", good[:3] + ["AAAAT 1 2 3 4294967296"] + good[4:], "t.tsv line 4: expected"),
             ("--targeting", "t.tsv", good[:3] + ["AAANT 1 2 3 4"] + good[4:], "t.tsv line 4: expected"),
             ("--targeting", "t.tsv", good + [good[9]], "t.tsv line 1025: the 5-mer AAAGC is given twice"),
             ("--v-regions", "r.tsv", ["# x", "V1 1 2 3"], "r.tsv line 2: expected"),
             ("--v-regions", "r.tsv", ["V1 1 2 3 -4"], "r.tsv line 1: expected"),
             ("--v-regions", "r.tsv", ["V1 9 2 0 0"], "r.tsv line 1: the interval 9 .. 2"),
             ("--v-regions", "r.tsv", ["V1 0 2 0 0"], "r.tsv line 1: the interval 0 .. 2"),
             ("--v-regions", "r.tsv", ["V1 1 2 0 0", "", "V1 1 2 0 0"], "r.tsv line 3: the name V1 is given twice")]
    for flag, name, lines, message in cases:
        if lines is not None:
            (tmp_path / name).write_text("\n".join(lines) + "\n")
        r = _run(tmp_path, ["--selection", "s.tsv", flag, name])
        _refused(r, tmp_path)
        assert message in r.stderr, (flag, message, r.stderr[-600:])


def test_cli_usage_names_the_flags(tmp_path):
    r = _run(tmp_path, ["--v-regions", "x"])
    for flag in ("--selection <file", "--v-regions <file", "--targeting <file"):
        assert flag in r.stderr, flag
