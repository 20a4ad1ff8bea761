"""The model of include/vdjx.h's vdjx_selection_convolve and vdjx_selection_compare on its own, without a GPU: the tree and the linear
binning of tests/selection_conv_model.py conserve mass and mean and do what the rule says on deltas; vdjx_selection_compare (plain host
code) through annot against cases worked by hand; the ABI mirror; every refusal of `vdjer --selection-combine` / `--selection-test`, each
of which comes before any GPU work; and the conditions under which the bounds of tests/test_gpu_selconv.py mean something."""
import ctypes
import os

import numpy as np
import pytest

from tests import selection_conv_cases as CC
from tests import selection_conv_model as CM
from tests.test_isotype_cpu import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = CM.T
SG = (np.arange(T) - 2000) / 100.0


def _leaves(m, dtype=np.float64):
    rng = np.random.default_rng(100 + m)
    ms = [(int(rng.integers(0, 8)), 0, int(rng.integers(2000, 9000)), int(rng.integers(1000, 4000))) for _ in range(m)]
    return [CM.leaf((x, x + int(rng.integers(1, 5)), er, es), dtype) for x, _, er, es in ms]


@pytest.mark.parametrize("m", [2, 3, 5, 7])
def test_tree_conserves_mass_and_mean(m):
    lv = _leaves(m)
    C, E, combines, depth = CM.tree(lv)
    assert combines == m - 1 and depth == (m - 1).bit_length() and E > 0
    assert abs(float(C.sum()) - 1.0) <= 1e-12 and float(C.min()) >= 0.0
    want = sum(float((SG * c).sum()) for c, _ in lv) / m
    assert abs(float((SG * C).sum()) - want) <= 1e-12, (float((SG * C).sum()), want)
    # the tree's two descriptions: the split at 2^(ceil(log2 m) - 1), and rounds of adjacent pairs with an odd last entry passed through
    assert np.array_equal(CM.pairs_tree(lv), C)
    assert [CM.split(k) for k in (2, 3, 4, 5, 7, 8, 9, 12)] == [1, 2, 2, 4, 4, 4, 8, 8]


def _delta(t):
    d = np.zeros(T)
    d[t] = 1.0
    return d


def test_deltas_follow_the_rule():
    # weights 2 : 1, u = +0.07 (index 2007), v = -0.03 (1997): num = 2 * 7 - 3 = 11, den = 3, q = 3, rem = 2: 1/3 to +0.03, 2/3 to +0.04
    C = CM.combine(_delta(2007), 2, _delta(1997), 1)
    assert np.flatnonzero(C).tolist() == [2003, 2004] and C[2003] == 1 / 3 and C[2004] == 2 / 3
    # negative numerators floor downwards: u = -0.07, v = +0.03: num = -11, q = -4, rem = 1: 2/3 to -0.04, 1/3 to -0.03
    C = CM.combine(_delta(1993), 2, _delta(2003), 1)
    assert np.flatnonzero(C).tolist() == [1996, 1997] and C[1996] == 2 / 3 and C[1997] == 1 / 3
    # rem = 0: one cell, and at u = v = +20.00 cell q + 1 = 4001 does not exist and is not touched
    for a, b in ((1, 1), (2, 1), (8, 1)):
        C = CM.combine(_delta(4000), a, _delta(4000), b)
        assert np.flatnonzero(C).tolist() == [4000] and C[4000] == 1.0
        C = CM.combine(_delta(0), a, _delta(0), b)
        assert np.flatnonzero(C).tolist() == [0] and C[0] == 1.0
    # equal weights, an odd numerator: half to either side
    C = CM.combine(_delta(2001), 1, _delta(2002), 1)
    assert np.flatnonzero(C).tolist() == [2001, 2002] and C[2001] == 0.5 and C[2002] == 0.5


# ---- vdjx_selection_compare (host code) ------------------------------------------------------------------------------------------------------
def test_compare_by_hand():
    from vdjer_amd import annot
    rng = np.random.default_rng(3)
    dens = np.zeros((6, T))
    dens[0] = rng.random(T)                                        # any positive scale
    dens[1] = 7.5 * dens[0]
    dens[2, 100:200] = 1.0                                         # disjoint supports: 2 below 3
    dens[3, 300:310] = 2.0
    dens[4, [10, 11, 12]] = [0.2, 0.5, 0.3]                        # the three-point case: a = 4, b = 5
    dens[5, [10, 11, 12]] = [0.6, 0.3, 0.1]
    r = annot.selection_compare(dens, [[0, 1], [3, 2], [2, 3], [4, 5]])
    assert abs(r["p_greater"][0] - 0.5) <= 1e-12 and abs(r["pvalue"][0] - 1.0) <= 2e-12
    assert abs(r["p_greater"][1] - 1.0) <= 1e-12 and r["p_greater"][1] <= 1.0 and r["p_greater"][2] == 0.0 and r["pvalue"][1] <= 2e-12 and r["pvalue"][2] == 0.0
    # P(a > b) = 0.5 * 0.6 + 0.3 * 0.9 = 0.57; P(equal) = 0.12 + 0.15 + 0.03 = 0.30: 0.57 + 0.15 = 0.72; pvalue 2 * 0.28
    assert abs(r["p_greater"][3] - 0.72) <= 1e-15 and abs(r["pvalue"][3] - 0.56) <= 1e-15
    for k, (a, b) in enumerate([(0, 1), (3, 2), (2, 3), (4, 5)]):
        pg, pv = CM.compare(dens[a], dens[b])
        assert abs(r["p_greater"][k] - pg) <= 1e-12 and abs(r["pvalue"][k] - pv) <= 1e-12
    with pytest.raises(ValueError, match="rows 6 and 0 of 6"):
        annot.selection_compare(dens, [[6, 0]])
    assert annot.selection_compare(dens, np.zeros((0, 2), np.uint32))["fdr"].shape == (0,)


def _two_point(pg):
    """a density pair with p_greater = pg exactly representable cases: a on point 1, b split between points 0 and 2"""
    a, b = np.zeros(T), np.zeros(T)
    a[1] = 1.0
    b[0], b[2] = pg, 1.0 - pg
    return a, b


def test_benjamini_hochberg_by_hand():
    from vdjer_amd import annot
    # p_greater 0.005, 0.02, 0.02, (skipped), 0.25 and 0.5 -> pvalues 0.01, 0.04, 0.04, 0.5, 1 over five rows that take part
    pgs = [0.02, 0.005, 0.5, 0.125, 0.02, 0.25]
    skip = [0, 0, 0, 1, 0, 0]
    dens = np.concatenate([np.stack(_two_point(p)) for p in pgs])
    r = annot.selection_compare(dens, [[2 * k, 2 * k + 1] for k in range(6)], skip)
    assert np.allclose(r["pvalue"], [0.04, 0.01, 1.0, 0.0, 0.04, 0.5], rtol=0, atol=1e-15)
    # sorted: 0.01 (row 1), 0.04 (row 0), 0.04 (row 4), 0.5 (row 5), 1 (row 2); p * 5 / rank: 0.05, 0.1, 0.0667, 0.625, 1; running minimum from
    # the top: 0.05, 0.0667, 0.0667, 0.625, 1 -- the tie takes the smaller value through the minimum, the skipped row stays 0
    want = [0.2 / 3, 0.05, 1.0, 0.0, 0.2 / 3, 0.625]
    assert np.allclose(r["fdr"], want, rtol=0, atol=1e-15), r["fdr"]
    assert r["p_greater"][3] == 0.0 and r["pvalue"][3] == 0.0
    got = CM.bh([0.04, 0.01, 1.0, 0.0, 0.04, 0.5], skip)
    assert got[3] is None and np.allclose([x for x in got if x is not None], [w for k, w in enumerate(want) if k != 3], rtol=0, atol=1e-15)


# ---- the ABI mirror ------------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_exports():
    from vdjer_amd import _lib, annot, api
    assert ctypes.sizeof(_lib.SelConvInfo) == 48 and ctypes.sizeof(_lib.SelTest) == 24
    assert [f for f, _ in _lib.SelConvInfo._fields_][:-1] == list(api.Context.SELCONV_INFO_FIELDS)
    for sym in ("vdjx_selection_convolve", "vdjx_selection_compare"):
        assert sym in _lib.SYMBOLS and hasattr(_lib.lib(), sym), sym
    assert callable(api.Context.selection_convolve) and callable(annot.selection_compare)
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    for word in ("typedef struct { uint64_t members, leaves, combines; uint32_t groups, regions, rows, levels, batches, pad; } vdjx_selconv_info;",
                 "typedef struct { double p_greater, pvalue, fdr; } vdjx_sel_test;", "VDJX_CONV_CELLS", "linear binning", "weighted_conv"):
        assert word in header, word
    source = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_selconv.hip")).read()
    assert 'vdjx_env_num("VDJX_CONV_CELLS", 1 << 15, 4, 1 << 20)' in source and "atomic" not in source.replace("no atomics", "")


# ---- the command line, up to where a GPU would be needed -----------------------------------------------------------------------------------
def _refused(r, tmp_path):
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr, r.stderr[-500:]
    assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
    assert not (tmp_path / "s.tsv").exists() and not (tmp_path / "t.tsv").exists()


def test_cli_refusals(tmp_path):
    (tmp_path / "r.tsv").write_text("V1 1 2 0 0\n")
    cases = [(["--selection", "s.tsv", "--selection-combine", "median"], "--selection-combine must be shared or mean: median"),
             (["--selection", "s.tsv", "--selection-combine", "Mean"], "--selection-combine must be shared or mean: Mean"),
             (["--selection-combine", "mean"], "--selection-combine is how the --selection table combines the members of a row: it needs --selection <file>"),
             (["--selection-combine", "shared"], "it needs --selection <file>"),
             (["--selection-test", "t.tsv", "--v-regions", "r.tsv"], "--selection-test compares the densities of the --selection table: it needs --selection <file>"),
             (["--selection", "s.tsv", "--selection-test", "t.tsv"], "--selection-test compares the cdr rows with the fwr rows: it needs --v-regions <file>"),
             (["--selection", "s.tsv", "--selection-combine", "mean", "--selection-test", "t.tsv"], "it needs --v-regions <file>")]
    for flags, message in cases:
        r = _run(tmp_path, flags)
        _refused(r, tmp_path)
        assert message in r.stderr, (flags, r.stderr[-600:])


# ---- the conditions of the GPU test's bounds -------------------------------------------------------------------------------------------------
_MODEL = {}


def model(name):
    """the np.longdouble model of a case of tests/selection_conv_cases.py, computed once per process (tests/test_gpu_selconv.py shares it)"""
    if name not in _MODEL:
        c = CC.CASES[name]()
        _MODEL[name] = (c, CM.rows(c["counts"], c["K"], c["group"], c["G"]))
    return _MODEL[name]


# E <= 1e-9 of the row's peak keeps the bound from growing vacuous.  One row cannot meet it, and not for want of a better choice of counts:
# in the group of nine every leaf of the block of eight has its bound doubled at three levels and multiplied by 9 / 8 at the fourth, so the
# near-delta leaf (n = 1,900, log-odds 0: tolerance 8 * 2^-52 * 38,040 = 6.8e-11 of ITS peak) alone gives 6.1e-10 of its own peak; the flat
# leaf (n = 1) it meets at 8 : 1 spreads the root over about 21 grid points where the near-delta leaf has 4.6, so the root's peak is about
# 4.6 times lower: 2.8e-9 of the root's peak at the least.  The case is the issue's and stays; its row is held to 3e-9.
PEAK_SHARE = {"a": 1e-9, "b": 1e-9, "ends": 1e-9, "delta": 3e-9}


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_gpu_case_conditions(name):
    c, ld = model(name)
    f64 = CM.rows(c["counts"], c["K"], c["group"], c["G"], np.float64)
    assert len(ld) == c["G"] + 1
    for r, (row_ld, row_64) in enumerate(zip(ld, f64)):
        for k in range(c["K"]):
            p, q = row_ld[k], row_64[k]
            peak = float(p["mass"].max())
            assert 0 < p["E"] <= PEAK_SHARE[name] * peak, (name, r, k, p["E"] / peak)
            assert CM.quantile_margin(p) > 2 * T * p["E"], (name, r, k, CM.quantile_margin(p), p["E"])
            dev = float(np.abs(q["mass"].astype(CM.LD) - p["mass"]).max())
            assert dev <= p["E"], (name, r, k, dev, p["E"])
            assert q["lower_t"] == p["lower_t"] and q["upper_t"] == p["upper_t"]
            assert abs(float(p["mass"].sum()) - 1.0) < 1e-15
    # the shapes the cases are there for
    seq = [[p["sequences"] for p in row] for row in ld]
    if name == "a":
        assert seq == [[0, 0], [1, 1], [2, 2], [3, 3], [5, 5], [12, 12]] and ld[5][0]["depth"] == 4 and CM.split(12) == 8
    if name == "b":
        assert seq == [[6], [7], [9], [22]]
    if name == "delta":
        assert seq == [[9], [9]] and ld[0][0]["combines"] == 8
    if name == "ends":
        assert seq == [[2], [2], [0], [4]] and int(np.argmax(ld[0][0]["mass"])) == 4000 and int(np.argmax(ld[1][0]["mass"])) == 0
        assert abs(float(ld[2][0]["sigma"])) < 1e-15 and abs(float(ld[2][0]["p_positive"]) - 0.5) < 1e-15
