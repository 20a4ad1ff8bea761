"""The diversity model of include/vdjx.h (vdjx_diversity): the draw rule against its check values and against vdjer_amd/annot.py's
diversity_draw, the counts, Hill numbers that are known, the weights of `vdjer --diversity` on handmade cells, the table writer, the ABI
mirror and the command line up to where a GPU would be needed.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import diversity_model as M
from tests.test_isotype_cpu import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_CASES = [((1, 3), 100000, 1, 1), ((0, 5, 0, 0, 7, 0), 1000, 1, 1), ((1, 1, 1), 12, 1, 1), ((1, 1 << 45), 500, 0, 2), ((9,), 77, M.M64, 4096),
               (tuple(range(300)), 5003, 7, 3)]


# ---- the draw rule ---------------------------------------------------------------------------------------------------------------------
def test_draw_check_values():
    assert M.mix64(0) == 0xE220A8397B1DCDAF == M.CHECK
    assert [M.draw(1, 1, i, 3) for i in range(12)] == [0, 2, 0, 2, 1, 1, 1, 2, 2, 2, 1, 0]
    assert M.draw(0, 1, 0, 1 << 62) == 2241935815489788276
    assert M.draw(M.M64, 4096, (1 << 31) - 2, (1 << 63) - 1) == 4159382355531584464


def test_counts_check_values():
    assert M.counts((1, 3), 100000, 1, 1).tolist() == [24932, 75068]
    assert M.counts((0, 5, 0, 0, 7, 0), 1000, 1, 1).tolist() == [0, 405, 0, 0, 595, 0]


def test_diversity_draw_is_the_models_rule():
    from vdjer_amd import annot
    for seed, r, i, W in ((1, 1, 0, 3), (0, 1, 0, 1 << 62), (M.M64, 4096, (1 << 31) - 2, (1 << 63) - 1), (7, 200, 99999, 1234567), (5, 3, 17, 1)):
        assert annot.diversity_draw(seed, r, i, W) == M.draw(seed, r, i, W), (seed, r, i, W)
    assert annot.diversity_orders() == M.orders() and len(M.orders()) == 41 and M.orders()[10] == 1.0 and M.orders()[40] == 4.0
    assert all(not 0.0 < abs(q - 1.0) < 1.0 / 64.0 for q in M.orders())


@pytest.mark.parametrize("weight,N,seed,r", COUNT_CASES)
def test_counts_sum_to_the_depth_and_both_paths_agree(weight, N, seed, r):
    c = M.counts(weight, N, seed, r)
    assert int(c.sum()) == N and c.shape == (len(weight),)
    assert all(c[k] == 0 for k, w in enumerate(weight) if w == 0)       # a clone of weight 0 is never drawn
    if N <= 5003:
        assert c.tolist() == M.counts_plain(weight, N, seed, r)


def test_every_t_on_a_boundary_of_cum():
    """weights (1, 1, 1): t is cum[k] itself, the lower (inclusive) end of clone k"""
    ts = [M.draw(1, 1, i, 3) for i in range(12)]
    assert M.counts((1, 1, 1), 12, 1, 1).tolist() == [ts.count(0), ts.count(1), ts.count(2)] == [3, 4, 5]


def test_the_draws_are_fair():
    """weight (1, 3) at N = 100,000: within five standard deviations of 25,000 (the largest seen: 1.8)"""
    sd = math.sqrt(100000 * 0.25 * 0.75)
    dev = [abs(int(M.counts((1, 3), 100000, seed, r)[0]) - 25000) / sd for seed in (0, 1, 7) for r in (1, 2, 200)]
    assert max(dev) < 5.0, dev


# ---- Hill numbers that are known ---------------------------------------------------------------------------------------------------------
def test_equal_weights_give_the_number_of_clones():
    for C in (1, 2, 7, 300):
        for q in M.orders():
            assert M.hill([5] * C, 5 * C, q) == pytest.approx(C, rel=1e-12), (C, q)
    assert M.hill([0, 5, 0, 5], 10, 0.0) == 2.0 and M.hill([3], 3, 2.5) == 1.0


def test_hill_numbers_by_hand():
    assert M.hill([1, 3], 4, 2.0) == pytest.approx(1.0 / (0.0625 + 0.5625), rel=1e-15)
    assert M.hill([1, 3], 4, 1.0) == pytest.approx(math.exp(-(0.25 * math.log(0.25) + 0.75 * math.log(0.75))), rel=1e-15)
    d = [M.hill([50, 30, 15, 4, 1], 100, q) for q in M.orders()]
    assert d[0] == 5.0 and all(a > b for a, b in zip(d, d[1:]))          # the curve falls with q


def test_model_of_a_small_case_and_batches():
    r = M.diversity((0, 5, 0, 0, 7, 0), 1000, replicates=3)
    assert r["counts"][0].tolist() == [0, 405, 0, 0, 595, 0] and r["d"].shape == (3, 41) and (r["d"][:, 0] == 2.0).all()
    assert r["info"] == dict(clones=6, weighted=2, weight=12, depth=1000, replicates=3, batches=1, path=M.PATH_LDS)
    assert r["mean"][0] == 2.0 and r["sd"][0] == 0.0 and r["sd"][20] > 0.0
    assert r["observed"][20] == pytest.approx(1.0 / ((5 / 12) ** 2 + (7 / 12) ** 2), rel=1e-15)
    one = M.diversity((1, 3), 50, q=[2.0], replicates=1)
    assert one["sd"].tolist() == [0.0] and one["mean"][0] == one["d"][0][0]
    w = [1] * 5000
    for cells, batches in ((M.CELLS, 1), (10000, 4), (5000, 7), (1, 7), (35000, 1), (34999, 2)):
        assert M.diversity(w, 10, q=[0.0], replicates=7, cells=cells)["info"]["batches"] == batches, cells
    assert M.diversity(w, 10, q=[0.0], replicates=1, lds_clones=0)["info"]["path"] == M.PATH_GLOBAL


def test_tolerance_is_the_derived_one():
    assert M.rel_tol(0.0, 5) == 0.0
    assert M.rel_tol(2.0, 36) == 100 * 2.0 ** -52 and M.rel_tol(1.5, 36) == 200 * 2.0 ** -52
    assert M.rel_tol(1.0, 1) == 65 * 2.0 ** -52 and M.rel_tol(1.0, 1000) == 1064 * 2.0 ** -52 * math.log(1000)


# ---- the weights of `vdjer --diversity` --------------------------------------------------------------------------------------------------
def test_diversity_weights_on_handmade_cells():
    from vdjer_amd import annot
    clone = [0, 1, -1, 0, 2, 3, 3]
    cells = ["12.34", "0.00", "99.99", "0.66", "1.00", "0.00", "0.01"]
    w, numbers = annot.diversity_weights(clone, cells)
    assert w.dtype == np.uint64 and w.tolist() == [1300, 100, 1] and numbers == [0, 2, 3]      # lineage 1 has weight 0; contig 2 is in no lineage
    assert (w.tolist(), numbers) == M.weights(clone, cells)
    assert annot.diversity_weights([0], ["184467440737095516.15"])[0].tolist() == [(1 << 64) - 1]      # read from the digits, no float
    assert annot.diversity_weights([-1, -1], ["1.00", "2.00"])[0].shape == (0,) and annot.diversity_weights([], [])[1] == []
    for bad in ("1.5", "1", "1.234", "-1.00", "1e2", ".50"):
        with pytest.raises(ValueError):
            annot.diversity_weights([0], [bad])
    assert M.default_depth([1300, 100, 1]) == 14 and M.default_depth([149]) == 1 and M.default_depth([150]) == 2 and M.default_depth([]) == 1
    assert M.default_depth([49]) == 1                                   # at least 1


def test_table_rows_and_summary_line():
    r = M.diversity((50, 30, 15, 4, 1), 100, replicates=8, seed=3)
    rows = M.table_rows(M.orders(), r["observed"], r["mean"], r["sd"])
    assert len(rows) == 41 and [row[0] for row in rows[:3]] == ["0.0", "0.1", "0.2"] and rows[40][0] == "4.0"
    assert all(re.fullmatch(r"\d+\.\d{4}", cell) for row in rows for cell in row[1:])
    assert rows[0][1] == "5.0000" and rows[0][6] == "1.0000"             # observed richness; e at q = 0
    j = 20
    lo = max(r["mean"][j] - M.Z95 * r["sd"][j], 0.0)
    assert rows[j][2] == "%.4f" % r["mean"][j] and rows[j][4] == "%.4f" % lo and rows[j][7] == "%.4f" % (lo / r["mean"][0])
    text = M.table_text(rows)
    assert text.splitlines()[0] == "q\td_observed\td\td_sd\td_lower\td_upper\te\te_lower\te_upper" and text.count("\n") == 42
    assert M.table_text([]) == "\t".join(M.COLUMNS) + "\n"
    line = M.summary_line(9, [1300, 100, 1], 14, 8, 3, r["mean"], 1)
    assert line == (f"diversity: 3 lineages with weight of 9, 14.01 expected pairs, depth 14, 8 replicates (seed 3), richness {r['mean'][0]:.2f}, "
                    f"shannon {r['mean'][10]:.4f}, simpson {r['mean'][20]:.4f}, 1 batches")
    assert M.summary_line(2, [], 1, 200, 1, None, 0) == ("diversity: 0 lineages with weight of 2, 0.00 expected pairs, depth 1, 200 replicates (seed 1), "
                                                         "richness 0.00, shannon 0.0000, simpson 0.0000, 0 batches")


# ---- the ABI mirror ----------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_exports():
    from vdjer_amd import _lib, api
    assert ctypes.sizeof(_lib.DiversityInfo) == 32 and ctypes.sizeof(_lib.DiversityParams) == 16
    assert [f for f, _ in _lib.DiversityInfo._fields_] == M.FIELDS == list(api.Context.DIVERSITY_FIELDS)
    assert [f for f, _ in _lib.DiversityParams._fields_] == ["replicates", "depth", "seed"]
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    assert re.search(r"\bint vdjx_diversity\(vdjx_ctx\* ctx, const uint64_t\* weight, size_t C, const double\* q, size_t Q, const vdjx_diversity_params\* params,", header)
    assert "2241935815489788276" in header and "(24932, 75068)" in header
    for word in ("Chao1", "rank-abundance", "second field", "several depths", "beta diversity"):      # what is not modelled is said
        assert word in header, word
    assert re.search(r"#define VDJX_DIV_PATH_LDS\s+%d\b" % M.PATH_LDS, header) and re.search(r"#define VDJX_DIV_PATH_GLOBAL\s+%d\b" % M.PATH_GLOBAL, header)
    assert "vdjx_diversity" in _lib.SYMBOLS and hasattr(_lib.lib(), "vdjx_diversity")
    source = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_diversity.hip")).read()
    assert re.search(r'vdjx_env_num\("VDJX_DIV_CELLS", 1ll << 28, 1, 1ll << 30\)', source)
    assert re.search(r'vdjx_env_num\("VDJX_DIV_LDS_CLONES", DIV_LDS_MAX, 0, DIV_LDS_MAX\)', source) and re.search(r"#define DIV_LDS_MAX %du\b" % M.LDS_CLONES, source)


# ---- the command line, up to where a GPU would be needed ---------------------------------------------------------------------------------
FULL = ["--quant", "q.tsv", "--lineages", "l.tsv", "--diversity", "d.tsv"]


def _refused(r, tmp_path):
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr, r.stderr[-500:]
    assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
    assert not any((tmp_path / f).exists() for f in ("d.tsv", "l.tsv", "q.tsv", "c.tsv"))


def test_cli_diversity_needs_lineages(tmp_path):
    for extra in (["--diversity", "d.tsv"], ["--quant", "q.tsv", "--diversity", "d.tsv"]):
        r = _run(tmp_path, extra)
        _refused(r, tmp_path)
        assert "--diversity" in r.stderr and "it needs --lineages" in r.stderr, (extra, r.stderr[-500:])


def test_cli_diversity_needs_the_quant_step(tmp_path):
    r = _run(tmp_path, ["--lineages", "l.tsv", "--diversity", "d.tsv"])
    _refused(r, tmp_path)
    assert "--diversity" in r.stderr and "it needs --quant <file> or --clones <file>" in r.stderr, r.stderr[-500:]
    for extra in (["--quant", "q.tsv"], ["--clones", "c.tsv"]):         # either gives the counts: the flags pass, and --gpus 2 ends the run before any GPU work
        r = _run(tmp_path, ["--lineages", "l.tsv", "--diversity", "d.tsv", "--gpus", "2"] + extra)
        _refused(r, tmp_path)
        assert "it needs" not in r.stderr and f"{extra[0]} runs on one GPU only" in r.stderr, r.stderr[-500:]


def test_cli_diversity_runs_on_one_gpu(tmp_path):
    r = _run(tmp_path, FULL + ["--gpus", "2"])
    _refused(r, tmp_path)
    assert "--quant runs on one GPU only" in r.stderr


@pytest.mark.parametrize("flag,value", [("--diversity-depth", "5000"), ("--diversity-boot", "16"), ("--diversity-seed", "7")])
def test_cli_diversity_options_need_diversity(flag, value, tmp_path):
    r = _run(tmp_path, ["--quant", "q.tsv", "--lineages", "l.tsv", flag, value])
    _refused(r, tmp_path)
    assert flag in r.stderr and "it needs --diversity <file>" in r.stderr, r.stderr[-500:]


def test_cli_diversity_values_out_of_range(tmp_path):
    for bad in ("0", "2147483648", "-1", "16x", "1.5", "", "+4", " 4", "99999999999999999999999"):
        r = _run(tmp_path, FULL + ["--diversity-depth", bad])
        _refused(r, tmp_path)
        assert "--diversity-depth must be a whole decimal number in 1 .. 2147483647" in r.stderr, (bad, r.stderr[-500:])
    for bad in ("0", "4097", "-1", "16x", "1.5", "", "+4", "99999999999999999999999"):
        r = _run(tmp_path, FULL + ["--diversity-boot", bad])
        _refused(r, tmp_path)
        assert "--diversity-boot must be a whole decimal number in 1 .. 4096" in r.stderr, (bad, r.stderr[-500:])
    for bad in ("18446744073709551616", "-1", "7x", "", "0x10"):
        r = _run(tmp_path, FULL + ["--diversity-seed", bad])
        _refused(r, tmp_path)
        assert "--diversity-seed must be a whole decimal number below 2^64" in r.stderr, (bad, r.stderr[-500:])
    for flag, good in (("--diversity-depth", "2147483647"), ("--diversity-boot", "4096"), ("--diversity-seed", "18446744073709551615")):
        r = _run(tmp_path, FULL + [flag, good, "--gpus", "2"])          # the ends of the ranges are values: the flags pass, --gpus 2 ends the run
        _refused(r, tmp_path)
        assert "must be a whole decimal number" not in r.stderr and "--quant runs on one GPU only" in r.stderr, (flag, r.stderr[-500:])


def test_cli_usage_names_the_flags(tmp_path):
    r = _run(tmp_path, ["--diversity", "d.tsv"])
    for flag in ("--diversity <file", "--diversity-depth <n", "--diversity-boot <B", "--diversity-seed <seed"):
        assert flag in r.stderr, flag
