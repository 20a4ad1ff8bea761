"""CPU checks of the abundance bootstrap (include/vdjx.h, vdjx_quant_boot): the model of tests/quant_boot_model.py that
tests/test_gpu_quant_boot.py holds the device to, vdjx_quant_boot_summary (plain C, no GPU), and the parts of `vdjer --quant-boot`
that run before any GPU work.

The many-iteration tolerance.  test_reordering_the_sums_moves_the_weighted_model_by_less_than_1e_10 evaluates the weighted model on
case A for 200 iterations with the sums inside pairs and inside contigs made in shuffled orders: the replicates stay within rtol 1e-10,
atol 1e-13 of each other (the worst relative spread measured here: 7.1e-16 where N > 1e-12), a factor of ten inside the suite's rtol 1e-9,
atol 1e-12, which the GPU tests therefore use unchanged.  The figure is the model's against itself, never the device's."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import quant_boot_model as QB
from tests import quant_cases as K
from tests import quant_model as Q
from tests import test_quant_cpu as T
from vdjer_amd import annot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANY_RTOL, MANY_ATOL = 1e-9, 1e-12           # the suite's many-iteration tolerance (kept: see the module's docstring)
STOP_SEED, STOP_REPLICATES = 1, 4


@functools.lru_cache(maxsize=None)
def mult_a(seed, r):
    return QB.draws(seed, r, QB.slots(K.case_a()["pid"]).size)


@functools.lru_cache(maxsize=None)
def trace_a(seed, r, iters):
    return QB.trace(*K.triples(K.case_a()), 101, 360, mult_a(seed, r), iters)


# ---- the draw rule ---------------------------------------------------------------------------------------------------------------------
def test_draws_sum_to_the_placed_pairs_and_depend_on_seed_and_replicate():
    Pp = QB.slots(K.case_a()["pid"]).size
    assert Pp == 3 * len(K.A_DEGREES) + K.A_BIG
    m1, m2, m1s = QB.draws(1, 1, Pp), QB.draws(1, 2, Pp), QB.draws(2, 1, Pp)
    for m in (m1, m2, m1s):
        assert m.dtype == np.uint32 and m.shape == (Pp,) and int(m.sum()) == Pp
    assert np.array_equal(m1, QB.draws(1, 1, Pp))
    assert not np.array_equal(m1, m2) and not np.array_equal(m1, m1s)
    # about 1 / e of the slots are not drawn at all
    assert 0.3 < (m1 == 0).mean() < 0.45
    # the rule is vdjx_diversity's with W = Pp
    assert [annot.quant_boot_draw(7, 3, i, 11) for i in range(20)] == [annot.diversity_draw(7, 3, i, 11) for i in range(20)]
    assert all(0 <= annot.quant_boot_draw(1, 1, i, 3) < 3 for i in range(50))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_multiplicities_of_one_give_the_point_estimates_trace_exactly():
    a = K.case_a()
    Pp = QB.slots(a["pid"]).size
    N, d = QB.trace(*K.triples(a), 101, 360, np.ones(Pp, np.uint32), 40)
    Nq, dq = Q.quant_trace(*K.triples(a), 101, 360, 40)
    assert N.tobytes() == Nq.tobytes() and d.tobytes() == dq.tobytes()
    Nr, it, conv = QB.run(*K.triples(a), 101, 360, np.ones(Pp, np.uint32))
    Np, info = Q.quant(*K.triples(a), 101, 360)
    assert Nr.tobytes() == Np.tobytes() and (it, conv) == (info["iterations"], info["converged"])


def test_case_b_counts_are_the_sums_of_the_multiplicities():
    """every pair is placed once and every r is 1.0: N_c is the sum of its pairs' multiplicities after iteration 1 and for good"""
    b = K.case_b()
    pr, ct, ins = K.triples(b)
    ids = QB.slots(pr)
    for r in (1, 2):
        m = QB.draws(5, r, ids.size)
        want = np.bincount(ct, weights=m[np.searchsorted(ids, pr)].astype(np.float64), minlength=b["n"])
        N, d = QB.trace(pr, ct, ins, b["n"], b["L"], m, 4)
        assert all(N[t].tolist() == want.tolist() for t in range(4)) and d[1:].tolist() == [0.0] * 3
        assert N[0].sum() == ids.size


# ---- the summary -------------------------------------------------------------------------------------------------------------------------
def test_summary_indices_by_hand():
    assert [QB.summary_indices(B) for B in (1, 2, 40, 41, 1024)] == [(0, 0), (0, 1), (0, 39), (1, 39), (25, 998)]


@pytest.mark.parametrize("B", [1, 2, 40, 41, 1024])
def test_summary_in_c_against_the_definition(B):
    rng = np.random.default_rng(B)
    boot = rng.gamma(2.0, 50.0, (B, 7))
    boot[:, 3] = 0.0                                                     # a contig without a placement
    boot[:, 5] = 12.5                                                    # a contig that never moves
    got, want = annot.quant_boot_summary(boot), QB.summary(boot)
    lo, hi = QB.summary_indices(B)
    srt = np.sort(boot, axis=0)
    assert got["lower"].tolist() == want["lower"] == srt[lo].tolist()
    assert got["upper"].tolist() == want["upper"] == srt[hi].tolist()
    for k in ("mean", "sd"):
        for x, y, mu in zip(got[k], want[k], want["mean"]):
            assert abs(x - y) <= 1e-12 * abs(y) + 1e-12 * max(1.0, mu), (k, x, y)
    assert got["sd"][3] == 0.0 and got["mean"][3] == 0.0 and got["lower"][5] == got["upper"][5] == 12.5
    if B == 1:
        assert got["sd"].tolist() == [0.0] * 7 and got["mean"].tolist() == boot[0].tolist()


# ---- tolerances and the stop rule's inputs -------------------------------------------------------------------------------------------
def test_reordering_the_sums_moves_the_weighted_model_by_less_than_1e_10():
    a = K.case_a()
    pr, ct, ins = K.triples(a)
    m = mult_a(1, 1)
    base = QB.trace(pr, ct, ins, 101, 360, m, 200)[0][-1]
    worst = 0.0
    for k in range(3):
        o = np.random.default_rng(k).permutation(pr.size)
        N = QB.trace(pr, ct, ins, 101, 360, m, 200, order=o)[0][-1]
        np.testing.assert_allclose(N, base, rtol=MANY_RTOL / 10, atol=MANY_ATOL / 10)
        big = base > 1e-12
        worst = max(worst, float(np.max(np.abs(N - base)[big] / base[big])))
    print("worst relative spread after 200 iterations:", worst)
    assert base.sum() == pytest.approx(float(m.sum()), rel=1e-9)


@functools.lru_cache(maxsize=None)
def boot_stop_tol():
    """-> (tol, [iterations of replicate 1 .. 4 of case A, seed 1 under it]): the first tol of a geometric grid under which every
    replicate's deltas keep stop_tolerances' margin (every delta before the stop above tol (1 + 4e-4), the stopping one below
    tol (1 - 4e-4)), the iterations differ between replicates and lie on both sides of Q_BATCH"""
    deltas = [trace_a(STOP_SEED, r, 120)[1] for r in range(1, STOP_REPLICATES + 1)]
    for k in range(0, 200):
        tol = float(10.0 ** (-1.0 - k / 50.0))
        its = []
        for d in deltas:
            below = np.flatnonzero(d < tol)
            if below.size == 0:
                break
            t = int(below[0]) + 1
            if not (d[t - 1] < tol * (1 - 4e-4) and (d[:t - 1] > tol * (1 + 4e-4)).all()):
                break
            its.append(t)
        if len(its) == len(deltas) and len(set(its)) > 1 and min(its) < K.Q_BATCH < max(its):
            return tol, its
    raise AssertionError("no tol of the grid separates the replicates")


def test_a_tol_stops_the_replicates_on_both_sides_of_a_batch():
    tol, its = boot_stop_tol()
    print("tol", tol, "iterations", its)
    assert len(its) == STOP_REPLICATES and len(set(its)) > 1 and min(its) < K.Q_BATCH < max(its)
    for r, t in zip(range(1, STOP_REPLICATES + 1), its):
        N, it, conv = QB.run(*K.triples(K.case_a()), 101, 360, mult_a(STOP_SEED, r), tol=tol)
        assert (it, conv) == (t, True) and N.tobytes() == trace_a(STOP_SEED, r, 120)[0][t - 1].tobytes()
    # the prototype's figures: the traces cross 0.01 at iterations 20, 32, 40 and 43
    assert [int(np.flatnonzero(trace_a(STOP_SEED, r, 120)[1] < 0.01)[0]) + 1 for r in range(1, 5)] == [20, 32, 40, 43]


# ---- the command line and the ABI ----------------------------------------------------------------------------------------------------------
def _run_cli(tmp_path, *flags):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    assert os.path.exists(exe), "build it: make -C vdjer_amd/csrc/host"
    T._cli_inputs(str(tmp_path))
    return subprocess.run([exe, "--in", "reads.txt", "--chain", "IGH", "--ref-dir", "ref", "--ins", "175"] + list(flags), cwd=tmp_path,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


@pytest.mark.parametrize("flags,message", [
    (["--quant-boot", "20"], "--quant-boot bootstraps the --quant table: it needs --quant <file>"),
    (["--quant", "q.tsv", "--quant-boot", "0"], "--quant-boot must be a whole decimal number in 1 .. 1024: 0"),
    (["--quant", "q.tsv", "--quant-boot", "1025"], "--quant-boot must be a whole decimal number in 1 .. 1024: 1025"),
    (["--quant", "q.tsv", "--quant-boot", "2.5"], "--quant-boot must be a whole decimal number in 1 .. 1024: 2.5"),
    (["--quant", "q.tsv", "--quant-seed", "3"], "--quant-seed is the seed of the --quant-boot replicates: it needs --quant-boot <B>"),
    (["--quant", "q.tsv", "--quant-boot", "20", "--quant-seed", "18446744073709551616"], "--quant-seed must be a whole decimal number below 2^64"),
    (["--quant", "q.tsv", "--quant-boot", "20", "--quant-seed", "-1"], "--quant-seed must be a whole decimal number below 2^64"),
])
def test_cli_refuses_before_any_gpu_work(tmp_path, flags, message):
    r = _run_cli(tmp_path, *flags)
    assert r.returncode != 0
    assert message in r.stderr
    assert "ELAPSED_SECS" not in r.stderr
    assert not (tmp_path / "q.tsv").exists()


def test_cli_usage_names_the_flags(tmp_path):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    r = subprocess.run([exe, "--help", "x"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--quant-boot" in r.stderr and "--quant-seed" in r.stderr


def test_symbols():
    from vdjer_amd import _lib
    for s in ("vdjx_quant_boot", "vdjx_quant_pairs_boot", "vdjx_quant_boot_summary"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)
