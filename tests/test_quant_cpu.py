"""CPU checks of the contig-abundance model (tests/quant_model.py, the restatement vdjx_quant is tested against) and of the parts of
`vdjer --quant` that run before any GPU work.

The handmade cases of tests/quant_cases.py (no GPU), and the models against each other on them: what tests/test_gpu_quant_edges.py then
holds vdjx_quant_pairs to.

The one-iteration bound.  Relative, per contig c: k u / (1 - k u) with u = 2^-53 and k = D_c + m_c + 10, D_c the largest degree among
the pairs with an alignment on c and m_c the alignments on c.  In float64 g(f) costs 2 roundings (P(f) and the division by the span;
the counts are exact integers), the start value 1, the product N g 1; a pair's sum of D non-negative terms costs D - 1 in any order; the
division 1 (2 allowed); the contig's sum of m non-negative r costs m - 1 in any order; a fused multiply-add only removes roundings.  The
numerator of r carries 4 of these, its denominator 4 + D - 1, so r has at most D + 8 with the division and N_c at most D + m + 7."""
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import golden_util as G
from tests import quant_cases as K
from tests import quant_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = ["e2e_tiled", "e2e_mixed", "e2e_k25", "e2e_igk", "e2e_igl", "e2e_rl100", "e2e_rl151"]


@pytest.mark.parametrize("tag", E2E)
def test_model_on_golden_sam_counts_pairs_per_contig(tag):
    """no golden SAM places a pair twice: every r is 1, so the counts are the pairs per contig exactly, after at most two iterations"""
    ids, L, names, a = Q.sam_placements(G.text(f"{tag}.sam.gz"))
    assert L == 360 and len(ids) > 0 and a.shape[0] > 0
    assert np.unique(a[:, 0]).size == a.shape[0]             # (one placement per pair)
    N, info = Q.quant(a[:, 0], a[:, 1], a[:, 2], len(ids), L)
    assert np.array_equal(N, np.bincount(a[:, 1], minlength=len(ids)).astype(np.float64))
    assert info["pairs"] == len(names) == info["unique_pairs"] == info["alignments"]
    assert info["iterations"] <= 2 and info["converged"]
    assert 0 < info["eff_len"] < L


def _multi_set():
    """three contigs: contig 0 holds pairs placed there alone, contigs 1 and 2 share pairs, contig 3 has none; pair 9 is placed twice
    on contig 1"""
    rows = [(0, 0, 170), (1, 0, 180), (2, 0, 175),                       # unique on 0
            (3, 1, 160), (4, 2, 190), (5, 1, 175),                       # unique on 1 / 2
            (6, 1, 170), (6, 2, 170), (7, 1, 200), (7, 2, 210), (8, 2, 150), (8, 1, 150),
            (9, 1, 120), (9, 1, 300), (10, 0, 175), (10, 1, 176), (10, 2, 177)]
    return np.array(rows, np.int64)


def test_model_invariants_on_multi_mapping_set():
    a = _multi_set()
    N, info = Q.quant(a[:, 0], a[:, 1], a[:, 2], 4, 360, tol=0, max_iter=300)
    assert info["pairs"] == 11 and info["alignments"] == a.shape[0] and info["iterations"] == 300 and not info["converged"]
    assert info["unique_pairs"] == 6
    assert N.sum() == pytest.approx(11, rel=1e-12)                      # every placed pair is shared out in full
    assert N[3] == 0.0                                                   # no placement: stays 0
    assert N[0] >= 3 and N[1] >= 2 and N[2] >= 1                         # unique pairs keep their contig's share
    assert np.all(N[:3] <= np.array([4, 7, 6]))
    # the default stop rule ends early and lands near the fixed point
    Nd, infod = Q.quant(a[:, 0], a[:, 1], a[:, 2], 4, 360)
    assert infod["converged"] and infod["iterations"] < 300
    assert np.allclose(Nd, N, rtol=1e-3)


def test_model_edge_cases():
    N, info = Q.quant([], [], [], 3, 360)
    assert np.array_equal(N, np.zeros(3)) and info["pairs"] == 0 and info["iterations"] == 0
    # one pair, two placements on the same contig: the contig explains one pair
    N, info = Q.quant([0, 0], [1, 1], [150, 250], 2, 360)
    assert N.tolist() == [0.0, 1.0] and info["pairs"] == 1 and info["unique_pairs"] == 0


def test_frag_weights_are_a_distribution():
    g, eff, uniq = Q.frag_weights([0, 1, 1, 2], [175, 175, 180, 200], 360)
    assert uniq == 2
    f = np.arange(50, 401)
    h = np.zeros(351)
    h[175 - 50] += 1
    h[200 - 50] += 1
    Pf = (h + 1) / (h + 1).sum()
    assert eff == pytest.approx(float((Pf * (360 - f + 1))[f <= 360].sum()), rel=1e-12)
    assert g[0] == pytest.approx(Pf[125] / (360 - 175 + 1), rel=1e-15)


def _cli_inputs(d):
    open(os.path.join(d, "reads.txt"), "w").write("P r1 1 0 ACGTACGTAC IIIIIIIIII\nP r1 2 1 ACGTACGTAC IIIIIIIIII\n")
    os.makedirs(os.path.join(d, "ref"), exist_ok=True)
    for fn in ("v_index", "j_index"):
        open(os.path.join(d, "ref", fn), "w").write("1\t0\n")
    open(os.path.join(d, "ref", "v_region.fa"), "w").write(">v\nACGT\n")


def test_cli_quant_refuses_sharded_runs_before_any_gpu_work(tmp_path):
    """`--quant` is one GPU only: with VDJX_FORCE_MGPU (the sharded code path on one rank) the command line stops after parsing,
    with a message and without a table -- no GPU is needed to get there"""
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    assert os.path.exists(exe), "build it: make -C vdjer_amd/csrc/host"
    _cli_inputs(str(tmp_path))
    r = subprocess.run([exe, "--in", "reads.txt", "--chain", "IGH", "--ref-dir", "ref", "--ins", "175", "--quant", "q.tsv"], cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=dict(os.environ, VDJX_FORCE_MGPU="1"))
    assert r.returncode != 0
    assert "--quant runs on one GPU only" in r.stderr
    assert "ELAPSED_SECS" not in r.stderr
    assert not (tmp_path / "q.tsv").exists()


def test_cli_usage_names_quant(tmp_path):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    r = subprocess.run([exe, "--help", "x"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--quant" in r.stderr


# ---- the handmade cases and the exact model ----------------------------------------------------------------------------------------------
U = 2.0 ** -53
F_ITERS = (2, 31, 32, 33, 64, 65)


def one_iteration_bounds(case, degree):
    """the bound of the module's docstring for every contig (0 where it has no alignment)"""
    pr, ct, _ = K.triples(case)
    d = np.array([degree[int(p)] for p in pr], np.int64)
    out = np.zeros(case["n"])
    for c in np.unique(ct):
        k = int(d[ct == c].max()) + int((ct == c).sum()) + 10
        out[c] = k * U / (1.0 - k * U)
    return out


def assert_within_one_iteration_bound(N, exact, bounds, what):
    """|N_c - exact_c| <= bound_c exact_c, decided in rationals; -> the worst error as a fraction of its bound"""
    worst = 0.0
    for c, (x, e, b) in enumerate(zip(N, exact, bounds)):
        err = abs(Fraction(float(x)) - e)
        assert err <= Fraction(float(b)) * e, (what, c, float(x), float(e), float(err / e) if e else None, float(b))
        if e:
            worst = max(worst, float(err / e) / b)
    return worst


@functools.lru_cache(maxsize=None)
def exact_a():
    return Q.quant_one_exact(*K.triples(K.case_a()), 101, 360)


@functools.lru_cache(maxsize=None)
def trace_a():
    return Q.quant_trace(*K.triples(K.case_a()), 101, 360, 70)


def stop_tolerances(delta, iters):
    """{t: tol} such that the stop rule first holds after iteration t: the geometric mean of delta_t and delta_(t-1), after the
    precondition that every earlier delta lies above it and delta_t below it by a factor of 1 - 1e-3 at least"""
    out = {}
    for t in iters:
        assert delta[t - 1] < delta[t - 2] * (1 - 1e-3), (t, delta[t - 2], delta[t - 1])
        tol = float(np.sqrt(delta[t - 1] * delta[t - 2]))
        assert delta[t - 1] < tol * (1 - 4e-4) and (delta[:t - 1] > tol * (1 + 4e-4)).all(), (t, tol, delta[:t])
        out[t] = tol
    return out


def test_case_a_is_on_the_edges_it_names():
    a = K.case_a()
    pr, ct, ins = K.triples(a)
    ids, deg = np.unique(pr, return_counts=True)
    assert a["n"] == 101 and 6000 < pr.size < 7000 and ins.min() >= 50 and ins.max() <= 360
    assert all((deg == d).sum() >= 3 for d in K.A_DEGREES) and deg.max() == 100 > K.Q_LIGHT
    assert (ids % 2 == 1).all() and ids[0] == 1 and ids[-1] == a["n_pairs"] - 2          # ids 0 and n_pairs - 1, and every other id, are free
    slot = {d: np.flatnonzero(deg == d) for d in (32, 33)}
    assert set(slot[32] + 1) == set(slot[33])                                             # degrees 32 and 33 are neighbours
    assert any(q % 256 == 255 for q in slot[32])                                          # ... once across two workgroups
    heavy = np.flatnonzero(deg > K.Q_LIGHT)
    waves = heavy // K.WAVE
    assert np.bincount(waves).max() >= 2                                                  # two whole-wave pairs in one wave
    assert all((deg[w * K.WAVE:(w + 1) * K.WAVE] <= K.Q_LIGHT).any() for w in set(waves))   # ... beside light ones
    assert ids.size % K.WAVE and (ids.size - 1) // K.WAVE in set(waves)                   # ... and in the grid's last, partial wave
    assert np.bincount(ct)[100] == K.A_BIG == 2 * K.Q_CHUNK + 1                           # three chunks of the M step, the last of one
    on_big = pr[ct == 100]
    assert np.unique(on_big).size == K.A_BIG and (np.bincount(pr)[on_big] == 2).sum() == (K.A_BIG + 2) // 3


def test_float64_first_iteration_within_the_bound_of_the_exact_one():
    exact, degree = exact_a()
    bounds = one_iteration_bounds(K.case_a(), degree)
    assert 0 < bounds.max() < 6e-13
    worst = assert_within_one_iteration_bound(trace_a()[0][0], exact, bounds, "case A")
    print("worst error / bound:", worst)
    assert sum(exact) == len(degree)                                                      # every placed pair is shared out whole


def test_trace_of_case_a_satisfies_the_stop_tests_precondition():
    N, delta = trace_a()
    assert N.shape == (70, 101) and delta.shape == (70,)
    tol = stop_tolerances(delta, F_ITERS)
    assert sorted(tol) == list(F_ITERS) and all(tol[a] > tol[b] for a, b in zip(F_ITERS, F_ITERS[1:]))
    # an off-by-one around a batch of 32 iterations shows: N_t is far from N_32 and N_64 at 1e-9 where t is neither
    for t in F_ITERS:
        for s in (32, 64):
            if t != s:
                assert np.max(np.abs(N[t - 1] - N[s - 1]) / np.maximum(N[s - 1], 1e-12)) > 1e-4, (t, s)
    # the trace is quant's own iteration
    for t in (1, 33):
        Nq, info = Q.quant(*K.triples(K.case_a()), 101, 360, max_iter=t, tol=0)
        assert Nq.tobytes() == N[t - 1].tobytes() and info["iterations"] == t and not info["converged"]
    Nq, info = Q.quant(*K.triples(K.case_a()), 101, 360, tol=tol[33])
    assert Nq.tobytes() == N[32].tobytes() and info["iterations"] == 33 and info["converged"]


# the cases the GPU tests hold to 1e-9 / 1e-12 after many iterations, with the iterations they run for
MANY = [("A", lambda: K.case_a(), 200)] + [(f"D{p}{'+' if last else '-'}", lambda p=p, last=last: K.case_d(p, last), 50)
                                            for p in (4095, 4096, 4097, 8193) for last in (0, 1)] \
    + [(f"E{L}", lambda L=L: K.case_e(L), 50) for L in K.E_LENS] + [(f"C{n}", lambda n=n: K.case_c(n), 12) for n in (1023, 1024, 1025, 2049)]


@pytest.mark.parametrize("name,make,iters", MANY, ids=[m[0] for m in MANY])
def test_reordering_the_placements_moves_the_model_by_less_than_1e_10(name, make, iters):
    """1e-9 relative (1e-12 absolute for the starved contigs, which are below 1e-57 after 70 iterations of case A and go on falling) is attainable: another summation order alone
    moves the float64 model by far less.  (No case had to be run for fewer iterations to pass this.)"""
    case = make()
    pr, ct, ins = K.triples(case)
    N, _ = Q.quant(pr, ct, ins, case["n"], case["L"], max_iter=iters, tol=0)
    Nr, _ = Q.quant(pr[::-1], ct[::-1], ins[::-1], case["n"], case["L"], max_iter=iters, tol=0)
    np.testing.assert_allclose(Nr, N, rtol=1e-10, atol=1e-12)


def test_exact_model_on_small_inputs():
    # one pair on two contigs with equal inserts: half each; a pair outside the window: nothing; contig 2 has no placement
    N, deg = Q.quant_one_exact([0, 0, 1, 2], [0, 1, 1, 3], [100, 100, 200, 401], 4, 360)
    assert N == [Fraction(1, 2), Fraction(3, 2), 0, 0] and deg == {0: 2, 1: 1, 2: 1}
    # unequal inserts, nothing placed once: g = 1 / (351 (L - f + 1)), so r = (1 / 261) / (1 / 261 + 1 / 61)
    N, _ = Q.quant_one_exact([5, 5], [0, 1], [100, 300], 2, 360)
    assert N == [Fraction(61, 322), Fraction(261, 322)]
    # an insert longer than the contig weighs nothing
    N, _ = Q.quant_one_exact([5, 5], [0, 1], [100, 300], 2, 299)
    assert N == [1, 0]
    assert Q.quant_one_exact([], [], [], 3, 360) == ([0, 0, 0], {})
    Nt, d = Q.quant_trace([], [], [], 3, 360, 5)
    assert Nt.shape == (0, 3) and d.shape == (0,)
