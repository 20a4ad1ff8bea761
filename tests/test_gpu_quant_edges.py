"""vdjx_quant_pairs on the GPU: the EM of vdjer_amd/csrc/vdjx_quant.hip over handmade placements (tests/quant_cases.py), at every edge the
kernels turn on, against the models of tests/quant_model.py.  vdjx_quant maps its contigs itself, so tests/test_gpu_quant.py can only
feed these kernels what the goldens happen to place; vdjx_quant_pairs runs the same code over placements the test writes down.

Which case runs which path (every test asserts from its own inputs that its case is where it says):
  the whole-wave path of k_q_order and k_q_estep for pairs of more than Q_LIGHT = 32 alignments (__ballot / readlane hand-over, strided
      rank loop, float64 butterfly): case A, degrees 33, 63, 64, 65 and 100 beside 1, 2, 31 and 32 -- two of them in one wave, a
      32 | 33 across two workgroups, one run in the grid's last wave of 28 pairs
  a contig of more than Q_CHUNK = 2,048 alignments (several k_q_mpart workgroups, added in order by k_q_mfin): A (4,097 on contig 100), B
  k_q_mfin past 1,024 contigs (its c += 1024 loop feeds N and the stop rule's maximum): C
  the stop flag across the host's batches of Q_BATCH = 32 iterations, the iterations queued behind it, buffer iters & 1: F (and B, E)
  weights that are zero (inserts outside [50, 400], inserts longer than the contig, len < 50; the sum > 0 ? ... : 0 arm): E
  pairs of degree zero at id 0 and id P - 1, P around VDJX_SCAN_BLOCK: A, B, D
  contigs without placements first, last, between two others and adjacent (k_q_align's binary search, k_q_init): B; every 7th: C
  vdjx_quant = map + the same function: G;  refusals, the empty calls, nothing kept on the device: H

Tolerances.  One iteration (A, C): the bound derived in tests/test_quant_cpu.py's docstring, relative per contig k u / (1 - k u), u = 2^-53,
k = D_c + m_c + 10 (D_c the largest degree of a pair on c, m_c the alignments on c): g costs 2 roundings, the start value 1, the product
1, a pair's sum of D non-negative terms D - 1 in any order, the division 1 (2 allowed), the contig's sum of m non-negative r m - 1 in
any order; FMA contraction only removes roundings.  About 5e-13 at worst in A.  Many iterations: rtol 1e-9, atol 1e-12, the numbers of
tests/test_gpu_quant.py, shown attainable by test_quant_cpu.py's reordering check.  B and the degree-1 contigs of C: equality.

All device calls run in one child process; every model result is computed once."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import quant_cases as K
from tests import quant_model as Q
from tests import test_quant_cpu as T
from tests.scan_shapes import BLOCK
from tests.test_gpu_quant import _child_env, _context, _golden_contigs, _multi_set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_MAX_ITER = (1, 31, 32, 33, 64)
C_SIZES = (1023, 1024, 1025, 2049)
C_STOP = 5                                                               # the iteration case C's tol lets the model stop after
D_PAIRS = (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
FIELDS = ("pairs", "alignments", "unique_pairs", "iterations", "converged", "eff_len")


# ---- the models, each once -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trace_c(n):
    c = K.case_c(n)
    return Q.quant_trace(*K.triples(c), n, c["L"], 12)


@functools.lru_cache(maxsize=None)
def tolerances():
    """what the child needs from the models: the stop rule's tol for every iteration case F and case C stop after"""
    return dict(F={str(t): tol for t, tol in T.stop_tolerances(T.trace_a()[1], T.F_ITERS).items()},
                C={str(n): T.stop_tolerances(trace_c(n)[1], (C_STOP,))[C_STOP] for n in C_SIZES})


@functools.lru_cache(maxsize=None)
def model(name, iters):
    case = _cases()[name]
    return Q.quant(*K.triples(case), case["n"], case["L"], max_iter=iters, tol=0)


@functools.lru_cache(maxsize=None)
def model_default(name):
    case = _cases()[name]
    return Q.quant(*K.triples(case), case["n"], case["L"])


@functools.lru_cache(maxsize=None)
def _cases():
    out = {"A": K.case_a(), "B": K.case_b()}
    out.update({f"C{n}": K.case_c(n) for n in C_SIZES})
    out.update({f"D{p}/{last}": K.case_d(p, last) for p in D_PAIRS for last in (0, 1)})
    out.update({f"E{L}": K.case_e(L) for L in K.E_LENS})
    return out


# ---- the device, once ----------------------------------------------------------------------------------------------------------------------
def _pack(res):
    N, info = res
    return dict(N=N.tobytes().hex(), info=info)


def _device(tols):
    import ctypes as C
    from vdjer_amd import _lib, api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    cases = _cases()

    def run(name, **kw):
        c = cases[name]
        return _pack(ctx.quant_pairs(c["offs"], (c["pid"], c["ins"]), c["L"], c["n_pairs"], **kw))

    run("A", max_iter=2)                                                 # (the workspace is there before the kept bytes are read)
    kept0, allocs0 = ctx.stat("kept_device_bytes"), ctx.stat("kept_allocs")
    out = {}
    out["A/1"] = run("A", max_iter=1, tol=0)
    out["A/200"] = run("A", max_iter=200, tol=0)
    out["A/200 again"] = run("A", max_iter=200, tol=0)
    out["map_us"] = ctx.stat("quant_map_us")
    for t, tol in tols["F"].items():
        out[f"F/tol{t}"] = run("A", tol=tol)
    for m in F_MAX_ITER:
        out[f"F/max{m}"] = run("A", max_iter=m, tol=0)
    out["B/1"] = run("B", max_iter=1, tol=0)
    out["B/default"] = run("B")
    for n in C_SIZES:
        out[f"C{n}/1"] = run(f"C{n}", max_iter=1, tol=0)
        out[f"C{n}/tol"] = run(f"C{n}", tol=tols["C"][str(n)])
    for name in cases:
        if name[0] == "D":
            out[f"{name}/50"] = run(name, max_iter=50, tol=0)
        if name[0] == "E":
            out[f"{name}/1"] = run(name, max_iter=1, tol=0)
            out[f"{name}/50"] = run(name, max_iter=50, tol=0)
            out[f"{name}/default"] = run(name)
    # the packed form of `pairs` is the same call
    a = cases["A"]
    packed = np.zeros(a["pid"].size, api.PAIR_DTYPE)
    packed["pair_id"], packed["insert"] = a["pid"], a["ins"]
    packed["rec1"], packed["pos1"], packed["rc2"] = 0xFFFFFFFF, -7, 255   # (fields that are not read)
    assert _pack(ctx.quant_pairs(a["offs"], packed, 360, a["n_pairs"], max_iter=1, tol=0)) == out["A/1"]

    # H: the empty calls
    N0, i0 = ctx.quant_pairs([0], (np.zeros(0, np.uint32), np.zeros(0, np.int16)), 360, 10)
    assert N0.shape == (0,) and i0 == dict(pairs=0, alignments=0, unique_pairs=0, iterations=0, converged=True, eff_len=0.0)
    N0, i0 = ctx.quant_pairs([0, 0, 0, 0], (np.zeros(0, np.uint32), np.zeros(0, np.int16)), 360, 0)
    uniform = sum((360 - f + 1) / 351.0 for f in range(50, 361))
    assert N0.tolist() == [0.0] * 3 and i0 == dict(pairs=0, alignments=0, unique_pairs=0, iterations=0, converged=True, eff_len=i0["eff_len"])
    assert i0["eff_len"] == pytest.approx(uniform, rel=1e-12)
    # H: refusals; vdjx_last_error names the rule
    off, pid, ins = np.array([0, 2, 3], np.uint64), np.array([1, 0, 6], np.uint32), np.array([100, 200, 300], np.int16)
    assert ctx.quant_pairs(off, (pid, ins), 360, 7)[1]["pairs"] == 3
    for kw, match in ((dict(offsets=[1, 2, 3]), r"\(-1\).*offsets\[0\]=1 must be 0"), (dict(offsets=[0, 4, 3]), r"\(-1\).*decrease at contig 1"),
                      (dict(offsets=[0, 3, 3, 2, 3]), r"\(-1\).*decrease at contig 2"), (dict(n_pairs=6), r"\(-1\).*placement 2 names pair 6 of 6"),
                      (dict(n_pairs=0), r"\(-1\).*placement 0 names pair 1 of 0"), (dict(max_iter=0), r"\(-1\).*max_iter=0 must be at least 1"),
                      (dict(max_iter=-3), r"\(-1\).*max_iter=-3"), (dict(tol=-1e-300), r"\(-1\).*tol must be >= 0"),
                      (dict(tol=float("nan")), r"\(-1\).*tol must be >= 0"), (dict(length=0), r"\(-1\).*len=0"), (dict(length=-360), r"\(-1\).*len=-360"),
                      (dict(length=4096), r"\(-3\).*fewer than 4096 bases"),
                      (dict(offsets=np.concatenate([np.zeros((1 << 20) - 2, np.uint64), off])), r"\(-3\).*2\^20 - 1 contigs")):
        args = dict(dict(offsets=off, pairs=(pid, ins), length=360, n_pairs=7), **kw)
        with pytest.raises(VdjxError, match=match):
            ctx.quant_pairs(**args)
    assert ctx.quant_pairs(np.concatenate([np.zeros((1 << 20) - 3, np.uint64), off]), (pid, ins), 4095, 7)[0].shape == ((1 << 20) - 1,)
    # (the raw call: NULL arguments, and 2^32 placements, which are refused before a placement is read)
    L, h = ctx.L, ctx.h
    info, prm, cnt = _lib.QuantInfo(), _lib.QuantParams(10, 1e-5), np.zeros(2)
    pk = np.zeros(3, api.PAIR_DTYPE)
    pk["pair_id"], pk["insert"] = pid, ins
    good = dict(h=h, off=api._p(off), pk=api._p(pk), prm=C.byref(prm), cnt=api._p(cnt), info=C.byref(info))

    def raw(**kw):
        a_ = dict(good, **kw)
        return L.vdjx_quant_pairs(a_["h"], a_["off"], a_["pk"], 2, 360, 7, a_["prm"], a_["cnt"], a_["info"])

    assert raw() == 0 and info.pairs == 3
    for kw in (dict(h=None), dict(off=None), dict(pk=None), dict(prm=None), dict(cnt=None), dict(info=None)):
        info.pairs = 99
        assert raw(**kw) == -1 and b"vdjx_quant_pairs: NULL argument" in L.vdjx_last_error(), kw
        assert info.pairs == (0 if "pk" in kw else 99), kw                # (as in vdjx_quant: info is zeroed once ctx, params and info are there)
    wide = np.array([0, 3, 1 << 32], np.uint64)
    assert raw(off=api._p(wide)) == -3 and b"2^32 placements" in L.vdjx_last_error()
    # nothing is kept: scratch and the uploaded placements are the workspace's
    assert ctx.stat("kept_device_bytes") == kept0 and ctx.stat("kept_allocs") == allocs0
    ctx.close()

    # G: vdjx_quant is map + the same function
    c = G.Case("e2e_mixed")
    ctx, p = _context(c.pool)
    _, seqs = _golden_contigs("e2e_mixed")
    S = _multi_set(seqs, c.clones)
    offs, pairs = ctx.map_emit(S)
    pairs = pairs.copy()
    out["G/pairs"] = _pack(ctx.quant_pairs(offs, pairs, 360, c.pool.n_pairs))
    out["G/pairs map_us"] = ctx.stat("quant_map_us")
    out["G/pairs placed"] = ctx.stat("quant_contigs_placed")
    out["G/quant"] = _pack(ctx.quant(S))
    out["G/quant placed"] = ctx.stat("quant_contigs_placed")
    out["G/pairs 200"] = _pack(ctx.quant_pairs(offs, pairs, 360, c.pool.n_pairs, max_iter=200, tol=0))
    out["G/quant 200"] = _pack(ctx.quant(S, max_iter=200, tol=0))
    out["G/shape"] = [len(S), int(offs[-1]), int(np.unique(pairs["pair_id"]).size)]
    p.free()
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def device():
    code = f"import json; from tests.test_gpu_quant_edges import _device; print('QUANT', json.dumps(_device({tolerances()!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=_child_env("shipped"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("QUANT ")).split(" ", 1)[1])


def _got(key):
    d = device()[key]
    return np.frombuffer(bytes.fromhex(d["N"]), np.float64), d["info"]


def _counts_match(info, im, what):
    assert (info["pairs"], info["alignments"], info["unique_pairs"]) == (im["pairs"], im["alignments"], im["unique_pairs"]), (what, info, im)
    assert info["eff_len"] == pytest.approx(im["eff_len"], rel=1e-12), what


def _many(key, name, iters):
    """a fixed number of iterations against the float64 model"""
    N, info = _got(key)
    Nm, im = model(name, iters)
    np.testing.assert_allclose(N, Nm, rtol=1e-9, atol=1e-12, err_msg=key)
    _counts_match(info, im, key)
    assert info["iterations"] == iters and not info["converged"], (key, info)
    return N, info, Nm, im


# ---- A ---------------------------------------------------------------------------------------------------------------------------------
def test_degrees_around_a_wave_after_one_iteration_against_the_exact_model():
    """A: pairs of degree 1, 2, 31, 32 (one lane each) and 33, 63, 64, 65, 100 (the whole wave: k_q_order's strided rank loop and
    k_q_estep's butterfly), heavy beside light in one wave, 32 | 33 across two workgroups, a run in the grid's last wave of 28 pairs;
    contig 100 has three chunks of the M step.  One iteration, every contig within k u / (1 - k u) of the exact rational model
    (k = D_c + m_c + 10; the derivation is in the module's docstring)."""
    T.test_case_a_is_on_the_edges_it_names()                             # (degree above 32, 4,097 alignments on one contig, ... from the inputs)
    exact, degree = T.exact_a()
    assert max(degree.values()) == 100 > K.Q_LIGHT and {33, 64, 65} <= set(degree.values())
    N, info = _got("A/1")
    worst = T.assert_within_one_iteration_bound(N, exact, T.one_iteration_bounds(K.case_a(), degree), "A")
    print("A, one iteration: worst error / bound =", worst)
    assert (info["iterations"], info["converged"], info["pairs"], info["alignments"]) == (1, False, len(degree), K.case_a()["pid"].size)
    assert info["unique_pairs"] == sum(1 for d in degree.values() if d == 1)
    assert device()["map_us"] == 0


def test_degrees_around_a_wave_after_200_iterations():
    """A at 200 iterations against the float64 model (1e-9 / 1e-12), the counts exactly, the same bits from a second call"""
    N, info, Nm, im = _many("A/200", "A", 200)
    assert N.sum() == pytest.approx(im["pairs"], rel=1e-9) and im["pairs"] == 3 * len(K.A_DEGREES) + K.A_BIG
    assert device()["A/200 again"] == device()["A/200"]


# ---- B ---------------------------------------------------------------------------------------------------------------------------------
def test_chunk_edges_exactly():
    """B: contigs of 1, 255, 256, 257, 2047, 2048, 2049, 4096 and 4097 alignments (k_q_mpart's 256-thread tree and its chunks of
    Q_CHUNK = 2,048: one, one full, two, two full, three), contigs without placements first, last, between two others and adjacent
    (k_q_align's binary search over equal offsets, k_q_init).  Every pair has degree 1, so every r is w / w = 1.0 and N_c == m_c
    exactly, after one iteration and under the default stop rule, which then holds after the second iteration."""
    b = K.case_b()
    m = np.diff(b["offs"]).astype(np.int64)
    assert m.tolist() == list(K.B_SIZES) and m[0] == m[-1] == m[3] == 0 and m[6] == m[7] == 0 and m[2] and m[4]
    assert {K.Q_CHUNK - 1, K.Q_CHUNK, K.Q_CHUNK + 1, 2 * K.Q_CHUNK, 2 * K.Q_CHUNK + 1, 255, 256, 257, 1} <= set(m.tolist()) and m.max() > K.Q_CHUNK
    assert np.unique(b["pid"]).size == b["pid"].size and b["pid"].min() > 0 and b["pid"].max() < b["n_pairs"] - 1
    assert b["ins"].min() >= 50 and b["ins"].max() <= 360
    N1, i1 = _got("B/1")
    assert N1.tolist() == m.astype(np.float64).tolist() and (i1["iterations"], i1["converged"]) == (1, False)
    N2, i2 = _got("B/default")
    assert N2.tolist() == m.astype(np.float64).tolist() and i2["iterations"] <= 2 and i2["converged"]
    _, im = model_default("B")
    assert im["iterations"] == 2 == i2["iterations"]
    for info in (i1, i2):
        _counts_match(info, im, "B")
        assert info["pairs"] == info["unique_pairs"] == m.sum()


# ---- C ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C_SIZES)
def test_past_1024_contigs(n):
    """C: k_q_mfin is one workgroup of 1,024 threads, thread t takes the contigs t, t + 1024, ...: n = 1023, 1024, 1025 and 2049.  One
    pair of degree 1 on every contig but each 7th (these stay 0.0); five pairs of degree 2 with unequal inserts make the only contigs
    whose N moves: the two last ones (1023 | 1024 at n = 1025), indices of 1,024 and more only at n = 2049.  The degree-1 contigs are
    1.0 exactly, the others within the one-iteration bound of the exact model; under a tol between the model's delta_4 and delta_5 the
    device stops after iteration 5 like the model -- where a stop rule that saw only the contigs up to 1,023 would have stopped before."""
    c = K.case_c(n)
    pr, ct, ins = K.triples(c)
    m = np.bincount(ct, minlength=n)
    moving = np.array(c["moving"])
    still = np.setdiff1d(np.arange(n), moving)
    once = ct[np.bincount(pr)[pr] == 1]
    assert sorted(once.tolist()) == [c_ for c_ in range(n) if c_ % 7 != K.C_EMPTY] and np.bincount(pr).max() == 2
    assert m[K.C_EMPTY] == 0 and (m == 0).sum() >= n // 7 - 3                  # (contigs without a placement among the others)
    Nt, delta = trace_c(n)
    assert (Nt[0, still] == Nt[-1, still]).all() and (Nt[0, moving] != Nt[-1, moving]).all()          # exactly `moving` moves
    if n > K.Q_FIN:
        assert moving.max() >= K.Q_FIN and (n != 2049 or moving.min() >= K.Q_FIN)
        seen = np.array([np.max((np.abs(Nt[t] - Nt[t - 1]) / np.maximum(Nt[t], 1.0))[:K.Q_FIN]) for t in range(1, C_STOP - 1)])
        assert (seen < tolerances()["C"][str(n)]).any(), "a stop rule blind past contig 1,023 would not stop early"
    else:
        assert moving.tolist() == [n - 2, n - 1]
    N1, i1 = _got(f"C{n}/1")
    exact, degree = Q.quant_one_exact(pr, ct, ins, n, 360)
    assert N1[still].tolist() == [1.0 if m[c_] else 0.0 for c_ in still]
    T.assert_within_one_iteration_bound(N1, exact, T.one_iteration_bounds(c, degree), f"C{n}")
    assert i1["iterations"] == 1 and i1["pairs"] == len(degree)
    N, info = _got(f"C{n}/tol")
    assert (info["iterations"], info["converged"]) == (C_STOP, True)
    np.testing.assert_allclose(N, Nt[C_STOP - 1], rtol=1e-9, atol=1e-12)
    assert N[still].tolist() == N1[still].tolist()


# ---- D ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last_placed", [0, 1])
@pytest.mark.parametrize("n_pairs", D_PAIRS)
def test_pair_counts_around_the_scan_block(n_pairs, last_placed):
    """D: the degree scan over n_pairs = BLOCK - 1, BLOCK, BLOCK + 1 and 2 BLOCK + 1 ids of which every other one has degree zero, the
    last id placed or not (k_q_csr's seg[placed] = A comes from the scan's total); degrees 1 to 3 on five contigs, 50 iterations"""
    d = K.case_d(n_pairs, last_placed)
    ids = np.unique(d["pid"])
    assert (np.diff(ids) == 2).all() and (ids[-1] == n_pairs - 1) == bool(last_placed) and ids[-1] >= n_pairs - 2 and ids[0] <= 1
    assert set(np.bincount(d["pid"])[ids]) == {1, 2, 3}
    N, info, Nm, im = _many(f"D{n_pairs}/{last_placed}/50", f"D{n_pairs}/{last_placed}", 50)
    assert info["pairs"] == ids.size and N.sum() == pytest.approx(ids.size, rel=1e-9)


# ---- E ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", K.E_LENS)
def test_zero_weights(L):
    """E: inserts -5, 0, 49, 50, len, len + 1, 400, 401 and 32767 beside inserts inside the window, at len 49 (every weight is zero),
    50, 51, 360, 400, 401 and 4095: alone on a pair of degree 1 and in pairs of degree 3 of which two, one or none of the alignments
    weigh anything (none: the `sum > 0 ? ... : 0` arm of k_q_estep), neighbours by id.  Contig 0 has no placement."""
    e = K.case_e(L)
    pr, ct, ins = K.triples(e)
    weighs = (ins >= 50) & (ins <= min(400, L))
    per_pair = {int(p): (int(weighs[pr == p].sum()), int((pr == p).sum())) for p in np.unique(pr)}
    assert {1, 3} == {d for _, d in per_pair.values()} and e["offs"][1] == 0
    assert {-5, 0, 49, 50, L, L + 1, 400, 401, 32767} <= set(ins.tolist())
    if L >= 50:
        assert {(0, 3), (2, 3), (0, 1), (1, 1)} <= set(per_pair.values())
        assert any(w == 0 and d == 3 and per_pair[p - 2] == (1, 3) for p, (w, d) in per_pair.items())      # no weight at all, beside a pair with some
    else:
        assert not weighs.any()
    alive = sum(1 for w, _ in per_pair.values() if w)
    N1, i1 = _got(f"E{L}/1")
    Nm1, im1 = model(f"E{L}", 1)
    np.testing.assert_allclose(N1, Nm1, rtol=1e-9, atol=1e-12)
    N, info, Nm, im = _many(f"E{L}/50", f"E{L}", 50)
    assert info["unique_pairs"] == sum(1 for p, (w, d) in per_pair.items() if d == 1 and 50 <= ins[pr == p][0] <= 400)
    assert N.sum() == pytest.approx(alive, rel=1e-9) and N[0] == 0.0
    Nd, idef = _got(f"E{L}/default")
    Nmd, imd = model_default(f"E{L}")
    if L < 50:
        assert info["eff_len"] == 0.0 and alive == 0
        assert N1.tolist() == [0.0] * e["n"] and N.tolist() == [0.0] * e["n"] and Nd.tolist() == [0.0] * e["n"]
        assert (idef["iterations"], idef["converged"]) == (imd["iterations"], imd["converged"]) == (2, True)
    else:
        np.testing.assert_allclose(Nd, Nmd, rtol=1e-6, atol=1e-9)
        assert abs(idef["iterations"] - imd["iterations"]) <= 1 and idef["converged"] and imd["converged"]


# ---- F ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", T.F_ITERS)
def test_stop_flag_inside_and_across_the_batches(t):
    """F: the host queues Q_BATCH = 32 iterations between two looks at the flag k_q_mfin sets.  On case A a tol between the model's
    delta_(t-1) and delta_t (their geometric mean; the precondition is asserted in tests/test_quant_cpu.py) makes the run converge
    after iteration 2 (inside the first batch), 31, 32 (the batch's last), 33 (the first of the next), 64 and 65: the device reports
    exactly t, converged, and the model's N_t -- the iterations queued behind the flag left N alone, and the result came out of buffer
    t & 1.  (N_t is far from N_32 and N_64 at 1e-9 where t is neither: asserted there too.)"""
    assert any(x % K.Q_BATCH == 0 for x in T.F_ITERS) and any(x % K.Q_BATCH == 1 for x in T.F_ITERS) and {x & 1 for x in T.F_ITERS} == {0, 1}
    Nt, _ = T.trace_a()
    N, info = _got(f"F/tol{t}")
    assert (info["iterations"], info["converged"]) == (t, True), info
    np.testing.assert_allclose(N, Nt[t - 1], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("m", F_MAX_ITER)
def test_max_iter_inside_and_across_the_batches(m):
    """F: tol = 0 and max_iter = 1, 31, 32, 33 and 64: both parities of the result's buffer, a whole batch, a second batch of one
    iteration and two whole batches.  iterations == max_iter, not converged, the model's N at that iteration."""
    Nt, _ = T.trace_a()
    N, info = _got(f"F/max{m}")
    assert (info["iterations"], info["converged"]) == (m, False), info
    np.testing.assert_allclose(N, Nt[m - 1], rtol=1e-9, atol=1e-12)


# ---- G, H ------------------------------------------------------------------------------------------------------------------------------
def test_the_two_entries_give_the_same_bits():
    """G: vdjx_quant(S) and vdjx_quant_pairs over vdjx_map_emit(S)'s placements, S = e2e_mixed's contigs with their point variants and
    shifted windows: the same bits and the same info under the default stop rule and at 200 iterations; quant_map_us is 0 under
    vdjx_quant_pairs"""
    d = device()
    n, A, P = d["G/shape"]
    assert A > P > 0 and n > 1
    assert d["G/pairs"] == d["G/quant"] and d["G/pairs 200"] == d["G/quant 200"]
    assert d["G/pairs"]["info"]["alignments"] == A and d["G/pairs"]["info"]["pairs"] == P and d["G/pairs 200"]["info"]["iterations"] == 200
    assert d["G/pairs map_us"] == 0 and d["G/pairs placed"] == d["G/quant placed"] > 0


def test_refusals_empty_calls_and_nothing_kept():
    """H: every refusal of include/vdjx.h by its error text, n == 0, no placement at all, kept_device_bytes and kept_allocs unchanged
    across all calls of this file: the assertions run in the child (_device); here only that it ran to its end"""
    assert set(FIELDS) == set(device()["A/1"]["info"])
