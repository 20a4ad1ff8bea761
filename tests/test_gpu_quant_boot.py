"""vdjx_quant_boot / vdjx_quant_pairs_boot on the GPU: the batched, weighted EM of vdjer_amd/csrc/vdjx_quant.hip (k_qb_*) over the handmade
placements of tests/quant_cases.py, against the model of tests/quant_boot_model.py.

Tolerances.  One iteration: the bound of tests/test_quant_cpu.py with k raised by 1 for the product with the integer m (relative per contig
k u / (1 - k u), k = D_c + m_c + 11), against the exact rational model.  Many iterations: rtol 1e-9, atol 1e-12, fixed in
tests/test_quant_boot_cpu.py from the model's own spread under reordered sums.  Case B and the zeros: equality.

All device calls run in one child process with a time limit; every model result is computed once."""
import functools
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import golden_util as G
from tests import quant_boot_model as QB
from tests import quant_cases as K
from tests import test_quant_boot_cpu as TB
from tests import test_quant_cpu as T
from tests.scan_shapes import BLOCK
from tests.test_gpu_quant import _child_env, _context, _golden_contigs, _multi_set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1
C_SIZES = (1023, 1024, 1025, 2049)
D_PAIRS = (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
WAVE_B = (1, 63, 64, 65)
ZERO_CONTIG = 7                                                          # the contig of case A whose pairs get multiplicity 0
EDGE_ITERS = {"C": 12, "D": 50, "E": 50}                                 # as tests/test_quant_cpu.py's MANY runs them


@functools.lru_cache(maxsize=None)
def _cases():
    out = {"A": K.case_a(), "B": K.case_b()}
    out.update({f"C{n}": K.case_c(n) for n in C_SIZES})
    out.update({f"D{p}/{last}": K.case_d(p, last) for p in D_PAIRS for last in (0, 1)})
    out.update({f"E{L}": K.case_e(L) for L in K.E_LENS})
    rows = T._multi_set()
    rows = rows[np.argsort(rows[:, 1], kind="stable")]
    offs = np.zeros(5, np.uint64)
    offs[1:] = np.cumsum(np.bincount(rows[:, 1], minlength=4))
    out["M"] = dict(offs=offs, pid=rows[:, 0].astype(np.uint32), ins=rows[:, 2].astype(np.int16), n=4, L=360, n_pairs=11)
    return out


@functools.lru_cache(maxsize=None)
def ids_of(name):
    return QB.slots(_cases()[name]["pid"])


@functools.lru_cache(maxsize=None)
def mult_of(name, r, seed=SEED):
    return QB.draws(seed, r, ids_of(name).size)


@functools.lru_cache(maxsize=None)
def model_trace(name, r, iters):
    c = _cases()[name]
    return QB.trace(*K.triples(c), c["n"], c["L"], mult_of(name, r), iters)


def _given():
    """the multiplicities the `mult` tests hand over, by pair id"""
    a, b = _cases()["A"], _cases()["B"]
    pr, ct, _ = K.triples(a)
    zero = np.ones((2, a["n_pairs"]), np.uint32)
    zero[1] = 3
    zero[:, np.unique(pr[ct == ZERO_CONTIG])] = 0
    zero[:, 0] = 77                                                      # (an id without a placement: ignored)
    rng = np.random.default_rng(31)
    big = rng.integers(0, 1000, (2, b["n_pairs"])).astype(np.uint32)
    big[0, b["pid"][0]] = 1 << 31
    big[1, b["pid"][-1]] = (1 << 31) + 12345
    over = np.zeros((2, b["n_pairs"]), np.uint32)
    over[1, b["pid"][0]] = over[1, b["pid"][1]] = 1 << 31                # replicate 2 sums to 2^32
    return dict(ones=np.ones((2, a["n_pairs"]), np.uint32), zero=zero, big=big, over=over)


# ---- the device, once ----------------------------------------------------------------------------------------------------------------------
def _pack(res):
    out = dict(counts=res["counts"].tobytes().hex(), boot=res["boot"].tobytes().hex(), iterations=res["iterations"].tolist(), info=res["info"],
               boot_info=res["boot_info"])
    if "mult" in res:
        out["mult"] = res["mult"].tobytes().hex()
    return out


def _device(tol):
    import ctypes as C
    from vdjer_amd import _lib, api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    cases = _cases()
    given = _given()

    def run(name, **kw):
        c = cases[name]
        return ctx.quant_pairs_boot(c["offs"], (c["pid"], c["ins"]), c["L"], c["n_pairs"], **kw)

    def cells(v):
        if v is None:
            os.environ.pop("VDJX_QBOOT_CELLS", None)
        else:
            os.environ["VDJX_QBOOT_CELLS"] = str(v)

    cells(None)
    run("A", replicates=5, max_iter=2)                                   # (the workspace is there before the kept bytes are read)
    kept0, allocs0 = ctx.stat("kept_device_bytes"), ctx.stat("kept_allocs")
    out = {}
    a = cases["A"]
    N, info = ctx.quant_pairs(a["offs"], (a["pid"], a["ins"]), 360, a["n_pairs"])
    out["A/point"] = dict(counts=N.tobytes().hex(), info=info)
    out["A/default"] = _pack(run("A", replicates=2, seed=SEED))
    out["A/draws"] = _pack(run("A", replicates=3, seed=SEED, return_mult=True, max_iter=1, tol=0))
    out["A/1"] = _pack(run("A", replicates=5, seed=SEED, max_iter=1, tol=0))
    out["A/200"] = _pack(run("A", replicates=5, seed=SEED, max_iter=200, tol=0))
    per = int(info["pairs"]) + a["n"]
    for name, v in (("1", 1), ("2", 2 * per), ("2+", 3 * per - 1)):
        cells(v)
        out[f"A/200 batches of {name}"] = _pack(run("A", replicates=5, seed=SEED, max_iter=200, tol=0))
    cells(None)
    out["A/200 again"] = _pack(run("A", replicates=5, seed=SEED, max_iter=200, tol=0))
    for b in WAVE_B:
        out[f"M/{b}"] = _pack(run("M", replicates=b, seed=SEED, max_iter=50, tol=0))
    out["A/stop"] = _pack(run("A", replicates=TB.STOP_REPLICATES, seed=TB.STOP_SEED, tol=tol))
    out["A/ones"] = _pack(run("A", replicates=2, mult=given["ones"]))
    for m in (1, 20):
        out[f"A/zero/{m}"] = _pack(run("A", replicates=2, mult=given["zero"], return_mult=True, max_iter=m, tol=0))
    out["B/big"] = _pack(run("B", replicates=2, mult=given["big"], max_iter=3, tol=0))
    with pytest.raises(VdjxError, match=r"\(-1\).*multiplicities of replicate 2 sum to 4294967296"):
        run("B", replicates=2, mult=given["over"])
    for name in cases:
        if name[0] in "CDE":
            out[f"{name}/edge"] = _pack(run(name, replicates=2, seed=SEED, max_iter=EDGE_ITERS[name[0]], tol=0, return_mult=name[0] == "E"))

    # the empty calls
    e = ctx.quant_pairs_boot([0], (np.zeros(0, np.uint32), np.zeros(0, np.int16)), 360, 10, replicates=3, return_mult=True)
    assert e["boot"].shape == (3, 0) and e["iterations"].tolist() == [0, 0, 0] and not e["mult"].any()
    assert e["boot_info"] == dict(replicates=3, converged=3, batches=0, max_iterations=0, iterations=0) and e["info"]["converged"]
    e = ctx.quant_pairs_boot([0, 0, 0, 0], (np.zeros(0, np.uint32), np.zeros(0, np.int16)), 360, 0, replicates=4)
    assert e["boot"].tolist() == [[0.0] * 3] * 4 and e["counts"].tolist() == [0.0] * 3 and e["iterations"].tolist() == [0] * 4
    assert e["boot_info"] == dict(replicates=4, converged=4, batches=0, max_iterations=0, iterations=0)
    assert e["mean"].tolist() == e["sd"].tolist() == e["lower"].tolist() == e["upper"].tolist() == [0.0] * 3
    # refusals: the bootstrap's own, and vdjx_quant_pairs' through this entry
    off, pid, ins = np.array([0, 2, 3], np.uint64), np.array([1, 0, 6], np.uint32), np.array([100, 200, 300], np.int16)
    good = ctx.quant_pairs_boot(off, (pid, ins), 360, 7, replicates=2)
    assert good["info"]["pairs"] == 3 and good["boot"].shape == (2, 2) and good["boot_info"]["replicates"] == 2
    for kw, match in ((dict(replicates=0), r"\(-1\).*0 replicates \(1 \.\. 1024\)"), (dict(replicates=1025), r"\(-1\).*1025 replicates"),
                      (dict(replicates=-1), r"\(-1\).*-1 replicates"), (dict(offsets=[1, 2, 3]), r"\(-1\).*vdjx_quant_pairs_boot: offsets\[0\]=1 must be 0"),
                      (dict(offsets=[0, 4, 3]), r"\(-1\).*decrease at contig 1"), (dict(n_pairs=6), r"\(-1\).*placement 2 names pair 6 of 6"),
                      (dict(max_iter=0), r"\(-1\).*max_iter=0 must be at least 1"), (dict(tol=float("nan")), r"\(-1\).*tol must be >= 0"),
                      (dict(length=0), r"\(-1\).*len=0"), (dict(length=4096), r"\(-3\).*fewer than 4096 bases")):
        args = dict(dict(offsets=off, pairs=(pid, ins), length=360, n_pairs=7, replicates=2), **kw)
        with pytest.raises(VdjxError, match=match):
            ctx.quant_pairs_boot(**args)
    # (the raw call: NULL arguments, and replicates * n = 2^27, refused before anything is written)
    L, h = ctx.L, ctx.h
    info, binfo, prm = _lib.QuantInfo(), _lib.QuantBootInfo(), _lib.QuantParams(10, 1e-5)
    pk = np.zeros(3, api.PAIR_DTYPE)
    pk["pair_id"], pk["insert"] = pid, ins
    cnt, boot, iters = np.zeros(2), np.zeros((2, 2)), np.zeros(1024, np.uint32)
    ok = dict(h=h, off=api._p(off), pk=api._p(pk), prm=C.byref(prm), bprm=C.byref(_lib.QuantBootParams(2, 1)), cnt=api._p(cnt), info=C.byref(info),
              boot=api._p(boot), iters=api._p(iters), binfo=C.byref(binfo), n=2)

    def raw(**kw):
        a_ = dict(ok, **kw)
        return L.vdjx_quant_pairs_boot(a_["h"], a_["off"], a_["pk"], a_["n"], 360, 7, a_["prm"], a_["bprm"], None, None, a_["cnt"], a_["info"], a_["boot"],
                                       a_["iters"], a_["binfo"])

    assert raw() == 0 and info.pairs == 3 and binfo.replicates == 2
    for kw in (dict(h=None), dict(off=None), dict(prm=None), dict(bprm=None), dict(cnt=None), dict(info=None), dict(boot=None), dict(iters=None),
               dict(binfo=None)):
        assert raw(**kw) == -1 and b"vdjx_quant_pairs_boot: NULL argument" in L.vdjx_last_error(), kw
    wide = np.zeros((1 << 17) + 1, np.uint64)
    assert raw(off=api._p(wide), n=1 << 17, bprm=C.byref(_lib.QuantBootParams(1024, 1))) == -3 and b"fewer than 2^27 counts" in L.vdjx_last_error()
    # nothing is kept: scratch, the uploaded placements and multiplicities are the workspace's
    assert ctx.stat("kept_device_bytes") == kept0 and ctx.stat("kept_allocs") == allocs0
    ctx.close()

    # vdjx_quant_boot is map + the same function
    c = G.Case("e2e_mixed")
    ctx, p = _context(c.pool)
    _, seqs = _golden_contigs("e2e_mixed")
    S = _multi_set(seqs, c.clones)
    offs, pairs = ctx.map_emit(S)
    pairs = pairs.copy()
    out["G/pairs"] = _pack(ctx.quant_pairs_boot(offs, pairs, 360, c.pool.n_pairs, replicates=3, seed=9))
    out["G/boot"] = _pack(ctx.quant_boot(S, replicates=3, seed=9))
    N, info = ctx.quant(S)
    out["G/quant"] = dict(counts=N.tobytes().hex(), info=info)
    out["G/shape"] = [len(S), int(offs[-1]), int(np.unique(pairs["pair_id"]).size)]
    with pytest.raises(VdjxError, match=r"\(-1\).*vdjx_quant_boot: 0 replicates"):
        ctx.quant_boot(S, replicates=0)
    e = ctx.quant_boot([], replicates=2)
    assert e["boot"].shape == (2, 0) and e["boot_info"]["converged"] == 2
    p.free()
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def _child():
    """the child's exit status and output: it runs once, also when it fails"""
    tol = TB.boot_stop_tol()[0]
    code = f"import json; from tests.test_gpu_quant_boot import _device; print('QBOOT', json.dumps(_device({tol!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=_child_env("shipped"))
    return r.returncode, r.stdout, r.stderr


@functools.lru_cache(maxsize=None)
def device():
    rc, out, err = _child()
    assert rc == 0, (out[-3000:], err[-4000:])
    return json.loads(next(l for l in out.splitlines() if l.startswith("QBOOT ")).split(" ", 1)[1])


def _boot(key, n):
    d = device()[key]
    return np.frombuffer(bytes.fromhex(d["boot"]), np.float64).reshape(-1, n), d


def _mult(key, n_pairs):
    return np.frombuffer(bytes.fromhex(device()[key]["mult"]), np.uint32).reshape(-1, n_pairs)


def _one_iteration_bounds(case, degree):
    """tests/test_quant_cpu.py's bound with k raised by 1"""
    pr, ct, _ = K.triples(case)
    d = np.array([degree[int(p)] for p in pr], np.int64)
    out = np.zeros(case["n"])
    for c in np.unique(ct):
        k = int(d[ct == c].max()) + int((ct == c).sum()) + 11
        out[c] = k * T.U / (1.0 - k * T.U)
    return out


def _many(got, want, what):
    np.testing.assert_allclose(got, want, rtol=TB.MANY_RTOL, atol=TB.MANY_ATOL, err_msg=what)


# ---- the point estimate, the draws -------------------------------------------------------------------------------------------------------
def test_point_estimate_is_quant_pairs_bit_for_bit():
    d = device()
    assert d["A/default"]["counts"] == d["A/point"]["counts"] and d["A/default"]["info"] == d["A/point"]["info"]
    assert d["A/200"]["info"]["iterations"] == 200 and d["A/200"]["counts"] != d["A/point"]["counts"]
    assert d["A/default"]["boot_info"]["converged"] == 2 and d["A/default"]["boot_info"]["batches"] == 1


def test_draws_are_the_models():
    a = K.case_a()
    m = _mult("A/draws", a["n_pairs"])
    ids = ids_of("A")
    assert m.shape == (3, a["n_pairs"])
    for r in (1, 2, 3):
        assert np.array_equal(m[r - 1], QB.mult_by_id(mult_of("A", r), ids, a["n_pairs"])), r
        assert int(m[r - 1].sum()) == ids.size and not m[r - 1][np.setdiff1d(np.arange(a["n_pairs"]), ids)].any()


# ---- values --------------------------------------------------------------------------------------------------------------------------------
def test_one_iteration_against_the_exact_weighted_model():
    """A at B = 5: whole-wave pairs of 33 to 100 alignments, a contig of 4,097 alignments (nine chunks of the boot M step), pairs across
    a workgroup boundary; every replicate within the one-iteration bound (k + 1) of the exact rational model"""
    T.test_case_a_is_on_the_edges_it_names()
    a = K.case_a()
    boot, d = _boot("A/1", 101)
    assert boot.shape == (5, 101) and d["iterations"] == [1] * 5 and d["boot_info"]["converged"] == 0
    for r in range(1, 6):
        exact, degree = QB.one_exact(*K.triples(a), 101, 360, mult_of("A", r))
        worst = T.assert_within_one_iteration_bound(boot[r - 1], exact, _one_iteration_bounds(a, degree), f"A, replicate {r}")
        print("A, one iteration, replicate", r, ": worst error / bound =", worst)
        assert sum(exact) == Fraction(int(mult_of("A", r).sum()))


def test_200_iterations_against_the_model():
    boot, d = _boot("A/200", 101)
    assert d["iterations"] == [200] * 5 and d["boot_info"] == dict(replicates=5, converged=0, batches=1, max_iterations=200, iterations=1000)
    for r in range(1, 6):
        _many(boot[r - 1], model_trace("A", r, 200)[0][-1], f"A/200 replicate {r}")
    assert len({boot[r].tobytes() for r in range(5)}) == 5


def test_bits_do_not_depend_on_the_batches():
    d = device()
    want = d["A/200"]["boot"]
    assert [d[f"A/200 batches of {k}"]["boot_info"]["batches"] for k in ("1", "2", "2+")] == [5, 3, 3]
    for k in ("batches of 1", "batches of 2", "batches of 2+", "again"):
        assert d[f"A/200 {k}"]["boot"] == want and d[f"A/200 {k}"]["iterations"] == [200] * 5, k
        assert d[f"A/200 {k}"]["counts"] == d["A/200"]["counts"]


def test_replicate_counts_around_a_wave():
    """B = 1, 63, 64 and 65 (a tile of one lane, a tile short of a wave, a whole wave, a wave and one lane): replicate r has the same
    bytes whatever B, and is the model's"""
    full, d = _boot(f"M/{WAVE_B[-1]}", 4)
    assert full.shape == (65, 4)
    for b in WAVE_B[:-1]:
        got, _ = _boot(f"M/{b}", 4)
        assert got.shape == (b, 4) and got.tobytes() == full[:b].tobytes(), b
    for r in range(1, 66):
        _many(full[r - 1], model_trace("M", r, 50)[0][-1], f"M replicate {r}")
        assert full[r - 1].sum() == pytest.approx(11.0, rel=1e-9) and full[r - 1][3] == 0.0


def test_stop_flags_per_replicate():
    """case A, four replicates, the tol of tests/test_quant_boot_cpu.py: every replicate stops at the model's iteration, below and above
    the Q_BATCH = 32 iterations the host queues between two looks, and keeps the N of that iteration"""
    tol, its = TB.boot_stop_tol()
    boot, d = _boot("A/stop", 101)
    assert d["iterations"] == its and min(its) < K.Q_BATCH < max(its)
    assert d["boot_info"] == dict(replicates=4, converged=4, batches=1, max_iterations=max(its), iterations=sum(its))
    for r, t in zip(range(1, 5), its):
        _many(boot[r - 1], TB.trace_a(TB.STOP_SEED, r, 120)[0][t - 1], f"stop, replicate {r}")


# ---- given multiplicities ---------------------------------------------------------------------------------------------------------------------
def test_multiplicities_of_one_give_the_point_estimate():
    boot, d = _boot("A/ones", 101)
    point = np.frombuffer(bytes.fromhex(device()["A/point"]["counts"]), np.float64)
    for r in range(2):
        _many(boot[r], point, "ones")
    assert d["iterations"] == [device()["A/point"]["info"]["iterations"]] * 2 and d["boot_info"]["converged"] == 2


@pytest.mark.parametrize("m", [1, 20])
def test_a_contig_whose_pairs_have_multiplicity_zero(m):
    a = K.case_a()
    pr, ct, _ = K.triples(a)
    given = _given()["zero"]
    boot, d = _boot(f"A/zero/{m}", 101)
    used = _mult(f"A/zero/{m}", a["n_pairs"])
    ids = ids_of("A")
    assert np.array_equal(used[:, ids], given[:, ids]) and not used[:, 0].any()        # (id 0 has no placement: its 77 is ignored)
    assert (ct == ZERO_CONTIG).sum() > 0
    for r in range(2):
        assert boot[r][ZERO_CONTIG] == 0.0
        assert boot[r].sum() == pytest.approx(float(given[r, ids].sum()), rel=1e-12)


def test_multiplicities_up_to_2_31_exactly():
    b = K.case_b()
    pr, ct, _ = K.triples(b)
    given = _given()["big"]
    boot, d = _boot("B/big", b["n"])
    assert given.max() > 1 << 31 and d["iterations"] == [3, 3]
    for r in range(2):
        want = np.bincount(ct, weights=given[r, pr].astype(np.float64), minlength=b["n"])
        assert boot[r].tolist() == want.tolist()


# ---- other edges ---------------------------------------------------------------------------------------------------------------------------
def _edge(name):
    c = _cases()[name]
    boot, d = _boot(f"{name}/edge", c["n"])
    iters = EDGE_ITERS[name[0]]
    assert boot.shape == (2, c["n"]) and d["iterations"] == [iters] * 2
    for r in (1, 2):
        _many(boot[r - 1], model_trace(name, r, iters)[0][-1], f"{name} replicate {r}")
    return c, boot


@pytest.mark.parametrize("n", C_SIZES)
def test_past_1024_contigs(n):
    c, boot = _edge(f"C{n}")
    assert (boot[:, K.C_EMPTY] == 0.0).all() and boot.shape[1] == n


@pytest.mark.parametrize("last_placed", [0, 1])
@pytest.mark.parametrize("n_pairs", D_PAIRS)
def test_pair_counts_around_the_scan_block(n_pairs, last_placed):
    c, boot = _edge(f"D{n_pairs}/{last_placed}")
    assert boot.sum(axis=1) == pytest.approx([float(ids_of(f"D{n_pairs}/{last_placed}").size)] * 2, rel=1e-9)


@pytest.mark.parametrize("L", K.E_LENS)
def test_zero_weights(L):
    """pairs all of whose alignments weigh zero add nothing whatever their multiplicity: the counts sum to the multiplicities of the rest"""
    c, boot = _edge(f"E{L}")
    pr, ct, ins = K.triples(c)
    weighs = (ins >= 50) & (ins <= min(400, L))
    ids = ids_of(f"E{L}")
    alive = np.array([weighs[pr == p].any() for p in ids])
    used = _mult(f"E{L}/edge", c["n_pairs"])
    for r in (1, 2):
        assert np.array_equal(used[r - 1][ids], mult_of(f"E{L}", r))
        assert boot[r - 1].sum() == pytest.approx(float(mult_of(f"E{L}", r)[alive].sum()), rel=1e-9)
        assert boot[r - 1][0] == 0.0
    if not alive.any():
        assert not boot.any()
    else:
        assert (~alive).any() and mult_of(f"E{L}", 1)[~alive].sum() > 0


# ---- the two entries, refusals ---------------------------------------------------------------------------------------------------------------
def test_the_two_entries_give_the_same_bits():
    d = device()
    n, A, P = d["G/shape"]
    assert A > P > 0 and n > 1
    assert d["G/pairs"] == d["G/boot"]
    assert d["G/boot"]["counts"] == d["G/quant"]["counts"] and d["G/boot"]["info"] == d["G/quant"]["info"]
    assert d["G/boot"]["boot_info"]["replicates"] == 3 and len(set(d["G/boot"]["iterations"])) >= 1 and min(d["G/boot"]["iterations"]) >= 1


def test_refusals_empty_calls_and_nothing_kept():
    """every refusal by its error text, n == 0, no placement at all, kept_device_bytes and kept_allocs unchanged across all calls of this
    file: the assertions run in the child (_device); here only that it ran to its end"""
    assert "G/quant" in device()
