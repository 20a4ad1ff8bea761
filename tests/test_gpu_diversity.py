"""vdjx_diversity on the GPU against the model of tests/diversity_model.py: the counts exactly, the Hill numbers to a derived tolerance.

Shapes (the smallest at which the kernels can go wrong): one clone; weights (1, 1, 1) at N = 12, every t on a boundary of cum; zero weights
first, last and adjacent; W > 2^32; N = 1; N = 100,003 with B = 7, odd against every tile; C = 300 in LDS and with VDJX_DIV_LDS_CLONES=0;
C = 5,000 (a coarse table with a stride, 20 tiles of the Hill pass) in one batch and with VDJX_DIV_CELLS=10000 in four, the last of one
replicate; C = 20,000, past the LDS histogram by default; seeds 0 and 2^64 - 1; Q = 1 and the 41-order grid; counts=False.

Tolerances.  d and observed, relative: M.rel_tol(q, m), m the clones drawn in the replicate (of weight, for observed).  mean, relative: the
largest of its replicates' tolerances (a mean of positive numbers each within tol is within tol) plus (B + 2) eps for its own B
additions and the division.  sd: a RELATIVE bound on sd itself cannot be derived from relative bounds on d (sd is a difference of numbers
a thousand times its size where the replicates agree to three digits), so sd is held to the absolute bound that can: sd is the norm
of the centred d over sqrt(B - 1), so a perturbation of at most delta per replicate moves it by at most sqrt(B / (B - 1)) delta <= 2
delta, delta = (tol + (B + 4) eps) max d.  Where q = 0 every d is an integer and mean and sd are equal bits.
mean and sd are also recomputed from the device's own d in the header's order, at 1e-12.

Then `vdjer --quant --lineages --diversity` on the e2e_families and e2e_mixed goldens against the model's table.  The API cases run in
two child processes that set the two variables themselves; every model result is computed once."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import annot_model as A
from tests import diversity_model as M
from tests import families as F
from tests import quant_model as Q
from tests.test_gpu_annot import _child_env, _vdjer as _vdjer_e2e, _write_inputs
from tests.test_gpu_tables import _sha, _vdjer as _vdjer_families

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = None                                                              # q=None: the 41 orders
FEW = [0.0, 0.5, 1.0, 2.0, 16.0]
KNOBS = {"c300/global": ("c300", dict(VDJX_DIV_LDS_CLONES="0")), "c5000/global": ("c5000", dict(VDJX_DIV_LDS_CLONES="0")),
         "c5000/batches": ("c5000", dict(VDJX_DIV_CELLS="10000")), "c5000/cell": ("c5000", dict(VDJX_DIV_CELLS="1")),
         "c20000/lds_off_is_the_same": ("c20000", dict(VDJX_DIV_LDS_CLONES="0"))}


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_diversity import {fn}; print('DIVERSITY', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("DIVERSITY ")).split(" ", 1)[1])


# ---- the cases: name -> (weight, N, q, replicates, seed) --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261)
    zipf = lambda C: [int(x) for x in np.maximum(1, (1e6 / np.arange(1, C + 1) ** 1.1)).astype(np.int64) * rng.integers(1, 4, C)]      # noqa: E731
    w50 = [int(x) for x in rng.integers(0, 1000, 50)]
    c300 = zipf(300)
    for k in (0, 17, 18, 299):
        c300[k] = 0
    return {
        "one_clone": ([9], 77, GRID, 3, 1),
        "boundaries": ([1, 1, 1], 12, GRID, 2, 1),
        "zero_weights": ([0, 5, 0, 0, 7, 0], 1000, GRID, 3, 1),
        "wide": ([1, 1 << 45], 2000, GRID, 3, 1),
        "wide_both": ([(1 << 45) + 12345, 1 << 44, 3 << 43], 2000, FEW, 2, 9),
        "one_draw": ([3, 1, 4, 1, 5], 1, GRID, 4, 1),
        "odd": ([int(x) for x in rng.integers(1, 100000, 37)], 100003, GRID, 7, 1),
        "c300": (c300, 20011, GRID, 3, 1),
        "c5000": (zipf(5000), 30000, FEW, 7, 1),
        "c20000": (zipf(20000), 50000, [0.0, 1.0, 2.0], 2, 1),
        "seed_0": (w50, 5000, FEW, 2, 0),
        "seed_max": (w50, 5000, FEW, 2, M.M64),
        "one_order": (w50, 5000, [2.0], 3, 1),
    }


@functools.lru_cache(maxsize=None)
def models():
    return {name: M.diversity(w, N, q, b, seed) for name, (w, N, q, b, seed) in cases().items()}


def _pack(res):
    return dict(observed=res["observed"].tolist(), mean=res["mean"].tolist(), sd=res["sd"].tolist(), d=res["d"].tolist(),
                d_hex=res["d"].tobytes().hex(), counts=None if res["counts"] is None else res["counts"].tolist(),
                dtype=None if res["counts"] is None else str(res["counts"].dtype), info=res["info"])


def _device(_):
    import ctypes as C
    from vdjer_amd import _lib, api
    from vdjer_amd._lib import VdjxError
    for k in ("VDJX_DIV_CELLS", "VDJX_DIV_LDS_CLONES"):
        os.environ.pop(k, None)
    ctx = api.Context(0)
    ctx.diversity([1, 2], 10, replicates=1)                             # (the workspace is there before the kept bytes are read)
    kept0, allocs0 = ctx.stat("kept_device_bytes"), ctx.stat("kept_allocs")
    out = dict(cases={}, stat={}, dispatches={})
    for name, (w, N, q, b, seed) in cases().items():
        ctx.profile(True)
        ctx.profile_reset()
        res = ctx.diversity(w, N, q, b, seed, counts=True)
        out["dispatches"][name] = {k: v[1] for k, v in ctx.profile_get().items()}
        ctx.profile(False)
        out["stat"][name] = ctx.stat("diversity_batches")
        again = ctx.diversity(w, N, q, b, seed, counts=True)              # the same settings called twice give the same bits
        for f in ("observed", "mean", "sd", "d", "counts"):
            assert again[f].tobytes() == res[f].tobytes(), (name, f)
        assert again["info"] == res["info"], name
        out["cases"][name] = _pack(res)
    assert ctx.stat("kept_device_bytes") == kept0 and ctx.stat("kept_allocs") == allocs0      # scratch is the workspace's: nothing is kept
    w, N, q, b, seed = cases()["c300"]
    plain = ctx.diversity(w, N, q, b, seed)                              # counts=False
    assert plain["counts"] is None
    out["no_counts"] = _pack(plain)
    out["defaults"] = ctx.diversity([5, 7], 10)["info"]
    # no clone; refusals: vdjx_last_error names the rule
    r0 = ctx.diversity([], 10, [2.0], 3, 1, counts=True)
    assert r0["info"] == dict.fromkeys(M.FIELDS, 0) and r0["counts"].shape == (3, 0)
    good = [3, 1, 4]
    for w, match in (([0, 0, 0], "weight 0"), ([1 << 62, 1 << 62], "2\\^63"), ([1 << 63], "2\\^63"), (np.ones(1 << 20, np.uint64), "2\\^20")):
        with pytest.raises(VdjxError, match=match):
            ctx.diversity(w, 10, [2.0], 2, 1)
    assert ctx.diversity([(1 << 63) - 1], 10, [2.0], 2, 1)["info"]["weight"] == (1 << 63) - 1
    for b in (0, 4097, 4000000000):
        with pytest.raises(VdjxError, match="replicates"):
            ctx.diversity(good, 10, [2.0], b, 1)
    for n in (0, 1 << 31, (1 << 32) - 1):
        with pytest.raises(VdjxError, match="depth"):
            ctx.diversity(good, n, [2.0], 2, 1)
    for q in ([], [0.1] * 65):
        with pytest.raises(VdjxError, match="orders"):
            ctx.diversity(good, 10, q, 2, 1)
    assert ctx.diversity(good, 10, [0.1 * k for k in range(64)], 1, 1)["d"].shape == (1, 64)
    for bad in (float("nan"), -0.5, -1e-300, 16.5, float("inf")):
        with pytest.raises(VdjxError, match="order 1 is"):
            ctx.diversity(good, 10, [2.0, bad], 2, 1)
    for bad in (1.01, 0.99, 1.0 + 2.0 ** -52, 1.0 - 1.0 / 64.0 + 1e-9):
        with pytest.raises(VdjxError, match="within 1/64 of 1"):
            ctx.diversity(good, 10, [bad], 2, 1)
    assert ctx.diversity(good, 10, [1.0 - 1.0 / 64.0, 1.0, 1.0 + 1.0 / 64.0, 16.0], 2, 1)["d"].shape == (2, 4)
    # the raw call: a NULL among the required pointers; info is zeroed first
    Lb, h = ctx.L, ctx.h
    info = _lib.DiversityInfo()
    params = _lib.DiversityParams(2, 10, 1)
    w3, q1 = np.array(good, np.uint64), np.array([2.0])
    o = [np.zeros(1), np.zeros(2), np.zeros(1), np.zeros(1)]             # observed, d, mean, sd

    def raw(weight=w3, q=q1, par=params, outs=None, inf=info):
        outs = list(o) if outs is None else outs
        return Lb.vdjx_diversity(h, api._p(weight), 3, api._p(q), 1, C.byref(par) if par is not None else None, *[api._p(x) for x in outs], None,
                                 C.byref(inf) if inf is not None else None)

    for kw, word in ((dict(weight=None), b"NULL"), (dict(q=None), b"NULL"), (dict(par=None), b"NULL"), (dict(outs=[None] + o[1:]), b"out_observed"),
                     (dict(outs=[o[0], None] + o[2:]), b"out_d"), (dict(outs=o[:2] + [None, o[3]]), b"out_mean"), (dict(outs=o[:3] + [None]), b"out_sd")):
        info.clones = 99
        assert raw(**kw) == -1 and b"NULL" in Lb.vdjx_last_error() and word in Lb.vdjx_last_error() and info.clones == 0, kw
    assert raw(inf=None) == 0 and raw() == 0 and [getattr(info, f) for f in M.FIELDS] == [3, 3, 8, 10, 2, 1, M.PATH_LDS]
    info.batches = 5
    rc = Lb.vdjx_diversity(h, None, 0, None, 0, None, None, None, None, None, None, C.byref(info))      # C = 0 returns at once
    assert rc == 0 and [getattr(info, f) for f in M.FIELDS] == [0] * 7
    ctx.close()
    return out


def _device_knobs(_):
    """the KNOBS cases, each under its own setting of the two variables (they are read per call)"""
    from vdjer_amd import api
    ctx = api.Context(0)
    out = {}
    for key, (name, env) in KNOBS.items():
        for k in ("VDJX_DIV_CELLS", "VDJX_DIV_LDS_CLONES"):
            os.environ.pop(k, None)
        os.environ.update(env)
        w, N, q, b, seed = cases()[name]
        ctx.profile(True)
        ctx.profile_reset()
        res = _pack(ctx.diversity(w, N, q, b, seed, counts=True))
        res["dispatches"] = {k: v[1] for k, v in ctx.profile_get().items()}
        ctx.profile(False)
        res["stat"] = ctx.stat("diversity_batches")
        out[key] = res
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def device():
    return _run_child("_device", "x", _child_env("shipped"))


@functools.lru_cache(maxsize=None)
def device_knobs():
    return _run_child("_device_knobs", "x", _child_env("shipped"))


def _close(got, want, rel, what, extra_abs=0.0):
    assert abs(got - want) <= rel * abs(want) + extra_abs, (what, got, want, abs(got - want) / abs(want) if want else None, rel)


def _same(dev, name, what=None):
    """counts exactly; observed, d, mean, sd to the tolerances of the module's docstring; mean and sd again from the device's own d"""
    what = what or name
    w, N, q, b, seed = cases()[name]
    q = M.orders() if q is None else q
    mod = models()[name]
    assert dev["dtype"] == "uint32" and np.array_equal(np.asarray(dev["counts"], np.int64), mod["counts"]), what
    assert dev["info"] == dict(mod["info"], batches=dev["info"]["batches"], path=dev["info"]["path"]), (what, dev["info"], mod["info"])
    drawn = (mod["counts"] > 0).sum(axis=1).tolist()
    weighted = mod["info"]["weighted"]
    for j, x in enumerate(q):
        _close(dev["observed"][j], mod["observed"][j], M.rel_tol(x, weighted), (what, "observed", x))
        tols = [M.rel_tol(x, m) for m in drawn]
        for r in range(b):
            _close(dev["d"][r][j], mod["d"][r][j], tols[r], (what, "d", r, x))
        tol = max(tols)
        _close(dev["mean"][j], mod["mean"][j], tol + (b + 2) * M.EPS if tol else 0.0, (what, "mean", x))
        delta = (tol + (b + 4) * M.EPS) * max(abs(v) for v in mod["d"][:, j]) if tol else 0.0
        _close(dev["sd"][j], mod["sd"][j], 0.0, (what, "sd", x), extra_abs=2.0 * delta)
    mean, sd = M.mean_sd(dev["d"])
    for j in range(len(q)):
        _close(dev["mean"][j], mean[j], 1e-12, (what, "mean of the device's d", j))
        _close(dev["sd"][j], sd[j], 1e-12, (what, "sd of the device's d", j))
    return mod


def _case(name):
    mod = _same(device()["cases"][name], name)
    dev = device()["cases"][name]
    assert dev["info"] == mod["info"] and device()["stat"][name] == mod["info"]["batches"], (name, dev["info"], mod["info"])
    # a batch is one draw dispatch and one each of the Hill kernels, which ran once more for `observed`: whatever B, C and N are
    nb = mod["info"]["batches"]
    assert device()["dispatches"][name] == {"k_div_draw": nb, "k_div_hill": nb + 1, "k_div_fin": nb + 1}, (name, device()["dispatches"][name])
    return mod


def test_one_clone():
    mod = _case("one_clone")
    assert mod["counts"].tolist() == [[77]] * 3 and (mod["d"] == 1.0).all() and np.asarray(device()["cases"]["one_clone"]["d"]).tolist() == mod["d"].tolist()


def test_every_t_on_a_boundary_of_cum():
    mod = _case("boundaries")
    assert mod["counts"][0].tolist() == [3, 4, 5] and mod["observed"] == pytest.approx([3.0] * 41, rel=1e-13)      # equal weights: C at every order


def test_zero_weights_first_last_and_adjacent():
    mod = _case("zero_weights")
    assert mod["counts"][0].tolist() == [0, 405, 0, 0, 595, 0] and mod["info"]["weighted"] == 2 and (mod["counts"][:, [0, 2, 3, 5]] == 0).all()


def test_total_weight_past_32_bits():
    assert _case("wide")["info"]["weight"] == (1 << 45) + 1
    mod = _case("wide_both")
    assert mod["info"]["weight"] > 1 << 46 and (mod["counts"] > 0).all()


def test_one_draw():
    mod = _case("one_draw")
    assert (mod["counts"].sum(axis=1) == 1).all() and (mod["d"] == 1.0).all() and mod["sd"].tolist() == [0.0] * 41


def test_odd_depth_and_replicates():
    mod = _case("odd")
    assert (mod["counts"].sum(axis=1) == 100003).all() and mod["d"].shape == (7, 41) and (mod["sd"][1:] > 0).all()


def test_seeds_at_both_ends():
    a, b = _case("seed_0"), _case("seed_max")
    assert a["counts"].tolist() != b["counts"].tolist()


def test_one_order_and_counts_not_asked_for():
    mod = _case("one_order")
    assert mod["d"].shape == (3, 1)
    plain, full = device()["no_counts"], device()["cases"]["c300"]
    assert plain["counts"] is None and plain["d_hex"] == full["d_hex"] and plain["info"] == full["info"]
    assert all(plain[f] == full[f] for f in ("observed", "mean", "sd"))
    assert device()["defaults"] == dict(clones=2, weighted=2, weight=12, depth=10, replicates=200, batches=1, path=M.PATH_LDS)


def test_lds_and_global_histograms_give_the_same_bits():
    mod = _case("c300")
    assert mod["info"]["path"] == M.PATH_LDS and mod["info"]["weighted"] == 296
    for key in ("c300/global", "c5000/global"):
        name = KNOBS[key][0]
        _case(name)
        got, want = device_knobs()[key], device()["cases"][name]
        assert got["info"] == dict(want["info"], path=M.PATH_GLOBAL) and want["info"]["path"] == M.PATH_LDS, key
        assert got["counts"] == want["counts"] and got["d_hex"] == want["d_hex"], key


def test_past_the_lds_histogram_by_default():
    mod = _case("c20000")
    assert mod["info"]["path"] == M.PATH_GLOBAL and mod["info"]["clones"] == 20000 > M.LDS_CLONES
    got = device_knobs()["c20000/lds_off_is_the_same"]
    assert got["counts"] == device()["cases"]["c20000"]["counts"] and got["d_hex"] == device()["cases"]["c20000"]["d_hex"]


def test_several_batches_give_the_same_bits():
    want = device()["cases"]["c5000"]
    assert _case("c5000")["info"]["batches"] == 1
    for key, batches in (("c5000/batches", 4), ("c5000/cell", 7)):       # 10,000 cells: two replicates of 5,000 a batch, the last of one
        got = device_knobs()[key]
        assert got["info"] == dict(want["info"], batches=batches) and got["stat"] == batches, (key, got["info"])
        assert got["counts"] == want["counts"] and got["d_hex"] == want["d_hex"] and got["observed"] == want["observed"], key
        assert got["dispatches"] == {"k_div_draw": batches, "k_div_hill": batches + 1, "k_div_fin": batches + 1}, key
        w, N, q, b, seed = cases()["c5000"]
        assert M.diversity([1] * 5000, 1, [0.0], b, seed, cells=int(KNOBS[key][1]["VDJX_DIV_CELLS"]))["info"]["batches"] == batches


# ---- vdjer --quant --lineages --diversity ------------------------------------------------------------------------------------------------
BOOT = ["--diversity-boot", "16", "--diversity-depth", "5000"]
SUMMARY = re.compile(r"diversity: (\d+) lineages with weight of (\d+), (\d+\.\d\d) expected pairs, depth (\d+), (\d+) replicates \(seed (\d+)\), "
                     r"richness (\d+\.\d\d), shannon (\d+\.\d{4}), simpson (\d+\.\d{4}), (\d+) batches")


def _check_run(d, lines, plain, seed):
    """the run's own tables -> the model's inputs -> the model's table, cell by cell"""
    from vdjer_amd import annot
    head, q = Q.read_table(d / "q.tsv")
    lhead, lrows = A.read_table(d / "l.tsv")
    assert head == Q.HEADER and lhead[1] == "clone_id" and lhead[-1] == "clone_expected_count" and [r[0] for r in lrows] == [r[0] for r in q]
    clone = [int(r[1][4:]) - 1 if r[1] else -1 for r in lrows]
    cells = [r[4] for r in q]
    weight, numbers = M.weights(clone, cells)
    w2, n2 = annot.diversity_weights(clone, cells)
    assert w2.tolist() == weight and n2 == numbers
    printed = {clone[c]: r[-1] for c, r in enumerate(lrows) if clone[c] >= 0}      # the lineage table's own sums, as printed
    assert [M.hundredths(printed[k]) for k in numbers] == weight and all(M.hundredths(v) == 0 for k, v in printed.items() if k not in numbers)
    n_lineages = len(set(clone) - {-1})
    text = (d / "d.tsv").read_text()
    rows = [l.split("\t") for l in text.split("\n")[:-1]]
    assert rows[0] == M.COLUMNS and text.endswith("\n")
    m = SUMMARY.fullmatch(lines[-1])                                     # the line follows all other summary lines
    assert m, lines[-3:]
    if not weight:
        assert len(rows) == 1 and lines[-1] == M.summary_line(n_lineages, weight, 5000, 16, seed, None, 0)
    else:
        mod = M.diversity(weight, 5000, None, 16, seed)
        want = M.table_rows(M.orders(), mod["observed"], mod["mean"], mod["sd"])
        assert len(rows) == 42 and [r[0] for r in rows[1:]] == [r[0] for r in want]
        for got, exp in zip(rows[1:], want):
            assert all(re.fullmatch(r"\d+\.\d{4}", cell) for cell in got[1:]), got
            for a, b, col in zip(got[1:], exp[1:], M.COLUMNS[1:]):
                assert abs(float(a) - float(b)) <= 1.5e-4, (got[0], col, a, b)
        want_line = M.summary_line(n_lineages, weight, 5000, 16, seed, mod["mean"], 1)
        mw = SUMMARY.fullmatch(want_line)
        assert [m.group(k) for k in (1, 2, 3, 4, 5, 6, 10)] == [mw.group(k) for k in (1, 2, 3, 4, 5, 6, 10)], (lines[-1], want_line)
        assert abs(float(m.group(7)) - float(mw.group(7))) <= 0.015 and all(abs(float(m.group(k)) - float(mw.group(k))) <= 1.5e-4 for k in (8, 9))
    # without --diversity: the same lineages and quant tables, byte for byte, and no line
    plain_d, plain_lines = plain
    assert not any(l.startswith("diversity: ") for l in plain_lines) and not (plain_d / "d.tsv").exists()
    for fn in ("q.tsv", "l.tsv"):
        assert _sha(d / fn) == _sha(plain_d / fn), fn
    return weight


def test_vdjer_cli_diversity_families(tmp_path):
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    env = _child_env("shipped")
    tables = ["--quant", "q.tsv", "--lineages", "l.tsv"]
    d, lines = _vdjer_families(tmp_path, "div", tables + ["--diversity", "d.tsv", "--diversity-seed", "7"] + BOOT, env)      # (FASTA, SAM and dot: the golden's)
    plain = _vdjer_families(tmp_path, "plain", tables, env)
    weight = _check_run(d, lines, plain, 7)
    assert len(weight) >= 40                                            # the golden has lineages to speak of


def test_vdjer_cli_diversity_mixed(tmp_path):
    env = _child_env("shipped")
    tables = ["--quant", "q.tsv", "--lineages", "l.tsv"]
    runs = {}
    for name, extra in (("div", ["--diversity", "d.tsv"] + BOOT), ("plain", [])):
        d = tmp_path / name
        d.mkdir()
        _write_inputs("e2e_mixed", str(d))
        r = _vdjer_e2e(d, "e2e_mixed", tables + extra, env)              # (FASTA, SAM and dot: the golden's)
        runs[name] = (d, r.stderr.splitlines())
    _check_run(*runs["div"], runs["plain"], 1)                          # the seed's default is 1
