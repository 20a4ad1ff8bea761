"""vdjx_lineage_threshold on the GPU: the histogram, the density row, the peak counts of every bandwidth and every info field against the
model of tests/threshold_model.py, exactly, for every case of tests/threshold_cases.py under the default and one other parameter set, each
called twice (two calls give the same bits); the multiply-add count; the dispatches; the refusals, after each of which the context still
works; and vdjx_lineage -> vdjx_lineage_threshold on junctions built from a case, so that the distances come from the device.  The calls
run in one child process (as tests/test_gpu_lineage_dist.py runs its own); every model result is computed once."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import threshold_cases as TC
from tests import threshold_model as M
from tests.test_gpu_annot import _child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(TC.cases("default"))
DISPATCHES = {"k_thr_hist": 1, "k_thr_number": 1, "k_thr_compact": 1, "k_thr_density": 1, "k_thr_peaks": 1}
DISPATCH_CASES = ("one_bin", "sampler_80", "largest_bin", "every_bin")
MACS_CASES = ("grid_ends", "sampler_80", "valley_on_guard")
CHAINED = "sampler_80"


def chained_junctions():
    """junctions whose nearest distances are the chained case's: an item at distance d of length L becomes a bucket of its own with two
    junctions that differ at d places (both get d); an item without a distance a bucket of one"""
    near, length, _, _ = TC.cases("default")[CHAINED]
    rng = np.random.default_rng(8)
    js, grp, want = [], [], []
    for g, (d, L) in enumerate(zip(near.tolist(), length.tolist())):
        a = rng.integers(0, 4, L)
        js.append("".join("ACGT"[x] for x in a))
        grp.append(g)
        want.append(d)
        if d > 0:
            b = a.copy()
            at = rng.choice(L, d, replace=False)
            b[at] = (b[at] + 1 + rng.integers(0, 3, d)) % 4
            js.append("".join("ACGT"[x] for x in b))
            grp.append(g)
            want.append(d)
    return js, grp, want


def _device(path):
    import ctypes as C
    from vdjer_amd import _lib, api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    kept0, allocs0 = ctx.stat("kept_device_bytes"), ctx.stat("kept_allocs")
    arrays, out = {}, dict(info={}, macs={}, dispatches={}, dtypes={})
    for which in TC.SETS:
        for name, (near, length, unit, _) in TC.cases(which).items():
            P = TC.params(which, name)
            res = ctx.lineage_threshold(near, length, unit, **P)
            macs = ctx.stat("threshold_macs")
            again = ctx.lineage_threshold(near, length, unit, **P)            # two calls give the same bits
            for f in ("hist", "density", "peaks"):
                assert again[f].tobytes() == res[f].tobytes(), (which, name, f)
                arrays[f"{which}/{name}/{f}"] = res[f]
            assert again["info"] == res["info"] and ctx.stat("threshold_macs") == macs, (which, name)
            out["info"][f"{which}/{name}"] = res["info"]
            out["dtypes"][f"{which}/{name}"] = [str(res[f].dtype) for f in ("hist", "density", "peaks")]
            if which == "default" and name in MACS_CASES:
                out["macs"][name] = macs
    assert ctx.stat("kept_device_bytes") == kept0 and ctx.stat("kept_allocs") == allocs0      # scratch is the workspace's: nothing is kept
    for name in DISPATCH_CASES:                                              # five dispatches whatever n is
        near, length, unit, _ = TC.cases("default")[name]
        ctx.profile(True)
        ctx.profile_reset()
        ctx.lineage_threshold(near, length, unit)
        out["dispatches"][name] = {k: v[1] for k, v in ctx.profile_get().items()}
        ctx.profile(False)
    # the distances from the device: vdjx_lineage, then the threshold of its nearest
    js, grp, _ = chained_junctions()
    lin = ctx.lineage(js, grp)
    lens = np.array([len(s) for s in js], np.uint32)
    res = ctx.lineage_threshold(lin["nearest"], lens)
    out["chained"] = dict(nearest=lin["nearest"].tolist(), info=res["info"])
    for f in ("hist", "density", "peaks"):
        arrays[f"chained/{f}"] = res[f]
    # the refusals: an error each, and the context goes on working
    good = TC.cases("default")["grid_ends"]
    want = ctx.lineage_threshold(*good[:3])

    def refused(match, near=good[0], length=good[1], unit=good[2], **P):
        with pytest.raises(VdjxError, match=match):
            ctx.lineage_threshold(near, length, unit, **P)
        now = ctx.lineage_threshold(*good[:3])
        assert now["info"] == want["info"] and now["density"].tobytes() == want["density"].tobytes(), match

    refused("at most 2\\^20 - 1", np.zeros(1 << 20, np.int32), np.ones(1 << 20, np.uint32), 1)
    refused("has nearest -2", np.array([3, -2], np.int32), np.array([40, 40], np.uint32), 1)
    refused("has length 0", np.array([3, 3], np.int32), np.array([40, 0], np.uint32), 1)
    refused("has length 256", np.array([3, 3], np.int32), np.array([256, 40], np.uint32), 1)
    for unit in (0, (1 << 20) + 1):
        refused("unit", unit=unit)
    for k in (0, -1, 201):
        refused("max_k", max_k=k)
    for s in (-1, 14):
        refused("peak_shift", peak_shift=s)
    for v in ((1, 0), (-1, 2), (3, 2), (1, 1000001)):
        refused("valley guard", valley=v)
    for mv in (0, -5):
        refused("min_values", min_values=mv)
    with pytest.raises(VdjxError):
        ctx.lineage_threshold(np.zeros((2, 2), np.int32), np.ones((2, 2), np.uint32))
    with pytest.raises(VdjxError):
        ctx.lineage_threshold([1.5], [40])
    with pytest.raises(VdjxError):
        ctx.lineage_threshold([1], [40], unit=-1)
    prm = _lib.ThresholdParams(200, 5, 1, 2, 10)
    rc = ctx.L.vdjx_lineage_threshold(ctx.h, api._p(good[0]), api._p(good[1]), len(good[0]), 2000, C.byref(prm), None, None, None, None)
    assert rc == -1 and b"NULL argument" in ctx.L.vdjx_last_error()
    info = _lib.ThresholdInfo()                                              # every output but info may be NULL
    rc = ctx.L.vdjx_lineage_threshold(ctx.h, api._p(good[0]), api._p(good[1]), len(good[0]), 2000, C.byref(prm), None, None, None, C.byref(info))
    assert rc == 0 and {f: int(getattr(info, f)) for f in api.Context.THRESHOLD_FIELDS} == want["info"] and info.reserved == 0
    assert ctx.lineage_threshold(np.full(3, -1, np.int32), np.array([0, 999, 1 << 31], np.uint32))["info"]["status"] == M.FEW      # lengths not read
    ctx.close()
    np.savez(path, **arrays)
    return out


@functools.lru_cache(maxsize=None)
def device():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "device.npz")
        code = f"import json; from tests.test_gpu_threshold import _device; print('THRESHOLD', json.dumps(_device({path!r})))"
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=_child_env("shipped"))
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
        out = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("THRESHOLD ")).split(" ", 1)[1])
        with np.load(path) as z:
            out["arrays"] = {k: z[k] for k in z.files}
    return out


def _same(key, model):
    dev = device()
    info = dev["info"][key] if key != "chained" else dev["chained"]["info"]
    assert info == model["info"], (key, info, model["info"])
    for f in ("hist", "density", "peaks"):
        a, b = dev["arrays"][f"{key}/{f}"], model[f]
        assert a.dtype == b.dtype and a.shape == b.shape, (key, f, a.dtype, a.shape)
        assert np.array_equal(a, b), (key, f, np.argwhere(a != b)[:5].tolist(), a[a != b][:5].tolist(), b[a != b][:5].tolist())


@pytest.mark.parametrize("which", list(TC.SETS))
@pytest.mark.parametrize("name", NAMES)
def test_threshold_case(which, name):
    _same(f"{which}/{name}", TC.model(which, name))
    assert device()["dtypes"][f"{which}/{name}"] == ["uint32", "uint64", "uint32"]


def test_threshold_multiply_adds():
    for name in MACS_CASES:
        near, length, unit, _ = TC.cases("default")[name]
        assert device()["macs"][name] == M.macs(M.bins(near, length, unit), 200) > 0, name


def test_threshold_dispatches_do_not_depend_on_the_input():
    assert device()["dispatches"] == {name: DISPATCHES for name in DISPATCH_CASES}, device()["dispatches"]


def test_threshold_of_the_device_own_nearest():
    js, grp, want = chained_junctions()
    near = device()["chained"]["nearest"]
    assert near == want and sum(d > 0 for d in near) > 100
    model = M.threshold(M.bins(near, [len(s) for s in js], 1))
    _same("chained", model)
    base = TC.model("default", CHAINED)
    assert np.array_equal(model["hist"], 2 * base["hist"]) and model["info"]["status"] == M.FOUND      # every distance twice: the same valley
    assert model["info"]["threshold"] == base["info"]["threshold"] and model["info"]["k"] == base["info"]["k"]
