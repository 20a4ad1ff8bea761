"""vdjx_lineage_model on the GPU: clone, nearest, every info field and the walked pairs against the model of tests/lineage_dist_model.py,
exactly, for every case of tests/lineage_dist_cases.py under both symmetries -- bucket sizes around the row block and the column tile,
junction lengths without a 5-mer, around the 32-base words and at 255, single substitutions placed at the ends and across the word
boundaries, characters that are not ACGT at and beside a mismatch, pairs the model links and Hamming does not (and the other way), a
bucket whose clones depend on the symmetry, the largest D, a bucket of 4,097 with column slices of 128, interleaved buckets; the uniform
table against vdjx_lineage itself, a permutation, the refusals, the dispatches.  The calls run in one child process (as
tests/test_gpu_lineage.py runs its own); every model result is computed once."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lineage_dist_cases as LC
from tests import lineage_dist_model as LM
from tests import lineage_model as M
from tests.test_gpu_annot import _child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["items", "buckets", "largest_bucket", "clones", "pairs", "links"]
DISPATCHES = {"k_lin_pack": 1, "k_lin_pairs_model": 1, "k_lin_flatten": 1, "k_lin_number": 1, "k_lin_out": 1}
DISPATCH_CASES = ("size_1", "size_129", "interleaved")


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_lineage_dist import {fn}; print('LINDIST', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("LINDIST ")).split(" ", 1)[1])


def _pack(res):
    return dict(clone=res["clone"].tolist(), nearest=res["nearest"].tolist(), info=res["info"], dtypes=[str(res["clone"].dtype), str(res["nearest"].dtype)])


def _device(_):
    import ctypes as C
    from vdjer_amd import _lib, api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    kept0, allocs0 = ctx.stat("kept_device_bytes"), ctx.stat("kept_allocs")
    out = dict(cases={}, hamming={}, perm={}, dispatches={})
    for name, (js, grp, md, tab) in LC.cases().items():
        table = LC.tables()[tab]
        for sym in LM.SYMMETRY:
            res = ctx.lineage(js, grp, md, table=table, symmetry=sym)
            stats = dict(work_items=ctx.stat("lineage_work_items"), walked=ctx.stat("lineage_model_walked"))
            again = ctx.lineage(js, grp, md, table=table, symmetry=sym)  # two calls give the same bits
            assert again["clone"].tobytes() == res["clone"].tobytes() and again["nearest"].tobytes() == res["nearest"].tobytes() and again["info"] == res["info"], name
            assert ctx.stat("lineage_model_walked") == stats["walked"], name
            out["cases"][f"{name}/{sym}"] = dict(_pack(res), **stats)
        if tab == "uniform":                                               # the same call without a table: vdjx_lineage
            out["hamming"][name] = _pack(ctx.lineage(js, grp, md))
    assert ctx.stat("kept_device_bytes") == kept0 and ctx.stat("kept_allocs") == allocs0      # scratch is the workspace's: nothing is kept
    js, grp, md, tab = LC.cases()[LC.PERMUTED]
    order = LC.permutation()
    for sym in LM.SYMMETRY:
        out["perm"][sym] = _pack(ctx.lineage([js[i] for i in order], [grp[i] for i in order], md, table=LC.tables()[tab], symmetry=sym))
    bare = ctx.lineage(js, grp, md, nearest=False, table=LC.tables()[tab])    # out_nearest = NULL
    assert bare["nearest"] is None and bare["clone"].tolist() == out["cases"][f"{LC.PERMUTED}/avg"]["clone"]
    for name in DISPATCH_CASES:                                              # five dispatches whatever n and the number of buckets are
        js, grp, md, tab = LC.cases()[name]
        ctx.profile(True)
        ctx.profile_reset()
        ctx.lineage(js, grp, md, table=LC.tables()[tab])
        out["dispatches"][name] = {k: v[1] for k, v in ctx.profile_get().items()}
        ctx.profile(False)
    # no item; the refusals of vdjx_lineage; the three new ones
    uniform = LC.tables()["uniform"]
    r0 = ctx.lineage([], [], table=uniform)
    assert r0["clone"].shape == (0,) and r0["nearest"].shape == (0,) and r0["info"] == dict.fromkeys(FIELDS, 0)
    good = (["ACGTACGT", "ACGTACGA"], [0, 0])
    assert ctx.lineage(*good, table=uniform)["nearest"].tolist() == [2000, 2000]
    for bad in ((1, 0), (1, -1), (1, 1000001), (-1, 10), (11, 10)):
        with pytest.raises(VdjxError, match="vdjx_lineage_model: threshold"):
            ctx.lineage(*good, max_dist=bad, table=uniform)
    for js in (["ACGT", ""], ["ACGT", "A" * 256]):
        with pytest.raises(VdjxError, match="bases"):
            ctx.lineage(js, [0, 0], table=uniform)
    for sym in (2, -1):
        with pytest.raises(VdjxError, match="symmetry"):
            ctx.lineage(*good, table=uniform, symmetry=sym)
        with pytest.raises(VdjxError, match="symmetry"):
            ctx.lineage([], [], table=uniform, symmetry=sym)
    with pytest.raises(VdjxError, match="symmetry"):
        ctx.lineage(*good, table=uniform, symmetry="mid")
    holed = uniform.copy()
    holed[27, 3] = 0                                                         # AACGT -> T: off-centre
    with pytest.raises(VdjxError, match=r"cell \[27\]\[3\] is 0"):
        ctx.lineage(*good, table=holed)
    centre = uniform.copy()
    centre[27, 1] = 7                                                        # (the centre's column is not looked at)
    assert ctx.lineage(*good, table=centre)["nearest"].tolist() == [2000, 2000]
    L, h = ctx.L, ctx.h
    prm, info = _lib.LineageModelParams(1500, 10000, 0), _lib.LineageInfo()
    clone, grp2 = np.zeros(2, np.int32), np.zeros(2, np.uint32)
    info.items = 99
    rc = L.vdjx_lineage_model(h, b"ACGTACGT", api._p(np.array([0, 4, 8], np.uint64)), api._p(grp2), 2, C.byref(prm), None, api._p(clone), None, C.byref(info))
    assert rc == -1 and b"NULL table" in L.vdjx_last_error() and info.items == 0
    for shape in ((1024, 3), (4096,)):
        with pytest.raises(VdjxError, match="table of shape"):
            ctx.lineage(*good, table=np.ones(shape, np.uint16))
    with pytest.raises(VdjxError, match="table of shape"):
        ctx.lineage(*good, table=np.full((1024, 4), 65536, np.int64))
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def device():
    return _run_child("_device", "x", _child_env("shipped"))


def _same(dev, model, what):
    clone, near, info, walked = model
    assert dev["dtypes"] == ["int32", "int32"], what
    a, b = np.asarray(dev["clone"], np.int64), clone.astype(np.int64)
    assert np.array_equal(a, b), (what, "clone", np.argwhere(a != b)[:5].tolist(), a[:16].tolist(), b[:16].tolist())
    a, b = np.asarray(dev["nearest"], np.int64), near.astype(np.int64)
    assert np.array_equal(a, b), (what, "nearest", np.argwhere(a != b)[:5].tolist(), a[:16].tolist(), b[:16].tolist())
    assert dev["info"] == info, (what, dev["info"], info)
    if walked is not None:
        assert dev["walked"] == walked, (what, "walked", dev["walked"], walked)


def _both(name):
    for sym in LM.SYMMETRY:
        _same(device()["cases"][f"{name}/{sym}"], LC.models()[name, sym], f"{name}/{sym}")


@pytest.mark.parametrize("m", LC.SIZES)
def test_lineage_model_bucket_sizes(m):
    _both(f"size_{m}")
    assert device()["cases"][f"size_{m}/avg"]["work_items"] == (-(-m // 64)) ** 2


@pytest.mark.parametrize("L", LC.LENGTHS)
def test_lineage_model_lengths(L):
    for name in (f"len_{L}", f"len_{L}_extreme", f"len_{L}_uniform"):
        _both(name)


@pytest.mark.parametrize("L", LC.LENGTHS)
def test_uniform_table_is_2000_times_hamming(L):
    """the same clones as vdjx_lineage, nearest = 2000 x its nearest, under both symmetries"""
    name = f"len_{L}_uniform"
    ham = device()["hamming"][name]
    js, grp, md, _ = LC.cases()[name]
    clone, near, info = M.lineage(js, grp, md)
    assert ham["clone"] == clone.tolist() and ham["nearest"] == near.tolist() and ham["info"] == info
    for sym in LM.SYMMETRY:
        dev = device()["cases"][f"{name}/{sym}"]
        assert dev["clone"] == ham["clone"] and dev["info"] == ham["info"], (name, sym)
        assert dev["nearest"] == [2000 * d if d >= 0 else -1 for d in ham["nearest"]], (name, sym)


@pytest.mark.parametrize("name", [k for k in LC.cases() if k.startswith(("placed_", "not_acgt_"))])
def test_lineage_model_placed_mismatches_and_other_characters(name):
    _both(name)


@pytest.mark.parametrize("name", ["heavier_than_hamming", "lighter_than_hamming", "symmetry_matters", "largest_d", "interleaved", "interleaved_extreme"])
def test_lineage_model_named_cases(name):
    _both(name)
    if name == "largest_d":
        assert device()["cases"]["largest_d/avg"]["nearest"] == [251 * 2 * 65535 + 4 * 2000] * 2
    if name == "symmetry_matters":
        assert device()["cases"][f"{name}/avg"]["clone"] != device()["cases"][f"{name}/min"]["clone"]


def test_lineage_model_one_large_bucket():
    """4,097 junctions: 65 row blocks x 33 column slices of 128 (two tiles each, the last slice one column)"""
    _both(LC.BIG)
    for sym in LM.SYMMETRY:
        assert device()["cases"][f"{LC.BIG}/{sym}"]["work_items"] == 65 * 33 and LM.slice_width([4097]) == 128


def test_lineage_model_permutation_keeps_the_partition():
    order = LC.permutation()
    js, grp, md, tab = LC.cases()[LC.PERMUTED]
    for sym in LM.SYMMETRY:
        dev, base = device()["perm"][sym], device()["cases"][f"{LC.PERMUTED}/{sym}"]
        back = {new: old for new, old in enumerate(order)}
        assert {frozenset(back[i] for i in s) for s in M.partition(dev["clone"])} == M.partition(base["clone"]), sym
        assert [dev["nearest"][new] for new in np.argsort(order)] == base["nearest"] and dev["info"] == base["info"], sym
        clone, near, info, _ = LM.lineage([js[i] for i in order], [grp[i] for i in order], LC.tables()[tab], md, sym)
        _same(dev, (clone, near, info, None), f"permuted/{sym}")


def test_lineage_model_dispatches_do_not_depend_on_the_input():
    assert device()["dispatches"] == {name: DISPATCHES for name in DISPATCH_CASES}, device()["dispatches"]
