"""vdjx_lineage_link on the GPU: clone, nearest, the single-linkage info and the link info against the model of tests/lineage_link_model.py,
bitwise, under complete and average linkage for every case of tests/lineage_link_cases.py -- the handmade partitions (a component of 2, the
tie and its reversed order, the merge on exact equality, identical junctions with and without an N, num = 0 and num = den, the chain single
linkage keeps and complete linkage cuts, items that take no part and interleaved buckets), component sizes around the row block of
k_link_matrix, around LINK_LDS_M and past k_link_merge's thread count, Hamming, a uniform, a realistic and an extreme table under both
symmetries, twenty seeded repertoires --; VDJX_LINK_CELLS at 1 and at a value that splits the components; the limit of 4,096 members on
both sides; linkage 0 against vdjx_lineage and vdjx_lineage_model bit for bit.  The calls run in child processes (as
tests/test_gpu_lineage.py runs its own); every model result is computed once."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lineage_link_cases as KC
from tests import lineage_link_model as KM
from tests import lineage_model as M
from tests.test_gpu_annot import _child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(KC.cases())


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_lineage_link import {fn}; print('LINLINK', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("LINLINK ")).split(" ", 1)[1])


def _pack(res):
    return dict(clone=res["clone"].tolist(), nearest=res["nearest"].tolist(), info=res["info"], link=res.get("link"),
                dtypes=[str(res["clone"].dtype), str(res["nearest"].dtype)])


def _call(ctx, name, link):
    js, grp, md, tab, sym = KC.cases()[name]
    if link == "single":                                                       # vdjx_lineage / vdjx_lineage_model themselves
        return ctx.lineage(js, grp, md, table=KC.table_of(tab), symmetry=sym)
    return ctx.lineage_link(js, grp, md, table=KC.table_of(tab), symmetry=sym, link=link)


def _device(_):
    from vdjer_amd import api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    kept0, allocs0 = ctx.stat("kept_device_bytes"), ctx.stat("kept_allocs")
    out = dict(cases={}, old={}, stats={}, dispatches={}, limit={})
    for name in NAMES:
        for link in ("complete", "average", 0):
            res = _call(ctx, name, link)
            if link != 0:
                out["stats"][f"{name}/{link}"] = ctx.stat("lineage_link_cells")
            again = _call(ctx, name, link)                                    # two calls give the same bits
            assert again["clone"].tobytes() == res["clone"].tobytes() and again["nearest"].tobytes() == res["nearest"].tobytes(), (name, link)
            assert again["info"] == res["info"] and again["link"] == res["link"], (name, link)
            out["cases"][f"{name}/{link}"] = _pack(res)
        out["old"][name] = _pack(_call(ctx, name, "single"))                   # vdjx_lineage / vdjx_lineage_model themselves
    assert ctx.stat("kept_device_bytes") == kept0 and ctx.stat("kept_allocs") == allocs0      # scratch is the workspace's: nothing is kept
    for name, link in (("size_89", "complete"), ("table_size_89", "average"), (KC.BATCHED, "average"), ("component_of_2", "complete")):
        ctx.profile(True)
        ctx.profile_reset()
        _call(ctx, name, link)
        out["dispatches"][f"{name}/{link}"] = {k: v[1] for k, v in ctx.profile_get().items()}
        ctx.profile(False)
    # no item, no participating item, no component of two; the refusals
    for link in ("complete", "average", 0):
        r0 = ctx.lineage_link([], [], link=link)
        assert r0["clone"].shape == (0,) and not any(r0["info"].values()) and not any(r0["link"].values())
        r1 = ctx.lineage_link(["ACGT", "ACGA"], [M.NONE, M.NONE], link=link)
        assert r1["clone"].tolist() == [-1, -1] and not any(r1["link"].values())
        r2 = ctx.lineage_link(["ACGTACGT", "TTTTTTTT"], [0, 0], link=link)
        assert r2["clone"].tolist() == [0, 1] and r2["link"] == dict.fromkeys(KM.LINK_FIELDS, 0) | (dict(clones_single=2) if link else {})
    good = (["ACGTACGT", "ACGTACGA"], [0, 0])
    for link in (3, -1):
        with pytest.raises(VdjxError, match="vdjx_lineage_link: linkage"):
            ctx.lineage_link(*good, link=link)
    with pytest.raises(VdjxError, match="link 'ward'"):
        ctx.lineage_link(*good, link="ward")
    for bad in ((1, 0), (1, 1000001), (-1, 10), (11, 10)):
        with pytest.raises(VdjxError, match="vdjx_lineage_link: threshold"):
            ctx.lineage_link(*good, max_dist=bad, link="average")
    with pytest.raises(VdjxError, match="bases"):
        ctx.lineage_link(["ACGT", ""], [0, 0], link="complete")
    from tests import lineage_dist_cases as LC
    uniform = LC.tables()["uniform"]
    with pytest.raises(VdjxError, match="symmetry"):
        ctx.lineage_link(*good, table=uniform, symmetry=2, link="complete")
    holed = uniform.copy()
    holed[27, 3] = 0
    with pytest.raises(VdjxError, match=r"cell \[27\]\[3\] is 0"):
        ctx.lineage_link(*good, table=holed, link="complete")
    # the limit: 4,096 identical junctions are one component and one clone; 4,097 are refused, and the context goes on working
    same = ["ACGTTGCAACGTACGTTGCA"] * (KM.MAX_M + 1)
    for link in ("complete", "average"):
        res = ctx.lineage_link(same[:KM.MAX_M], [0] * KM.MAX_M, link=link)
        out["limit"][link] = dict(clones=int(res["clone"].max()) + 1, zero=not res["clone"].any(), info=res["info"], link=res["link"])
        with pytest.raises(VdjxError, match=f"component of {KM.MAX_M + 1} junctions"):
            ctx.lineage_link(same, [0] * (KM.MAX_M + 1), link=link)
        after = _call(ctx, "tie", link)
        assert after["clone"].tolist() == out["cases"][f"tie/{link}"]["clone"]
    single = ctx.lineage_link(same, [0] * (KM.MAX_M + 1), link=0)                      # single linkage has no such limit
    assert not single["clone"].any() and single["info"]["clones"] == 1
    ctx.close()
    return out


def _device_batched(_):
    """the batched case under both linkages with whatever VDJX_LINK_CELLS the parent set"""
    from vdjer_amd import api
    ctx = api.Context(0)
    out = {link: _pack(_call(ctx, KC.BATCHED, link)) for link in KC.LINKAGES}
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def device():
    env = _child_env("shipped")
    env.pop("VDJX_LINK_CELLS", None)
    return _run_child("_device", "x", env)


def _same(dev, model, what):
    clone, near, info, link = model
    assert dev["dtypes"] == ["int32", "int32"], what
    a, b = np.asarray(dev["clone"], np.int64), clone.astype(np.int64)
    assert np.array_equal(a, b), (what, "clone", np.argwhere(a != b)[:5].tolist(), a[:16].tolist(), b[:16].tolist())
    a, b = np.asarray(dev["nearest"], np.int64), near.astype(np.int64)
    assert np.array_equal(a, b), (what, "nearest", np.argwhere(a != b)[:5].tolist())
    assert dev["info"] == info, (what, dev["info"], info)
    assert dev["link"] == link, (what, dev["link"], link)


@pytest.mark.parametrize("name", NAMES)
def test_lineage_link_against_the_model(name):
    for link in KC.LINKAGES:
        _same(device()["cases"][f"{name}/{link}"], KC.model(name, link), f"{name}/{link}")
        assert device()["stats"][f"{name}/{link}"] == KC.model(name, link)[3]["cells"]


@pytest.mark.parametrize("name", list(KC.HANDMADE))
def test_handmade_partitions_on_the_device(name):
    for link, want in KC.HANDMADE[name].items():
        clone = device()["cases"][f"{name}/{link}"]["clone"]
        assert sorted(sorted(p) for p in M.partition(clone)) == want, (name, link)


@pytest.mark.parametrize("name", NAMES)
def test_linkage_0_is_the_existing_call_bit_for_bit(name):
    zero, old = device()["cases"][f"{name}/0"], device()["old"][name]
    assert zero["clone"] == old["clone"] and zero["nearest"] == old["nearest"] and zero["info"] == old["info"] and zero["dtypes"] == old["dtypes"]
    assert zero["link"] == dict.fromkeys(KM.LINK_FIELDS, 0) and old["link"] is None
    _same(zero, KC.model(name, "single"), f"{name}/0")


def test_dispatches():
    """gather once, matrix and merge once per batch, beside the five of the single-linkage pass; the matrix kernel is the table's"""
    d = device()["dispatches"]
    base = {"k_lin_pack": 1, "k_lin_flatten": 1, "k_lin_number": 1, "k_lin_out": 1, "k_link_gather": 1, "k_link_matrix": 1, "k_link_merge": 1}
    assert d["size_89/complete"] == dict(base, k_lin_pairs=1)
    assert d["table_size_89/average"] == dict(base, k_lin_pairs_model=1)
    assert d[f"{KC.BATCHED}/average"] == dict(base, k_lin_pairs=1) and d["component_of_2/complete"] == dict(base, k_lin_pairs=1)


@pytest.mark.parametrize("which", ["one", "split"])
def test_batches_give_the_same_bytes(which, monkeypatch):
    knob = 1 if which == "one" else KC.splitting_knob(KC.BATCHED)
    monkeypatch.setenv("VDJX_LINK_CELLS", str(knob))
    got = _run_child("_device_batched", "x", _child_env("shipped"))
    sizes = KC.component_sizes(KC.BATCHED)
    want = KM.batches(sizes, knob)
    assert want == (len(sizes) if which == "one" else want) and 1 < want
    for link in KC.LINKAGES:
        ref = device()["cases"][f"{KC.BATCHED}/{link}"]
        assert got[link]["clone"] == ref["clone"] and got[link]["nearest"] == ref["nearest"] and got[link]["info"] == ref["info"], (which, link)
        assert got[link]["link"] == dict(ref["link"], batches=want) == KC.model(KC.BATCHED, link, knob)[3], (which, link)


def test_limit_of_4096():
    for link in KC.LINKAGES:
        got = device()["limit"][link]
        assert got["clones"] == 1 and got["zero"] and got["info"]["clones"] == 1 and got["info"]["links"] == KM.MAX_M * (KM.MAX_M - 1) // 2
        assert got["link"] == dict(components=1, largest_component=KM.MAX_M, merges=KM.MAX_M - 1, clones_single=1, batches=1, cells=KM.MAX_M ** 2)
