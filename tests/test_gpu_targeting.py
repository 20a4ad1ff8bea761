"""vdjx_targeting_counts on the GPU: every counter against the integer model of tests/targeting_model.py on the cases of
tests/targeting_cases.py (what each is for: tests/test_targeting_cpu.py) -- selection's count cases with every contig a unit of its own and
the opportunities vdjx_selection counts with unit weights, the group rules, one hot bin, the batches at VDJX_TGT_UNITS 1, 3 and default --
and the refusals by message.  The API runs in child processes; the main one runs once for the tests that share it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import selection_cases as SC
from tests import targeting_cases as TC
from tests import targeting_model as T
from tests import test_gpu_mutation as TM
from tests.test_gpu_annot import _child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("1", "3", None)                                              # VDJX_TGT_UNITS of the batch case; None: the default


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_targeting import {fn}; print('TGT', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("TGT ")).split(" ", 1)[1])


def _launches(ctx):
    return {k: x[1] for k, x in ctx.profile_get().items()}


def _device_main(path):
    from vdjer_amd import api
    ctx = api.Context(0)
    ctx.germline_load(TM.records())
    save, infos = {}, {}
    os.environ.pop("VDJX_TGT_UNITS", None)

    def call(name, ct, v, lim, grp, batches=1):
        ctx.profile_reset()
        r = ctx.targeting_counts(ct, v, limit=lim, group=grp)
        assert _launches(ctx) == ({"k_tgt_mark": batches, "k_tgt_count": batches} if batches else {}), (name, _launches(ctx))
        again = ctx.targeting_counts(ct, v, limit=lim, group=grp)
        assert again["counts"].tobytes() == r["counts"].tobytes() and again["info"] == r["info"], name
        assert ctx.stat("targeting_units") == r["info"]["units"] and ctx.stat("targeting_batches") == r["info"]["batches"]
        assert ctx.stat("targeting_us") > 0 or not batches
        save[name], infos[name] = r["counts"], r["info"]

    ctx.profile(True)
    # selection's count cases, every contig on its own; and the opportunities vdjx_selection counts with unit weights
    ct, v, lim = TC.count_inputs()
    call("count", ct, v, lim, None)
    sel = ctx.selection(ct, v, limit=lim, weight=np.ones((1024, 4), np.uint32))["counts"]
    infos["sel_exp"] = [int(sel["exp_s"].sum()), int(sel["exp_r"].sum())]
    call("count_own", ct, v, lim, -1 - np.arange(len(ct), dtype=np.int32))
    # the groups, as given and permuted
    ct, v, lim, grp = TC.group_inputs()
    call("group", ct, v, lim, grp)
    call("ungrouped", ct, v, lim, None)
    pm = TC.permutation()
    call("permuted", [ct[i] for i in pm], {f: x[pm] for f, x in v.items()}, lim[pm], grp[pm])
    # the batches
    ct, v, lim, grp = TC.group_inputs(TC.batch_cases())
    units = TC.batch_model()[1]["units"]
    for u in UNITS:
        if u is None:
            os.environ.pop("VDJX_TGT_UNITS", None)
        else:
            os.environ["VDJX_TGT_UNITS"] = u                          # (read per call)
        call(f"batch_{u}", ct, v, lim, grp, batches=-(-units // int(u or 1 << 18)))
    os.environ.pop("VDJX_TGT_UNITS", None)
    # no contig, and no usable hit
    r0 = ctx.targeting_counts([], SC.hits([]))
    assert not r0["counts"].any() and not any(r0["info"].values())
    none = [dict(v=TM.NONE)] * 3
    call("no_hit", ["ACGT" * 10] * 3, SC.hits(none), None, None, batches=0)
    ctx.profile(False)
    ctx.close()
    np.savez(path, **save)
    return infos


@pytest.fixture(scope="module")
def main(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tgt") / "dev.npz")
    infos = _run_child("_device_main", path, _child_env("shipped"))
    return np.load(path), infos


def _same(dev, info, want, what):
    cnt, winfo = want
    assert dev.dtype == np.uint64 and dev.shape == (2, 2, 1024, 4)
    assert np.array_equal(dev, cnt), (what, [(tuple(i), int(dev[tuple(i)]), int(cnt[tuple(i)])) for i in np.argwhere(dev != cnt)[:5]])
    assert info == winfo, (what, info, winfo)


def test_count_cases_vs_model(main):
    dev, infos = main
    _same(dev["count"], infos["count"], TC.count_model(), "count")
    _same(dev["count_own"], infos["count_own"], TC.count_model(), "count_own")
    # with unit weights k_sel_counts and k_tgt_* count the same opportunities
    assert infos["sel_exp"] == [infos["count"]["opp_s"], infos["count"]["opp_r"]]
    assert infos["no_hit"] == dict(dict.fromkeys(T.INFO, 0), contigs=3) and not dev["no_hit"].any()


def test_group_rules(main):
    dev, infos = main
    _same(dev["group"], infos["group"], TC.group_model(), "group")
    _same(dev["ungrouped"], infos["ungrouped"], TC.group_model(grouped=False), "ungrouped")
    assert dev["permuted"].tobytes() == dev["group"].tobytes() and infos["permuted"] == infos["group"]
    assert infos["group"]["units"] < infos["ungrouped"]["units"] and infos["group"]["obs_s"] + infos["group"]["obs_r"] < infos["ungrouped"]["obs_s"] + infos["ungrouped"]["obs_r"]


def test_batches_give_the_same_bytes(main):
    dev, infos = main
    units = TC.batch_model()[1]["units"]
    for u in UNITS:
        want = TC.batch_model()
        _same(dev[f"batch_{u}"], infos[f"batch_{u}"], (want[0], dict(want[1], batches=-(-units // int(u or 1 << 18)))), u)
    assert dev["batch_1"].tobytes() == dev["batch_3"].tobytes() == dev["batch_None"].tobytes()
    assert [infos[f"batch_{u}"]["batches"] for u in UNITS] == [units, -(-units // 3), 1]


def _device_hot(_):
    from vdjer_amd import api
    ctx = api.Context(0)
    ctx.germline_load(TC.HOT_RECORDS)
    ct, v, lim, grp = TC.group_inputs(TC.hot_cases())
    r = ctx.targeting_counts(ct, v, limit=lim, group=grp)
    again = ctx.targeting_counts(ct, v, limit=lim, group=grp)
    assert again["counts"].tobytes() == r["counts"].tobytes()
    ctx.close()
    return dict(counts=r["counts"].ravel().tolist(), info=r["info"])


def test_one_hot_bin():
    res = _run_child("_device_hot", "x", _child_env("shipped"))
    _same(np.array(res["counts"], np.uint64).reshape(2, 2, 1024, 4), res["info"], TC.hot_model(), "hot")


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------
def _device_refusals(_):
    from vdjer_amd import api
    from vdjer_amd._lib import VdjxError
    cs = SC.count_cases()
    good = [c for c in cs if c["name"] == "frame1"][0]
    H = TM.H
    pair = lambda **kw: [good, dict(good, **kw)]

    def call(ctx, cs2, match, **kw):
        with pytest.raises(VdjxError, match=match):
            ctx.targeting_counts([c["contig"] for c in cs2], SC.hits(cs2), **kw)
        return 1

    ctx = api.Context(0)
    done = call(ctx, pair(), "vdjx_targeting_counts: no germline set is loaded")
    ctx.germline_load(TM.records())
    vh = good["v"]
    hit = lambda h, **kw: dict(h, **kw)
    # one refused hit per message of the shared check, word for word what vdjx_selection says under its own name
    for cs2, msg in ((pair(v=hit(vh, gene=11)), "is not a V record of the loaded set"), (pair(v=hit(vh, gene=TM.J0)), "is not a V record of the loaded set"),
                     (pair(v=hit(vh, runs=[(100 << 4) | 3] + [0] * 63)), "a run with an op outside 0..2 or a length of 0"),
                     (pair(v=hit(vh, runs=[0] + [0] * 63)), "a run with an op outside 0..2 or a length of 0"),
                     (pair(v=hit(H(TM.V0, 1, 1, [("M", 9)]), seq_start=0, seq_end=8)), "contig positions 0 .. 8"),
                     (pair(v=H(TM.V0, 290, 1, [("M", 20)])), "contig positions 290 .. 309"),
                     (pair(v=H(TM.V2, 5, 1, [("M", 2)])), "germline positions 1 .. 2"),
                     (pair(v=hit(vh, seq_end=vh["seq_end"] + 1)), "runs hold"), (pair(v=hit(vh, germ_end=vh["germ_end"] + 1)), "runs hold")):
        with pytest.raises(VdjxError, match="vdjx_targeting_counts: contig 1: the V hit") as tgt:
            ctx.targeting_counts([c["contig"] for c in cs2], SC.hits(cs2))
        assert msg in str(tgt.value), (msg, str(tgt.value))
        with pytest.raises(VdjxError) as sel:
            ctx.selection([c["contig"] for c in cs2], SC.hits(cs2))
        assert str(sel.value).replace("vdjx_selection", "vdjx_targeting_counts") == str(tgt.value)
        done += 1
    for bad in (-1, TM.LEN + 1):
        done += call(ctx, pair(), "vdjx_targeting_counts: contig 1: limit", limit=[TM.LEN, bad])
    with pytest.raises(VdjxError, match="^vdjx_targeting_counts: 2 contigs, v\\['runs'\\] of shape"):
        ctx.targeting_counts([c["contig"] for c in pair()], dict(SC.hits(pair()), runs=np.zeros((2, 63), np.int64)))
    with pytest.raises(VdjxError, match="group of shape"):
        ctx.targeting_counts([c["contig"] for c in pair()], SC.hits(pair()), group=[0])
    two = pair()
    with pytest.raises(VdjxError, match="vdjx_targeting_counts: contigs of unequal length"):
        ctx.targeting_counts((two[0]["contig"].encode() + b"ACG\0" + two[1]["contig"].encode()[4:], 2, TM.LEN), SC.hits(two))
    with pytest.raises(VdjxError, match="vdjx_targeting_counts: len=4096"):
        ctx.targeting_counts(["A" * 4096], SC.hits([dict(v=TM.NONE)]))
    done += 4
    raw, n, ln = ctx.pack_strings([c["contig"] for c in pair()])
    hv = ctx._hit_array(SC.hits(pair()), 2, "v", "vdjx_targeting_counts")
    rc = ctx.L.vdjx_targeting_counts(ctx.h, raw, 2, ln, hv.ctypes.data, None, None, None, None)
    assert rc != 0 and b"vdjx_targeting_counts: NULL argument" in ctx.L.vdjx_last_error()
    big = 1 << 20
    zero = np.zeros(big, api.Context.ANNOT_HIT)
    out = np.zeros((2, 2, 1024, 4), np.uint64)
    rc = ctx.L.vdjx_targeting_counts(ctx.h, b"A" * big, big, 1, zero.ctypes.data, None, None, out.ctypes.data, None)
    assert rc != 0 and b"2^20" in ctx.L.vdjx_last_error()
    # a refused call leaves the context usable
    ok = ctx.targeting_counts([c["contig"] for c in pair()], SC.hits(pair()))
    assert ok["info"]["used"] == 2 and ok["info"]["units"] == 2
    ctx.close()
    return done + 2


def test_refusals_by_message():
    assert _run_child("_device_refusals", "x", _child_env("shipped")) == 18
