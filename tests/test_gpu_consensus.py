"""vdjx_consensus on the GPU: rows, cover, best, units and info bitwise the integer model of tests/consensus_model.py on the cases of
tests/consensus_cases.py (what each is for: tests/test_consensus_cpu.py) -- the edges at 0.6 and at mostCommon, 300 lone contigs, one unit
of 300 voters over the 2,047-base record, the batches at VDJX_CONS_CELLS 1, 4,096 and default, a permutation inside the groups --, planted
sisters of the e2e_families contigs (no model: the founder with the shared changes), the round trip of vdjx_consensus_hits through
vdjx_mutations and vdjx_selection, and the refusals by message.  The API runs in child processes; the main one runs once."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import consensus_cases as CC
from tests import consensus_model as CM
from tests import mutation_model as M
from tests import selection_cases as SC
from tests import targeting_cases as TC
from tests import test_gpu_mutation as TM
from tests.test_gpu_annot import _child_env
from tests.test_mutation_cpu import planted_families

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = ("1", "4096", None)                                           # VDJX_CONS_CELLS; None: the default


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_consensus import {fn}; print('CONS', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("CONS ")).split(" ", 1)[1])


def _pack(r):
    return dict(unit=np.asarray(r["unit"]).tolist(), units={f: np.asarray(x).tolist() for f, x in r["units"].items()}, cons=r["cons"], germ=r["germ"],
                cover=[np.asarray(x).tolist() for x in r["cover"]], best=[np.asarray(x).tolist() for x in r["best"]], info=r["info"])


def _launches(ctx):
    return {k: x[1] for k, x in ctx.profile_get().items()}


def _none_hits(n):
    return CC.hits([dict(v=TM.NONE)] * n)


def _device_main(_):
    from vdjer_amd import annot, api
    ctx = api.Context(0)
    ctx.germline_load(TM.records())
    os.environ.pop("VDJX_CONS_CELLS", None)
    out = {}
    ctx.profile(True)

    def call(name, ct, v, lim, grp, freq=CM.DEFAULT):
        ctx.profile_reset()
        r = ctx.consensus(ct, v, limit=lim, group=grp, min_freq=freq, counts=True)
        ln = _launches(ctx)
        batches = r["info"]["batches"]
        assert ln.get("k_cons_vote", 0) == ln.get("k_cons_decide", 0) <= batches and (ln.get("k_cons_vote", 0) >= 1) == (r["info"]["columns"] > 0), (name, ln)
        again = ctx.consensus(ct, v, limit=lim, group=grp, min_freq=freq, counts=True)
        assert _pack(again) == _pack(r), name
        bare = ctx.consensus(ct, v, limit=lim, group=grp, min_freq=freq)
        assert bare["cover"] is None and bare["best"] is None and bare["cons"] == r["cons"] and bare["info"] == r["info"], name
        assert ctx.stat("consensus_units") == r["info"]["units"] and ctx.stat("consensus_batches") == batches, name
        assert ctx.stat("consensus_us") > 0 or not batches, name
        out[name] = _pack(r)
        return r

    ct, v, lim, grp = CC.inputs(CC.edge_cases())
    edges = call("edges", ct, v, lim, grp)
    call("edges_common", ct, v, lim, grp, CC.MOST_COMMON)
    # a permutation of the contigs: the groups keep their members, the units their order only where their first contigs keep theirs
    pm = CC.permutation()
    call("edges_permuted", [ct[i] for i in pm], {f: x[pm] for f, x in v.items()}, lim[pm], grp[pm])
    lone_in = TC.group_inputs(TC.batch_cases())
    for cells in CELLS:
        if cells is None:
            os.environ.pop("VDJX_CONS_CELLS", None)
        else:
            os.environ["VDJX_CONS_CELLS"] = cells                     # (read per call)
        call(f"edges_{cells}", ct, v, lim, grp)
        call(f"lone_{cells}", *lone_in)
    os.environ.pop("VDJX_CONS_CELLS", None)
    big = CC.inputs(CC.big_cases())
    for cells in ("1", None):
        if cells:
            os.environ["VDJX_CONS_CELLS"] = cells
        else:
            os.environ.pop("VDJX_CONS_CELLS", None)
        call(f"big_{cells}", *big)
    # no contig; no usable hit
    r0 = ctx.consensus([], _none_hits(0))
    assert r0["cons"] == [] and not any(r0["info"].values()) and len(r0["unit"]) == 0
    call("no_hit", ["ACGT" * 10] * 3, _none_hits(3), None, None)

    # the round trip: the rows as pseudo-contigs through vdjx_mutations and vdjx_selection
    trip = {}
    for name, r in (("edges", edges), ("edges_common", None)):
        r = r or ctx.consensus(ct, v, limit=lim, group=grp, min_freq=CC.MOST_COMMON)
        pc, hv = annot.consensus_hits(r["units"], r["cons"], r["germ"])
        mu = ctx.mutations(pc, hv, _none_hits(len(pc)), rows=False)
        se = ctx.selection(pc, hv)
        tg = ctx.targeting_counts(pc, hv)
        trip[name] = dict(aligned=mu["info"]["aligned"], truncated=mu["info"]["truncated"], used=se["info"]["used"], tgt_used=tg["info"]["used"],
                          genes=np.asarray(hv["gene"]).tolist(), n_runs=np.asarray(hv["n_runs"]).tolist())
    lct, lv, llim, lgrp = lone_in
    r = ctx.consensus(lct, lv)                                        # every contig on its own, limit = len
    pc, hv = annot.consensus_hits(r["units"], r["cons"], r["germ"])
    own = ctx.mutations(lct, lv, _none_hits(len(lct)), rows=False)["counts"]
    got = ctx.mutations(pc, hv, _none_hits(len(pc)), rows=False)["counts"]
    sel_own, sel_got = ctx.selection(lct, lv)["counts"], ctx.selection(pc, hv)["counts"]
    trip["lone"] = dict(unit=np.asarray(r["unit"]).tolist(), n_runs=np.asarray(lv["n_runs"]).tolist(),
                        own={f: np.asarray(own[f]).tolist() for f in ("v_r", "v_s", "v_stop", "v_codons")},
                        got={f: np.asarray(got[f]).tolist() for f in ("v_r", "v_s", "v_stop", "v_codons")},
                        sel_own=np.asarray(sel_own["obs_r"]).tolist(), sel_got=np.asarray(sel_got["obs_r"]).tolist())
    out["trip"] = trip
    ctx.profile(False)
    ctx.close()
    return out


@pytest.fixture(scope="module")
def main():
    return _run_child("_device_main", "x", _child_env("shipped"))


def _same(dev, want, what, batches=None):
    for k in ("unit", "cons", "germ", "cover", "best"):
        assert dev[k] == want[k], (what, k, [(u, a, b) for u, (a, b) in enumerate(zip(dev[k], want[k])) if a != b][:2])
    for f in CM.UNIT:
        assert dev["units"][f] == want["units"][f], (what, f)
    winfo = dict(want["info"]) if batches is None else dict(want["info"], batches=batches)
    assert dev["info"] == winfo, (what, dev["info"], winfo)


def test_edges_vs_model(main):
    _same(main["edges"], CC.edge_model(), "edges")
    _same(main["edges_common"], CC.edge_model(CC.MOST_COMMON), "edges_common")
    assert main["edges"]["cons"] != main["edges_common"]["cons"]
    ct, v, lim, grp = CC.inputs(CC.edge_cases())
    assert main["no_hit"]["info"] == dict(dict.fromkeys(CM.INFO, 0), contigs=3) and main["no_hit"]["cons"] == []


def test_permutation_inside_the_groups(main):
    """the same multiset of votes per unit: the rows are identical, unit for unit (found by group; the lone contigs by their place)"""
    pm = CC.permutation()
    ct, v, lim, grp = CC.inputs(CC.edge_cases())
    _same(main["edges_permuted"], CM.consensus([ct[i] for i in pm], {f: x[pm] for f, x in v.items()}, TM.germs(), lim[pm], grp[pm]), "permuted")
    a, b = main["edges"], main["edges_permuted"]
    by_group = {g: u for u, g in enumerate(b["units"]["group"]) if g >= 0}
    inv = {int(old): new for new, old in enumerate(pm)}
    seen = 0
    for u, g in enumerate(a["units"]["group"]):
        if g >= 0:
            w = by_group[g]
        else:
            first = a["unit"].index(u)
            w = b["unit"][inv[first]]
        assert (a["cons"][u], a["germ"][u], a["cover"][u], a["best"][u]) == (b["cons"][w], b["germ"][w], b["cover"][w], b["best"][w]), (u, w)
        assert all(a["units"][f][u] == b["units"][f][w] for f in ("group", "gene", "members", "off_record", "lo", "hi"))
        seen += 1
    assert seen == a["info"]["units"] == b["info"]["units"] and {k: x for k, x in a["info"].items()} == b["info"]


def test_batches_give_the_same_bytes(main):
    for what, model in (("edges", CC.edge_model), ("lone", CC.lone_model)):
        for cells in CELLS:
            want = model(cells=int(cells)) if cells else model()
            _same(main[f"{what}_{cells}"], want, (what, cells))
        ref = dict(main[f"{what}_None"], info=None)
        assert all(dict(main[f"{what}_{c}"], info=None) == ref for c in CELLS)
        nb = [main[f"{what}_{c}"]["info"]["batches"] for c in CELLS]
        assert nb[0] == main[f"{what}_None"]["info"]["units"] > nb[1] >= nb[2] == 1 and (what == "edges" or nb[1] > 1), nb
    assert main["lone_None"]["info"]["units"] > 300 and main["lone_None"]["units"]["members"].count(1) >= TC.SINGLES


def test_one_unit_of_300_voters(main):
    _same(main["big_None"], CC.big_model(), "big")
    _same(main["big_1"], CC.big_model(), "big_1")
    info = main["big_None"]["info"]
    assert info["large_units"] >= 1 and info["units"] == 1 and info["columns"] == TC.HOT_LEN and max(main["big_None"]["cover"][0]) > 40


def test_round_trip_through_mutations_and_selection(main):
    trip = main["trip"]
    for name in ("edges", "edges_common"):
        t = trip[name]
        usable = sum(g >= 0 and r <= 64 for g, r in zip(t["genes"], t["n_runs"]))
        over = sum(g >= 0 and r > 64 for g, r in zip(t["genes"], t["n_runs"]))
        assert t["aligned"] == t["used"] == t["tgt_used"] == usable > 15 and t["truncated"] == over == 1 and t["genes"].count(-1) >= 2
    lone = trip["lone"]
    plain = [i for i, (u, r) in enumerate(zip(lone["unit"], lone["n_runs"])) if u >= 0 and r == 1]
    assert len(plain) >= TC.SINGLES
    for f in ("v_r", "v_s", "v_stop", "v_codons"):
        assert [lone["got"][f][lone["unit"][i]] for i in plain] == [lone["own"][f][i] for i in plain], f
    assert [lone["sel_got"][lone["unit"][i]] for i in plain] == [lone["sel_own"][i] for i in plain]
    assert sum(lone["own"]["v_r"][i] + lone["own"]["v_s"][i] for i in plain) > 300


# ---- planted sisters: no model, the founder with exactly the shared changes ------------------------------------------------------------------
FOUNDERS, COPIES = 8, 5
SHARED = ((0, 1, 2), (0, 1, 2, 3), (0, 1, 2, 3, 4))                   # the copies that carry the three shared changes: 3 of 5 meets 0.6 exactly
PRIVATE = (0, 1, 3, 4)                                                # the copies that carry one private change each


def _device_sisters(_):
    from vdjer_amd import api
    ids, seqs, recs, _ = planted_families()
    clean = [(h, q.upper()) for h, q, _ in recs]
    ctx = api.Context(0)
    ctx.germline_load(clean)
    v = ctx.annotate(seqs)["v"]
    lim = M.mutation_limit(ids, seqs)
    other = lambda ch, k: "ACGT"[("ACGT".index(ch) + k) % 4]
    found = []
    for c in range(len(seqs)):                                        # founders: one M run, 150 bases or more below the limit, ACGT only
        if len(found) == 3 * FOUNDERS:
            break
        a, b = int(v["seq_start"][c]) - 1, min(int(v["seq_end"][c]), int(lim[c]))
        if v["gene"][c] >= 0 and v["n_runs"][c] == 1 and v["n_tied"][c] == 1 and b - a >= 150 and set(seqs[c][a:b]) <= set("ACGT"):
            found.append(c)
    batch, plan = [], []
    for c in found:
        a, b = int(v["seq_start"][c]) - 1, min(int(v["seq_end"][c]), int(lim[c]))
        sites = [int(x) for x in np.linspace(a + 30, b - 30, len(SHARED) + len(PRIVATE))]      # 90 bases and more between 7 sites: apart
        copies = [list(seqs[c]) for _ in range(COPIES)]
        truth = list(seqs[c])
        for k, who in enumerate(SHARED):
            q = sites[k]
            truth[q] = other(seqs[c][q], 1 + k % 3)
            for w in who:
                copies[w][q] = truth[q]
        for k, w in enumerate(PRIVATE):
            q = sites[len(SHARED) + k]
            copies[w][q] = other(seqs[c][q], 2)
        batch += ["".join(x) for x in copies]
        plan.append(dict(founder=c, truth="".join(truth)))
    hv = ctx.annotate(batch)["v"]
    keep = []
    for k, pl in enumerate(plan):                                     # the copies are laid as their founder is: the same record, run and positions
        c = pl["founder"]
        same = all(all(int(hv[f][COPIES * k + w]) == int(v[f][c]) for f in ("gene", "seq_start", "seq_end", "germ_start", "germ_end", "n_runs")) for w in range(COPIES))
        if same and len(keep) < FOUNDERS:
            keep.append(k)
    idx = [COPIES * k + w for w in range(COPIES) for k in keep]      # copy by copy, the founders interleaved
    sub = [batch[i] for i in idx]
    r = ctx.consensus(sub, {f: np.asarray(x)[idx] for f, x in hv.items()}, limit=[int(lim[plan[i // COPIES]["founder"]]) for i in idx],
                      group=[1000 - 7 * (i // COPIES) for i in idx], counts=True)
    ctx.close()
    out = []
    for u, k in enumerate(keep):
        c = plan[k]["founder"]
        a, b = int(v["seq_start"][c]) - 1, min(int(v["seq_end"][c]), int(lim[c]))
        g0 = int(v["germ_start"][c]) - 1
        rec = clean[int(v["gene"][c])][1]
        out.append(dict(cons=r["cons"][u], germ=r["germ"][u], want=plan[k]["truth"][a:b], founder=seqs[c][a:b], rec=rec[g0:g0 + b - a], lo=int(r["units"]["lo"][u]), g0=g0,
                        members=int(r["units"]["members"][u]), group=int(r["units"]["group"][u]), min_cover=int(min(r["cover"][u]))))
    return dict(found=len(found), kept=len(keep), units=out, info=r["info"])


def test_planted_sisters():
    res = _run_child("_device_sisters", "x", _child_env("shipped"))
    assert res["kept"] == FOUNDERS and res["info"]["units"] == FOUNDERS and res["info"]["off_record"] == 0, (res["found"], res["kept"], res["info"])
    assert len({u["group"] for u in res["units"]}) == FOUNDERS
    for k, u in enumerate(res["units"]):
        assert u["members"] == COPIES and u["min_cover"] == COPIES and u["lo"] == u["g0"]
        assert u["cons"] == u["want"], (k, [(i, a, b) for i, (a, b) in enumerate(zip(u["cons"], u["want"])) if a != b])
        assert u["germ"] == "".join(ch if ch in "ACGT" else "N" for ch in u["rec"])
        assert sum(a != b for a, b in zip(u["want"], u["founder"])) == len(SHARED)


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
            ctx.consensus([c["contig"] for c in cs2], SC.hits(cs2), **kw)
        return 1

    ctx = api.Context(0)
    with pytest.raises(VdjxError, match="vdjx_consensus: no germline set is loaded") as e:
        ctx.consensus([c["contig"] for c in pair()], SC.hits(pair()))
    assert "failed (-4)" in str(e.value)                              # VDJX_ESTATE
    done = 1
    ctx.germline_load(TM.records())
    vh = good["v"]
    hit = lambda h, **kw: dict(h, **kw)
    # one refused hit per message of the shared check, word for word what vdjx_targeting_counts says under its own name
    for cs2, msg in ((pair(v=hit(vh, gene=11)), "is not a V record of the loaded set"), (pair(v=hit(vh, gene=TM.J0)), "is not a V record of the loaded set"),
                     (pair(v=hit(vh, runs=[(100 << 4) | 3] + [0] * 63)), "a run with an op outside 0..2 or a length of 0"),
                     (pair(v=hit(vh, runs=[0] + [0] * 63)), "a run with an op outside 0..2 or a length of 0"),
                     (pair(v=hit(H(TM.V0, 1, 1, [("M", 9)]), seq_start=0, seq_end=8)), "contig positions 0 .. 8"),
                     (pair(v=H(TM.V0, 290, 1, [("M", 20)])), "contig positions 290 .. 309"),
                     (pair(v=H(TM.V2, 5, 1, [("M", 2)])), "germline positions 1 .. 2"),
                     (pair(v=hit(vh, seq_end=vh["seq_end"] + 1)), "runs hold"), (pair(v=hit(vh, germ_end=vh["germ_end"] + 1)), "runs hold")):
        with pytest.raises(VdjxError, match="vdjx_consensus: contig 1: the V hit") as con:
            ctx.consensus([c["contig"] for c in cs2], SC.hits(cs2))
        assert msg in str(con.value), (msg, str(con.value))
        with pytest.raises(VdjxError) as tgt:
            ctx.targeting_counts([c["contig"] for c in cs2], SC.hits(cs2))
        assert str(tgt.value).replace("vdjx_targeting_counts", "vdjx_consensus") == str(con.value)
        done += 1
    for bad in (-1, TM.LEN + 1):
        done += call(ctx, pair(), "vdjx_consensus: contig 1: limit", limit=[TM.LEN, bad])
    for freq in ((1, 0), (0, 1000001), (5, 4), (-1, 10)):
        done += call(ctx, pair(), "vdjx_consensus: the minimum share", min_freq=freq)
    with pytest.raises(VdjxError, match="^vdjx_consensus: 2 contigs, v\\['runs'\\] of shape"):
        ctx.consensus([c["contig"] for c in pair()], dict(SC.hits(pair()), runs=np.zeros((2, 63), np.int64)))
    with pytest.raises(VdjxError, match="group of shape"):
        ctx.consensus([c["contig"] for c in pair()], SC.hits(pair()), group=[0])
    two = pair()
    with pytest.raises(VdjxError, match="vdjx_consensus: contigs of unequal length"):
        ctx.consensus((two[0]["contig"].encode() + b"ACG\0" + two[1]["contig"].encode()[4:], 2, TM.LEN), SC.hits(two))
    with pytest.raises(VdjxError, match="vdjx_consensus: len=4096"):
        ctx.consensus(["A" * 4096], SC.hits([dict(v=TM.NONE)]))
    done += 4
    # NULL outputs: every required one, one at a time; the two optional ones may be NULL
    raw, n, ln = ctx.pack_strings([c["contig"] for c in pair()])
    hv = ctx._hit_array(SC.hits(pair()), 2, "v", "vdjx_consensus")
    bufs = [np.zeros(4096, np.uint8), np.zeros(4096, np.uint8), None, None, np.zeros(2, api.Context.CONS_UNIT), np.zeros(2, np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data
    for k in (0, 1, 4, 5):
        args = [ptr(b) if i != k else None for i, b in enumerate(bufs)]
        rc = ctx.L.vdjx_consensus(ctx.h, raw, 2, ln, hv.ctypes.data, None, None, None, *args, None)
        assert rc != 0 and b"vdjx_consensus: NULL argument" in ctx.L.vdjx_last_error()
        done += 1
    assert ctx.L.vdjx_consensus(ctx.h, raw, 2, ln, hv.ctypes.data, None, None, None, *[ptr(b) for b in bufs], None) == 0      # (params NULL: 0.6)
    big = 1 << 20
    zero = np.zeros(big, api.Context.ANNOT_HIT)
    units, unit = np.zeros(big, api.Context.CONS_UNIT), np.zeros(big, np.int32)
    rc = ctx.L.vdjx_consensus(ctx.h, b"A" * big, big, 1, zero.ctypes.data, None, None, None, ptr(bufs[0]), ptr(bufs[1]), None, None, units.ctypes.data, unit.ctypes.data, None)
    assert rc != 0 and b"2^20" in ctx.L.vdjx_last_error()
    # a refused call leaves the context usable
    ok = ctx.consensus([c["contig"] for c in pair()], SC.hits(pair()))
    assert ok["info"]["used"] == 2 and ok["info"]["units"] == 2
    ctx.close()
    return done + 2


def test_refusals_by_message():
    assert _run_child("_device_refusals", "x", _child_env("shipped")) == 1 + 9 + 2 + 4 + 4 + 4 + 2
