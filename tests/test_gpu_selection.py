"""vdjx_selection on the GPU: the counts and weights bit for bit against the integer model of tests/selection_model.py on the handmade hits
of tests/test_gpu_mutation.py and a call of its own (tests/selection_cases.py), three ways (uniform and seeded weights up to 2^32 - 1, with
and without a region map); the posterior of every row -- contigs, groups of 0, 1, 3, 4, 5 and 9 members, all contigs -- against the
model's 80-bit one within the derived bound, at VDJX_SEL_CHUNK 1024 and 4; the quantiles for equality (the margins: tests/
test_selection_cpu.py); the same bits from two calls; the refusals by message.  The API runs in child processes, once per knob setting."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import selection_cases as SC
from tests import selection_model as S
from tests import test_gpu_mutation as TM
from tests.test_gpu_annot import KNOBS, _child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = SC.CALL
# |pdf_device - pdf_model| <= 8 * 2^-52 * A * peak (selection_model.tolerance).  The largest ratio of a deviation to its bound measured on an
# MI355X over every row, region and chunk setting of this file is MEASURED_RATIO (0.0136 at VDJX_SEL_CHUNK 1024 and at 4; the test prints it).
MEASURED_RATIO = 0.0136


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_selection import {fn}; print('SEL', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("SEL ")).split(" ", 1)[1])


def _sub(h, sl):
    return {f: x[sl] for f, x in h.items()}


def _ctx():
    from vdjer_amd import api
    ctx = api.Context(0)
    ctx.germline_load(TM.records())
    return ctx


# ---- the counts ----------------------------------------------------------------------------------------------------------------------------
def _device_counts(_):
    ctx = _ctx()
    cs = SC.count_cases()
    ct, v, j = [c["contig"] for c in cs], SC.hits(cs), SC.hits(cs, "j")
    lim = np.array([c["limit"] for c in cs], np.int32)
    out = {}
    ctx.profile(True)
    for weighted in (False, True):
        for mapped in (False, True):
            calls = []
            for a in range(0, len(cs), CALL):
                sl = slice(a, a + CALL)
                kw = dict(limit=lim[sl], cdr=SC.region_map() if mapped else None, weight=SC.weights() if weighted else None)
                ctx.profile_reset()
                r = ctx.selection(ct[sl], _sub(v, sl), **kw)
                launches = {k: x[1] for k, x in ctx.profile_get().items()}
                assert launches == {"k_sel_counts": 1, "k_sel_finish": 1}, launches
                again = ctx.selection(ct[sl], _sub(v, sl), **kw)
                for f, x in r["counts"].items():
                    assert again["counts"][f].tobytes() == x.tobytes(), (a, f)
                for f, x in r["stat"].items():
                    assert again["stat"][f].tobytes() == x.tobytes() and x.shape == (CALL + 1, 2 if mapped else 1), (a, f)
                m = ctx.mutations(ct[sl], _sub(v, sl), _sub(j, sl), limit=lim[sl], rows=False)["counts"]
                take = (r["counts"]["flags"] & 1) > 0
                for f, g in (("obs_r", "v_r"), ("obs_s", "v_s"), ("codons", "v_codons")):
                    assert np.array_equal(r["counts"][f].sum(axis=1)[take], m[g][take]), (weighted, mapped, a, f)
                assert r["info"]["contigs"] == CALL and r["info"]["regions"] == (2 if mapped else 1) and r["info"]["chunks"] == 0
                calls.append(dict({f: x.tolist() for f, x in r["counts"].items()}, info=r["info"]))
            out[f"{int(weighted)}{int(mapped)}"] = calls
    ctx.profile(False)
    r0 = ctx.selection([], SC.hits([]))
    assert r0["counts"]["flags"].shape == (0,) and not any(r0["info"].values())
    ctx.close()
    return out


@pytest.mark.parametrize("knobs", KNOBS)
def test_counts_bitwise_vs_model(knobs):
    res = _run_child("_device_counts", "x", _child_env(knobs))
    cs = SC.count_cases()
    assert len(cs) % CALL == 0 and len(cs) // CALL == 5
    for weighted in (False, True):
        for mapped in (False, True):
            want = SC.count_model(weighted, mapped)
            for k, dev in enumerate(res[f"{int(weighted)}{int(mapped)}"]):
                sl = slice(k * CALL, (k + 1) * CALL)
                for f in ("obs_r", "obs_s", "codons", "exp_r", "exp_s"):
                    a, b = [[int(y) for y in row] for row in dev[f]], [[int(y) for y in row] for row in want[f][sl]]
                    assert a == b, (weighted, mapped, k, f, [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:3])
                assert dev["flags"] == [int(x) for x in want["flags"][sl]], (weighted, mapped, k)
                part = {f: want[f][sl] for f in want}
                assert {f: dev["info"][f] for f in ("contigs", "used", "no_regions", "truncated", "groups", "regions")} == S.info(part, 0, 2 if mapped else 1)


# ---- the posterior -------------------------------------------------------------------------------------------------------------------------
def _device_posterior(path):
    ctx = _ctx()
    cs, group = SC.posterior_cases()
    ct, v = [c["contig"] for c in cs], SC.hits(cs)
    kw = dict(cdr=SC.posterior_map(), weight=SC.weights(True), pdf=True)
    runs = {"main": dict(group=group, groups=SC.PGROUPS), "one": dict(group=np.zeros(len(cs), np.int32), groups=1),
            "own": dict(group=np.arange(len(cs), dtype=np.int32), groups=len(cs))}
    save, infos = {}, {}
    for name, g in runs.items():
        r = ctx.selection(ct, v, **kw, **g)
        again = ctx.selection(ct, v, **kw, **g)
        assert again["pdf"].tobytes() == r["pdf"].tobytes() and all(again["stat"][f].tobytes() == x.tobytes() for f, x in r["stat"].items())
        assert ctx.stat("selection_chunks") == r["info"]["chunks"] and ctx.stat("selection_us") > 0
        infos[name] = r["info"]
        save[name + "_pdf"] = r["pdf"]
        for f, x in r["stat"].items():
            save[f"{name}_{f}"] = x
        for f, x in r["counts"].items():
            save[f"{name}_c_{f}"] = x
    ctx.close()
    np.savez(path, **save)
    return infos


def _check_rows(dev, name, rows, pdf_rows, worst):
    """rows: the model's [R][2]; pdf_rows: the indices of the rows whose density came back, in order"""
    for r, row in enumerate(rows):
        for k, p in enumerate(row):
            for f, g in (("sequences", "sequences"), ("x", "x"), ("n", "n"), ("exp_r", "exp_r"), ("exp_s", "exp_s")):
                assert int(dev[f"{name}_{f}"][r, k]) == p[g], (name, r, k, f)
            tol = S.tolerance(p["A"])
            ds = abs(float(dev[f"{name}_sigma"][r, k]) - float(p["sigma"]))
            dp = abs(float(dev[f"{name}_p_positive"][r, k]) - float(p["p_positive"]))
            assert ds <= 40 * tol and dp <= 2 * tol, (name, r, k, ds, dp, tol)
            assert float(dev[f"{name}_lower"][r, k]) == p["lower"] and float(dev[f"{name}_upper"][r, k]) == p["upper"], (name, r, k)
            worst[0] = max(worst[0], ds / (40 * tol), dp / (2 * tol))
            if r in pdf_rows:
                got = dev[f"{name}_pdf"][pdf_rows.index(r), k]
                dev_pdf = float(np.abs(got.astype(S.LD) - p["pdf"]).max() / p["pdf"].max())
                assert dev_pdf <= tol, (name, r, k, dev_pdf, tol)
                worst[0] = max(worst[0], dev_pdf / tol)
                assert abs(float(got.sum()) * 0.01 - 1.0) < 1e-12


@pytest.mark.parametrize("chunk", [1024, 4])
def test_posterior_vs_model(chunk, tmp_path):
    path = str(tmp_path / "dev.npz")
    infos = _run_child("_device_posterior", path, _child_env("shipped", VDJX_SEL_CHUNK=str(chunk)))
    dev = np.load(path)
    main, one = SC.posterior_model(False), SC.posterior_model(True)
    n, G = 26, SC.PGROUPS
    want = SC.posterior_counts()
    for f in ("obs_r", "obs_s", "codons", "exp_r", "exp_s"):
        assert [[int(y) for y in row] for row in dev[f"main_c_{f}"]] == [[int(y) for y in row] for row in want[f]], f
    worst = [0.0]
    _check_rows(dev, "main", main, list(range(n, n + G + 1)), worst)
    _check_rows(dev, "one", one, [n, n + 1], worst)
    _check_rows(dev, "own", main[:n] + main[:n] + [main[-1]], list(range(n, 2 * n + 1)), worst)
    print(f"vdjx_selection, VDJX_SEL_CHUNK={chunk}: the largest deviation is {worst[0]:.3g} of its bound")
    # rows of more than `chunk` members go through partial sums, per region: at 4 the sample (26: 7 chunks), the groups of 9 (3) and 5 (2)
    # -- a group of 4 does not --, with one group that group and the sample
    assert {k: (i["chunks"], i["large_rows"]) for k, i in infos.items()} == (
        {"main": (24, 3), "one": (28, 2), "own": (14, 1)} if chunk == 4 else {"main": (0, 0), "one": (0, 0), "own": (0, 0)})
    assert all(i["regions"] == 2 and i["contigs"] == n and i["used"] == n for i in infos.values()) and infos["main"]["groups"] == G
    # the prior alone, where no member contributes
    assert abs(float(dev["main_sigma"][n, 0])) < 1e-12 and abs(float(dev["main_p_positive"][n + 6, 1]) - 0.5) < 1e-12


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------
def _device_refusals(_):
    import ctypes as C
    from vdjer_amd import api
    from vdjer_amd._lib import VdjxError
    cs = SC.count_cases()
    good = [c for c in cs if c["name"] == "frame1"][0]
    H = TM.H

    def pair(**kw):
        return [good, dict(good, **kw)]

    def call(ctx, cs2, match, **kw):
        with pytest.raises(VdjxError, match=match):
            ctx.selection([c["contig"] for c in cs2], SC.hits(cs2), **kw)
        return 1

    ctx = api.Context(0)
    done = call(ctx, pair(), "no germline set")
    ctx.germline_load(TM.records())
    vh = good["v"]
    hit = lambda h, **kw: dict(h, **kw)
    by_layout = 0
    for cs2 in (pair(v=hit(vh, gene=11)), pair(v=hit(vh, gene=TM.J0)), pair(v=hit(vh, gene=TM.C1)), pair(v=H(TM.V2, 5, 1, [("M", 2)])),
                pair(v=hit(H(TM.V0, 1, 1, [("M", 9)]), seq_start=0, seq_end=8)), pair(v=hit(H(TM.V0, 5, 1, [("M", 9)]), germ_start=0, germ_end=8)),
                pair(v=H(TM.V0, 290, 1, [("M", 20)])), pair(v=hit(vh, runs=[(100 << 4) | 3] + [0] * 63)), pair(v=hit(vh, runs=[0] + [0] * 63)),
                pair(v=hit(vh, seq_end=vh["seq_end"] + 1)), pair(v=hit(vh, germ_end=vh["germ_end"] + 1))):
        with pytest.raises(VdjxError, match="vdjx_selection: contig 1") as sel:
            ctx.selection([c["contig"] for c in cs2], SC.hits(cs2))
        done += 1
        # one hit check behind both calls: where vdjx_mutations refuses the same V hit (J: none), it says the same under its own name.
        # A run with a bad op or a length of 0 never reaches it: vdjx_mutations_layout meets it first.
        with pytest.raises(VdjxError) as mut:
            ctx.mutations([c["contig"] for c in cs2], SC.hits(cs2), SC.hits([dict(j=TM.NONE)] * 2, "j"))
        if str(mut.value).startswith("vdjx_mutations_layout"):
            by_layout += 1
        else:
            assert str(mut.value) == str(sel.value).replace("vdjx_selection", "vdjx_mutations")
            done += 1
    assert by_layout == 2
    with pytest.raises(VdjxError, match="^vdjx_selection: 2 contigs, v\\['runs'\\] of shape"):        # the caller's name in _hit_array's message
        ctx.selection([c["contig"] for c in pair()], dict(SC.hits(pair()), runs=np.zeros((2, 63), np.int64)))
    done += 1
    for bad in (-1, TM.LEN + 1):
        done += call(ctx, pair(), "contig 1: limit", limit=[TM.LEN, bad])
    two = pair()
    with pytest.raises(VdjxError, match="NUL"):
        ctx.selection((two[0]["contig"].encode() + b"ACG\0" + two[1]["contig"].encode()[4:], 2, TM.LEN), SC.hits(two))
    with pytest.raises(VdjxError, match="len=4096"):
        ctx.selection(["A" * 4096], SC.hits([dict(v=TM.NONE)]))
    done += 2
    m = SC.region_map()
    done += call(ctx, pair(), "a region map of 10 records, 11 records were loaded", cdr=m[:10])

    def with_row(r, iv):
        x = m.copy()
        x[r] = iv
        return x

    done += call(ctx, pair(), "record 0: the interval 40 .. 35", cdr=with_row(TM.V0, (40, 35, 0, 0)))
    done += call(ctx, pair(), "record 0: the interval 300 .. 361", cdr=with_row(TM.V0, (1, 2, 300, 361)))
    done += call(ctx, pair(), "record 3: the interval 0 .. 1", cdr=with_row(TM.V2, (0, 1, 0, 0)))
    ok = ctx.selection([c["contig"] for c in pair()], SC.hits(pair()), cdr=with_row(TM.J0, (9, 1, 9999, 3)))       # (no V record: not read)
    assert ok["info"]["used"] == 2
    done += call(ctx, pair(), "contig 1: group 2 of 2", group=[0, 2], groups=2)
    done += call(ctx, pair(), "1048576 groups", group=[0, 1], groups=1 << 20)
    done += call(ctx, pair(), "densities of 65536 groups", group=[0, 1], groups=65536, pdf=True)
    raw, n, ln = ctx.pack_strings([c["contig"] for c in pair()])
    hv = ctx._hit_array(SC.hits(pair()), 2, "v", "vdjx_selection")
    cnt, st = np.zeros(2, api.Context.SEL_COUNTS), np.zeros((3, 1), api.Context.SEL_STAT)
    for a, b in ((None, st.ctypes.data), (cnt.ctypes.data, None)):
        rc = ctx.L.vdjx_selection(ctx.h, raw, 2, ln, hv.ctypes.data, None, None, 0, None, None, 0, a, b, None, None)
        assert rc != 0 and b"vdjx_selection: NULL argument" in ctx.L.vdjx_last_error()
        done += 1
    big = 1 << 20
    zero = np.zeros(big, api.Context.ANNOT_HIT)
    rc = ctx.L.vdjx_selection(ctx.h, b"A" * big, big, 1, zero.ctypes.data, None, None, 0, None, None, 0, cnt.ctypes.data, st.ctypes.data, None, None)
    assert rc != 0 and b"2^20" in ctx.L.vdjx_last_error()
    ctx.close()
    return done + 1


def test_refusals_by_message():
    assert _run_child("_device_refusals", "x", _child_env("shipped")) == 36
