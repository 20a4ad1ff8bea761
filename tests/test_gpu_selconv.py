"""vdjx_selection_convolve on the device against tests/selection_conv_model.py (np.longdouble): handmade count rows (tests/
selection_conv_cases.py), every group and sample row of every case within the bound E that the model carries through the tree
(tests/test_selection_conv_cpu.py asserts, without a GPU, that E stays small against the row's peak and clear of the quantiles'
thresholds); the same bytes from a second call and from VDJX_CONV_CELLS=4, where rows are streamed block by block; a group of one member
against vdjx_selection's own density of that contig; and the refusals by message.  The API runs in child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import selection_conv_cases as CC
from tests import selection_conv_model as CM
from tests import selection_model as S
from tests.test_gpu_annot import _child_env
from tests.test_selection_conv_cpu import model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The largest ratio of a device deviation (mass, sigma, p_positive) to its bound measured on an MI355X over every row of this file; the test
# prints it (0.00174: a mass cell of a single-member row; the combined rows stay under 0.001).
MEASURED_RATIO = 0.00174


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_selconv import {fn}; print('SELCONV', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("SELCONV ")).split(" ", 1)[1])


def _same(a, b):
    return a["pdf"].tobytes() == b["pdf"].tobytes() and all(b["stat"][f].tobytes() == x.tobytes() for f, x in a["stat"].items())


def _device_cases(path):
    from vdjer_amd import api
    ctx = api.Context(0)
    save, infos = {}, {}
    for name, make in CC.CASES.items():
        c = make()
        os.environ.pop("VDJX_CONV_CELLS", None)
        r = ctx.selection_convolve(c["counts"], c["K"], c["group"], c["G"], pdf=True)
        assert ctx.stat("selconv_combines") == r["info"]["combines"] and ctx.stat("selconv_batches") == r["info"]["batches"] and ctx.stat("selconv_us") > 0
        assert _same(r, ctx.selection_convolve(c["counts"], c["K"], c["group"], c["G"], pdf=True)), name
        bare = ctx.selection_convolve(c["counts"], c["K"], c["group"], c["G"])
        assert bare["pdf"] is None and all(bare["stat"][f].tobytes() == x.tobytes() for f, x in r["stat"].items()), name
        os.environ["VDJX_CONV_CELLS"] = "4"                        # (read per call)
        small = ctx.selection_convolve(c["counts"], c["K"], c["group"], c["G"], pdf=True)
        assert _same(r, small) and _same(small, ctx.selection_convolve(c["counts"], c["K"], c["group"], c["G"], pdf=True)), name
        os.environ["VDJX_CONV_CELLS"] = "9"
        assert _same(r, ctx.selection_convolve(c["counts"], c["K"], c["group"], c["G"], pdf=True)), name
        os.environ.pop("VDJX_CONV_CELLS")
        infos[name] = dict(r["info"], batches_small=small["info"]["batches"], same_info={k: v for k, v in small["info"].items() if k != "batches"}
                           == {k: v for k, v in r["info"].items() if k != "batches"})
        save[name + "_pdf"] = r["pdf"]
        for f, x in r["stat"].items():
            save[f"{name}_{f}"] = x
    r0 = ctx.selection_convolve(dict(obs_r=np.zeros((0, 2)), obs_s=np.zeros((0, 2)), exp_r=np.zeros((0, 2)), exp_s=np.zeros((0, 2))), 2)
    assert not any(r0["info"].values())
    ctx.close()
    np.savez(path, **save)
    return infos


def test_cases_vs_model(tmp_path):
    path = str(tmp_path / "dev.npz")
    infos = _run_child("_device_cases", path, _child_env("shipped"))
    dev = np.load(path)
    worst = 0.0
    for name in CC.CASES:
        c, rows = model(name)
        want = CM.info(rows, c["G"], c["K"])
        got = infos[name]
        assert {k: got[k] for k in want} == want, (name, got, want)
        assert got["same_info"] and got["batches"] == 1 and got["batches_small"] > 1, (name, got)
        for r, row in enumerate(rows):
            for k, p in enumerate(row):
                for f in ("sequences", "x", "n", "exp_r", "exp_s"):
                    assert int(dev[f"{name}_{f}"][r, k]) == p[f], (name, r, k, f)
                E = p["E"]
                mass = dev[f"{name}_pdf"][r, k].astype(CM.LD) * CM.LD(0.01)
                dm = float(np.abs(mass - p["mass"]).max())
                ds = abs(float(dev[f"{name}_sigma"][r, k]) - float(p["sigma"]))
                dp = abs(float(dev[f"{name}_p_positive"][r, k]) - float(p["p_positive"]))
                print(f"{name} row {r} region {k}: mass {dm / E:.3g}, sigma {ds / (40020 * E):.3g}, p_positive {dp / (2001 * E):.3g} of the bound")
                assert dm <= E, (name, r, k, dm, E)
                assert ds <= 40020 * E and dp <= 2001 * E, (name, r, k, ds, dp, E)
                assert float(dev[f"{name}_lower"][r, k]) == p["lower"] and float(dev[f"{name}_upper"][r, k]) == p["upper"], (name, r, k)
                assert abs(float(dev[f"{name}_pdf"][r, k].sum()) * 0.01 - 1.0) < 1e-12
                worst = max(worst, dm / E, ds / (40020 * E), dp / (2001 * E))
    print(f"vdjx_selection_convolve: the largest deviation is {worst:.3g} of its bound")
    # the empty group is the prior; the two ends keep their mass on the last grid points
    assert abs(float(dev["a_sigma"][0, 0])) < 1e-12 and abs(float(dev["a_p_positive"][0, 1]) - 0.5) < 1e-12
    assert int(np.argmax(dev["ends_pdf"][0, 0])) == 4000 and int(np.argmax(dev["ends_pdf"][1, 0])) == 0


def _device_single(_):
    """every contig of tests/selection_cases.py's posterior cases as a group of its own: vdjx_selection's density of the group against
    vdjx_selection_convolve's, which is that member's leaf -> the largest difference over its bound E(leaf)"""
    from tests import selection_cases as SC
    from tests.test_gpu_selection import _ctx
    ctx = _ctx()
    cs, _ = SC.posterior_cases()
    ct, v = [c["contig"] for c in cs], SC.hits(cs)
    n = len(cs)
    own = np.arange(n, dtype=np.int32)
    sel = ctx.selection(ct, v, cdr=SC.posterior_map(), weight=SC.weights(True), pdf=True, group=own, groups=n)
    conv = ctx.selection_convolve(sel["counts"], 2, own, n, pdf=True)
    ctx.close()
    mem = S.members(sel["counts"], 2)
    worst, seen = 0.0, 0
    for i in range(n):
        for k in range(2):
            a, b = sel["pdf"][i, k] * 0.01, conv["pdf"][i, k] * 0.01
            for f in ("sequences", "x", "n", "exp_r", "exp_s", "lower", "upper"):
                assert sel["stat"][f][n + i, k] == conv["stat"][f][i, k], (i, k, f)
            A = 40.0 if mem[k][i] is None else 40.0 + mem[k][i][1] * (20.0 + abs(float(np.log(mem[k][i][2]) - np.log(mem[k][i][3]))))
            E = S.tolerance(A) * float(a.max())
            worst = max(worst, float(np.abs(a - b).max()) / E)
            assert abs(float(sel["stat"]["sigma"][n + i, k]) - float(conv["stat"]["sigma"][i, k])) <= 40020 * E
            seen += mem[k][i] is not None
    # the sample rows differ: a shared sigma there, the mean of the members' here
    assert seen > n and abs(float(sel["stat"]["sigma"][2 * n, 0]) - float(conv["stat"]["sigma"][n, 0])) > 1e-6
    return worst


def test_single_member_is_selections_density():
    worst = _run_child("_device_single", "x", _child_env("shipped"))
    print(f"a group of one member against vdjx_selection's density: {worst:.3g} of E(leaf)")
    assert worst <= 1.0


def _device_refusals(_):
    import ctypes as C

    from vdjer_amd import _lib, api
    from vdjer_amd.api import VdjxError
    ctx = api.Context(0)
    c = CC.call_b()
    out = []

    def refused(what, fn):
        try:
            fn()
        except VdjxError as e:
            out.append([what, str(e)])
        else:
            out.append([what, "ACCEPTED"])

    refused("K0", lambda: ctx.selection_convolve(c["counts"], 0, c["group"], c["G"]))
    refused("K3", lambda: ctx.selection_convolve(c["counts"], 3, c["group"], c["G"]))
    refused("group", lambda: ctx.selection_convolve(c["counts"], 1, c["group"], 2))
    refused("G", lambda: ctx.selection_convolve(c["counts"], 1, c["group"], 1 << 20))
    refused("nogroup", lambda: ctx.selection_convolve(c["counts"], 1, None, 3))
    refused("pdf", lambda: ctx.selection_convolve(c["counts"], 1, c["group"], 65536, pdf=True))
    big = 1 << 20
    z = np.zeros((big, 2))
    refused("n", lambda: ctx.selection_convolve(dict(obs_r=z, obs_s=z, exp_r=z, exp_s=z), 1))
    raw = np.zeros(4, api.Context.SEL_COUNTS)
    stat = np.zeros((1, 1), api.Context.SEL_STAT)
    L = _lib.lib()
    for what, a, b in (("counts", None, stat.ctypes.data_as(C.c_void_p)), ("stat", raw.ctypes.data_as(C.c_void_p), None)):
        rc = L.vdjx_selection_convolve(ctx.h, a, 4, 1, None, 0, b, None, None)
        L.vdjx_last_error.restype = C.c_char_p
        out.append([what, L.vdjx_last_error().decode() if rc else "ACCEPTED"])
    # a refusal leaves the context usable
    ok = ctx.selection_convolve(c["counts"], 1, c["group"], c["G"])
    ctx.close()
    return dict(refusals=out, after=ok["info"]["rows"])


def test_refusals_by_message():
    res = _run_child("_device_refusals", "x", _child_env("shipped"))
    want = {"K0": "0 regions (1 or 2)", "K3": "3 regions (1 or 2)", "group": "group 2 of 2", "G": "1048576 groups (at most 2^20 - 1)",
            "nogroup": "3 groups and no group array", "pdf": "densities of 65536 groups and the sample (at most 65536 rows)",
            "n": "1048576 contigs (at most 2^20 - 1)", "counts": "NULL argument", "stat": "NULL argument"}
    got = dict(res["refusals"])
    assert set(got) == set(want)
    for k, msg in want.items():
        assert "vdjx_selection_convolve" in got[k] and msg in got[k], (k, got[k])
    assert res["after"] == 4
