"""k_window_cover through vdjx_window_cover -- the entry point that takes pair lists as they are -- on the handmade windows of
tests/cover_cases.py (what each family is for: there and in tests/test_cover_cpu.py): every sub-rule of rule 1 at its edge, the private and
the shared histogram, windows of up to MAP_MAXOFF + rl bases with reads of up to 160, the bit grid and the difference arrays on the same
lists, delta batches, the chunked replay, the reference's array bounds, insert_low < insert_high, and lists that arrive as several sources.

Held: every verdict equals the oracle's (vdjo_coverage_is_valid on the rows the mapper would have made of the list), EXACTLY, named by
case; a second call gives the same bytes; a call is one k_window_cover launch; what the entry point refuses it refuses by message, and
the context answers the next call.  One leg goes through vdjx_window_score, the entry point real runs use, with reads of 151 bases and
windows of 1088, 1089 and 1175 bases.

Not reached: the replay's perm_stride = 1 branch (a list of 1,000,003 pairs in one window), batches of 3 deltas and `pos + delta > len +
1023` (tests/cover_cases.py says why no valid window gets there).

The API runs in one child process (one Context), the oracle here.  Measured on an MI355X: the child's work on the device (94 groups
twice, the source splits, the refusals and the end-to-end leg: 525 windows, 88,000 entries) takes 0.46 s, the child 2.4 s with its start,
the whole module 3.0 s.

That the cases bite was tried on scratch builds with one line broken: `cg >= i0 - fl` for `cg > i0 - fl` gave 89 wrong verdicts here (the
first: tiny_1_last_beyond+) and failed the source and the end-to-end tests too; a `req` mask one delta short gave 39 (the first:
forms_ms64_f1_high-)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import cover_cases as CC
from tests.test_gpu_annot import _child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = [(1, "one"), (2, "round"), (2, "one"), (3, "round"), (3, "one"), (3, "ends")]


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_cover import {fn}; print('COVER', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("COVER ")).split(" ", 1)[1])


def _cover(ctx, torch, ln, rl, par, parts_per_window, nsrc, null_lists=False):
    """one vdjx_window_cover call: parts_per_window[w][s] = the entries of window w that come from source s -> (verdicts, launches)"""
    n = len(parts_per_window)
    counts = np.array([[len(parts_per_window[w][s]) for w in range(n)] for s in range(nsrc)], np.uint32).reshape(nsrc, n)
    flat = [e for s in range(nsrc) for w in range(n) for e in parts_per_window[w][s]]          # source after source, window after window
    lists = torch.from_numpy(CC.pack(flat).view(np.int64).copy()).cuda() if flat else None
    ctx.profile_reset()
    valid = ctx.window_cover(n, ln, rl, 0 if (lists is None or null_lists) else lists.data_ptr(), nsrc, counts, par.lo, e0=par.e0, e1=par.e1, rs=par.rs,
                             ms=par.ms, floor=par.floor, ins_high=par.hi)
    launches = ctx.profile_get().get("k_window_cover", (0.0, 0))[1]
    return valid.tolist(), launches


def _device_all(_):
    import ctypes as C
    import torch
    from vdjer_amd import api
    from vdjer_amd._lib import CovParams
    t0 = time.perf_counter()
    ctx = api.Context(0)
    ctx.profile(True)
    out = dict(groups=[], splits=[], refusals={}, e2e=[])
    for (ln, rl, par), wins in CC.groups().items():
        whole = [[w.entries] for w in wins]
        a, la = _cover(ctx, torch, ln, rl, par, whole, 1)
        b, lb = _cover(ctx, torch, ln, rl, par, whole, 1)
        out["groups"].append(dict(names=[w.name for w in wins], valid=a, again=b, launches=[la, lb]))
    # the 70 windows of one geometry as 1, 2 and 3 sources
    mixed = [w for w in CC.singles() if w.family == "mixed"]
    ln, rl, par = mixed[0].group
    for nsrc, how in SPLITS:
        v, l = _cover(ctx, torch, ln, rl, par, [CC.split_sources(w.entries, nsrc, how) for w in mixed], nsrc)
        out["splits"].append(dict(nsrc=nsrc, how=how, valid=v, launches=l))
    # refusals; after each the context answers a good call
    good = [[w.entries] for w in mixed[:3]]
    want = _cover(ctx, torch, ln, rl, par, good, 1)[0]
    bad_calls = dict(
        rl_too_long=lambda: _cover(ctx, torch, CC.MAX_READ_LEN + 1 + 500, CC.MAX_READ_LEN + 1, par, good, 1),      # (nothing else is wrong with these two)
        rl_thousands=lambda: _cover(ctx, torch, 5000, 4000, par, good, 1),
        len_not_above_rl=lambda: _cover(ctx, torch, rl, rl, par, good, 1),
        len_too_long=lambda: _cover(ctx, torch, CC.MAP_MAXOFF + rl + 1, rl, par, good, 1),
        no_sources=lambda: api.check(ctx.L.vdjx_window_cover(ctx.h, 3, ln, rl, C.byref(CovParams(*par)), None, 0, np.zeros(3, np.uint32).ctypes.data_as(C.c_void_p),
                                                             np.zeros(3, np.uint8).ctypes.data_as(C.c_void_p)), "vdjx_window_cover"),
        null_lists=lambda: _cover(ctx, torch, ln, rl, par, good, 1, null_lists=True),
        eval_start_0=lambda: _cover(ctx, torch, ln, rl, par._replace(e0=0), good, 1),
        eval_stop_at_start=lambda: _cover(ctx, torch, ln, rl, par._replace(e1=par.e0), good, 1),
        eval_range_too_long=lambda: _cover(ctx, torch, ln, rl, par._replace(e1=par.e0 + CC.COV_WORDS), good, 1),
    )
    for name, call in bad_calls.items():
        try:
            call()
            msg = None
        except api.VdjxError as e:
            msg = str(e)
        out["refusals"][name] = dict(message=msg, then=_cover(ctx, torch, ln, rl, par, good, 1)[0] == want)
    # through vdjx_window_score: reads of 151 bases, windows of 1088, 1089 and 1175 bases
    pool, wins = CC.e2e_pool()
    p = ctx.pool_load(pool.primary, pool.secondary, pool.rl)
    ctx.read_index_build(p, pool.pair_id, pool.read_num, pool.is_rc, pool.reg_rank, pool.n_pairs)
    for ln, ws in wins:
        valid, npairs = ctx.window_score(ws, CC.E2E_INS, **CC.E2E_PARAMS)
        out["e2e"].append(dict(len=ln, valid=valid.tolist(), npairs=npairs.tolist()))
    p.free()
    ctx.close()
    out["seconds"] = round(time.perf_counter() - t0, 3)
    return out


@pytest.fixture(scope="module")
def device():
    t0 = time.perf_counter()
    d = _run_child("_device_all", 0, _child_env("shipped"))
    print("child: %.3f s of GPU work, %.3f s in all" % (d["seconds"], time.perf_counter() - t0))
    return d


def test_every_verdict_equals_the_oracle(device):
    wrong, seen = [], 0
    by_name = {w.name: w for w in CC.all_windows()}
    for g in device["groups"]:
        for name, v in zip(g["names"], g["valid"]):
            seen += 1
            if v != CC.verdict(by_name[name]):
                wrong.append((name, "kernel", v, "oracle", CC.verdict(by_name[name]), by_name[name]))
    assert seen == len(by_name) and len(device["groups"]) == len(CC.groups())
    assert not wrong, (len(wrong), wrong[:20])


def test_second_call_gives_the_same_bytes(device):
    for g in device["groups"]:
        assert g["again"] == g["valid"], g["names"][0]


def test_one_launch_per_call(device):
    for g in device["groups"]:
        assert g["launches"] == [1, 1], (g["names"][0], g["launches"])
    assert all(s["launches"] == 1 for s in device["splits"])


def test_sources_give_the_verdicts_of_their_union(device):
    """the 70 windows of one call (sizes 0 to 966, so the largest-first order is no identity) as 1, 2 and 3 sources: dealt out in turn,
    everything in the last source, and the middle source empty"""
    mixed = [w for w in CC.singles() if w.family == "mixed"]
    exp = [CC.verdict(w) for w in mixed]
    assert [(s["nsrc"], s["how"]) for s in device["splits"]] == SPLITS
    for s in device["splits"]:
        assert s["valid"] == exp, (s["nsrc"], s["how"], [(w.name, a, b) for w, a, b in zip(mixed, s["valid"], exp) if a != b])


@pytest.mark.parametrize("name,text", [("rl_too_long", "bad geometry"), ("rl_thousands", "bad geometry"), ("len_not_above_rl", "bad geometry"),
                                       ("len_too_long", "bad geometry"), ("no_sources", "bad geometry"), ("null_lists", "NULL lists"),
                                       ("eval_start_0", "bad eval range"), ("eval_stop_at_start", "bad eval range"),
                                       ("eval_range_too_long", "eval range too long")])
def test_refusals_by_message(device, name, text):
    r = device["refusals"][name]
    assert r["message"] is not None and "vdjx_window_cover" in r["message"] and text in r["message"], (name, r)
    assert r["then"], (name, "the context no longer answers a good call")


def test_window_score_on_long_windows_with_long_reads(device):
    """vdjx_window_score, reads of 151 bases tiled over one transcript, windows of 1088, 1089 and 1175 bases: pair counts and verdicts
    against oracle.ReadIndex (tests/test_cover_cpu.py holds that both verdicts occur at every length)"""
    from oracle import oracle
    pool, wins = CC.e2e_pool()
    ix = oracle.ReadIndex(pool)
    assert [d["len"] for d in device["e2e"]] == list(CC.E2E_LENS)
    for (ln, ws), d in zip(wins, device["e2e"]):
        for i, w in enumerate(ws):
            pairs, starts = ix.quick_map(w)
            exp = ix.coverage_is_valid(starts, len(w), CC.E2E_INS, **CC.E2E_PARAMS)
            assert d["npairs"][i] == len(pairs) and d["valid"][i] == exp, (ln, i, d["npairs"][i], len(pairs), d["valid"][i], exp)
        assert set(d["valid"]) == {0, 1}, (ln, d["valid"])
