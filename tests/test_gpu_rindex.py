"""vdjx_read_index_build on the handmade pools of tests/rindex_cases.py (what each is for: tests/test_rindex_cpu.py): every folding route of
k_ri_fold_members and k_ri_fold_big -- a thread per member, a wave's table, a workgroup's table, the unfolded overflow --, multiplicities cut
into pieces of 255, s_big[] at its limit, reads that are their own reverse complement, pairs with one read-2 record or an N, and the three
member orders (as recorded, a merge of two runs, a sort by rank), each under the couples build, the general build (VDJX_NO_SYM_INDEX=1) and,
for sizes / pieces / overflow, the long-read build (rl 100).

Held per case and build: window_score's pair counts and verdicts and every field of every pair of map_emit, in order, against the oracle;
window_pairs' entries per window -- the direct view of the fold: a pair planted 600 times is 3 entries folded and 600 unfolded -- and the
index's counts against the model.  EXACTLY, the overflow cases included: k_ri_fold_big reads the fill of its table once per row of 512
members, between two barriers, and every member of a row before is in the table by then, so the row at which a class starts to leave
unfolded is a function of the class alone (the model walks the same rows); the overflow cases must also show more entries than the folded
minimum.  A second build of the same pool in the same context (the index arrays are recycled) gives the same.

The API runs in one child process per build (one Context each), all its cases in turn; the oracle and the model run here, once per case."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import rindex_cases as RC
from tests.test_gpu_annot import _child_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("pair_id", "rec1", "rec2", "pos1", "pos2", "insert", "rc1", "rc2")
STATS = ("read_index_sym", "read_index_r1_members", "read_index_r1_distinct", "read_index_classes", "read_index_rank_order")


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_rindex import {fn}; print('RINDEX', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RINDEX ")).split(" ", 1)[1])


def _device_build(build):
    """every case of the build: index, scores, mapped pairs, entries and counts; twice per pool"""
    from vdjer_amd import api
    rl, names = RC.BUILDS[build]
    assert (os.environ.get("VDJX_NO_SYM_INDEX") == "1") == (build == "general")
    ctx = api.Context(0)
    out = {}
    for name in names:
        c = RC.case(name, rl)
        pool = c.pool
        t0 = time.perf_counter()
        p = ctx.pool_load(pool.primary, pool.secondary, rl)
        turns = []
        for _ in range(2):
            ctx.read_index_build(p, pool.pair_id, pool.read_num, pool.is_rc, pool.reg_rank, pool.n_pairs)
            stats = {s: int(ctx.stat(s)) for s in STATS}
            valid, npairs = ctx.window_score(c.wins, RC.INS)
            offs, pairs = ctx.map_emit(c.wins)
            ent, np2 = ctx.window_pairs(c.wins)
            turns.append(dict(stats=stats, symmetric=int(ctx.stat("pool_symmetric")), valid=valid.tolist(), npairs=npairs.tolist(), offs=offs.tolist(),
                              pairs={f: pairs[f].tolist() for f in FIELDS}, entries=ent.tolist(), npairs_of_window_pairs=np2.tolist()))
        p.free()
        out[name] = dict(turns[0], again=turns[1] == turns[0], seconds=round(time.perf_counter() - t0, 3))
    ctx.close()
    return out


@pytest.fixture(scope="module")
def device():
    """build -> case -> what the device gave (a child per build, run when the build is first asked for)"""
    got = {}

    def get(build):
        if build not in got:
            env = _child_env("shipped")
            env.pop("VDJX_NO_SYM_INDEX", None)
            env.pop("VDJX_NO_SYM", None)
            env.pop("VDJX_WINDOW_GROUP", None)
            if build == "general":
                env["VDJX_NO_SYM_INDEX"] = "1"           # (read per build)
            got[build] = _run_child("_device_build", build, env)
            print(build, {n: d["seconds"] for n, d in got[build].items()})
        return got[build]

    return get


CASES = [(b, n) for b, (_, names) in RC.BUILDS.items() for n in names]


@pytest.mark.parametrize("build,name", CASES)
def test_index_of_case_vs_oracle_and_model(device, build, name):
    rl = RC.BUILDS[build][0]
    c = RC.case(name, rl)
    m = c.model
    d = device(build)[name]
    what = (build, name)
    # the kind of build
    assert d["symmetric"] == (1 if rl <= 64 else 0) and d["stats"]["read_index_sym"] == (1 if build == "couples" else 0), what
    # the counts of the index
    assert d["stats"]["read_index_r1_members"] == m.r1_members, what
    assert d["stats"]["read_index_classes"] == (m.classes_couples if build == "couples" else m.classes_general), what
    assert d["stats"]["read_index_rank_order"] == m.rank_order, what
    print(what, "entries", d["stats"]["read_index_r1_distinct"], "model", m.entries(), "folded minimum", m.entries_folded_minimum(), "members", m.r1_members)
    assert d["stats"]["read_index_r1_distinct"] == m.entries(), what
    if name in RC.OVERFLOWS and name != "overflow_at_6144":
        assert m.entries_folded_minimum() < d["stats"]["read_index_r1_distinct"] <= m.r1_members, what      # the overflow ran
    else:
        assert d["stats"]["read_index_r1_distinct"] == m.entries_folded_minimum(), what
    # scores, mapped pairs and entries of every string
    offs = d["offs"]
    for i, (w, (pairs, valid)) in enumerate(zip(c.wins, RC.oracle_results(name, rl))):
        assert d["npairs"][i] == len(pairs) and d["valid"][i] == valid, (what, i, d["npairs"][i], len(pairs), d["valid"][i], valid)
        assert offs[i + 1] - offs[i] == d["npairs"][i], (what, i, "map_emit's count")
        for f in FIELDS:
            got = d["pairs"][f][offs[i]:offs[i + 1]]
            assert got == pairs[f].astype(np.int64).tolist(), (what, i, f, [(j, a, b) for j, (a, b) in enumerate(zip(got, pairs[f].tolist())) if a != b][:5])
        ent, npairs, _ = m.window(w)
        assert npairs == len(pairs)
        assert d["npairs_of_window_pairs"][i] == npairs and d["entries"][i] == ent, (what, i, "window_pairs", d["entries"][i], ent, d["npairs_of_window_pairs"][i], npairs)
    assert set(d["valid"]) >= set(c.verdicts), what
    assert d["again"], (what, "a second build of the same pool in the same context gives something else")


@pytest.mark.parametrize("build", ["couples", "general"])
def test_member_orders_give_the_same_index(device, build):
    """the `sizes` pool laid out five ways, every record with the same registration rank: as recorded (read_index_rank_order 0), two runs
    (1: a merge; with all read-1 members in the first run and with none there, too), permuted (2: a sort).  Registration order is what the
    CSR promises: the same pairs in the same order, by pair id and positions (the records are numbered by the layout)"""
    got = device(build)
    first = got[RC.ORDERS[0]]
    seen = set()
    for name in RC.ORDERS:
        d = got[name]
        seen.add(d["stats"]["read_index_rank_order"])
        assert d["stats"]["read_index_rank_order"] == RC.case(name).model.rank_order, name
        assert d["npairs"] == first["npairs"] and d["valid"] == first["valid"] and d["offs"] == first["offs"] and d["entries"] == first["entries"], name
        for f in FIELDS:
            if not f.startswith("rec"):
                assert d["pairs"][f] == first["pairs"][f], (name, f)
        for s in STATS[1:4]:
            assert d["stats"][s] == first["stats"][s], (name, s)
    assert seen == {0, 1, 2}
