"""The HIP stages judged by the compiled reference itself, where they have only been judged by the oracle: the configurations of
tests/test_oracle_vs_reference_live.py (same draws from the same seeds, the first six to eight of each), live against
oracle/_ref/vdjer_ref where it was built (tests/ref_live.py), and the edges_* fixtures everywhere.  Bit-exact throughout.

The symmetric form of the build exists for pools of couples with reads of at most 64 bases and odd k (vdjx_kmer.hip: build_sym);
every graph test asserts which form ran, so that even k provably took the other one on a pool the symmetric one would take.
The scorer leg runs twice: under the suite's knobs (tests/conftest.py) and, in a child process, under the shipped ones."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ref_live as R
from tests.test_gpu_annot import _child_env
from tests.test_oracle_vs_reference_live import GRAPH_RUNS, MAP_RUN, SCORE_RUN, graph_mode_conditions, map_conditions

pytestmark = pytest.mark.gpu
live = pytest.mark.skipif(not R.available(), reason=R.SKIP_REASON)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_N = {"mq_edges": 6}             # configurations per graph test (every --mq edge once); the other modes take 8
GPU_N_MAP, GPU_N_SCORE = 8, 8


@pytest.fixture(scope="module")
def ctx():
    from vdjer_amd import api
    c = api.Context(0)
    yield c
    c.close()


def check_graph(ctx, c, rep, pool, pre, surv, nodes):
    """ctx.kmer_build against a graph dump, as test_gpu_parity.test_kmer_build_vs_reference_dump compares them"""
    k = c["k"]
    vc, jc = R.codes(rep)
    ctx.anchor_sets_load(vc, jc)
    p = ctx.pool_load(pool.primary, pool.secondary, pool.rl)
    hg = ctx.kmer_build(p, k, c["mf"], c["mq"])
    p.free()
    short = 1 if pool.rl <= 64 else 0                       # (the pools are couples throughout: tests/ref_live.py put_read)
    assert ctx.stat("pool_symmetric") == short, c
    assert ctx.stat("kmer_build_sym") == (k & 1) * short, c
    assert hg.pre_nodes == pre, c
    assert hg.n == len(nodes), c
    for i, (nid, km, freq, hv, hj, to, fr) in enumerate(nodes):
        assert nid == i + 1
        assert hg.kmer(i) == km, (c, i)
        assert int(hg.freq[i]) == freq, (c, i)
        assert (int(hg.has_v[i]), int(hg.has_j[i])) == (hv, hj), (c, i)
        assert list(hg.to_ids[i, :hg.to_deg[i]]) == to, (c, i)
        assert list(hg.from_ids[i, :hg.from_deg[i]]) == fr, (c, i)
    assert {hg.kmer(i): int(hg.gated_count[i]) for i in range(hg.n)} == surv, c


def check_map(ctx, c, pool, wins, ref):
    """ctx.window_score and ctx.map_emit against a map dump's W and P rows, per window length"""
    p = ctx.pool_load(pool.primary, pool.secondary, pool.rl)
    ctx.read_index_build(p, pool.pair_id, pool.read_num, pool.is_rc, pool.reg_rank, pool.n_pairs)
    by_len = {}
    for i, w in enumerate(wins):
        by_len.setdefault(len(w), []).append(i)
    for ln, idxs in by_len.items():
        ws = [wins[i] for i in idxs]
        valid, npairs = ctx.window_score(ws, c["ins"], e0=c["e0"], e1=c["e1"], rs=c["rs"], ms=c["ms"], floor=c["rf"])
        assert npairs.tolist() == [ref[i]["n"] for i in idxs], c
        assert valid.tolist() == [ref[i]["valid"] for i in idxs], c
        offs, pairs = ctx.map_emit(ws)
        for j, i in enumerate(idxs):
            mine = [(f"r{q['pair_id']}", int(q["pos1"]), int(q["pos2"]), int(q["insert"]), int(q["rc1"]), int(q["rc2"]))
                    for q in pairs[int(offs[j]):int(offs[j + 1])]]
            assert mine == ref[i]["pairs"], (c, i)
    p.free()


@live
@pytest.mark.parametrize("mode,seed", [(m, s) for m, s, _ in GRAPH_RUNS])
def test_kmer_build_random_configurations(ctx, mode, seed):
    rng = np.random.default_rng(seed)
    cfgs, n_nodes = [], []
    for it in range(GPU_N.get(mode, 8)):
        c = R.draw_graph(rng, mode, it)
        rep, pool = R.make_pool(c)
        pre, surv, nodes = R.graph(rep, pool, c["k"], c["mf"], c["mq"])
        check_graph(ctx, c, rep, pool, pre, surv, nodes)
        cfgs.append(c)
        n_nodes.append(len(nodes))
    graph_mode_conditions(mode, cfgs, n_nodes)


def _scorer_leg(_arg=None, ctx=None):
    """the window scorer and the pair emission on the first draws of the map run, the root scorer on the first of the score run;
    returns the tallies the conditions are asserted on (as JSON from the child process)"""
    from vdjer_amd import api
    own = ctx is None
    if own:
        ctx = api.Context(0)
    rng = np.random.default_rng(MAP_RUN[0])
    verdicts, with_pairs, n_clone_windows = [], 0, 0
    for it in range(GPU_N_MAP):
        c = R.draw_map(rng)
        rep, pool, wins = R.make_map_case(c)
        ref = R.map_windows(rep, pool, wins, c["ins"], c["e0"], c["e1"], c["rs"], c["ms"], c["rf"])
        check_map(ctx, c, pool, wins, ref)
        verdicts += [r["valid"] for r in ref]
        with_pairs += sum(r["n"] >= 1 for r in ref[:-1])
        n_clone_windows += len(ref) - 1
    rng = np.random.default_rng(SCORE_RUN[0])
    seen = [0, 0]
    for it in range(GPU_N_SCORE):
        c = R.draw_score(rng, it)
        ctx.vregion_load(c["lines"], c["vk"])
        for thr in c["thrs"]:
            want = R.score(c["lines"], c["k"], c["vk"], thr, c["queries"])
            got = ctx.root_score(c["queries"], c["k"], thr).tolist()
            bad = [i for i in range(len(got)) if got[i] != want[i]]
            assert not bad, (c["it"], c["k"], c["vk"], thr, [(c["queries"][i], got[i], want[i]) for i in bad[:5]])
            seen[0] += want.count(0)
            seen[1] += want.count(1)
    if own:
        ctx.close()
    return dict(verdicts=verdicts, with_pairs=with_pairs, n_clone_windows=n_clone_windows, seen=seen,
                knobs=[os.environ.get("VDJX_HIT_CHUNK"), os.environ.get("VDJX_GROUP_MIN")])


def _scorer_conditions(res):
    map_conditions(res["verdicts"], res["with_pairs"], res["n_clone_windows"])
    assert res["seen"][0] and res["seen"][1], res["seen"]


@live
def test_scorers_random_configurations_suite_knobs(ctx):
    res = _scorer_leg(ctx=ctx)
    _scorer_conditions(res)
    assert res["knobs"] == ["128", "1"]


@live
def test_scorers_random_configurations_shipped_knobs():
    code = "import json; from tests.test_gpu_vs_reference_live import _scorer_leg; print('LIVE', json.dumps(_scorer_leg('x')))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=_child_env("shipped"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    res = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("LIVE ")).split(" ", 1)[1])
    _scorer_conditions(res)
    assert res["knobs"] == [None, None]


@pytest.mark.parametrize("tag", sorted(R.EDGE_GRAPH))
def test_kmer_build_edge_fixtures(ctx, tag):
    c, rep, pool, pre, surv, nodes = R.edge_graph_case(tag)
    check_graph(ctx, c, rep, pool, pre, surv, nodes)
    R.edge_conditions(tag, c, pre, surv, nodes)


@pytest.mark.parametrize("tag", sorted(R.EDGE_MAP))
def test_scorers_edge_fixtures(ctx, tag):
    c, rep, pool, wins, ref = R.edge_map_case(tag)
    check_map(ctx, c, pool, wins, ref)
    assert any(r["n"] for r in ref[:-1])
