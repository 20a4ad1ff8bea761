"""Pins oracle/vdjx_oracle.c to the compiled reference where tests/test_oracle_vs_golden.py's fixed dumps do not reach: even k (the
build that cannot pair mirrored k-mers), k above 45 and below 17, read lengths 36 ... 160, --mq on both sides of the "a sum of 214
reads as 255" rule and past the clamp, --mf 4, reads with N, identical reads, the frequency cap, tandem repeats, mate spans past 64,
--e0 / --e1 / --rs off their defaults, floors 0 ... 3 and other insert sizes.

Two kinds of test: live ones, which run oracle/_ref/vdjer_ref (tests/ref_live.py) on configurations drawn from a seed and exist only
where the binary does, and one over the edges_* fixtures (tests/golden/make_golden_edges.py), which never skips.  Everything is
bit-exact.  The seeds are chosen so that the REFERENCE's results meet the conditions asserted at the end of each test (enough
configurations with nodes, both verdicts, every --mq edge): a test whose inputs went vacuous fails, it does not skip."""
import numpy as np
import pytest

from oracle import oracle
from tests import ref_live as R

live = pytest.mark.skipif(not R.available(), reason=R.SKIP_REASON)


def check_graph(c, rep, pool, pre, surv, nodes):
    """oracle.KmerTable, prune and Graph against a graph dump, as test_oracle_vs_golden.test_kmer_table_prune_graph compares them"""
    k = c["k"]
    vc, jc = R.codes(rep)
    t = oracle.KmerTable(pool, k)
    assert t.size() == pre, c
    assert t.prune(c["mf"], c["mq"]) == len(surv), c
    first, count, _, _ = t.export()
    assert {oracle.inst_kmer(pool, int(f), k): int(n) for f, n in zip(first, count)} == surv, c
    g = oracle.Graph(t, vc, jc)
    assert g.n == len(nodes), c
    for i, (nid, km, freq, hv, hj, to, fr) in enumerate(nodes):
        assert nid == i + 1
        assert oracle.inst_kmer(pool, int(g.first[i]), k) == km, (c, i)
        assert int(g.freq[i]) == freq, (c, i)
        assert (int(g.has_v[i]), int(g.has_j[i])) == (hv, hj), (c, i)
        assert list(g.to_ids[i, :g.to_deg[i]]) == to, (c, i)
        assert list(g.from_ids[i, :g.from_deg[i]]) == fr, (c, i)


def check_map(c, pool, wins, ref):
    """oracle.ReadIndex.quick_map and coverage_is_valid against a map dump, as test_quick_map_and_coverage compares them"""
    ix = oracle.ReadIndex(pool)
    for i, (w, r) in enumerate(zip(wins, ref)):
        pairs, starts = ix.quick_map(w)
        mine = [(f"r{q['pair_id']}", int(q["pos1"]), int(q["pos2"]), int(q["insert"]), int(q["rc1"]), int(q["rc2"])) for q in pairs]
        assert mine == r["pairs"], (c, i)
        assert [tuple(x) for x in starts.tolist()] == r["starts"], (c, i)
        v = 1 if c["rf"] == 0 else ix.coverage_is_valid(starts, len(w), c["ins"], e0=c["e0"], e1=c["e1"], rs=c["rs"], ms=c["ms"], floor=c["rf"])
        assert v == r["valid"], (c, i)


def graph_mode_conditions(mode, cfgs, n_nodes):
    """what keeps a graph test from passing on nothing (shared with tests/test_gpu_vs_reference_live.py)"""
    assert 2 * sum(n >= 1 for n in n_nodes) >= len(n_nodes) and max(n_nodes) >= 500, n_nodes
    if mode == "even_k":
        assert all(c["k"] % 2 == 0 and c["rl"] <= 64 for c in cfgs)
    if mode == "k46_50":
        assert all(c["k"] > 45 for c in cfgs)
    if mode == "long":
        assert all(c["rl"] > 64 for c in cfgs)
    if mode == "gt32":
        assert sum(c["rl"] - c["k"] + 1 > 32 for c in cfgs) * 2 >= len(cfgs)
    if mode == "le32":
        assert all(c["rl"] - c["k"] + 1 <= 32 for c in cfgs)
    if mode == "mq_edges":
        assert {c["mq"] for c in cfgs} == set(R.MQ_EDGES)


def map_conditions(verdicts, with_pairs, n_clone_windows):
    n = len(verdicts)
    assert 10 * verdicts.count(0) >= n and 10 * verdicts.count(1) >= n, (verdicts.count(0), verdicts.count(1))
    assert 2 * with_pairs >= n_clone_windows, (with_pairs, n_clone_windows)


# (mode, seed, configurations); the GPU file runs the first GPU_N of each
GRAPH_RUNS = [("le32", 1, 10), ("gt32", 2, 10), ("long", 5, 10), ("even_k", 1, 10), ("k46_50", 2, 10), ("mq_edges", 5, 12)]
MAP_RUN = (2, 12)
SCORE_RUN = (7, 12)


@live
@pytest.mark.parametrize("mode,seed,n", GRAPH_RUNS)
def test_graph_random_configurations(mode, seed, n):
    rng = np.random.default_rng(seed)
    cfgs, n_nodes = [], []
    for it in range(n):
        c = R.draw_graph(rng, mode, it)
        rep, pool = R.make_pool(c)
        pre, surv, nodes = R.graph(rep, pool, c["k"], c["mf"], c["mq"])
        check_graph(c, rep, pool, pre, surv, nodes)
        cfgs.append(c)
        n_nodes.append(len(nodes))
    graph_mode_conditions(mode, cfgs, n_nodes)


@live
def test_map_random_configurations():
    seed, n = MAP_RUN
    rng = np.random.default_rng(seed)
    verdicts, with_pairs, n_clone_windows, floors = [], 0, 0, set()
    for it in range(n):
        c = R.draw_map(rng)
        rep, pool, wins = R.make_map_case(c)
        ref = R.map_windows(rep, pool, wins, c["ins"], c["e0"], c["e1"], c["rs"], c["ms"], c["rf"])
        check_map(c, pool, wins, ref)
        verdicts += [r["valid"] for r in ref]
        with_pairs += sum(r["n"] >= 1 for r in ref[:-1])          # (the last window is the random string)
        n_clone_windows += len(ref) - 1
        floors.add(c["rf"])
    map_conditions(verdicts, with_pairs, n_clone_windows)
    assert floors == {0, 1, 2, 3}


@live
def test_score_random_configurations():
    seed, n = SCORE_RUN
    rng = np.random.default_rng(seed)
    seen = {0: 0, 1: 0}
    for it in range(n):
        c = R.draw_score(rng, it)
        s = oracle.RootScorer(c["lines"], c["vk"])
        for thr in c["thrs"]:
            want = R.score(c["lines"], c["k"], c["vk"], thr, c["queries"])
            got = [s.score(q, thr) for q in c["queries"]]
            bad = [i for i in range(len(got)) if got[i] != want[i]]
            assert not bad, (c["it"], c["k"], c["vk"], thr, [(c["queries"][i], got[i], want[i]) for i in bad[:5]])
            seen[0] += want.count(0)
            seen[1] += want.count(1)
    assert seen[0] and seen[1], seen


@live
@pytest.mark.parametrize("tag", R.HANDMADE)
def test_handmade_pools(tag):
    """tandem repeats, all-N reads, '#' qualities, k = rl, a pool with no primary record, and the pool whose hot k-mers reach the
    frequency cap, at k 35 and k 34: the recipes of the fixtures, run live"""
    c = R.EDGE_GRAPH[tag]
    rep, pool = R.make_pool(c)
    pre, surv, nodes = R.graph(rep, pool, c["k"], c["mf"], c["mq"], timeout=R.timeout_of(c))
    check_graph(c, rep, pool, pre, surv, nodes)
    R.edge_conditions(tag, c, pre, surv, nodes)


@pytest.mark.parametrize("tag", sorted(R.EDGE_GRAPH))
def test_edge_fixtures_graph(tag):
    c, rep, pool, pre, surv, nodes = R.edge_graph_case(tag)
    assert c == R.EDGE_GRAPH[tag]
    check_graph(c, rep, pool, pre, surv, nodes)
    R.edge_conditions(tag, c, pre, surv, nodes)


@pytest.mark.parametrize("tag", sorted(R.EDGE_MAP))
def test_edge_fixtures_map(tag):
    c, rep, pool, wins, ref = R.edge_map_case(tag)
    assert c == R.EDGE_MAP[tag]
    check_map(c, pool, wins, ref)
    assert any(r["n"] for r in ref[:-1])


def test_edge_fixtures_hold_both_verdicts():
    verdicts = [r["valid"] for tag in sorted(R.EDGE_MAP) if R.EDGE_MAP[tag]["rf"] for r in R.edge_map_case(tag)[4]]
    assert 10 * verdicts.count(0) >= len(verdicts) and 10 * verdicts.count(1) >= len(verdicts)
