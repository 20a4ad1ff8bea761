"""The model of vdjx_tree_mp (tests/tree_mp_model.py) on the CPU: its two versions against each other, its properties against independent
recounts and a brute force over every topology, the tie rule on handmade member orders, the floors of the search on the seeded cases, the
texts of the command line by hand, and that every case of tests/test_gpu_tree_mp.py reaches the edge it is named for -- for the stride
and pick cases by MP_FILL_WAVES and MP_PICK_T as vdjx_mp.hip defines them: the candidates, the column tiles and the height of
k_mp_score's grid, the candidate indices of the applied moves -- and that a scorer which never left its first column tile would be
caught by the stride cases and by no case from before them.  No GPU."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import tree_mp_cases as C
from tests import tree_mp_model as M
from tests import tree_nj_cases as K
from tests import tree_nj_model as N
from tests.tree_model import distance_matrix, members_of, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _case(name):
    return C.gpu_cases()[name]()


def _run(case, **kw):
    kw.setdefault("max_rounds", case.get("max_rounds", 0))
    return M.tree_mp(case["contigs"], case["clone"], case["anchor"], case["prio"], start=case.get("start"), **kw)


@functools.lru_cache(maxsize=None)
def _model(name):
    return _run(_case(name))


def _lineages(case, res):
    """per lineage key: (m, root, local parents, children, leaf sets) of the result's trees"""
    groups = members_of(case["clone"])
    out, slot0 = {}, len(case["contigs"])
    for key in sorted(groups):
        members, m = groups[key], len(groups[key])
        nodes = m + max(0, m - 2)
        slots = members + list(range(slot0, slot0 + nodes - m))
        local = {s: v for v, s in enumerate(slots)}
        par = [local.get(int(res["parent"][s]), -1) for s in slots]
        root = par.index(-1)
        assert root == C.root_of(case, members) and par.count(-1) == 1
        out[key] = (m, root, par, M.tree_of_parents(m, root, par), M.leaf_sets(windows(case["contigs"], members, case["anchor"])[0]))
        slot0 += nodes - m
    return out


PROPERTY_CASES = ["m4_cat", "m5_cat", "w65", "cat20", "random_wild", "random_12", "identical_cat", "mixed_random", "one_round", "stride_all",
                  "stride_mixed"]
STRIDE_CASES = ["stride_all", "stride_mixed", "pick_cat140", "pick_random300", "widths"]      # a wave over several tiles, a thread over several candidates
OLD_CASES = ["m1", "m2", "m3", "m4_nj", "m4_cat", "m5_nj", "m5_cat", "w1", "w64", "w65", "w513", "cat20", "cat130", "lds_bound", "lds_bound_plus1",
             "random_wild", "random_12", "identical", "identical_cat", "many_small", "mixed", "mixed_random", "one_round"]     # neither happens in these
SAMPLE = 300                                               # lineages of a case of thousands that the per-candidate checks look at


def _sample_keys(case, seed=1):
    """every lineage key of a case of up to SAMPLE lineages; of a larger one SAMPLE keys chosen by seed"""
    keys = sorted(members_of(case["clone"]))
    if len(keys) <= SAMPLE:
        return set(keys)
    return set(keys[i] for i in np.random.default_rng(seed).permutation(len(keys))[:SAMPLE])


@pytest.mark.parametrize("name", PROPERTY_CASES)
def test_no_neighbour_is_better_and_p_never_rises(name):
    """the recount, the falling trace and the totals on every lineage of every case; the recount of every neighbour of the final tree on
    every lineage too, except in the stride cases (thousands of lineages), where it is made on SAMPLE lineages chosen by seed"""
    case, res = _case(name), _model(name)
    sample = _sample_keys(case)
    total = 0
    for key, (m, root, par, kids, leaves) in _lineages(case, res).items():
        p = M.count(leaves, m, root, kids)                                            # an independent full recount of the final tree
        total += p
        trace = res["trace"].get(key, [])
        assert all(a[0] > b[0] for a, b in zip(trace, trace[1:])), (name, key)        # every move lowers P
        if m > 3 and not case["max_rounds"]:
            assert trace[-1] == (p, None, None)
        if m > 3 and not case["max_rounds"] and key in sample:
            for v, k in M.candidates(m, par):
                p2, k2 = list(par), [list(x) for x in kids]
                M.swap(p2, k2, v, k)
                assert M.tree_of_parents(m, root, p2) == k2                           # a swap keeps it a tree, the children ascending
                assert M.count(leaves, m, root, k2) >= p, (name, key, v, k)
    assert total == res["info"]["parsimony"] == int(res["mutations"][res["parent"] >= 0].sum())
    assert res["info"]["parsimony"] <= res["info"]["parsimony_start"]
    assert (res["info"]["parsimony"] < res["info"]["parsimony_start"]) == (res["info"]["moves"] > 0)


def _all_topologies(m):
    """the edge lists of all (2m - 5)!! unrooted binary trees on m >= 3 leaves: every new leaf into every edge"""
    def grow(edges, leaf, nxt):
        if leaf == m:
            yield edges
            return
        for i, (a, b) in enumerate(edges):
            yield from grow(edges[:i] + edges[i + 1:] + [(a, nxt), (nxt, b), (leaf, nxt)], leaf + 1, nxt + 1)
    yield from grow([(0, m), (1, m), (2, m)], 3, m + 1)


def test_p_against_the_brute_force_minimum():
    reached = 0
    for m, seed, start in [(4, 104, "cat"), (5, 105, "cat"), (6, 41, "cat"), (7, 42, "cat"), (6, 43, "nj"), (7, 44, "nj")]:
        case = K.infinite_sites(m, seed) if start == "cat" else K.random_case(m, 40, seed)
        case = C.with_caterpillars(case) if start == "cat" else C.plain(case)
        res = _run(case)
        (m_, root, _, _, leaves), = _lineages(case, res).values()
        trees = list(_all_topologies(m))
        assert len(trees) == int(np.prod(np.arange(2 * m - 5, 0, -2)))
        best = min(M.count(leaves, m, root, N.orient(m, [(a, b, 0) for a, b in e], root)[3]) for e in trees)
        assert res["info"]["parsimony"] >= best, (m, seed)
        reached += res["info"]["parsimony"] == best and res["info"]["moves"] > 0
    assert reached >= 1                                                               # the search does find the optimum somewhere it had to move


def test_the_two_versions_agree():
    for name in sorted(C.gpu_cases()):
        if name in ("cat130", "mixed", "many_small", "pick_cat140", "pick_random300", "widths"):       # a full count per candidate of 65 .. 300 leaves: minutes
            continue
        if name in ("stride_all", "stride_mixed"):                                     # thousands of lineages: a sample of them below, not dropped
            continue
        a, b = _run(_case(name), plain=True), _run(_case(name), plain=False)
        assert a["trace"] == b["trace"] and a["info"] == b["info"] and a["anc"] == b["anc"], name
        for f in ("parent", "mutations", "depth", "clone"):
            assert np.array_equal(a[f], b[f]), (name, f)
    small = C.plain(K.many_small(300, 20))
    a, b = _run(small, plain=True), _run(small, plain=False)
    assert a["trace"] == b["trace"] and a["info"] == b["info"] and np.array_equal(a["parent"], b["parent"])
    assert a["info"]["moved"] == 22 and a["info"]["searched"] == 199
    # the stride cases on SAMPLE of their lineages, chosen by seed: cut out of the case as they are, so the traces are the whole case's
    for name, start in [("stride_all", C.plain), ("stride_mixed", C.with_caterpillars)]:
        part = dict({"max_rounds": 0}, **start(C.sample_of(_case(name), SAMPLE, 2)))
        a, b = _run(part, plain=True), _run(part, plain=False)
        assert a["trace"] == b["trace"] and a["info"] == b["info"] and a["anc"] == b["anc"], name
        for f in ("parent", "mutations", "depth", "clone"):
            assert np.array_equal(a[f], b[f]), (name, f)
        assert len(a["trace"]) == SAMPLE and all(_model(name)["trace"][key] == t for key, t in a["trace"].items()), name


def test_infinite_sites_from_the_nj_start_make_no_move():
    for m, seed in [(12, 5), (4, 104), (30, 9)]:
        case = C.plain(K.infinite_sites(m, seed))
        res = _run(case)
        nj = N.tree_nj(case["contigs"], case["clone"], case["anchor"], case["prio"])
        assert res["info"]["moves"] == 0 and res["info"]["rounds"] == 1 and res["info"]["candidates"] == 2 * (m - 3)
        assert res["info"]["parsimony_start"] == res["info"]["parsimony"] == nj["info"]["parsimony"]
        for f in ("parent", "mutations", "depth", "clone"):
            assert np.array_equal(res[f], nj[f])
        assert res["anc"] == nj["anc"]
    assert _run(C.plain(K.infinite_sites(12, 5)))["info"]["parsimony"] == 34


def test_max_rounds_1_is_the_first_step():
    case = _case("one_round")
    one, full = _model("one_round"), _model("mixed")
    assert one["info"]["rounds"] == 1 and 0 < one["info"]["moves"] == one["info"]["moved"] <= one["info"]["searched"]
    for key, trace in one["trace"].items():
        assert len(trace) == 1 and trace[0] == full["trace"][key][0]
    start = _lineages(case, dict(parent=case["start"]))
    for key, (m, root, par, kids, _) in _lineages(case, one).items():
        p0, k0 = list(start[key][2]), [list(x) for x in start[key][3]]
        move = one["trace"].get(key, [(0, None, None)])[0][1]
        if move:
            M.swap(p0, k0, *move)
        assert (p0, k0) == (par, kids), key
    two = _run(dict(case, max_rounds=2))
    assert two["info"]["rounds"] == 2 and all(t == full["trace"][key][:2] for key, t in two["trace"].items())


def _hand(order):
    """four members, the root first: R = AA, X = GG, Y = GA (shares column 1 with X), Z = AG (shares column 2 with X), from a caterpillar"""
    seqs = dict(R="AA", X="GG", Y="GA", Z="AG")
    case = dict(contigs=[seqs[x] for x in order], clone=np.zeros(4, np.int32), anchor=np.zeros(4, np.int32), prio=np.zeros(4, np.uint32))
    res = _run(C.with_caterpillars(case))
    (m, root, par, kids, _), = _lineages(case, res).values()
    sisters = next(sorted(order[c] for c in kids[v]) for v in (4, 5) if all(c < 4 for c in kids[v]))
    return res["info"], sisters, res["trace"][0]


def test_the_tie_rule_on_three_member_orders():
    # the caterpillar pairs the last two members.  In R X Y Z both swaps of node 5 lower P from 4 to 3 -- (X, Z) with k = 0, (X, Y) with
    # k = 1 --: the key (P, v, k) takes k = 0.  With Y and Z exchanged the same rule pairs X with Y: the tree depends on the order of the
    # contigs.  In R Y X Z the start already pairs X with Z at P = 3, and no swap is better
    info, sisters, trace = _hand("RXYZ")
    assert (info["parsimony_start"], info["parsimony"], info["moves"]) == (4, 3, 1) and sisters == ["X", "Z"] and trace[0] == (4, (5, 0), 0)
    info, sisters, trace = _hand("RXZY")
    assert (info["parsimony_start"], info["parsimony"], info["moves"]) == (4, 3, 1) and sisters == ["X", "Y"] and trace[0] == (4, (5, 0), 0)
    info, sisters, trace = _hand("RYXZ")
    assert (info["parsimony_start"], info["parsimony"], info["moves"]) == (3, 3, 0) and sisters == ["X", "Z"] and trace == [(3, None, None)]


def test_the_floors_of_the_search():
    cat = _model("cat20")["info"]
    assert cat["moves"] >= 10 and cat["parsimony"] < cat["parsimony_start"]
    nj = N.tree_nj(*(_case("cat20")[f] for f in ("contigs", "clone", "anchor", "prio")))["info"]["parsimony"]
    assert cat["parsimony"] > nj                                                      # a local optimum: far above the neighbour-joining tree's total
    assert _model("random_wild")["info"]["moves"] >= 1
    many = _model("many_small")["info"]
    assert many["searched"] > 1000 and 0.05 * many["searched"] <= many["moved"] < many["searched"]
    for name in ("mixed", "mixed_random"):
        assert len(set(len(t) for t in _model(name)["trace"].values())) >= 3, name    # lineages finish in different rounds


def test_small_lineages_and_texts_by_hand():
    one = M.tree_mp(["ACGT"], [3], [0])
    assert one["parent"].tolist() == [-1] and one["mutations"].tolist() == [-1] and one["depth"].tolist() == [0] and one["info"]["batches"] == 0
    hand = dict(ids=["c1", "c2", "c3", "c4", "c5"], contigs=["GGAAAA", "GGAAAC", "TTTTTT", "GGAACC", "GGACCC"], clone=[0, 0, -1, 0, 1], anchor=[2, 2, 0, 2, 1])
    res = M.tree_mp(hand["contigs"], hand["clone"], hand["anchor"])
    assert M.table_text(M.table_rows(hand["ids"], hand["contigs"], hand["clone"], hand["anchor"], res)) == (
        "clone_id\tnode_id\tparent_id\tbranch_length\tmutations\tdepth\tchildren\tobserved\tsequence\n"
        "lin_1\tc1\t\t0.0000\t\t0\t1\tT\tGGAAAA\n"
        "lin_1\tc2\tlin_1_a1\t0.0000\t0\t2\t0\tT\tGGAAAC\n"
        "lin_1\tc4\tlin_1_a1\t1.0000\t1\t2\t0\tT\tGGAACC\n"
        "lin_1\tlin_1_a1\tc1\t1.0000\t1\t1\t2\tF\tGGAAAC\n"
        "lin_2\tc5\t\t0.0000\t\t0\t0\tT\tGGACCC\n")
    assert M.newick_text(hand["ids"], hand["clone"], res) == "lin_1\t(('c2':0.0000,'c4':1.0000)'lin_1_a1':1.0000)'c1';\n"
    assert M.summary_line(res["info"]) == ("trees mp: 4 contigs in 2 lineages (largest 3), 0 searched, 0 improved, 0 moves in 0 rounds, 0 candidates, "
                                           "parsimony 2 -> 2, 1 batches")
    from vdjer_amd import annot
    assert np.array_equal(annot.tree_mp_lengths(res["parent"], res["mutations"], res["clone"]), M.lengths_of(res))
    assert M.lengths_of(res).tolist() == [0, 0, -1, 1 << 16, 0, 1 << 16]


def test_bad_starts_are_named():
    root, l = 0, [1, 2, 3, 4]
    good = C.caterpillar(5, root)
    assert good == [-1, 5, 6, 7, 7, 0, 5, 6] and M.tree_of_parents(5, root, good) == [[5], [], [], [], [], [1, 6], [2, 7], [3, 4]]
    for v, p in [(1, -2), (1, 0), (4, 5), (4, 1)]:
        bad = list(good)
        bad[v] = p
        with pytest.raises(ValueError):
            M.tree_of_parents(5, root, bad)
    with pytest.raises(ValueError, match="cycle"):
        M.tree_of_parents(5, root, [-1, 5, 5, 6, 7, 0, 7, 6])


def test_the_abi_is_exported():
    """the entry point exists and refuses without a context, before anything else; the limit is vdjx_tree_nj's"""
    L = ctypes.CDLL(os.path.join(ROOT, "vdjer_amd", "libvdjx.so"))
    L.vdjx_tree_mp.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 11
    assert L.vdjx_tree_mp(None, None, 0, 0, *([None] * 11)) == -1                     # VDJX_EINVAL
    with open(os.path.join(ROOT, "include", "vdjx.h")) as f:
        assert "#define VDJX_MP_MAX_MEMBERS VDJX_NJ_MAX_MEMBERS" in f.read()
    from vdjer_amd import _lib
    assert "vdjx_tree_mp" in _lib.SYMBOLS and M.MAX_MEMBERS == _lib.NJ_MAX_MEMBERS


def test_gpu_cases_reach_their_edges():
    bound = K.header_constant("VDJX_NJ_LDS_MEMBERS")
    names = sorted(C.gpu_cases())
    sizes = {k: K.sizes_of(_case(k)) for k in names}
    assert [sizes[k] for k in ("m1", "m2", "m3", "m4_nj", "m4_cat", "m5_nj", "m5_cat")] == [[1], [2], [3], [4], [4], [5], [5]]
    for k in ("m1", "m2", "m3"):
        assert _model(k)["info"]["candidates"] == 0 and _model(k)["info"]["searched"] == 0
    assert _model("m4_nj")["info"]["candidates"] == 2 and _model("m4_cat")["info"]["candidates"] == 4 and _model("m5_cat")["info"]["moves"] == 2
    climbs = {k: [t[2] for tr in _model(k)["trace"].values() for t in tr if t[1]] for k in names}
    assert climbs["m4_cat"] == [0] and 0 in climbs["cat20"] and max(climbs["cat20"]) >= 5      # the root step alone, and deep in the tree
    assert sizes["cat130"] == [130] and max(climbs["cat130"]) > 64 and _model("cat130")["info"]["moves"] > 64      # a path longer than a wave is wide
    for k, w in [("w1", 1), ("w64", 64), ("w65", 65), ("w513", 513)]:
        members = list(range(sizes[k][0]))
        assert len(windows(_case(k)["contigs"], members, _case(k)["anchor"])[0][0]) == w
        assert _case(k)["start"] is not None and (_model(k)["info"]["moves"] > 0 or w == 1)
    assert sizes["lds_bound"] == [bound] and sizes["lds_bound_plus1"] == [bound + 1]
    assert all(_case(k)["start"] is None and _model(k)["info"]["moves"] == 0 for k in ("lds_bound", "lds_bound_plus1"))
    wild = "".join(_case("random_wild")["contigs"])
    assert "N" in wild and any(ch.islower() for ch in wild) and _model("random_wild")["info"]["moves"] == 3
    assert (_model("random_wild")["info"]["parsimony_start"], _model("random_wild")["info"]["parsimony"]) == (258, 255)
    assert (_model("random_12")["info"]["parsimony_start"], _model("random_12")["info"]["parsimony"]) == (54, 53)
    for k in ("identical", "identical_cat"):
        assert len(set(_case(k)["contigs"])) == 1 and _model(k)["info"]["moves"] == 0 and _model(k)["info"]["parsimony"] == 0
    many = _case("many_small")
    assert len(sizes["many_small"]) == 3000 and (many["clone"] == -1).sum() == 200 and _model("many_small")["info"]["rounds"] >= 3
    assert sizes["mixed"] == K.MIXED_SIZES == sizes["mixed_random"] == sizes["one_round"]
    assert [_run(_case("mixed"), cells_knob=knob, max_rounds=1)["info"]["batches"] for knob in (1, 2500, 1 << 26)] == [7, 3, 1]
    assert _case("one_round")["max_rounds"] == 1 and all(_case(k)["max_rounds"] == 0 for k in names if k != "one_round")
    # k_mp_score's grid, by the host's formulas and the constants of vdjx_mp.hip.  Every case is one batch (the knob unset)
    fill, pick = C.kernel_constant("MP_FILL_WAVES"), C.kernel_constant("MP_PICK_T")
    assert all(_model(k)["info"]["batches"] <= 1 for k in names) and sorted(OLD_CASES + STRIDE_CASES) == names
    grid = {k: C.scorer_grid(_case(k)) for k in names}
    for k in OLD_CASES:                                                               # before the stride cases: a wave never took a second tile
        assert grid[k][0] == 0 or grid[k][2] == max(grid[k][1]), k
    assert max(grid[k][0] for k in OLD_CASES) == grid["many_small"][0] < fill and max(grid["many_small"][1]) == 2 and max(grid["w513"][1]) == 9
    n_cand, tiles, grid_y = grid["stride_all"]
    assert n_cand >= fill and grid_y == 1 and set(tiles) == {3} and len(tiles) == len(sizes["stride_all"]) == 2100 and set(sizes["stride_all"]) == {7}
    assert _case("stride_all")["start"] is None and (_case("stride_all")["clone"] == -1).sum() == 50
    n_cand, tiles, grid_y = grid["stride_mixed"]
    assert fill / 2 <= n_cand < fill and grid_y == 2 and set(tiles) == {1, 2, 3, 4, 5} and set(sizes["stride_mixed"]) == {6, 7, 8}
    assert _case("stride_mixed")["start"] is not None and len(tiles) == 1200 and min(tiles.count(t) for t in (1, 2, 3, 4, 5)) >= 100
    for k in ("stride_all", "stride_mixed"):
        info = _model(k)["info"]
        assert info["rounds"] >= 5 and info["moves"] >= 1500 and info["moved"] < info["searched"]      # lineages go out round by round
        first = {int(c): i for i, c in reversed(list(enumerate(_case(k)["clone"]))) if c >= 0}
        last = {int(c): i for i, c in enumerate(_case(k)["clone"]) if c >= 0}
        assert sum(last[c] - first[c] + 1 > 8 for c in first) > 0.95 * len(first)                       # interleaved
    n_cand, tiles, grid_y = grid["widths"]                                            # 20 lineages of 70: 1 .. 17 tiles under waves of every 7th tile
    assert sorted(K.lineage_words(_case("widths"))) == K.WIDTH_WORDS and sizes["widths"] == [K.WIDTH_MEMBERS] * 20 and _case("widths")["start"] is None
    assert n_cand == 20 * 2 * (K.WIDTH_MEMBERS - 3) and (min(tiles), max(tiles)) == (1, 17) and 1 < grid_y == -(-fill // n_cand) < max(tiles)
    assert {t for t in tiles if t < grid_y} and {t for t in tiles if grid_y < t <= 2 * grid_y} and {t for t in tiles if t > 2 * grid_y}
    assert _model("widths")["info"]["moved"] >= 15 and _model("widths")["info"]["moves"] >= 100           # and moves at nearly every width
    # k_mp_pick: more candidates than threads, and applied moves on both sides of the first stride
    applied = {}
    for k in ("pick_cat140", "pick_random300"):
        (key, (m, root, par, kids, _)), = _lineages(_case(k), _model(k)).items()
        applied[k] = [C.candidate_index(m, kids[root][0], v, kk) for _, (v, kk), _ in _model(k)["trace"][key][:-1]]
        assert M.candidates(m, par) == sorted(M.candidates(m, par)) and len(M.candidates(m, par)) == 2 * (m - 3)
        assert [C.candidate_index(m, kids[root][0], v, kk) for v, kk in M.candidates(m, par)] == list(range(2 * (m - 3)))
        assert any(i >= pick for i in applied[k]) and any(i < pick for i in applied[k]), (k, applied[k])
    assert sizes["pick_cat140"] == [140] and pick < 2 * (140 - 3) <= 2 * pick and _case("pick_cat140")["start"] is not None
    assert sizes["pick_random300"] == [300] and 2 * pick < 2 * (300 - 3) <= 3 * pick and _case("pick_random300")["start"] is None
    assert grid["pick_random300"][1:] == ([7], 7) and len(applied["pick_cat140"]) >= 50 and len(applied["pick_random300"]) >= 10
    for k in OLD_CASES:                                                               # before: no lineage had a candidate for a second stride
        assert max([0] + [2 * (m - 3) for m in sizes[k]]) < pick, k


def _starts(case):
    """key -> (m, root, leaf sets, local parents, children) of the start tree of every searched lineage, as the model makes them"""
    out = {}
    groups = members_of(case["clone"])
    for key in sorted(groups):
        members, m = groups[key], len(groups[key])
        if m > 3:
            ws = windows(case["contigs"], members, case["anchor"])[0]
            root = C.root_of(case, members)
            if case["start"] is None:
                par, _, _, kids = N.orient(m, N.nj_edges([[int(x) << N.SHIFT for x in row] for row in distance_matrix(ws)]), root)
            else:
                par = C.caterpillar(m, root)
                kids = M.tree_of_parents(m, root, par)
            out[key] = (m, root, M.leaf_sets(ws), par, kids)
    return out


def test_a_scorer_that_stays_on_its_first_tile_is_caught_by_the_stride_cases_alone():
    """the mutant: k_mp_score without `col0 += gridDim.y * 64` scores a candidate on the first 64 * grid_y columns of its lineage.  That is
    M.search on leaves cut to those columns.  On SAMPLE lineages of each stride case (chosen by seed; the whole case has thousands) the
    moves then differ from the full search's in many lineages; in every case from before, 64 * grid_y columns are the whole window of
    every lineage, so the mutant computes what the kernel computes and no comparison with the model could tell them apart"""
    for k in OLD_CASES:
        n_cand, tiles, grid_y = C.scorer_grid(_case(k))
        assert all(len(ws[0]) <= 64 * grid_y for ws in C.lineage_windows(_case(k)).values() if len(ws) > 3), k
    for name in ("stride_all", "stride_mixed"):
        case = _case(name)
        n_cand, tiles, grid_y = C.scorer_grid(case)
        starts, sample = _starts(case), _sample_keys(case, seed=3)
        caught = cut_lineages = 0
        for key in sorted(sample):
            m, root, leaves, par, kids = starts[key]
            moves = [t[1] for t in M.search(leaves, m, root, par, kids)[2]]
            assert moves == [t[1] for t in _model(name)["trace"][key]], (name, key)  # (the start is the model's: the full search is its trace)
            if len(leaves[0]) > 64 * grid_y:
                cut_lineages += 1
                caught += [t[1] for t in M.search([x[:64 * grid_y] for x in leaves], m, root, par, kids)[2]] != moves
        assert cut_lineages >= SAMPLE // 2 and caught >= cut_lineages // 4, (name, cut_lineages, caught)
