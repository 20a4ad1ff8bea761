"""The model of vdjx_tree_sankoff (tests/tree_sankoff_model.py) on the CPU: the naive path -- every candidate applied to a copy, the whole
tree recounted column by column -- against the numpy path on every case both can run; W against a brute force over all state
assignments, which shares nothing with the recursion; the unit matrix against tests/tree_mp_model.py; the sum of the edge costs; the
figures the feature was specified with; that every bound case of tests/test_gpu_tree_sankoff.py reaches its bound; the exported symbols
and struct sizes; and vdjx_sankoff_costs through ctypes against a restatement.  No GPU."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest

from tests import tree_mp_cases as MK
from tests import tree_mp_model as M
from tests import tree_nj_cases as K
from tests import tree_nj_model as N
from tests import tree_sankoff_cases as C
from tests import tree_sankoff_model as S
from tests.tree_model import distance_matrix, members_of, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("parent", "cost", "mutations", "depth", "clone")
# the naive search counts 2 (m - 3) whole trees per round, column by column: the cases it finishes in a second or two
PLAIN_CASES = ["m1", "m2", "m3", "m4_nj", "m4_cat", "m5_nj", "m5_cat", "small_wild_cat", "w1", "w64", "w65", "cat20", "cat20_tstv", "random_12",
               "identical", "identical_cat", "many_small", "handmade", "no_search", "unit_m4_cat", "unit_m5_cat", "unit_random_12", "unit_w65"]


def _run(case, **kw):
    return S.tree_sankoff(case["contigs"], case["clone"], case["anchor"], case["prio"], cost=case["cost"], start=case["start"],
                          search_=case["search"], max_rounds=case["max_rounds"], **kw)


def test_the_naive_and_the_numpy_path_agree():
    for name in PLAIN_CASES:
        a, b = _run(C.case(name), plain=True), _run(C.case(name), plain=False)
        assert a["trace"] == b["trace"] and a["info"] == b["info"] and a["anc"] == b["anc"], name
        for f in ARRAYS:
            assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), (name, f)
        w = C.want(name)                                                              # (whichever path the case runs by itself)
        assert w["info"] == a["info"] and w["anc"] == a["anc"] and all(np.array_equal(w[f], a[f]) for f in ARRAYS), name


def _brute(c, leaves, m, root, parent):
    """the smallest sum of edge costs over every assignment of states to the inferred nodes (and to a wildcard root), column by column;
    a wildcard leaf takes its parent's state, which costs 0"""
    nodes, total = len(parent), 0
    for q in range(len(leaves[0])):
        free = list(range(m, nodes)) + ([root] if leaves[root][q] > 3 else [])
        best = None
        for states in itertools.product(range(4), repeat=len(free)):
            st = dict(zip(free, states))
            cost = 0
            for v in range(nodes):
                if v == root:
                    continue
                sp = st[parent[v]] if parent[v] in st else leaves[parent[v]][q]
                sv = st[v] if v in st else (leaves[v][q] if leaves[v][q] < 4 else sp)
                cost += c[sp][sv]
            best = cost if best is None or cost < best else best
        total += best
    return total


@pytest.mark.parametrize("matrix", sorted(C.MATRICES))
def test_w_is_the_minimum_over_all_state_assignments(matrix):
    """lineages of 3 .. 5 members and 1 .. 6 columns with wildcards, from the neighbour-joining tree and from a caterpillar"""
    c = S.check_cost(C.MATRICES[matrix])
    rng = np.random.default_rng(90)
    checked = wild_roots = 0
    for m in (3, 4, 5):
        for rep in range(6):
            ws = K.random_windows(m, 1 + rep, rng, wild=0.35, per_member=0.6)
            leaves = S.codes(ws)
            root = int(rng.integers(m))
            wild_roots += 4 in leaves[root]
            edges = N.nj_edges([[int(x) << N.SHIFT for x in row] for row in distance_matrix(ws)])
            for par in (N.orient(m, edges, root)[0], MK.caterpillar(m, root)):
                kids = M.tree_of_parents(m, root, par)
                want = _brute(c, leaves, m, root, par)
                assert S.count(c, leaves, m, root, kids) == want == S._np_count(c, leaves, m, root, kids), (matrix, m, rep)
                for rec in (S.reconstruct, S.reconstruct_numpy):
                    state, cost, _ = rec(c, leaves, m, root, par, kids)
                    assert sum(x for v, x in enumerate(cost) if v != root) == want
                    assert all(state[v][q] == leaves[v][q] for v in range(m) for q in range(len(ws[0])) if leaves[v][q] < 4)
                checked += 1
    assert checked == 36 and wild_roots >= 3


@pytest.mark.parametrize("name", C.UNIT_SHARED)
def test_under_unit_costs_the_search_is_tree_mps(name):
    """the weighted cost of every candidate is its Fitch count: the same moves, the same parents; the edges sum to that model's P"""
    case = MK.gpu_cases()[name]()
    mp = M.tree_mp(case["contigs"], case["clone"], case["anchor"], case["prio"], start=case["start"], max_rounds=case["max_rounds"])
    got = C.want("unit_" + name)
    assert got["trace"] == mp["trace"]
    for f in ("parent", "depth", "clone"):
        assert np.array_equal(got[f], mp[f]), (name, f)
    assert got["info"]["cost"] == got["info"]["mutations"] == mp["info"]["parsimony"]
    assert got["info"]["cost_start"] == mp["info"]["parsimony_start"]
    assert all(got["info"][f] == mp["info"][f] for f in S.FIELDS if f in mp["info"])
    assert np.array_equal(got["cost"], got["mutations"].astype(np.int64))
    null = S.tree_sankoff(case["contigs"], case["clone"], case["anchor"], case["prio"], cost=None, start=case["start"], max_rounds=case["max_rounds"])
    assert null["info"] == got["info"] and all(np.array_equal(null[f], got[f]) for f in ARRAYS)


def test_the_edge_costs_sum_to_the_total_on_every_case():
    for name in sorted(C.gpu_cases()):
        res = C.want(name)
        assert int(res["cost"][res["parent"] >= 0].sum()) == res["info"]["cost"], name
        assert int(res["mutations"][res["parent"] >= 0].sum()) == res["info"]["mutations"], name
        assert np.array_equal(res["cost"] < 0, res["parent"] < 0) and res["cost"].dtype == np.int64
        assert res["info"]["cost"] <= res["info"]["cost_start"]
        if res["trace"]:                                                              # W where the search stopped is what the edges cost
            assert res["info"]["moves"] == sum(1 for t in res["trace"].values() for _, mv, _ in t if mv)


def test_the_figures_the_feature_was_specified_with():
    """(cost start, cost, moves) from the committed model, and what vdjx_tree_mp's final tree costs under the same matrix"""
    figure = lambda name: tuple(C.want(name)["info"][f] for f in ("cost_start", "cost", "moves"))
    assert figure("random_12") == (83, 80, 2) and figure("random_wild") == (420, 416, 4) and figure("random_wild_asym") == (1109, 1090, 11)
    assert figure("cat20") == (649, 367, 25) and figure("w65") == (340, 191, 15) and figure("handmade") == (113, 94, 3)
    assert figure("cat20_tstv") == (263, 171, 23)
    for name, mp_costs in [("random_12", 81), ("random_wild", 417), ("random_wild_asym", 1104), ("cat20", 435), ("w65", 258), ("handmade", 100),
                           ("cat20_tstv", 171)]:
        case = C.case(name)
        mp = M.tree_mp(case["contigs"], case["clone"], case["anchor"], case["prio"], start=case["start"], ancestors=False)
        scored = S.tree_sankoff(case["contigs"], case["clone"], case["anchor"], case["prio"], cost=case["cost"], start=mp["parent"], search_=False)
        assert scored["info"]["cost"] == scored["info"]["cost_start"] == mp_costs, name
        assert np.array_equal(scored["parent"], mp["parent"])
    same = C.case("cat20_tstv")                                                       # ... where the two searches end in the same tree
    assert np.array_equal(C.want("cat20_tstv")["parent"], M.tree_mp(same["contigs"], same["clone"], same["anchor"], same["prio"], start=same["start"])["parent"])


def test_gpu_cases_reach_their_edges():
    names = sorted(C.gpu_cases())
    sizes = {k: K.sizes_of(C.case(k)) for k in names}
    info = {k: C.want(k)["info"] for k in names}
    assert [sizes[k] for k in ("m1", "m2", "m3", "m4_nj", "m4_cat", "m5_nj", "m5_cat")] == [[1], [2], [3], [4], [4], [5], [5]]
    assert sizes["small_wild_cat"] == [1, 2, 3, 4, 5] and C.case("small_wild_cat")["start"] is not None
    for k in ("m1", "m2", "m3"):
        assert info[k]["candidates"] == 0 and info[k]["searched"] == 0 and info[k]["rounds"] == 0
    assert info["m2"]["cost"] > 0 and info["m3"]["cost"] > 0 and info["m4_cat"]["moves"] == 1 and info["m5_cat"]["moves"] == 2
    for k, w in [("w1", 1), ("w64", 64), ("w65", 65), ("w513", 513)]:
        assert len(windows(C.case(k)["contigs"], list(range(sizes[k][0])), C.case(k)["anchor"])[0][0]) == w
        assert C.case(k)["start"] is not None and (info[k]["moves"] > 0 or w == 1)
    for k in ("random_wild", "small_wild_cat"):                                       # wildcards in leaves and in the root member
        case = C.case(k)
        for members in members_of(case["clone"]).values():
            ws = windows(case["contigs"], members, case["anchor"])[0]
            root = MK.root_of(case, members)
            assert len(members) < 3 or (any(ch not in "ACGT" for ch in ws[root]) and any(ch not in "ACGT" for i, w_ in enumerate(ws) if i != root for ch in w_))
    for k in ("identical", "identical_cat"):
        assert len(set(C.case(k)["contigs"])) == 1 and info[k]["moves"] == 0 and info[k]["cost"] == 0 and info[k]["rounds"] == 1
    assert len(sizes["many_small"]) == 300 and set(sizes["many_small"]) == {3, 4, 5} and info["many_small"]["moved"] > 20
    assert sizes["mixed"] == K.MIXED_SIZES == sizes["mixed_random"] == sizes["one_round"]
    for k in ("mixed", "mixed_random"):
        assert len(set(len(t) for t in C.want(k)["trace"].values())) >= 3, k          # lineages finish in different rounds of one batch
        assert [C.want(k, knob)["info"]["batches"] for knob in (2500, 1 << 26)] == [3, 1]
    assert C.case("one_round")["max_rounds"] == 1 and info["one_round"]["rounds"] == 1 and 0 < info["one_round"]["moves"] == info["one_round"]["moved"]
    assert C.case("handmade")["start"] is not None and info["handmade"]["moves"] > 0
    assert not np.array_equal(C.case("handmade")["start"], C.with_caterpillars(C.case("handmade"))["start"])
    quiet = info["no_search"]
    assert not C.case("no_search")["search"] and quiet["cost"] == quiet["cost_start"] > 0 and (quiet["searched"], quiet["rounds"], quiet["candidates"]) == (0, 0, 0)
    assert _run(dict(C.case("no_search"), search=True, max_rounds=1))["info"]["moves"] == 1      # (a search would have moved)
    # the kernels' bounds, by the constants of vdjx_sankoff.hip
    pick, fill = C.kernel_constant("SK_PICK_T"), C.kernel_constant("SK_FILL_WAVES")
    assert 2 * (sizes["pick_bound"][0] - 3) == pick and 2 * (sizes["pick_bound_plus1"][0] - 3) == pick + 2
    assert info["pick_bound"]["moves"] == info["pick_bound_plus1"]["moves"] == 1
    (_, (v, k), _), = C.want("pick_bound_plus1")["trace"][0]
    assert 2 * max(max(s) for n_, s in sizes.items() if not n_.startswith("pick_bound") and n_ != "big") - 6 <= pick
    n_cand, tiles, grid_y = C.scorer_grid(C.case("stride_tiles"))
    assert n_cand < fill and 1 < grid_y < min(tiles) and info["stride_tiles"]["moved"] > 100      # every wave takes a second tile, none a third
    assert 2 * grid_y >= max(tiles)
    for k in names:                                                                   # everywhere else a wave has one tile
        if k != "stride_tiles" and info[k]["searched"]:
            _, t, g = C.scorer_grid(C.case(k))
            assert g == max(t), k
    big = C.want("big")
    assert C.case("big")["cost"] == C.BIG and info["big"]["cost"] > 1 << 32 and info["big"]["cost_start"] > info["big"]["cost"] and info["big"]["moves"] == 1
    assert info["big"]["cost"] // 513 > 1 << 16 and int(big["cost"].max()) > 1 << 16 and (sizes["big"][0] * 2 - 3) * 65535 < 1 << 31
    assert sum(1 for row in C.BIG for x in row if x == 1) == 1 and sum(1 for row in C.BIG for x in row if x == 65535) == 11


def test_a_bad_matrix_is_refused_by_the_model():
    for s, t, x in [(0, 0, 1), (1, 2, 0), (3, 1, 65536)]:
        bad = [list(row) for row in C.TSTV]
        bad[s][t] = x
        with pytest.raises(ValueError, match=rf"cost\[{s}\]\[{t}\] is {x}"):
            S.check_cost(bad)
    assert S.check_cost(None) == C.UNIT == S.UNIT and S.check_cost(C.BIG) == C.BIG


def test_the_abi_is_exported():
    """the entry points exist and refuse without a context or arguments, before anything else; the structs are the header's"""
    L = ctypes.CDLL(os.path.join(ROOT, "vdjer_amd", "libvdjx.so"))
    L.vdjx_tree_sankoff.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 13
    assert L.vdjx_tree_sankoff(None, None, 0, 0, *([None] * 13)) == -1                # VDJX_EINVAL
    L.vdjx_sankoff_costs.argtypes = [ctypes.c_void_p] * 3
    from vdjer_amd import _lib, api
    assert {"vdjx_tree_sankoff", "vdjx_sankoff_costs"} <= set(_lib.SYMBOLS)
    assert ctypes.sizeof(_lib.TreeSankoffParams) == 16 and ctypes.sizeof(_lib.TreeSankoffInfo) == 80 and ctypes.sizeof(_lib.SankoffCostsInfo) == 16
    assert api.Context.TREE_SANKOFF_FIELDS == tuple(S.FIELDS) and callable(api.Context.tree_sankoff)
    assert K.header_constant("VDJX_NJ_MAX_MEMBERS") == S.MAX_MEMBERS
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()                     # test_cabi_cpu's list is the header's
    import re
    assert sorted(set(re.findall(r"\b(vdjx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))) == sorted(_lib.SYMBOLS)


def _costs_restated(weight):
    """vdjx_sankoff_costs in Python: the same libm, the same order of operations"""
    Wc = [[0] * 4 for _ in range(4)]
    for row in range(1024):
        for e in range(4):
            Wc[(row >> 4) & 3][e] += int(weight[row][e])
    cells = [(c, e) for c in range(4) for e in range(4) if c != e]
    wp = {ce: max(Wc[ce[0]][ce[1]], 1) for ce in cells}
    total = sum(wp.values())
    d = {ce: -math.log10(float(wp[ce]) / float(total)) for ce in cells}
    acc = 0.0
    for ce in cells:
        acc += d[ce]
    mean = acc / 12.0
    cost = [[0] * 4 for _ in range(4)]
    for c, e in cells:
        cost[c][e] = int(min(max(math.floor(1000.0 * d[(c, e)] / mean + 0.5), 1), 65535))
    return cost, mean


def test_sankoff_costs_through_ctypes():
    from vdjer_amd import _lib, annot
    rng = np.random.default_rng(91)
    uniform = np.full((1024, 4), 9, np.uint32)
    cost, info = annot.sankoff_costs(uniform)
    assert cost.dtype == np.uint32 and cost.tolist() == [[0 if s == t else 1000 for t in range(4)] for s in range(4)]
    assert (info["min_cost"], info["max_cost"]) == (1000, 1000)
    models = [rng.integers(0, 5000, (1024, 4)).astype(np.uint32) for _ in range(5)]
    models.append(np.zeros((1024, 4), np.uint32))                                     # every sum 0: w' = 1 everywhere, the uniform model
    models.append(np.full((1024, 4), 0xFFFFFFFF, np.uint32))                          # sums of 256 x (2^32 - 1): past 2^32
    sparse = np.zeros((1024, 4), np.uint32)
    sparse[(1 << 4) | 5, 3] = 0xFFFFFFFF                                              # one cell C -> T, the other eleven 0
    models.append(sparse)
    ts = np.zeros((1024, 4), np.uint32)                                               # all weight on transitions A <-> G, C <-> T
    for row in range(1024):
        ts[row, {0: 2, 1: 3, 2: 0, 3: 1}[(row >> 4) & 3]] = 100 + row % 7
    models.append(ts)
    for w in models:
        cost, info = annot.sankoff_costs(w)
        want, mean = _costs_restated(w.tolist())
        assert cost.tolist() == want and info["mean"] == mean
        off = [want[s][t] for s in range(4) for t in range(4) if s != t]
        assert (info["min_cost"], info["max_cost"]) == (min(off), max(off)) and all(want[s][s] == 0 for s in range(4))
        assert S.check_cost(want) == want                                             # a matrix vdjx_tree_sankoff takes
    assert annot.sankoff_costs(models[5])[0].tolist() == annot.sankoff_costs(uniform)[0].tolist() == annot.sankoff_costs(models[6])[0].tolist()
    cost = annot.sankoff_costs(ts)[0]
    transitions = {(0, 2), (2, 0), (1, 3), (3, 1)}
    assert max(cost[s, t] for s, t in transitions) < min(cost[s, t] for s in range(4) for t in range(4) if s != t and (s, t) not in transitions)
    L = _lib.lib()
    out, w = np.zeros(16, np.uint32), np.ascontiguousarray(uniform)
    assert L.vdjx_sankoff_costs(None, out.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert L.vdjx_sankoff_costs(w.ctypes.data_as(ctypes.c_void_p), None, None) == -1
    assert L.vdjx_sankoff_costs(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), None) == 0 and out[1] == 1000
    with pytest.raises(ValueError):
        annot.sankoff_costs(np.zeros((1024, 3), np.uint32))


def test_the_command_line_is_what_it_was():
    """there is no flag for the call yet: the usage text's golden file does not name it"""
    with open(os.path.join(ROOT, "tests", "golden", "cli_refusals.json")) as f:
        assert "sankoff" not in f.read().lower()
