"""The model of vdjx_tree_spr (tests/tree_spr_model.py) on the CPU: the naive search_plain -- every candidate applied to a copy, the whole
tree recounted -- against the numpy variant with the edge formula on every case both can run; the figures the search was specified with;
P against the nearest-neighbour search of tests/tree_mp_model.py from the same start; lineages of four against that search as trees;
that no candidate of a finished tree is better; that every kind of move the device has to rewire occurs in some case of
tests/test_gpu_tree_spr.py and every bound case reaches its bound; and that a scorer without the down sets would be caught.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import tree_mp_model as M
from tests import tree_nj_cases as K
from tests import tree_nj_model as N
from tests import tree_spr_cases as C
from tests import tree_spr_model as S
from tests.tree_model import members_of, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("parent", "mutations", "depth", "clone")
# search_plain counts (2m)^2 trees of m leaves per round: the cases it finishes in seconds.  random_wild (40 members, wildcards) runs its
# first round only; the larger ones are the numpy variant's alone
PLAIN_CASES = ["m1", "m2", "m3", "m4_nj", "m4_cat", "m5_nj", "m5_cat", "cat20", "random_12", "random_12_cat", "identical", "identical_cat", "w1",
               "w64", "w65", "handmade"]


def _run(case, **kw):
    kw.setdefault("max_rounds", case.get("max_rounds", 0))
    return S.tree_spr(case["contigs"], case["clone"], case["anchor"], case["prio"], start=case.get("start"), **kw)


def _same(a, b, what):
    assert a["trace"] == b["trace"] and a["info"] == b["info"] and a["anc"] == b["anc"] and a["geometry"] == b["geometry"], what
    for f in ARRAYS:
        assert np.array_equal(a[f], b[f]), (what, f)


def _lineages(case, parent):
    """per lineage key: (m, root, local parents, children, leaf sets, slots) of the trees `parent` describes"""
    groups = members_of(case["clone"])
    out, slot0 = {}, len(case["contigs"])
    for key in sorted(groups):
        members, m = groups[key], len(groups[key])
        slots = members + list(range(slot0, slot0 + max(0, m - 2)))
        local = {s: v for v, s in enumerate(slots)}
        root = C.root_of(case, members)
        par = [-1 if v == root else local.get(int(parent[s]), -2) for v, s in enumerate(slots)]
        out[key] = (m, root, par, M.tree_of_parents(m, root, par), M.leaf_sets(windows(case["contigs"], members, case["anchor"])[0]), slots)
        slot0 += max(0, m - 2)
    return out


def test_the_naive_search_and_the_numpy_variant_agree():
    for name in PLAIN_CASES:
        _same(_run(C.case(name), plain=True), _run(C.case(name), plain=False), name)
        _same(_run(C.case(name), plain=False), C.want(name), name)                     # whichever the default takes
    wild = dict(C.case("random_wild"), max_rounds=1)
    _same(_run(wild, plain=True), _run(wild, plain=False), "random_wild, one round")
    assert _run(wild, plain=True)["trace"][0] == [C.want("random_wild")["trace"][0][0]]
    small = C.plain(K.many_small(300, 20))                                             # lineages of 3 .. 5 with wildcards
    a = _run(small, plain=True)
    _same(a, _run(small, plain=False), "many_small(300)")
    assert a["info"]["searched"] == 199 and a["info"]["moved"] > 10
    assert S.PLAIN_MEMBERS < 12                                                       # so the default ran the numpy variant on most cases


def test_the_figures_the_search_was_specified_with():
    """from the committed model; cat20 by the naive search too (the test above)"""
    cat = C.want("cat20")["info"]
    assert (cat["parsimony_start"], cat["parsimony"], cat["moves"], cat["rounds"], cat["candidates"]) == (159, 72, 11, 12, 12236)
    nj = N.tree_nj(*(C.case("cat20")[f] for f in ("contigs", "clone", "anchor", "prio")))
    assert nj["info"]["parsimony"] == 72                                              # the neighbour-joining tree of the same members
    figures = lambda name: tuple(C.want(name)["info"][f] for f in ("parsimony_start", "parsimony", "moves"))
    assert figures("random_wild") == (258, 244, 10) and figures("random_wild_cat") == (277, 245, 22)
    assert figures("random_12") == (54, 53, 1) and figures("random_12_cat") == (57, 54, 3)
    traces = C.want("mixed_random")["trace"]
    sizes = {key: len(v) for key, v in members_of(C.case("mixed_random")["clone"]).items()}
    by_size = {sizes[key]: (t[0][0], t[-1][0], sum(1 for _, mv in t if mv)) for key, t in traces.items()}
    assert by_size[20] == (213, 210, 3) and by_size[65] == (842, 818, 16)


def test_p_is_never_above_the_nearest_neighbour_searchs():
    """from the same start and under the same max_rounds, on every case.  Not a theorem for a steepest descent -- it holds on all of these"""
    for name in sorted(C.gpu_cases()):
        c = C.case(name)
        nni = M.tree_mp(c["contigs"], c["clone"], c["anchor"], c["prio"], start=c["start"], max_rounds=c["max_rounds"])["info"]
        spr = C.want(name)["info"]
        assert spr["parsimony_start"] == nni["parsimony_start"] and spr["parsimony"] <= nni["parsimony"], name
    assert C.want("cat20")["info"]["parsimony"] == 72 < 103 == M.tree_mp(*(C.case("cat20")[f] for f in ("contigs", "clone", "anchor", "prio")),
                                                                       start=C.case("cat20")["start"])["info"]["parsimony"]


def _by_clade(case, res):
    """per lineage: {the leaves below an inferred node: (its mutations, depth, sequence)}, and the leaves' rows as they are"""
    out, a = {}, 0
    for key, (m, root, par, kids, _, slots) in _lineages(case, res["parent"]).items():
        for v in range(m, len(par)):
            clade = frozenset(u for u in S.subtree(m, kids, v) if u < m)
            out[key, clade] = (int(res["mutations"][slots[v]]), int(res["depth"][slots[v]]), res["anc"][a])
            a += 1
        for v in range(m):
            out[key, v] = (int(res["mutations"][slots[v]]), int(res["depth"][slots[v]]), int(res["parent"][slots[v]] >= 0))
    return out


def test_a_lineage_of_four_ends_as_the_nearest_neighbour_search_ends():
    """at m = 4 the candidates reach exactly the trees of the nearest-neighbour interchanges, each by three (c, y).  The tree is that
    search's: the same P, rounds and moves, every clade with the same mutations, depth and sequence, every leaf's row the same.  Where no
    move is made the arrays are equal as they are.  After a move the two inferred ids can be exchanged: vdjx_tree_mp's swap keeps v
    below p, here p goes with c, and the key (P, c, y) prefers the smallest pruned node, not the (v, k) of that swap -- m4_cat is such a
    case -- and the candidates count 6 per round here, 2 there"""
    for name in ("m4_nj", "m4_cat"):
        c = C.case(name)
        nni = M.tree_mp(c["contigs"], c["clone"], c["anchor"], c["prio"], start=c["start"])
        spr = C.want(name)
        for f in ("parsimony_start", "parsimony", "moves", "rounds", "moved", "searched"):
            assert spr["info"][f] == nni["info"][f], (name, f)
        assert spr["info"]["candidates"] == 3 * nni["info"]["candidates"] == 6 * spr["info"]["rounds"]
        assert _by_clade(c, spr) == _by_clade(c, nni), name
        if not spr["info"]["moves"]:
            assert all(np.array_equal(spr[f], nni[f]) for f in ARRAYS) and spr["anc"] == nni["anc"]
    assert C.want("m4_nj")["info"]["moves"] == 0 and C.want("m4_cat")["info"]["moves"] == 1
    # on every lineage of four of a case of thousands: both searches stand on the best of the three topologies after one move, so P and the
    # rounds agree; where two of the three tie, the two keys may take different ones, so the clades need not
    c = C.case("many_small")
    nni, spr = M.tree_mp(c["contigs"], c["clone"], c["anchor"], c["prio"]), C.want("many_small")
    fours = [key for key, members in members_of(c["clone"]).items() if len(members) == 4]
    assert len(fours) > 500 and sum(1 for key in fours if any(mv for _, mv in spr["trace"][key])) > 20
    for key in fours:
        assert [t[0] for t in spr["trace"][key]] == [t[0] for t in nni["trace"][key]], key


@pytest.mark.parametrize("name", ["m5_cat", "cat20", "random_12_cat", "w65", "handmade", "mixed_random"])
def test_no_candidate_is_better_and_every_candidate_is_a_tree(name):
    case, res = C.case(name), C.want(name)
    total = 0
    for key, (m, root, par, kids, leaves, _) in _lineages(case, res["parent"]).items():
        p = M.count(leaves, m, root, kids)                                            # an independent full recount of the final tree
        total += p
        trace = res["trace"].get(key, [])
        assert all(a[0] > b[0] for a, b in zip(trace, trace[1:])), (name, key)        # every move lowers P
        if 3 < m <= 20:
            assert trace[-1] == (p, None)
            cands = S.candidates(m, root, par, kids)
            leaves_below = lambda v: sum(1 for u in S.subtree(m, kids, v) if u < m)
            assert len(cands) == sum(2 * (m - leaves_below(c)) - 4 for c in S.prunes(m, root, kids))
            for c, y in cands:
                p2, k2 = list(par), [list(x) for x in kids]
                s = next(u for u in kids[par[c]] if u != c)
                S.apply(p2, k2, c, y)
                assert M.tree_of_parents(m, root, p2) == k2                           # a move keeps it a tree, the children ascending
                assert M.count(leaves, m, root, k2) >= p, (name, key, c, y)
                S.apply(p2, k2, c, s)                                                  # the inverse regraft
                assert (p2[:root] + p2[root + 1:], k2) == (par[:root] + par[root + 1:], kids)
    assert total == res["info"]["parsimony"] == int(res["mutations"][res["parent"] >= 0].sum())


def test_gpu_cases_reach_their_edges():
    names = sorted(C.gpu_cases())
    sizes = {k: K.sizes_of(C.case(k)) for k in names}
    info = {k: C.want(k)["info"] for k in names}
    assert [sizes[k] for k in ("m1", "m2", "m3", "m4_nj", "m4_cat", "m5_nj", "m5_cat")] == [[1], [2], [3], [4], [4], [5], [5]]
    for k in ("m1", "m2", "m3"):
        assert info[k]["candidates"] == 0 and info[k]["searched"] == 0 and info[k]["rounds"] == 0
    assert info["m4_nj"]["candidates"] == 6 and info["m4_cat"]["candidates"] == 12 and info["m5_cat"]["moves"] == 2
    for k, w in [("w1", 1), ("w64", 64), ("w65", 65), ("w513", 513)]:
        assert len(windows(C.case(k)["contigs"], list(range(sizes[k][0])), C.case(k)["anchor"])[0][0]) == w
        assert C.case(k)["start"] is not None and (info[k]["moves"] > 0 or w == 1)
    wild = "".join(C.case("random_wild")["contigs"])
    assert "N" in wild and any(ch.islower() for ch in wild)
    for k in ("identical", "identical_cat"):
        assert len(set(C.case(k)["contigs"])) == 1 and info[k]["moves"] == 0 and info[k]["parsimony"] == 0 and info[k]["rounds"] == 1
    assert len(sizes["many_small"]) == 3000 and info["many_small"]["rounds"] >= 3 and info["many_small"]["moved"] > 100
    assert sizes["mixed"] == K.MIXED_SIZES == sizes["mixed_random"] == sizes["one_round"]
    for k in ("mixed", "mixed_random"):
        assert len(set(len(t) for t in C.want(k)["trace"].values())) >= 3, k          # lineages finish in different rounds of one batch
        assert [C.want(k, knob)["info"]["batches"] for knob in (2500, 1 << 26)] == [3, 1]
    assert C.case("one_round")["max_rounds"] == 1 and info["one_round"]["rounds"] == 1 and 0 < info["one_round"]["moves"] == info["one_round"]["moved"]
    for key, t in C.want("one_round")["trace"].items():
        assert t == C.want("mixed")["trace"][key][:1]
    assert C.case("handmade")["start"] is not None and info["handmade"]["moves"] > 0
    assert not np.array_equal(C.case("handmade")["start"], C.with_caterpillars(C.case("handmade"))["start"])
    # the kernels' bounds, by the constants of vdjx_spr.hip
    bound, wgs, pick = (C.kernel_constant(x) for x in ("VDJX_SPR_LDS_MEMBERS", "SPR_SLAB_WGS", "SPR_PICK_T"))
    assert sizes["lds_bound"] == [bound] and sizes["lds_bound_plus1"] == [bound + 1]
    assert all(0 < C.case(k)["max_rounds"] <= 3 and info[k]["moves"] >= 1 for k in ("lds_bound", "lds_bound_plus1", "slab_stride"))
    assert max(max(sizes[k]) for k in names if k not in ("lds_bound_plus1", "slab_stride")) <= bound      # the workspace path: these two alone
    m, = sizes["slab_stride"]
    assert m > bound and 2 * m - 4 > wgs and 2 * m - 2 > pick                         # a workgroup's second prune, a thread's second key
    (c, y), = [mv for _, mv in C.want("slab_stride")["trace"][0] if mv]
    assert c >= pick and C.displaced(m, 64, pick)[1] == c                             # the applied key lies past the first stride: the clade put back
    assert all(2 * max(sizes[k]) - 2 <= pick for k in names if k != "slab_stride")    # no other case has a second key
    # every kind of move k_spr_pick rewires, in cases that run on the GPU
    seen = {k: set().union(*[set(w) for t in C.want(k)["geometry"].values() for w in t]) for k in names}
    for word in C.GEOMETRY:
        assert any(word in seen[k] for k in names), word
    assert "g_root" in seen["m4_cat"] and "x_root" in seen["m5_cat"] and {"c_leaf", "c_inferred", "y_leaf", "y_inferred"} <= seen["cat20"]
    assert "c_inferred" in seen["slab_stride"] and {"g_root", "x_root"} <= seen["many_small"] and {"g_root", "x_root", "c_inferred"} <= seen["mixed"]


def test_a_scorer_without_the_down_sets_is_caught():
    """the mutant: a scorer that joins c to U'(y) alone and never makes D' (search_numpy(blind=True)).  On the lineages of these cases
    that the true search moves at all, its moves differ in most -- the cases can see the down pass"""
    caught = moved = 0
    for name in ("cat20", "random_wild", "random_12_cat", "w64", "w65", "mixed_random", "handmade", "m5_cat"):
        case = C.case(name)
        start = case["start"] if case["start"] is not None else N.tree_nj(case["contigs"], case["clone"], case["anchor"], case["prio"])["parent"]
        starts = _lineages(case, start)                                               # (vdjx_tree_nj's tree is the search's own start)
        for key, (m, root, par, kids, leaves, _) in starts.items():
            if m < 4 or not any(mv for _, mv in C.want(name)["trace"][key]):
                continue
            true = S.search_numpy(leaves, m, root, par, kids, 3)[2]
            assert true == C.want(name)["trace"][key][:3]
            moved += 1
            caught += [mv for _, mv in S.search_numpy(leaves, m, root, par, kids, 3, blind=True)[2]] != [mv for _, mv in true]
    assert moved >= 10 and caught > moved // 2, (moved, caught)


def test_the_abi_is_exported():
    """the entry point exists and refuses without a context, before anything else; the limit and the structs are the header's"""
    L = ctypes.CDLL(os.path.join(ROOT, "vdjer_amd", "libvdjx.so"))
    L.vdjx_tree_spr.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 11
    assert L.vdjx_tree_spr(None, None, 0, 0, *([None] * 11)) == -1                    # VDJX_EINVAL
    assert K.header_constant("VDJX_SPR_MAX_MEMBERS") == S.MAX_MEMBERS == 1024 <= M.MAX_MEMBERS
    from vdjer_amd import _lib, api
    assert "vdjx_tree_spr" in _lib.SYMBOLS and ctypes.sizeof(_lib.TreeSprInfo) == 72 and ctypes.sizeof(_lib.TreeSprParams) == 8
    assert api.Context.TREE_SPR_FIELDS == tuple(S.FIELDS) and callable(api.Context.tree_spr)
    assert C.kernel_constant("VDJX_SPR_LDS_MEMBERS") < S.MAX_MEMBERS


def test_the_command_line_is_what_it_was():
    """there is no flag for the search yet: the usage text's golden file does not name it"""
    with open(os.path.join(ROOT, "tests", "golden", "cli_refusals.json")) as f:
        assert "spr" not in f.read().lower()
