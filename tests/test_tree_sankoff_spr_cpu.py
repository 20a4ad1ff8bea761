"""The model of vdjx_tree_sankoff_spr (tests/tree_sankoff_spr_model.py) on the CPU: the naive search_plain -- every candidate applied to a
copy, the whole tree recounted -- against the numpy variant with the rooted identity, under four matrices; under equal costs the moves of
tests/tree_spr_model.py; the figures the search was specified with, below both existing searches; a scorer without E' is caught; lineages
of four against the nearest-neighbour search of tests/tree_sankoff_model.py; the edge costs sum to W; every case of
tests/test_gpu_tree_sankoff_spr.py reaches the edge it is named for; and the entry point is exported.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import tree_nj_cases as K
from tests import tree_sankoff_model as KM
from tests import tree_sankoff_spr_cases as C
from tests import tree_sankoff_spr_model as X
from tests import tree_spr_cases as SC
from tests import tree_spr_model as S
from tests.tree_model import windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("parent", "cost", "mutations", "depth", "clone")
PLAIN_CASES = ["m4_nj", "m4_cat", "m5_cat", "handmade", "random_12", "w1", "w65", "identical", "cat20"]      # cat20: its first two rounds


def _run(case, cost, **kw):
    kw.setdefault("max_rounds", case.get("max_rounds", 0))
    return X.tree_sankoff_spr(case["contigs"], case["clone"], case["anchor"], case["prio"], cost=cost, start=case.get("start"), **kw)


def _same(a, b, what):
    assert a["trace"] == b["trace"] and a["info"] == b["info"] and a["anc"] == b["anc"] and a["geometry"] == b["geometry"], what
    for f in ARRAYS:
        assert np.array_equal(a[f], b[f]), (what, f)


@pytest.mark.parametrize("matrix", sorted(C.MATRICES))
def test_the_naive_search_and_the_identity_agree(matrix):
    """trace (W before every round, the applied move), parents, W and everything else"""
    moved = 0
    for name in PLAIN_CASES:
        case = dict(SC.case(name), max_rounds=2) if name == "cat20" else SC.case(name)
        a = _run(case, C.MATRICES[matrix], plain=True)
        _same(a, _run(case, C.MATRICES[matrix], plain=False), (name, matrix))
        moved += a["info"]["moves"]
    assert moved >= 6 and X.PLAIN_MEMBERS < 12
    if matrix == "ASYM":                                                              # the recount in Python ints, column by column
        case = SC.case("handmade")
        lin = _lineage(case)
        assert X.search_plain(C.ASYM, *lin, ints=True) == X.search_plain(C.ASYM, *lin) == X.search_numpy(C.ASYM, *lin)


def _lineage(case):
    """(leaves, m, root, parent, kids) of a case of one lineage with a start"""
    from tests import tree_mp_model as M
    m = len(case["contigs"])
    members = list(range(m))
    root = SC.root_of(case, members)
    slots = members + list(range(m, 2 * m - 2))
    par = [-1 if v == root else int(case["start"][s]) for v, s in enumerate(slots)]
    return KM.codes(windows(case["contigs"], members, case["anchor"])[0]), m, root, par, M.tree_of_parents(m, root, par)


@pytest.mark.parametrize("name", C.SPR_SHARED)
def test_under_equal_costs_the_moves_are_tree_sprs(name):
    """with UNIT, and with all twelve costs 7, W is a multiple of Fitch's count: the keys order alike"""
    c, spr = SC.case(name), SC.want(name)
    for cost, times in ((C.UNIT, 1), (C.SEVENS, 7)):
        got = _run(c, cost)
        assert {k: [mv for _, mv in t] for k, t in got["trace"].items()} == {k: [mv for _, mv in t] for k, t in spr["trace"].items()}, name
        assert {k: [w for w, _ in t] for k, t in got["trace"].items()} == {k: [times * p for p, _ in t] for k, t in spr["trace"].items()}
        assert np.array_equal(got["parent"], spr["parent"]) and got["geometry"] == spr["geometry"]
        assert all(got["info"][f] == spr["info"][f] for f in ("moves", "rounds", "candidates", "moved", "searched", "batches", "edges", "internal"))
        assert got["info"]["cost"] == times * spr["info"]["parsimony"] and got["info"]["cost_start"] == times * spr["info"]["parsimony_start"]
        assert got["info"]["mutations"] == spr["info"]["parsimony"]


def test_the_figures_the_search_was_specified_with():
    """from the committed model: start, end, moves, candidates -- and on random_wild the end lies strictly below vdjx_tree_sankoff's
    (nearest-neighbour interchanges under the matrix) and below the cost of vdjx_tree_spr's tree under the matrix"""
    fig = lambda name, cost: tuple(_run(SC.case(name), cost)["info"][f] for f in ("cost_start", "cost", "moves", "candidates"))
    nni = lambda name, cost, **kw: KM.tree_sankoff(*(SC.case(name)[f] for f in ("contigs", "clone", "anchor", "prio")), cost=cost,
                                                   start=kw.pop("start", SC.case(name)["start"]), **kw)["info"]["cost"]
    assert fig("random_wild", C.TSTV) == (420, 391, 14, 76832) and fig("random_wild", C.ASYM) == (1109, 1026, 20, 107756)
    assert fig("cat20", C.ASYM) == (649, 306, 11, 12056) and fig("cat20", C.TSTV)[:3] == (263, 120, 11)
    assert fig("handmade", C.TSTV)[:3] == (41, 34, 1) and fig("random_12", C.TSTV)[:3] == (83, 80, 1)
    assert fig("cat20", C.UNIT) == (159, 72, 11, 12236) and fig("random_wild", C.UNIT)[:3] == (258, 244, 10)
    assert C.want("random_wild")["info"]["cost"] == 391 and C.want("cat20")["info"]["cost"] == 306      # the GPU cases are these
    spr = {name: SC.want(name)["parent"] for name in ("random_wild", "cat20", "handmade", "random_12")}
    for cost, ends, nni_end, spr_tree in ((C.TSTV, 391, 416, 398), (C.ASYM, 1026, 1090, 1060)):
        assert nni("random_wild", cost) == nni_end > ends and nni("random_wild", cost, start=spr["random_wild"], search_=False) == spr_tree > ends
    assert (nni("cat20", C.ASYM), nni("cat20", C.ASYM, start=spr["cat20"], search_=False)) == (367, 306)
    assert (nni("cat20", C.TSTV), nni("cat20", C.TSTV, start=spr["cat20"], search_=False)) == (171, 120)
    assert (nni("handmade", C.TSTV), nni("handmade", C.TSTV, start=spr["handmade"], search_=False)) == (36, 34)
    assert (nni("random_12", C.TSTV), nni("random_12", C.TSTV, start=spr["random_12"], search_=False)) == (80, 81)


def test_a_scorer_without_e_is_caught():
    """the mutant: a scorer that joins c to H'_y alone and never makes E' (search_numpy(blind=True)): on random_12 under ASYM its move is
    another one"""
    from tests import tree_nj_model as N
    case = SC.case("random_12")
    nj = N.tree_nj(case["contigs"], case["clone"], case["anchor"], case["prio"])["parent"]
    lin = _lineage(dict(case, start=nj))
    true, blind = X.search_numpy(C.ASYM, *lin, 3), X.search_numpy(C.ASYM, *lin, 3, blind=True)   # (the mutant's figure always falls: capped)
    assert true[2] == C.want("random_12_asym")["trace"][0] and true[3] == 202
    assert [mv for _, mv in blind[2]] != [mv for _, mv in true[2]] and blind[3] >= true[3]


@pytest.mark.parametrize("matrix", sorted(C.MATRICES))
def test_a_lineage_of_four_ends_where_the_nearest_neighbour_search_ends(matrix):
    """the three topologies of four members are mutual neighbours in both searches: the same final cost, rounds and moves"""
    for name in ("m4_nj", "m4_cat"):
        c = SC.case(name)
        nni = KM.tree_sankoff(c["contigs"], c["clone"], c["anchor"], c["prio"], cost=C.MATRICES[matrix], start=c["start"])["info"]
        spr = _run(c, C.MATRICES[matrix])["info"]
        assert all(spr[f] == nni[f] for f in ("cost_start", "cost", "moves", "rounds", "searched")), (name, matrix)
        assert spr["candidates"] == 3 * nni["candidates"] == 6 * spr["rounds"]


def test_the_edge_costs_sum_to_w():
    for name in sorted(C.gpu_cases()):
        res = C.want(name)
        finished = all(t[-1][1] is None for t in res["trace"].values())            # (no max_rounds cut a lineage short)
        final = sum(t[-1][0] for t in res["trace"].values()) if finished else None
        assert int(res["cost"][res["parent"] >= 0].sum()) == res["info"]["cost"] <= res["info"]["cost_start"], name
        assert int(res["mutations"][res["parent"] >= 0].sum()) == res["info"]["mutations"]
        c = C.case(name)
        recount = KM.tree_sankoff(c["contigs"], c["clone"], c["anchor"], c["prio"], cost=c["cost"], start=res["parent"], search_=False, plain=False)
        assert recount["info"]["cost"] == res["info"]["cost"] and np.array_equal(recount["cost"], res["cost"]) and recount["anc"] == res["anc"]
        if final is not None and all(m > 3 for m in K.sizes_of(c)):
            assert final == res["info"]["cost"], name
        for t in res["trace"].values():
            assert all(a[0] > b[0] for a, b in zip(t, t[1:])), name                   # every move lowers W


def test_gpu_cases_reach_their_edges():
    names = sorted(C.gpu_cases())
    sizes = {k: K.sizes_of(C.case(k)) for k in names}
    info = {k: C.want(k)["info"] for k in names}
    assert [sizes[k] for k in ("m1", "m2", "m3", "m4_nj", "m4_cat", "m5_nj", "m5_cat", "handmade")] == [[1], [2], [3], [4], [4], [5], [5], [6]]
    for k in ("m1", "m2", "m3"):
        assert info[k]["candidates"] == 0 and info[k]["searched"] == 0 and info[k]["rounds"] == 0
    assert info["m4_nj"]["candidates"] == 6 and info["m4_cat"]["candidates"] == 12 and info["m5_cat"]["moves"] == 2 and info["handmade"]["moves"] == 1
    for k, w in [("w1", 1), ("w64", 64), ("w65", 65), ("w513", 513)]:
        assert len(windows(C.case(k)["contigs"], list(range(sizes[k][0])), C.case(k)["anchor"])[0][0]) == w
        assert C.case(k)["start"] is not None and (info[k]["moves"] > 0 or w == 1)
    wild = "".join(C.case("random_wild")["contigs"])
    assert "N" in wild and any(ch.islower() for ch in wild)
    for k in ("identical", "identical_cat"):
        assert len(set(C.case(k)["contigs"])) == 1 and info[k]["moves"] == 0 and info[k]["cost"] == 0 and info[k]["rounds"] == 1
    assert {C.case(f"random_12_{x.lower()}")["cost"] is C.MATRICES[x] for x in C.MATRICES} == {True}
    assert all(info[f"random_12_{x.lower()}"]["moves"] >= 1 for x in C.MATRICES)
    assert sizes["mixed"] == K.MIXED_SIZES == sizes["mixed_random"]
    for k in ("mixed", "mixed_random"):
        assert len(set(len(t) for t in C.want(k)["trace"].values())) >= 3, k          # lineages finish in different rounds of one batch
        assert [C.want(k, knob)["info"]["batches"] for knob in (2500, 1 << 26)] == [3, 1]
    # the kernels' bounds, by the constants of vdjx_sankoff_spr.hip
    small, bound, wgs, pick = (C.kernel_constant(x) for x in ("SKSP_LDS_MEMBERS_8", "VDJX_SKSP_LDS_MEMBERS", "SKSP_SLAB_WGS", "SKSP_PICK_T"))
    assert small < bound < S.MAX_MEMBERS
    assert sizes["lds8_bound"] == [small] and sizes["lds8_bound_plus1"] == [small + 1]
    assert sizes["lds_bound"] == [bound] and sizes["lds_bound_plus1"] == [bound + 1]
    assert all(0 < C.case(k)["max_rounds"] <= 3 and info[k]["moves"] >= 1 for k in ("lds_bound", "lds_bound_plus1", "slab_stride", "big"))
    assert C.case("lds_bound")["max_rounds"] == C.case("lds_bound_plus1")["max_rounds"] == 2
    beyond = sorted(k for k in names if max(sizes[k]) > bound)                        # the workspace path
    assert beyond == ["big", "lds_bound_plus1", "mixed", "mixed_random", "random_wild", "random_wild_unit", "slab_stride"]
    assert any(small < max(sizes[k]) <= bound for k in names) and any(3 < max(sizes[k]) <= small for k in names)
    m, = sizes["slab_stride"]
    assert 2 * m - 4 > wgs and 2 * m - 2 > pick                                       # a workgroup's second prune, a thread's second key
    (c, y), = [mv for _, mv in C.want("slab_stride")["trace"][0] if mv]
    assert c >= pick and SC.displaced(m, 64, pick)[1] == c                            # the applied key lies past the first stride: the clade put back
    assert all(2 * max(sizes[k]) - 2 <= pick for k in names if k != "slab_stride")    # no other case has a second key
    # the 64-bit total, on the wide-window path: 63 column tiles
    assert info["big"]["cost"] > 1 << 32 and info["big"]["cost_start"] - info["big"]["cost"] > 0 and C.case("big")["max_rounds"] == 1
    assert len(windows(C.case("big")["contigs"], list(range(sizes["big"][0])), C.case("big")["anchor"])[0][0]) == 4000
    assert info["lds_bound_plus1"]["cost"] > 1 << 23 and info["random_12_big"]["cost"] > 1 << 21
    # every kind of move k_sksp_pick rewires, in cases that run on the GPU
    seen = {k: set().union(*[set(w) for t in C.want(k)["geometry"].values() for w in t]) for k in names}
    for word in C.GEOMETRY:
        assert any(word in seen[k] for k in names), word
    assert "g_root" in seen["m4_cat"] and "x_root" in seen["m5_cat"] and {"c_leaf", "c_inferred", "y_leaf", "y_inferred", "g_root", "x_root"} <= seen["cat20"]
    assert "c_inferred" in seen["slab_stride"] and {"g_root", "x_root", "c_inferred"} <= seen["mixed"]


def test_the_abi_is_exported():
    """the entry point exists and refuses without a context, before anything else; the structs are the header's"""
    L = ctypes.CDLL(os.path.join(ROOT, "vdjer_amd", "libvdjx.so"))
    L.vdjx_tree_sankoff_spr.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 13
    assert L.vdjx_tree_sankoff_spr(None, None, 0, 0, *([None] * 13)) == -1            # VDJX_EINVAL
    from vdjer_amd import _lib, api
    assert "vdjx_tree_sankoff_spr" in _lib.SYMBOLS and hasattr(_lib.lib(), "vdjx_tree_sankoff_spr")
    assert ctypes.sizeof(_lib.TreeSankoffSprParams) == 16 and ctypes.sizeof(_lib.TreeSankoffInfo) == 80
    assert api.Context.TREE_SANKOFF_FIELDS == tuple(X.FIELDS) and callable(api.Context.tree_sankoff_spr)
    assert K.header_constant("VDJX_SPR_MAX_MEMBERS") == X.MAX_MEMBERS == 1024
    with open(os.path.join(ROOT, "include", "vdjx.h")) as f:
        text = f.read()
    assert "vdjx_tree_sankoff_spr_params;" in text and "/* 16 bytes; reserved must be 0 */" in text.split("vdjx_tree_sankoff_spr_params;")[1][:60]


def test_the_command_line_is_what_it_was():
    """there is no flag for the search: the usage text's golden file does not name it"""
    with open(os.path.join(ROOT, "tests", "golden", "cli_refusals.json")) as f:
        assert "sankoff" not in f.read().lower()
