"""vdjx_tree_sankoff_spr on the GPU: every output array, the ancestors and every info field against the model of
tests/tree_sankoff_spr_model.py, exactly -- on the cases of tests/tree_sankoff_spr_cases.py (tests/test_tree_sankoff_spr_cpu.py checks that
each reaches the edge it is named for: lineages of 1 .. 6 members, four matrices, the search's specified figures, wildcards, all-identical
members, windows of 1, 64, 65, 513 and 4,000 columns, mixed sizes that finish in different rounds of one batch, both LDS geometries at
their bounds and one member more, more prunes than the workspace path launches workgroups and more keys than k_sksp_pick has threads, a
total above 2^32), under a VDJX_NJ_CELLS that cuts several batches, against vdjx_tree_spr under unit costs, without ancestors, two calls,
the refusals, and the result in the hands of tree_split_support, tree_split_compare and the Newick writer.  Every model result is computed
once (tests/tree_sankoff_spr_cases.want)."""
import numpy as np
import pytest

from tests import tree_nj_cases as NK
from tests import tree_sankoff_spr_cases as K
from tests import tree_sankoff_spr_model as X
from tests import tree_split_cases as SK

pytestmark = pytest.mark.gpu
ARRAYS = ("parent", "cost", "mutations", "depth", "clone")
STATS = ("tree_sankoff_spr_us", "tree_sankoff_spr_candidates")


@pytest.fixture(scope="module")
def ctx():
    from vdjer_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _call(ctx, name, **kw):
    c = K.case(name)
    kw.setdefault("start", c["start"])
    kw.setdefault("cost", np.array(c["cost"], np.uint32))
    return ctx.tree_sankoff_spr(c["contigs"], c["clone"], c["anchor"], c["prio"], max_rounds=c["max_rounds"], **kw)


def _same(got, want, what, ancestors=True):
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())
    assert got["info"] == want["info"], (what, got["info"], want["info"])
    if ancestors:
        assert got["anc"] == want["anc"], (what, [i for i, (a, b) in enumerate(zip(got["anc"], want["anc"])) if a != b][:5])
    else:
        assert got["anc"] is None


@pytest.mark.parametrize("name", sorted(K.gpu_cases()))
def test_tree_sankoff_spr_is_the_model(ctx, name, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    got = _call(ctx, name)
    _same(got, K.want(name), name)
    assert ctx.stat("tree_sankoff_spr_candidates") == got["info"]["candidates"] and ctx.stat("tree_sankoff_spr_us") > 0


@pytest.mark.parametrize("name", ["cat20_unit", "random_wild_unit"])
def test_unit_costs_give_tree_sprs_search(ctx, name, monkeypatch):
    """between the two device calls: the same parents, moves, rounds and candidates; NULL costs are unit costs"""
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    c = K.case(name)
    spr = ctx.tree_spr(c["contigs"], c["clone"], c["anchor"], c["prio"], start=c["start"])
    for got in (_call(ctx, name), _call(ctx, name, cost=None)):
        for f in ("parent", "depth", "clone"):
            assert got[f].tobytes() == spr[f].tobytes(), (name, f)
        assert got["info"]["cost"] == got["info"]["mutations"] == spr["info"]["parsimony"]
        assert got["info"]["cost_start"] == spr["info"]["parsimony_start"]
        assert all(got["info"][f] == spr["info"][f] for f in ("moves", "rounds", "candidates", "searched", "moved", "batches", "edges", "internal"))
        assert np.array_equal(got["cost"], got["mutations"].astype(np.int64))
    assert ctx.stat("tree_sankoff_spr_candidates") == ctx.stat("tree_spr_candidates") > 0


@pytest.mark.parametrize("name", ["mixed", "mixed_random"])
def test_several_batches_give_the_same_bytes(ctx, name, monkeypatch):
    """under a knob of 2,500 cells the lineages go in three batches (mixed_random's start is vdjx_nj_parents', which cuts the same)"""
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    unset = _call(ctx, name)
    monkeypatch.setenv("VDJX_NJ_CELLS", "2500")
    got = _call(ctx, name)
    assert got["info"]["batches"] == 3 and unset["info"]["batches"] == 1
    _same(got, K.want(name, 2500), (name, 2500))
    for f in ARRAYS:                                                                  # nothing but info["batches"] moves with the knob
        assert got[f].tobytes() == unset[f].tobytes()
    rest = lambda info: {k: v for k, v in info.items() if k != "batches"}
    assert got["anc"] == unset["anc"] and rest(got["info"]) == rest(unset["info"]) and got["info"]["moves"] > 0


def test_tree_njs_own_parents_as_the_start_give_the_same_bytes(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    c = K.case("random_wild")
    nj = ctx.tree_nj(c["contigs"], c["clone"], c["anchor"], c["prio"])
    got = _call(ctx, "random_wild", start=nj["parent"])
    _same(got, K.want("random_wild"), "start = tree_nj's parents")
    assert (got["info"]["cost_start"], got["info"]["cost"], got["info"]["moves"], got["info"]["candidates"]) == (420, 391, 14, 76832)


def test_without_ancestors_the_counts_are_still_made(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    _same(_call(ctx, "w65", ancestors=False), K.want("w65"), "no ancestors", ancestors=False)


def test_two_calls_give_the_same_bits(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    a, b = _call(ctx, "cat20"), _call(ctx, "cat20")
    for f in ARRAYS:
        assert a[f].tobytes() == b[f].tobytes()
    assert a["anc"] == b["anc"] and a["info"] == b["info"]
    assert (a["info"]["cost_start"], a["info"]["cost"], a["info"]["moves"], a["info"]["rounds"]) == (649, 306, 11, 12)
    assert ctx.stat("tree_sankoff_spr_candidates") == 12056 and ctx.stat("tree_sankoff_spr_us") > 0


def test_refusals(ctx):
    from vdjer_amd.api import VdjxError
    ok = (["ACGT", "ACGA"], [0, 0], [1, 1])
    assert ctx.tree_sankoff_spr(*ok, cost=K.ASYM)["info"] == dict(dict.fromkeys(X.FIELDS, 0), members=2, clones=1, largest_clone=2, batches=1, edges=1,
                                                                   cost_start=7, cost=7, mutations=1)       # T over A
    before = tuple(ctx.stat(s) for s in STATS + ("tree_nj_us",))
    for contigs, clone, anchor, word in [(["ACGT", "ACGA"], [0, -2], [1, 1], "clone"), (["ACGT", "ACGA"], [0, 0], [1, 5], "vdjx_tree_sankoff_spr.*anchor"),
                                         (["ACGT", "ACGA"], [0, 0], [0, 4], "vdjx_tree_sankoff_spr.*empty window"),
                                         (["A" * 4096] * 2, [0, 0], [0, 0], "vdjx_tree_sankoff_spr.*characters")]:
        with pytest.raises(VdjxError, match=word):
            ctx.tree_sankoff_spr(contigs, clone, anchor)
    for cell, value, word in [((2, 2), 1, r"cost\[2\]\[2\] is 1 .the diagonal is 0."), ((1, 3), 0, r"cost\[1\]\[3\] is 0 .an off-diagonal cell"),
                              ((3, 0), 65536, r"cost\[3\]\[0\] is 65536 .an off-diagonal cell")]:
        bad = np.array(K.TSTV, np.uint32)
        bad[cell] = value
        with pytest.raises(VdjxError, match="vdjx_tree_sankoff_spr: " + word):
            ctx.tree_sankoff_spr(*ok, cost=bad)
    with pytest.raises(VdjxError, match="vdjx_tree_sankoff_spr: params.reserved is .1, 0, 0."):
        ctx.tree_sankoff_spr(*ok, _reserved=1)
    assert tuple(ctx.stat(s) for s in STATS + ("tree_nj_us",)) == before              # nothing ran
    empty = ctx.tree_sankoff_spr([], np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert empty["info"] == dict.fromkeys(X.FIELDS, 0) and len(empty["parent"]) == 0 and len(empty["cost"]) == 0 and empty["anc"] == []


def test_a_start_that_is_no_tree_is_refused_before_any_work(ctx):
    from vdjer_amd.api import VdjxError
    case, bad = SK.bad_trees()
    call = lambda start: ctx.tree_sankoff_spr(case["contigs"], case["clone"] + 7, case["anchor"], case["prio"], cost=K.ASYM, start=start)
    assert call(case["start"])["info"]["moves"] > 0
    before = tuple(ctx.stat(s) for s in STATS)
    for what, tree in bad.items():
        with pytest.raises(VdjxError, match="vdjx_tree_sankoff_spr: the start parents of clone 7 .5 members. are no tree"):
            call(tree)
        assert tuple(ctx.stat(s) for s in STATS) == before, what
    outside = case["start"].copy()
    outside[int(np.argmax(outside >= 0))] = len(outside)                              # a slot past the last
    with pytest.raises(VdjxError, match="outside the lineage"):
        call(outside)


def test_a_lineage_of_1025_is_refused_by_size(ctx):
    from vdjer_amd.api import VdjxError
    n = X.MAX_MEMBERS + 1
    before = tuple(ctx.stat(s) for s in STATS + ("tree_nj_us", "tree_mp_us"))
    with pytest.raises(VdjxError, match=f"vdjx_tree_sankoff_spr: clone 5 has {n} members .at most 1024."):
        ctx.tree_sankoff_spr(["ACGTACGT"] * n + ["ACGTACGA"] * 3, [5] * n + [2] * 3, [0] * (n + 3), cost=K.TSTV)
    assert tuple(ctx.stat(s) for s in STATS + ("tree_nj_us", "tree_mp_us")) == before
    four = ctx.tree_sankoff_spr(["ACGTACGT"] * 3 + ["ACGTACGA"], [5] * 4, [0] * 4)    # (and four members are searched)
    assert four["info"]["searched"] == 1 and four["info"]["rounds"] == 1


def test_the_tree_goes_into_split_support_compare_and_newick(ctx, monkeypatch):
    from vdjer_amd import annot
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    c = K.case("mixed_random")
    sk = _call(ctx, "mixed_random", ancestors=False)
    nj = ctx.tree_nj(c["contigs"], c["clone"], c["anchor"], c["prio"], ancestors=False)
    sup = ctx.tree_split_support(c["contigs"], c["clone"], c["anchor"], sk["parent"], prio=c["prio"], replicates=8, seed=5)
    scored = sum(max(0, m - 3) for m in NK.sizes_of(c))
    assert sup["info"]["scored"] == scored == int((sup["support"] >= 0).sum()) and int(sup["support"].max()) <= 8
    both = annot.tree_split_compare(c["clone"], sk["parent"], nj["parent"])
    assert both["info"]["scored"] == scored and both["info"]["rf"] == 2 * (scored - both["info"]["shared"]) > 0
    same = annot.tree_split_compare(c["clone"], sk["parent"], sk["parent"])
    assert same["info"]["shared"] == scored and same["info"]["rf"] == 0
    ids = [f"c{i}" for i in range(len(c["contigs"]))]
    text = annot.tree_nj_newick(ids, c["clone"], sk["parent"], annot.tree_mp_lengths(sk["parent"], sk["mutations"], sk["clone"]),
                                support=sup["support"], replicates=8)
    assert len(text) == sum(1 for m in NK.sizes_of(c) if m > 1) and sum(t.count("/") for t in text) == scored
