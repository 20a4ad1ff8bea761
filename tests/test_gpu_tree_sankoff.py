"""vdjx_tree_sankoff on the GPU: every output array, the ancestors and every info field against the model of tests/tree_sankoff_model.py,
exactly -- on the cases of tests/tree_sankoff_cases.py (tests/test_tree_sankoff_cpu.py checks that each reaches the edge it is named for:
lineages of 1 .. 5 members, windows of 1, 64, 65 and 513 columns, wildcards in leaves and in the root member, all-identical members,
hundreds of small lineages, mixed sizes, a handmade start, a search cut by max_rounds, no search, as many candidates as k_sk_pick has
threads and two more, a scorer wave over several column tiles, and costs past 2^16 per column and 2^32 in all), the unit matrix against
vdjx_tree_mp itself, a VDJX_NJ_CELLS that cuts several batches, without ancestors, two calls, the refusals, and the result in the hands of
tree_split_support, tree_split_compare and the Newick writer.  Every model result is computed once (tests/tree_sankoff_cases.want)."""
import numpy as np
import pytest

from tests import tree_nj_cases as NK
from tests import tree_sankoff_cases as K
from tests import tree_sankoff_model as S
from tests import tree_split_cases as SK

pytestmark = pytest.mark.gpu
ARRAYS = ("parent", "cost", "mutations", "depth", "clone")


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
    return ctx.tree_sankoff(c["contigs"], c["clone"], c["anchor"], c["prio"], search=c["search"], max_rounds=c["max_rounds"], **kw)


def _same(got, want, what, ancestors=True):
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())
    assert got["info"] == want["info"], (what, got["info"], want["info"])
    if ancestors:
        assert got["anc"] == want["anc"], (what, [i for i, (a, b) in enumerate(zip(got["anc"], want["anc"])) if a != b][:5])
    else:
        assert got["anc"] is None


@pytest.mark.parametrize("name", sorted(K.gpu_cases()))
def test_tree_sankoff_is_the_model(ctx, name, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    got = _call(ctx, name)
    _same(got, K.want(name), name)
    assert ctx.stat("tree_sankoff_candidates") == got["info"]["candidates"]
    assert int(got["cost"][got["parent"] >= 0].sum()) == got["info"]["cost"]


@pytest.mark.parametrize("name", [f"unit_{x}" for x in K.UNIT_SHARED])
def test_under_unit_costs_the_tree_is_tree_mps(ctx, name, monkeypatch):
    """parent, depth and clone byte for byte vdjx_tree_mp's on the same input, with the matrix given and with NULL; the totals are its P"""
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    c = K.case(name)
    mp = ctx.tree_mp(c["contigs"], c["clone"], c["anchor"], c["prio"], start=c["start"], max_rounds=c["max_rounds"])
    for got in (_call(ctx, name), _call(ctx, name, cost=None)):
        for f in ("parent", "depth", "clone"):
            assert got[f].tobytes() == mp[f].tobytes(), (name, f)
        assert got["info"]["cost"] == got["info"]["mutations"] == mp["info"]["parsimony"]
        assert got["info"]["cost_start"] == mp["info"]["parsimony_start"]
        assert all(got["info"][f] == mp["info"][f] for f in ("moves", "rounds", "candidates", "searched", "moved", "batches", "edges", "internal"))
        assert np.array_equal(got["cost"], got["mutations"].astype(np.int64))


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
    c = K.case("random_wild_asym")
    nj = ctx.tree_nj(c["contigs"], c["clone"], c["anchor"], c["prio"])
    got = _call(ctx, "random_wild_asym", start=nj["parent"])
    _same(got, K.want("random_wild_asym"), "start = tree_nj's parents")
    assert (got["info"]["cost_start"], got["info"]["cost"], got["info"]["moves"]) == (1109, 1090, 11)


def test_without_ancestors_the_counts_are_still_made(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    _same(_call(ctx, "w65", ancestors=False), K.want("w65"), "no ancestors", ancestors=False)


def test_two_calls_give_the_same_bits(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    a, b = _call(ctx, "cat20"), _call(ctx, "cat20")
    for f in ARRAYS:
        assert a[f].tobytes() == b[f].tobytes()
    assert a["anc"] == b["anc"] and a["info"] == b["info"]
    assert (a["info"]["cost_start"], a["info"]["cost"], a["info"]["moves"], a["info"]["rounds"]) == (649, 367, 25, 26)
    assert ctx.stat("tree_sankoff_candidates") == 26 * 34 and ctx.stat("tree_sankoff_us") > 0
    tiles = K.scorer_grid(K.case("cat20"))[1][0]
    assert 0 < ctx.stat("tree_sankoff_steps") <= 26 * 34 * 18 * tiles                  # at most full rescoring: candidates x (m - 2) per tile


def test_refusals(ctx):
    from vdjer_amd.api import VdjxError
    ok = (["ACGT", "ACGA"], [0, 0], [1, 1])
    assert ctx.tree_sankoff(*ok, cost=K.ASYM)["info"] == dict(dict.fromkeys(S.FIELDS, 0), members=2, clones=1, largest_clone=2, batches=1, edges=1,
                                                               cost_start=7, cost=7, mutations=1)       # T over A
    edge = np.array(K.TSTV, np.uint32)
    edge[3, 0] = 65535
    assert ctx.tree_sankoff(*ok, cost=edge)["info"]["cost"] == 65535
    before = ctx.stat("tree_sankoff_us"), ctx.stat("tree_sankoff_candidates"), ctx.stat("tree_nj_us")
    for contigs, clone, anchor, word in [(["ACGT", "ACGA"], [0, -2], [1, 1], "clone"), (["ACGT", "ACGA"], [0, 0], [1, 5], "vdjx_tree_sankoff.*anchor"),
                                         (["ACGT", "ACGA"], [0, 0], [0, 4], "vdjx_tree_sankoff.*empty window"),
                                         (["A" * 4096] * 2, [0, 0], [0, 0], "vdjx_tree_sankoff.*characters")]:
        with pytest.raises(VdjxError, match=word):
            ctx.tree_sankoff(contigs, clone, anchor)
    for cell, value, word in [((2, 2), 1, r"cost\[2\]\[2\] is 1 .the diagonal is 0."), ((1, 3), 0, r"cost\[1\]\[3\] is 0 .an off-diagonal cell"),
                              ((3, 0), 65536, r"cost\[3\]\[0\] is 65536 .an off-diagonal cell")]:
        bad = np.array(K.TSTV, np.uint32)
        bad[cell] = value
        with pytest.raises(VdjxError, match="vdjx_tree_sankoff: " + word):
            ctx.tree_sankoff(*ok, cost=bad)
    with pytest.raises(VdjxError, match="vdjx_tree_sankoff: params.search is 2"):
        ctx.tree_sankoff(*ok, search=2)
    with pytest.raises(VdjxError, match="vdjx_tree_sankoff: params.reserved is .1, 0."):
        ctx.tree_sankoff(*ok, _reserved=1)
    assert (ctx.stat("tree_sankoff_us"), ctx.stat("tree_sankoff_candidates"), ctx.stat("tree_nj_us")) == before      # nothing ran
    empty = ctx.tree_sankoff([], np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert empty["info"] == dict.fromkeys(S.FIELDS, 0) and len(empty["parent"]) == 0 and len(empty["cost"]) == 0 and empty["anc"] == []


def test_a_start_that_is_no_tree_is_refused_before_any_work(ctx):
    from vdjer_amd.api import VdjxError
    case, bad = SK.bad_trees()
    call = lambda start: ctx.tree_sankoff(case["contigs"], case["clone"] + 7, case["anchor"], case["prio"], cost=K.ASYM, start=start)
    assert call(case["start"])["info"]["moves"] > 0
    before = ctx.stat("tree_sankoff_us"), ctx.stat("tree_sankoff_candidates"), ctx.stat("tree_sankoff_steps")
    for what, tree in bad.items():
        with pytest.raises(VdjxError, match="vdjx_tree_sankoff: the start parents of clone 7 .5 members. are no tree"):
            call(tree)
        assert (ctx.stat("tree_sankoff_us"), ctx.stat("tree_sankoff_candidates"), ctx.stat("tree_sankoff_steps")) == before, what
    outside = case["start"].copy()
    outside[int(np.argmax(outside >= 0))] = len(outside)                              # a slot past the last
    with pytest.raises(VdjxError, match="outside the lineage"):
        call(outside)


def test_a_lineage_past_the_member_limit_is_refused_by_size(ctx):
    from vdjer_amd.api import VdjxError
    n = S.MAX_MEMBERS + 1
    before = ctx.stat("tree_sankoff_us"), ctx.stat("tree_sankoff_candidates"), ctx.stat("tree_nj_us"), ctx.stat("tree_mp_us")
    with pytest.raises(VdjxError, match=f"vdjx_tree_sankoff: clone 5 has {n} members .at most {S.MAX_MEMBERS}."):
        ctx.tree_sankoff(["ACGTACGT"] * n + ["ACGTACGA"] * 3, [5] * n + [2] * 3, [0] * (n + 3))
    assert (ctx.stat("tree_sankoff_us"), ctx.stat("tree_sankoff_candidates"), ctx.stat("tree_nj_us"), ctx.stat("tree_mp_us")) == before


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
