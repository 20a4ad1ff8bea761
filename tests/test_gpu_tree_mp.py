"""vdjx_tree_mp on the GPU: every output array, the ancestors and every info field against the model of tests/tree_mp_model.py, exactly --
on the cases of tests/tree_mp_cases.py (tests/test_tree_mp_cpu.py checks that each reaches the edge it is named for: lineages of 1 .. 5
members, swaps whose walk is the root step alone and swaps deep in the tree, windows of 1, 64, 65 and 513 columns, a caterpillar of 130
members, the exported LDS bound and the bound + 1 from the neighbour-joining start, wildcards, all-identical members, thousands of small
lineages that finish in different rounds; stride_all and stride_mixed: so many candidates that k_mp_score's grid is one and two waves
high and a wave walks three column tiles, or tiles 0, 2, 4 and 1, 3, next to lineages of one tile; `widths`: 1 .. 17 tiles in one batch
under a grid of 7; pick_cat140 and pick_random300: more candidates than k_mp_pick has threads, and moves applied from both sides of
its first stride), under three values of VDJX_NJ_CELLS with the start given and with vdjx_nj_parents' start (its batch loop), the stride
cases' trees recounted by a plain Fitch pass, from tree_nj's own parents as the start, with max_rounds = 1, without ancestors, two calls,
and the refusals.  Every model result is computed once."""
import functools

import numpy as np
import pytest

from tests import tree_mp_cases as K
from tests import tree_mp_model as M
from tests import tree_nj_cases as NK
from tests.tree_model import members_of, windows

pytestmark = pytest.mark.gpu
ARRAYS = ("parent", "mutations", "depth", "clone")


@pytest.fixture(scope="module")
def ctx():
    from vdjer_amd import api
    c = api.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _case(name):
    return K.gpu_cases()[name]()


@functools.lru_cache(maxsize=None)
def _want(name, knob=1 << 26):
    c = _case(name)
    return M.tree_mp(c["contigs"], c["clone"], c["anchor"], c["prio"], start=c["start"], max_rounds=c["max_rounds"], cells_knob=knob)


def _call(ctx, name, **kw):
    c = _case(name)
    kw.setdefault("start", c["start"])
    return ctx.tree_mp(c["contigs"], c["clone"], c["anchor"], c["prio"], max_rounds=c["max_rounds"], **kw)


def _same(got, want, what, ancestors=True):
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())
    assert got["info"] == want["info"], (what, got["info"], want["info"])
    if ancestors:
        assert got["anc"] == want["anc"], (what, [i for i, (a, b) in enumerate(zip(got["anc"], want["anc"])) if a != b][:5])
    else:
        assert got["anc"] is None


@pytest.mark.parametrize("name", sorted(K.gpu_cases()))
def test_tree_mp_is_the_model(ctx, name, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    _same(_call(ctx, name), _want(name), name)


@pytest.mark.parametrize("knob,batches", [(1, 7), (2500, 3), (None, 1)])
def test_any_knob_gives_the_same_bytes(ctx, knob, batches, monkeypatch):
    if knob is None:
        monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    else:
        monkeypatch.setenv("VDJX_NJ_CELLS", str(knob))
    got = _call(ctx, "mixed")
    assert got["info"]["batches"] == batches
    _same(got, _want("mixed", knob or 1 << 26), knob)
    for f in ARRAYS:                                                                  # nothing but info["batches"] moves with the knob
        assert np.array_equal(got[f], _want("mixed")[f])
    assert got["anc"] == _want("mixed")["anc"]
    assert {k: v for k, v in got["info"].items() if k != "batches"} == {k: v for k, v in _want("mixed")["info"].items() if k != "batches"}


@pytest.mark.parametrize("knob,batches", [(1, 7), (2500, 3), (None, 1)])
def test_any_knob_gives_the_same_bytes_from_the_neighbour_joining_start(ctx, knob, batches, monkeypatch):
    """mixed_random has no start given: vdjx_nj_parents cuts the same batches as the search, so under a small knob it goes round its batch
    loop several times (with `mixed`, whose start is given, it never runs)"""
    assert _case("mixed_random")["start"] is None
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    unset = _call(ctx, "mixed_random")
    if knob is not None:
        monkeypatch.setenv("VDJX_NJ_CELLS", str(knob))
    got = _call(ctx, "mixed_random")
    assert got["info"]["batches"] == batches == _want("mixed_random", knob or 1 << 26)["info"]["batches"] and unset["info"]["batches"] == 1
    _same(got, _want("mixed_random", knob or 1 << 26), knob)
    for f in ARRAYS:                                                                  # nothing but info["batches"] moves with the knob
        assert got[f].tobytes() == unset[f].tobytes() and np.array_equal(got[f], _want("mixed_random")[f])
    assert got["anc"] == unset["anc"] == _want("mixed_random")["anc"] and got["info"]["moves"] > 0
    rest = lambda info: {k: v for k, v in info.items() if k != "batches"}
    assert rest(got["info"]) == rest(unset["info"]) == rest(_want("mixed_random")["info"])


@pytest.mark.parametrize("name", ["stride_all", "stride_mixed"])
def test_the_stride_cases_trees_recounted_by_plain_fitch(ctx, name, monkeypatch):
    """without the search model: the returned parents of every lineage are a tree, and Fitch's upward pass over it (M.count, all columns
    in one go: no tiles) gives the lineage's mutations, the call's parsimony and no more than the start's.  This holds for any tree, so a
    scorer that mis-summed a tile would pass it with the wrong moves: only test_tree_mp_is_the_model tells, which is why both stay"""
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    case, got = _case(name), _call(ctx, name)
    groups = members_of(case["clone"])
    total, slot0 = 0, len(case["contigs"])
    for key in sorted(groups):
        members, m = groups[key], len(groups[key])
        slots = members + list(range(slot0, slot0 + max(0, m - 2)))
        local = {s: v for v, s in enumerate(slots)}
        root = K.root_of(case, members)
        par = [-1 if v == root else local.get(int(got["parent"][s]), -2) for v, s in enumerate(slots)]
        kids = M.tree_of_parents(m, root, par)
        p = M.count(M.leaf_sets(windows(case["contigs"], members, case["anchor"])[0]), m, root, kids)
        assert p == sum(int(got["mutations"][s]) for v, s in enumerate(slots) if v != root), (name, key)
        total += p
        slot0 += max(0, m - 2)
    assert total == int(got["mutations"][got["parent"] >= 0].sum()) == got["info"]["parsimony"] <= got["info"]["parsimony_start"]
    assert got["info"]["parsimony"] < got["info"]["parsimony_start"] and got["info"]["moves"] > 0


def test_tree_njs_own_parents_as_the_start_give_the_same_bytes(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    c = _case("random_wild")
    nj = ctx.tree_nj(c["contigs"], c["clone"], c["anchor"], c["prio"])
    got = _call(ctx, "random_wild", start=nj["parent"])
    _same(got, _want("random_wild"), "start = tree_nj's parents")
    assert got["info"]["moves"] > 0 and got["info"]["parsimony_start"] == nj["info"]["parsimony"]


def test_without_ancestors_the_counts_are_still_made(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    _same(_call(ctx, "random_wild", ancestors=False), _want("random_wild"), "no ancestors", ancestors=False)


def test_two_calls_give_the_same_bits(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    a = _call(ctx, "cat20")
    steps = ctx.stat("tree_mp_steps")
    b = _call(ctx, "cat20")
    for f in ARRAYS:
        assert a[f].tobytes() == b[f].tobytes()
    assert a["anc"] == b["anc"] and a["info"] == b["info"]
    want = _want("cat20")["info"]["candidates"]
    assert ctx.stat("tree_mp_candidates") == want == 816
    # per column tile a candidate updates v and p at least, and at most every inferred node on its way up: 18 in this lineage of 20
    tiles = (len(a["anc"][0]) + 63) // 64
    assert 2 * want * tiles <= steps == ctx.stat("tree_mp_steps") <= 18 * want * tiles


def _bad_starts():
    """a lineage of five from the caterpillar: (what, local parents) for every way a start can fail to be a tree"""
    case = K.with_caterpillars(NK.infinite_sites(5, 105))
    root = K.root_of(case, list(range(5)))
    l = [v for v in range(5) if v != root]
    good = K.caterpillar(5, root)

    def changed(**kw):
        p = list(good)
        for v, x in kw.items():
            p[int(v[1:])] = x
        return p
    cycle = [-1] * 8
    for v, p in [(5, root), (l[0], 5), (l[1], 5), (6, 7), (7, 6), (l[2], 6), (l[3], 7)]:
        cycle[v] = p                                                                  # every node has the children it should have
    return case, {"a parent outside the lineage": changed(**{f"v{l[0]}": -1}),
                  "a root leaf with two children": changed(**{f"v{l[0]}": root}),
                  "an inferred node with three children": changed(**{f"v{l[3]}": 5}),
                  "a leaf with children": changed(**{f"v{l[3]}": l[0]}),
                  "a cycle": cycle}


def test_refusals(ctx):
    from vdjer_amd.api import VdjxError
    ok = (["ACGT", "ACGA"], [0, 0], [1, 1])
    assert ctx.tree_mp(*ok)["info"]["edges"] == 1
    for contigs, clone, anchor, word in [(["ACGT", "ACGA"], [0, -2], [1, 1], "clone"), (["ACGT", "ACGA"], [0, 0], [1, 5], "anchor"),
                                         (["ACGT", "ACGA"], [0, 0], [0, 4], "empty window"), (["A" * 4096] * 2, [0, 0], [0, 0], "characters")]:
        with pytest.raises(VdjxError, match=word):
            ctx.tree_mp(contigs, clone, anchor)
    with pytest.raises(VdjxError, match="reserved"):
        ctx.tree_mp(*ok, _reserved=1)
    empty = ctx.tree_mp([], np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert empty["info"] == dict.fromkeys(M.FIELDS, 0) and len(empty["parent"]) == 0 and empty["anc"] == []


def test_a_start_that_is_no_tree_is_refused_before_any_work(ctx):
    from vdjer_amd.api import VdjxError
    case, bad = _bad_starts()
    call = lambda start: ctx.tree_mp(case["contigs"], case["clone"] + 7, case["anchor"], case["prio"], start=start)
    assert call(case["start"])["info"]["moves"] > 0
    before = ctx.stat("tree_mp_us")
    for what, local in bad.items():
        with pytest.raises(VdjxError, match="of clone 7 .* are no tree"):
            call(K.start_slots(case, {0: local}))
        assert ctx.stat("tree_mp_us") == before, what
    outside = case["start"].copy()
    outside[int(np.argmax(outside >= 0))] = len(outside)                              # a slot past the last
    with pytest.raises(VdjxError, match="outside the lineage"):
        call(outside)


def test_a_lineage_of_4097_is_refused_by_size(ctx):
    from vdjer_amd.api import VdjxError
    n = M.MAX_MEMBERS + 1
    before = ctx.stat("tree_mp_us"), ctx.stat("tree_nj_us")
    with pytest.raises(VdjxError, match=f"{n} members"):
        ctx.tree_mp(["ACGTACGT"] * n + ["ACGTACGA"] * 3, [5] * n + [2] * 3, [0] * (n + 3))
    assert (ctx.stat("tree_mp_us"), ctx.stat("tree_nj_us")) == before               # refused before the call did anything
