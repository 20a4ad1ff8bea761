"""vdjx_tree_split_support on the GPU: every replicate's tree, every support and every info field against the model of
tests/tree_split_model.py, exactly -- on the cases of tests/tree_split_cases.py (tests/test_tree_split_cpu.py checks what each reaches:
lineages of 1 .. 5, 63, 64, 65, 128 and 129 members, the root first, last and in the middle with clades that are complemented, windows of
1 .. 513 and 1,100 bases, replicates that keep no column, identical members, an N column, the neighbour-joining tree, a caterpillar and
the parsimony tree scored) --, under three values of VDJX_NJ_CELLS, without the trees, the kept columns read back from the trees, two calls,
and the refusals before any GPU work.  Every model result is computed once (tree_split_cases.want)."""
import numpy as np
import pytest

from tests import tree_nj_model as N
from tests import tree_split_cases as K
from tests import tree_split_model as M
from tests.tree_model import distance_matrix, members_of, windows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vdjer_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _call(ctx, name, **kw):
    c = K.case(name)
    kw.setdefault("return_trees", True)
    return ctx.tree_split_support(c["contigs"], c["clone"], c["anchor"], c["parent"], prio=c["prio"], replicates=c["replicates"], seed=c["seed"], **kw)


def _same(got, want, what):
    assert got["support"].dtype == np.int32 and got["trees"].dtype == np.int32 and got["trees"].shape == want["trees"].shape
    bad = np.argwhere(got["trees"] != want["trees"])
    assert len(bad) == 0, (what, "replicate, slot", bad[:5].tolist())
    assert np.array_equal(got["support"], want["support"]), (what, np.flatnonzero(got["support"] != want["support"])[:5].tolist(),
                                                             got["support"][got["support"] != want["support"]][:5].tolist())
    assert got["info"] == want["info"], (what, got["info"], want["info"])


@pytest.mark.parametrize("name", sorted(K.gpu_cases()))
def test_split_support_is_the_model(ctx, name, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    got = _call(ctx, name)
    _same(got, K.want(name), name)
    assert ctx.stat("tree_split_units") == got["info"]["units"] and ctx.stat("tree_split_batches") == got["info"]["batches"]
    plain = _call(ctx, name, return_trees=False)
    assert plain["trees"] is None and plain["support"].tobytes() == got["support"].tobytes() and plain["info"] == got["info"]


@pytest.mark.parametrize("name", ["mixed", "mp_tree"])
@pytest.mark.parametrize("knob", [1, K.SPLIT_KNOB, None])
def test_any_knob_gives_the_same_bytes(ctx, name, knob, monkeypatch):
    if knob is None:
        monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    else:
        monkeypatch.setenv("VDJX_NJ_CELLS", str(knob))
    got = _call(ctx, name)
    _same(got, K.want(name, knob or 1 << 26), (name, knob))
    assert got["info"]["batches"] == (got["info"]["units"] if knob == 1 else 1 if knob is None else got["info"]["batches"])
    if knob == K.SPLIT_KNOB:
        assert got["info"]["replicates"] < got["info"]["batches"] < got["info"]["units"]
    for f in ("support", "trees"):                                                    # nothing but info["batches"] moves with the knob
        assert got[f].tobytes() == K.want(name)[f].tobytes()
    rest = lambda info: {k: v for k, v in info.items() if k != "batches"}
    assert rest(got["info"]) == rest(K.want(name)["info"])
    assert _call(ctx, name, return_trees=False)["support"].tobytes() == got["support"].tobytes()


def test_a_replicates_tree_is_the_joining_on_the_kept_columns(ctx, monkeypatch):
    """with one seed, replicate r's tree is tree_nj_model's joining on exactly the columns annot.jackknife_keep(seed, r, w) gives"""
    from vdjer_amd import annot
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    c = K.case("infinite_sites_20")
    got = _call(ctx, "infinite_sites_20")
    members = members_of(c["clone"])[0]
    ws, _ = windows(c["contigs"], members, c["anchor"])
    m, w, n = len(members), len(ws[0]), len(c["contigs"])
    root = M.root_of(members, c["prio"])
    differ = 0
    for r in range(1, c["replicates"] + 1):
        keep = annot.jackknife_keep(c["seed"], r, w)
        sub = ["".join(ch for ch, k in zip(s, keep) if k) for s in ws]
        par = N.orient(m, N.nj_edges([[int(x) << 16 for x in row] for row in distance_matrix(sub)]), root)[0]
        slot = lambda v: members[v] if v < m else n + v - m
        mine = np.full(len(c["parent"]), -1, np.int32)
        for v, p in enumerate(par):
            mine[slot(v)] = slot(p) if p >= 0 else -1
        assert np.array_equal(got["trees"][r - 1], mine), r
        other = annot.jackknife_keep(c["seed"] + 1, r, w)
        differ += not np.array_equal(keep, other)
    assert differ == c["replicates"]                                                  # (another seed keeps other columns)
    assert _call(ctx, "infinite_sites_20")["trees"].tobytes() == got["trees"].tobytes()
    again = ctx.tree_split_support(c["contigs"], c["clone"], c["anchor"], c["parent"], prio=c["prio"], replicates=c["replicates"], seed=c["seed"] + 1)
    want = M.split_support(c["contigs"], c["clone"], c["anchor"], c["parent"], c["prio"], c["replicates"], c["seed"] + 1)
    assert np.array_equal(again["support"], want["support"]) and again["info"] == want["info"] and not np.array_equal(want["support"], got["support"])


def test_the_scored_tree_from_the_device_and_the_labels(ctx, monkeypatch):
    """tree_nj's and tree_mp's own parents go in as they come out; the supports label the Newick string"""
    from vdjer_amd import annot
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    c = K.case("mixed")
    nj = ctx.tree_nj(c["contigs"], c["clone"], c["anchor"], c["prio"], ancestors=False)
    assert np.array_equal(nj["parent"], c["parent"])
    got = ctx.tree_split_support(c["contigs"], c["clone"], c["anchor"], nj["parent"], prio=c["prio"], replicates=c["replicates"], seed=c["seed"])
    assert np.array_equal(got["support"], K.want("mixed")["support"]) and got["trees"] is None
    c = K.case("mp_tree")
    mp = ctx.tree_mp(c["contigs"], c["clone"], c["anchor"], c["prio"], ancestors=False)
    got = ctx.tree_split_support(c["contigs"], c["clone"], c["anchor"], mp["parent"], prio=c["prio"], replicates=c["replicates"], seed=c["seed"])
    assert np.array_equal(got["support"], K.want("mp_tree")["support"])
    ids = [f"c{i}" for i in range(len(c["contigs"]))]
    text = annot.tree_nj_newick(ids, c["clone"], mp["parent"], annot.tree_mp_lengths(mp["parent"], mp["mutations"], mp["clone"]),
                                support=got["support"], replicates=c["replicates"])
    assert sum(t.count("/") for t in text) == got["info"]["scored"]


def test_refusals_come_before_any_gpu_work(ctx, monkeypatch):
    from vdjer_amd.api import VdjxError
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    assert _call(ctx, "one_replicate")["info"]["units"] == 1
    before = ctx.stat("tree_split_us"), ctx.stat("tree_split_units"), ctx.stat("tree_nj_us")
    assert before[0] > 0
    c = K.case("one_replicate")
    call = lambda **kw: ctx.tree_split_support(**dict(dict(contigs=c["contigs"], clone=c["clone"], anchor=c["anchor"], parent=c["parent"], prio=c["prio"],
                                                           replicates=2, seed=1), **kw))
    two = (["ACGT", "ACGA"], [0, 0], [1, 1], [-1, 0])
    assert ctx.tree_split_support(*two)["info"]["scored"] == 0
    before = ctx.stat("tree_split_us"), ctx.stat("tree_split_units"), ctx.stat("tree_nj_us")
    for contigs, clone, anchor, word in [(["ACGT", "ACGA"], [0, -2], [1, 1], "clone"), (["ACGT", "ACGA"], [0, 0], [1, 5], "anchor"),
                                         (["ACGT", "ACGA"], [0, 0], [0, 4], "empty window"), (["A" * 4096] * 2, [0, 0], [0, 0], "characters")]:
        with pytest.raises(VdjxError, match=word):
            ctx.tree_split_support(contigs, clone, anchor, [-1, 0])
    for b in (0, 1025):
        with pytest.raises(VdjxError, match="replicates"):
            call(replicates=b)
    with pytest.raises(VdjxError, match="reserved"):
        call(_reserved=1)
    with pytest.raises(VdjxError, match="shape"):
        call(parent=c["parent"][:-1])
    case, bad = K.bad_trees()
    for what, tree in bad.items():
        with pytest.raises(VdjxError, match="the parents of clone 7 .5 members. are no tree"):
            ctx.tree_split_support(case["contigs"], case["clone"] + 7, case["anchor"], tree, prio=case["prio"], replicates=2)
    outside = case["start"].copy()
    outside[int(np.argmax(outside >= 0))] = len(outside)
    with pytest.raises(VdjxError, match="outside the lineage"):
        ctx.tree_split_support(case["contigs"], case["clone"], case["anchor"], outside, prio=case["prio"], replicates=2)
    n = N.MAX_MEMBERS + 1
    with pytest.raises(VdjxError, match=f"{n} members"):
        ctx.tree_split_support(["ACGTACGT"] * n, [5] * n, [0] * n, np.full(2 * n - 2, -1, np.int32), replicates=2)
    from vdjer_amd import _lib
    L, i32 = ctx.L, np.zeros(4, np.int32)
    raw = b"ACGTACGA"
    ptr = lambda a: a.ctypes.data_as(_lib.C.c_void_p)
    prm = _lib.TreeSplitParams(2, 0, 1)
    for parent, params, out in ((None, _lib.C.byref(prm), ptr(i32)), (ptr(i32), None, ptr(i32)), (ptr(i32), _lib.C.byref(prm), None)):
        assert L.vdjx_tree_split_support(ctx.h, raw, 2, 4, ptr(i32), ptr(i32), None, parent, params, out, None, None) != 0
        assert b"NULL argument" in L.vdjx_last_error()
    assert (ctx.stat("tree_split_us"), ctx.stat("tree_split_units"), ctx.stat("tree_nj_us")) == before      # refused before any call did anything
    empty = ctx.tree_split_support([], np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), return_trees=True)
    assert empty["info"] == dict.fromkeys(M.FIELDS, 0) and len(empty["support"]) == 0 and empty["trees"].shape == (100, 0)
