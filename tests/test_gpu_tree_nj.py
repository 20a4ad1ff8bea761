"""vdjx_tree_nj on the GPU: every output array, the ancestors and every info field against the plain model of tests/tree_nj_model.py,
exactly -- on the cases of tests/tree_nj_cases.py (tests/test_tree_nj_cpu.py checks that each reaches the edge it is named for: lineages of
1 .. 5 members, the exported LDS bound and the bound + 1, about 300 members on the global path, windows of 1 word, of 512 bases and of 513,
shifted anchors, N and lower case, all-identical members, thousands of small lineages interleaved; `widths`: lineages of 70 members at
every packed word count from 1 to 17 and at 31, 32 and 33, so every register width of k_nj_matrix, its second LDS tile and the chunked
path with a full and a partial last chunk; rand_*: distances that are not additive, whose joins halve odd sums and divide with a
remainder, on the LDS bound, one past it, with a last row block of one row, and at 300 members), under three values of VDJX_NJ_CELLS,
`widths` a lineage and two lineages per batch, without ancestors, the refusals, a lineage of 4,097 and two calls.  No case has a
negative branch: no sequence input that gives one is known.  Every model result is computed once."""
import functools

import numpy as np
import pytest

from tests import tree_nj_cases as K
from tests import tree_nj_model as N

pytestmark = pytest.mark.gpu
ARRAYS = ("parent", "length", "mutations", "depth", "clone")


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
    return N.tree_nj(c["contigs"], c["clone"], c["anchor"], c["prio"], cells_knob=knob)


def _call(ctx, name, **kw):
    c = _case(name)
    return ctx.tree_nj(c["contigs"], c["clone"], c["anchor"], c["prio"], **kw)


def _same(got, want, what, ancestors=True):
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].tolist())
    assert got["info"] == want["info"], (what, got["info"], want["info"])
    if ancestors:
        assert got["anc"] == want["anc"], (what, [i for i, (a, b) in enumerate(zip(got["anc"], want["anc"])) if a != b][:5])
    else:
        assert got["anc"] is None


@pytest.mark.parametrize("name", sorted(K.gpu_cases()))
def test_tree_nj_is_the_model(ctx, name, monkeypatch):
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


@pytest.mark.parametrize("knob,batches", [(K.WIDTH_MEMBERS ** 2, 20), (2 * K.WIDTH_MEMBERS ** 2, 10)])
def test_widths_batch_by_batch_give_the_same_bytes(ctx, knob, batches, monkeypatch):
    """a lineage, or two, per batch: every batch's rows start at another word of the packed rows and have another word count, and the
    distances round (in `mixed`, the other case cut into batches, they are whole)"""
    monkeypatch.setenv("VDJX_NJ_CELLS", str(knob))
    got = _call(ctx, "widths")
    assert got["info"]["batches"] == batches == K.batches_under(K.sizes_of(_case("widths")), knob)
    want = _want("widths")                                                            # (nothing but info["batches"] moves with the knob)
    _same(got, dict(want, info=dict(want["info"], batches=batches)), knob)


def test_without_ancestors_the_counts_are_still_made(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    _same(_call(ctx, "random_wild", ancestors=False), _want("random_wild"), "no ancestors", ancestors=False)


def test_two_calls_give_the_same_bits(ctx, monkeypatch):
    monkeypatch.delenv("VDJX_NJ_CELLS", raising=False)
    a, b = _call(ctx, "lds_bound_plus1"), _call(ctx, "lds_bound_plus1")
    for f in ARRAYS:
        assert a[f].tobytes() == b[f].tobytes()
    assert a["anc"] == b["anc"] and a["info"] == b["info"]
    assert ctx.stat("tree_nj_cells") == 65 * 65 and ctx.stat("tree_nj_joins") == 62


def test_refusals(ctx):
    from vdjer_amd.api import VdjxError
    ok = (["ACGT", "ACGA"], [0, 0], [1, 1])
    assert ctx.tree_nj(*ok)["info"]["edges"] == 1
    for contigs, clone, anchor, word in [(["ACGT", "ACGA"], [0, -2], [1, 1], "clone"), (["ACGT", "ACGA"], [0, 0], [1, 5], "anchor"),
                                         (["ACGT", "ACGA"], [0, 0], [0, 4], "empty window"), (["A" * 4096] * 2, [0, 0], [0, 0], "characters")]:
        with pytest.raises(VdjxError, match=word):
            ctx.tree_nj(contigs, clone, anchor)
    with pytest.raises(VdjxError):
        ctx.tree_nj(["ACGT", "ACG"], [0, 0], [0, 0])                                  # unequal lengths
    empty = ctx.tree_nj([], np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert empty["info"] == dict.fromkeys(N.FIELDS, 0) and len(empty["parent"]) == 0 and empty["anc"] == []


def test_a_lineage_of_4097_is_refused_by_size(ctx):
    from vdjer_amd.api import VdjxError
    n = N.MAX_MEMBERS + 1
    launches = ctx.stat("tree_nj_us")
    with pytest.raises(VdjxError, match=f"{n} members"):
        ctx.tree_nj(["ACGTACGT"] * n + ["ACGTACGA"] * 3, [5] * n + [2] * 3, [0] * (n + 3))
    assert ctx.stat("tree_nj_us") == launches                                         # refused before the call did anything
