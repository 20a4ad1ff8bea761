"""vdjx_tree_split_support without a GPU: the case table of tests/tree_split_cases.py reaches what it is there for -- proved by the model of
tests/tree_split_model.py alone --, vdjx_tree_split_compare (plain C) against the model with every refusal, the Newick labels, and what
the header, vdjer_amd/_lib.py and vdjer_amd/api.py say about the call.

A signature run longer than one (two different clades of one lineage with the same wrap-around sum of mix64) cannot be made by hand: it
would take a collision of a 64-bit mix.  The verify step behind the signature is checked instead through vdjx_tree_split_compare, on two
trees whose clades differ in the last word only (test_clades_that_differ_in_the_last_word_only)."""
import ctypes as C

import numpy as np
import pytest

from tests import tree_nj_model as N
from tests import tree_split_cases as K
from tests import tree_split_model as M
from tests import tree_support_model as S
from tests.tree_model import members_of, window_of

NAMES = sorted(K.gpu_cases())


def _lineages(name):
    c = K.case(name)
    groups = members_of(c["clone"])
    return c, [(groups[k], K.want(name)["reach"]["per_lineage"][k]) for k in sorted(groups)]


def test_the_table_holds_the_sizes_roots_and_windows():
    sizes, widths, roots = set(), set(), set()
    for name in NAMES:
        c, lin = _lineages(name)
        assert c["replicates"] <= 16 and 0 < len(c["parent"]) == N.nodes_of(c["clone"])
        for members, r in lin:
            m = len(members)
            assert m == r["m"] <= 129
            sizes.add(m)
            widths.add(sum(window_of(members, c["anchor"], len(c["contigs"][0]))))
            if m >= 4:
                roots.add("first" if r["root"] == 0 else "last" if r["root"] == m - 1 else "middle")
    assert sizes >= {1, 2, 3, 4, 5, 63, 64, 65, 128, 129}
    assert widths >= {1, 3, 31, 32, 33, 64, 65, 513, K.WIDE}
    assert roots == {"first", "last", "middle"}
    assert {K.case(n)["replicates"] for n in NAMES} >= {1, 16}


def test_four_members_have_one_scored_node_and_three_have_none():
    c, lin = _lineages("small_sizes")
    assert [len(r["support"]) for _, r in lin] == [0, 0, 0, 1, 2]
    want = K.want("small_sizes")
    assert want["info"]["scored"] == 3 and int((want["support"] >= 0).sum()) == 3 and want["info"]["units"] == 2 * 8
    assert (want["support"][:len(c["contigs"])] == -1).all()


def test_some_clade_is_complemented_wherever_the_root_is():
    """the join order's union of children holds the root in some replicate -- with the root first, last and in the middle, with one word
    per clade and with two, and with the root alone in the last word (m129_last: leaf 128)"""
    for name in ("m63_first", "m64_last", "m65_middle", "m128_last", "m129_last", "m129_first", "small_sizes", "w1", "w3", "w31"):
        assert K.want(name)["reach"]["flipped"] > 0, name
    c, lin = _lineages("m129_last")
    assert lin[0][1]["root"] == 128


def test_supports_of_none_all_and_some_replicates():
    seen = set()
    for name in NAMES:
        b = K.case(name)["replicates"]
        for _, r in _lineages(name)[1]:
            seen |= {"none" if s == 0 else "all" if s == b else "some" for s in r["support"]}
            assert all(0 <= s <= b for s in r["support"])
    assert seen == {"none", "all", "some"}
    want = K.want("infinite_sites_20")
    assert 0 < want["info"]["full"] < want["info"]["scored"] and want["info"]["matched"] == int(want["support"][want["support"] >= 0].sum())


def test_a_replicate_keeps_no_column_of_a_lineage():
    assert K.want("w1")["reach"]["empty"] > 0 and K.want("w3")["reach"]["empty"] > 0
    c = K.case("w1")
    assert not all(S.keeps(c["seed"], r, 0) for r in range(1, c["replicates"] + 1))


def test_the_wide_window_keeps_more_than_sixteen_words():
    c = K.case(f"w{K.WIDE}")
    kept = [sum(S.keep(c["seed"], r, K.WIDE)) for r in range(1, c["replicates"] + 1)]
    assert min(kept) > 16 * 32                                                        # past the matrix kernel's register path
    c = K.case("w513")
    assert all(sum(S.keep(c["seed"], r, 513)) <= 16 * 32 for r in range(1, c["replicates"] + 1))


def test_the_scored_trees():
    """the neighbour-joining tree, a caterpillar nobody would infer, tree_mp_model's tree"""
    for name in ("caterpillar", "caterpillar_70"):
        assert K.want(name)["info"]["matched"] < K.want(name)["info"]["scored"]
    c = K.case("mp_tree")
    nj = K.scored_nj(c)
    assert not np.array_equal(nj, c["parent"])                                        # the search moved something
    assert M.split_compare(c["clone"], nj, c["parent"])["info"]["rf"] > 0
    # identical members, tied keys: every replicate has the same tree
    assert K.want("identical")["info"]["full"] == K.want("identical")["info"]["scored"] == 4
    c, lin = _lineages("n_column")
    a, b = window_of(lin[0][0], c["anchor"], len(c["contigs"][0]))
    ws = [c["contigs"][i][c["anchor"][i] - a:c["anchor"][i] + b] for i in lin[0][0]]
    assert all(s[20] == "N" for s in ws) and [s[3] == "N" for s in ws] == [False, True] + [False] * 7


@pytest.mark.parametrize("knob,batches", [(1, 25), (K.SPLIT_KNOB, 11), (1 << 26, 1)])
def test_the_batches_of_mixed(knob, batches):
    want = K.want("mixed", knob)
    assert want["info"]["batches"] == batches and want["info"]["units"] == 25
    assert np.array_equal(want["support"], K.want("mixed")["support"]) and np.array_equal(want["trees"], K.want("mixed")["trees"])
    assert want["info"]["replicates"] < 11 < want["info"]["units"]                    # 2500 cells: neither whole replicates nor single units


def _lib():
    from vdjer_amd import _lib
    return _lib


def test_the_symbols_and_the_struct_sizes():
    L = _lib()
    for s in ("vdjx_tree_split_support", "vdjx_tree_split_compare"):
        assert s in L.SYMBOLS and hasattr(L.lib(), s)
    assert C.sizeof(L.TreeSplitParams) == 16 and C.sizeof(L.TreeSplitInfo) == 64
    assert [f for f, _ in L.TreeSplitInfo._fields_] == M.FIELDS
    from vdjer_amd import api
    assert list(api.Context.TREE_SPLIT_FIELDS) == M.FIELDS
    with open(K.K.HERE + "/../include/vdjx.h") as f:
        text = f.read()
    assert "vdjx_tree_split_params;" in text and "/* 64 bytes */" in text.split("vdjx_tree_split_info;")[1][:120]
    assert "support values for this tree;" not in text


def _compare(clone, a, b):
    from vdjer_amd import annot
    return annot.tree_split_compare(clone, a, b)


def _same(got, want):
    assert got["shared"].dtype == np.int32 and np.array_equal(got["shared"], want["shared"]) and got["info"] == want["info"]


@pytest.mark.parametrize("name", ["small_sizes", "m64_last", "m65_middle", "m129_last", "mixed", "mp_tree", "infinite_sites_20"])
def test_compare_is_the_model(name):
    c = K.case(name)
    nj, cat = K.scored_nj(c), K.scored_caterpillar(c)
    me = _compare(c["clone"], nj, nj)
    _same(me, M.split_compare(c["clone"], nj, nj))
    assert me["info"]["rf"] == 0 and me["info"]["shared"] == me["info"]["scored"] == K.want(name)["info"]["scored"]
    for a, b in ((nj, cat), (cat, nj), (c["parent"], nj)):
        _same(_compare(c["clone"], a, b), M.split_compare(c["clone"], a, b))
    if name != "small_sizes":
        assert _compare(c["clone"], nj, cat)["info"]["rf"] > 0


def test_compare_one_replicate_with_the_scored_tree_is_the_support():
    """with one replicate the support is the indicator that vdjx_tree_split_compare gives for the replicate's tree"""
    c, want = K.case("one_replicate"), K.want("one_replicate")
    got = _compare(c["clone"], c["parent"], want["trees"][0])
    assert np.array_equal(got["shared"], want["support"]) and got["info"]["shared"] == want["info"]["matched"]


def test_clades_that_differ_in_the_last_word_only():
    for m in (67, 128):
        clone, a, b, odd = K.last_word_pair(m)
        got = _compare(clone, a, b)
        _same(got, M.split_compare(clone, a, b))
        assert got["info"] == {"shared": m - 4, "scored": m - 3, "rf": 2} and got["shared"][odd] == 0
        assert (got["shared"][m + 1:odd] == 1).all() and got["shared"][m] == -1 and (got["shared"][:m] == -1).all()


def test_compare_of_trees_rooted_at_different_members():
    """tree b rooted elsewhere has the same splits: the clades of both are taken against tree a's root"""
    c = K.case("infinite_sites_20")
    other = dict(c, prio=np.where(np.arange(len(c["contigs"])) == 3, 0, 1).astype(np.uint32))
    a, b = c["parent"], K.scored_nj(other)
    assert int(np.argmin(a[:20])) != int(np.argmin(b[:20]))
    got = _compare(c["clone"], a, b)
    _same(got, M.split_compare(c["clone"], a, b))
    assert got["info"]["rf"] == 0


def test_compare_refusals():
    from vdjer_amd.api import VdjxError
    case, bad = K.bad_trees()
    good = case["start"]
    assert _compare(case["clone"], good, good)["info"] == {"shared": 2, "scored": 2, "rf": 0}
    for what, tree in bad.items():
        for a, b, which in ((tree, good, "tree a"), (good, tree, "tree b")):
            with pytest.raises(VdjxError, match=f"the parents of {which} of clone 0 .5 members. are no tree"):
                _compare(case["clone"], a, b)
    outside = good.copy()
    outside[int(np.argmax(outside >= 0))] = len(outside)
    with pytest.raises(VdjxError, match="outside the lineage"):
        _compare(case["clone"], outside, good)
    with pytest.raises(VdjxError, match="nodes"):
        _compare(case["clone"], good[:-1], good[:-1])
    with pytest.raises(VdjxError, match="clone below -1"):
        _compare(np.full(5, -2, np.int32), good[:5], good[:5])
    with pytest.raises(VdjxError, match="shape"):
        _compare(case["clone"], good, good[:-1])
    empty = _compare(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert empty["info"] == {"shared": 0, "scored": 0, "rf": 0} and len(empty["shared"]) == 0


def test_the_newick_labels():
    from vdjer_amd import annot
    c, want = K.case("small_sizes"), K.want("small_sizes")
    n = len(c["contigs"])
    ids = [f"c{i}" for i in range(n)]
    keys = sorted(members_of(c["clone"]))
    clone = np.array([keys.index(int(k)) if k >= 0 else -1 for k in c["clone"]], np.int32)      # 0-based lineage numbers
    res = N.tree_nj(c["contigs"], clone, c["anchor"], c["prio"], ancestors=False)
    plain = N.newick(N.node_ids(ids, clone), res["clone"], res["parent"], res["length"])
    assert annot.tree_nj_newick(ids, clone, res["parent"], res["length"]) == plain     # the old output, byte for byte
    b = c["replicates"]
    names = M.newick_names(N.node_ids(ids, clone), n, want["support"], b)
    labelled = annot.tree_nj_newick(ids, clone, res["parent"], res["length"], support=want["support"], replicates=b)
    assert labelled == N.newick(names, res["clone"], res["parent"], res["length"]) != plain
    text = "".join(labelled)
    assert sum(text.count(f"_a{j}/") for j in range(1, 5)) == 3 and "'lin_4_a" in text
    for v in np.flatnonzero(want["support"] >= 0):
        assert f"'{N.node_ids(ids, clone)[v]}/{want['support'][v] / b:.4f}':" in text
    with pytest.raises(ValueError):
        annot.tree_nj_newick(ids, clone, res["parent"], res["length"], support=want["support"])
    with pytest.raises(ValueError):
        annot.tree_nj_newick(ids, clone, res["parent"], res["length"], support=want["support"][:-1], replicates=b)
