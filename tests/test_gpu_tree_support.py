"""vdjx_tree_support on the GPU: out_support and every info field against the plain model of tests/tree_support_model.py, exactly -- clone
sizes around k_tree_min's row block, window lengths around the 32-base words of the kept columns (486: the 8-word register body; 1100:
about 550 kept columns, the chunked path), a replicate that keeps no column, members cut at shifts, characters that are not ACGT, 1, 2
and 16 replicates, two seeds, 300 small clones interleaved and permuted, several batches (VDJX_TREE_SUPPORT_ROWS), a parent that is not
the tree's, the refusals, the dispatch counts -- and `vdjer --trees --tree-support` on the e2e_families golden against the model's table.
The inputs are built as tests/test_gpu_tree.py builds its descents, parent is the model's tree.  The API cases run in one child
process, the batch cases in another; every model result is computed once."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import families as F
from tests import lineage_model as L
from tests import tree_model as T
from tests import tree_support_model as S
from tests.test_gpu_annot import _child_env
from tests.test_gpu_tables import _api_hits, _sha, _vdjer, golden  # noqa: F401  (_api_hits runs in the child)
from tests.test_gpu_tree import _cut, _descent, _rand

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 3, 63, 64, 65, 129]                                         # the row-block edge; w = 96, B = 4
WINDOWS = [1, 2, 31, 32, 33, 64, 65, 486, 1100]                         # m = 9, B = 3
REPLICATES = [1, 2, 16]
SHIFTS = [0, 1, 31, 33]
BATCHED = ["size_129", "clones_300"]                                    # run again in batches of one replicate and of two (B = 5)
TABLES = ["--airr", "a.tsv", "--quant", "q.tsv", "--lineages", "l.tsv"]


def _run_child(fn, arg, env, timeout=900):
    code = f"import json; from tests.test_gpu_tree_support import {fn}; print('TSUP', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("TSUP ")).split(" ", 1)[1])


def _tree_parent(cs, cl, an):
    return T.tree(cs, cl, an)[0].tolist()


def _empty_seed(replicates):
    """the smallest seed with which some replicate r <= `replicates` keeps neither column of a window of two: found with the model's rule"""
    return next(s for s in range(1, 10000) if any(not S.keeps(s, r, 0) and not S.keeps(s, r, 1) for r in range(1, replicates + 1)))


# ---- the cases: name -> (contigs, clone, anchor, parent, replicates, seed) -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20260)
    out = {}

    def add(name, cs, cl, an, replicates, seed, parent=None):
        out[name] = (cs, cl, an, _tree_parent(cs, cl, an) if parent is None else parent, replicates, seed)

    for m in SIZES:                                                      # one clone of m contigs whose window is all their 96 bases
        add(f"size_{m}", _descent(rng, m, 96), [6] * m, [40] * m, 5 if f"size_{m}" in BATCHED else 4, 1)
    for w in WINDOWS:                                                    # a clone of 9 whose window is w bases, in contigs of w + 3
        longs = _descent(rng, 9, w, 3)
        a0 = w // 3
        cs = [_rand(rng, 3) + s if k % 2 else s + _rand(rng, 3) for k, s in enumerate(longs)]
        add(f"window_{w}", cs, [0] * 9, [a0 + 3 if k % 2 else a0 for k in range(9)], 3, 2)
    # a replicate that keeps nothing: a window of two and a seed with which some r <= 4 keeps neither column
    add("keeps_nothing", ["AC", "AG", "AC", "TC", "TG", "AC"], [0] * 6, [1] * 6, 4, _empty_seed(4))
    # members cut at shifts 0, 1, 31 and 33 inside one clone: windows of 70 bases in contigs of 103, the anchor at 10 + shift
    wins = _descent(rng, 8, 70)
    shifts = [SHIFTS[k % 4] for k in range(8)]
    add("shifts", [_rand(rng, s) + win + _rand(rng, 33 - s) for win, s in zip(wins, shifts)], [0] * 8, [10 + s for s in shifts], 4, 3)
    f = _rand(rng, 40)
    other = [f, f[:10] + "N" + f[11:], f[:10] + "N" + f[11:], f.lower(), f[:39] + "*", f[:39] + "*", f[:20] + f[20:].lower(), "N" * 40, "N" * 40,
             f[:5] + "n" + f[6:], f[:31] + "N" + f[32:], f[:32] + "N" + f[33:], f]
    add("not_acgt", other, [0] * len(other), [0] * len(other), 4, 5)
    cs = _descent(rng, 20, 64)
    for b in REPLICATES:
        add(f"replicates_{b}", cs, [2] * 20, [30] * 20, b, 1)
    add("other_seed", cs, [2] * 20, [30] * 20, 16, 2)
    # 300 clones of 1 .. 8 members, interleaved, with items that take no part among them
    cs, cl, an = [], [], []
    for k in range(300):
        m = 1 + k % 8
        c1, a1 = _cut(rng, _descent(rng, m, 36), 30, 16)
        cs += c1
        an += a1
        cl += [k * 2000003 % 2147483647] * m
    for _ in range(60):
        cs.append(_rand(rng, 30))
        an.append(int(rng.integers(-5, 40)))                             # (any anchor where the item takes no part)
        cl.append(-1)
    order = rng.permutation(len(cs)).tolist()
    cs, cl, an = [cs[k] for k in order], [cl[k] for k in order], [an[k] for k in order]
    add("clones_300", cs, cl, an, 5, 1)
    # the same items in another order, scored on the same undirected edges
    order = np.random.default_rng(5).permutation(len(cs)).tolist()
    at = {old: new for new, old in enumerate(order)}
    parent = out["clones_300"][3]
    add("clones_300_permuted", [cs[k] for k in order], [cl[k] for k in order], [an[k] for k in order], 5, 1,
        [-1 if parent[k] < 0 else at[parent[k]] for k in order])
    # a parent that is not the tree: every member points at the clone's smallest index
    cs, cl, an = out["size_65"][:3]
    add("star_parent", cs, cl, an, 4, 1, [-1] + [0] * 64)
    return out


@functools.lru_cache(maxsize=None)
def models():
    return {name: S.support(*c) for name, c in cases().items()}


def _in_trees(name):
    """the members of the case's clones of two and more: the rows of one replicate"""
    return sum(len(v) for v in T.members_of(cases()[name][1]).values() if len(v) > 1)


def _pack(res):
    return dict(support=res["support"].tolist(), dtype=str(res["support"].dtype), info=res["info"])


def _dispatch_inputs():
    """same largest clone (8), very different clone counts; and a larger clone"""
    rng = np.random.default_rng(9)
    one = _descent(rng, 8, 45)
    many = [s for _ in range(500) for s in _descent(rng, 8, 45)]
    big = _descent(rng, 200, 45)
    star = [-1 if k % 8 == 0 else k - k % 8 for k in range(4000)]        # (scored: every member's edge to its clone's first)
    return {"one_clone_of_8": (one, [0] * 8, [5] * 8, star[:8]), "500_clones_of_8": (many, [k // 8 for k in range(4000)], [5] * 4000, star),
            "one_clone_of_200": (big, [0] * 200, [5] * 200, [-1] + [0] * 199)}


def _device(_):
    import ctypes as C
    from vdjer_amd import _lib, api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    ctx.tree_support(["ACGT", "ACGA"], [0, 0], [0, 0], [-1, 0], 1, 1)    # (the workspace is there before the kept bytes are read)
    kept0, allocs0 = ctx.stat("kept_device_bytes"), ctx.stat("kept_allocs")
    out = dict(cases={}, batches={}, work_items={}, dispatches={})
    for name, (cs, cl, an, pa, b, seed) in cases().items():
        res = ctx.tree_support(cs, cl, an, pa, b, seed)
        out["batches"][name], out["work_items"][name] = ctx.stat("tree_support_batches"), ctx.stat("tree_support_work_items")
        again = ctx.tree_support(cs, cl, an, pa, b, seed)                # the same seed called twice gives the same bits
        assert again["support"].tobytes() == res["support"].tobytes() and again["info"] == res["info"], name
        out["cases"][name] = _pack(res)
    assert ctx.stat("kept_device_bytes") == kept0 and ctx.stat("kept_allocs") == allocs0      # scratch is the workspace's: nothing is kept
    cs, cl, an, pa, b, seed = cases()["not_acgt"]
    packed = ctx.tree_support(api.Context.pack_strings(cs), cl, an, pa, b, seed)              # (the contigs packed by the caller)
    assert packed["support"].tolist() == out["cases"]["not_acgt"]["support"]
    # the parent of vdjx_tree itself, and the defaults (100 replicates, seed 1)
    cs, cl, an = cases()["size_65"][:3]
    tr = ctx.tree(cs, cl, an)
    out["from_tree"] = _pack(ctx.tree_support(cs, cl, an, tr["parent"], 4, 1))
    out["defaults"] = ctx.tree_support(cs[:5], cl[:5], an[:5], [-1, 0, 0, 0, 0])["info"]
    for name, (cs, cl, an, pa) in _dispatch_inputs().items():
        ctx.profile(True)
        ctx.profile_reset()
        out["dispatches"][name] = dict(info=ctx.tree_support(cs, cl, an, pa, 3, 1)["info"])
        out["dispatches"][name]["counts"] = {k: v[1] for k, v in ctx.profile_get().items()}
        ctx.profile(False)
    # no item; refusals: vdjx_last_error names the argument
    r0 = ctx.tree_support([], [], [], [], 3, 1)
    assert r0["support"].shape == (0,) and r0["info"] == dict.fromkeys(S.FIELDS, 0)
    good = ["ACGTACGT", "ACGTACGA", "ACGTACGG", "ACGTACGT"]
    cl, an, pa = [0, 0, 0, 1], [0, 0, 0, 0], [-1, 0, 0, -1]
    assert ctx.tree_support(good, cl, an, pa, 2, 1)["support"].tolist() == [-1, 2, 2, -1]
    for b in (0, 1025, 4000000000):
        with pytest.raises(VdjxError, match="replicates"):
            ctx.tree_support(good, cl, an, pa, b, 1)
    assert ctx.tree_support(good, cl, an, pa, 1024, (1 << 64) - 1)["info"]["replicates"] == 1024
    for bad_parent in ([-1, 1, 0, -1], [-1, 0, 4, -1], [-2, 0, 0, -1], [-1, 0, 0, 0], [-1, 0, 3, -1]):      # itself; outside -1 .. n-1; another clone
        with pytest.raises(VdjxError, match="parent"):
            ctx.tree_support(good, cl, an, bad_parent, 2, 1)
    with pytest.raises(VdjxError, match="parent.*no clone"):            # a parent on an item that takes no part
        ctx.tree_support(good, [0, 0, -1, 1], an, [-1, 0, 0, -1], 2, 1)
    assert ctx.tree_support(good, [0, 0, -1, 1], [0, 0, 99, 0], [-1, 0, -1, -1], 2, 1)["support"].tolist() == [-1, 2, -1, -1]
    # everything vdjx_tree refuses
    for bad_clone in ([0, -2, 0, 1], [-5, 0, 0, 1]):
        with pytest.raises(VdjxError, match="clone"):
            ctx.tree_support(good, bad_clone, an, [-1] * 4, 2, 1)
    for bad_anchor in ([0, -1, 0, 0], [0, 0, 9, 0]):
        with pytest.raises(VdjxError, match="anchor"):
            ctx.tree_support(good, cl, bad_anchor, pa, 2, 1)
    with pytest.raises(VdjxError, match="empty window"):
        ctx.tree_support(good, cl, [0, 3, 8, 0], pa, 2, 1)
    with pytest.raises(VdjxError, match="NUL"):
        ctx.tree_support((b"ACGTAC\0TACGTACGTACGTACGT", 3, 8), [0, 0, 0], [0, 0, 0], [-1, 0, 0], 2, 1)
    with pytest.raises(VdjxError, match="characters"):
        ctx.tree_support((b"A" * 8192, 2, 4096), [0, 0], [0, 0], [-1, 0], 2, 1)
    assert ctx.tree_support((b"A" * 8190, 2, 4095), [0, 0], [0, 0], [-1, 0], 2, 1)["support"].tolist() == [-1, 2]
    # the raw call: NULL parent, NULL out_support, 2^20 items, n = 0
    Lb, h = ctx.L, ctx.h
    info = _lib.TreeSupportInfo()
    params = _lib.TreeSupportParams(2, 1)
    z3, o3 = np.zeros(3, np.int32), np.zeros(3, np.int32)
    p3 = np.array([-1, 0, 0], np.int32)
    info.members = 99
    rc = Lb.vdjx_tree_support(h, b"ACGTACGTACGT", 3, 4, api._p(z3), api._p(z3), None, C.byref(params), api._p(o3), C.byref(info))
    assert rc == -1 and b"NULL" in Lb.vdjx_last_error() and b"parent" in Lb.vdjx_last_error() and info.members == 0
    rc = Lb.vdjx_tree_support(h, b"ACGTACGTACGT", 3, 4, api._p(z3), api._p(z3), api._p(p3), C.byref(params), None, None)
    assert rc == -1 and b"NULL" in Lb.vdjx_last_error() and b"out_support" in Lb.vdjx_last_error()
    rc = Lb.vdjx_tree_support(h, b"ACGTACGTACGT", 3, 4, api._p(z3), api._p(z3), api._p(p3), C.byref(params), api._p(o3), C.byref(info))
    assert rc == 0 and o3.tolist() == [-1, 2, 2] and [getattr(info, f) for f in S.FIELDS] == [3, 1, 3, 2, 1, 2, 2, 4, 2]
    big = 1 << 20
    zb = np.zeros(big, np.int32)
    none = np.full(big, -1, np.int32)
    rc = Lb.vdjx_tree_support(h, b"A" * big, big, 1, api._p(none), api._p(zb), api._p(none), C.byref(params), api._p(zb.copy()), None)
    assert rc == -1 and b"2^20" in Lb.vdjx_last_error()
    info.matched = 5
    rc = Lb.vdjx_tree_support(h, None, 0, 0, None, None, None, None, None, C.byref(info))      # n = 0 returns at once
    assert rc == 0 and [getattr(info, f) for f in S.FIELDS] == [0] * 9
    ctx.close()
    return out


def _device_batched(_):
    """the BATCHED cases with VDJX_TREE_SUPPORT_ROWS such that a batch holds exactly one replicate, then two (which does not divide B = 5)"""
    from vdjer_amd import api
    ctx = api.Context(0)
    out = {}
    for name in BATCHED:
        cs, cl, an, pa, b, seed = cases()[name]
        m = _in_trees(name)
        for per_batch, rows in ((1, 2 * m - 1), (2, 2 * m + m // 2)):
            os.environ["VDJX_TREE_SUPPORT_ROWS"] = str(rows)
            res = _pack(ctx.tree_support(cs, cl, an, pa, b, seed))
            res["stat"] = ctx.stat("tree_support_batches")
            out[f"{name}/{per_batch}"] = res
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def device():
    env = _child_env("shipped")
    env.pop("VDJX_TREE_SUPPORT_ROWS", None)
    return _run_child("_device", "x", env)


@functools.lru_cache(maxsize=None)
def device_batched():
    return _run_child("_device_batched", "x", _child_env("shipped", VDJX_TREE_SUPPORT_ROWS="1"))


def _same(dev, model, what):
    sup, info = model
    assert dev["dtype"] == "int32", what
    a, b = np.asarray(dev["support"], np.int64), sup.astype(np.int64)
    assert np.array_equal(a, b), (what, np.argwhere(a != b)[:5].tolist(), a[:16].tolist(), b[:16].tolist())
    assert dev["info"] == info, (what, dev["info"], info)


def _case(name):
    _same(device()["cases"][name], models()[name], name)
    assert device()["batches"][name] == models()[name][1]["batches"], name
    return models()[name]


@pytest.mark.parametrize("m", SIZES)
def test_support_clone_sizes_around_the_row_block(m):
    sup, info = _case(f"size_{m}")
    b = cases()[f"size_{m}"][4]
    assert info["largest_clone"] == m and info["edges"] == m - 1 and info["rounds"] == (m - 1).bit_length() and info["batches"] == 1
    assert device()["work_items"][f"size_{m}"] == b * (-(-m // 64)) ** 2 and 0 <= sup[1:].min() and sup.max() <= b


@pytest.mark.parametrize("w", WINDOWS)
def test_support_window_lengths(w):
    name = f"window_{w}"
    _case(name)
    cs, cl, an = cases()[name][:3]
    assert sum(T.window_of(range(9), an, len(cs[0]))) == w
    kept = [sum(S.keep(2, r, w)) for r in (1, 2, 3)]
    if w == 486:
        assert [-(-k // 32) for k in kept] == [8, 8, 9], kept            # the register bodies of 8 and of 9 words
    if w == 1100:
        assert [-(-k // 32) for k in kept] == [18, 17, 18], kept          # past the 16 words of the register path: the chunked one


def test_support_a_replicate_that_keeps_nothing():
    sup, info = _case("keeps_nothing")
    seed = cases()["keeps_nothing"][5]
    empty = [r for r in range(1, 5) if not any(S.keep(seed, r, 2))]
    assert empty and info["edges"] == 5
    # with nothing kept the replicate's tree is the star at index 0: an edge to 0 is in it, any other is not
    parent = cases()["keeps_nothing"][3]
    assert all(sup[i] >= len(empty) for i in range(6) if parent[i] == 0) and all(sup[i] <= 4 - len(empty) for i in range(6) if parent[i] > 0)
    assert any(parent[i] > 0 for i in range(6))


def test_support_members_cut_at_shifts():
    _case("shifts")
    cs, cl, an = cases()["shifts"][:3]
    assert sorted({a - 10 for a in an}) == SHIFTS and sum(T.window_of(range(8), an, 103)) == 70


def test_support_characters_that_are_not_acgt():
    sup, info = _case("not_acgt")
    parent = cases()["not_acgt"][3]
    assert parent[12] == 0 and sup[12] == 4                               # the only pair at distance 0, in every replicate


@pytest.mark.parametrize("b", REPLICATES)
def test_support_replicate_counts(b):
    sup, info = _case(f"replicates_{b}")
    assert info["replicates"] == b and info["edges"] == 19 and sup.max() <= b


def test_support_two_seeds_differ_and_replicates_are_a_prefix():
    a, b = _case("replicates_16")[0], _case("other_seed")[0]
    assert a.tolist() != b.tolist()
    # replicate r does not depend on B: the supports grow with the replicates
    one, two = models()["replicates_1"][0], models()["replicates_2"][0]
    assert (one <= two).all() and (two <= a).all()


def test_support_many_small_clones_and_a_permutation():
    """The permuted input is scored on the same undirected edges.  Its supports are the model's for the permuted input, bit for bit; they
    are the first input's supports moved along only where no replicate meets a tie, because the index tie-break follows the order"""
    sup, info = _case("clones_300")
    assert info["clones"] == 300 and info["largest_clone"] == 8 and info["rounds"] == 3 and (sup == -1).sum() == 60 + 300
    psup, pinfo = _case("clones_300_permuted")
    assert {k: v for k, v in pinfo.items() if k not in ("matched", "full")} == {k: v for k, v in info.items() if k not in ("matched", "full")}
    assert sorted((psup >= 0).tolist()) == sorted((sup >= 0).tolist())


@pytest.mark.parametrize("name", BATCHED)
def test_support_in_several_batches(name):
    want = device()["cases"][name]
    assert want["info"]["batches"] == 1 and want["info"]["replicates"] == 5
    for per_batch, batches in ((1, 5), (2, 3)):
        got = device_batched()[f"{name}/{per_batch}"]
        assert got["support"] == want["support"], (name, per_batch)
        assert got["info"] == dict(want["info"], batches=batches) and got["stat"] == batches, (name, per_batch, got["info"])
        m = _in_trees(name)
        rows = 2 * m - 1 if per_batch == 1 else 2 * m + m // 2
        assert S.support(*cases()[name], rows=rows)[1] == got["info"]


def test_support_of_a_parent_that_is_not_the_tree():
    sup, info = _case("star_parent")
    tree_parent = cases()["size_65"][3]
    assert info["edges"] == 64 and any(tree_parent[i] != 0 for i in range(1, 65))
    # where the star's edge is the tree's edge the two cases count the same replicates
    ref = models()["size_65"][0]
    assert all(sup[i] == ref[i] for i in range(1, 65) if tree_parent[i] == 0)


def test_support_from_vdjx_trees_own_parent_and_the_defaults():
    _same(device()["from_tree"], models()["size_65"], "from_tree")
    assert device()["defaults"]["replicates"] == 100 and device()["defaults"]["edges"] == 4
    cs, cl, an = cases()["size_65"][:3]
    assert device()["defaults"] == S.support(cs[:5], cl[:5], an[:5], [-1, 0, 0, 0, 0], 100, 1)[1]


def test_support_dispatches_grow_with_the_rounds_only():
    d = device()["dispatches"]
    small = {"k_tree_pack_sel": 1, "k_tree_min_first": 1, "k_tree_min": 2, "k_tree_hook": 3, "k_tree_flat": 3, "k_tree_support": 1}
    assert d["one_clone_of_8"]["counts"] == d["500_clones_of_8"]["counts"] == small, d
    assert d["one_clone_of_200"]["counts"] == {"k_tree_pack_sel": 1, "k_tree_min_first": 1, "k_tree_min": 7, "k_tree_hook": 8, "k_tree_flat": 8,
                                               "k_tree_support": 1}, d
    assert all(v["info"]["batches"] == 1 and v["info"]["replicates"] == 3 for v in d.values())
    assert d["500_clones_of_8"]["info"]["clones"] == 500 and d["one_clone_of_8"]["info"]["clones"] == 1


# ---- vdjer --trees --tree-support --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tree_support")
    fam = F.build()
    F.write_ref_dir(fam, str(d / "ref"))
    F.write_cfa(fam, str(d / "c.fa"))
    F.pool(fam).write_reads_file(str(d / "reads.txt"))
    return d


def test_vdjer_cli_tree_support_table(inputs):
    from vdjer_amd import annot
    env = _child_env("shipped")
    env.pop("VDJX_TREE_SUPPORT_ROWS", None)
    code = "import json; from tests.test_gpu_tree_support import _api_hits; print('TSUP', json.dumps(_api_hits(0)))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    x = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("TSUP ")).split(" ", 1)[1])
    ids, seqs = golden()
    clone = L.lineage(x["junctions"], x["group"])[0]
    v = {k: np.asarray(a) for k, a in x["v"].items()}
    anchor, prio = annot.tree_inputs(ids, seqs, v, clone)
    parent, dist, depth, tinfo = T.tree(seqs, clone, anchor, prio)
    sup, info = S.support(seqs, clone, anchor, parent, 16, 7)
    want = S.table_text(S.table_rows(ids, seqs, clone, anchor, prio, parent, dist, depth, sup, 16))
    assert info["edges"] == tinfo["edges"] >= 3 and info["matched"] > 0 and (clone < 0).any()      # the golden has edges to speak of

    d, lines = _vdjer(inputs, "support", TABLES + ["--trees", "t.tsv", "--tree-support", "16", "--tree-seed", "7"], env)
    assert (d / "t.tsv").read_text() == want
    at = next(i for i, l in enumerate(lines) if l.startswith("trees: "))
    assert lines[at] == T.summary_line(tinfo) and lines[at + 1] == S.summary_line(info, 7), lines[at:at + 3]
    plain, lines0 = _vdjer(inputs, "plain", TABLES + ["--trees", "t.tsv"], env)
    assert not any(l.startswith("tree support: ") for l in lines0)
    # without the support column the table is the plain --trees table
    rows = [l.split("\t") for l in (d / "t.tsv").read_text().split("\n")[:-1]]
    assert all(len(row) == 10 for row in rows) and rows[0][9] == "support"
    assert "".join("\t".join(row[:9]) + "\n" for row in rows) == (plain / "t.tsv").read_text()
    for fn in ("a.tsv", "q.tsv", "l.tsv", "out.sam", "vdj_contigs.fa", "vdjer.dot"):
        assert _sha(d / fn) == _sha(plain / fn), fn
    # the seed's default is 1; rank 0 calls under --gpus 2
    sup1, info1 = S.support(seqs, clone, anchor, parent, 16, 1)
    want1 = S.table_text(S.table_rows(ids, seqs, clone, anchor, prio, parent, dist, depth, sup1, 16))
    two, lines2 = _vdjer(inputs, "two", ["--gpus", "2", "--airr", "a.tsv", "--lineages", "l.tsv", "--trees", "t.tsv", "--tree-support", "16"],
                         _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert any("k-mer table sharded over 2 GPUs" in l for l in lines2)
    assert (two / "t.tsv").read_text() == want1 and S.summary_line(info1, 1) in lines2
