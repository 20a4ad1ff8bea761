"""vdjx_lineage on the GPU: clone, nearest and every info field against the plain model of tests/lineage_model.py, exactly -- bucket sizes
around the pair pass's row block and column tile (64), junction lengths around its 32-base words and at every word count, interleaved buckets, a chain that only
holds together link by link, two families one substitution past the threshold, characters that are not ACGT, seeded random repertoires,
permutations, the refusals; buckets of 4,096 and 4,097 and eleven buckets whose column slices hold two tiles, a bucket of 1,000 equal junctions,
2^20 - 1 items, offsets that start past zero -- and `vdjer --lineages` on a heavy-chain and a light-chain golden against the model's table.  The API cases
run in one child process (as tests/test_gpu_dcall.py runs its own); every model result is computed once."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import annot_model as A
from tests import golden_util as G
from tests import lineage_model as M
from tests.test_gpu_annot import RECIPES, _child_env, _vdjer, _write_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 63, 64, 65, 129, 200]                                    # row-block and column-tile edges
LENGTHS = [1, 3, 31, 32, 33, 64, 65, 96, 255]                          # word edges
THRESHOLDS = [0, 500, 1500, 3000, 10000]
FIELDS = ["items", "buckets", "largest_bucket", "clones", "pairs", "links"]
DISPATCHES = {"k_lin_pack": 1, "k_lin_pairs": 1, "k_lin_flatten": 1, "k_lin_number": 1, "k_lin_out": 1}


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_lineage import {fn}; print('LINEAGE', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("LINEAGE ")).split(" ", 1)[1])


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(list(alpha), int(n)))


def _subst(rng, s, positions):
    s = list(s)
    for q in positions:
        s[q] = rng.choice([ch for ch in "ACGT" if ch != s[q]])
    return "".join(s)


def _family(rng, founder, m, frac=0.12):
    """m junctions: the founder and copies with up to frac * L substitutions (the last position among them now and then)"""
    L, out = len(founder), [founder]
    while len(out) < m:
        k = int(rng.integers(0, max(1, int(frac * L)) + 1))
        pos = set(rng.choice(L, size=min(k, L), replace=False).tolist())
        if rng.integers(0, 3) == 0:
            pos.add(L - 1)
        out.append(_subst(rng, founder, sorted(pos)))
    return out


# ---- the cases: name -> (junctions, group, (num, den)) ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20240)
    out = {}
    out["one_item"] = (["ACGTACGTAC"], [7], M.DEFAULT)
    out["all_none"] = (["", "ACGT", "A" * 300, "ACGT"], [M.NONE] * 4, M.DEFAULT)
    for m in SIZES:                                                      # one bucket of m items: two families and a few strangers
        js = (_family(rng, _rand(rng, 45), (m + 1) // 2) + _family(rng, _rand(rng, 45), m // 2))[:m]
        for k in range(0, m, 17):
            js[k] = _rand(rng, 45)
        out[f"size_{m}"] = (js, [3] * m, M.DEFAULT)
    for L in LENGTHS:                                                    # 21 items of L bases; some pairs differ in the last base only
        f = _rand(rng, L)
        js = _family(rng, f, 12, 0.2) + _family(rng, _rand(rng, L), 7, 0.2) + [_subst(rng, f, [L - 1]), f]
        out[f"len_{L}"] = (js, [0] * len(js), (2000, 10000))
        out[f"len_{L}_exact"] = (js, [0] * len(js), (0, 1))
    js, grp = [], []
    founders = {(g, L): _rand(rng, L) for g, L in ((0, 45), (0, 48), (9, 45), (4000000000, 33), (2, 96))}
    for (g, L), f in founders.items():                                  # five buckets, 70 / 30 / 90 / 20 / 66 items, shuffled together
        fam = _family(rng, f, {45: 70, 48: 30, 33: 20, 96: 66}[L] + (20 if g == 9 else 0))
        js += fam
        grp += [g] * len(fam)
    order = rng.permutation(len(js))
    out["interleaved"] = ([js[i] for i in order], [grp[i] for i in order], M.DEFAULT)
    f = _rand(rng, 30)
    out["same_junction_other_group"] = ([f, f, f, _subst(rng, f, [3]), f], [1, 2, 1, 2, M.NONE], M.DEFAULT)
    out["same_group_other_length"] = ([f, f[:29], f[:29], f, f + "A", f[:29] + "C"], [5] * 6, M.DEFAULT)
    # a chain of 200 at L = 60, each one substitution from the previous (position k mod 60 moves on to the next base), shuffled so that the
    # smallest index sits mid-chain.  With 1/60 of the length only neighbours are linked (two steps apart is d = 2): one clone exists only
    # if every one of the 199 links is kept and followed to the end.  With the default 0.15 (d <= 9) the links overlap; one clone as well.
    chain = [_rand(rng, 60)]
    for k in range(1, 200):
        s = chain[-1]
        q = k % 60
        chain.append(s[:q] + "ACGT"[("ACGT".index(s[q]) + 1) % 4] + s[q + 1:])
    order = rng.permutation(200).tolist()
    order.remove(100)
    order.insert(0, 100)                                                 # index 0 is the middle of the chain
    shuffled = [chain[i] for i in order]
    out["chain_neighbours_only"] = (shuffled, [0] * 200, (1, 60))
    out["chain_default"] = (shuffled, [0] * 200, M.DEFAULT)
    # two families of 100 whose closest members (the founders) are at d = 10, one past floor(0.15 * 60) = 9: a's family varies in 0 .. 19,
    # b's in 20 .. 39, and b is a with ten substitutions in 40 .. 59
    a = _rand(rng, 60)
    b = _subst(rng, a, range(40, 50))
    fa = [a] + [_subst(rng, a, rng.choice(20, size=int(rng.integers(1, 3)), replace=False).tolist()) for _ in range(99)]
    fb = [b] + [_subst(rng, b, (20 + rng.choice(20, size=int(rng.integers(1, 3)), replace=False)).tolist()) for _ in range(99)]
    order = rng.permutation(200)
    both = fa + fb
    out["two_families"] = ([both[i] for i in order], [1] * 200, M.DEFAULT)
    f = _rand(rng, 40)
    other = [f, f[:10] + "N" + f[11:], f[:10] + "N" + f[11:], f.lower(), f[:39] + "*", f[:39] + "*", f[:20] + f[20:].lower(), "N" * 40, "N" * 40,
             f[:5] + "n" + f[6:], f[:31] + "N" + f[32:], f[:32] + "N" + f[33:]]
    out["not_acgt"] = (other, [0] * len(other), M.DEFAULT)
    out["not_acgt_exact"] = (other, [0] * len(other), (0, 10000))
    for seed in range(20):                                               # seeded random repertoires
        r = np.random.default_rng(1000 + seed)
        ng = int(r.integers(1, 7))
        js, grp = [], []
        for _ in range(int(r.integers(3, 12))):
            L = int(r.choice([30, 33, 45, 48, 64, 66]))
            founder, g = _rand(r, L), int(r.integers(0, ng))
            for _ in range(int(r.integers(1, 30))):
                k = int(r.integers(0, L // 4 + 1))                        # 0 .. 25 % of the positions
                js.append(_subst(r, founder, r.choice(L, size=k, replace=False).tolist()))
                grp.append(g if r.integers(0, 25) else M.NONE)
        order = r.permutation(len(js))
        out[f"random_{seed}"] = ([js[i] for i in order], [grp[i] for i in order], (int(r.choice(THRESHOLDS)), 10000))
    out.update(_past_one_tile(np.random.default_rng(20241)))
    # every word count from 4 to 8 (1, 2, 3 and 8 are above): in one group a bucket of 65 (two row blocks, two column tiles) and a bucket
    # of 3 of the same word count; two families and a few strangers, the last member of the 65 with an N for its last base
    rng = np.random.default_rng(20242)
    for L in WORD_LENGTHS:
        big = (_family(rng, _rand(rng, L), 33) + _family(rng, _rand(rng, L), 32))
        for k in range(0, 65, 17):
            big[k] = _rand(rng, L)
        big[64] = big[64][:L - 1] + "N"
        small = _family(rng, _rand(rng, small_length(L)), 3)
        order = rng.permutation(68).tolist()
        out[f"words_{L}"] = ([(big + small)[i] for i in order], [2] * 68, M.DEFAULT)
    return out


WORD_LENGTHS = [97, 128, 129, 160, 161, 192, 193, 224, 225]            # 4 .. 8 words, a full last word and one base in it


def small_length(L):
    """another length of the same word count"""
    return L + 1 if L % 32 == 1 else L - 1


def work_items(sizes):
    """the work items vdjx_lineage makes of buckets of these sizes (ham_slice_items, vdjx_hamming.h): row blocks of 64 times column slices of
    max(64, ceil(cells / (64 * 4096) / 64) * 64) columns, cells the sum of the squared sizes -> (items, slice)"""
    cells = sum(m * m for m in sizes)
    per = -(-cells // (64 * 4096))
    width = max(64, -(-per // 64) * 64)
    return sum(-(-m // 64) * -(-m // width) for m in sizes), width


BIG = ["bucket_4096", "bucket_4097", "slice_128_small_buckets", "all_equal_1000", "n_2_20_minus_1"]
SMALL_BUCKETS = [1500, 100, 1500, 1500, 65, 1500, 1500, 1, 1500, 1500, 1500]      # bucket g has SMALL_BUCKETS[g] items


def _step(s, k):
    """s with position k mod len(s) moved on to the next base"""
    q = k % len(s)
    return s[:q] + "ACGT"[("ACGT".index(s[q]) + 1) % 4] + s[q + 1:]


def _past_one_tile(rng):
    """the cases whose column slices hold more than one tile of 64 (a slice is 64 wide until the squared bucket sizes pass 64 * 4096 * 64),
    and those with item indices up to 2^20 - 2"""
    out = {}
    for m, md in ((4096, (1, 45)), (4097, M.DEFAULT)):
        # one bucket of random junctions (none within reach of another at L = 45).  A chain of 131, each one substitution from the
        # previous, lies at random rows: at 1/45 only neighbours are linked, so one clone exists only if every link across row blocks,
        # tiles and slices is found.  Exact duplicates: row 0 and the last row (in the 4,097 case the only column of the last slice), and three more.
        a = rng.integers(0, 4, (m, 45))
        js = ["".join("ACGT"[x] for x in row) for row in a.tolist()]
        at = (1 + rng.choice(m - 2, size=131 + 7, replace=False)).tolist()      # neither row 0 nor the last
        for k in range(1, 131):
            js[at[k]] = _step(js[at[k - 1]], k)
        js[m - 1] = js[0]
        for k in range(3):
            js[at[131 + 2 * k]] = js[at[132 + 2 * k]]
        js[at[137]] = js[at[60]]                                                  # (a copy of a member of the chain: linked to it and to its two neighbours)
        out[f"bucket_{m}"] = (js, [11] * m, md)
    # eleven buckets (one group each), interleaved: 8 x 1500^2 > 64 * 4096 * 64, so every bucket is cut into slices of 128, the 1,500 into
    # eleven of them and 92 columns (a full tile and 28), the buckets of 100, 65 and 1 into one that is narrower than a slice
    js, grp = [], []
    for g, m in enumerate(SMALL_BUCKETS):
        fams = []
        while len(fams) < m:
            fams += _family(rng, _rand(rng, 45), min(m - len(fams), int(rng.integers(1, 40))))
        js += fams
        grp += [g] * m
    order = rng.permutation(len(js)).tolist()
    out["slice_128_small_buckets"] = ([js[i] for i in order], [grp[i] for i in order], M.DEFAULT)
    out["all_equal_1000"] = ([_rand(rng, 45)] * 1000, [0] * 1000, M.DEFAULT)     # every pair a link, every union onto one root
    # 2^20 - 1 items, 300 of which take part: indices 0 .. 99, 2^19 - 50 .. 2^19 + 49 and 2^20 - 101 .. 2^20 - 2, in two groups; every family
    # has members in all three ranges (the sort key keeps the index in its low 20 bits)
    n = (1 << 20) - 1
    where = list(range(100)) + list(range((1 << 19) - 50, (1 << 19) + 50)) + list(range(n - 100, n))
    js, grp = [""] * n, [M.NONE] * n
    members = []
    for g in (3, 0xFFFFFFFE):
        for _ in range(5):
            members += [(g, s) for s in _family(rng, _rand(rng, 45), 30)]
    for k, member in enumerate(members):                                        # member k goes to range k mod 3
        i = where[(k % 3) * 100 + k // 3]
        grp[i], js[i] = member
    out["n_2_20_minus_1"] = (js, grp, M.DEFAULT)
    return out


@functools.lru_cache(maxsize=None)
def models():
    return {name: M.lineage(js, grp, md) for name, (js, grp, md) in cases().items()}


def _pack(res):
    return dict(clone=res["clone"].tolist(), nearest=None if res["nearest"] is None else res["nearest"].tolist(), info=res["info"],
                dtypes=[str(res["clone"].dtype), None if res["nearest"] is None else str(res["nearest"].dtype)])


def _device(_):
    import ctypes as C
    from vdjer_amd import _lib, api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    kept0, allocs0 = ctx.stat("kept_device_bytes"), ctx.stat("kept_allocs")
    out = dict(cases={}, perm={}, dispatches={}, work_items={}, raw={})
    for name, (js, grp, md) in cases().items():
        res = ctx.lineage(js, grp, md)
        out["work_items"][name] = ctx.stat("lineage_work_items")
        again = ctx.lineage(js, grp, md)                                 # two calls give the same bits
        assert again["clone"].tobytes() == res["clone"].tobytes() and again["nearest"].tobytes() == res["nearest"].tobytes() and again["info"] == res["info"], name
        out["cases"][name] = _pack(res)
    assert ctx.stat("kept_device_bytes") == kept0 and ctx.stat("kept_allocs") == allocs0      # scratch is the workspace's: nothing is kept
    bare = ctx.lineage(*cases()["interleaved"][:2], nearest=False)      # out_nearest = NULL
    assert bare["nearest"] is None and bare["clone"].tolist() == out["cases"]["interleaved"]["clone"]
    asbytes = ctx.lineage([s.encode() for s in cases()["not_acgt"][0]], cases()["not_acgt"][1])
    assert asbytes["clone"].tolist() == out["cases"]["not_acgt"]["clone"]
    for name in ("interleaved", "two_families", "random_3", "random_11"):   # the same input in another order
        js, grp, md = cases()[name]
        order = np.random.default_rng(5).permutation(len(js)).tolist()
        out["perm"][name] = dict(order=order, res=_pack(ctx.lineage([js[i] for i in order], [grp[i] for i in order], md)))
    for name in ("one_item", "size_200", "interleaved"):                  # five dispatches whatever n and the number of buckets are
        ctx.profile(True)
        ctx.profile_reset()
        ctx.lineage(*cases()[name])
        out["dispatches"][name] = {k: v[1] for k, v in ctx.profile_get().items()}
        ctx.profile(False)
    # no item; refusals
    r0 = ctx.lineage([], [])
    assert r0["clone"].shape == (0,) and r0["nearest"].shape == (0,) and r0["info"] == dict.fromkeys(FIELDS, 0)
    good = (["ACGTACGT", "ACGTACGA"], [0, 0])
    for bad in ((1, 0), (1, -1), (1, 1000001), (-1, 10), (11, 10)):
        with pytest.raises(VdjxError, match="threshold"):
            ctx.lineage(*good, max_dist=bad)
        with pytest.raises(VdjxError, match="threshold"):
            ctx.lineage([], [], max_dist=bad)
    assert ctx.lineage(*good, max_dist=(1000000, 1000000))["clone"].tolist() == [0, 0]      # (the largest denominator)
    for js in (["ACGT", ""], ["ACGT", "A" * 256]):
        with pytest.raises(VdjxError, match="bases"):
            ctx.lineage(js, [0, 0])
        assert ctx.lineage(js, [0, M.NONE])["clone"].tolist() == [0, -1]                    # (any length where the item takes no part)
    assert ctx.lineage(["A" * 255, "A" * 255], [0, 0])["info"]["links"] == 1
    # the raw call: offsets that decrease, NULL out_clone, 2^20 items
    L, h = ctx.L, ctx.h
    prm, info = _lib.LineageParams(1500, 10000), _lib.LineageInfo()
    clone, grp2 = np.zeros(2, np.int32), np.zeros(2, np.uint32)
    for off in ([0, 4, 3], [4, 0, 8]):
        info.items = 99
        rc = L.vdjx_lineage(h, b"ACGTACGT", api._p(np.array(off, np.uint64)), api._p(grp2), 2, C.byref(prm), api._p(clone), None, C.byref(info))
        assert rc == -1 and b"decrease" in L.vdjx_last_error() and info.items == 0, (off, rc)
    rc = L.vdjx_lineage(h, b"ACGTACGT", api._p(np.array([0, 4, 8], np.uint64)), api._p(grp2), 2, C.byref(prm), None, None, None)
    assert rc == -1 and b"NULL" in L.vdjx_last_error()
    big = 1 << 20
    rc = L.vdjx_lineage(h, b"", api._p(np.zeros(big + 1, np.uint64)), api._p(np.full(big, M.NONE, np.uint32)), big, C.byref(prm), api._p(np.zeros(big, np.int32)),
                        None, None)
    assert rc == -1 and b"2^20" in L.vdjx_last_error()
    rc = L.vdjx_lineage(h, None, None, None, 0, C.byref(prm), None, None, C.byref(info))      # n = 0 returns at once
    assert rc == 0 and [getattr(info, f) for f in FIELDS] == [0] * 6
    # offsets that do not start at 0: seven bytes that belong to no item in front
    js, grp, md = cases()["interleaved"]
    text = "".join(js).encode()
    ends = np.cumsum([0] + [len(s) for s in js]).astype(np.uint64)
    prm = _lib.LineageParams(*md)
    for first, buf in ((0, text), (7, b"GATTACA" + text)):
        clone, near, info = np.zeros(len(js), np.int32), np.zeros(len(js), np.int32), _lib.LineageInfo()
        rc = L.vdjx_lineage(h, buf, api._p(ends + np.uint64(first)), api._p(np.asarray(grp, np.uint32)), len(js), C.byref(prm), api._p(clone), api._p(near), C.byref(info))
        assert rc == 0, L.vdjx_last_error()
        out["raw"][str(first)] = _pack(dict(clone=clone, nearest=near, info={f: int(getattr(info, f)) for f in FIELDS}))
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def device():
    return _run_child("_device", "x", _child_env("shipped"))


def _same(dev, model, what):
    clone, near, info = model
    assert dev["dtypes"] == ["int32", "int32"], what
    a, b = np.asarray(dev["clone"], np.int64), clone.astype(np.int64)
    assert np.array_equal(a, b), (what, "clone", np.argwhere(a != b)[:5].tolist(), a[:16].tolist(), b[:16].tolist())
    a, b = np.asarray(dev["nearest"], np.int64), near.astype(np.int64)
    assert np.array_equal(a, b), (what, "nearest", np.argwhere(a != b)[:5].tolist(), a[:16].tolist(), b[:16].tolist())
    assert dev["info"] == info, (what, dev["info"], info)


def _names(prefix):
    return [k for k in cases() if k.startswith(prefix)]


@pytest.mark.parametrize("name", ["one_item", "all_none"] + [f"size_{m}" for m in SIZES] + ["interleaved", "same_junction_other_group", "same_group_other_length"])
def test_lineage_api_vs_model_bucket_shapes(name):
    _same(device()["cases"][name], models()[name], name)
    clone, near, info = models()[name]
    if name == "all_none":
        assert clone.tolist() == [-1] * 4 and near.tolist() == [-1] * 4 and info == dict.fromkeys(FIELDS, 0)
    if name == "one_item":
        assert clone.tolist() == [0] and near.tolist() == [-1]
    if name.startswith("size_") and int(name[5:]) >= 63:
        assert 1 < info["clones"] < info["items"] and info["links"] > 0 and info["largest_bucket"] == int(name[5:])
    if name == "interleaved":
        assert info["buckets"] == 5 and info["largest_bucket"] == 90 and info["items"] == 276
    if name == "same_junction_other_group":
        assert clone.tolist() == [0, 1, 0, 1, -1]
    if name == "same_group_other_length":
        assert clone.tolist() == [0, 1, 1, 0, 2, 0] and info["buckets"] == 3      # (the last has 30 bases again: one substitution from the first)


@pytest.mark.parametrize("L", LENGTHS)
def test_lineage_api_vs_model_word_edges(L):
    for name in (f"len_{L}", f"len_{L}_exact"):
        _same(device()["cases"][name], models()[name], name)
    clone, near, info = models()[f"len_{L}_exact"]
    assert clone[0] == clone[-1] and (L == 1 or near[-2] == 1) and clone[-2] != clone[0]      # the copy is linked, the one that differs in the last base is not
    if L > 1:
        assert models()[f"len_{L}"][1].max() <= L


@pytest.mark.parametrize("L", WORD_LENGTHS)
def test_lineage_every_word_count(L):
    """every unrolled body of k_lin_pairs that LENGTHS leaves out, at a full last word and at one base in it, past one row block and
    one column tile"""
    name = f"words_{L}"
    _same(device()["cases"][name], models()[name], name)
    js, grp, md = cases()[name]
    clone, near, info = models()[name]
    lengths = [len(s) for s in js]
    assert sorted((lengths.count(ln), ln) for ln in set(lengths)) == [(3, small_length(L)), (65, L)]
    assert -(-small_length(L) // 32) == -(-L // 32) in range(4, 9) and max(lengths) <= 255
    assert info["buckets"] == 2 and info["largest_bucket"] == 65 and info["pairs"] == 65 * 32 + 3 and md == (1500, 10000)
    assert 2 < info["clones"] < 68 and info["links"] > 0 and sum(s.count("N") for s in js) == 1 and [s for s in js if "N" in s][0][-1] == "N"
    assert device()["work_items"][name] == 2 * 2 + 1


def test_lineage_chain_is_one_clone():
    for name in ("chain_neighbours_only", "chain_default"):
        _same(device()["cases"][name], models()[name], name)
        assert device()["cases"][name]["clone"] == [0] * 200 and device()["cases"][name]["info"]["clones"] == 1
    assert models()["chain_neighbours_only"][2]["links"] == 199 and models()["chain_neighbours_only"][1].tolist() == [1] * 200


def test_lineage_two_families_one_past_the_threshold():
    _same(device()["cases"]["two_families"], models()["two_families"], "two_families")
    js, grp, _ = cases()["two_families"]
    clone = np.asarray(device()["cases"]["two_families"]["clone"])
    assert sorted(np.bincount(clone).tolist()) == [100, 100]
    D = M.distance_matrix(js)
    assert D[clone[:, None] != clone[None, :]].min() == 10 and 10 * 10000 > 1500 * 60 >= 9 * 10000


def test_lineage_characters_that_are_not_acgt():
    for name in ("not_acgt", "not_acgt_exact"):
        _same(device()["cases"][name], models()[name], name)
    clone, near, info = models()["not_acgt_exact"]
    assert info["links"] == 0 and info["clones"] == 12 and near[7] == 40 and near[1] == 1      # N against N, '*' against '*': never a match


@pytest.mark.parametrize("seed", range(20))
def test_lineage_random_repertoires(seed):
    name = f"random_{seed}"
    _same(device()["cases"][name], models()[name], name)


def test_lineage_permutation_keeps_the_partition():
    for name, p in device()["perm"].items():
        order, dev = p["order"], p["res"]
        base = device()["cases"][name]
        back = {new: old for new, old in enumerate(order)}              # item `new` of the permuted input is item `old` of the original
        sets = {frozenset(back[i] for i in s) for s in M.partition(dev["clone"])}
        assert sets == M.partition(base["clone"]), name
        assert sorted(dev["nearest"]) == sorted(base["nearest"]) and [dev["nearest"][new] for new in np.argsort(order)] == base["nearest"], name
        assert dev["info"] == base["info"], name
        js, grp, md = cases()[name]
        _same(dev, M.lineage([js[i] for i in order], [grp[i] for i in order], md), name + " permuted")


@pytest.mark.parametrize("name", BIG)
def test_lineage_past_one_column_tile(name):
    """slices of more than one tile (the second trip of k_lin_pairs' tile loop, a partial last tile), a bucket that collapses into one root,
    item indices up to 2^20 - 2.  The work items prove which slice width the call used."""
    js, grp, md = cases()[name]
    _same(device()["cases"][name], models()[name], name)
    clone, near, info = models()[name]
    sizes = {"bucket_4096": [4096], "bucket_4097": [4097], "slice_128_small_buckets": SMALL_BUCKETS, "all_equal_1000": [1000], "n_2_20_minus_1": [150, 150]}[name]
    items, width = work_items(sizes)
    assert device()["work_items"][name] == items, (name, device()["work_items"][name], items, width)
    if name == "bucket_4096":
        assert (items, width) == (64 * 64, 64)
    if name == "bucket_4097":
        assert (items, width) == (65 * 33, 128) and clone[4096] == clone[0] == 0
    if name.startswith("bucket_"):
        m = len(js)
        assert info["largest_bucket"] == m and info["clones"] == m - 130 - 5 and np.bincount(clone).max() == 132 and (near == -1).sum() == 0
        assert info["links"] == 130 + 1 + 3 + 3 if md == (1, 45) else info["links"] > 137
    if name == "slice_128_small_buckets":
        assert width == 128 and items == 8 * 24 * 12 + 2 + 2 + 1 and info["buckets"] == 11 and info["largest_bucket"] == 1500
        assert sorted(np.bincount(np.asarray(grp)).tolist()) == sorted(SMALL_BUCKETS)
    if name == "all_equal_1000":
        assert clone.tolist() == [0] * 1000 and near.tolist() == [-1] * 1000 and info["links"] == 499500 == info["pairs"] and info["clones"] == 1
    if name == "n_2_20_minus_1":
        n = (1 << 20) - 1
        assert len(js) == n and info["items"] == 300 and info["buckets"] == 2 and (clone >= 0).sum() == 300
        for members in M.partition(clone):                               # the families reach across the three index ranges
            if len(members) >= 20:
                assert min(members) < 100 and max(members) >= n - 100 and any(abs(i - (1 << 19)) <= 50 for i in members)
        assert sum(len(s) >= 20 for s in M.partition(clone)) >= 6


def test_lineage_raw_call_with_offsets_that_start_past_zero():
    raw = device()["raw"]
    assert raw["7"] == raw["0"]
    _same(raw["7"], models()["interleaved"], "off[0] = 7")


def test_lineage_dispatches_do_not_depend_on_the_input():
    assert device()["dispatches"] == {name: DISPATCHES for name in ("one_item", "size_200", "interleaved")}, device()["dispatches"]


# ---- vdjer --lineages --------------------------------------------------------------------------------------------------------------------
def _cli_inputs(tag):
    """in a child process: the inputs `vdjer --lineages` derives, from api.Context.annotate and annot.lineage_inputs"""
    from vdjer_amd import annot, api, synth
    rep = synth.make_repertoire(**RECIPES[tag])
    fa = G.text(f"{tag}.contigs.fa.gz").splitlines()
    ids, seqs = [fa[i][1:] for i in range(0, len(fa), 2)], [fa[i + 1] for i in range(0, len(fa), 2)]
    ctx = api.Context(0)
    info = ctx.germline_load([(f"V{i}", v) for i, v in enumerate(rep.v_germ)] + [(f"J{i}", j) for i, j in enumerate(rep.j_germ)])
    hits = ctx.annotate(seqs)
    junctions, group, vgene, jgene = annot.lineage_inputs(ids, seqs, hits["v"], hits["j"], info["names"])
    ctx.close()
    return dict(ids=ids, junctions=junctions, group=group.tolist(), vgene=vgene, jgene=jgene)


def _lineages_line(r):
    lines = r.stderr.splitlines()
    at = next(i for i, l in enumerate(lines) if l.startswith("lineages: "))
    assert not any(l.startswith(("airr: ", "dcalls: ")) for l in lines[at:])      # after the airr: / dcalls: lines
    return lines[at]


def _fresh(tmp_path, name, tag):
    d = tmp_path / name
    d.mkdir()
    _write_inputs(tag, str(d))
    return d


@pytest.mark.parametrize("tag", ["e2e_mixed", "e2e_igk"])
def test_vdjer_cli_lineages_table(tag, tmp_path):
    env = _child_env("shipped")
    x = _run_child("_cli_inputs", tag, env)
    ids, n = x["ids"], len(x["ids"])
    clone, near, info = M.lineage(x["junctions"], x["group"])
    assert info["items"] > 0, info                                       # (the goldens have one and two contigs: the kernels' own cases are above)

    def table(counts=None, model=(clone, near)):
        return M.table_text(M.table_rows(ids, x["junctions"], x["group"], x["vgene"], x["jgene"], model[0], model[1], counts), counts is not None)

    # alone: no quant column
    d = _fresh(tmp_path, "alone", tag)
    r = _vdjer(d, tag, ["--lineages", "l.tsv"], env)
    assert (d / "l.tsv").read_text() == table()
    assert _lineages_line(r) == M.summary_line(n, info)
    assert not any(l.startswith(("airr: ", "quant: ")) for l in r.stderr.splitlines())
    # with the quant step, --airr and --clones: the extra columns; every other output as without --lineages
    full = _fresh(tmp_path, "full", tag)
    r = _vdjer(full, tag, ["--quant", "q.tsv", "--airr", "a.tsv", "--lineages", "l.tsv", "--clones", "c.tsv"], env)
    counts = [l.split("\t")[4] for l in (full / "q.tsv").read_text().splitlines()[1:]]
    assert (full / "l.tsv").read_text() == table(counts) and _lineages_line(r) == M.summary_line(n, info)
    plain = _fresh(tmp_path, "plain", tag)
    r0 = _vdjer(plain, tag, ["--quant", "q.tsv", "--airr", "a.tsv", "--clones", "c.tsv"], env)
    assert not any(l.startswith("lineages: ") for l in r0.stderr.splitlines()) and not (plain / "l.tsv").exists()
    for fn in ("q.tsv", "c.tsv"):
        assert (full / fn).read_bytes() == (plain / fn).read_bytes(), fn
    head, rows = A.read_table(full / "a.tsv")
    head0, rows0 = A.read_table(plain / "a.tsv")
    assert head0 == A.AIRR_COLUMNS + ["expected_count"] and head == A.AIRR_COLUMNS + ["clone_id", "expected_count"]
    ids_of = [f"lin_{k + 1}" if k >= 0 else "" for k in clone.tolist()]
    assert rows == [r_[:-1] + [ids_of[c], r_[-1]] for c, r_ in enumerate(rows0)]
    # --airr without the quant step: clone_id is the last column
    d = _fresh(tmp_path, "airr", tag)
    _vdjer(d, tag, ["--lineages", "l.tsv", "--airr", "a.tsv"], env)
    head, rows = A.read_table(d / "a.tsv")
    assert head == A.AIRR_COLUMNS + ["clone_id"] and rows == [r_[:-1] + [ids_of[c]] for c, r_ in enumerate(rows0)]
    assert (d / "l.tsv").read_text() == table()
    if tag != "e2e_mixed":
        return
    # another threshold, read exactly
    d = _fresh(tmp_path, "dist", tag)
    r = _vdjer(d, tag, ["--lineage-dist", "0.05", "--lineages", "l.tsv"], env)
    m05 = M.lineage(x["junctions"], x["group"], (500, 10000))
    assert (d / "l.tsv").read_text() == table(model=m05[:2]) and _lineages_line(r) == M.summary_line(n, m05[2], (500, 10000))
    # two ranks (on one device): rank 0 writes the same table, without the quant column
    d = _fresh(tmp_path, "two", tag)
    r = _vdjer(d, tag, ["--gpus", "2", "--lineages", "l.tsv"], _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert (d / "l.tsv").read_text() == table() and _lineages_line(r) == M.summary_line(n, info)
