"""vdjx_tree on the GPU: parent, dist, depth and every info field against the plain model of tests/tree_model.py, exactly -- clone sizes
around k_tree_min's row block and column tiles, window lengths around its 32-base words, the default span, both sides of the register
path's 512 bases and the chunked path up to 4,095, every word count from 1 to 16 and 17 and 33, windows cut at shifts of 1, 31, 32 and 33, a chain of 200, 100 equal sequences, two
families one substitution apart, characters that are not ACGT, 1,000 small clones interleaved, seeded random repertoires, a permutation, a
clone of 4,097 (13 rounds, column slices of two tiles), 2^20 - 1 items in pairs, the dispatch counts, the refusals -- and `vdjer --trees`
on the e2e_families golden against the model's table.  The API cases run in one child process (as tests/test_gpu_lineage.py runs its own);
every model result is computed once."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import families as F
from tests import lineage_model as L
from tests import tree_model as T
from tests.test_gpu_annot import _child_env
from tests.test_gpu_tables import _api_hits, _sha, _vdjer, golden  # noqa: F401  (_api_hits runs in the child)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 63, 64, 65, 129, 200]                                 # row-block and column-tile edges
WINDOWS = [1, 31, 32, 33, 64, 65, 486, 512, 513, 1000, 4095]            # word edges, the default span, the register path's limit, chunks
SHIFTS = [1, 31, 32, 33]
LISTED = 5000                                                           # results of more items than this come back as digests
TABLES = ["--airr", "a.tsv", "--quant", "q.tsv", "--lineages", "l.tsv"]


def _run_child(fn, arg, env, timeout=900):
    code = f"import json; from tests.test_gpu_tree import {fn}; print('TREE', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("TREE ")).split(" ", 1)[1])


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(list(alpha), int(n)))


def _step(s, k):
    """s with position k mod len(s) moved on to the next base"""
    q = k % len(s)
    return s[:q] + "ACGT"[("ACGT".index(s[q]) + 1) % 4] + s[q + 1:]


def _descent(rng, m, length, most=2):
    """m sequences: a founder, and every later one 0 .. `most` substitutions from a random earlier one"""
    out = [_rand(rng, length)]
    while len(out) < m:
        s = out[int(rng.integers(0, len(out)))]
        for q in rng.choice(length, size=min(length, int(rng.integers(0, most + 1))), replace=False).tolist():
            s = _step(s, q)
        out.append(s)
    return out


def _cut(rng, longs, length, at):
    """contigs of `length` cut out of the longer sequences at random offsets -> (contigs, anchors): position `at` of the long sequence is
    every member's anchor, so the anchors differ inside the clone by the offsets"""
    spread = len(longs[0]) - length
    offs = rng.integers(0, spread + 1, len(longs)).tolist()
    return [s[o:o + length] for s, o in zip(longs, offs)], [at - o for o in offs]


# ---- the cases: name -> (contigs, clone, anchor, prio) -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20250)
    out = {}
    for m in SIZES:                                                      # one clone of m contigs of 45 bases, anchors 15 .. 25
        cs, an = _cut(rng, _descent(rng, m, 55), 45, 25)
        out[f"size_{m}"] = (cs, [6] * m, an, None)
    for w in WINDOWS:                                                    # a clone of 21 whose window is w bases
        longs = _descent(rng, 17, w, 3)
        f = longs[0]
        longs += [_step(f, 0), _step(f, w - 1), _step(_step(f, 0), w - 1), f]      # the first and the last window position alone tell these apart
        if w == 4095:                                                    # (the longest contig there is: the anchors are equal)
            out[f"window_{w}"] = (longs, [0] * 21, [w // 2] * 21, None)
            continue
        # contigs of w + 3 bases whose anchors are 3 apart: a = a0, b = w + 3 - (a0 + 3)
        a0 = w // 3
        cs, an = [], []
        for k, s in enumerate(longs):
            if k % 2:
                cs.append(_rand(rng, 3) + s)
                an.append(a0 + 3)
            else:
                cs.append(s + _rand(rng, 3))
                an.append(a0)
        out[f"window_{w}"] = (cs, [0] * 21, an, None)
    for s in SHIFTS:                                                     # windows of 70 bases in contigs of 70 + s, the anchors s apart
        w0 = _rand(rng, 70)
        cs, an = [], []
        for k, win in enumerate([w0, _step(w0, 0), _step(w0, 69), w0, _step(_step(w0, 0), 69)]):
            late = k in (1, 3, 4)
            cs.append(_rand(rng, s) + win if late else win + _rand(rng, s))
            an.append(10 + s if late else 10)
        out[f"shift_{s}"] = (cs, [0] * 5, an, None)
    # a chain of 200 at 60 bases, each one substitution from the previous, shuffled so that index 0 is mid-chain
    chain = [_rand(rng, 60)]
    for k in range(1, 200):
        chain.append(_step(chain[-1], k))
    order = rng.permutation(200).tolist()
    order.remove(100)
    order.insert(0, 100)
    shuffled = [chain[k] for k in order]
    out["chain"] = (shuffled, [3] * 200, [0] * 200, None)
    prio = [7] * 200
    prio[order.index(0)] = 2
    out["chain_from_one_end"] = (shuffled, [3] * 200, [0] * 200, prio)
    out["all_equal_100"] = ([_rand(rng, 45)] * 100, [0] * 100, [20] * 100, None)
    # two families of 40: b is a with one substitution at 45; a's copies vary in 0 .. 19, b's in 20 .. 39, one or two substitutions each
    a = _rand(rng, 60)
    b = _step(a, 45)

    def copies(f, lo):
        res = [f]
        for _ in range(39):
            s = f
            for q in (lo + rng.choice(20, size=int(rng.integers(1, 3)), replace=False)).tolist():
                s = _step(s, q)
            res.append(s)
        return res

    both = copies(a, 0) + copies(b, 20)
    order = rng.permutation(80).tolist()
    out["two_families"] = ([both[k] for k in order], [1] * 80, [30] * 80, None)
    f = _rand(rng, 40)
    other = [f, f[:10] + "N" + f[11:], f[:10] + "N" + f[11:], f.lower(), f[:39] + "*", f[:39] + "*", f[:20] + f[20:].lower(), "N" * 40, "N" * 40,
             f[:5] + "n" + f[6:], f[:31] + "N" + f[32:], f[:32] + "N" + f[33:], f]
    out["not_acgt"] = (other, [0] * len(other), [0] * len(other), None)
    # 1,000 clones of 1 .. 5 members, interleaved, with items that take no part among them; clone keys of any size
    cs, cl, an = [], [], []
    for k in range(1000):
        m = 1 + k % 5
        c1, a1 = _cut(rng, _descent(rng, m, 36), 30, 16)
        cs += c1
        an += a1
        cl += [k * 2000003 % 2147483647] * m
    for _ in range(200):
        cs.append(_rand(rng, 30))
        an.append(int(rng.integers(-5, 40)))                             # (any anchor where the item takes no part)
        cl.append(-1)
    order = rng.permutation(len(cs)).tolist()
    out["small_clones_1000"] = ([cs[k] for k in order], [cl[k] for k in order], [an[k] for k in order], None)
    for seed in range(20):                                               # seeded random repertoires
        r = np.random.default_rng(3000 + seed)
        length = int(r.choice([33, 45, 64, 70, 100, 130]))
        cs, cl, an, pr = [], [], [], []
        for k in range(int(r.integers(2, 12))):
            m = int(r.integers(1, 80))
            extra = int(r.integers(0, min(40, length // 2)))             # the anchors of a clone lie within `extra` of each other
            c1, a1 = _cut(r, _descent(r, m, length + extra, int(r.integers(1, 6))), length, int(r.integers(extra, length + 1)))
            cs += c1
            an += a1
            cl += [k if r.integers(0, 20) else -1 for _ in range(m)]
            pr += r.integers(0, 4, m).tolist()
        order = r.permutation(len(cs)).tolist()
        out[f"random_{seed}"] = ([cs[k] for k in order], [cl[k] for k in order], [an[k] for k in order],
                                 [pr[k] for k in order] if seed % 2 else None)
    # one clone of 4,097 at 40 bases: 13 rounds, and 4097^2 cells make column slices of 128, two tiles of 64
    out["clone_4097"] = (_descent(np.random.default_rng(20251), 4097, 40, 2), [0] * 4097, [11] * 4097, None)
    # every word count k_tree_min has a body for: a clone of 65 (two row blocks; two column tiles of 64, three of 32 from 9 words on) and,
    # laid out after it, a clone of 3; the windows lie at offset 0 or 1 of contigs of w + 1 bases; member 64 has an N in its last word
    rng = np.random.default_rng(20253)
    for words in WORDS:
        w = words_window(words)
        a0 = w // 3
        longs = _descent(rng, 65, w, 3) + _descent(rng, 3, w, 3)
        longs[64] = longs[64][:w - 1] + "N"
        cs = [_rand(rng, 1) + s if k % 3 == 1 else s + _rand(rng, 1) for k, s in enumerate(longs)]
        out[f"words_{words}"] = (cs, [4] * 65 + [9] * 3, [a0 + 1 if k % 3 == 1 else a0 for k in range(68)], None)
    return out


WORDS = list(range(1, 17)) + [17, 33]                                   # the sixteen register bodies; the chunked path with a partial second chunk, with three chunks


def words_window(words):
    """a window of `words` words: one base in the last for an odd count, a full last word for an even one"""
    return 32 * (words - 1) + 1 if words % 2 else 32 * words


def pairs_case():
    """2^20 - 1 items of 6 bases in pairs: item i and item i + 524,287 share a clone, the last item is alone -> (raw bytes, n, 6), clone, anchor"""
    n, half = (1 << 20) - 1, ((1 << 20) - 1) // 2
    rng = np.random.default_rng(20252)
    a = rng.integers(0, 4, (half, 6), dtype=np.uint8)
    b = np.where(rng.random((half, 6)) < 0.3, (a + 1) % 4, a).astype(np.uint8)
    text = np.frombuffer(b"ACGT", np.uint8)[np.concatenate([a, b, np.zeros((1, 6), np.uint8)])]
    clone = np.concatenate([np.arange(half), np.arange(half), [half]]).astype(np.int32)
    return (text.tobytes(), n, 6), clone, np.full(n, 2, np.int32)


@functools.lru_cache(maxsize=None)
def models():
    return {name: T.tree(*c) for name, c in cases().items()}


def _digest(parent, dist, depth):
    return hashlib.sha256(np.asarray(parent, np.int32).tobytes() + np.asarray(dist, np.int32).tobytes() + np.asarray(depth, np.int32).tobytes()).hexdigest()


def _pack(res):
    n = len(res["parent"])
    out = dict(info=res["info"], dtypes=[str(res[k].dtype) for k in ("parent", "dist", "depth")], digest=_digest(res["parent"], res["dist"], res["depth"]))
    if n <= LISTED:
        out.update(parent=res["parent"].tolist(), dist=res["dist"].tolist(), depth=res["depth"].tolist())
    return out


def _same_result(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("parent", "dist", "depth")) and a["info"] == b["info"]


def _dispatch_inputs():
    """same largest clone (8), very different clone counts; and a larger clone"""
    rng = np.random.default_rng(9)
    one = _descent(rng, 8, 45)
    many = [s for _ in range(500) for s in _descent(rng, 8, 45)]
    big = _descent(rng, 200, 45)
    return {"one_clone_of_8": (one, [0] * 8, [5] * 8), "500_clones_of_8": (many, [k // 8 for k in range(4000)], [5] * 4000),
            "one_clone_of_200": (big, [0] * 200, [5] * 200)}


def _device(_):
    import ctypes as C
    from vdjer_amd import _lib, api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    ctx.tree(["ACGT", "ACGA"], [0, 0], [0, 0])                           # (the workspace is there before the kept bytes are read)
    kept0, allocs0 = ctx.stat("kept_device_bytes"), ctx.stat("kept_allocs")
    out = dict(cases={}, perm={}, dispatches={}, work_items={}, rounds={})
    for name, (cs, cl, an, pr) in cases().items():
        res = ctx.tree(cs, cl, an, pr)
        out["work_items"][name], out["rounds"][name] = ctx.stat("tree_work_items"), ctx.stat("tree_rounds")
        assert _same_result(ctx.tree(cs, cl, an, pr), res), name         # two calls give the same bits
        out["cases"][name] = _pack(res)
    packed, clone, anchor = pairs_case()
    res = ctx.tree(packed, clone, anchor)
    out["work_items"]["pairs_2_20_minus_1"], out["rounds"]["pairs_2_20_minus_1"] = ctx.stat("tree_work_items"), ctx.stat("tree_rounds")
    out["cases"]["pairs_2_20_minus_1"] = _pack(res)
    assert ctx.stat("kept_device_bytes") == kept0 and ctx.stat("kept_allocs") == allocs0      # scratch is the workspace's: nothing is kept
    cs, cl, an, pr = cases()["not_acgt"]
    assert _same_result(ctx.tree(api.Context.pack_strings(cs), cl, an), ctx.tree(cs, cl, an))      # (the contigs packed by the caller)
    for name in ("random_3", "random_8", "small_clones_1000"):            # the same input in another order
        cs, cl, an, pr = cases()[name]
        order = np.random.default_rng(5).permutation(len(cs)).tolist()
        out["perm"][name] = dict(order=order, res=_pack(ctx.tree([cs[i] for i in order], [cl[i] for i in order], [an[i] for i in order],
                                                                 None if pr is None else [pr[i] for i in order])))
    for name, args in _dispatch_inputs().items():
        ctx.profile(True)
        ctx.profile_reset()
        ctx.tree(*args)
        out["dispatches"][name] = {k: v[1] for k, v in ctx.profile_get().items()}
        ctx.profile(False)
    # no item; refusals
    r0 = ctx.tree([], [], [])
    assert all(r0[k].shape == (0,) for k in ("parent", "dist", "depth")) and r0["info"] == dict.fromkeys(T.FIELDS, 0)
    good = ["ACGTACGT", "ACGTACGA", "ACGTACGG"]
    for bad_clone in ([0, -2, 0], [-5, 0, 0]):
        with pytest.raises(VdjxError, match="clone"):
            ctx.tree(good, bad_clone, [0, 0, 0])
    for bad_anchor in ([0, -1, 0], [0, 0, 9]):
        with pytest.raises(VdjxError, match="anchor"):
            ctx.tree(good, [0, 0, 0], bad_anchor)
    assert ctx.tree(good, [0, 0, -1], [3, 4, 9])["parent"].tolist() == [-1, 0, -1]             # (any anchor where the item takes no part)
    with pytest.raises(VdjxError, match="empty window"):
        ctx.tree(good, [4, 4, 4], [0, 3, 8])
    assert ctx.tree(good, [4, 5, 4], [0, 8, 7])["info"]["members"] == 3                         # anchors 0 and len in different clones; a window of 1
    with pytest.raises(VdjxError, match="NUL"):
        ctx.tree((b"ACGTAC\0TACGTACGTACGTACGT", 3, 8), [0, 0, 0], [0, 0, 0])
    with pytest.raises(VdjxError, match="characters"):
        ctx.tree((b"A" * 8192, 2, 4096), [0, 0], [0, 0])
    assert ctx.tree((b"A" * 8190, 2, 4095), [0, 0], [0, 0])["info"]["weight"] == 0
    # the raw call: len 0, NULL outputs, 2^20 items, n = 0
    Lb, h = ctx.L, ctx.h
    info = _lib.TreeInfo()
    z3, o3 = np.zeros(3, np.int32), [np.zeros(3, np.int32) for _ in range(3)]
    info.members = 99
    rc = Lb.vdjx_tree(h, b"ACGTACGTACGT", 3, 0, api._p(z3), api._p(z3), None, api._p(o3[0]), api._p(o3[1]), api._p(o3[2]), C.byref(info))
    assert rc == -1 and b"characters" in Lb.vdjx_last_error() and info.members == 0
    for missing in range(3):
        ptrs = [None if k == missing else api._p(o3[k]) for k in range(3)]
        rc = Lb.vdjx_tree(h, b"ACGTACGTACGT", 3, 4, api._p(z3), api._p(z3), None, ptrs[0], ptrs[1], ptrs[2], None)
        assert rc == -1 and b"NULL" in Lb.vdjx_last_error(), missing
    big = 1 << 20
    zb = np.zeros(big, np.int32)
    rc = Lb.vdjx_tree(h, b"A" * big, big, 1, api._p(np.full(big, -1, np.int32)), api._p(zb), None, api._p(zb.copy()), api._p(zb.copy()), api._p(zb.copy()), None)
    assert rc == -1 and b"2^20" in Lb.vdjx_last_error()
    info.weight = 5
    rc = Lb.vdjx_tree(h, None, 0, 0, None, None, None, None, None, None, C.byref(info))       # n = 0 returns at once
    assert rc == 0 and [getattr(info, f) for f in T.FIELDS] == [0] * 6
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def device():
    return _run_child("_device", "x", _child_env("shipped"))


def _same(dev, model, what):
    parent, dist, depth, info = model
    assert dev["dtypes"] == ["int32"] * 3, what
    assert dev["info"] == info, (what, dev["info"], info)
    if "parent" in dev:
        for key, want in (("parent", parent), ("dist", dist), ("depth", depth)):
            a, b = np.asarray(dev[key], np.int64), want.astype(np.int64)
            assert np.array_equal(a, b), (what, key, np.argwhere(a != b)[:5].tolist(), a[:16].tolist(), b[:16].tolist())
    assert dev["digest"] == _digest(parent, dist, depth), what


@pytest.mark.parametrize("m", SIZES)
def test_tree_clone_sizes_around_the_row_block(m):
    name = f"size_{m}"
    _same(device()["cases"][name], models()[name], name)
    cs, cl, an, _ = cases()[name]
    info = models()[name][3]
    assert info["largest_clone"] == m and info["rounds"] == (m - 1).bit_length() == device()["rounds"][name] and (m < 3 or len(set(an)) > 1)
    assert device()["work_items"][name] == (0 if m < 2 else (-(-m // 64)) ** 2)


@pytest.mark.parametrize("w", WINDOWS)
def test_tree_window_lengths(w):
    name = f"window_{w}"
    _same(device()["cases"][name], models()[name], name)
    cs, cl, an, _ = cases()[name]
    members = list(range(21))
    assert sum(T.window_of(members, an, len(cs[0]))) == w
    ws, _ = T.windows(cs, members, an)
    D = T.distance_matrix(ws)
    assert D[0, 20] == 0 and D[0, 17] == 1 and (w == 1 or (D[0, 18] == 1 and D[17, 18] == 2 and D[0, 19] == 2))      # the two ends of the window count


@pytest.mark.parametrize("words", WORDS)
def test_tree_every_word_count(words):
    """every unrolled body of k_tree_min and two shapes of the chunked path, at one base in the last word and at a full one: two row blocks,
    more than one column tile, a second clone whose first row and first word are not 0"""
    name = f"words_{words}"
    _same(device()["cases"][name], models()[name], name)
    cs, cl, an, _ = cases()[name]
    w = words_window(words)
    big, small = list(range(65)), list(range(65, 68))
    assert sum(T.window_of(big, an, len(cs[0]))) == sum(T.window_of(small, an, len(cs[0]))) == w and -(-w // 32) == words and w % 32 == words % 2
    assert all({an[i] - min(an) for i in members} == {0, 1} for members in (big, small))      # windows at offset 0 and at offset 1
    ws, _ = T.windows(cs, big, an)
    assert [i for i, s in enumerate(ws) if "N" in s] == [64] and ws[64].index("N") == w - 1
    D = T.distance_matrix(ws)
    assert D[64, 64] == 1 and D[:64, :64].max() < 32 and (np.bincount(D[np.triu_indices(65, 1)]).max() > 65)      # small distances, many ties
    info = models()[name][3]
    assert info["clones"] == 2 and info["largest_clone"] == 65 and info["rounds"] == 7 == device()["rounds"][name]
    assert device()["work_items"][name] == 2 * 2 + 1


@pytest.mark.parametrize("s", SHIFTS)
def test_tree_windows_cut_at_a_shift(s):
    name = f"shift_{s}"
    _same(device()["cases"][name], models()[name], name)
    cs, cl, an, _ = cases()[name]
    parent, dist, depth, info = models()[name]
    assert max(an) - min(an) == s and sum(T.window_of(range(5), an, 70 + s)) == 70
    # 0 and 3 are equal over the window; 1 differs from them at its first position, 2 at its last, 4 at both
    assert parent.tolist() == [-1, 0, 0, 0, 1] and dist.tolist() == [-1, 1, 1, 0, 1] and info["weight"] == 3


def test_tree_chain_is_the_chain():
    for name in ("chain", "chain_from_one_end"):
        _same(device()["cases"][name], models()[name], name)
    parent, dist, depth, info = models()["chain"]
    assert info["rounds"] == 8 == device()["rounds"]["chain"] and info["weight"] == 199 and depth[0] == 0 and depth.max() == 100
    assert sorted(dist.tolist()) == [-1] + [1] * 199 and np.bincount(parent[parent >= 0]).max() == 2
    parent, dist, depth, info = models()["chain_from_one_end"]
    assert sorted(depth.tolist()) == list(range(200)) and info["weight"] == 199
    dev = device()["cases"]["chain_from_one_end"]
    assert sorted(dev["depth"]) == list(range(200)) and dev["info"]["rounds"] == 8


def test_tree_equal_sequences_make_a_star_at_the_smallest_index():
    _same(device()["cases"]["all_equal_100"], models()["all_equal_100"], "all_equal_100")
    dev = device()["cases"]["all_equal_100"]
    assert dev["parent"] == [-1] + [0] * 99 and dev["dist"] == [-1] + [0] * 99 and dev["info"]["weight"] == 0 and dev["info"]["rounds"] == 7


def test_tree_two_families_are_joined_by_one_edge():
    _same(device()["cases"]["two_families"], models()["two_families"], "two_families")
    cs = cases()["two_families"][0]
    dev = device()["cases"]["two_families"]
    side = [s[45] for s in cs]                                           # (the base that tells the founders apart: no copy changes it)
    crossing = [(i, p) for i, p in enumerate(dev["parent"]) if p >= 0 and side[i] != side[p]]
    assert len(set(side)) == 2 and len(crossing) == 1 and dev["dist"][crossing[0][0]] == 1


def test_tree_characters_that_are_not_acgt():
    _same(device()["cases"]["not_acgt"], models()["not_acgt"], "not_acgt")
    dev = device()["cases"]["not_acgt"]
    assert dev["parent"][12] == 0 and dev["dist"][12] == 0                # the only pair at distance 0: N against N, '*' against '*' never match
    assert dev["dist"][2] == 1 and dev["dist"][8] == 40 and dev["dist"][3] == 40


def test_tree_many_small_clones_interleaved():
    name = "small_clones_1000"
    _same(device()["cases"][name], models()[name], name)
    info = models()[name][3]
    assert info["clones"] == 1000 and info["members"] == 3000 and info["largest_clone"] == 5 and info["rounds"] == 3 and info["edges"] == 2000
    assert device()["work_items"][name] == 800
    assert device()["cases"][name]["depth"].count(-1) == 200


@pytest.mark.parametrize("seed", range(20))
def test_tree_random_repertoires(seed):
    name = f"random_{seed}"
    _same(device()["cases"][name], models()[name], name)


def test_tree_permuted_input():
    for name, p in device()["perm"].items():
        order = p["order"]
        cs, cl, an, pr = cases()[name]
        model = T.tree([cs[i] for i in order], [cl[i] for i in order], [an[i] for i in order], None if pr is None else [pr[i] for i in order])
        _same(p["res"], model, name + " permuted")
        assert p["res"]["info"] == device()["cases"][name]["info"], name   # the weight of a minimum spanning tree does not depend on the order


def test_tree_clone_of_4097():
    name = "clone_4097"
    _same(device()["cases"][name], models()[name], name)
    assert device()["rounds"][name] == 13 and models()[name][3]["edges"] == 4096
    assert device()["work_items"][name] == 65 * 33                       # slices of 128 columns: two tiles each, the last slice one column


def test_tree_pairs_up_to_2_20_minus_1():
    """item i < half and item i + half are a clone: the tree is the one edge, the smaller index the root.  What the definition gives for
    that shape is written down with numpy (the plain model spends ten seconds on half a million clones); the model itself is run on
    the first, the middle and the last 500 pairs and must give the same rows."""
    name = "pairs_2_20_minus_1"
    (raw, n, ln), clone, anchor = pairs_case()
    half = n // 2
    text = np.frombuffer(raw, np.uint8).reshape(n, ln)
    d = (text[:half] != text[half:2 * half]).sum(1).astype(np.int32)     # (every character is ACGT)
    none, zero = np.full(half, -1, np.int32), np.zeros(half, np.int32)
    parent = np.concatenate([none, np.arange(half, dtype=np.int32), [-1]]).astype(np.int32)
    dist = np.concatenate([none, d, [-1]]).astype(np.int32)
    depth = np.concatenate([zero, zero + 1, [0]]).astype(np.int32)
    info = dict(members=n, clones=half + 1, largest_clone=2, rounds=1, edges=half, weight=int(d.sum()))
    for first in (0, half // 2, half - 500):
        idx = list(range(first, first + 500)) + list(range(half + first, half + first + 500))
        mp, md, mdepth, _ = T.tree([bytes(text[i]).decode() for i in idx], clone[idx], anchor[idx])
        assert md.tolist() == dist[idx].tolist() and mdepth.tolist() == depth[idx].tolist() and mp[500:].tolist() == list(range(500)) and (mp[:500] == -1).all()
    _same(device()["cases"][name], (parent, dist, depth, info), name)
    assert info["weight"] > half and device()["work_items"][name] == half and device()["rounds"][name] == 1


def test_tree_dispatches_grow_with_the_rounds_only():
    d = device()["dispatches"]
    # (the first round's k_tree_min, in which no column can be skipped, is timed under a name of its own)
    assert d["one_clone_of_8"] == d["500_clones_of_8"] == {"k_tree_pack": 1, "k_tree_min_first": 1, "k_tree_min": 2, "k_tree_hook": 3, "k_tree_flat": 3}, d
    assert d["one_clone_of_200"] == {"k_tree_pack": 1, "k_tree_min_first": 1, "k_tree_min": 7, "k_tree_hook": 8, "k_tree_flat": 8}, d


# ---- vdjer --trees -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("trees")
    fam = F.build()
    F.write_ref_dir(fam, str(d / "ref"))
    F.write_cfa(fam, str(d / "c.fa"))
    F.pool(fam).write_reads_file(str(d / "reads.txt"))
    return d


def _trees_line(lines):
    at = next(i for i, l in enumerate(lines) if l.startswith("lineages: "))
    assert lines[at + 1].startswith("trees: "), lines[at:at + 3]
    return lines[at + 1]


def test_vdjer_cli_trees_table(inputs):
    from vdjer_amd import annot
    env = _child_env("shipped")
    code = "import json; from tests.test_gpu_tree import _api_hits; print('TREE', json.dumps(_api_hits(0)))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    x = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("TREE ")).split(" ", 1)[1])
    ids, seqs = golden()
    clone = L.lineage(x["junctions"], x["group"])[0]
    v = {k: np.asarray(a) for k, a in x["v"].items()}
    anchor, prio = annot.tree_inputs(ids, seqs, v, clone)
    parent, dist, depth, info = T.tree(seqs, clone, anchor, prio)
    want = T.table_text(T.table_rows(ids, seqs, clone, anchor, prio, parent, dist, depth))
    assert info["largest_clone"] >= 3 and info["edges"] >= 3 and info["weight"] > 0 and (clone < 0).any()      # the golden has trees to speak of

    d, lines = _vdjer(inputs, "trees", TABLES + ["--trees", "t.tsv"], env)
    assert (d / "t.tsv").read_text() == want
    assert _trees_line(lines) == T.summary_line(info)
    plain, lines0 = _vdjer(inputs, "plain", TABLES, env)
    assert not any(l.startswith("trees: ") for l in lines0) and not (plain / "t.tsv").exists()
    for fn in ("a.tsv", "q.tsv", "l.tsv", "out.sam", "vdj_contigs.fa", "vdjer.dot"):
        assert _sha(d / fn) == _sha(plain / fn), fn
    two, lines2 = _vdjer(inputs, "two", ["--gpus", "2", "--airr", "a.tsv", "--lineages", "l.tsv", "--trees", "t.tsv"],
                         _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert any("k-mer table sharded over 2 GPUs" in l for l in lines2)
    assert (two / "t.tsv").read_text() == want and _trees_line(lines2) == T.summary_line(info)
