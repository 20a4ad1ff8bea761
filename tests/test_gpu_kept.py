"""What a context keeps from call to call (vdjx_kept, vdjer_amd/csrc/vdjx_common.h) seen through vdjx_stat's "kept_device_bytes",
"kept_pinned_bytes" and "kept_allocs": nothing on a fresh context, no allocation when a call sequence is repeated or shrinks, the
V region's margin of a quarter, vdjx_trim and vdjx_read_index_drop releasing what they name (and the calls after them giving the
same results from new buffers), the index arrays growing on the read-index thread, and an orderly close.  The pool is small
(2,000 pairs of 50 bases, k = 35, two dozen windows and contigs).  All cases run in one child process with a timeout, as
tests/test_gpu_scan.py does: the child prints the figures, the tests below assert on them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("kept_device_bytes", "kept_pinned_bytes", "kept_allocs")
N_PAIRS, RL, K, VK = 2000, 50, 35, 15


def _first_pairs(pool, n_pairs):
    """the pairs 0 .. n_pairs - 1 of a synth.ReadPool as a pool of their own"""
    from vdjer_amd import synth
    npri = pool.primary.shape[0]
    keep = pool.pair_id < n_pairs
    return synth.ReadPool(pool.rl, pool.primary[keep[:npri]], pool.secondary[keep[npri:]], pool.pair_id[keep], pool.read_num[keep],
                          pool.is_rc[keep], pool.reg_rank[keep], n_pairs)


def _child():
    from vdjer_amd import api, synth
    from vdjer_amd._lib import VdjxError
    rep = synth.make_repertoire(24, seed=911)
    vc = np.array(sorted({synth.seq_to_int(a) for a in rep.v_anchors}), dtype=np.uint32)
    jc = np.array(sorted({synth.seq_to_int(a) for a in rep.j_anchors}), dtype=np.uint32)
    whole = synth.make_reads(rep, N_PAIRS, noise_frac=0.25, rl=RL, seed=912)
    half = _first_pairs(whole, N_PAIRS // 2)
    wins = [w for w in rep.windows() if w]
    res = {"n_windows": len(wins)}
    ctx = api.Context(0)
    stats = lambda: {s: ctx.stat(s) for s in STATS}
    res["fresh"] = stats()
    live = []                                                   # the pool the index was built from

    def scorers(w):
        """the scorer and SAM calls of S -> their outputs as bytes"""
        contigs = [x[51:411] for x in w]
        valid, npairs = ctx.window_score(w, 175)
        offs, pairs = ctx.map_emit(contigs)                      # (both calls: count, then write)
        text = ctx.sam_text_device(contigs, [f"c{i}" for i in range(len(contigs))])
        return [valid.tobytes(), npairs.tobytes(), offs.tobytes(), pairs.tobytes(), bytes(text)]

    def run_s(pool, w):
        while live:
            live.pop().free()
        ctx.anchor_sets_load(vc, jc)
        ctx.vregion_load([rep.v_region], VK)
        p = ctx.pool_load(pool.primary, pool.secondary, pool.rl)
        live.append(p)
        g = ctx.kmer_build(p, K, 3, 90)
        ctx.read_index_build(p, pool.pair_id, pool.read_num, pool.is_rc, pool.reg_rank, pool.n_pairs)
        ctx.sam_names_load(pool.names())
        return [g.first_inst.tobytes(), g.freq.tobytes(), g.to_ids.tobytes(), g.from_ids.tobytes()] + scorers(w)

    # grow-only
    out1 = run_s(whole, wins)
    st1 = stats()
    res["mapped_pairs"] = len(out1[7]) // api.PAIR_DTYPE.itemsize
    res["sam_bytes"] = len(out1[8])
    out2 = run_s(whole, wins)
    res["grow"] = {"first": st1, "again": stats(), "again_equal": out2 == out1}
    out_half = run_s(half, wins[:len(wins) // 2])
    res["grow"]["half"] = stats()
    res["grow"]["half_mapped_pairs"] = len(out_half[7]) // api.PAIR_DTYPE.itemsize

    # the V region's margin: a quarter (+ 64 bytes) over what a load needs.  One line of L bases has L - VK seeds, all distinct
    # (a seed is its code AND its position)
    rng = np.random.default_rng(913)
    line = lambda n: "".join(rng.choice(list("ACGT"), n))
    L0 = len(rep.v_region)
    ctx.vregion_load([line(L0 * 12 // 10)], VK)
    m12 = stats()
    ctx.vregion_load([line(2 * L0)], VK)
    res["margin"] = {"before": res["grow"]["half"], "x1.2": m12, "x2": stats()}

    # trim and drop, with the whole pool's index in hand again
    res["again_after_margin_equal"] = run_s(whole, wins) == out1
    before = stats()
    ctx.trim()
    trimmed = stats()
    after_trim = scorers(wins)
    res["trim"] = {"before": before, "trimmed": trimmed, "after_calls": stats(), "equal": after_trim == out1[4:]}
    ctx.read_index_drop()
    res["drop"] = {"before": res["trim"]["after_calls"], "dropped": stats()}
    try:
        ctx.window_score(wins, 175)
        res["drop"]["error"] = None
    except VdjxError as e:
        res["drop"]["error"] = str(e)
    ctx.read_index_build(live[0], whole.pair_id, whole.read_num, whole.is_rc, whole.reg_rank, whole.n_pairs)
    res["drop"]["rebuilt_equal"] = scorers(wins) == out1[4:]

    # the index arrays grow on the read-index thread: from nothing for the half pool, then past their margin for the whole one
    ctx.read_index_drop()
    res["thread"] = {"before": stats()}
    for name, pool, w, want in (("half", half, wins[:len(wins) // 2], out_half), ("whole", whole, wins, out1)):
        while live:
            live.pop().free()
        p = ctx.pool_load(pool.primary, pool.secondary, pool.rl)
        live.append(p)
        ctx.read_index_build_begin(p, pool.pair_id, pool.read_num, pool.is_rc, pool.reg_rank, pool.n_pairs)
        g = ctx.kmer_build(p, K, 3, 90)                          # <- beside the index
        ctx.read_index_wait()
        waited = stats()                                         # (before the scorers: only the index can have grown)
        ctx.sam_names_load(pool.names())
        got = [g.first_inst.tobytes(), g.freq.tobytes(), g.to_ids.tobytes(), g.from_ids.tobytes()] + scorers(w)
        res["thread"][name] = {"waited": waited, "stats": stats(), "equal": got == want}
    ctx.close()
    res["closed"] = True
    print("KEPT", json.dumps(res))


@pytest.fixture(scope="module")
def r():
    out = subprocess.run([sys.executable, "-c", "from tests.test_gpu_kept import _child; _child()"], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    return json.loads(next(l for l in out.stdout.splitlines() if l.startswith("KEPT ")).split(" ", 1)[1])


def test_workload_is_not_empty(r):
    assert r["n_windows"] >= 20 and r["mapped_pairs"] > 0 and r["sam_bytes"] > 0 and r["grow"]["half_mapped_pairs"] > 0, r


def test_fresh_context_keeps_no_device_memory(r):
    assert r["fresh"]["kept_device_bytes"] == 0, r["fresh"]
    assert r["fresh"]["kept_pinned_bytes"] == 16384 and r["fresh"]["kept_allocs"] == 1, r["fresh"]      # (the 16 KB read-back scratch)


def test_repeated_and_smaller_sequences_allocate_nothing(r):
    g = r["grow"]
    assert g["first"]["kept_device_bytes"] > 0 and g["first"]["kept_allocs"] > 20, g
    assert g["again"] == g["first"] and g["again_equal"], g
    assert g["half"] == g["first"], g


def test_vregion_margin_is_a_quarter(r):
    m = r["margin"]
    assert m["x1.2"] == m["before"], m
    assert m["x2"]["kept_allocs"] > m["before"]["kept_allocs"] and m["x2"]["kept_device_bytes"] > m["before"]["kept_device_bytes"], m


def test_trim_releases_the_result_buffers(r):
    t = r["trim"]
    assert t["trimmed"]["kept_device_bytes"] < t["before"]["kept_device_bytes"], t
    assert t["trimmed"]["kept_allocs"] == t["before"]["kept_allocs"], t
    assert r["again_after_margin_equal"] and t["equal"] and t["after_calls"]["kept_allocs"] > t["before"]["kept_allocs"], t


def test_read_index_drop_releases_the_index(r):
    d = r["drop"]
    assert d["dropped"]["kept_device_bytes"] < d["before"]["kept_device_bytes"], d
    assert d["error"] and "call vdjx_read_index_build first" in d["error"], d
    assert d["rebuilt_equal"], d


def test_index_arrays_grow_on_the_index_thread(r):
    t = r["thread"]
    assert t["half"]["equal"] and t["whole"]["equal"], t
    assert t["before"]["kept_allocs"] < t["half"]["waited"]["kept_allocs"], t
    assert t["half"]["stats"]["kept_allocs"] < t["whole"]["waited"]["kept_allocs"], t
    assert t["half"]["stats"]["kept_device_bytes"] < t["whole"]["waited"]["kept_device_bytes"], t


def test_close_returns(r):
    assert r["closed"]
