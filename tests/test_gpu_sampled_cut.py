"""The k-mer build's cut from a SAMPLED histogram (vdjx_kmer.hip: stage_gated_hist S > 1, the layout by capacities, the cursors as bucket
ends, the checked fallback to the exact cut).

Every case builds the graph in a fresh process (the knobs are read once), compares it with the oracle (KmerTable, prune, Graph: as the
parity tests do) and says through the context's stats which path ran: `kmer_build_cut_sample` is the row stride the build began with,
`kmer_build_cut_retries` counts the builds that ran over a bucket's capacity and cut again exactly.  The pools are a few tens of
thousands of pairs; VDJX_GATED_BUCKET shrinks the buckets until the cut takes the passes a 10 M-pair pool takes."""
import functools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CASE = r'''
import hashlib, json, sys, types
sys.path.insert(0, %r)
import numpy as np
from oracle import oracle
from vdjer_amd import api, synth

pool_kind, k, mf, mq = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
SEED = 20261002
S_ROWS = 4                     # the stride the sampled cases set (VDJX_HIST_SAMPLE): rows 2, 6, 10, ... of 64 couples = 32 pairs each

def pairs_of(pool):            # [pairs, 4, record]: a pair's four records (R1, rc R1, R2, rc R2) travel together, so couples stay couples
    assert pool.secondary.shape[0] == 0
    return pool.primary.reshape(-1, 4, pool.primary.shape[1])

if pool_kind == "zipf":        # 300 clones, Zipf 1.1, 30 %% noise pairs
    rep = synth.make_repertoire(300, seed=SEED)
    pool = synth.make_reads(rep, 60000, noise_frac=0.3, seed=SEED + 7919)
elif pool_kind == "deep":      # one clone holds nearly every read: its k-mers' buckets are hundreds of tuples deep
    rep = synth.make_repertoire(3, seed=SEED, zipf_s=4.0)
    pool = synth.make_reads(rep, 60000, noise_frac=0.1, seed=SEED + 7919)
elif pool_kind == "hidden":    # a deep clone whose reads lie only in rows the sample skips; everything the sample sees is another repertoire
    rep = synth.make_repertoire(200, seed=SEED)
    seen = pairs_of(synth.make_reads(rep, 10016, noise_frac=0.0, seed=SEED + 1))
    deep = pairs_of(synth.make_reads(synth.make_repertoire(1, seed=SEED + 5), 30048, noise_frac=0.0, seed=SEED + 2))
    rows, si, di = [], 0, 0
    for row in range(10**9):
        if row %% S_ROWS == S_ROWS // 2:
            if si + 32 > seen.shape[0]: break
            rows.append(seen[si:si + 32]); si += 32
        else:
            if di + 32 > deep.shape[0]: break
            rows.append(deep[di:di + 32]); di += 32
    assert di > 25000 and si > 8000
    pri = np.ascontiguousarray(np.concatenate(rows).reshape(-1, seen.shape[2]))
    pool = types.SimpleNamespace(primary=pri, secondary=np.zeros((0, pri.shape[1]), np.uint8), rl=50)
elif pool_kind == "ragged":    # 64 * S * m + 37 couples: the last sampled row is short and the sampled rows are no multiple of a workgroup's share
    rep = synth.make_repertoire(100, seed=SEED)
    full = synth.make_reads(rep, 7000, noise_frac=0.0, seed=SEED + 3)
    couples = 64 * S_ROWS * 50 + 37
    assert full.primary.shape[0] >= 2 * couples
    pri = np.ascontiguousarray(full.primary[:2 * couples])
    pool = types.SimpleNamespace(primary=pri, secondary=np.zeros((0, pri.shape[1]), np.uint8), rl=50)
else:
    raise SystemExit("unknown pool " + pool_kind)

vc = np.array(sorted({synth.seq_to_int(a) for a in rep.v_anchors}), dtype=np.uint32)
jc = np.array(sorted({synth.seq_to_int(a) for a in rep.j_anchors}), dtype=np.uint32)
ctx = api.Context(0)
ctx.anchor_sets_load(vc, jc)
ctx.profile(True)
p = ctx.pool_load(pool.primary, pool.secondary, pool.rl)
g = ctx.kmer_build(p, k, mf, mq)
kernels = sorted(ctx.profile_get())
out = {n: int(ctx.stat(n)) for n in ("kmer_build_cut_sample", "kmer_build_cut_retries", "kmer_build_sym", "kmer_build_sym_walk_retries", "gated_instances")}
g2 = ctx.kmer_build(p, k, mf, mq)                      # again: the same graph, and the retry count moves the same way
out["retries_after_two_builds"] = int(ctx.stat("kmer_build_cut_retries"))
t = oracle.KmerTable(pool, k)
assert g.pre_nodes == t.size(), (g.pre_nodes, t.size())
t.prune(mf, mq)
og = oracle.Graph(t, vc, jc)
assert g.n == og.n and g.n > 0, (g.n, og.n)
np.testing.assert_array_equal(g.first_inst, og.first)
np.testing.assert_array_equal(g.freq, og.freq)
np.testing.assert_array_equal(g.has_v, og.has_v)
np.testing.assert_array_equal(g.has_j, og.has_j)
np.testing.assert_array_equal(g.to_ids, og.to_ids)
np.testing.assert_array_equal(g.from_ids, og.from_ids)
h = hashlib.sha1()
for f in ("first_inst", "freq", "gated_count", "to_ids", "from_ids", "kmers"):
    np.testing.assert_array_equal(getattr(g, f), getattr(g2, f))
    h.update(np.ascontiguousarray(getattr(g, f)).tobytes())
out.update(digest=h.hexdigest(), nodes=int(g.n), pre_nodes=int(g.pre_nodes), kernels=kernels, records=int(pool.primary.shape[0]))
p.free()
ctx.close()
print("SAMPLED_CUT_CASE " + json.dumps(out))
'''

_KNOBS = ("VDJX_HIST_SAMPLE", "VDJX_CUT_MARGIN", "VDJX_GATED_BUCKET", "VDJX_REFINE_TUPLES", "VDJX_NO_SYM", "VDJX_SYNC_DEBUG")


@functools.lru_cache(maxsize=None)
def _run(pool_kind, k, mf, mq, env):
    """One build in a fresh process with the knobs of `env` (a tuple of pairs) and no other of the cut's knobs; what the case reports."""
    e = {n: v for n, v in os.environ.items() if n not in _KNOBS}
    e.update(dict(env))
    r = subprocess.run([sys.executable, "-c", _CASE % _ROOT, pool_kind, str(k), str(mf), str(mq)], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SAMPLED_CUT_CASE ")]
    assert r.returncode == 0 and lines, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[-1][len("SAMPLED_CUT_CASE "):])


def _env(**kw):
    return tuple(sorted((n, str(v)) for n, v in kw.items()))


_TWO_PASS = dict(VDJX_GATED_BUCKET=16)                              # T = 14 or 15 at 60 k pairs: 256 coarse buckets, then the fine ones
_EXTRA = dict(VDJX_GATED_BUCKET=4, VDJX_REFINE_TUPLES=4)            # more than 2^15 buckets (test_large_pool_code_paths_on_a_small_pool)


@pytest.mark.parametrize("sym", [True, False])
def test_sampled_cut_two_passes(sym):
    """Both passes write into the layout by capacities and the reduce kernel reads the buckets up to the second pass's cursors; SYM
    (k odd, the pool in couples) and, with VDJX_NO_SYM, the form that walks every record."""
    extra = {} if sym else {"VDJX_NO_SYM": 1}
    r = _run("zipf", 35, 3, 90, _env(VDJX_HIST_SAMPLE=4, **_TWO_PASS, **extra))
    assert r["kmer_build_cut_sample"] == 4 and r["kmer_build_sym"] == (1 if sym else 0)
    assert r["kmer_build_cut_retries"] == 0 and r["retries_after_two_builds"] == 0 and r["kmer_build_sym_walk_retries"] == 0
    assert "k_part_tuples" in r["kernels"] and "k_seg_hist" not in r["kernels"], r["kernels"]
    assert r["gated_instances"] // (2 if sym else 1) > 16 << 10, r            # more than 2^10 buckets of 16: the two passes


def test_sampled_cut_beyond_the_histograms_buckets():
    """extra > 0: only the coarse cut is sized from the sample, k_seg_hist counts the fine buckets from the first pass's output (read up
    to its cursors) and the second pass writes dense."""
    r = _run("zipf", 35, 3, 90, _env(VDJX_HIST_SAMPLE=4, **_EXTRA))
    assert r["kmer_build_cut_sample"] == 4 and r["kmer_build_cut_retries"] == 0 and r["retries_after_two_builds"] == 0
    assert "k_seg_hist" in r["kernels"] and "k_part_tuples" in r["kernels"], r["kernels"]
    exact = _run("zipf", 35, 3, 90, _env(VDJX_HIST_SAMPLE=1, **_EXTRA))
    assert exact["kmer_build_cut_sample"] == 1 and "k_seg_hist" in exact["kernels"]
    assert (r["digest"], r["gated_instances"]) == (exact["digest"], exact["gated_instances"])


def test_a_bucket_over_its_capacity_falls_back_to_the_exact_cut():
    """No margin (VDJX_CUT_MARGIN=0 leaves S * h and the floor of 264) and one row in 64 on a pool whose one deep clone fills buckets ~500
    tuples deep: S * h is 64 * (8 +- 3) there, so some of the hundreds of them get less than they hold by more than the floor.  They run
    over, no pass writes past a limit, the reduce stage's read-back says so and the build cuts again exactly -- the oracle's graph and the
    graph of the build that never sampled."""
    r = _run("deep", 35, 3, 90, _env(VDJX_HIST_SAMPLE=64, VDJX_CUT_MARGIN=0, **_TWO_PASS))
    assert r["kmer_build_cut_sample"] == 64
    assert r["kmer_build_cut_retries"] >= 1 and r["retries_after_two_builds"] == 2 * r["kmer_build_cut_retries"], r
    exact = _run("deep", 35, 3, 90, _env(VDJX_HIST_SAMPLE=1, **_TWO_PASS))
    assert exact["kmer_build_cut_sample"] == 1 and exact["kmer_build_cut_retries"] == 0
    assert (r["digest"], r["nodes"], r["gated_instances"]) == (exact["digest"], exact["nodes"], exact["gated_instances"])
    # with the shipped margin the same pool fits
    fit = _run("deep", 35, 3, 90, _env(VDJX_HIST_SAMPLE=4, **_TWO_PASS))
    assert fit["kmer_build_cut_retries"] == 0 and fit["digest"] == exact["digest"]


def test_a_clone_the_sample_never_sees():
    """The deep clone's reads lie in the rows between the sampled ones: its buckets get the margin's floor and no more.  The floor or the
    fallback carries them; the graph is the oracle's and the exact build's either way."""
    r = _run("hidden", 35, 3, 90, _env(VDJX_HIST_SAMPLE=4, **_TWO_PASS))
    assert r["kmer_build_cut_sample"] == 4 and r["kmer_build_cut_retries"] in (0, 1)
    exact = _run("hidden", 35, 3, 90, _env(VDJX_HIST_SAMPLE=1, **_TWO_PASS))
    assert exact["kmer_build_cut_retries"] == 0
    assert (r["digest"], r["gated_instances"]) == (exact["digest"], exact["gated_instances"])


def test_stride_one_is_the_exact_cut_and_counts_the_same_instances():
    """VDJX_HIST_SAMPLE=1: the exact histogram's path; gated_instances -- exact on both paths, on the sampled one from the cursors -- and
    the graph agree with the sampled build of the same pool."""
    exact = _run("zipf", 35, 3, 90, _env(VDJX_HIST_SAMPLE=1, **_TWO_PASS))
    assert exact["kmer_build_cut_sample"] == 1 and exact["kmer_build_cut_retries"] == 0
    sampled = _run("zipf", 35, 3, 90, _env(VDJX_HIST_SAMPLE=4, **_TWO_PASS))
    assert sampled["kmer_build_cut_sample"] == 4
    assert exact["gated_instances"] == sampled["gated_instances"] > 0
    assert exact["digest"] == sampled["digest"]
    # a small pool with no knob set: below the size from which the sample is taken unasked
    dflt = _run("zipf", 35, 3, 90, _env(**_TWO_PASS))
    assert dflt["kmer_build_cut_sample"] == 1 and dflt["digest"] == exact["digest"]


@pytest.mark.parametrize("k,mf,mq", [(35, 3, 90), (24, 2, 60)])
def test_sampled_rows_that_do_not_fill_the_workgroups_shares(k, mf, mq):
    """64 * S * m + 37 couples (k = 24: as many records): a short last row, and sampled rows that are no multiple of a workgroup's share."""
    r = _run("ragged", k, mf, mq, _env(VDJX_HIST_SAMPLE=4, VDJX_GATED_BUCKET=2))
    assert r["records"] == 2 * (64 * 4 * 50 + 37)
    assert r["kmer_build_cut_sample"] == 4 and r["kmer_build_sym"] == (k & 1)
    assert r["kmer_build_cut_retries"] == 0 and r["retries_after_two_builds"] == 0
    assert "k_part_tuples" in r["kernels"], r["kernels"]
