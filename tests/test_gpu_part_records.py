"""k_part_records_g (vdjx_kmer.hip): the first pass of the k-mer build's cut makes every gated tuple -- key, canonical side, instance,
bucket -- once, in its counting pass, and the rest of the round only moves it.

Every case builds the graph in a fresh process (the knobs are read once) and compares it with the oracle (KmerTable, prune, Graph),
array for array and exactly, the gated count of every node and `gated_instances` with the oracle's count: integers throughout, no
tolerance.  The pools are circles of bases read at every start (tests/part_records_pools.py; tests/test_part_records_pools.py checks
on the CPU that every k-mer is gated at least twice and survives mf = 2, so that a wrong key or instance of any tuple shows)."""
import functools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CASE = r'''
import json, sys
sys.path.insert(0, %r)
import numpy as np
from oracle import oracle
from vdjer_amd import api
from tests import part_records_pools as PP

kind, k = sys.argv[1], int(sys.argv[2])
MF, MQ = 2, 60
pool = PP.make(kind)
vc = np.array([5, 77, 4242], dtype=np.uint32)
jc = np.array([9, 123456], dtype=np.uint32)
t = oracle.KmerTable(pool, k)
pre = t.size()
want_gated = int(t.export()[1].sum())
assert t.prune(MF, MQ) == pre
first, count, _, _ = t.export()
og = oracle.Graph(t, vc, jc)
ctx = api.Context(0)
ctx.anchor_sets_load(vc, jc)
ctx.profile(True)
p = ctx.pool_load(pool.primary, pool.secondary, pool.rl)
g = ctx.kmer_build(p, k, MF, MQ)
out = {n: int(ctx.stat(n)) for n in ("kmer_build_cut_sample", "kmer_build_cut_retries", "kmer_build_sym", "gated_instances")}
out.update(kernels=sorted(ctx.profile_get()), nodes=int(g.n), want_gated=want_gated, records=int(pool.primary.shape[0]))
assert g.pre_nodes == pre, (g.pre_nodes, pre)
assert g.n == og.n == pre, (g.n, og.n, pre)
np.testing.assert_array_equal(g.first_inst, og.first)
np.testing.assert_array_equal(g.freq, og.freq)
np.testing.assert_array_equal(g.has_v, og.has_v)
np.testing.assert_array_equal(g.has_j, og.has_j)
np.testing.assert_array_equal(g.to_deg, og.to_deg)
np.testing.assert_array_equal(g.from_deg, og.from_deg)
np.testing.assert_array_equal(g.to_ids, og.to_ids)
np.testing.assert_array_equal(g.from_ids, og.from_ids)
# the gated count of every node, by k-mer (a node's first sight may be an instance that is not gated, the table's first is a gated one)
o_cnt = {oracle.inst_kmer(pool, int(f), k): int(n) for f, n in zip(first, count)}
kmers = [g.kmer(i) for i in range(g.n)]
assert kmers == [oracle.inst_kmer(pool, int(f), k) for f in og.first]
assert len(o_cnt) == g.n and [o_cnt[s] for s in kmers] == g.gated_count.tolist()
assert out["gated_instances"] == want_gated, out
p.free()
ctx.close()
print("PART_RECORDS_CASE " + json.dumps(out))
'''

_KNOBS = ("VDJX_HIST_SAMPLE", "VDJX_CUT_MARGIN", "VDJX_GATED_BUCKET", "VDJX_REFINE_TUPLES", "VDJX_NO_SYM", "VDJX_SYNC_DEBUG")


@functools.lru_cache(maxsize=None)
def _run(kind, k, env=()):
    """One build in a fresh process with the knobs of `env` (a tuple of pairs) and no other of the cut's knobs; what the case reports."""
    e = {n: v for n, v in os.environ.items() if n not in _KNOBS}
    e.update(dict(env))
    r = subprocess.run([sys.executable, "-c", _CASE % _ROOT, kind, str(k)], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PART_RECORDS_CASE ")]
    assert r.returncode == 0 and lines, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[-1][len("PART_RECORDS_CASE "):])


def _env(**kw):
    return tuple(sorted((n, str(v)) for n, v in kw.items()))


@pytest.mark.parametrize("kind", ["clean", "clean37"])
def test_all_reads_clean_several_rounds_per_workgroup(kind):
    """2,048 couples of 16 gated offsets each are 32,768 tuples for one or two workgroups whose round holds 5,200: several rounds each;
    with 37 couples more the last wave's row is short."""
    r = _run(kind, 35)
    assert r["kmer_build_sym"] == 1 and r["records"] == 2 * (2048 + (37 if kind == "clean37" else 0))
    assert r["gated_instances"] == r["records"] * 16


@pytest.mark.parametrize("sym", [True, False])
def test_a_round_that_does_not_fit_is_retried_twice(sym):
    """The head's 512 clean couples hold 8,192 tuples; the round, sized from the pool's mean, starts at more than 1,024 couples and fits
    only at the second halving (tests/test_part_records_pools.py)."""
    r = _run("dense_head", 35, _env() if sym else _env(VDJX_NO_SYM=1))
    assert r["kmer_build_sym"] == (1 if sym else 0) and r["gated_instances"] == 2 * 512 * 16


@pytest.mark.parametrize("kind", ["forward", "reverse"])
def test_the_canonical_side_on_either_record(kind):
    """The k-mer of the couple's first record is the smaller one at every offset (the tuple names the instance it was cut from), or the
    larger one at every offset (the tuple names the mirror: record 2r + 1, offset rl - k - o); `clean` mixes both within a read."""
    assert _run(kind, 35)["kmer_build_sym"] == 1


@pytest.mark.parametrize("k", [25, 35])
def test_gated_offsets_in_pieces(k):
    """One spoiled base per other read, moving from read to read: a record's gated offsets lie before, behind and on both sides of the
    boundaries of the listing trips (k = 25: 26 offsets, two trips of 16)."""
    assert _run("pieces", k)["kmer_build_sym"] == 1


@pytest.mark.parametrize("k", [25, 47])
def test_other_k(k):
    """k = 25: 26 offsets a record, two listing trips; k = 47: 24-byte tuples (the key's high part has a word of its own), 4 offsets."""
    r = _run("clean", k)
    assert r["kmer_build_sym"] == 1 and r["gated_instances"] == 2 * 2048 * (50 - k + 1)


@pytest.mark.parametrize("kind,k", [("clean", 35), ("clean37", 35), ("pieces", 25), ("forward", 35), ("clean", 47), ("odd", 35)])
def test_the_general_short_form(kind, k):
    """Every record walked for itself: with VDJX_NO_SYM, and unasked on a pool that is not made of couples (an odd record dropped)."""
    r = _run(kind, k, _env() if kind == "odd" else _env(VDJX_NO_SYM=1))
    assert r["kmer_build_sym"] == 0
    if kind == "odd":
        assert r["records"] == 2 * 2048 - 1


def test_long_reads_build_the_same_graph():
    """Reads of 100 bases: the LONG instantiation (instances record << 8 | offset, 66 offsets a record)."""
    r = _run("long", 35)
    assert r["kmer_build_sym"] == 0 and r["gated_instances"] == 2 * 1024 * 66


def test_two_passes_and_the_sampled_layout():
    """VDJX_GATED_BUCKET=16: 2,048 buckets, so the records' pass cuts 256 coarse ones and k_part_tuples the rest;
    VDJX_HIST_SAMPLE=4: the buckets laid out by capacities from a sampled histogram, the passes checking their runs against them."""
    two = _run("clean", 35, _env(VDJX_GATED_BUCKET=16))
    assert "k_part_tuples" in two["kernels"] and two["kmer_build_cut_sample"] == 1, two
    smp = _run("clean", 35, _env(VDJX_GATED_BUCKET=16, VDJX_HIST_SAMPLE=4))
    assert smp["kmer_build_cut_sample"] == 4 and "k_part_tuples" in smp["kernels"], smp
