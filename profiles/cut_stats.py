"""What the k-mer build's sampled cut did on the four workloads its margin was measured on (profiles/README.md, sampled cut): the pools of
`bench.py` (default flags; --k 25 --mf 2 --mq 60; --repertoire private; --pairs 1000000), three builds each, and the context's counters
as one JSON line per workload -- kmer_build_cut_sample, kmer_build_cut_retries, kmer_build_sym_walk_retries, gated_instances -- since
bench.py's own line does not carry the cut's counters.  Run from the repository root on the GPU:  python profiles/cut_stats.py"""
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from vdjer_amd import api  # noqa: E402

WORKLOADS = (("configs[2]: 10 M pairs, k = 35", 10_000_000, 35, 3, 90, {}),
             ("configs[3]: 10 M pairs, k = 25", 10_000_000, 25, 2, 60, {}),
             ("--repertoire private, 10 M pairs", 10_000_000, 35, 3, 90, dict(private_v=True, private_j=True, zipf_s=0.25)),
             ("--pairs 1000000", 1_000_000, 35, 3, 90, {}))
SEED = 20261002

for name, pairs, k, mf, mq, rep_kw in WORKLOADS:
    bench.REP_KW.clear()
    bench.REP_KW.update(rep_kw)
    clones = max(4, pairs // (4000 if rep_kw else 500))
    rep, pool, vc, jc, _ = bench.make_workload(pairs, clones, SEED, 0, 1, "cuda:0")
    ctx = api.Context(0)
    ctx.anchor_sets_load(vc, jc)
    p = ctx.pool_load_device(pool.primary.data_ptr(), pool.primary.shape[0], pool.secondary.data_ptr(), pool.secondary.shape[0], pool.rl)
    nodes = [int(ctx.kmer_build(p, k, mf, mq).n) for _ in range(3)]
    out = {"workload": name, "builds": 3, "nodes": nodes}
    out.update({n: int(ctx.stat(n)) for n in ("kmer_build_cut_sample", "kmer_build_cut_retries", "kmer_build_sym", "kmer_build_sym_walk_retries", "gated_instances")})
    print(json.dumps(out), flush=True)
    p.free()
    ctx.close()
    del pool, p, ctx
    gc.collect()
    torch.cuda.empty_cache()
