"""vdjx_quant_boot at size: the placements profiles/quant_at_size.py uses (the --repertoire private 10 M-pair workload, cfg2_pv,
through `vdjer`, then vdjx_map_emit over its contigs), bootstrapped with 100 replicates through vdjx_quant_pairs_boot.  Records the EM
kernels' time (HIP events around the batches' launches, and the host clock around the same loop), the iterations per replicate, the
modelled bytes one iteration of a batch moves against the HBM peak, and what a user could do without the feature: 100 separate
vdjx_quant_pairs calls, each forced to its replicate's iteration count with tol = 0 (the point estimate's kernels, unchanged from the
parent commit), their EM times added.  The condition "the batched EM takes no longer than those calls" is written out with both times.
   python profiles/quant_boot_at_size.py [out.json] [case]"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import midscale_util as M  # noqa: E402

HBM_PEAK = 8.0e12          # MI355X HBM3E, spec
QB_CHUNK = 512             # vdjx_quant.hip: alignments per workgroup of the bootstrap's M step
B = 100
MAX_ITER = 2000


def boot_bytes_per_iteration(alignments: int, pairs: int, contigs: int, chunks: int, reps: int) -> int:
    """shared by the batch, read once per iteration: E per alignment its contig (4) and g (8), per pair its CSR start (4); M per
    alignment its pair's slot (4) and g (8).  Per replicate: E writes a sum per pair (8); M gathers per alignment its pair's sum (8)
    and multiplicity (4), writes and reads a partial per chunk (16), per contig N old and new (16).  The gathers of N_c are not counted
    (a few thousand contigs: cached)."""
    return 24 * alignments + 4 * pairs + reps * (8 * pairs + 12 * alignments + 16 * chunks + 16 * contigs)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    name = sys.argv[2] if len(sys.argv) > 2 else "cfg2_pv"
    case = M.cases()[name]
    from vdjer_amd import api
    out = {"what": "profiles/quant_boot_at_size.py, as printed", "where": "one MI355X", "case": name, "pairs_in_pool": case["pairs"], "replicates": B}
    with tempfile.TemporaryDirectory() as td:
        rep, pool = M.gen.write_inputs(case, td)
        exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
        r = subprocess.run([exe] + M.gen.argv_of(case, threads=16), cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, errors="replace")
        if r.returncode:
            out.update(cli_exit=r.returncode, stderr_tail=r.stderr[-1500:])
            print(json.dumps(out))
            return 1
        fa = open(os.path.join(td, "vdj_contigs.fa")).read().splitlines()
        seqs = [fa[i + 1] for i in range(0, len(fa), 2)]
    ctx = api.Context(0)
    p = ctx.pool_load(pool.primary, pool.secondary, pool.rl)
    ctx.read_index_build(p, pool.pair_id, pool.read_num, pool.is_rc, pool.reg_rank, pool.n_pairs)
    packed = ctx.pack_strings(seqs)
    offs, pairs = ctx.map_emit(packed)
    offs, pairs = offs.copy(), pairs.copy()
    L, n, P = len(seqs[0]), len(seqs), int(pool.n_pairs)
    args = (offs, pairs, L, P)
    ctx.quant_pairs_boot(*args, replicates=B, max_iter=MAX_ITER)       # (warm-up: code objects, workspace)
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = ctx.quant_pairs_boot(*args, replicates=B, max_iter=MAX_ITER)
        runs.append((ctx.stat("quant_boot_em_us"), ctx.stat("quant_boot_us"), time.perf_counter() - t0))
    ctx.profile(True)
    ctx.profile_reset()
    ctx.quant_pairs_boot(*args, replicates=B, max_iter=MAX_ITER)
    prof = ctx.profile_get()
    ctx.profile(False)
    iters = res["iterations"].astype(int).tolist()
    info, binfo = res["info"], res["boot_info"]
    per = [int(offs[i + 1] - offs[i]) for i in range(n)]
    chunks = sum((x + QB_CHUNK - 1) // QB_CHUNK for x in per)
    reps_per_batch = -(-B // binfo["batches"])
    bpi = boot_bytes_per_iteration(info["alignments"], info["pairs"], n, chunks, reps_per_batch)
    em_s = min(x[0] for x in runs) / 1e6
    batch_iterations = binfo["max_iterations"] if binfo["batches"] == 1 else None
    # what a user could already do: one vdjx_quant_pairs call per replicate, forced to the replicate's iteration count
    ctx.quant_pairs(*args, max_iter=2, tol=0)                           # (warm-up)
    sep = []
    for _ in range(2):
        us = 0
        for it in iters:
            ctx.quant_pairs(*args, max_iter=max(1, it), tol=0)
            us += ctx.stat("quant_em_us")
        sep.append(us)
    sep_s = min(sep) / 1e6
    out.update(contigs=n, placed_pairs=info["pairs"], alignments=info["alignments"], multi_placed_pairs=info["pairs"] - info["unique_pairs"],
               point_iterations=info["iterations"], boot_info=binfo, iterations_per_replicate=dict(min=min(iters), max=max(iters), mean=round(sum(iters) / B, 2)),
               boot_em_ms=round(em_s * 1e3, 3), boot_em_ms_all_runs=[round(x[0] / 1e3, 3) for x in runs], boot_call_ms=round(min(x[1] for x in runs) / 1e3, 3),
               boot_wall_ms=round(min(x[2] for x in runs) * 1e3, 3), kernel_ms={k: round(v[0], 4) for k, v in prof.items() if k.startswith("k_quant")},
               dispatch_scopes={k: v[1] for k, v in prof.items() if k.startswith("k_quant")}, replicates_per_batch=reps_per_batch,
               bytes_per_iteration_of_a_batch=bpi,
               hbm_fraction=round(bpi * batch_iterations / em_s / HBM_PEAK, 4) if batch_iterations and em_s > 0 else None,
               separate_calls_em_ms=round(sep_s * 1e3, 3), separate_calls_em_ms_all_runs=[round(x / 1e3, 3) for x in sep],
               condition="batched EM time <= EM time of B separate vdjx_quant_pairs calls at the same iteration counts",
               ratio_batched_over_separate=round(em_s / sep_s, 4) if sep_s > 0 else None, condition_holds=bool(em_s <= sep_s),
               mean_sd=round(float(np.mean(res["sd"])), 3))
    p.free()
    ctx.close()
    print(json.dumps(out))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
