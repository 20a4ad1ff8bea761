"""vdjx_tree at size: one JSON line per leg with the info, the best-of-three wall time of the call after a warm-up, the kernels'
own time (HIP events, one more call), the dispatches, and k_tree_min's time per round: the first round, in which every pair is compared,
and the mean of the later ones, which skip the columns of a lane's own component.
   python profiles/tree_at_size.py
     small_lineages     20,000 lineages of 1 .. 8 contigs of 486 bases, interleaved: the shape of a repertoire
     one_lineage        one lineage of 65,536 contigs of 486 bases (16 words a row, 16 rounds): the rate when the device is full
     lineage_baseline   vdjx_lineage on ONE bucket of the same 65,536 members, the 48 bases from the anchor on (2 words a row): one
                        k_lin_pairs pass, the kernel k_tree_min is measured against.  Nearly every pair of these is within the threshold,
                        so the pass spends its time uniting; lineage_baseline_unlinked is the same bucket of 65,536 random junctions, of
                        which no two are linked: the pass's distance work alone
With `cli <golden>`: the wall time of `vdjer --quant --airr --lineages` with and without `--trees`, best of three each.
   python profiles/tree_at_size.py cli e2e_mixed"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ["k_tree_pack", "k_tree_min_first", "k_tree_min", "k_tree_hook", "k_tree_flat"]
ACGT = np.frombuffer(b"ACGT", np.uint8)


def descent(rng, m, length, rate):
    """m sequences as codes 0 .. 3: a founder, every later one a copy of a random earlier one with each base changed at `rate`"""
    out = np.empty((m, length), np.uint8)
    out[0] = rng.integers(0, 4, length)
    src = (rng.random(m) * np.arange(m)).astype(np.int64)               # (an earlier row each)
    hit = rng.random((m, length)) < rate
    add = rng.integers(1, 4, (m, length), dtype=np.uint8)
    for i in range(1, m):
        out[i] = np.where(hit[i], (out[src[i]] + add[i]) % 4, out[src[i]])
    return out


def leg(ctx, name, packed, clone, anchor):
    ctx.tree((packed[0][:64 * packed[2]], 64, packed[2]), clone[:64], anchor[:64])      # (warm-up: code objects, workspace)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        res = ctx.tree(packed, clone, anchor)
        wall = time.perf_counter() - t0
        cur = (ctx.stat("tree_us"), wall)
        best = cur if best is None or cur[0] < best[0] else best
    ctx.profile(True)
    ctx.profile_reset()
    ctx.tree(packed, clone, anchor)
    prof = ctx.profile_get()
    ctx.profile(False)
    info = res["info"]
    later = prof.get("k_tree_min", (0.0, 0))
    out = dict(leg=name, n=packed[1], len=packed[2], **info, work_items=ctx.stat("tree_work_items"), call_ms=round(best[0] / 1e3, 3), wall_ms=round(best[1] * 1e3, 3),
               kernels_ms=round(sum(prof.get(k, (0.0, 0))[0] for k in KERNELS), 3), kernel_ms={k: round(prof.get(k, (0.0, 0))[0], 4) for k in KERNELS},
               dispatches={k: v[1] for k, v in prof.items()}, min_first_round_ms=round(prof.get("k_tree_min_first", (0.0, 0))[0], 4),
               min_later_round_mean_ms=round(later[0] / max(later[1], 1), 4))
    print(json.dumps(out), flush=True)
    return out


def at_size():
    from vdjer_amd import api
    ctx = api.Context(0)
    rng = np.random.default_rng(486)
    L = 486
    sizes = 1 + np.arange(20000) % 8
    rows = np.concatenate([descent(rng, int(m), L, 0.01) for m in sizes])
    clone = np.repeat(np.arange(20000), sizes).astype(np.int32)
    order = rng.permutation(len(rows))
    leg(ctx, "small_lineages", (ACGT[rows[order]].tobytes(), len(rows), L), clone[order], np.full(len(rows), 300, np.int32))
    m = 65536
    rows = descent(rng, m, L, 0.004)[rng.permutation(m)]
    tree = leg(ctx, "one_lineage", (ACGT[rows].tobytes(), m, L), np.zeros(m, np.int32), np.full(m, 300, np.int32))
    group = np.zeros(m, np.uint32)
    for name, codes in (("lineage_baseline", rows[:, 300:348]), ("lineage_baseline_unlinked", rng.integers(0, 4, (m, 48), dtype=np.uint8))):
        junctions = [bytes(r) for r in ACGT[codes]]
        ctx.lineage(junctions[:64], group[:64])
        ctx.lineage(junctions, group)
        ctx.profile(True)
        ctx.profile_reset()
        res = ctx.lineage(junctions, group)
        prof = ctx.profile_get()
        ctx.profile(False)
        pairs_ms = prof["k_lin_pairs"][0]
        print(json.dumps(dict(leg=name, n=m, len=48, **res["info"], work_items=ctx.stat("lineage_work_items"), pairs_kernel_ms=round(pairs_ms, 4),
                              tree_min_first_round_ms=tree["min_first_round_ms"], ratio_first_round=round(tree["min_first_round_ms"] / pairs_ms, 3),
                              ratio_later_round_mean=round(tree["min_later_round_mean_ms"] / pairs_ms, 3), word_ratio=8.0)), flush=True)
    ctx.close()


def cli(tag):
    from tests.test_gpu_annot import _argv, _write_inputs
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    out = dict(golden=tag)
    base = ["--quant", "q.tsv", "--airr", "a.tsv", "--lineages", "l.tsv"]
    with tempfile.TemporaryDirectory() as d:
        _write_inputs(tag, d)
        for name, extra in (("quant_airr_lineages_s", base), ("quant_airr_lineages_trees_s", base + ["--trees", "t.tsv"])):
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                r = subprocess.run([exe] + _argv(tag) + extra, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
                walls.append(time.perf_counter() - t0)
                if r.returncode:
                    raise SystemExit(r.stderr[-2000:])
            out[name] = round(min(walls), 3)
            out[name.replace("_s", "_all_s")] = [round(w, 3) for w in walls]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "cli":
        cli(sys.argv[2] if len(sys.argv) > 2 else "e2e_mixed")
    else:
        at_size()
