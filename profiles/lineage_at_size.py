"""vdjx_lineage at size: one JSON line per leg with items, buckets, largest bucket, pairs, links, the best-of-five wall time of
the call after a warm-up, the kernels' own time (HIP events, a sixth call), the dispatches and pairs per second.
   python profiles/lineage_at_size.py
     at_size            the 2,172 contigs of the at_size_contigs recipe, grouped by the repertoire's own V / J assignment.  That repertoire
                        is private (every clone its own V and J), so this is 2,172 buckets of one: the call's fixed cost.
     at_size_one_group  the same junctions under ONE group: a bucket per junction length, the shape of an expanded sample
     one_bucket         65,536 junctions of 48 bases in one bucket (2.1e9 pairs; families of 64 around 1,024 founders): the rate when the
                        device is full
With `cli <tag>`: the wall time of `vdjer --quant --airr` with and without `--lineages` on one e2e golden, best of three each.
   python profiles/lineage_at_size.py cli e2e_mixed"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_gpu_annot import _argv, _write_inputs, at_size_contigs  # noqa: E402

KERNELS = ["k_lin_pack", "k_lin_pairs", "k_lin_flatten", "k_lin_number", "k_lin_out"]


def leg(ctx, name, junctions, group):
    ctx.lineage(junctions[:64], group[:64])                    # (warm-up: code objects, workspace)
    ctx.lineage(junctions, group)
    best = None
    for _ in range(5):
        t0 = time.perf_counter()
        res = ctx.lineage(junctions, group)
        wall = time.perf_counter() - t0
        cur = (ctx.stat("lineage_us"), wall)
        best = cur if best is None or cur[0] < best[0] else best
    ctx.profile(True)
    ctx.profile_reset()
    ctx.lineage(junctions, group)
    prof = ctx.profile_get()
    ctx.profile(False)
    info = res["info"]
    words = -(-max(len(j) for j in junctions) // 32)
    pairs_ms = prof.get("k_lin_pairs", (0.0, 0))[0]
    kernels_ms = sum(prof.get(k, (0.0, 0))[0] for k in KERNELS)
    # (the pair pass compares every ordered pair: each row against every column of its bucket)
    print(json.dumps(dict(leg=name, n=len(junctions), **info, work_items=ctx.stat("lineage_work_items"), call_ms=round(best[0] / 1e3, 3),
                          wall_ms=round(best[1] * 1e3, 3), kernels_ms=round(kernels_ms, 3), pairs_kernel_ms=round(pairs_ms, 3),
                          kernel_ms={k: round(prof.get(k, (0.0, 0))[0], 4) for k in KERNELS}, dispatches={k: v[1] for k, v in prof.items()},
                          pairs_per_s_call=float("%.4g" % (info["pairs"] / max(best[0] * 1e-6, 1e-9))),
                          pairs_per_s_kernel=float("%.4g" % (info["pairs"] / max(pairs_ms * 1e-3, 1e-9))),
                          word_compares_per_s_kernel=float("%.4g" % (2 * info["pairs"] * words / max(pairs_ms * 1e-3, 1e-9))))), flush=True)


def at_size():
    from vdjer_amd import api
    ids, _, rep, clone = at_size_contigs()
    junctions = [i.split("_", 2)[2] for i in ids]
    seen = {}
    group = np.array([seen.setdefault((rep.clone_v[c], rep.clone_j[c]), len(seen)) for c in clone], np.uint32)
    ctx = api.Context(0)
    leg(ctx, "at_size", junctions, group)
    leg(ctx, "at_size_one_group", junctions, np.zeros(len(junctions), np.uint32))
    rng = np.random.default_rng(48)
    founders = rng.integers(0, 4, (1024, 48), dtype=np.uint8)
    fam = np.repeat(founders, 64, axis=0)
    hit = rng.random(fam.shape) < 0.04                         # about two substitutions per junction
    fam = np.where(hit, (fam + rng.integers(1, 4, fam.shape, dtype=np.uint8)) % 4, fam).astype(np.uint8)
    text = np.frombuffer(b"ACGT", np.uint8)[fam[rng.permutation(len(fam))]]
    leg(ctx, "one_bucket", [bytes(r) for r in text], np.zeros(len(text), np.uint32))
    ctx.close()


def cli(tag):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    out = dict(golden=tag)
    with tempfile.TemporaryDirectory() as d:
        _write_inputs(tag, d)
        for name, extra in (("quant_airr_s", ["--quant", "q.tsv", "--airr", "a.tsv"]),
                            ("quant_airr_lineages_s", ["--quant", "q.tsv", "--airr", "a.tsv", "--lineages", "l.tsv"])):
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
