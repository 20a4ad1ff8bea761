"""vdjx_dcall at size: one JSON line for 2,172 contigs of 360 bases (the at_size_contigs recipe of tests/test_gpu_annot.py)
with their V and J hits, the windows d_window makes of them, and a D set of 34 records of 11 to 37 bases -- 24 cut from the middle of the
cores of 24 of the contigs' own clones, 10 decoys: the DP cells of the scoring phase, the milliseconds of the scoring and the traceback
phase (host clock around calls that end in a wait), cells per second and the profiling scopes of one call.  After a warm-up, best of five.
   python profiles/dcall_at_size.py
With `cli <tag>` instead: the wall time of `vdjer --quant --airr` against `vdjer --quant --airr --d-calls` on one e2e golden (what the
flag adds to a run), best of three each.
   python profiles/dcall_at_size.py cli e2e_mixed"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_gpu_annot import _argv, _rand, _write_inputs, at_size_contigs  # noqa: E402
from tests.test_gpu_dcall import _write_d  # noqa: E402


def d_set(rep, clone):
    """34 records of 11 .. 37 bases: 24 from the middle of the core (after the 300 bases of the V, before the J) of every 90th contig's
    clone, 10 random decoys among them"""
    rng = np.random.default_rng(34)
    recs = []
    for k in range(24):
        t = rep.clones[clone[90 * k]]
        core = t[300:len(t) - len(rep.j_germ[rep.clone_j[clone[90 * k]]])]
        n = min(int(rng.integers(11, 38)), len(core))
        o = (len(core) - n) // 2
        recs.append(core[o:o + n])
    for k in range(10):
        recs.insert(3 * k, _rand(rng, rng.integers(11, 38)))
    assert len(recs) == 34 and all(11 <= len(r) <= 37 for r in recs)
    return recs


def at_size():
    from vdjer_amd import annot, api
    ids, seqs, rep, clone = at_size_contigs()
    ctx = api.Context(0)
    ctx.germline_load([(f"V{i}", v) for i, v in enumerate(rep.v_germ)] + [(f"J{i}", j) for i, j in enumerate(rep.j_germ)])
    vj = ctx.annotate(seqs)
    ws, wl = annot.d_window(vj["v"], vj["j"])
    recs = d_set(rep, clone)
    ctx.dsegment_load([(f"D{k}", r) for k, r in enumerate(recs)])
    ctx.dcall(seqs[:64], ws[:64], wl[:64])                    # (warm-up: code objects, workspace)
    best = None
    for _ in range(5):
        t0 = time.perf_counter()
        h = ctx.dcall(seqs, ws, wl)
        wall = time.perf_counter() - t0
        cur = (ctx.stat("dcall_score_us"), ctx.stat("dcall_trace_us"), wall)
        best = cur if best is None or cur[0] + cur[1] < best[0] + best[1] else best
    cells = ctx.stat("dcall_cells")
    ctx.profile(True)
    ctx.profile_reset()
    ctx.dcall(seqs, ws, wl)
    prof = ctx.profile_get()
    us = max(best[0], 1)
    print(json.dumps(dict(contigs=len(seqs), records=len(recs), windows=int((wl > 0).sum()), longest_window=int(wl.max()), cells=cells,
                          score_ms=round(us / 1e3, 3), trace_ms=round(best[1] / 1e3, 3), wall_ms=round(best[2] * 1e3, 3),
                          cells_per_s=float("%.4g" % (cells / (us * 1e-6))), kernels_ms={k: round(v[0], 3) for k, v in prof.items()},
                          dispatches={k: v[1] for k, v in prof.items()}, called=int((h["d"]["gene"] >= 0).sum()),
                          tied=int((h["d"]["n_tied"] > 1).sum()))), flush=True)
    ctx.close()


def cli(tag):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    out = dict(golden=tag)
    with tempfile.TemporaryDirectory() as d:
        _write_inputs(tag, d)
        _write_d(tag, d)
        for name, extra in (("quant_airr_s", ["--quant", "q.tsv", "--airr", "a.tsv"]),
                            ("quant_airr_d_calls_s", ["--quant", "q.tsv", "--airr", "a.tsv", "--d-calls"])):
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                r = subprocess.run([exe] + _argv(tag) + extra, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
                wall = time.perf_counter() - t0
                if r.returncode:
                    raise SystemExit(r.stderr[-2000:])
                best = wall if best is None else min(best, wall)
            out[name] = round(best, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "cli":
        cli(sys.argv[2] if len(sys.argv) > 2 else "e2e_mixed")
    else:
        at_size()
