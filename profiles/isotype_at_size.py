"""vdjx_isotype at size: one JSON line for the at-size case of tests/test_gpu_isotype.py -- 2,172 contigs of 360 bases
(the at_size_contigs recipe) against 9 constant records of 1,000 bases -- with the DP cells of the scoring phase, the milliseconds of
the scoring and the traceback phase (host clock around calls that end in a wait), cells per second and the kernel dispatches of the call.
   python profiles/isotype_at_size.py
With `cli <tag>` instead: the wall time of `vdjer --quant --airr` against `vdjer --quant --airr --isotypes --clones --cfa` on one e2e
golden (what the feature adds to a run), best of three each.
   python profiles/isotype_at_size.py cli e2e_mixed"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_gpu_isotype import _write_cfa, at_size_case  # noqa: E402
from tests.test_gpu_annot import _argv, _write_inputs  # noqa: E402


def at_size():
    from vdjer_amd import api
    ids, seqs, recs = at_size_case()
    ctx = api.Context(0)
    ctx.constant_load([(f"C{k}", r) for k, r in enumerate(recs)])
    ctx.isotype(seqs[:64])                                    # (warm-up: code objects, workspace)
    best = None
    for _ in range(5):
        t0 = time.perf_counter()
        h = ctx.isotype(seqs)
        wall = time.perf_counter() - t0
        cur = (ctx.stat("iso_score_us"), ctx.stat("iso_trace_us"), wall)
        best = cur if best is None or cur[0] < best[0] else best
    ctx.profile(True)
    ctx.profile_reset()
    ctx.isotype(seqs)
    prof = ctx.profile_get()
    cells = ctx.stat("iso_cells")
    us = max(best[0], 1)
    kernel_ms = prof.get("k_iso_score", (0.0, 0))[0]
    print(json.dumps(dict(contigs=len(seqs), records=len(recs), cells=cells, score_ms=round(us / 1e3, 3), trace_ms=round(best[1] / 1e3, 3),
                          wall_ms=round(best[2] * 1e3, 3), cells_per_s=float("%.4g" % (cells / (us * 1e-6))),
                          score_kernels_ms=round(kernel_ms, 3), cells_per_s_kernels=float("%.4g" % (cells / max(kernel_ms * 1e-3, 1e-9))),
                          dispatches={k: v[1] for k, v in prof.items()}, called=int((h["c"]["gene"] >= 0).sum()))), flush=True)
    ctx.close()


def cli(tag):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    out = dict(golden=tag)
    with tempfile.TemporaryDirectory() as d:
        rep = _write_inputs(tag, d)
        _write_cfa(rep, d)
        for name, extra in (("quant_airr_s", ["--quant", "q.tsv", "--airr", "a.tsv"]),
                            ("quant_airr_isotypes_clones_s", ["--quant", "q.tsv", "--airr", "a.tsv", "--isotypes", "i.tsv", "--clones", "c.tsv", "--cfa", "c.fa"])):
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
