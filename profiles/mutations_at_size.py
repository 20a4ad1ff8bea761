"""vdjx_mutations at size: one JSON line for the largest input of profiles/annot_at_size.py -- 2,172 contigs of 360 bases (the
at_size_contigs recipe of tests/test_gpu_annot.py) against their repertoire's own 20,000 V + 20,000 J germlines -- with the hits of
vdjx_annotate: the kernel's time by the context's profiling scope (HIP events around the one dispatch) over repeated calls after a warm-up,
the bytes the kernel must move (contig bytes read, three rows written, the uploaded 64-byte contig records and 4-byte runs read, the
32-byte rows written), the share of the HBM peak that makes, the call's host-clock time, and vdjx_annotate's time on the same input.
   python profiles/mutations_at_size.py [out.json]
With `cli <tag>` instead: the wall time of `vdjer --quant --airr` against `vdjer --quant --airr --mutations` on one e2e golden (what the
flag adds to a run), best of three each.
   python profiles/mutations_at_size.py cli e2e_mixed"""
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

HBM_PEAK = 8.0e12                                # bytes per second (MI355X, HBM3E)
REPEATS = 50


def at_size(out_path=None):
    from vdjer_amd import annot, api
    ids, seqs, rep, _ = at_size_contigs()
    ctx = api.Context(0)
    ctx.germline_load([(f"V{i}", v) for i, v in enumerate(rep.v_germ)] + [(f"J{i}", j) for i, j in enumerate(rep.j_germ)])
    ctx.annotate(seqs[:64])                      # (warm-up: code objects, workspace)
    t0 = time.perf_counter()
    vj = ctx.annotate(seqs)
    annot_wall = time.perf_counter() - t0
    annot_ms = (ctx.stat("annot_score_us") + ctx.stat("annot_trace_us")) / 1e3
    limit = annot.mutation_limit(ids, seqs)
    for _ in range(3):                           # (warm-up)
        r = ctx.mutations(seqs, vj["v"], vj["j"], limit=limit)
    ctx.profile(True)
    ctx.profile_only("k_mutations")
    kernel_ms, call_ms = [], []
    for _ in range(REPEATS):
        ctx.profile_reset()
        ctx.mutations(seqs, vj["v"], vj["j"], limit=limit)
        ms, launches = ctx.profile_get()["k_mutations"]
        assert launches == 1
        kernel_ms.append(ms)
        call_ms.append(ctx.stat("mutations_us") / 1e3)
    ctx.profile_only(None)
    ctx.profile(False)
    n, m = len(seqs), len(seqs[0])
    cols = int(r["counts"]["cols"].sum())
    used = (r["counts"]["flags"] & 1) > 0
    runs = int(vj["v"]["n_runs"][used].sum()) + int(vj["j"]["n_runs"][(r["counts"]["flags"] & 2) > 0].sum())
    germ = sum(len(x) - x.count("-") - x.count("N") for x in r["germ"])       # germline codes read (a base of a mismatching codon is read twice: not counted)
    must = dict(contig_bytes=n * m, row_bytes=3 * cols, germline_bytes=germ, contig_records=64 * n, run_bytes=4 * runs, out_rows=32 * n)
    total = sum(must.values())
    k_med, k_min = float(np.median(kernel_ms)), float(min(kernel_ms))
    res = dict(contigs=n, len=m, germlines=len(rep.v_germ) + len(rep.j_germ), aligned=r["info"]["aligned"], cols=cols, v_codons=r["info"]["v_codons"],
               v_r=r["info"]["v_r"], v_s=r["info"]["v_s"], v_stop=r["info"]["v_stop"], v_na=r["info"]["v_na"], repeats=REPEATS,
               kernel_ms_median=round(k_med, 4), kernel_ms_min=round(k_min, 4), kernel_ms_max=round(float(max(kernel_ms)), 4),
               call_ms_median=round(float(np.median(call_ms)), 3), bytes_must_move=must, bytes_total=total,
               bytes_per_s=float("%.4g" % (total / (k_med * 1e-3))), share_of_hbm_peak=float("%.3g" % (total / (k_med * 1e-3) / HBM_PEAK)),
               floor_ms_at_hbm_peak=float("%.3g" % (total / HBM_PEAK * 1e3)), annotate_ms=round(annot_ms, 2), annotate_wall_ms=round(annot_wall * 1e3, 1),
               kernel_over_annotate=float("%.3g" % (k_med / annot_ms)), call_over_annotate=float("%.3g" % (float(np.median(call_ms)) / annot_ms)))
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    ctx.close()


def cli(tag):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    out = dict(golden=tag)
    with tempfile.TemporaryDirectory() as d:
        _write_inputs(tag, d)
        for name, extra in (("quant_airr_s", ["--quant", "q.tsv", "--airr", "a.tsv"]),
                            ("quant_airr_mutations_s", ["--quant", "q.tsv", "--airr", "a.tsv", "--mutations", "m.tsv"])):
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
        at_size(sys.argv[1] if len(sys.argv) > 1 else None)
