"""vdjx_selection at size: one JSON line for the largest input of profiles/annot_at_size.py -- 2,172 contigs of 360 bases (the
at_size_contigs recipe of tests/test_gpu_annot.py) against their repertoire's own 20,000 V + 20,000 J germlines -- with 3 % seeded
substitutions planted in the contigs, the hits of vdjx_annotate, two regions (CDR1 24 bases from a quarter of the V record on, CDR2 30 bases from its half on) and the lineages of
vdjx_lineage as groups; twice, with the uniform model and with seeded random weights.  Per leg: each kernel's time by the context's
profiling scopes (HIP events around every dispatch) over repeated calls after a warm-up, the grid-point-members per second of k_sel_finish
(and of k_sel_loglik where rows are large), the call's host-clock time, and k_mutations' time on the same input next to k_sel_counts.
Once: the numpy model's time on the same input (tests/selection_model.py in float64: the counts in plain Python, the posterior in numpy),
and the largest deviation of the device's sigma from it.  A second pair of legs runs with VDJX_SEL_CHUNK=64, so that the sample row and
the large lineages go through k_sel_loglik.
   python profiles/selection_at_size.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import selection_model as S  # noqa: E402
from tests.test_gpu_annot import at_size_contigs  # noqa: E402

REPEATS = 20
KERNELS = ("k_sel_counts", "k_sel_loglik", "k_sel_finish")


def leg(ctx, name, seqs, v, limit, cdr, weight, clone, G, mut_ms):
    kw = dict(limit=limit, cdr=cdr, weight=weight, group=clone, groups=G)
    for _ in range(3):                           # (warm-up)
        r = ctx.selection(seqs, v, **kw)
    ctx.profile(True)
    ms = {k: [] for k in KERNELS}
    call_ms = []
    for _ in range(REPEATS):
        ctx.profile_reset()
        ctx.selection(seqs, v, **kw)
        got = ctx.profile_get()
        for k in KERNELS:
            ms[k].append(got[k][0] if k in got else 0.0)
        call_ms.append(ctx.stat("selection_us") / 1e3)
    ctx.profile(False)
    n, K = len(seqs), 2
    sizes = [1] * n + [int((clone == g).sum()) for g in range(G)] + [n]
    chunk = int(os.environ.get("VDJX_SEL_CHUNK", "1024"))
    direct = sum(m for m in sizes if m <= chunk) * K * S.T
    chunked = sum(m for m in sizes if m > chunk) * K * S.T
    med = {k: float(np.median(x)) for k, x in ms.items()}
    out = dict(leg=name, chunk=chunk, contigs=n, used=r["info"]["used"], groups=G, regions=K, rows=len(sizes), chunks=r["info"]["chunks"],
               large_rows=r["info"]["large_rows"], repeats=REPEATS, call_ms_median=round(float(np.median(call_ms)), 3), mutations_kernel_ms=round(mut_ms, 4))
    for k in KERNELS:
        out[k + "_ms_median"] = round(med[k], 4)
        out[k + "_ms_min"] = round(float(min(ms[k])), 4)
        out[k + "_ms_max"] = round(float(max(ms[k])), 4)
    out["finish_grid_point_members"] = direct
    out["finish_grid_point_members_per_s"] = float("%.4g" % (direct / (med["k_sel_finish"] * 1e-3)))
    if chunked:
        out["loglik_grid_point_members"] = chunked
        out["loglik_grid_point_members_per_s"] = float("%.4g" % (chunked / (med["k_sel_loglik"] * 1e-3)))
    return out, r


def main(out_path=None):
    from vdjer_amd import annot, api
    ids, seqs, rep, _ = at_size_contigs()
    rng = np.random.default_rng(5)               # the recipe's contigs are verbatim germline: 3 % substitutions, so that there is something to weigh
    seqs = ["".join("ACGT"[("ACGT".index(ch) + 1 + int(rng.integers(0, 3))) % 4] if rng.random() < 0.03 else ch for ch in q) for q in seqs]
    germs = list(rep.v_germ) + list(rep.j_germ)
    names = [f"V{i}" for i in range(len(rep.v_germ))] + [f"J{i}" for i in range(len(rep.j_germ))]
    ctx = api.Context(0)
    ginfo = ctx.germline_load(list(zip(names, germs)))
    ctx.annotate(seqs[:64])                      # (warm-up: code objects, workspace)
    vj = ctx.annotate(seqs)
    limit = annot.mutation_limit(ids, seqs)
    junctions, group, _, _ = annot.lineage_inputs(ids, seqs, vj["v"], vj["j"], ginfo["names"])
    clone = ctx.lineage(junctions, group)["clone"].astype(np.int32)
    G = int(clone.max()) + 1
    cdr = np.zeros((len(germs), 4), np.int32)
    for r_, g in enumerate(rep.v_germ):
        L = len(g)
        cdr[r_] = (L // 4, L // 4 + 23, L // 2, L // 2 + 29)
    weight = np.random.default_rng(11).integers(0, 10 ** 7, (1024, 4)).astype(np.uint32)
    for _ in range(3):
        ctx.mutations(seqs, vj["v"], vj["j"], limit=limit, rows=False)
    ctx.profile(True)
    mm = []
    for _ in range(REPEATS):
        ctx.profile_reset()
        ctx.mutations(seqs, vj["v"], vj["j"], limit=limit, rows=False)
        mm.append(ctx.profile_get()["k_mutations"][0])
    ctx.profile(False)
    mut_ms = float(np.median(mm))
    res = dict(input="at_size_contigs: 2,172 x 360 against 20,000 V + 20,000 J", lineages=G, largest_lineage=int(np.bincount(clone[clone >= 0]).max()), legs=[])
    dev = {}
    for chunk in ("1024", "64"):
        os.environ["VDJX_SEL_CHUNK"] = chunk     # (read per call)
        for name, w in (("uniform", None), ("weighted", weight)):
            out, r = leg(ctx, name, seqs, vj["v"], limit, cdr, w, clone, G, mut_ms)
            res["legs"].append(out)
            if chunk == "1024":
                dev[name] = r
    ctx.close()
    # the numpy model on the same input, float64
    t0 = time.perf_counter()
    cnt = S.counts(seqs, vj["v"], limit, germs, cdr, weight)
    t1 = time.perf_counter()
    rows = S.rows(cnt, 2, clone, G, np.float64)
    t2 = time.perf_counter()
    r = dev["weighted"]
    same = all([[int(y) for y in row] for row in r["counts"][f]] == [[int(y) for y in row] for row in cnt[f]] for f in ("obs_r", "obs_s", "codons", "exp_r", "exp_s"))
    ds = max(abs(float(r["stat"]["sigma"][i, k]) - float(rows[i][k]["sigma"])) for i in range(len(rows)) for k in range(2))
    res.update(numpy_counts_s=round(t1 - t0, 3), numpy_posterior_s=round(t2 - t1, 3), counts_equal_the_model=bool(same), sigma_max_abs_deviation=float("%.3g" % ds))
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
