"""vdjx_selection_convolve at size: one JSON line for the input of profiles/selection_at_size.py -- 2,172 contigs of 360 bases
with 3 % seeded substitutions against their repertoire's 20,000 V + 20,000 J germlines, two regions, seeded random weights -- whose count
rows (one vdjx_selection call) are convolved under three groupings: the lineages of vdjx_lineage, all contigs in one group, and groups of
64 contigs.  Per grouping: three warm-up calls, twenty timed ones, medians; each kernel's time by the context's profiling scopes (HIP
events around every dispatch), the combinations per second and the float64 multiply-adds per second of k_conv_combine (counted from the
trees: 4,001^2 per combination of equal weights, 6 x 4,001^2 per one of unequal weights, the six candidates it weighs per pair), the
call's host-clock time.  Once: vdjx_selection's time on the same input, and the float64 numpy model's time (tests/selection_conv_model.py)
for the lineage grouping with the largest deviation of the device's sigma from it.
   python profiles/selconv_at_size.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import selection_conv_model as CM  # noqa: E402
from tests.test_gpu_annot import at_size_contigs  # noqa: E402

REPEATS = 20
KERNELS = ("k_conv_leaf", "k_conv_combine", "k_conv_finish")
T = 4001
# MI355X: 256 CUs x 4 SIMDs x 16 float64 lanes per clock x 2.4 GHz: half the 157.3 TFLOP/s float32 vector peak of the datasheet
FP64_VECTOR_FMA_PER_S = 256 * 4 * 16 * 2.4e9


def combos(m):
    """(equal, unequal) combinations of the tree of m leaves"""
    if m <= 1:
        return 0, 0
    h = CM.split(m)
    a, b = combos(h), combos(m - h)
    return a[0] + b[0] + (h == m - h), a[1] + b[1] + (h != m - h)


def leg(ctx, name, counts, group, G):
    for _ in range(3):
        r = ctx.selection_convolve(counts, 2, group, G)
    ctx.profile(True)
    ms = {k: [] for k in KERNELS}
    call_ms = []
    for _ in range(REPEATS):
        ctx.profile_reset()
        ctx.selection_convolve(counts, 2, group, G)
        got = ctx.profile_get()
        for k in KERNELS:
            ms[k].append(got[k][0] if k in got else 0.0)
        call_ms.append(ctx.stat("selconv_us") / 1e3)
    ctx.profile(False)
    launches = {k: got[k][1] for k in KERNELS if k in got}
    mem = CM.members(dict(counts, flags=np.zeros(len(counts["obs_r"]))), 2)
    sets = [np.flatnonzero(group == g) for g in range(G)] + [np.arange(len(group))]
    eq = un = 0
    for st in sets:
        for k in range(2):
            e, u = combos(sum(mem[k][i] is not None for i in st))
            eq, un = eq + e, un + u
    assert eq + un == r["info"]["combines"], (eq, un, r["info"])
    med = {k: float(np.median(x)) for k, x in ms.items()}
    fma = eq * T * T + un * 6 * T * T
    out = dict(leg=name, groups=G, rows=r["info"]["rows"], members=r["info"]["members"], leaves=r["info"]["leaves"], combines=r["info"]["combines"],
               combines_equal=eq, combines_unequal=un, levels=r["info"]["levels"], batches=r["info"]["batches"], launches=launches, repeats=REPEATS,
               call_ms_median=round(float(np.median(call_ms)), 3), call_ms_min=round(float(min(call_ms)), 3), call_ms_max=round(float(max(call_ms)), 3))
    for k in KERNELS:
        out[k + "_ms_median"] = round(med[k], 4)
        out[k + "_ms_min"] = round(float(min(ms[k])), 4)
        out[k + "_ms_max"] = round(float(max(ms[k])), 4)
    if med["k_conv_combine"] > 0:
        out["combines_per_s"] = float("%.4g" % (r["info"]["combines"] / (med["k_conv_combine"] * 1e-3)))
        out["fma_per_s"] = float("%.4g" % (fma / (med["k_conv_combine"] * 1e-3)))
        out["share_of_fp64_vector_peak"] = float("%.3g" % (out["fma_per_s"] / FP64_VECTOR_FMA_PER_S))
    return out, r


def main(out_path=None):
    from vdjer_amd import annot, api
    ids, seqs, rep, _ = at_size_contigs()
    rng = np.random.default_rng(5)               # (profiles/selection_at_size.py's input: 3 % substitutions)
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
    kw = dict(limit=limit, cdr=cdr, weight=weight, group=clone, groups=G)
    for _ in range(3):
        sel = ctx.selection(seqs, vj["v"], **kw)
    sel_ms = []
    for _ in range(REPEATS):
        ctx.selection(seqs, vj["v"], **kw)
        sel_ms.append(ctx.stat("selection_us") / 1e3)
    counts = sel["counts"]
    n = len(seqs)
    res = dict(input="at_size_contigs: 2,172 x 360 against 20,000 V + 20,000 J, two regions, random weights", contigs=n, lineages=G,
               largest_lineage=int(np.bincount(clone[clone >= 0]).max()), selection_call_ms_median=round(float(np.median(sel_ms)), 3),
               fp64_vector_fma_per_s_peak=FP64_VECTOR_FMA_PER_S, legs=[])
    groupings = (("lineages", clone, G), ("one_group", np.zeros(n, np.int32), 1), ("groups_of_64", (np.arange(n) // 64).astype(np.int32), (n + 63) // 64))
    dev = None
    for name, grp, g in groupings:
        out, r = leg(ctx, name, counts, grp, g)
        res["legs"].append(out)
        if name == "lineages":
            dev = r
    ctx.close()
    t0 = time.perf_counter()
    rows = CM.rows(counts, 2, clone, G, np.float64)
    t1 = time.perf_counter()
    ds = max(abs(float(dev["stat"]["sigma"][i, k]) - float(rows[i][k]["sigma"])) for i in range(len(rows)) for k in range(2))
    res.update(numpy_model_s=round(t1 - t0, 3), sigma_max_abs_deviation=float("%.3g" % ds))
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
