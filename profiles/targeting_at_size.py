"""vdjx_targeting_counts at size: one JSON line for the input of profiles/selection_at_size.py -- 2,172 contigs of 360 bases (the
at_size_contigs recipe of tests/test_gpu_annot.py) against their repertoire's own 20,000 V + 20,000 J germlines, with 3 % seeded
substitutions planted in the contigs, the hits of vdjx_annotate and the lineages of vdjx_lineage as groups.  Two legs, VDJX_TGT_UNITS at its
default and at 4,096: the two kernels' times by the context's profiling scopes (HIP events around every dispatch; summed over a call's
batches) over repeated calls after a warm-up, and the call's host-clock time.  Once: k_sel_counts' time on the same input (uniform model,
one region) next to k_tgt_mark, which does the same walk; the time of the model finish (vdjx_targeting_model, plain C); the numpy model's
time on the same input and whether the device's counts equal it.
   python profiles/targeting_at_size.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import targeting_model as T  # noqa: E402
from tests.test_gpu_annot import at_size_contigs  # noqa: E402

REPEATS = 20
KERNELS = ("k_tgt_mark", "k_tgt_count")


def leg(ctx, units, seqs, v, limit, clone, sel_ms):
    if units is None:
        os.environ.pop("VDJX_TGT_UNITS", None)
    else:
        os.environ["VDJX_TGT_UNITS"] = units     # (read per call)
    for _ in range(3):                           # (warm-up)
        r = ctx.targeting_counts(seqs, v, limit=limit, group=clone)
    ctx.profile(True)
    ms = {k: [] for k in KERNELS}
    call_ms = []
    for _ in range(REPEATS):
        ctx.profile_reset()
        ctx.targeting_counts(seqs, v, limit=limit, group=clone)
        got = ctx.profile_get()
        for k in KERNELS:
            ms[k].append(got[k][0] if k in got else 0.0)
        call_ms.append(ctx.stat("targeting_us") / 1e3)
    ctx.profile(False)
    out = dict(units_per_batch=int(units or 1 << 18), repeats=REPEATS, call_ms_median=round(float(np.median(call_ms)), 3), k_sel_counts_ms=round(sel_ms, 4),
               bitmap_bytes=1024 * min(r["info"]["units"], int(units or 1 << 18)), **r["info"])
    for k in KERNELS:
        out[k + "_ms_median"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_min"] = round(float(min(ms[k])), 4)
        out[k + "_ms_max"] = round(float(max(ms[k])), 4)
    out["mark_over_sel_counts"] = round(out["k_tgt_mark_ms_median"] / sel_ms, 2)
    return out, r


def main(out_path=None):
    from vdjer_amd import annot, api
    ids, seqs, rep, _ = at_size_contigs()
    rng = np.random.default_rng(5)               # (selection_at_size.py's planting: the recipe's contigs are verbatim germline)
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
    for _ in range(3):
        ctx.selection(seqs, vj["v"], limit=limit)
    ctx.profile(True)
    sm = []
    for _ in range(REPEATS):
        ctx.profile_reset()
        ctx.selection(seqs, vj["v"], limit=limit)
        sm.append(ctx.profile_get()["k_sel_counts"][0])
    ctx.profile(False)
    sel_ms = float(np.median(sm))
    res = dict(input="at_size_contigs: 2,172 x 360 against 20,000 V + 20,000 J, 3 % substitutions", lineages=int(clone.max()) + 1,
               largest_lineage=int(np.bincount(clone[clone >= 0]).max()), legs=[])
    dev = None
    for units in (None, "4096"):
        out, r = leg(ctx, units, seqs, vj["v"], limit, clone, sel_ms)
        res["legs"].append(out)
        same = dev is None or dev["counts"].tobytes() == r["counts"].tobytes()
        dev = r
    os.environ.pop("VDJX_TGT_UNITS", None)
    ctx.close()
    t0 = time.perf_counter()
    for _ in range(REPEATS):
        w, lv = annot.targeting_model(dev["counts"], "rs", 50, 500)
    t1 = time.perf_counter()
    cnt, info = T.counts(seqs, vj["v"], limit, germs, clone)
    t2 = time.perf_counter()
    mw, mlv = T.model(cnt, "rs", 50, 500)
    res.update(model_finish_ms=round((t1 - t0) / REPEATS * 1e3, 3), numpy_counts_s=round(t2 - t1, 3), legs_equal=bool(same),
               counts_equal_the_model=bool(np.array_equal(cnt, dev["counts"]) and info == dict(dev["info"], batches=info["batches"])),
               weights_equal_the_model=bool(np.array_equal(w, mw) and np.array_equal(lv, mlv)), levels_rs=T.level_counts(lv))
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
