"""vdjx_consensus at size: one JSON line.  Leg "lineages": the input of profiles/targeting_at_size.py -- 2,172 contigs of 360
bases (the at_size_contigs recipe of tests/test_gpu_annot.py) against their repertoire's own 20,000 V + 20,000 J germlines, 3 % seeded
substitutions planted, the hits of vdjx_annotate and the lineages of vdjx_lineage as groups.  Leg "one_unit": ONE unit of 65,536 voters, the
first contig with a V hit copied with 3 % seeded substitutions of its own per copy and its hit repeated (257 workgroups of 255 voters over
one record: LDS counters flushed with global atomics).  Per leg: the two kernels' times by the context's profiling scopes (HIP events around
every dispatch) over repeated calls after a warm-up and the call's host-clock time; for the first leg k_tgt_mark's time on the same input
(the same walk) and whether the device's bytes equal the Python model.
   python profiles/consensus_at_size.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import consensus_model as CM  # noqa: E402
from tests.test_gpu_annot import at_size_contigs  # noqa: E402

REPEATS = 20
KERNELS = ("k_cons_vote", "k_cons_decide")
ONE_UNIT = 65536


def leg(ctx, name, seqs, v, limit, group):
    for _ in range(3):                           # (warm-up)
        r = ctx.consensus(seqs, v, limit=limit, group=group, counts=True)
    ctx.profile(True)
    ms = {k: [] for k in KERNELS}
    call_ms = []
    for _ in range(REPEATS):
        ctx.profile_reset()
        ctx.consensus(seqs, v, limit=limit, group=group, counts=True)
        got = ctx.profile_get()
        for k in KERNELS:
            ms[k].append(got[k][0] if k in got else 0.0)
        call_ms.append(ctx.stat("consensus_us") / 1e3)
    ctx.profile(False)
    out = dict(leg=name, repeats=REPEATS, call_ms_median=round(float(np.median(call_ms)), 3), largest_unit=int(max(r["units"]["members"])), **r["info"])
    for k in KERNELS:
        out[k + "_ms_median"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_min"] = round(float(min(ms[k])), 4)
        out[k + "_ms_max"] = round(float(max(ms[k])), 4)
    return out, r


def main(out_path=None):
    from vdjer_amd import annot, api
    ids, seqs, rep, _ = at_size_contigs()
    rng = np.random.default_rng(5)               # (targeting_at_size.py's planting: the recipe's contigs are verbatim germline)
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
    res = dict(input="at_size_contigs: 2,172 x 360 against 20,000 V + 20,000 J, 3 % substitutions", lineages=int(clone.max()) + 1, legs=[])
    out, r = leg(ctx, "lineages", seqs, vj["v"], limit, clone)
    for _ in range(3):
        ctx.targeting_counts(seqs, vj["v"], limit=limit, group=clone)
    ctx.profile(True)
    tm = []
    for _ in range(REPEATS):
        ctx.profile_reset()
        ctx.targeting_counts(seqs, vj["v"], limit=limit, group=clone)
        tm.append(ctx.profile_get()["k_tgt_mark"][0])
    ctx.profile(False)
    out["k_tgt_mark_ms"] = round(float(np.median(tm)), 4)
    out["vote_over_tgt_mark"] = round(out["k_cons_vote_ms_median"] / out["k_tgt_mark_ms"], 2)
    want = CM.consensus(seqs, vj["v"], germs, limit, clone)
    out["equal_the_model"] = bool(r["cons"] == want["cons"] and r["germ"] == want["germ"] and [x.tolist() for x in r["cover"]] == want["cover"]
                                  and [x.tolist() for x in r["best"]] == want["best"] and r["info"] == want["info"])
    res["legs"].append(out)
    # one unit of 65,536 voters
    c0 = int(np.flatnonzero((np.asarray(vj["v"]["gene"]) >= 0) & (np.asarray(vj["v"]["n_runs"]) <= 64))[0])
    base = np.frombuffer(seqs[c0].encode(), np.uint8)
    block = np.tile(base, (ONE_UNIT, 1))
    hit = rng.random(block.shape) < 0.03
    block[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    many = (block.tobytes(), ONE_UNIT, len(seqs[c0]))
    v1 = {f: np.repeat(np.asarray(x)[c0:c0 + 1], ONE_UNIT, axis=0) for f, x in vj["v"].items()}
    out, r1 = leg(ctx, "one_unit", many, v1, np.full(ONE_UNIT, int(limit[c0]), np.int32), np.zeros(ONE_UNIT, np.int32))
    a, b = int(vj["v"]["seq_start"][c0]) - 1, min(int(vj["v"]["seq_end"][c0]), int(limit[c0]))
    out["voters_per_column"] = int(min(r1["cover"][0])) if len(r1["cover"][0]) else 0
    out["consensus_is_the_founder"] = bool(int(vj["v"]["n_runs"][c0]) != 1 or r1["cons"][0] == seqs[c0][a:b])
    res["legs"].append(out)
    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
