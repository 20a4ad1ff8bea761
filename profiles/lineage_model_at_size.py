"""vdjx_lineage_model at size, on the input of profiles/lineage_at_size.py: the time of k_lin_pairs (the Hamming pass) and of
k_lin_pairs_model under three tables -- uniform, realistic (annot.targeting_model over seeded counts) and extreme (seeded cells, a quarter
of them 1 and a quarter 65,535) -- from the context's event scopes, after a warm-up, the median of REPEATS calls; beside each time the pairs
walked and the positions per walked pair, which explain it.  One JSON line per leg; with `--out <file>` the lines are kept in that file.
   python profiles/lineage_model_at_size.py [--out profiles/lineage_model_at_size.json]
The pre-filter is measured by running the ablation build (make -C vdjer_amd/csrc ablate) twice:
   VDJX_LIB_PATH=vdjer_amd/libvdjx_ablate.so python profiles/lineage_model_at_size.py
   VDJX_LIB_PATH=vdjer_amd/libvdjx_ablate.so VDJX_LIN_NOFILTER=1 python profiles/lineage_model_at_size.py"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lineage_dist_cases as LC  # noqa: E402
from tests.test_gpu_annot import at_size_contigs  # noqa: E402

REPEATS = 7


def kernel_ms(ctx, scope, call):
    """the median over REPEATS calls of the scope's event time, after one warm-up call"""
    call()
    times = []
    res = None
    for _ in range(REPEATS):
        ctx.profile(True)
        ctx.profile_reset()
        res = call()
        times.append(ctx.profile_get()[scope][0])
        ctx.profile(False)
    return statistics.median(times), times, res


def legs(ctx, name, junctions, group, out):
    base, all_, res = kernel_ms(ctx, "k_lin_pairs", lambda: ctx.lineage(junctions, group))
    info = res["info"]
    row = dict(leg=name, kernel="k_lin_pairs", n=len(junctions), **info, work_items=ctx.stat("lineage_work_items"), ms=round(base, 4), all_ms=[round(t, 4) for t in all_])
    out.append(row)
    print(json.dumps(row), flush=True)
    for tab in ("uniform", "realistic", "extreme"):
        for sym in ("avg", "min"):
            ms, all_, res = kernel_ms(ctx, "k_lin_pairs_model", lambda: ctx.lineage(junctions, group, table=LC.tables()[tab], symmetry=sym))
            walked, positions = ctx.stat("lineage_model_walked"), ctx.stat("lineage_model_positions")
            row = dict(leg=name, kernel="k_lin_pairs_model", table=tab, symmetry=sym, filter=not os.environ.get("VDJX_LIN_NOFILTER"), **res["info"], ms=round(ms, 4),
                       all_ms=[round(t, 4) for t in all_], ratio_to_hamming=round(ms / base, 2), walked=walked, ordered_pairs=2 * res["info"]["pairs"],
                       positions=positions, positions_per_walked_pair=round(positions / max(walked, 1), 2))
            out.append(row)
            print(json.dumps(row), flush=True)


def main():
    from vdjer_amd import api
    ids, _, rep, clone = at_size_contigs()
    junctions = [i.split("_", 2)[2] for i in ids]
    ctx = api.Context(0)
    out = []
    legs(ctx, "at_size_one_group", junctions, np.zeros(len(junctions), np.uint32), out)
    rng = np.random.default_rng(48)
    founders = rng.integers(0, 4, (1024, 48), dtype=np.uint8)
    fam = np.repeat(founders, 64, axis=0)
    hit = rng.random(fam.shape) < 0.04                         # about two substitutions per junction
    fam = np.where(hit, (fam + rng.integers(1, 4, fam.shape, dtype=np.uint8)) % 4, fam).astype(np.uint8)
    text = np.frombuffer(b"ACGT", np.uint8)[fam[rng.permutation(len(fam))]]
    legs(ctx, "one_bucket", [bytes(r) for r in text], np.zeros(len(text), np.uint32), out)
    ctx.close()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(dict(lib=os.environ.get("VDJX_LIB_PATH", "vdjer_amd/libvdjx.so"), repeats=REPEATS, legs=out), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
