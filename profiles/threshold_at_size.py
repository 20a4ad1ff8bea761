"""vdjx_lineage_threshold at size: per input every kernel's time from the context's event scopes (after a warm-up, the median of
REPEATS calls), the call's host time, the one build of the kernel tables, the multiply-adds of the density pass and their rate.  Inputs:
  at_size_one_group  the nearest distances vdjx_lineage gives for the 2,172 contigs of profiles/lineage_at_size.py under one group, with
                     k_lin_pairs' time on the same input beside it (what the second pair pass of `vdjer --lineage-threshold` costs) and the
                     model's time in Python
  sampler_max        2^20 - 1 values of the two-mode sampler of tests/threshold_cases.py
  every_bin          all 10,001 bins non-zero: every window spans every tile
   python profiles/threshold_at_size.py [out.json]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import threshold_cases as TC  # noqa: E402
from tests import threshold_model as M  # noqa: E402
from tests.test_gpu_annot import at_size_contigs  # noqa: E402

REPEATS = 7
KERNELS = ["k_thr_hist", "k_thr_number", "k_thr_compact", "k_thr_density", "k_thr_peaks"]


def leg(ctx, name, near, length, unit=1):
    t0 = time.perf_counter()
    res = ctx.lineage_threshold(near, length, unit)               # the first call of the process builds the tables
    first_ms = (time.perf_counter() - t0) * 1e3
    times, host = {k: [] for k in KERNELS}, []
    for _ in range(REPEATS):
        ctx.profile(True)
        ctx.profile_reset()
        again = ctx.lineage_threshold(near, length, unit)
        got = ctx.profile_get()
        ctx.profile(False)
        assert again["info"] == res["info"] and {k: got[k][1] for k in KERNELS} == dict.fromkeys(KERNELS, 1)
        for k in KERNELS:
            times[k].append(got[k][0])
    for _ in range(REPEATS):                                     # the host clock without the event brackets
        ctx.lineage_threshold(near, length, unit)
        host.append(ctx.stat("threshold_us") / 1e3)
    macs = ctx.stat("threshold_macs")
    dens = statistics.median(times["k_thr_density"])
    row = dict(leg=name, n=len(near), unit=unit, **res["info"], status_name=M.STATUS[res["info"]["status"]], macs=macs,
               kernel_ms={k: round(statistics.median(v), 4) for k, v in times.items()}, kernel_all_ms={k: [round(t, 4) for t in v] for k, v in times.items()},
               macs_per_s=round(macs / (dens * 1e-3)) if dens > 0 else None, host_ms=round(statistics.median(host), 3), host_all_ms=[round(t, 3) for t in host],
               first_call_ms=round(first_ms, 3), table_build_ms=round(ctx.stat("threshold_table_us") / 1e3, 3))
    print(json.dumps(row), flush=True)
    return row


def main():
    from vdjer_amd import api
    ids, _, _, _ = at_size_contigs()
    junctions = [i.split("_", 2)[2] for i in ids]
    ctx = api.Context(0)
    out = []
    lin = ctx.lineage(junctions, np.zeros(len(junctions), np.uint32))
    pair = []
    for _ in range(REPEATS):
        ctx.profile(True)
        ctx.profile_reset()
        ctx.lineage(junctions, np.zeros(len(junctions), np.uint32))
        pair.append(ctx.profile_get()["k_lin_pairs"][0])
        ctx.profile(False)
    lens = np.array([len(j) for j in junctions], np.uint32)
    row = leg(ctx, "at_size_one_group", lin["nearest"], lens)
    row["k_lin_pairs_ms"] = round(statistics.median(pair), 4)
    row["lineage_host_ms"] = round(ctx.stat("lineage_us") / 1e3, 3)
    t0 = time.perf_counter()
    M.kernel.cache_clear()
    model = M.threshold(M.bins(lin["nearest"], lens, 1))
    row["model_python_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert model["info"] == {k: row[k] for k in M.INFO_FIELDS}
    out.append(row)
    near, length, unit, _ = TC.sampler(65536, (1 << 20) - 1 - 65536, 3)
    out.append(leg(ctx, "sampler_max", near, length, unit))
    near, length, unit, _ = TC.cases("default")["every_bin"]
    out.append(leg(ctx, "every_bin", near, length, unit))
    ctx.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(dict(repeats=REPEATS, legs=out), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
