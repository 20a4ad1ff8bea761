"""vdjx_annotate at size, two legs, each printing one JSON line: the DP cells of the scoring phase, the milliseconds of the
scoring and the traceback phase, and the scoring phase's cells per second against the ceiling DESIGN §9 estimates.
  private   2,172 windows of make_repertoire(20000, private_v=True, private_j=True), cut to the 360 bases a contig keeps and named
            vjf_<n>_<junction>, against that repertoire's own germlines (20,000 V + 20,000 J)
  human     the same contigs against a human-sized set: 300 V of 300 bases and 13 J of 60 bases (random, seeded)
   python profiles/annot_at_size.py [private|human ...]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_gpu_annot import at_size_contigs  # noqa: E402

CEILING = 256 * 4 * 16 * 2 * 2.4e9 / 10       # CUs x SIMDs x lanes/clk x 2 (packed i16) x clock / ~10 VALU ops per cell


def leg(ctx, name, ids, seqs, recs):
    ctx.germline_load(recs)
    ctx.annotate(seqs[:64])                                   # (warm-up: code objects, workspace)
    t0 = time.perf_counter()
    h = ctx.annotate(seqs)
    wall = time.perf_counter() - t0
    cells = ctx.stat("annot_cells")
    us = max(ctx.stat("annot_score_us"), 1)
    return dict(leg=name, contigs=len(seqs), germlines=len(recs), cells=cells, score_ms=round(us / 1e3, 2),
                trace_ms=round(ctx.stat("annot_trace_us") / 1e3, 2), wall_ms=round(wall * 1e3, 1), cells_per_s=float("%.4g" % (cells / (us * 1e-6))),
                of_ceiling=round(cells / (us * 1e-6) / CEILING, 4), v_called=int((h["v"]["gene"] >= 0).sum()), j_called=int((h["j"]["gene"] >= 0).sum()))


def main():
    legs = sys.argv[1:] or ["private", "human"]
    from vdjer_amd import api
    ids, seqs, rep, _ = at_size_contigs()
    ctx = api.Context(0)
    for name in legs:
        if name == "private":
            recs = [(f"V{i}", v) for i, v in enumerate(rep.v_germ)] + [(f"J{i}", j) for i, j in enumerate(rep.j_germ)]
        else:
            rng = np.random.default_rng(7)
            recs = [(f"IGHV{i}*01", "".join(rng.choice(list("ACGT"), 300))) for i in range(300)]
            recs += [(f"IGHJ{i}*01", "".join(rng.choice(list("ACGT"), 60))) for i in range(13)]
        print(json.dumps(leg(ctx, name, ids, seqs, recs)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
