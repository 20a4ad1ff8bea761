"""vdjx_tree_support at size, B = 100 replicates: one JSON line per leg with the info, the best-of-three time of the call after
a warm-up, the kernels' own time (HIP events, one more call) in all, by kernel and PER REPLICATE, and next to it the kernels' time of
vdjx_tree on the same input, measured in the same session -- its kernels are the ones a replicate runs on about half the words, so that
figure is the baseline -- and the ratio of the two.
   python profiles/tree_support_at_size.py [out.json]
     small_lineages     §13's input: 20,000 lineages of 1 .. 8 contigs of 486 bases, interleaved
     one_lineage_4096   one lineage of 4,096 contigs of 486 bases (about 8 words a row and replicate, 12 rounds)
With a file name the legs are written there as well, as profiles/tree_support_at_size.json holds them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.tree_at_size import ACGT, KERNELS, descent  # noqa: E402

B = 100
ROUNDS = ["k_tree_min_first", "k_tree_min", "k_tree_hook", "k_tree_flat"]
SUPPORT_KERNELS = ["k_tree_pack_sel"] + ROUNDS + ["k_tree_support"]


def _profiled(ctx, call):
    ctx.profile(True)
    ctx.profile_reset()
    call()
    prof = ctx.profile_get()
    ctx.profile(False)
    return prof


def leg(ctx, name, packed, clone, anchor):
    small = (packed[0][:64 * packed[2]], 64, packed[2])
    tree = ctx.tree(packed, clone, anchor)                              # (also the warm-up of vdjx_tree)
    parent = tree["parent"]
    ctx.tree_support(small, clone[:64], anchor[:64], np.full(64, -1, np.int32), 2, 1)      # (warm-up: code objects)
    ctx.tree_support(packed, clone, anchor, parent, B, 1)                                  # (... and the workspace)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        res = ctx.tree_support(packed, clone, anchor, parent, B, 1)
        wall = time.perf_counter() - t0
        cur = (ctx.stat("tree_support_us"), wall)
        best = cur if best is None or cur[0] < best[0] else best
    prof = _profiled(ctx, lambda: ctx.tree_support(packed, clone, anchor, parent, B, 1))
    base = _profiled(ctx, lambda: ctx.tree(packed, clone, anchor))
    ms = {k: prof.get(k, (0.0, 0))[0] for k in SUPPORT_KERNELS}
    kernels, tree_kernels = sum(ms.values()), sum(base.get(k, (0.0, 0))[0] for k in KERNELS)
    parts = dict(pack=ms["k_tree_pack_sel"], rounds=sum(ms[k] for k in ROUNDS), support=ms["k_tree_support"])
    tree_parts = dict(pack=base.get("k_tree_pack", (0.0, 0))[0], rounds=sum(base.get(k, (0.0, 0))[0] for k in ROUNDS))
    out = dict(leg=name, n=packed[1], len=packed[2], **res["info"], work_items=ctx.stat("tree_support_work_items"), call_ms=round(best[0] / 1e3, 3),
               wall_ms=round(best[1] * 1e3, 3), kernels_ms=round(kernels, 3), kernel_ms={k: round(v, 4) for k, v in ms.items()},
               dispatches={k: v[1] for k, v in prof.items()}, per_replicate_kernels_ms=round(kernels / B, 4),
               per_replicate_ms={k: round(v / B, 4) for k, v in parts.items()},
               tree_kernels_ms=round(tree_kernels, 4), tree_ms={k: round(v, 4) for k, v in tree_parts.items()},
               ratio_replicate_to_tree=round(kernels / B / tree_kernels, 3),
               ratio_by_part={k: round(parts[k] / B / tree_parts[k], 3) for k in tree_parts},
               mean_support=round(res["info"]["matched"] / max(1, res["info"]["edges"] * B), 4))
    print(json.dumps(out), flush=True)
    return out


def at_size():
    from vdjer_amd import api
    ctx = api.Context(0)
    rng = np.random.default_rng(486)
    L = 486
    sizes = 1 + np.arange(20000) % 8
    rows = np.concatenate([descent(rng, int(m), L, 0.01) for m in sizes])
    clone = np.repeat(np.arange(20000), sizes).astype(np.int32)
    order = rng.permutation(len(rows))
    legs = [leg(ctx, "small_lineages", (ACGT[rows[order]].tobytes(), len(rows), L), clone[order], np.full(len(rows), 300, np.int32))]
    m = 4096
    rows = descent(rng, m, L, 0.004)[rng.permutation(m)]
    legs.append(leg(ctx, "one_lineage_4096", (ACGT[rows].tobytes(), m, L), np.zeros(m, np.int32), np.full(m, 300, np.int32)))
    ctx.close()
    return legs


if __name__ == "__main__":
    legs = at_size()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(dict(what="profiles/tree_support_at_size.py, as printed", where="one MI355X", replicates=B, legs=legs), f, indent=1)
            f.write("\n")
