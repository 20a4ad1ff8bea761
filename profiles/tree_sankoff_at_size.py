"""vdjx_tree_sankoff at size: per input and cost matrix (UNIT, TSTV) the best-of-three host time of the call after a warm-up,
the time of its kernels (HIP events, one more call), the info (rounds, moves, candidates, cost start -> end) and the scorer's node updates
("tree_sankoff_steps") against full rescoring -- exactly, from a call of one round, where every lineage's candidates are known: 2 (m - 3)
(m - 2) per column tile.  Beside it the two yardsticks: vdjx_tree_mp on the same inputs and vdjx_tree_spr on the 65,536 contigs.  All three
clocks start after the calls' argument checks and span the key sort, the layout, the start tree, all transfers and all kernels.
Copied into a checkout of the parent commit (no api.Context.tree_sankoff) the script times the yardsticks alone, and a second argument
merges that run's JSON in as *_parent_commit_ms.
   python profiles/tree_sankoff_at_size.py [out.json [parent.json]]     (profiles/tree_sankoff_at_size.json is a run on an MI355X)
The inputs are profiles/tree_spr_at_size.py's (profiles/tree_mp_at_size.py's draws, in its order from its seed):
     one_lineage      one lineage of 1,024 members with 486-base windows
     small_lineages   65,536 contigs of 486 bases in 1,938 lineages of 2 .. 64 members, interleaved
one_lineage is searched under the max_rounds that a first call of one round says fits ONE_LINEAGE_BUDGET_MS (at most 64; 0 -- until
finished -- if 64 fit); the value is in the row.  small_lineages runs until finished."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from tree_mp_at_size import family  # noqa: E402

KERNELS = ["k_sk_up", "k_sk_score", "k_sk_pick", "k_sk_down", "k_nj_matrix", "k_nj_join_lds", "k_nj_join_global"]
ONE_LINEAGE_BUDGET_MS = 3000.0
MP_INFO = ("searched", "moved", "rounds", "moves", "candidates", "parsimony_start", "parsimony", "batches")
SK_INFO = ("searched", "moved", "rounds", "moves", "candidates", "cost_start", "cost", "mutations", "batches")
MATRICES = {"UNIT": [[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]], "TSTV": [[0, 2, 1, 2], [2, 0, 2, 1], [1, 2, 0, 2], [2, 1, 2, 0]]}


def best_of_three(call, stat):
    times = []
    for _ in range(3):
        res = call()
        times.append(stat())
    return res, round(min(times) / 1e3, 3), [round(t / 1e3, 3) for t in times]


def leg(ctx, name, codes, clone, capped, out):
    text = [bytes(r).decode() for r in np.frombuffer(b"ACGT", np.uint8)[codes]]
    contigs = ctx.pack_strings(text)
    anchor = np.full(len(clone), 100, np.int32)
    sizes = np.bincount(clone)
    tiles = (codes.shape[1] + 63) // 64
    nj_res = ctx.tree_nj(contigs, clone, anchor)             # (warm-up: code objects, workspace)
    ctx.tree_mp(contigs, clone, anchor)
    mp_res, mp_ms, mp_all = best_of_three(lambda: ctx.tree_mp(contigs, clone, anchor), lambda: ctx.stat("tree_mp_us"))
    row = dict(leg=name, n=len(clone), lineages=len(sizes), window=int(codes.shape[1]), nj_parsimony=nj_res["info"]["parsimony"], tree_mp_ms=mp_ms,
               tree_mp_all_ms=mp_all, tree_mp={f: mp_res["info"][f] for f in MP_INFO})
    if not capped and hasattr(ctx, "tree_spr"):
        ctx.tree_spr(contigs, clone, anchor)
        spr_res, row["tree_spr_ms"], row["tree_spr_all_ms"] = best_of_three(lambda: ctx.tree_spr(contigs, clone, anchor), lambda: ctx.stat("tree_spr_us"))
        row["tree_spr"] = {f: spr_res["info"][f] for f in MP_INFO}
    if hasattr(ctx, "tree_sankoff"):                         # (the parent commit: the yardsticks alone)
        full_round = int(sum(2 * (m - 3) * (m - 2) for m in sizes if m > 3)) * tiles
        for label, cost in MATRICES.items():
            call = lambda **kw: ctx.tree_sankoff(contigs, clone, anchor, cost=np.array(cost, np.uint32), **kw)
            call(max_rounds=1)
            first = call(max_rounds=1)
            one_round, steps_one = ctx.stat("tree_sankoff_us") / 1e3, ctx.stat("tree_sankoff_steps")
            fit = int(ONE_LINEAGE_BUDGET_MS / one_round)
            max_rounds = (0 if fit >= 64 else max(1, fit)) if capped else 0
            res, ms, all_ms = best_of_three(lambda: call(max_rounds=max_rounds), lambda: ctx.stat("tree_sankoff_us"))
            steps = ctx.stat("tree_sankoff_steps")
            _, given_ms, _ = best_of_three(lambda: call(start=nj_res["parent"], max_rounds=max_rounds), lambda: ctx.stat("tree_sankoff_us"))
            ctx.profile(True)
            ctx.profile_reset()
            call(max_rounds=max_rounds)
            prof = ctx.profile_get()
            ctx.profile(False)
            if label == "UNIT":                              # the anchor: the interchange search's own tree
                mp_capped = ctx.tree_mp(contigs, clone, anchor, max_rounds=max_rounds)
                assert all(np.array_equal(res[f], mp_capped[f]) for f in ("parent", "depth", "clone")) and res["info"]["cost"] == mp_capped["info"]["parsimony"]
            row["tree_sankoff_" + label] = dict(
                max_rounds=max_rounds, one_round_ms=round(one_round, 3), ms=ms, all_ms=all_ms, given_start_ms=given_ms, over_tree_mp=round(ms / mp_ms, 2),
                info={f: res["info"][f] for f in SK_INFO}, steps=steps, first_round=dict(candidates=first["info"]["candidates"], steps=steps_one,
                                                                                            full_rescoring_steps=full_round,
                                                                                            steps_share=round(steps_one / full_round, 5)),
                steps_per_candidate_and_tile=round(steps / (res["info"]["candidates"] * tiles), 2),
                kernel_ms={k: round(prof.get(k, (0.0, 0))[0], 4) for k in KERNELS}, dispatches={k: prof[k][1] for k in KERNELS if k in prof})
    print(json.dumps(row), flush=True)
    out.append(row)


def main(path=None, parent_path=None):
    from vdjer_amd import api
    out = []
    ctx = api.Context(0)
    rng = np.random.default_rng(1024)                        # tree_mp_at_size.main's draws, in its order
    one = family(rng, rng.integers(0, 4, 486, dtype=np.uint8), 1024)
    leg(ctx, "one_lineage", one[rng.permutation(1024)], np.zeros(1024, np.int32), True, out)
    fams, key = [], []
    total = 0
    while total < 65536:
        m = min(int(rng.integers(2, 65)), 65536 - total)
        if 65536 - total - m == 1:
            m += 1 if m < 64 else -1
        fams.append(family(rng, rng.integers(0, 4, 486, dtype=np.uint8), m))
        key += [len(fams) - 1] * m
        total += m
    order = rng.permutation(total)
    leg(ctx, "small_lineages", np.concatenate(fams)[order], np.asarray(key, np.int32)[order], False, out)
    ctx.close()
    if parent_path:
        with open(parent_path) as fp:
            parent = {r["leg"]: r for r in json.load(fp)["legs"]}
        for row in out:
            p = parent[row["leg"]]
            assert (p["n"], p["window"], p["nj_parsimony"], p["tree_mp"]) == (row["n"], row["window"], row["nj_parsimony"], row["tree_mp"]), (p, row)
            for f in ("tree_mp_ms", "tree_mp_all_ms", "tree_spr_ms", "tree_spr_all_ms"):
                if f in p:
                    row[f.replace("_ms", "_parent_commit_ms")] = p[f]
    if path:
        with open(path, "w") as fp:
            json.dump(dict(legs=out), fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
