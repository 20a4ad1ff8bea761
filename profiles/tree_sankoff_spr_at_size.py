"""vdjx_tree_sankoff_spr at size: per input and cost matrix (UNIT, TSTV) the best-of-three host time of the call after a
warm-up, the time of its kernels (HIP events, one more call) with k_sksp_score's time per round, and the info (rounds, moves, candidates,
cost start -> end).  Beside it the two yardsticks on the same inputs: vdjx_tree_spr (under UNIT the candidates are equal, so the ratio to
it is the price of the 16-byte messages and the 4 x 4 min-plus steps per candidate) and vdjx_tree_sankoff.  All clocks start after the
calls' argument checks and span the key sort, the layout, the start tree, all transfers and all kernels.
Copied into a checkout of the parent commit (no api.Context.tree_sankoff_spr) the script times the yardsticks alone, and a second argument
merges that run's JSON in as *_parent_commit_ms.
   python profiles/tree_sankoff_spr_at_size.py [out.json [parent.json]]     (profiles/tree_sankoff_spr_at_size.json is a run on an MI355X)
The inputs are profiles/tree_spr_at_size.py's (profiles/tree_mp_at_size.py's draws, in its order from its seed):
     one_lineage      one lineage of 1,024 members with 486-base windows
     small_lineages   65,536 contigs of 486 bases in 1,938 lineages of 2 .. 64 members, interleaved
one_lineage is searched under profiles/tree_spr_at_size.py's budget rule: the max_rounds that a first call of one round says fits
ONE_LINEAGE_BUDGET_MS (at most 64; 0 -- until finished -- if 64 fit); the value is in the row, one per call.  small_lineages runs until
finished."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from tree_mp_at_size import family  # noqa: E402

KERNELS = ["k_sk_up", "k_sksp_score", "k_sksp_score_slab", "k_sksp_pick", "k_sk_down", "k_nj_matrix", "k_nj_join_lds", "k_nj_join_global"]
ONE_LINEAGE_BUDGET_MS = 4000.0
MP_INFO = ("searched", "moved", "rounds", "moves", "candidates", "parsimony_start", "parsimony", "batches")
SK_INFO = ("searched", "moved", "rounds", "moves", "candidates", "cost_start", "cost", "mutations", "batches")
MATRICES = {"UNIT": [[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]], "TSTV": [[0, 2, 1, 2], [2, 0, 2, 1], [1, 2, 0, 2], [2, 1, 2, 0]]}


def best_of_three(call, stat):
    times = []
    for _ in range(3):
        res = call()
        times.append(stat())
    return res, round(min(times) / 1e3, 3), [round(t / 1e3, 3) for t in times]


def budget(one_round_ms, capped):
    fit = int(ONE_LINEAGE_BUDGET_MS / one_round_ms)
    return (0 if fit >= 64 else max(1, fit)) if capped else 0


def leg(ctx, name, codes, clone, capped, out):
    text = [bytes(r).decode() for r in np.frombuffer(b"ACGT", np.uint8)[codes]]
    contigs = ctx.pack_strings(text)
    anchor = np.full(len(clone), 100, np.int32)
    sizes = np.bincount(clone)
    nj_res = ctx.tree_nj(contigs, clone, anchor)             # (warm-up: code objects, workspace)
    row = dict(leg=name, n=len(clone), lineages=len(sizes), window=int(codes.shape[1]), nj_parsimony=nj_res["info"]["parsimony"])
    # the yardsticks: vdjx_tree_spr under its own budget rule, vdjx_tree_sankoff under UNIT and TSTV until finished
    ctx.tree_spr(contigs, clone, anchor, max_rounds=1)
    ctx.tree_spr(contigs, clone, anchor, max_rounds=1)
    spr_rounds = budget(ctx.stat("tree_spr_us") / 1e3, capped)
    spr_res, row["tree_spr_ms"], row["tree_spr_all_ms"] = best_of_three(lambda: ctx.tree_spr(contigs, clone, anchor, max_rounds=spr_rounds),
                                                                        lambda: ctx.stat("tree_spr_us"))
    row["tree_spr"] = dict({f: spr_res["info"][f] for f in MP_INFO}, max_rounds=spr_rounds)
    for label, cost in MATRICES.items():
        nni = lambda: ctx.tree_sankoff(contigs, clone, anchor, cost=np.array(cost, np.uint32))
        nni()
        res, ms, all_ms = best_of_three(nni, lambda: ctx.stat("tree_sankoff_us"))
        row["tree_sankoff_" + label] = dict(ms=ms, all_ms=all_ms, info={f: res["info"][f] for f in SK_INFO})
    if hasattr(ctx, "tree_sankoff_spr"):                     # (the parent commit: the yardsticks alone)
        for label, cost in MATRICES.items():
            call = lambda **kw: ctx.tree_sankoff_spr(contigs, clone, anchor, cost=np.array(cost, np.uint32), **kw)
            call(max_rounds=1)
            call(max_rounds=1)
            one_round = ctx.stat("tree_sankoff_spr_us") / 1e3
            max_rounds = budget(one_round, capped)
            res, ms, all_ms = best_of_three(lambda: call(max_rounds=max_rounds), lambda: ctx.stat("tree_sankoff_spr_us"))
            _, given_ms, _ = best_of_three(lambda: call(start=nj_res["parent"], max_rounds=max_rounds), lambda: ctx.stat("tree_sankoff_spr_us"))
            ctx.profile(True)
            ctx.profile_reset()
            call(max_rounds=max_rounds)
            prof = ctx.profile_get()
            ctx.profile(False)
            score_ms = sum(prof.get(k, (0.0, 0))[0] for k in ("k_sksp_score", "k_sksp_score_slab"))
            entry = dict(max_rounds=max_rounds, one_round_ms=round(one_round, 3), ms=ms, all_ms=all_ms, given_start_ms=given_ms,
                         info={f: res["info"][f] for f in SK_INFO}, score_ms_per_round=round(score_ms / max(1, res["info"]["rounds"]), 4),
                         kernel_ms={k: round(prof.get(k, (0.0, 0))[0], 4) for k in KERNELS}, dispatches={k: prof[k][1] for k in KERNELS if k in prof})
            if label == "UNIT":                              # the anchor: vdjx_tree_spr's own search under the same cap
                same = ctx.tree_spr(contigs, clone, anchor, max_rounds=max_rounds)
                same_ms = ctx.stat("tree_spr_us") / 1e3
                assert all(np.array_equal(res[f], same[f]) for f in ("parent", "depth", "clone")) and res["info"]["cost"] == same["info"]["parsimony"]
                assert res["info"]["candidates"] == same["info"]["candidates"]
                entry["tree_spr_same_cap_ms"] = round(same_ms, 3)
                entry["over_tree_spr"] = round(ms / same_ms, 2)
            row["tree_sankoff_spr_" + label] = entry
    print(json.dumps(row), flush=True)
    out.append(row)


def merge(out, parent_path):
    """the parent commit's yardsticks into the rows.  one_lineage's max_rounds for vdjx_tree_spr comes from a clock (the budget rule), so
    the two runs may differ by a round there: the parent's cap is kept beside its time"""
    with open(parent_path) as fp:
        parent = {r["leg"]: r for r in json.load(fp)["legs"]}
    for row in out:
        p = parent[row["leg"]]
        assert (p["n"], p["window"], p["nj_parsimony"]) == (row["n"], row["window"], row["nj_parsimony"]), (p, row)
        row["tree_spr_parent_commit_ms"], row["tree_spr_all_parent_commit_ms"] = p["tree_spr_ms"], p["tree_spr_all_ms"]
        row["tree_spr_parent_commit_max_rounds"] = p["tree_spr"]["max_rounds"]
        for label in MATRICES:
            assert p["tree_sankoff_" + label]["info"] == row["tree_sankoff_" + label]["info"], (p, row)
            row["tree_sankoff_" + label]["parent_commit_ms"] = p["tree_sankoff_" + label]["ms"]
            row["tree_sankoff_" + label]["all_parent_commit_ms"] = p["tree_sankoff_" + label]["all_ms"]


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
        merge(out, parent_path)
    if path:
        with open(path, "w") as fp:
            json.dump(dict(legs=out), fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
