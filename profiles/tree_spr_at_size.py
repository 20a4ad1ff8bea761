"""vdjx_tree_spr at size: per input the best-of-three host time of the call after a warm-up -- from vdjx_tree_nj's tree (the
call then contains that function) and from given parents (the search alone) --, the time of its kernels (HIP events, one more call), the
info (rounds, moves, candidates, parsimony start -> end) -- and beside it vdjx_tree_mp on the same input, the yardstick.  Both clocks
("tree_spr_us", "tree_mp_us") start after the calls' argument checks and span the key sort, the layout, all transfers and all kernels.
Copied into a checkout of the parent commit (no api.Context.tree_spr) the script times vdjx_tree_mp alone on the same inputs, and a second
argument merges that run's JSON in as tree_mp_parent_commit_ms.
   python profiles/tree_spr_at_size.py [out.json [parent.json]]     (profiles/tree_spr_at_size.json is a run on an MI355X)
The inputs are profiles/tree_mp_at_size.py's, drawn in its order from its seed:
     one_lineage      one lineage of 1,024 members with 486-base windows
     small_lineages   65,536 contigs of 486 bases in lineages of 2 .. 64 members, interleaved
A round of one lineage of 1,024 scores about four million candidates by 2,044 walks of two thousand nodes over eight column tiles, and a
search from the neighbour-joining tree takes more rounds than vdjx_tree_mp's: one_lineage is searched under the max_rounds that a first
call of one round says fits ONE_LINEAGE_BUDGET_MS (at least 1, at most 64); the value is in the row.  small_lineages runs until finished."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from tree_mp_at_size import family  # noqa: E402

KERNELS = ["k_mp_up", "k_spr_score", "k_spr_score_slab", "k_spr_pick", "k_nj_fitch", "k_nj_matrix", "k_nj_join_lds", "k_nj_join_global"]
ONE_LINEAGE_BUDGET_MS = 4000.0
INFO = ("searched", "moved", "rounds", "moves", "candidates", "parsimony_start", "parsimony", "batches")


def leg(ctx, name, codes, clone, capped, out):
    text = [bytes(r).decode() for r in np.frombuffer(b"ACGT", np.uint8)[codes]]
    contigs = ctx.pack_strings(text)
    anchor = np.full(len(clone), 100, np.int32)
    nj_res = ctx.tree_nj(contigs, clone, anchor)             # (warm-up: code objects, workspace)
    ctx.tree_mp(contigs, clone, anchor)
    mp = []
    for _ in range(3):
        mp_res = ctx.tree_mp(contigs, clone, anchor)
        mp.append(ctx.stat("tree_mp_us"))
    row = dict(leg=name, n=len(clone), window=int(codes.shape[1]), nj_parsimony=nj_res["info"]["parsimony"], tree_mp_ms=round(min(mp) / 1e3, 3),
               tree_mp_all_ms=[round(c / 1e3, 3) for c in mp], tree_mp={f: mp_res["info"][f] for f in INFO})
    if hasattr(ctx, "tree_spr"):                             # (the parent commit: the yardstick alone)
        ctx.tree_spr(contigs, clone, anchor, max_rounds=1)
        one_round = ctx.stat("tree_spr_us") / 1e3
        max_rounds = max(1, min(64, int(ONE_LINEAGE_BUDGET_MS / one_round))) if capped else 0
        spr, given = [], []
        for _ in range(3):
            res = ctx.tree_spr(contigs, clone, anchor, max_rounds=max_rounds)
            spr.append(ctx.stat("tree_spr_us"))
            again = ctx.tree_spr(contigs, clone, anchor, start=nj_res["parent"], max_rounds=max_rounds)
            given.append(ctx.stat("tree_spr_us"))
            assert all(np.array_equal(res[f], again[f]) for f in ("parent", "mutations", "depth"))
        ctx.profile(True)
        ctx.profile_reset()
        ctx.tree_spr(contigs, clone, anchor, max_rounds=max_rounds)
        prof = ctx.profile_get()
        ctx.profile(False)
        row.update(max_rounds=max_rounds, one_round_ms=round(one_round, 3), tree_spr={f: res["info"][f] for f in INFO},
                   tree_spr_ms=round(min(spr) / 1e3, 3), tree_spr_all_ms=[round(c / 1e3, 3) for c in spr],
                   tree_spr_given_start_ms=round(min(given) / 1e3, 3),
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
            row["tree_mp_parent_commit_ms"] = p["tree_mp_ms"]
            row["tree_mp_parent_commit_all_ms"] = p["tree_mp_all_ms"]
    if path:
        with open(path, "w") as fp:
            json.dump(dict(legs=out), fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
