"""vdjx_tree_mp at size: per input the best-of-three host time of the call after a warm-up -- from vdjx_tree_nj's tree (the
call then contains that function) and from given parents (the search alone) --, the time of its kernels (HIP events, one more call), the
info, the counted share of node updates the scorer made of what full rescoring would make -- and beside it vdjx_tree_nj's time on the same
input, the yardstick.  Both clocks ("tree_mp_us", "tree_nj_us") start after the calls' argument checks and span the key sort, the layout,
all transfers and all kernels.  vdjx_tree_nj is timed between the calls of vdjx_tree_mp here; copied into a checkout of the parent commit
(no api.Context.tree_mp) the script times vdjx_tree_nj alone on the same inputs, three calls in a row, and a second argument merges that
run's JSON in as vdjx_tree_nj_parent_commit_ms.
   python profiles/tree_mp_at_size.py [out.json [parent.json]]     (profiles/tree_mp_at_size.json is a run on an MI355X)
     one_lineage      one lineage of 1,024 members with 486-base windows
     small_lineages   65,536 contigs of 486 bases in lineages of 2 .. 64 members, interleaved (profiles/tree_nj_at_size.py's sizes)
Both are non-additive, so that moves occur: a member differs from its founder at 4 .. 12 of 48 hot columns, the same columns for the
whole lineage.  Full rescoring makes candidates x (m - 2) node updates per column tile; for small_lineages that needs the candidates per
lineage size, which the info does not have: the lineages of every size go through a call of their own (lineages do not interact)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ["k_mp_up", "k_mp_score", "k_mp_pick", "k_nj_fitch", "k_nj_matrix", "k_nj_join_lds", "k_nj_join_global"]


def family(rng, founder, m, lo=4, hi=12, hot=48):
    cols = rng.choice(len(founder), size=hot, replace=False)
    fam = np.repeat(founder[None, :], m, axis=0)
    for r in range(1, m):
        pos = rng.choice(cols, size=int(rng.integers(lo, hi + 1)), replace=False)
        fam[r, pos] = (fam[r, pos] + rng.integers(1, 4, len(pos), dtype=np.uint8)) % 4
    return fam


def full_rescoring(ctx, contigs_of, clone, anchor, tiles):
    """-> (node updates full rescoring would make, the scorer's own count), summed over one call per lineage size"""
    sizes = np.bincount(clone)
    full = made = 0
    for m in sorted(set(sizes.tolist())):
        if m < 4:
            continue
        pick = np.flatnonzero(sizes[clone] == m)
        res = ctx.tree_mp(contigs_of(pick), clone[pick], anchor[pick], ancestors=False)
        full += res["info"]["candidates"] * (m - 2) * tiles
        made += ctx.stat("tree_mp_steps")
    return full, made


def leg(ctx, name, codes, clone, out):
    text = [bytes(r).decode() for r in np.frombuffer(b"ACGT", np.uint8)[codes]]
    contigs = ctx.pack_strings(text)
    anchor = np.full(len(clone), 100, np.int32)
    nj_res = ctx.tree_nj(contigs, clone, anchor)             # (warm-up: code objects, workspace)
    if not hasattr(ctx, "tree_mp"):                          # the parent commit: the yardstick alone
        nj = []
        for _ in range(3):
            ctx.tree_nj(contigs, clone, anchor)
            nj.append(ctx.stat("tree_nj_us"))
        row = dict(leg=name, n=len(clone), window=int(codes.shape[1]), vdjx_tree_nj_ms=round(min(nj) / 1e3, 3),
                   vdjx_tree_nj_all_ms=[round(c / 1e3, 3) for c in nj], nj_parsimony=nj_res["info"]["parsimony"])
        print(json.dumps(row), flush=True)
        out.append(row)
        return
    ctx.tree_mp(contigs, clone, anchor)
    mp, given, nj = [], [], []
    for _ in range(3):
        res = ctx.tree_mp(contigs, clone, anchor)
        mp.append(ctx.stat("tree_mp_us"))
        steps = ctx.stat("tree_mp_steps")
        again = ctx.tree_mp(contigs, clone, anchor, start=nj_res["parent"])
        given.append(ctx.stat("tree_mp_us"))
        assert all(np.array_equal(res[f], again[f]) for f in ("parent", "mutations", "depth"))
        ctx.tree_nj(contigs, clone, anchor)
        nj.append(ctx.stat("tree_nj_us"))
    ctx.profile(True)
    ctx.profile_reset()
    ctx.tree_mp(contigs, clone, anchor)
    prof = ctx.profile_get()
    ctx.profile(False)
    tiles = (codes.shape[1] + 63) // 64
    full, made = full_rescoring(ctx, lambda pick: ctx.pack_strings([text[i] for i in pick]), clone, anchor, tiles)
    assert made == steps, (made, steps)                      # (the work items of a lineage do not depend on the others)
    row = dict(leg=name, n=len(clone), window=int(codes.shape[1]), **res["info"], tree_mp_ms=round(min(mp) / 1e3, 3),
               tree_mp_all_ms=[round(c / 1e3, 3) for c in mp], tree_mp_given_start_ms=round(min(given) / 1e3, 3), vdjx_tree_nj_ms=round(min(nj) / 1e3, 3),
               vdjx_tree_nj_all_ms=[round(c / 1e3, 3) for c in nj], nj_parsimony=nj_res["info"]["parsimony"], tree_mp_steps=steps, full_rescoring_steps=full, steps_share=round(steps / max(full, 1), 5),
               kernel_ms={k: round(prof.get(k, (0.0, 0))[0], 4) for k in KERNELS}, dispatches={k: prof[k][1] for k in KERNELS if k in prof})
    print(json.dumps(row), flush=True)
    out.append(row)


def main(path, parent_path=None):
    from vdjer_amd import api
    out = []
    ctx = api.Context(0)
    rng = np.random.default_rng(1024)
    one = family(rng, rng.integers(0, 4, 486, dtype=np.uint8), 1024)
    leg(ctx, "one_lineage", one[rng.permutation(1024)], np.zeros(1024, np.int32), out)
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
    leg(ctx, "small_lineages", np.concatenate(fams)[order], np.asarray(key, np.int32)[order], out)
    ctx.close()
    if parent_path:
        with open(parent_path) as fp:
            parent = {r["leg"]: r for r in json.load(fp)["legs"]}
        for row in out:
            p = parent[row["leg"]]
            assert (p["n"], p["window"], p["nj_parsimony"]) == (row["n"], row["window"], row["nj_parsimony"]), (p, row)   # the same input
            row["vdjx_tree_nj_parent_commit_ms"] = p["vdjx_tree_nj_ms"]
            row["vdjx_tree_nj_parent_commit_all_ms"] = p["vdjx_tree_nj_all_ms"]
    if path:
        with open(path, "w") as fp:
            json.dump(dict(legs=out), fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
