"""vdjx_tree_nj at size: per input the best-of-three host time of the call after a warm-up, the time of the matrix, join and
Fitch kernels (HIP events, one more call), the info -- and beside it vdjx_tree's time on the same input, the yardstick.
   python profiles/tree_nj_at_size.py [out.json]       (profiles/tree_nj_at_size.json is a run on an MI355X)
     one_lineage      one lineage of 4,096 members with 486-base windows (a founder, 1 .. 5 substitutions a member): ONE workgroup of
                      k_nj_join on the matrix in global memory, m^3 / 6 = 1.1e10 evaluations of Q
     small_lineages   65,536 contigs of 486 bases in lineages of 2 .. 64 members, interleaved: the LDS path, a workgroup per lineage"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ["k_nj_pack", "k_nj_matrix", "k_nj_join_lds", "k_nj_join_global", "k_nj_fitch"]


def family(rng, founder, m, lo, hi):
    fam = np.repeat(founder[None, :], m, axis=0)
    for r in range(1, m):
        pos = rng.choice(fam.shape[1], size=int(rng.integers(lo, hi + 1)), replace=False)
        fam[r, pos] = (fam[r, pos] + rng.integers(1, 4, len(pos), dtype=np.uint8)) % 4
    return fam


def leg(ctx, name, codes, clone, out):
    contigs = ctx.pack_strings([bytes(r).decode() for r in np.frombuffer(b"ACGT", np.uint8)[codes]])
    anchor = np.full(len(clone), 100, np.int32)
    ctx.tree_nj(contigs, clone, anchor)                      # (warm-up: code objects, workspace)
    ctx.tree(contigs, clone, anchor)
    nj, mst = [], []
    for _ in range(3):
        res = ctx.tree_nj(contigs, clone, anchor)
        nj.append(ctx.stat("tree_nj_us"))
        ctx.tree(contigs, clone, anchor)
        mst.append(ctx.stat("tree_us"))
    bare = []
    for _ in range(3):
        ctx.tree_nj(contigs, clone, anchor, ancestors=False)
        bare.append(ctx.stat("tree_nj_us"))
    ctx.profile(True)
    ctx.profile_reset()
    ctx.tree_nj(contigs, clone, anchor)
    prof = ctx.profile_get()
    ctx.profile(False)
    row = dict(leg=name, n=len(clone), window=int(codes.shape[1]), **res["info"], tree_nj_ms=round(min(nj) / 1e3, 3),
               tree_nj_all_ms=[round(c / 1e3, 3) for c in nj], tree_nj_no_ancestors_ms=round(min(bare) / 1e3, 3), vdjx_tree_ms=round(min(mst) / 1e3, 3),
               kernel_ms={k: round(prof.get(k, (0.0, 0))[0], 4) for k in KERNELS}, dispatches={k: prof[k][1] for k in KERNELS if k in prof})
    print(json.dumps(row), flush=True)
    out.append(row)


def main(path):
    from vdjer_amd import api
    out = []
    ctx = api.Context(0)
    rng = np.random.default_rng(4096)
    one = family(rng, rng.integers(0, 4, 486, dtype=np.uint8), 4096, 1, 5)
    leg(ctx, "one_lineage", one[rng.permutation(4096)], np.zeros(4096, np.int32), out)
    fams, key = [], []
    total = 0
    while total < 65536:
        m = min(int(rng.integers(2, 65)), 65536 - total)
        if 65536 - total - m == 1:
            m += 1 if m < 64 else -1
        fams.append(family(rng, rng.integers(0, 4, 486, dtype=np.uint8), m, 1, 5))
        key += [len(fams) - 1] * m
        total += m
    order = rng.permutation(total)
    leg(ctx, "small_lineages", np.concatenate(fams)[order], np.asarray(key, np.int32)[order], out)
    ctx.close()
    if path:
        with open(path, "w") as fp:
            json.dump(dict(legs=out), fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
