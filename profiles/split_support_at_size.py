"""vdjx_tree_split_support at size, run by hand on an MI355X: on the 65,536 contigs in 1,938 lineages of
profiles/tree_mp_at_size.py's small_lineages leg (the same generator and seed), after a warm-up,
   split_support_ms     the best of three calls of Context.tree_split_support with 100 replicates ("tree_split_us": from after the
                        argument checks, the layout, the scored tree's check, all transfers and all kernels), the scored tree vdjx_tree_nj's
   nj_parents_100_ms    100 calls of vdjx_nj_parents -- vdjx_tree_nj's own steps as far as the rooted parents, the code of the parent commit,
                        untouched by the call under test -- on contigs cut to the columns one jackknife keeps, timed with the host clock
                        around the 100 calls, best of three.  Every call is the SAME jackknife (replicate 1 of seed 1): the 100 replicates
                        keep different columns but as many of them on average, and one cut input spares 100 host-side cuts that are not
                        what is measured.  The function is internal (no C linkage): it is looked up under its C++ name.
and the kernels' times of one more call (HIP events), with the info.
   python profiles/split_support_at_size.py [out.json]     (profiles/split_support_at_size.json is a run on an MI355X)
The batched call has no upload per replicate, no Fitch pass and reads nothing back: it is expected to be the cheaper one.  Whatever the
run says is recorded as it is."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.tree_mp_at_size import family  # noqa: E402

KERNELS = ["k_split_pack", "k_nj_matrix", "k_nj_join_lds", "k_nj_join_global", "k_split_clades", "k_split_match"]
NJ_PARENTS = "_Z15vdjx_nj_parentsP8vdjx_ctxPKcmiPKiS4_PKjPi"      # int vdjx_nj_parents(vdjx_ctx*, const char*, size_t, int, const int32_t*, const int32_t*, const uint32_t*, int32_t*)
B, SEED, ANCHOR = 100, 1, 100


def small_lineages():
    """profiles/tree_mp_at_size.py's second leg: the generator is walked as its main() walks it"""
    rng = np.random.default_rng(1024)
    family(rng, rng.integers(0, 4, 486, dtype=np.uint8), 1024)
    rng.permutation(1024)
    fams, key, total = [], [], 0
    while total < 65536:
        m = min(int(rng.integers(2, 65)), 65536 - total)
        if 65536 - total - m == 1:
            m += 1 if m < 64 else -1
        fams.append(family(rng, rng.integers(0, 4, 486, dtype=np.uint8), m))
        key += [len(fams) - 1] * m
        total += m
    order = rng.permutation(total)
    return np.concatenate(fams)[order], np.asarray(key, np.int32)[order]


def main(path=None):
    from vdjer_amd import annot, api
    ctx = api.Context(0)
    codes, clone = small_lineages()
    letters = np.frombuffer(b"ACGT", np.uint8)
    text = [bytes(r).decode() for r in letters[codes]]
    contigs = ctx.pack_strings(text)
    anchor = np.full(len(clone), ANCHOR, np.int32)
    nj = ctx.tree_nj(contigs, clone, anchor, ancestors=False)
    res = ctx.tree_split_support(contigs, clone, anchor, nj["parent"], replicates=B, seed=SEED)      # (warm-up: code objects, workspace)
    split = []
    for _ in range(3):
        again = ctx.tree_split_support(contigs, clone, anchor, nj["parent"], replicates=B, seed=SEED)
        split.append(ctx.stat("tree_split_us"))
        assert again["support"].tobytes() == res["support"].tobytes()
    ctx.profile(True)
    ctx.profile_reset()
    ctx.tree_split_support(contigs, clone, anchor, nj["parent"], replicates=B, seed=SEED)
    prof = ctx.profile_get()
    ctx.profile(False)
    # the yardstick: every contig is its own window here (one anchor, one length), so a window position is a contig position
    keep = annot.jackknife_keep(SEED, 1, codes.shape[1])
    cut = np.ascontiguousarray(letters[codes[:, keep]])
    cut_anchor = np.full(len(clone), int(keep[:ANCHOR].sum()), np.int32)
    fn = getattr(ctx.L, NJ_PARENTS)
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int] + [C.c_void_p] * 4
    fn.restype = C.c_int
    out = np.zeros(len(nj["parent"]), np.int32)
    raw = cut.tobytes()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda: fn(ctx.h, raw, len(clone), cut.shape[1], ptr(clone), ptr(cut_anchor), None, ptr(out))
    assert call() == 0
    first = ctx.tree_split_support(contigs, clone, anchor, nj["parent"], replicates=1, seed=SEED, return_trees=True)
    assert np.array_equal(first["trees"][0], out)            # the yardstick joins what replicate 1 joins
    loops = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(B):
            assert call() == 0
        loops.append((time.perf_counter() - t0) * 1e3)
    row = dict(n=len(clone), window=int(codes.shape[1]), kept_columns=int(keep.sum()), **res["info"], split_support_ms=round(min(split) / 1e3, 3),
               split_support_all_ms=[round(c / 1e3, 3) for c in split], nj_parents_100_ms=round(min(loops), 3), nj_parents_100_all_ms=[round(c, 3) for c in loops],
               kernel_ms={k: round(prof.get(k, (0.0, 0))[0], 4) for k in KERNELS}, dispatches={k: prof[k][1] for k in KERNELS if k in prof})
    print(json.dumps(row), flush=True)
    ctx.close()
    if path:
        with open(path, "w") as fp:
            json.dump(row, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:2])
