"""The model of vdjx_tree_support (include/vdjx.h) in plain Python on top of tests/tree_model.py: the keep rule, every replicate's distances
over the kept window positions alone, Kruskal over the sorted (d, min, max) keys, the count of the replicates whose tree has the edge to the
scored parent, the info -- and the rows of `vdjer --trees --tree-support` with its stderr line, to predict the command line's bytes.
Nothing here is shared with the device code or with vdjer_main.c."""
import numpy as np

from tests import tree_model as T

M64 = (1 << 64) - 1
CHECK = 0xE220A8397B1DCDAF                                  # mix64(0)
ROWS = (1 << 20) - 1                                        # rows of a batch: VDJX_TREE_SUPPORT_ROWS' default
COLUMNS = T.COLUMNS + ["support"]
FIELDS = ["members", "clones", "largest_clone", "replicates", "batches", "rounds", "edges", "matched", "full"]


def mix64(x):
    """splitmix64's output step, in 64-bit wrap-around arithmetic"""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def keeps(seed, r, q):
    """replicate r (1 .. B) keeps window position q"""
    return (mix64(seed ^ ((r << 32) | (q >> 5))) >> (q & 31)) & 1 == 1


def keep(seed, r, w):
    return [keeps(seed, r, q) for q in range(w)]


def replicate_edges(ws, members, seed, r):
    """the replicate's tree of one clone: the undirected edges as a set of (i, j), i < j caller's indices"""
    at = [q for q in range(len(ws[0])) if keeps(seed, r, q)]
    sub = ["".join(s[q] for q in at) for s in ws]
    D = T.distance_matrix(sub) if at else np.zeros((len(ws), len(ws)), np.int32)
    return {(i, j) for i, j, _ in T.kruskal(members, D)}


def support(contigs, clone, anchor, parent, replicates, seed, rows=ROWS):
    """-> (support int32[n], info dict)"""
    n = len(contigs)
    assert 1 <= replicates <= 1024 and 0 <= seed <= M64 and 1 <= rows <= ROWS
    cs = [c.decode("latin-1") if isinstance(c, (bytes, bytearray)) else c for c in contigs]
    out = np.full(n, -1, np.int32)
    if n == 0:                                              # (returns at once with a zeroed info)
        return out, dict.fromkeys(FIELDS, 0)
    groups = T.members_of(clone)
    for i in range(n):
        p = int(parent[i])
        assert -1 <= p < n and p != i
        if p >= 0:
            assert int(clone[i]) >= 0 and int(clone[p]) == int(clone[i])
            out[i] = 0
    in_trees = 0                                            # members of the clones of two and more: the rows of a replicate
    for members in groups.values():
        ws, _ = T.windows(cs, members, anchor)
        if len(members) < 2:
            continue
        in_trees += len(members)
        for r in range(1, replicates + 1):
            edges = replicate_edges(ws, members, seed, r)
            for i in members:
                p = int(parent[i])
                if p >= 0 and (min(i, p), max(i, p)) in edges:
                    out[i] += 1
    largest = max([len(v) for v in groups.values()] or [0])
    scored = out[out >= 0]
    per_batch = max(1, rows // in_trees) if in_trees else 0
    info = dict(members=sum(len(v) for v in groups.values()), clones=len(groups), largest_clone=largest, replicates=replicates,
                batches=-(-replicates // per_batch) if in_trees else 0, rounds=(largest - 1).bit_length() if largest > 1 else 0,
                edges=int(len(scored)), matched=int(scored.sum()), full=int((scored == replicates).sum()))
    return out, info


def table_rows(ids, contigs, clone, anchor, prio, parent, dist, depth, sup, replicates):
    """the rows of `vdjer --trees --tree-support` (lists of strings, COLUMNS): the plain rows and support / B, empty where there is no parent"""
    rows = T.table_rows(ids, contigs, clone, anchor, prio, parent, dist, depth)
    return [row + ["%.4f" % (int(sup[c]) / replicates) if parent[c] >= 0 else ""] for c, row in enumerate(rows)]


def table_text(rows):
    return "".join("\t".join(r) + "\n" for r in [COLUMNS] + rows)


def summary_line(info, seed):
    return (f"tree support: {info['replicates']} replicates (seed {seed}), {info['edges']} edges, {info['matched']} of "
            f"{info['edges'] * info['replicates']} kept, {info['full']} in every replicate, {info['batches']} batches")
