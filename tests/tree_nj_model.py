"""The model of vdjx_tree_nj (include/vdjx.h) in plain Python: neighbour joining in 16.16 fixed point over each lineage's window distances,
the tree rooted at the member of smallest (prio, index), the inferred nodes' sequences by Fitch parsimony column by column, the info -- and
the rows of `vdjer --trees-nj`, the lines of `--trees-newick` and the stderr line, to predict the command line's bytes.  The items, windows
and distance are tests/tree_model.py's; nothing here is shared with the device code or with vdjer_main.c.

The distance and the parsimony treat a character that is not one of ACGT differently: in the distance it never matches (not even itself),
in Fitch's passes it is a wildcard (all four bases), so that an N costs branch length but never a mutation."""
import numpy as np

from tests.tree_model import distance_matrix, members_of, windows

BASES = "ACGT"                                              # the base order: A < C < G < T, bit k of a set is BASES[k]
SHIFT = 16
MAX_MEMBERS = 4096
COLUMNS = ["clone_id", "node_id", "parent_id", "branch_length", "mutations", "depth", "children", "observed", "sequence"]
FIELDS = ["members", "clones", "largest_clone", "internal", "batches", "negative", "edges", "joins", "cells", "parsimony", "length"]


def nj_edges(D):
    """D: m x m of Python ints (already << 16) -> the 2m - 3 edges (child id, parent-side id, length) in creation order; leaves are
    0 .. m - 1, inferred nodes m, m + 1, ... as they are made.  Python's // floors toward minus infinity."""
    m = len(D)
    if m < 2:
        return []
    if m == 2:
        return [(0, 1, int(D[0][1]))]
    if m > PLAIN_MEMBERS:
        return nj_edges_numpy(D)
    d = {(i, j): int(D[i][j]) for i in range(m) for j in range(m) if i != j}
    active = list(range(m))
    edges = []
    nxt = m
    while len(active) > 3:
        r = len(active)
        R = {i: sum(d[i, k] for k in active if k != i) for i in active}
        best = None
        for x, i in enumerate(active):
            for j in active[x + 1:]:
                key = ((r - 2) * d[i, j] - R[i] - R[j], i, j)
                if best is None or key < best:
                    best = key
        _, i, j = best
        u, nxt = nxt, nxt + 1
        bi = ((r - 2) * d[i, j] + R[i] - R[j]) // (2 * (r - 2))
        edges += [(i, u, bi), (j, u, d[i, j] - bi)]
        for k in active:
            if k != i and k != j:
                d[u, k] = d[k, u] = (d[i, k] + d[j, k] - d[i, j]) // 2
        active = [k for k in active if k != i and k != j] + [u]      # (ids ascend: u is the largest)
    x, y, z = active
    bx = (d[x, y] + d[x, z] - d[y, z]) // 2
    return edges + [(x, nxt, bx), (y, nxt, d[x, y] - bx), (z, nxt, d[x, z] - bx)]


PLAIN_MEMBERS = 24                                          # larger lineages: the same steps on int64 arrays (test_tree_nj_cpu.py compares the two)


def nj_edges_numpy(D):
    """nj_edges for m > 3 with the active nodes' matrix in a numpy int64 array.  The active ids ascend, so the first smallest Q of the
    upper triangle in row-major order is the smallest (Q, i, j).  Every value is checked to stay far inside 64 bits."""
    m = len(D)
    d = np.array(D, np.int64)
    np.fill_diagonal(d, 0)                                  # (d(i, i) counts i's non-ACGT characters: it is never used)
    ids = list(range(m))
    edges = []
    nxt = m
    big = np.iinfo(np.int64).max
    while len(ids) > 3:
        r = len(ids)
        assert int(np.abs(d).max()) * (r + 2) < 1 << 61
        R = d.sum(1)                                        # (the diagonal is 0)
        Q = (r - 2) * d - R[:, None] - R[None, :]
        Q[np.tril_indices(r)] = big
        a, b = divmod(int(Q.argmin()), r)
        i, j, dij = ids[a], ids[b], int(d[a, b])
        u, nxt = nxt, nxt + 1
        bi = ((r - 2) * dij + int(R[a]) - int(R[b])) // (2 * (r - 2))
        edges += [(i, u, bi), (j, u, dij - bi)]
        keep = [x for x in range(r) if x != a and x != b]
        du = (d[a, keep] + d[b, keep] - dij) // 2           # (numpy's // floors, as Python's)
        nd = np.zeros((r - 1, r - 1), np.int64)
        nd[:-1, :-1] = d[np.ix_(keep, keep)]
        nd[-1, :-1] = nd[:-1, -1] = du
        d = nd
        ids = [ids[x] for x in keep] + [u]
    x, y, z = ids
    dxy, dxz, dyz = int(d[0, 1]), int(d[0, 2]), int(d[1, 2])
    bx = (dxy + dxz - dyz) // 2
    return edges + [(x, nxt, bx), (y, nxt, dxy - bx), (z, nxt, dxz - bx)]


def orient(m, edges, root):
    """-> (parent, length, depth, children) over the 2m - 2 (m = 1: 1) nodes, rooted at leaf `root`; children ascend"""
    nodes = m + max(0, m - 2)
    near = [[] for _ in range(nodes)]
    for a, b, ln in edges:
        near[a].append((b, ln))
        near[b].append((a, ln))
    parent, length, depth = [-1] * nodes, [0] * nodes, [-1] * nodes
    kids = [[] for _ in range(nodes)]
    depth[root] = 0
    stack = [root]
    while stack:
        v = stack.pop()
        for c, ln in near[v]:
            if depth[c] < 0:
                parent[c], length[c], depth[c] = v, ln, depth[v] + 1
                kids[v].append(c)
                stack.append(c)
    assert all(x >= 0 for x in depth)
    for v in range(nodes):
        kids[v].sort()
        assert len(kids[v]) == (2 if v >= m else (1 if v == root and m > 1 else 0))
    return parent, length, depth, kids


def leaf_set(ch):
    return 1 << BASES.index(ch) if ch in BASES else 15


def lowest(s):
    return (s & -s).bit_length() - 1


def fitch(ws, m, root, parent, kids):
    """-> (states: per node a list of w base codes, mutations: per node, -1 for the root)"""
    nodes, w = len(parent), len(ws[0])
    state = [[0] * w for _ in range(nodes)]
    mut = [0] * nodes
    mut[root] = -1
    order = []                                              # parents before children
    stack = [root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(kids[v])
    for q in range(w):
        s = [leaf_set(ws[v][q]) if v < m else 0 for v in range(nodes)]
        for v in reversed(order):
            if v >= m:
                a, b = s[kids[v][0]], s[kids[v][1]]
                s[v] = a & b or a | b
        for v in order:
            if v == root:
                top = s[v] & s[kids[v][0]] if kids[v] else s[v]
                state[v][q] = lowest(top or s[v])
            else:
                p = state[parent[v]][q]
                state[v][q] = p if s[v] >> p & 1 else lowest(s[v])
                mut[v] += state[v][q] != p
    return state, mut


def tree_nj(contigs, clone, anchor, prio=None, ancestors=True, cells_knob=1 << 26):
    """-> {"parent", "length", "mutations", "depth", "clone": arrays[nodes], "anc": list[str] | None, "info": dict}: Context.tree_nj's"""
    n = len(contigs)
    cs = [c.decode("latin-1") if isinstance(c, (bytes, bytearray)) else c for c in contigs]
    groups = members_of(clone)
    for members in groups.values():
        assert len(members) <= MAX_MEMBERS
    nodes = n + sum(max(0, len(v) - 2) for v in groups.values())
    parent, depth, mutations = np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32)
    length, out_clone = np.full(nodes, -1, np.int64), np.full(nodes, -1, np.int32)
    anc = []
    info = dict.fromkeys(FIELDS, 0)
    slot0 = n
    batch_cells, sizes = 0, []
    for key in sorted(groups):
        members = groups[key]
        m = len(members)
        ws, _ = windows(cs, members, anchor)
        edges = nj_edges([[int(x) << SHIFT for x in row] for row in distance_matrix(ws)]) if m > 1 else []
        root = min(range(m), key=lambda p: (int(prio[members[p]]) if prio is not None else 0, members[p]))
        par, ln, dep, kids = orient(m, edges, root)
        state, mut = fitch(ws, m, root, par, kids)
        slot = lambda v: members[v] if v < m else slot0 + v - m
        for v in range(len(par)):
            s = slot(v)
            out_clone[s], depth[s], mutations[s] = key, dep[v], mut[v]
            parent[s] = slot(par[v]) if par[v] >= 0 else -1
            length[s] = ln[v]
            if v != root:
                info["parsimony"] += mut[v]
                info["length"] += ln[v]
                info["negative"] += ln[v] < 0
            if v >= m:
                anc.append("".join(BASES[x] for x in state[v]))
        slot0 += max(0, m - 2)
        info["edges"] += len(edges)
        info["joins"] += max(0, m - 3)
        info["internal"] += max(0, m - 2)
        if m > 1:
            info["cells"] += m * m
            sizes.append(m * m)
    for c in sizes:                                         # whole lineages while the cells fit; one with more than the knob goes alone
        if batch_cells and batch_cells + c > cells_knob:
            info["batches"] += 1
            batch_cells = 0
        batch_cells += c
    info["batches"] += batch_cells > 0
    info["members"] = sum(len(v) for v in groups.values())
    info["clones"] = len(groups)
    info["largest_clone"] = max([len(v) for v in groups.values()] or [0])
    return {"parent": parent, "length": length, "mutations": mutations, "depth": depth, "clone": out_clone,
            "anc": anc if ancestors else None, "info": info}


def nodes_of(clone):
    return len(clone) + sum(max(0, len(v) - 2) for v in members_of(clone).values())


def node_ids(ids, clone):
    """the node_id of every slot: a member's sequence_id, lin_<k>_a<j> (j from 1) for the inferred nodes; clone: 0-based lineage numbers"""
    out = list(ids)
    groups = members_of(clone)
    for k in sorted(groups):
        out += [f"lin_{k + 1}_a{j + 1}" for j in range(max(0, len(groups[k]) - 2))]
    return out


def fmt_length(x):
    return "%.4f" % (int(x) / 65536)


def table_rows(ids, contigs, clone, anchor, res):
    """the rows of `vdjer --trees-nj` (lists of strings, COLUMNS); clone: the 0-based lineage of every contig, -1 for none"""
    n = len(ids)
    names = node_ids(ids, clone)
    parent, nodes = res["parent"], len(res["parent"])
    kids = [0] * nodes
    for s in range(nodes):
        if parent[s] >= 0:
            kids[int(parent[s])] += 1
    groups = members_of(clone)
    rows, slot0 = [], n
    for k in sorted(groups):
        members = groups[k]
        ws, _ = windows(contigs, members, anchor)
        extra = max(0, len(members) - 2)
        seqs = ws + res["anc"][slot0 - n:slot0 - n + extra]
        for s, seq in zip(members + list(range(slot0, slot0 + extra)), seqs):
            root = parent[s] < 0
            rows.append([f"lin_{k + 1}", names[s], "" if root else names[int(parent[s])], fmt_length(res["length"][s]),
                         "" if root else str(int(res["mutations"][s])), str(int(res["depth"][s])), str(kids[s]), "T" if s < n else "F", seq])
        slot0 += extra
    return rows


def table_text(rows):
    return "".join("\t".join(r) + "\n" for r in [COLUMNS] + rows)


def newick(names, clone, parent, length):
    """one string per lineage of two and more members, in ascending clone key: (<the root's one subtree>)'<root id>'; -- children in
    ascending node id (slot), every node labelled and single-quoted, 'label':%.4f"""
    nodes = len(parent)
    kids = [[] for _ in range(nodes)]
    roots = {}
    for s in range(nodes):
        if parent[s] >= 0:
            kids[int(parent[s])].append(s)
        elif clone[s] >= 0:
            roots[int(clone[s])] = s

    def sub(s):
        inner = "(" + ",".join(sub(c) for c in kids[s]) + ")" if kids[s] else ""
        return f"{inner}'{names[s]}':{fmt_length(length[s])}"

    out = []
    for k in sorted(roots):
        r = roots[k]
        if kids[r]:
            out.append("(" + ",".join(sub(c) for c in kids[r]) + f")'{names[r]}';")
    return out


def newick_text(ids, clone, res):
    """the file of `vdjer --trees-newick`: lin_<k>, a tab, the tree"""
    names = node_ids(ids, clone)
    keys = sorted(k for k, v in members_of(clone).items() if len(v) > 1)
    lines = newick(names, res["clone"], res["parent"], res["length"])
    assert len(keys) == len(lines)
    return "".join(f"lin_{k + 1}\t{t}\n" for k, t in zip(keys, lines))


def summary_line(info):
    return (f"trees nj: {info['members']} contigs in {info['clones']} lineages (largest {info['largest_clone']}), {info['internal']} inferred nodes, "
            f"{info['edges']} edges, length {fmt_length(info['length'])}, parsimony {info['parsimony']}, {info['negative']} negative branches, "
            f"{info['batches']} batches")
