"""The model of vdjx_tree_sankoff (include/vdjx.h) in plain Python: vdjx_tree_mp's trees under a 4 x 4 cost matrix -- the weighted cost of a
rooted lineage tree by Sankoff's up pass, vdjx_tree_mp's search over nearest-neighbour interchanges under that cost, and the down pass that
gives every inferred node its states and every edge its cost.  Items, windows, root, node ids, candidates and the swap are
tests/tree_mp_model.py's and tests/tree_nj_model.py's; nothing here is shared with the device code.  Integer throughout.

  cost        c[s][t]: a parent in state s over a child in state t (A 0, C 1, G 2, T 3); the diagonal 0, the rest 1 .. 65535.
  message     H_x(s) of a child x for a parent state s: c[s][b] for a leaf with base b, 0 for a leaf with any other character,
              min_t (c[s][t] + S_x[t]) for an inferred node, S_v[s] = H_k0(s) + H_k1(s).
  W(T)        per column H_x(b_root) with x the root's child, min_s H_x(s) where the root's character is a wildcard; summed over the columns.
  down pass   the root: its base, or the lowest s of smallest H_x(s); an inferred node under a parent in state s: the lowest t of smallest
              c[s][t] + S_x[t]; a leaf: its base, or its parent's state.  An edge costs the sum of c[parent's state][child's state].
  round       vdjx_tree_mp's, under the key (W, v, k).

search_plain copies the tree per candidate and recounts it in full, column by column in Python ints; search_numpy keeps every node's
message as an int64 array over the columns and rescores a candidate along the path from v to the root only.
tests/test_tree_sankoff_cpu.py compares the two on every case both can run."""
import numpy as np

from tests import tree_mp_model as M
from tests import tree_nj_model as N
from tests.tree_model import distance_matrix, members_of, windows

FIELDS = ["members", "clones", "largest_clone", "internal", "batches", "searched", "moved", "rounds", "edges", "moves", "candidates",
          "cost_start", "cost", "mutations"]
PLAIN_MEMBERS = 12                                          # larger lineages: the same steps on int64 arrays over the columns
MAX_MEMBERS = M.MAX_MEMBERS
MAX_COST = 65535
UNIT = [[0 if s == t else 1 for t in range(4)] for s in range(4)]


def check_cost(cost):
    """the matrix as four lists of Python ints, or a ValueError naming the first bad cell"""
    c = [[int(x) for x in row] for row in (UNIT if cost is None else cost)]
    assert len(c) == 4 and all(len(row) == 4 for row in c)
    for s in range(4):
        for t in range(4):
            if (c[s][t] != 0) if s == t else not 1 <= c[s][t] <= MAX_COST:
                raise ValueError(f"cost[{s}][{t}] is {c[s][t]}")
    return c


def codes(ws):
    """per member the columns' codes: 0 .. 3 for ACGT, 4 for anything else"""
    return [[N.BASES.index(ch) if ch in N.BASES else 4 for ch in w] for w in ws]


def leaf_message(c, b):
    return [0, 0, 0, 0] if b > 3 else [c[s][b] for s in range(4)]


def message(c, S):
    return [min(c[s][t] + S[t] for t in range(4)) for s in range(4)]


def lowest_min(values):
    return min(range(len(values)), key=lambda i: (values[i], i))


def column_messages(c, leaves, m, root, kids, q):
    """column q: node -> its message to its parent, for every node but the root"""
    H = {v: leaf_message(c, leaves[v][q]) for v in range(m) if v != root}
    for v in M.post_order(m, root, kids):
        a, b = H[kids[v][0]], H[kids[v][1]]
        H[v] = message(c, [a[s] + b[s] for s in range(4)])
    return H


def count(c, leaves, m, root, kids):
    """W of the tree: a full up pass over every column"""
    if m < 2:
        return 0
    total = 0
    for q in range(len(leaves[0])):
        h = column_messages(c, leaves, m, root, kids, q)[kids[root][0]]
        total += h[leaves[root][q]] if leaves[root][q] < 4 else min(h)
    return total


def search_plain(c, leaves, m, root, parent, kids, max_rounds=0):
    """-> (parent, kids, trace, W): tree_mp_model.search_plain under the weighted count; the inputs are not changed"""
    parent, kids = list(parent), [list(x) for x in kids]
    cur = count(c, leaves, m, root, kids)
    trace = []
    while m > 3:
        best = None
        for v, k in M.candidates(m, parent):
            p2, k2 = list(parent), [list(x) for x in kids]
            M.swap(p2, k2, v, k)
            key = (count(c, leaves, m, root, k2), v, k)
            if best is None or key < best:
                best = key
        if best[0] >= cur:
            trace.append((cur, None, None))
            break
        trace.append((cur, best[1:], M.climb(parent, root, best[1])))
        M.swap(parent, kids, best[1], best[2])
        cur = best[0]
        if len(trace) == max_rounds:
            break
    return parent, kids, trace, cur


def _np_leaf(C, row):
    """[w, 4]: a leaf's messages over the columns"""
    row = np.asarray(row)
    return np.where((row > 3)[:, None], 0, C.T[np.minimum(row, 3)])


def _np_message(C, S):
    return (S[:, None, :] + C[None, :, :]).min(axis=2)


def _np_root(h, row):
    row = np.asarray(row)
    return int(np.where(row > 3, h.min(axis=1), h[np.arange(len(row)), np.minimum(row, 3)]).sum())


def search_numpy(c, leaves, m, root, parent, kids, max_rounds=0):
    """search_plain's results with every node's message as an int64 array [w, 4] and every candidate rescored along its path only"""
    parent, kids = list(parent), [list(x) for x in kids]
    C = np.array(c, np.int64)
    H = {v: _np_leaf(C, leaves[v]) for v in range(m) if v != root}
    for v in M.post_order(m, root, kids):
        H[v] = _np_message(C, H[kids[v][0]] + H[kids[v][1]])
    cur = _np_root(H[kids[root][0]], leaves[root])

    def walk(v, k, store):
        """W under candidate (v, k); store: keep the new messages"""
        p = parent[v]
        s = kids[p][0] if kids[p][1] == v else kids[p][1]
        cc, o = kids[v][k], kids[v][1 - k]
        nv = _np_message(C, H[s] + H[o])
        new = _np_message(C, H[cc] + nv)
        if store:
            H[v] = nv
        x = p
        while True:
            if store:
                H[x] = new
            g = parent[x]
            if g == root:
                return _np_root(new, leaves[root])
            new = _np_message(C, new + H[kids[g][0] if kids[g][1] == x else kids[g][1]])
            x = g

    trace = []
    while m > 3:
        best = None
        for v, k in M.candidates(m, parent):
            key = (walk(v, k, False), v, k)
            if best is None or key < best:
                best = key
        if best[0] >= cur:
            trace.append((cur, None, None))
            break
        trace.append((cur, best[1:], M.climb(parent, root, best[1])))
        walk(best[1], best[2], True)
        M.swap(parent, kids, best[1], best[2])
        cur = best[0]
        if len(trace) == max_rounds:
            break
    return parent, kids, trace, cur


def search(c, leaves, m, root, parent, kids, max_rounds=0, plain=None):
    use_plain = m <= PLAIN_MEMBERS if plain is None else plain
    return (search_plain if use_plain else search_numpy)(c, leaves, m, root, parent, kids, max_rounds)


def reconstruct(c, leaves, m, root, parent, kids):
    """the down pass -> (state: per node a list of w codes, cost: per node the cost of the edge above it, mutations: per node; -1 for the
    root in both)"""
    nodes, w = len(parent), len(leaves[0])
    state = [[0] * w for _ in range(nodes)]
    cost, mut = [0] * nodes, [0] * nodes
    cost[root] = mut[root] = -1
    if m < 2:
        return state, cost, mut
    order = M.post_order(m, root, kids)[::-1]                 # parents before children
    others = [v for v in range(m) if v != root]
    for q in range(w):
        H = column_messages(c, leaves, m, root, kids, q)
        b = leaves[root][q]
        state[root][q] = b if b < 4 else lowest_min(H[kids[root][0]])
        for v in order:
            s = state[parent[v]][q]
            a, b2 = H[kids[v][0]], H[kids[v][1]]
            state[v][q] = lowest_min([c[s][t] + a[t] + b2[t] for t in range(4)])
        for v in others:
            state[v][q] = leaves[v][q] if leaves[v][q] < 4 else state[parent[v]][q]
        for v in range(nodes):
            if v != root:
                s, t = state[parent[v]][q], state[v][q]
                cost[v] += c[s][t]
                mut[v] += s != t
    return state, cost, mut


def tree_sankoff(contigs, clone, anchor, prio=None, cost=None, start=None, search_=True, max_rounds=0, ancestors=True, cells_knob=1 << 26,
                 plain=None):
    """-> {"parent", "cost" (int64), "mutations", "depth", "clone": arrays[nodes], "anc": list[str] | None, "info": dict, "trace": per
    searched lineage key its rounds}: Context.tree_sankoff's, and the trace.  start: int32[nodes] parents in output slots, or None for
    tree_nj's tree; search_: Context.tree_sankoff's search"""
    c = check_cost(cost)
    n = len(contigs)
    cs = [x.decode("latin-1") if isinstance(x, (bytes, bytearray)) else x for x in contigs]
    groups = members_of(clone)
    for members in groups.values():
        assert len(members) <= MAX_MEMBERS
    nodes = n + sum(max(0, len(v) - 2) for v in groups.values())
    parent, depth, mutations = np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32)
    out_clone, out_cost = np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int64)
    anc, traces = [], {}
    info = dict.fromkeys(FIELDS, 0)
    slot0 = n
    sizes = []
    for key in sorted(groups):
        members = groups[key]
        m = len(members)
        ws, _ = windows(cs, members, anchor)
        root = min(range(m), key=lambda p: (int(prio[members[p]]) if prio is not None else 0, members[p]))
        slot = lambda v: members[v] if v < m else slot0 + v - m
        if start is None:
            edges = N.nj_edges([[int(x) << N.SHIFT for x in row] for row in distance_matrix(ws)]) if m > 1 else []
            par, _, _, kids = N.orient(m, edges, root)
        else:
            local = {slot(v): v for v in range(m + max(0, m - 2))}
            par = [-1 if v == root else local.get(int(start[slot(v)]), -2) for v in range(len(local))]
            kids = M.tree_of_parents(m, root, par)
        leaves = codes(ws)
        use_plain = m <= PLAIN_MEMBERS if plain is None else plain
        info["cost_start"] += (count if use_plain or m < 2 else _np_count)(c, leaves, m, root, kids)
        if m > 3 and search_:
            par, kids, trace, _ = search(c, leaves, m, root, par, kids, max_rounds, plain)
            traces[key] = trace
            moves = sum(1 for _, mv, _ in trace if mv is not None)
            info["searched"] += 1
            info["moved"] += moves > 0
            info["moves"] += moves
            info["rounds"] = max(info["rounds"], len(trace))
            info["candidates"] += len(trace) * 2 * (m - 3)
        dep = [-1] * len(par)
        dep[root] = 0
        stack = [root]
        while stack:
            v = stack.pop()
            for x in kids[v]:
                dep[x] = dep[v] + 1
                stack.append(x)
        state, ecost, mut = (reconstruct if use_plain or m < 2 else reconstruct_numpy)(c, leaves, m, root, par, kids)
        for v in range(len(par)):
            s = slot(v)
            out_clone[s], depth[s], mutations[s], out_cost[s] = key, dep[v], mut[v], ecost[v]
            parent[s] = slot(par[v]) if par[v] >= 0 else -1
            if v != root:
                info["mutations"] += mut[v]
                info["cost"] += ecost[v]
            if v >= m:
                anc.append("".join(N.BASES[x] for x in state[v]))
        slot0 += max(0, m - 2)
        info["edges"] += max(0, 2 * m - 3) if m > 1 else 0
        info["internal"] += max(0, m - 2)
        if m > 1:
            sizes.append(m)
    info["batches"] = M.batches_under(sizes, cells_knob)
    info["members"] = sum(len(v) for v in groups.values())
    info["clones"] = len(groups)
    info["largest_clone"] = max([len(v) for v in groups.values()] or [0])
    return {"parent": parent, "cost": out_cost, "mutations": mutations, "depth": depth, "clone": out_clone, "anc": anc if ancestors else None,
            "info": info, "trace": traces}


def _np_messages(C, leaves, m, root, kids):
    H = {v: _np_leaf(C, leaves[v]) for v in range(m) if v != root}
    for v in M.post_order(m, root, kids):
        H[v] = _np_message(C, H[kids[v][0]] + H[kids[v][1]])
    return H


def _np_count(c, leaves, m, root, kids):
    """count() on arrays"""
    return _np_root(_np_messages(np.array(c, np.int64), leaves, m, root, kids)[kids[root][0]], leaves[root])


def reconstruct_numpy(c, leaves, m, root, parent, kids):
    """reconstruct() on arrays over the columns (np.argmin gives the first, so the lowest, index of the minimum)"""
    C = np.array(c, np.int64)
    nodes = len(parent)
    H = _np_messages(C, leaves, m, root, kids)
    code = np.array(leaves, np.int64)
    state = [None] * nodes
    state[root] = np.where(code[root] < 4, code[root], H[kids[root][0]].argmin(axis=1))
    for v in M.post_order(m, root, kids)[::-1]:
        state[v] = (C[state[parent[v]]] + H[kids[v][0]] + H[kids[v][1]]).argmin(axis=1)
    cost, mut = [0] * nodes, [0] * nodes
    cost[root] = mut[root] = -1
    for v in range(nodes):
        if v == root:
            continue
        if v < m:
            state[v] = np.where(code[v] < 4, code[v], state[parent[v]])
        cost[v] = int(C[state[parent[v]], state[v]].sum())
        mut[v] = int((state[parent[v]] != state[v]).sum())
    return [[int(x) for x in row] for row in state], cost, mut
