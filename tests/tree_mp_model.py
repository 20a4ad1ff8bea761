"""The model of vdjx_tree_mp (include/vdjx.h) in plain Python: a search over nearest-neighbour interchanges for the tree of fewest Fitch
mutations inside every lineage, started from vdjx_tree_nj's tree or from the caller's -- and the rows of `vdjer --trees-mp`, the lines of
`--trees-mp-newick` and the stderr line.  Items, windows, root and node ids are tests/tree_nj_model.py's; nothing here is shared with the
device code or with vdjer_main.c.  Integer throughout.

  score       P(T): over the window columns, the union events of Fitch's upward pass.  A leaf's set is its base if that is one of ACGT,
              else all four; an inferred node's set is the intersection of its children's sets if that is not empty, else their union,
              and the column costs 1; at the root the column costs 1 more if the root leaf's set and its child's set do not meet.
  candidates  (v, k): an inferred node v whose parent p is an inferred node too, k in {0, 1}.  With s p's other child and c = kid[v][k]
              (children ascend), the candidate swaps s and c: v's children become {s, kid[v][1 - k]}, p's {c, v}, both ascending again,
              and the parents of s and c are exchanged.  Ids never change.  A lineage of m members has 2 (m - 3); m <= 3 is not searched.
  round       every candidate is scored; the one of smallest key (P, v, k) is applied if its P is below the current P, otherwise the
              lineage is finished.  max_rounds caps a lineage's scoring rounds (0: until it is finished).
  finish      Fitch's two passes of tests/tree_nj_model.py on the final topology: sequences, mutations, depth.

search_plain copies the tree per candidate and counts it in full; search_numpy (lineages above PLAIN_MEMBERS) keeps the sets of the
current tree as arrays over the columns and rescores a candidate along the path from v to the root only, stopping where no column's set
changed.  tests/test_tree_mp_cpu.py compares the two on every case both can run."""
import numpy as np

from tests import tree_nj_model as N
from tests.tree_model import distance_matrix, members_of, windows

COLUMNS = N.COLUMNS
FIELDS = ["members", "clones", "largest_clone", "internal", "batches", "searched", "moved", "rounds", "edges", "moves", "candidates",
          "parsimony_start", "parsimony"]
PLAIN_MEMBERS = 24
MAX_MEMBERS = N.MAX_MEMBERS


def leaf_sets(ws):
    return [[N.leaf_set(ch) for ch in w] for w in ws]


def post_order(m, root, kids):
    """the inferred nodes, children before parents"""
    out, stack = [], list(kids[root])
    while stack:
        v = stack.pop()
        if v >= m:
            out.append(v)
            stack.extend(kids[v])
    return out[::-1]


def count(leaves, m, root, kids):
    """P of the tree: a full upward pass over every column"""
    if m < 2:
        return 0
    s = dict(enumerate(leaves))
    total = 0
    for v in post_order(m, root, kids):
        a, b = s[kids[v][0]], s[kids[v][1]]
        s[v] = [x & y or x | y for x, y in zip(a, b)]
        total += sum(1 for x, y in zip(a, b) if not x & y)
    return total + sum(1 for x, y in zip(s[root], s[kids[root][0]]) if not x & y)


def candidates(m, parent):
    return [(v, k) for v in range(m, len(parent)) if parent[v] >= m for k in (0, 1)]


def swap(parent, kids, v, k):
    """applies candidate (v, k) in place"""
    p = parent[v]
    s = kids[p][0] if kids[p][1] == v else kids[p][1]
    c, o = kids[v][k], kids[v][1 - k]
    kids[v] = sorted([s, o])
    kids[p] = sorted([c, v])
    parent[s], parent[c] = v, p


def climb(parent, root, v):
    """the inferred nodes above v's parent: 0 where that parent is the root's child (the candidate's walk is then the root step alone)"""
    steps, x = 0, parent[parent[v]]
    while x != root:
        steps, x = steps + 1, parent[x]
    return steps


def search_plain(leaves, m, root, parent, kids, max_rounds=0):
    """-> (parent, kids, trace, P): trace[r] = (P before round r, the applied (v, k) or None, climb of v or None); the inputs are not
    changed"""
    parent, kids = list(parent), [list(x) for x in kids]
    cur = count(leaves, m, root, kids)
    trace = []
    while m > 3:
        best = None
        for v, k in candidates(m, parent):
            p2, k2 = list(parent), [list(x) for x in kids]
            swap(p2, k2, v, k)
            key = (count(leaves, m, root, k2), v, k)
            if best is None or key < best:
                best = key
        if best[0] >= cur:
            trace.append((cur, None, None))
            break
        trace.append((cur, best[1:], climb(parent, root, best[1])))
        swap(parent, kids, best[1], best[2])
        cur = best[0]
        if len(trace) == max_rounds:
            break
    return parent, kids, trace, cur


def _comb(a, b):
    x = a & b
    return np.where(x != 0, x, a | b), x == 0


def search_numpy(leaves, m, root, parent, kids, max_rounds=0):
    """search_plain's results with the sets as uint8 arrays over the columns and every candidate rescored along its path only"""
    parent, kids = list(parent), [list(x) for x in kids]
    nodes = len(parent)
    S = np.zeros((nodes, len(leaves[0])), np.uint8)
    S[:m] = np.array(leaves, np.uint8)
    cur = 0
    for v in post_order(m, root, kids):
        S[v], u = _comb(S[kids[v][0]], S[kids[v][1]])
        cur += int(u.sum())
    cur += int(((S[root] & S[kids[root][0]]) == 0).sum())

    def walk(v, k, store):
        """the change of P under candidate (v, k); store: write the new sets"""
        p = parent[v]
        s = kids[p][0] if kids[p][1] == v else kids[p][1]
        c, o = kids[v][k], kids[v][1 - k]
        nv, fv = _comb(S[s], S[o])
        new, fp = _comb(S[c], nv)
        delta = int(fv.sum()) - int(((S[c] & S[o]) == 0).sum()) + int(fp.sum()) - int(((S[v] & S[s]) == 0).sum())
        if store:
            S[v] = nv
        x, old = p, S[p].copy()
        if store:
            S[p] = new
        while not np.array_equal(new, old):
            g = parent[x]
            if g == root:
                delta += int(((S[root] & new) == 0).sum()) - int(((S[root] & old) == 0).sum())
                break
            a = S[kids[g][0] if kids[g][1] == x else kids[g][1]]
            ng, fg = _comb(new, a)
            delta += int(fg.sum()) - int(((old & a) == 0).sum())
            x, old, new = g, S[g].copy(), ng
            if store:
                S[g] = ng
        return delta

    trace = []
    while m > 3:
        best = None
        for v, k in candidates(m, parent):
            key = (walk(v, k, False), v, k)
            if best is None or key < best:
                best = key
        if best[0] >= 0:
            trace.append((cur, None, None))
            break
        trace.append((cur, best[1:], climb(parent, root, best[1])))
        walk(best[1], best[2], True)
        swap(parent, kids, best[1], best[2])
        cur += best[0]
        if len(trace) == max_rounds:
            break
    return parent, kids, trace, cur


def search(leaves, m, root, parent, kids, max_rounds=0, plain=None):
    use_plain = m <= PLAIN_MEMBERS if plain is None else plain
    return (search_plain if use_plain else search_numpy)(leaves, m, root, parent, kids, max_rounds)


def tree_of_parents(m, root, parent):
    """a lineage's local parents -> its children lists (ascending), or a ValueError naming what is wrong with the tree"""
    nodes = m + max(0, m - 2)
    kids = [[] for _ in range(nodes)]
    for v in range(nodes):
        if v == root:
            continue
        if not 0 <= parent[v] < nodes:
            raise ValueError("a parent outside the lineage")
        kids[parent[v]].append(v)
    for v in range(nodes):
        want = 2 if v >= m else (1 if v == root and m > 1 else 0)
        if len(kids[v]) != want:
            raise ValueError(f"node {v} has {len(kids[v])} children")
    seen, stack = 1, [root]
    while stack:
        for c in kids[stack.pop()]:
            seen += 1
            stack.append(c)
    if seen != nodes:
        raise ValueError("a cycle")
    return kids


def tree_mp(contigs, clone, anchor, prio=None, start=None, max_rounds=0, ancestors=True, cells_knob=1 << 26, plain=None):
    """-> {"parent", "mutations", "depth", "clone": arrays[nodes], "anc": list[str] | None, "info": dict, "trace": per searched lineage key
    its rounds}: Context.tree_mp's, and the trace.  start: int32[nodes] parents in output slots, or None for tree_nj's tree"""
    n = len(contigs)
    cs = [c.decode("latin-1") if isinstance(c, (bytes, bytearray)) else c for c in contigs]
    groups = members_of(clone)
    for members in groups.values():
        assert len(members) <= MAX_MEMBERS
    nodes = n + sum(max(0, len(v) - 2) for v in groups.values())
    parent, depth, mutations = np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32)
    out_clone = np.full(nodes, -1, np.int32)
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
            kids = tree_of_parents(m, root, par)
        leaves = leaf_sets(ws)
        info["parsimony_start"] += count(leaves, m, root, kids)
        if m > 3:
            par, kids, trace, _ = search(leaves, m, root, par, kids, max_rounds, plain)
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
            for c in kids[v]:
                dep[c] = dep[v] + 1
                stack.append(c)
        state, mut = N.fitch(ws, m, root, par, kids)
        for v in range(len(par)):
            s = slot(v)
            out_clone[s], depth[s], mutations[s] = key, dep[v], mut[v]
            parent[s] = slot(par[v]) if par[v] >= 0 else -1
            if v != root:
                info["parsimony"] += mut[v]
            if v >= m:
                anc.append("".join(N.BASES[x] for x in state[v]))
        slot0 += max(0, m - 2)
        info["edges"] += max(0, 2 * m - 3) if m > 1 else 0
        info["internal"] += max(0, m - 2)
        if m > 1:
            sizes.append(m)
    info["batches"] = batches_under(sizes, cells_knob)
    info["members"] = sum(len(v) for v in groups.values())
    info["clones"] = len(groups)
    info["largest_clone"] = max([len(v) for v in groups.values()] or [0])
    return {"parent": parent, "mutations": mutations, "depth": depth, "clone": out_clone, "anc": anc if ancestors else None, "info": info,
            "trace": traces}


def batches_under(sizes, knob):
    """whole lineages of two and more members while their m * m cells fit; one of more cells than the knob goes alone"""
    count_, cells = 0, 0
    for m in sizes:
        if cells and cells + m * m > knob:
            count_, cells = count_ + 1, 0
        cells += m * m
    return count_ + (cells > 0)


def lengths_of(res):
    """the branch lengths `vdjer --trees-mp` prints: the mutations in 1/65536, 0 for a root, -1 for an item in no lineage"""
    mut = res["mutations"].astype(np.int64)
    return np.where(res["clone"] < 0, -1, np.where(res["parent"] < 0, 0, mut << N.SHIFT))


def table_rows(ids, contigs, clone, anchor, res):
    return N.table_rows(ids, contigs, clone, anchor, dict(res, length=lengths_of(res)))


table_text = N.table_text


def newick_text(ids, clone, res):
    return N.newick_text(ids, clone, dict(res, length=lengths_of(res)))


def summary_line(info):
    return (f"trees mp: {info['members']} contigs in {info['clones']} lineages (largest {info['largest_clone']}), {info['searched']} searched, "
            f"{info['moved']} improved, {info['moves']} moves in {info['rounds']} rounds, {info['candidates']} candidates, "
            f"parsimony {info['parsimony_start']} -> {info['parsimony']}, {info['batches']} batches")
