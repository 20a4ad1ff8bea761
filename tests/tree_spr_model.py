"""The model of vdjx_tree_spr (include/vdjx.h) in plain Python: a search over subtree prunings and regraftings for the tree of fewest Fitch
mutations inside every lineage, started from vdjx_tree_nj's tree or from the caller's.  Items, windows, root, node ids, the score P(T), the
start's checks and the finish are tests/tree_mp_model.py's; nothing here is shared with the device code.  Integer throughout.

  candidates  (c, y): c, the pruned node, is any node other than the root leaf and its child.  With p = parent(c), s p's other child and
              g = parent(p), T' is the tree without c's subtree and with p dissolved: s takes p's place under g.  y is the lower end of an
              edge of T': any node of T' other than the root leaf and s (the edge above s is the old place).  For one c there are
              2 (m - leaves(c)) - 4.
  apply       s replaces p among g's children; with x = parent(y) in T', p replaces y among x's children; p's children become {c, y};
              every pair of children ascends again.  The root leaf never moves, ids never change.
  round       every candidate is scored; the one of smallest key (P, c, y) is applied if its P is below the current P, otherwise the
              lineage is finished.  max_rounds caps a lineage's scoring rounds (0: until it is finished).

search_plain is the definition: it applies every candidate to a copy and counts the whole tree with tree_mp_model.count -- no edge formula,
no down sets.  search_numpy (lineages above PLAIN_MEMBERS) scores a prune by one walk: Fitch's length of an unrooted tree does not depend
on the root, so P(T after (c, y)) = P(T') + P(subtree c) + #{columns: comb(U'(y), D'(y)) and U(c) do not meet}, with U' the up sets of T'
(they differ from T's on the path from g to the root only) and D' the down sets, D'(root's child) = the root's set, D'(y) = comb(D'(x),
U'(y's sibling)).  tests/test_tree_spr_cpu.py compares the two on every case both can run."""
import numpy as np

from tests import tree_mp_model as M
from tests import tree_nj_model as N
from tests.tree_model import distance_matrix, members_of, windows

FIELDS = M.FIELDS
PLAIN_MEMBERS = 8
MAX_MEMBERS = 1024                                          # VDJX_SPR_MAX_MEMBERS: a searched lineage


def subtree(m, kids, c):
    out, stack = set(), [c]
    while stack:
        v = stack.pop()
        out.add(v)
        if v >= m:
            stack.extend(kids[v])
    return out


def prunes(m, root, kids):
    return [c for c in range(2 * m - 2) if c != root and c != kids[root][0]]


def regrafts(m, root, parent, kids, c):
    """the y of a pruned c, ascending"""
    p = parent[c]
    s = kids[p][0] if kids[p][1] == c else kids[p][1]
    gone = subtree(m, kids, c) | {p, root, s}
    return [y for y in range(2 * m - 2) if y not in gone]


def candidates(m, root, parent, kids):
    return [(c, y) for c in prunes(m, root, kids) for y in regrafts(m, root, parent, kids, c)]


def apply(parent, kids, c, y):
    """applies candidate (c, y) in place (kids[root] is the list of the root's one child)"""
    p = parent[c]
    s = kids[p][0] if kids[p][1] == c else kids[p][1]
    g = parent[p]
    kids[g] = sorted(s if k == p else k for k in kids[g])
    parent[s] = g
    x = parent[y]
    kids[x] = sorted(p if k == y else k for k in kids[x])
    parent[p] = x
    kids[p] = sorted([c, y])
    parent[y] = p


def geometry(m, root, parent, c, y):
    """what kind of move (c, y) is on the tree before it: the words the tests look for"""
    p = parent[c]
    g = parent[p]
    x = g if parent[y] == p else parent[y]
    return frozenset(w for w, on in [("g_root", g == root), ("x_root", x == root), ("c_leaf", c < m), ("c_inferred", c >= m), ("y_leaf", y < m),
                                     ("y_inferred", y >= m)] if on)


def search_plain(leaves, m, root, parent, kids, max_rounds=0):
    """-> (parent, kids, trace, P, candidates scored): trace[r] = (P before round r, the applied (c, y) or None); the inputs are not
    changed"""
    parent, kids = list(parent), [list(x) for x in kids]
    cur = M.count(leaves, m, root, kids)
    trace, scored = [], 0
    while m > 3:
        best = None
        for c, y in candidates(m, root, parent, kids):
            p2, k2 = list(parent), [list(x) for x in kids]
            apply(p2, k2, c, y)
            key = (M.count(leaves, m, root, k2), c, y)
            scored += 1
            if best is None or key < best:
                best = key
        if best is None or best[0] >= cur:
            trace.append((cur, None))
            break
        trace.append((cur, best[1:]))
        apply(parent, kids, best[1], best[2])
        cur = best[0]
        if len(trace) == max_rounds:
            break
    return parent, kids, trace, cur, scored


def _comb(a, b):
    x = a & b
    return np.where(x != 0, x, a | b)


def _miss(a, b):
    return int(((a & b) == 0).sum())


def search_numpy(leaves, m, root, parent, kids, max_rounds=0, blind=False):
    """search_plain's results by the shortcut of the module text.  blind: the mutant of tests/test_tree_spr_cpu.py, a scorer that ignores
    the down sets (joins c to U'(y) alone)"""
    parent, kids = list(parent), [list(x) for x in kids]
    nodes = len(parent)
    S = np.zeros((nodes, len(leaves[0])), np.uint8)
    S[:m] = np.array(leaves, np.uint8)
    trace, scored = [], 0
    cur = None
    while m > 3:
        total = 0
        for v in M.post_order(m, root, kids):                                         # the up sets of the current tree, in full
            a, b = S[kids[v][0]], S[kids[v][1]]
            S[v] = _comb(a, b)
            total += _miss(a, b)
        total += _miss(S[root], S[kids[root][0]])
        assert cur is None or cur == total
        cur = total
        best = None
        for c in prunes(m, root, kids):
            p = parent[c]
            s = kids[p][0] if kids[p][1] == c else kids[p][1]
            g = parent[p]
            const = -_miss(S[c], S[s])
            over = {}                                                                  # U' where it differs from U: the path from g up
            prev, new, node = p, S[s], g
            while node != root:
                other = kids[node][0] if kids[node][1] == prev else kids[node][1]
                const += _miss(new, S[other]) - _miss(S[prev], S[other])
                new = _comb(new, S[other])
                over[node] = new
                prev, node = node, parent[node]
            const += _miss(S[root], new) - _miss(S[root], S[prev])
            up = lambda v: over[v] if v in over else S[v]
            kids_t = lambda x: [s if k == p else k for k in kids[x]]
            top = kids_t(root)[0]
            down = {top: S[root]}
            stack = [top]
            while stack:
                y = stack.pop()
                if y != s:
                    key = (const + _miss(up(y) if blind else _comb(up(y), down[y]), S[c]), c, y)
                    scored += 1
                    if best is None or key < best:
                        best = key
                if y >= m:
                    a, b = kids_t(y)
                    down[a], down[b] = _comb(down[y], up(b)), _comb(down[y], up(a))
                    stack += [a, b]
                del down[y]
        if best is None or best[0] >= 0:
            trace.append((cur, None))
            break
        trace.append((cur, best[1:]))
        apply(parent, kids, best[1], best[2])
        if blind:                                                                      # the mutant's own figure is no P: recount
            cur = None
        else:
            cur += best[0]
        if len(trace) == max_rounds:
            break
    if cur is None:
        cur = M.count(leaves, m, root, kids)
    return parent, kids, trace, cur, scored


def search(leaves, m, root, parent, kids, max_rounds=0, plain=None):
    use_plain = m <= PLAIN_MEMBERS if plain is None else plain
    return (search_plain if use_plain else search_numpy)(leaves, m, root, parent, kids, max_rounds)


def tree_spr(contigs, clone, anchor, prio=None, start=None, max_rounds=0, ancestors=True, cells_knob=1 << 26, plain=None):
    """-> what tree_mp_model.tree_mp returns ("parent", "mutations", "depth", "clone": arrays[nodes], "anc", "info"), "trace": per searched
    lineage key its rounds (P before, applied (c, y) or None), and "geometry": per searched lineage key, per applied move, geometry()'s
    words.  start: int32[nodes] parents in output slots, or None for tree_nj's tree"""
    n = len(contigs)
    cs = [c.decode("latin-1") if isinstance(c, (bytes, bytearray)) else c for c in contigs]
    groups = members_of(clone)
    for members in groups.values():
        assert len(members) <= (MAX_MEMBERS if len(members) > 3 else M.MAX_MEMBERS)
    nodes = n + sum(max(0, len(v) - 2) for v in groups.values())
    parent, depth, mutations = np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32)
    out_clone = np.full(nodes, -1, np.int32)
    anc, traces, geo = [], {}, {}
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
        leaves = M.leaf_sets(ws)
        info["parsimony_start"] += M.count(leaves, m, root, kids)
        if m > 3:
            before = (list(par), [list(x) for x in kids])
            par, kids, trace, _, scored = search(leaves, m, root, par, kids, max_rounds, plain)
            traces[key] = trace
            geo[key] = []
            for _, mv in trace:                                                        # replayed from the start: the words of every move
                if mv is not None:
                    geo[key].append(geometry(m, root, before[0], *mv))
                    apply(before[0], before[1], *mv)
            moves = len(geo[key])
            info["searched"] += 1
            info["moved"] += moves > 0
            info["moves"] += moves
            info["rounds"] = max(info["rounds"], len(trace))
            info["candidates"] += scored
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
    info["batches"] = M.batches_under(sizes, cells_knob)
    info["members"] = sum(len(v) for v in groups.values())
    info["clones"] = len(groups)
    info["largest_clone"] = max([len(v) for v in groups.values()] or [0])
    return {"parent": parent, "mutations": mutations, "depth": depth, "clone": out_clone, "anc": anc if ancestors else None, "info": info,
            "trace": traces, "geometry": geo}
