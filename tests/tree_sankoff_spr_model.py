"""The model of vdjx_tree_sankoff_spr (include/vdjx.h) in plain Python: tests/tree_spr_model.py's search over subtree prunings and
regraftings under tests/tree_sankoff_model.py's weighted cost W(T).  Items, windows, root, node ids, the start's checks are
tests/tree_mp_model.py's; candidates, apply and geometry are tree_spr_model's; cost, messages, W and the down pass are
tree_sankoff_model's; nothing here is shared with the device code.  Integer throughout.

  round       every candidate (c, y) is scored; the one of smallest key (W, c, y) is applied if its W is below the current W, otherwise the
              lineage is finished.  max_rounds caps a lineage's scoring rounds (0: until it is finished).

search_plain is the definition: it applies every candidate to a copy and counts the whole tree with tree_sankoff_model._np_count (count
with plain=True: Python ints, column by column) -- no edge formula.  search_numpy scores a prune by one walk.  Fitch's root-independence
does not hold for an asymmetric matrix; with T' the tree without c's subtree and with p dissolved, H' its messages (the stored H but on
the path from g to the root, recomputed upwards from S'_g = H_s + H_other) and E'_y(u) the cheapest cost of everything in T' outside y's
subtree plus the edge into a node in state u placed directly above y,
    E'_top(u) = c[b_root][u] for the root's child in T' (0 for all u where the root's character is a wildcard),
    E'_y(u) = min_v (E'_x(v) + H'_z(v) + c[v][u]) for the children y, z of an inferred node x,
    W(T after (c, y)) = sum over the columns of min_u (E'_y(u) + H_c(u) + H'_y(u)).
tests/test_tree_sankoff_spr_cpu.py compares the two on every case both can run."""
import numpy as np

from tests import tree_mp_model as M
from tests import tree_nj_model as N
from tests import tree_sankoff_model as K
from tests import tree_spr_model as S
from tests.tree_model import distance_matrix, members_of, windows

FIELDS = K.FIELDS
MAX_MEMBERS = S.MAX_MEMBERS                                 # VDJX_SPR_MAX_MEMBERS: a searched lineage
PLAIN_MEMBERS = 6                                           # larger lineages: the identity on arrays


def search_plain(c, leaves, m, root, parent, kids, max_rounds=0, ints=False):
    """-> (parent, kids, trace, W, candidates scored): trace[r] = (W before round r, the applied (c, y) or None); the inputs are not
    changed.  ints: recount with tree_sankoff_model.count (Python ints) and not with _np_count"""
    count = K.count if ints else K._np_count
    parent, kids = list(parent), [list(x) for x in kids]
    cur = count(c, leaves, m, root, kids)
    trace, scored = [], 0
    while m > 3:
        best = None
        for cc, y in S.candidates(m, root, parent, kids):
            p2, k2 = list(parent), [list(x) for x in kids]
            S.apply(p2, k2, cc, y)
            key = (count(c, leaves, m, root, k2), cc, y)
            scored += 1
            if best is None or key < best:
                best = key
        if best is None or best[0] >= cur:
            trace.append((cur, None))
            break
        trace.append((cur, best[1:]))
        S.apply(parent, kids, best[1], best[2])
        cur = best[0]
        if len(trace) == max_rounds:
            break
    return parent, kids, trace, cur, scored


def _np_down(C, T):
    """[w, 4]: min_v (T[v] + c[v][u]) for the four u"""
    return (T[:, :, None] + C[None, :, :]).min(axis=1)


def search_numpy(c, leaves, m, root, parent, kids, max_rounds=0, blind=False):
    """search_plain's results by the identity of the module text.  blind: the mutant of tests/test_tree_sankoff_spr_cpu.py, a scorer that
    drops E' (joins c to H'_y alone)"""
    parent, kids = list(parent), [list(x) for x in kids]
    C = np.array(c, np.int64)
    rcode = np.asarray(leaves[root])
    e_top = np.where((rcode > 3)[:, None], 0, C[np.minimum(rcode, 3)])               # [w, 4]: row b_root of the matrix, 0 for a wildcard
    trace, scored = [], 0
    cur = None
    while m > 3:
        H = K._np_messages(C, leaves, m, root, kids)                                  # the messages of the current tree, in full
        total = K._np_root(H[kids[root][0]], leaves[root])
        assert cur is None or cur == total
        cur = total
        best = None
        for cc in S.prunes(m, root, kids):
            p = parent[cc]
            s = kids[p][0] if kids[p][1] == cc else kids[p][1]
            g = parent[p]
            over = {}                                                                  # H' where it differs from H: the path from g up
            prev, new, node = p, H[s], g
            while node != root:
                other = kids[node][0] if kids[node][1] == prev else kids[node][1]
                new = K._np_message(C, new + H[other])
                over[node] = new
                prev, node = node, parent[node]
            up = lambda v: over[v] if v in over else H[v]
            kids_t = lambda x: [s if k == p else k for k in kids[x]]
            top = kids_t(root)[0]
            down = {top: e_top}
            stack = [top]
            while stack:
                y = stack.pop()
                if y != s:
                    join = H[cc] + up(y) if blind else down[y] + H[cc] + up(y)
                    key = (int(join.min(axis=1).sum()), cc, y)
                    scored += 1
                    if best is None or key < best:
                        best = key
                if y >= m:
                    a, b = kids_t(y)
                    down[a], down[b] = _np_down(C, down[y] + up(b)), _np_down(C, down[y] + up(a))
                    stack += [a, b]
                del down[y]
        if best is None or best[0] >= cur:
            trace.append((cur, None))
            break
        trace.append((cur, best[1:]))
        S.apply(parent, kids, best[1], best[2])
        cur = None if blind else best[0]                                               # (the mutant's own figure is no W: recount)
        if len(trace) == max_rounds:
            break
    if cur is None:
        cur = K._np_count(c, leaves, m, root, kids)
    return parent, kids, trace, cur, scored


def search(c, leaves, m, root, parent, kids, max_rounds=0, plain=None):
    use_plain = m <= PLAIN_MEMBERS if plain is None else plain
    return (search_plain if use_plain else search_numpy)(c, leaves, m, root, parent, kids, max_rounds)


def tree_sankoff_spr(contigs, clone, anchor, prio=None, cost=None, start=None, max_rounds=0, ancestors=True, cells_knob=1 << 26, plain=None):
    """-> what tree_sankoff_model.tree_sankoff returns ("parent", "cost", "mutations", "depth", "clone": arrays[nodes], "anc", "info"),
    "trace": per searched lineage key its rounds (W before, applied (c, y) or None), and "geometry": per searched lineage key, per applied
    move, tree_spr_model.geometry's words.  start: int32[nodes] parents in output slots, or None for tree_nj's tree"""
    c = K.check_cost(cost)
    n = len(contigs)
    cs = [x.decode("latin-1") if isinstance(x, (bytes, bytearray)) else x for x in contigs]
    groups = members_of(clone)
    for members in groups.values():
        assert len(members) <= (MAX_MEMBERS if len(members) > 3 else M.MAX_MEMBERS)
    nodes = n + sum(max(0, len(v) - 2) for v in groups.values())
    parent, depth, mutations = np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int32)
    out_clone, out_cost = np.full(nodes, -1, np.int32), np.full(nodes, -1, np.int64)
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
        leaves = K.codes(ws)
        info["cost_start"] += K._np_count(c, leaves, m, root, kids) if m > 1 else 0
        if m > 3:
            before = (list(par), [list(x) for x in kids])
            par, kids, trace, _, scored = search(c, leaves, m, root, par, kids, max_rounds, plain)
            traces[key] = trace
            geo[key] = []
            for _, mv in trace:                                                        # replayed from the start: the words of every move
                if mv is not None:
                    geo[key].append(S.geometry(m, root, before[0], *mv))
                    S.apply(before[0], before[1], *mv)
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
            for x in kids[v]:
                dep[x] = dep[v] + 1
                stack.append(x)
        state, ecost, mut = (K.reconstruct if m < 2 else K.reconstruct_numpy)(c, leaves, m, root, par, kids)
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
            "info": info, "trace": traces, "geometry": geo}
