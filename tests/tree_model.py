"""The model of vdjx_tree (include/vdjx.h) in plain Python: each clone's common window around the anchors, the distance character by
character, Kruskal over the sorted (d, min, max) keys with a plain union-find, a breadth-first walk from the root, the info -- and the rows
of `vdjer --trees`, to predict the command line's bytes.  Nothing here is shared with the device code or with vdjer_main.c."""
import numpy as np

BLOCK = 128                                                 # rows of distance_matrix compared at a time
COLUMNS = ["sequence_id", "clone_id", "parent_id", "dist_parent", "depth", "children", "v_mutations", "window_start", "window_length"]
FIELDS = ["members", "clones", "largest_clone", "rounds", "edges", "weight"]


def distance(a, b):
    """window positions at which the characters differ or either is not one of ACGT (N never matches, lower case is not ACGT)"""
    assert len(a) == len(b)
    return sum(1 for x, y in zip(a, b) if x != y or x not in "ACGT" or y not in "ACGT")


def distance_matrix(ws):
    """distance() of every pair of equally long windows -> int32[m, m]; character by character, in numpy blocks of BLOCK rows where the
    clone is large enough for that to pay"""
    m = len(ws)
    if m * m * len(ws[0]) <= 4096:
        return np.array([[distance(a, b) for b in ws] for a in ws], np.int32).reshape(m, m)
    a = np.frombuffer("".join(ws).encode("latin-1"), np.uint8).reshape(m, -1)
    bad = ~np.isin(a, np.frombuffer(b"ACGT", np.uint8))
    out = np.empty((m, m), np.int32)
    for r0 in range(0, m, BLOCK):
        r1 = r0 + BLOCK
        out[r0:r1] = ((a[r0:r1, None, :] != a[None, :, :]) | bad[r0:r1, None, :] | bad[None, :, :]).sum(-1)
    return out


def members_of(clone):
    """{clone key: its members' indices, ascending}, in order of first appearance"""
    out = {}
    for i, k in enumerate(clone):
        k = int(k)
        assert k >= -1
        if k >= 0:
            out.setdefault(k, []).append(i)
    return out


def window_of(members, anchor, length):
    """(a, b) of a clone: the bases before the anchor and from it on that every member has"""
    a = min(int(anchor[i]) for i in members)
    b = min(length - int(anchor[i]) for i in members)
    assert all(0 <= int(anchor[i]) <= length for i in members) and a + b > 0
    return a, b


def windows(contigs, members, anchor):
    """the members' windows as strings, and (a, b)"""
    a, b = window_of(members, anchor, len(contigs[members[0]]))
    return [contigs[i][int(anchor[i]) - a:int(anchor[i]) + b] for i in members], (a, b)


def kruskal(members, D):
    """the edges (i, j, d), i < j caller's indices, of the minimum spanning tree under the keys (d, i, j)"""
    m = len(members)
    if m < 2:
        return []
    idx = np.asarray(members, np.int64)
    ra, rb = np.triu_indices(m, 1)                          # members ascend, so ra < rb is i < j
    key = np.sort(D[ra, rb].astype(np.int64) << 40 | idx[ra] << 20 | idx[rb])
    parent = {i: i for i in members}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    for k in key.tolist():
        i, j = k >> 20 & 0xFFFFF, k & 0xFFFFF
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[ri] = rj
            out.append((i, j, k >> 40))
            if len(out) == m - 1:
                break
    assert len(out) == m - 1
    return out


def tree(contigs, clone, anchor, prio=None):
    """-> (parent int32[n], dist int32[n], depth int32[n], info dict)"""
    n = len(contigs)
    cs = [c.decode("latin-1") if isinstance(c, (bytes, bytearray)) else c for c in contigs]
    parent, dist, depth = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    groups = members_of(clone)
    weight = 0
    for members in groups.values():
        ws, _ = windows(cs, members, anchor)
        if len(members) == 2:                                # (the one edge there is)
            edges = [(members[0], members[1], distance(ws[0], ws[1]))]
        else:
            edges = kruskal(members, distance_matrix(ws))
        near = {i: [] for i in members}
        for i, j, d in edges:
            near[i].append((j, d))
            near[j].append((i, d))
        root = min(members, key=lambda i: (int(prio[i]) if prio is not None else 0, i))
        depth[root] = 0
        queue = [root]
        for i in queue:                                     # (breadth first: the list grows while it is walked)
            for j, d in near[i]:
                if depth[j] < 0:
                    parent[j], dist[j], depth[j] = i, d, depth[i] + 1
                    weight += d
                    queue.append(j)
        assert len(queue) == len(members)
    largest = max([len(v) for v in groups.values()] or [0])
    info = dict(members=sum(len(v) for v in groups.values()), clones=len(groups), largest_clone=largest,
                rounds=(largest - 1).bit_length() if largest > 1 else 0, edges=sum(len(v) - 1 for v in groups.values()), weight=int(weight))
    return parent, dist, depth, info


def prim_weight(D):
    """the weight of a minimum spanning tree of the complete graph with the distance matrix D, by Prim's algorithm"""
    m = len(D)
    inside = np.zeros(m, bool)
    inside[0] = True
    best = np.asarray(D[0], np.int64).copy()
    total = 0
    for _ in range(m - 1):
        j = int(np.where(inside, np.iinfo(np.int64).max, best).argmin())
        total += int(best[j])
        inside[j] = True
        best = np.minimum(best, D[j])
    return total


def table_rows(ids, contigs, clone, anchor, prio, parent, dist, depth):
    """the rows of `vdjer --trees` (lists of strings, COLUMNS); clone: the 0-based lineage of every contig, -1 for none"""
    n = len(ids)
    kids = [0] * n
    for c in range(n):
        if parent[c] >= 0:
            kids[int(parent[c])] += 1
    win = {k: window_of(members, anchor, len(contigs[0])) for k, members in members_of(clone).items()}
    rows = []
    for c, cid in enumerate(ids):
        k = int(clone[c])
        if k < 0:
            rows.append([cid] + [""] * 8)
            continue
        a, b = win[k]
        root = parent[c] < 0
        rows.append([cid, f"lin_{k + 1}", "" if root else ids[int(parent[c])], "" if root else str(int(dist[c])), str(int(depth[c])), str(kids[c]),
                     str(int(prio[c])), str(int(anchor[c]) - a), str(a + b)])
    return rows


def table_text(rows):
    return "".join("\t".join(r) + "\n" for r in [COLUMNS] + rows)


def summary_line(info):
    return (f"trees: {info['members']} contigs in {info['clones']} lineages (largest {info['largest_clone']}), {info['edges']} edges, "
            f"total distance {info['weight']}, {info['rounds']} rounds")
