"""The model of vdjx_lineage_distance_table and vdjx_lineage_model (include/vdjx.h) in plain Python and numpy: the table with math.log10 and
plain float adds (the same libm, the same order as the C function: the tables are compared for equality), the pair distance character by
character, the same distance for a whole bucket position by position in numpy, the lineage (buckets, links, clones, nearest, info as
tests/lineage_model.py has them), the pairs the device's pre-filter lets through, and the rows and stderr lines of `vdjer --lineages
--lineage-model`.  Nothing here is shared with the C or HIP code."""
import functools
import math

import numpy as np

from tests import lineage_model as M

MISS = 1000                                                  # a side without a full ACGT 5-mer
SYMMETRY = ("avg", "min")
INF = (1 << 31) - 1                                          # past every D (at most 255 * 2 * 65535)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def distance_table(weight):
    """uint32[1024, 4] targeting weights -> (uint16[1024, 4], dict(mean, min_cost, max_cost)).  No numpy log10 and no numpy sum."""
    w = [[max(int(x), 1) for x in row] for row in np.asarray(weight).tolist()]
    cells = [(m, x) for m in range(1024) for x in range(4) if x != (m >> 4 & 3)]
    S = 0
    for m, x in cells:
        S += w[m][x]
    d, total = {}, 0.0
    for m, x in cells:
        d[m, x] = -math.log10(float(w[m][x]) / float(S))
        total = total + d[m, x]
    mean = total / 3072.0
    table = np.zeros((1024, 4), np.uint16)
    for m, x in cells:
        t = math.floor(1000.0 * d[m, x] / mean + 0.5)
        table[m, x] = min(max(t, 1), 65535)
    off = [int(table[m, x]) for m, x in cells]
    return table, dict(mean=mean, min_cost=min(off), max_cost=max(off))


# ---- the pair distance ------------------------------------------------------------------------------------------------------------------------
def _side(a, b, p, table):
    """side(a -> b, p): what the change of a[p] into b[p] costs in a's 5-mer"""
    L = len(a)
    if 2 <= p <= L - 3 and all(ch in "ACGT" for ch in a[p - 2:p + 3]) and b[p] in "ACGT":
        idx = 0
        for ch in a[p - 2:p + 3]:
            idx = 4 * idx + "ACGT".index(ch)
        return int(table[idx][["A", "C", "G", "T"].index(b[p])])
    return MISS


def distance(a, b, table, symmetry="avg"):
    """D(a, b), character by character"""
    assert len(a) == len(b) and symmetry in SYMMETRY
    D = 0
    for p in range(len(a)):
        if a[p] != b[p] or a[p] not in "ACGT" or b[p] not in "ACGT":
            ab, ba = _side(a, b, p, table), _side(b, a, p, table)
            D += ab + ba if symmetry == "avg" else 2 * min(ab, ba)
    return D


def reads_5mer(a, b, p):
    """does D(a, b) look position p up in the table, in either direction (and is p a position that counts)?"""
    counts = a[p] != b[p] or a[p] not in "ACGT" or b[p] not in "ACGT"
    ok = lambda s, t: 2 <= p <= len(s) - 3 and all(ch in "ACGT" for ch in s[p - 2:p + 3]) and t[p] in "ACGT"
    return counts and (ok(a, b) or ok(b, a))


def _codes(js):
    a = np.frombuffer("".join(js).encode("latin-1"), np.uint8).reshape(len(js), -1)
    code = np.full(a.shape, 4, np.int64)
    for k, ch in enumerate(b"ACGT"):
        code[a == ch] = k
    return code


@functools.lru_cache(maxsize=4)
def _matrices(text, m, table_bytes):
    tab = np.frombuffer(table_bytes, np.uint16).reshape(1024, 4).astype(np.int32)
    code = _codes([text]).reshape(m, -1)
    L = code.shape[1]
    avg, low, H = np.zeros((m, m), np.int32), np.zeros((m, m), np.int32), np.zeros((m, m), np.int32)
    good = code < 4
    for p in range(L):
        cost = np.full((m, 5), MISS, np.int32)              # cost[i, y]: side(i -> a junction holding y at p, p)
        if 2 <= p <= L - 3:
            full = good[:, p - 2:p + 3].all(axis=1)
            idx = np.zeros(m, np.int64)
            for q in range(p - 2, p + 3):
                idx = 4 * idx + np.where(full, code[:, q], 0)
            cost[full, :4] = tab[idx[full]]
        own = good[:, p]
        cost[own, code[own, p]] = 0                          # the same base on both sides, both ACGT: the position does not count
        ba = np.ascontiguousarray(cost.T)[code[:, p]]        # ba[i, j] = cost[j, code[i]] = side(j -> i, p); 0 where the position does not count
        ab = ba.T                                            # (an off-centre cell is >= 1, so a position that counts costs > 0 on both sides)
        H += ba > 0
        avg += ab
        avg += ba
        low += np.minimum(ab, ba)
    low *= 2
    for x in (avg, low, H):
        x.setflags(write=False)
    return avg, low, H


def distance_matrix(js, table, symmetry="avg"):
    """distance() of every pair of equally long junctions -> (D int32[m, m], H int32[m, m]: the positions that count; read-only), a
    position at a time: per position a row's cost against each of the five things the other side may hold (A, C, G, T, something else),
    gathered by the other side's code, so that a temporary is m * m and never m * m * L (4,097 junctions: 67 MB).  Both symmetries come
    out of one pass; the last few buckets are kept, so that the second symmetry of a large case costs nothing"""
    assert symmetry in SYMMETRY
    avg, low, H = _matrices("".join(js), len(js), np.ascontiguousarray(table, np.uint16).tobytes())
    return (avg if symmetry == "avg" else low), H


# ---- the lineage ------------------------------------------------------------------------------------------------------------------------------
def slice_width(sizes):
    """the column slice of the pair pass (ham_slice_width of vdjx_hamming.h) for buckets of these sizes"""
    cells = sum(s * s for s in sizes)
    per = -(-cells // (64 * 4096))
    return max(64, -(-per // 64) * 64)


def min_cost(table):
    """the least a counted position can cost: 2 min(1000, smallest off-centre cell)"""
    t = np.asarray(table, np.int64)
    off = [int(t[m, x]) for m in range(1024) for x in range(4) if x != (m >> 4 & 3)]
    return 2 * min(MISS, min(off))


def lineage(junctions, group, table, max_dist=M.DEFAULT, symmetry="avg"):
    """-> (clone int32[n], nearest int32[n], info dict, walked): tests/lineage_model.py's lineage under D, linked when D * den <= 2000 *
    num * L.  walked: the ordered pairs (row, column != row) the device walks -- per row and column slice, in column order, a pair is left
    when h * cmin is past dmax and not below the smallest D > 0 among the slice's columns before it"""
    num, den = max_dist
    n = len(junctions)
    js = [j.decode("latin-1") if isinstance(j, (bytes, bytearray)) else j for j in junctions]
    buckets = {}
    for i in range(n):
        if int(group[i]) != M.NONE:
            assert 1 <= len(js[i]) <= M.MAXLEN
            buckets.setdefault((int(group[i]), len(js[i])), []).append(i)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    width, cmin = slice_width([len(v) for v in buckets.values()]), min_cost(table)
    nearest = np.full(n, -1, np.int32)
    pairs = links = walked = 0
    for (_, L), members in buckets.items():
        m = len(members)
        pairs += m * (m - 1) // 2
        D, H = distance_matrix([js[i] for i in members], table, symmetry)
        dmax = 2000 * num * L // den
        other = ~np.eye(m, dtype=bool)
        pos = np.where(other & (D > 0), D, INF)
        near = pos.min(axis=1)
        for a in range(m):
            if near[a] < INF:
                nearest[members[a]] = near[a]
        for c0 in range(0, m, width):
            before = np.minimum.accumulate(pos[:, c0:c0 + width], axis=1)
            before = np.concatenate([np.full((m, 1), INF, np.int32), before[:, :-1]], axis=1)
            low = H[:, c0:c0 + width] * cmin
            walked += int((other[:, c0:c0 + width] & ~((low > dmax) & (low >= before))).sum())
        for a, b in np.argwhere(np.triu(D <= dmax, 1)).tolist():      # D * den <= 2000 * num * L
            links += 1
            ri, rj = find(members[a]), find(members[b])
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)
    clone = np.full(n, -1, np.int32)
    number = {}
    for i in range(n):
        if int(group[i]) == M.NONE:
            continue
        r = find(i)
        if r not in number:
            assert r == i
            number[r] = len(number)
        clone[i] = number[r]
    info = dict(items=sum(len(v) for v in buckets.values()), buckets=len(buckets), largest_bucket=max([len(v) for v in buckets.values()] or [0]),
                clones=len(number), pairs=pairs, links=links)
    return clone, nearest, info, walked


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def table_rows(ids, junctions, group, vgene, jgene, clone, nearest, counts=None):
    """tests/lineage_model.py's rows with dist_nearest = D / (2000.0 * L)"""
    rows = M.table_rows(ids, junctions, group, vgene, jgene, clone, nearest, counts)
    at = M.COLUMNS.index("dist_nearest")
    for c, row in enumerate(rows):
        if clone[c] >= 0 and nearest[c] >= 0:
            row[at] = "%.4f" % (int(nearest[c]) / (2000.0 * len(junctions[c])))
    return rows


def model_line(path, symmetry, tinfo, walked, info):
    return (f"lineage model: {path}, symmetry {symmetry}, mean {'%.4f' % tinfo['mean']}, costs {tinfo['min_cost']} .. {tinfo['max_cost']}, "
            f"{walked} of {2 * info['pairs']} ordered pairs walked")
