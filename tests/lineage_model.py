"""The model of vdjx_lineage (include/vdjx.h) in plain Python: the distance character by character, a union-find over the linked pairs, the
clones numbered by first appearance, the nearest non-zero distance, the info -- and the rows of `vdjer --lineages`, to predict the command
line's bytes.  Nothing here is shared with the device code or with vdjer_main.c."""
import numpy as np

NONE = 0xFFFFFFFF
MAXLEN = 255
DEFAULT = (1500, 10000)
BLOCK = 128                                                 # rows of distance_matrix compared at a time
COLUMNS = ["sequence_id", "clone_id", "vgene", "jgene", "junction_length", "dist_nearest", "clone_size"]


def distance(a, b):
    """positions at which the characters differ or either is not one of ACGT (N never matches, lower case is not ACGT)"""
    assert len(a) == len(b)
    return sum(1 for x, y in zip(a, b) if x != y or x not in "ACGT" or y not in "ACGT")


def distance_matrix(js):
    """distance() of every pair of equally long junctions, character by character in numpy: int64[m, m].  BLOCK rows at a time, so that
    a temporary holds BLOCK * m * L comparisons and not m * m * L (a bucket of 4,097 junctions of 45 bases: 24 MB, not 755 MB)"""
    a = np.frombuffer("".join(js).encode("latin-1"), np.uint8).reshape(len(js), -1)
    bad = ~np.isin(a, np.frombuffer(b"ACGT", np.uint8))
    out = np.empty((len(js), len(js)), np.int64)
    for r0 in range(0, len(js), BLOCK):
        r1 = r0 + BLOCK
        out[r0:r1] = ((a[r0:r1, None, :] != a[None, :, :]) | bad[r0:r1, None, :] | bad[None, :, :]).sum(-1)
    return out


def lineage(junctions, group, max_dist=DEFAULT):
    """-> (clone int32[n], nearest int32[n], info dict)"""
    num, den = max_dist
    n = len(junctions)
    js = [j.decode("latin-1") if isinstance(j, (bytes, bytearray)) else j for j in junctions]
    buckets = {}
    for i in range(n):
        if int(group[i]) != NONE:
            assert 1 <= len(js[i]) <= MAXLEN
            buckets.setdefault((int(group[i]), len(js[i])), []).append(i)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    nearest = np.full(n, -1, np.int32)
    pairs = links = 0
    for (_, L), members in buckets.items():
        m = len(members)
        pairs += m * (m - 1) // 2
        D = distance_matrix([js[i] for i in members])
        for a in range(m):
            others = np.delete(D[a], a)
            if (others > 0).any():
                nearest[members[a]] = others[others > 0].min()
            for b in np.nonzero(D[a] * den <= num * L)[0]:
                if b <= a:
                    continue
                links += 1
                ri, rj = find(members[a]), find(members[int(b)])
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)
    clone = np.full(n, -1, np.int32)
    number = {}
    for i in range(n):                                      # components in the order of their smallest member: first appearance of a root
        if int(group[i]) == NONE:
            continue
        r = find(i)
        if r not in number:
            assert r == i
            number[r] = len(number)
        clone[i] = number[r]
    info = dict(items=sum(len(v) for v in buckets.values()), buckets=len(buckets), largest_bucket=max([len(v) for v in buckets.values()] or [0]),
                clones=len(number), pairs=pairs, links=links)
    return clone, nearest, info


def partition(clone):
    """the clones as a set of frozensets of item indices (what a permutation of the input must keep)"""
    sets = {}
    for i, c in enumerate(clone):
        if c >= 0:
            sets.setdefault(int(c), set()).add(i)
    return {frozenset(v) for v in sets.values()}


def table_rows(ids, junctions, group, vgene, jgene, clone, nearest, counts=None):
    """the rows of `vdjer --lineages` (lists of strings; COLUMNS [+ clone_expected_count]); counts: the contigs' expected_count as the
    quant table prints them (strings or floats of two decimals), summed per clone in contig order"""
    size, total = {}, {}
    for c, k in enumerate(clone):
        if k >= 0:
            size[int(k)] = size.get(int(k), 0) + 1
            if counts is not None:
                total[int(k)] = total.get(int(k), 0.0) + float("%.2f" % float(counts[c]))
    rows = []
    for c, cid in enumerate(ids):
        k = int(clone[c])
        if k < 0:
            row = [cid, "", vgene[c], jgene[c], "", "", ""]
        else:
            L = len(junctions[c])
            row = [cid, f"lin_{k + 1}", vgene[c], jgene[c], str(L), "%.4f" % (int(nearest[c]) / L) if nearest[c] >= 0 else "", str(size[k])]
        if counts is not None:
            row.append("%.2f" % total[k] if k >= 0 else "")
        rows.append(row)
    return rows


def table_text(rows, counted):
    head = COLUMNS + (["clone_expected_count"] if counted else [])
    return "".join("\t".join(r) + "\n" for r in [head] + rows)


def summary_line(n, info, max_dist=DEFAULT):
    return (f"lineages: {n} contigs, {info['items']} eligible, {info['buckets']} buckets (largest {info['largest_bucket']}), {info['pairs']} pairs, "
            f"{info['links']} links, {info['clones']} lineages at {max_dist[0]}/{max_dist[1]}")
