"""Seeded inputs for the tests of vdjx_tree_nj.  The main family is infinite-sites lineages: a random unrooted binary tree on m leaves
(every new leaf is inserted into a random edge), every edge with 1 .. 3 mutations, each at a window column of its own.  The Hamming
distance of the leaves is then additive, every value of the fixed-point neighbour joining is a whole multiple of 2^16, and the result has to
be the generator's own tree: its splits, its branch lengths, its inner nodes' sequences.  The generator is the independent yardstick.
The second family is random windows (random_windows): not additive, so the halvings and the floor division of the joins drop bits and the
model alone is the yardstick -- rand_* on both sides of the LDS bound, and `widths`, a lineage per packed word count.

A case is a dict: contigs (equally long str), clone, anchor (int32), prio (uint32), and for the infinite-sites ones "gen": per lineage key
{"members", "adj" (node -> {node: mutations}), "seq" (node -> window)}, leaves 0 .. m - 1 in member order."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def header_constant(name):
    """a #define of include/vdjx.h as an int (the CPU tests read the exported bound without loading the library)"""
    with open(os.path.join(HERE, "..", "include", "vdjx.h")) as f:
        return int(re.search(rf"#define\s+{name}\s+(\d+)u?\b", f.read()).group(1))


def kernel_constant(file, name):
    """a #define with a plain number of vdjer_amd/csrc/<file> as an int: the CPU tests recompute from the kernels' own constants which
    path a case takes, so a case stops passing for reaching its edge when a constant moves"""
    with open(os.path.join(HERE, "..", "vdjer_amd", "csrc", file)) as f:
        return int(re.search(rf"#define\s+{name}\s+(\d+)u?\b", f.read()).group(1))


def random_tree(m, rng):
    """adjacency {node: set} of a random unrooted binary tree: leaves 0 .. m - 1, inner nodes from m on (m >= 2)"""
    if m == 2:
        return {0: {1}, 1: {0}}
    adj = {0: {m}, 1: {m}, 2: {m}, m: {0, 1, 2}}
    edges = [(0, m), (1, m), (2, m)]
    nxt = m + 1
    for leaf in range(3, m):
        a, b = edges.pop(int(rng.integers(len(edges))))
        adj[a].remove(b)
        adj[b].remove(a)
        adj[nxt] = {a, b, leaf}
        adj[a].add(nxt)
        adj[b].add(nxt)
        adj[leaf] = {nxt}
        edges += [(a, nxt), (b, nxt), (leaf, nxt)]
        nxt += 1
    return adj


def infinite_sites_windows(m, rng, w=None):
    """-> (the m leaves' windows, gen); w pads the window with columns that never mutate (None: none)"""
    if m == 1:
        seq = "".join("ACGT"[x] for x in rng.integers(0, 4, w or 20))
        return [seq], {"adj": {0: {}}, "seq": {0: seq}}
    tree = random_tree(m, rng)
    weight = {v: {} for v in tree}
    for a in tree:
        for b in tree[a]:
            if a < b:
                weight[a][b] = weight[b][a] = int(rng.integers(1, 4))
    total = sum(sum(x.values()) for x in weight.values()) // 2
    w = total if w is None else w
    assert w >= total
    cols = [int(x) for x in rng.permutation(w)[:total]]
    seq = {0: [int(x) for x in rng.integers(0, 4, w)]}
    stack = [(0, -1)]
    while stack:
        v, up = stack.pop()
        for c in sorted(tree[v]):
            if c == up:
                continue
            s = list(seq[v])
            for _ in range(weight[v][c]):
                q = cols.pop()
                s[q] = (s[q] + 1 + int(rng.integers(3))) % 4
            seq[c] = s
            stack.append((c, v))
    assert not cols
    text = {v: "".join("ACGT"[x] for x in s) for v, s in seq.items()}
    return [text[v] for v in range(m)], {"adj": weight, "seq": text}


def assemble(lineages, rng, loose=0, shuffle=False, shift=0):
    """lineages: [(windows, gen or None)] -> a case.  The contigs are as long as the widest window + shift.  A lineage's window of w
    columns starts in its first member at 0 and in its second as far right as the contig allows, in the others anywhere between (the
    rest of a contig is random): the members' anchors differ, and their common window is exactly the w columns (a lineage of one member
    has its whole contig).  `loose` items of clone -1 are added; shuffle interleaves everything, the members of a lineage keeping their
    order, so that leaf p of the generator is the lineage's p-th member"""
    length = max(len(ws[0]) for ws, _ in lineages) + shift
    items = []                                              # (clone key, contig, anchor, leaf)
    for key, (ws, _) in enumerate(lineages):
        w = len(ws[0])
        a = int(rng.integers(0, w + 1))
        for p, win in enumerate(ws):
            left = 0 if p == 0 else (length - w if p == 1 else int(rng.integers(0, length - w + 1)))
            pad = "".join("ACGT"[x] for x in rng.integers(0, 4, length - w))
            items.append((key, pad[:left] + win + pad[left:], left + a, p))
    for _ in range(loose):
        items.append((-1, "".join("ACGTN"[x] for x in rng.integers(0, 5, length)), int(rng.integers(0, length + 1)), 0))
    if shuffle:
        items = [items[i] for i in rng.permutation(len(items))]
        slots = {}
        for s, it in enumerate(items):
            if it[0] >= 0:
                slots.setdefault(it[0], []).append(s)
        for mine in slots.values():
            for s, it in zip(mine, sorted((items[s] for s in mine), key=lambda it: it[3])):
                items[s] = it
    case = {"contigs": [x[1] for x in items], "clone": np.array([x[0] for x in items], np.int32), "anchor": np.array([x[2] for x in items], np.int32),
            "prio": rng.integers(0, 4, len(items)).astype(np.uint32), "gen": {}}
    for key, (ws, gen) in enumerate(lineages):
        if gen is not None:
            case["gen"][key] = dict(gen, members=[i for i, x in enumerate(items) if x[0] == key])
    return case


def infinite_sites(m, seed, w=None, shift=0):
    rng = np.random.default_rng(seed)
    return assemble([infinite_sites_windows(m, rng, w)], rng, shift=shift)


def random_windows(m, w, rng, wild=0.0, per_member=0.1):
    """a random base window and members that each change about per_member of its columns: not additive; wild: the share of N / lower case"""
    base = rng.integers(0, 4, w)
    out = []
    for _ in range(m):
        s = np.where(rng.random(w) < per_member, rng.integers(0, 4, w), base)
        chars = np.array(list("ACGT"))[s]
        if wild:
            r = rng.random(w)
            chars = np.where(r < wild / 2, "N", np.where(r < wild, np.char.lower(chars), chars))
        out.append("".join(chars))
    return out


def random_case(m, w, seed, wild=0.0):
    rng = np.random.default_rng(seed)
    return assemble([(random_windows(m, w, rng, wild), None)], rng)


def identical(m, seed, w=40):
    rng = np.random.default_rng(seed)
    win = "".join("ACGT"[x] for x in rng.integers(0, 4, w))
    return assemble([([win] * m, None)], rng)


def many_small(count, seed, loose=200):
    """`count` lineages of 3 .. 5 members with windows of 20 .. 70 columns, items of clone -1 among them, everything interleaved"""
    rng = np.random.default_rng(seed)
    lin = [(random_windows(int(rng.integers(3, 6)), int(rng.integers(20, 71)), rng, wild=0.02, per_member=0.15), None) for _ in range(count)]
    return assemble(lin, rng, loose=loose, shuffle=True)


MIXED_SIZES = [3, 1, 5, 20, 2, 65, 4, 8]                    # cells: 9 + 25 + 400 + 4 | 4225 | 16 + 64 under a knob of 2500


def mixed(seed):
    """lineages of MIXED_SIZES members, infinite sites each, interleaved: for the batches under VDJX_NJ_CELLS"""
    rng = np.random.default_rng(seed)
    return assemble([infinite_sites_windows(m, rng) for m in MIXED_SIZES], rng, loose=5, shuffle=True)


WIDTH_WORDS = list(range(1, 18)) + [31, 32, 33]            # every register width of k_nj_matrix; the chunked path at 17, below, at and above 2 x 16
WIDTH_MEMBERS = 70                                          # row blocks of 64 and 6, column slices of 64 and 6: tiles of 32, 32 and 6 from 9 words on


def widths(seed):
    """a lineage of WIDTH_MEMBERS members per word count of WIDTH_WORDS, non-additive windows with wildcards, interleaved: 16 and 32 words
    are full (32 W columns), the others end inside their last word"""
    rng = np.random.default_rng(seed)
    cols = [32 * W if W in (16, 32) else 32 * W - 1 - 7 * W % 31 for W in WIDTH_WORDS]
    lin = [(random_windows(WIDTH_MEMBERS, w, rng, wild=0.05, per_member=0.2), None) for w in cols]
    return assemble(lin, rng, loose=5, shuffle=True)


def batches_under(sizes, knob):
    """the batches of whole lineages (of two and more members, in key order) under a knob of matrix cells: how many"""
    count, cells = 0, 0
    for m in sizes:
        if m < 2:
            continue
        if cells and cells + m * m > knob:
            count, cells = count + 1, 0
        cells += m * m
    return count + (cells > 0)


def sizes_of(case):
    keys = sorted(set(int(k) for k in case["clone"] if k >= 0))
    return [int((case["clone"] == k).sum()) for k in keys]


def window_words(case):
    """the packed words (32 bases each) of the case's widest common window"""
    from tests.tree_model import members_of, window_of
    return max((sum(window_of(v, case["anchor"], len(case["contigs"][0]))) + 31) // 32 for v in members_of(case["clone"]).values())


def lineage_words(case):
    """the packed words of every lineage's common window, in key order"""
    from tests.tree_model import members_of, window_of
    groups = members_of(case["clone"])
    return [(sum(window_of(groups[k], case["anchor"], len(case["contigs"][0]))) + 31) // 32 for k in sorted(groups)]


def gpu_cases():
    """name -> builder of every case test_gpu_tree_nj.py runs; test_tree_nj_cpu.py checks that each reaches the edge it is named for"""
    bound = header_constant("VDJX_NJ_LDS_MEMBERS")
    out = {f"m{m}": (lambda m=m: infinite_sites(m, 100 + m)) for m in (1, 2, 3, 4, 5)}
    out.update({
        "lds_bound": lambda: infinite_sites(bound, 11),
        "lds_bound_plus1": lambda: infinite_sites(bound + 1, 12),
        "global_300": lambda: infinite_sites(300, 13),
        "one_word": lambda: infinite_sites(6, 14),
        "w512": lambda: infinite_sites(20, 15, w=512),
        "w513": lambda: infinite_sites(20, 16, w=513),
        "shifted": lambda: infinite_sites(12, 17, shift=9),
        "random_wild": lambda: random_case(40, 100, 18, wild=0.1),
        "identical": lambda: identical(7, 19),
        "many_small": lambda: many_small(3000, 20),
        "mixed": lambda: mixed(21),
        "widths": lambda: widths(23),
        # distances that are not additive: lengths that are odd and no whole multiple of 2^16 -- on the LDS bound, past it, with a last
        # row block of one row, and at size on the global path
        "rand_64": lambda: random_case(bound, 230, 24, wild=0.05),
        "rand_65": lambda: random_case(bound + 1, 230, 25, wild=0.05),
        "rand_129": lambda: random_case(129, 300, 26, wild=0.05),
        "rand_300": lambda: random_case(300, 400, 27, wild=0.05),
    })
    return out
