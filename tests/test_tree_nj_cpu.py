"""The model of vdjx_tree_nj (tests/tree_nj_model.py) against the generator of infinite-sites lineages (tests/tree_nj_cases.py), whose own
tree is the independent yardstick; Fitch's total against a brute force over every assignment; the tie rule on hand-written cases; the small
lineages; vdjx_tree_nj_nodes; annot.tree_nj_newick; the table and the stderr line on a hand-written lineage; the numpy steps against the
plain ones on the cases whose distances round, up to 129 members; and every case of the GPU tests reaching the edge it is named for, by
the kernels' own constants and formulas: the word counts of `widths` (every register width, the tiles of 32 columns, the chunked path at
17, 31, 32 and 33 words), and in rand_* the odd lengths on either side of the LDS bound.  No GPU."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from tests import tree_nj_cases as K
from tests import tree_nj_model as N
from tests.tree_model import distance_matrix, members_of, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(case, **kw):
    return N.tree_nj(case["contigs"], case["clone"], case["anchor"], case["prio"], **kw)


def _clades(m, parent_of, nodes):
    """node -> frozenset of the leaves below it, from a parent map over local ids"""
    below = {v: set([v]) if v < m else set() for v in nodes}
    for leaf in range(m):
        v = leaf
        while parent_of[v] >= 0:
            v = parent_of[v]
            below[v].add(leaf)
    return {v: frozenset(s) for v, s in below.items()}


def _generator_rooted(gen, m, root):
    """the generator's tree rooted at leaf `root`: {clade: (length to the parent in mutations, the node's window)}"""
    adj = gen["adj"]
    parent = {root: -1}
    stack = [root]
    while stack:
        v = stack.pop()
        for c in adj[v]:
            if c not in parent:
                parent[c] = v
                stack.append(c)
    clades = _clades(m, parent, list(adj))
    return {clades[v]: (adj[v][parent[v]] if parent[v] >= 0 else 0, gen["seq"][v]) for v in adj}


def _local(case, res, key):
    """the lineage's nodes as local ids: (m, slots, parent map over local ids)"""
    n = len(case["contigs"])
    members = members_of(case["clone"])[key]
    inferred = [s for s in range(n, len(res["parent"])) if res["clone"][s] == key]
    slots = members + inferred
    local = {s: v for v, s in enumerate(slots)}
    parent = {local[s]: (local[int(res["parent"][s])] if res["parent"][s] >= 0 else -1) for s in slots}
    return len(members), slots, parent


@pytest.mark.parametrize("m,seed,w", [(4, 1, None), (5, 2, None), (17, 3, None), (89, 4, 400), (64, 11, None), (65, 12, None), (20, 15, 512)])
def test_infinite_sites_give_the_generators_tree(m, seed, w):
    case = K.infinite_sites(m, seed, w=w)
    res = _model(case)
    n = len(case["contigs"])
    mm, slots, parent = _local(case, res, 0)
    root = next(v for v in range(mm) if parent[v] < 0)
    want = _generator_rooted(case["gen"][0], m, root)
    clades = _clades(mm, parent, list(parent))
    assert sorted(map(sorted, clades.values())) == sorted(map(sorted, want))          # the splits
    total = 0
    for v, s in enumerate(slots):
        length, seq = want[clades[v]]
        assert res["length"][s] == length << 16                                       # exact, none negative
        if v != root:
            assert res["mutations"][s] == length == res["length"][s] >> 16
            total += length
        if s >= n:
            assert res["anc"][s - n] == seq                                           # the inferred node is the generator's
    assert res["info"]["negative"] == 0 and res["info"]["length"] == total << 16 and res["info"]["parsimony"] == total
    assert res["info"]["internal"] == m - 2 and res["info"]["edges"] == 2 * m - 3 and res["info"]["joins"] == m - 3


def test_the_numpy_steps_are_the_plain_ones():
    rng = np.random.default_rng(5)
    for m in (4, 9, 23, 40):
        ws = K.random_windows(m, 60, rng, wild=0.1)
        D = [[int(x) << 16 for x in row] for row in distance_matrix(ws)]
        saved, N.PLAIN_MEMBERS = N.PLAIN_MEMBERS, 1 << 30
        try:
            plain = N.nj_edges(D)
        finally:
            N.PLAIN_MEMBERS = saved
        assert plain == N.nj_edges_numpy(D) and len(plain) == 2 * m - 3


@pytest.mark.parametrize("name", ["random_wild", "rand_64", "rand_65", "rand_129"])
def test_the_numpy_steps_are_the_plain_ones_on_the_cases_that_round(name):
    """the GPU tests of these cases compare with nj_edges_numpy alone (they are above PLAIN_MEMBERS): here it is held against the
    dictionary version on the very matrices, whose joins halve odd sums and divide with a remainder.  rand_300 is left to the numpy
    version: the plain one takes m^3 dictionary reads per join"""
    case = K.gpu_cases()[name]()
    ws, _ = windows(case["contigs"], list(range(len(case["contigs"]))), case["anchor"])
    D = [[int(x) << 16 for x in row] for row in distance_matrix(ws)]
    saved, N.PLAIN_MEMBERS = N.PLAIN_MEMBERS, 1 << 30
    try:
        plain = N.nj_edges(D)
    finally:
        N.PLAIN_MEMBERS = saved
    assert len(ws) > N.PLAIN_MEMBERS and plain == N.nj_edges_numpy(D) and len(plain) == 2 * len(ws) - 3
    assert any(ln & 1 for _, _, ln in plain) and any(ln % (1 << 16) for _, _, ln in plain)


def test_random_windows_stay_within_the_issues_bound():
    rng = np.random.default_rng(6)
    for m in (8, 40, 120):
        ws = K.random_windows(m, 200, rng)
        D = distance_matrix(ws)
        edges = N.nj_edges([[int(x) << 16 for x in row] for row in D])
        assert max(abs(e[2]) for e in edges) <= 0.6 * (int(D.max()) << 16)


def _brute(ws, m, root, parent, kids):
    """the smallest number of changes over all assignments of the inferred nodes, the leaves' wildcards free, column by column"""
    nodes, total = len(parent), 0
    for q in range(len(ws[0])):
        free = [v for v in range(nodes) if v >= m or ws[v][q] not in "ACGT"]
        best = None
        for pick in itertools.product(range(4), repeat=len(free)):
            st = {v: "ACGT".index(ws[v][q]) for v in range(m) if ws[v][q] in "ACGT"}
            st.update(zip(free, pick))
            cost = sum(st[v] != st[parent[v]] for v in range(nodes) if parent[v] >= 0)
            best = cost if best is None else min(best, cost)
        total += best
    return total


def test_fitch_total_is_the_brute_force_minimum():
    rng = np.random.default_rng(7)
    for m in (2, 3, 4, 5, 6, 6):
        for w in (1, 3, 4):
            ws = ["".join(rng.choice(list("ACGTN"), w, p=[0.22, 0.22, 0.22, 0.22, 0.12])) for _ in range(m)]
            edges = N.nj_edges([[int(x) << 16 for x in row] for row in distance_matrix(ws)])
            root = int(rng.integers(m))
            parent, _, _, kids = N.orient(m, edges, root)
            state, mut = N.fitch(ws, m, root, parent, kids)
            assert sum(x for x in mut if x >= 0) == _brute(ws, m, root, parent, kids), (ws, root)
            for v in range(m):                                                        # an observed base is kept, a wildcard takes its parent's
                for q in range(w):
                    assert state[v][q] == ("ACGT".index(ws[v][q]) if ws[v][q] in "ACGT" else state[parent[v]][q] if parent[v] >= 0 else state[v][q])


def test_tie_rule_is_pinned():
    s = "ACGTACGT"
    # three identical: the one step, x < y < z
    assert N.nj_edges([[0] * 3] * 3) == [(0, 3, 0), (1, 3, 0), (2, 3, 0)]
    # four identical: every Q ties at 0, so (0, 1) is joined into 4; then 2 < 3 < 4 meet in 5
    assert N.nj_edges([[0] * 4] * 4) == [(0, 4, 0), (1, 4, 0), (2, 5, 0), (3, 5, 0), (4, 5, 0)]
    res = N.tree_nj([s] * 4, [0] * 4, [0] * 4)
    assert res["parent"].tolist() == [-1, 4, 5, 5, 0, 4] and res["depth"].tolist() == [0, 2, 3, 3, 1, 2] and res["anc"] == [s, s]
    # two pairs, one mutation apart inside a pair and five between the pairs; in the order 0 1 2 3 and reversed.  The Qs of (0, 1) and
    # (2, 3) tie: the smaller ids are joined first -- whichever pair the caller listed first
    a, b, c, d = "AAAAAAAA", "CAAAAAAA", "ACCCCGAA", "ACCCCGAC"
    fwd = N.nj_edges([[int(x) << 16 for x in row] for row in distance_matrix([a, b, c, d])])
    rev = N.nj_edges([[int(x) << 16 for x in row] for row in distance_matrix([d, c, b, a])])
    one = 1 << 16
    # (D: ab 1, ac 5, ad 6, bc 6, bd 7, cd 1; R = 12, 14, 12, 14; Q(ab) = Q(cd) = 2 - 26 = -24.  a and c sit on their pairs' nodes)
    assert fwd == [(0, 4, 0), (1, 4, one), (2, 5, 0), (3, 5, one), (4, 5, 5 * one)]
    assert rev == [(0, 4, one), (1, 4, 0), (2, 5, one), (3, 5, 0), (4, 5, 5 * one)]   # leaf 0 pairs with leaf 1 both times: reversed that is d with c


def test_small_lineages():
    one = N.tree_nj(["ACGT"], [7], [2])
    assert one["parent"].tolist() == [-1] and one["length"].tolist() == [0] and one["mutations"].tolist() == [-1] and one["anc"] == []
    assert one["info"] == dict(members=1, clones=1, largest_clone=1, internal=0, batches=0, negative=0, edges=0, joins=0, cells=0, parsimony=0, length=0)
    two = N.tree_nj(["ACGTN", "ACCTA", "TTTTT"], [3, 3, -1], [0, 0, 0], prio=[5, 1, 0])
    assert two["parent"].tolist() == [1, -1, -1] and two["length"].tolist() == [2 << 16, 0, -1] and two["mutations"].tolist() == [1, -1, -1]
    assert two["depth"].tolist() == [1, 0, -1] and two["clone"].tolist() == [3, 3, -1]
    assert two["info"] == dict(members=2, clones=1, largest_clone=2, internal=0, batches=1, negative=0, edges=1, joins=0, cells=4, parsimony=1, length=2 << 16)
    three = N.tree_nj(["AAAA", "AAAC", "AACC"], [0, 0, 0], [0, 0, 0])
    assert three["parent"].tolist() == [-1, 3, 3, 0] and three["length"].tolist() == [0, 0, 1 << 16, 1 << 16] and three["anc"] == ["AAAC"]
    assert three["mutations"].tolist() == [-1, 0, 1, 1] and three["info"]["parsimony"] == 2 and three["info"]["joins"] == 0


def test_nodes_entry_against_the_model():
    lib = os.path.join(ROOT, "vdjer_amd", "libvdjx.so")
    L = ctypes.CDLL(lib)
    L.vdjx_tree_nj_nodes.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    rng = np.random.default_rng(8)
    for n in (0, 1, 7, 500):
        clone = np.ascontiguousarray(rng.integers(-1, max(2, n // 4), n), np.int32)
        out = ctypes.c_uint64(99)
        assert L.vdjx_tree_nj_nodes(clone.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(out)) == 0
        assert out.value == N.nodes_of(clone)
    bad = np.array([0, -2], np.int32)
    assert L.vdjx_tree_nj_nodes(bad.ctypes.data_as(ctypes.c_void_p), 2, ctypes.byref(out)) == -1       # VDJX_EINVAL


HAND = dict(ids=["c1", "c2", "c3", "c4", "c5"], contigs=["GGAAAA", "GGAAAC", "TTTTTT", "GGAACC", "GGACCC"], clone=[0, 0, -1, 0, 1], anchor=[2, 2, 0, 2, 1])


def test_table_newick_and_line_by_hand():
    res = N.tree_nj(HAND["contigs"], HAND["clone"], HAND["anchor"])
    rows = N.table_rows(HAND["ids"], HAND["contigs"], HAND["clone"], HAND["anchor"], res)
    assert N.table_text(rows) == (
        "clone_id\tnode_id\tparent_id\tbranch_length\tmutations\tdepth\tchildren\tobserved\tsequence\n"
        "lin_1\tc1\t\t0.0000\t\t0\t1\tT\tGGAAAA\n"
        "lin_1\tc2\tlin_1_a1\t0.0000\t0\t2\t0\tT\tGGAAAC\n"
        "lin_1\tc4\tlin_1_a1\t1.0000\t1\t2\t0\tT\tGGAACC\n"
        "lin_1\tlin_1_a1\tc1\t1.0000\t1\t1\t2\tF\tGGAAAC\n"
        "lin_2\tc5\t\t0.0000\t\t0\t0\tT\tGGACCC\n")
    assert N.newick_text(HAND["ids"], HAND["clone"], res) == "lin_1\t(('c2':0.0000,'c4':1.0000)'lin_1_a1':1.0000)'c1';\n"
    assert N.summary_line(res["info"]) == ("trees nj: 4 contigs in 2 lineages (largest 3), 1 inferred nodes, 3 edges, length 2.0000, parsimony 2, "
                                           "0 negative branches, 1 batches")


def test_annot_newick_is_the_models():
    from vdjer_amd import annot
    for case in (K.mixed(21), K.identical(7, 19), K.infinite_sites(2, 102)):
        res = _model(case)
        ids = [f"contig'{i}" for i in range(len(case["contigs"]))]
        keys = sorted(set(int(k) for k in case["clone"] if k >= 0))
        dense = np.array([keys.index(int(k)) if k >= 0 else -1 for k in case["clone"]], np.int32)      # lineage numbers, as the command line has them
        names = N.node_ids(ids, dense)
        assert annot.tree_nj_newick(ids, dense, res["parent"], res["length"]) == N.newick(names, res["clone"], res["parent"], res["length"])


def test_gpu_cases_reach_their_edges():
    bound = K.header_constant("VDJX_NJ_LDS_MEMBERS")
    cases = {k: f() for k, f in K.gpu_cases().items()}
    sizes = {k: K.sizes_of(c) for k, c in cases.items()}
    assert [sizes[f"m{m}"] for m in (1, 2, 3, 4, 5)] == [[1], [2], [3], [4], [5]]
    assert sizes["lds_bound"] == [bound] and sizes["lds_bound_plus1"] == [bound + 1] and sizes["global_300"] == [300] and 300 > bound
    assert K.window_words(cases["one_word"]) == 1 and K.window_words(cases["w512"]) == 16 and K.window_words(cases["w513"]) == 17
    for k in ("w512", "w513"):
        members = list(range(20))
        assert len(windows(cases[k]["contigs"], members, cases[k]["anchor"])[0][0]) == int(k[1:])
    assert len(set(cases["shifted"]["anchor"].tolist())) > 1
    wild = "".join(cases["random_wild"]["contigs"])
    assert "N" in wild and any(ch.islower() for ch in wild)
    assert len(set(cases["identical"]["contigs"])) == 1 and sizes["identical"] == [7]
    many = cases["many_small"]
    assert len(sizes["many_small"]) == 3000 and set(sizes["many_small"]) == {3, 4, 5} and (many["clone"] == -1).sum() == 200
    first = {int(k): i for i, k in reversed(list(enumerate(many["clone"]))) if k >= 0}
    last = {int(k): i for i, k in enumerate(many["clone"]) if k >= 0}
    assert sum(last[k] - first[k] + 1 > sizes["many_small"][k] for k in first) > 2900                   # the members are interleaved
    assert sizes["mixed"] == K.MIXED_SIZES
    assert [K.batches_under(K.MIXED_SIZES, knob) for knob in (1, 2500, 1 << 26)] == [7, 3, 1]
    assert [_model(cases["mixed"], cells_knob=knob)["info"]["batches"] for knob in (1, 2500, 1 << 26)] == [7, 3, 1]
    # widths: every instantiation nj_item<W> of k_nj_matrix's switch, and the chunked path at one word past it, at one below, at and
    # one above a whole number of chunks -- each on a lineage whose last row block and last column slice are partial, and whose slices
    # take more than one LDS tile where the tile holds 32 columns
    reg, rows, target = K.kernel_constant("vdjx_nj.hip", "NJ_REG_WORDS"), K.kernel_constant("vdjx_hamming.h", "HAM_ROWS"), K.kernel_constant("vdjx_hamming.h", "HAM_TARGET_ITEMS")
    words = K.lineage_words(cases["widths"])
    assert sorted(words) == K.WIDTH_WORDS and set(range(1, reg + 1)) <= set(words) and {reg + 1, 2 * reg - 1, 2 * reg, 2 * reg + 1} <= set(words)
    assert K.window_words(cases["widths"]) == 2 * reg + 1 and len(words) == 20 and (cases["widths"]["clone"] == -1).sum() == 5
    m = K.WIDTH_MEMBERS
    assert sizes["widths"] == [m] * 20 and rows < m < 2 * rows and m > bound
    assert -(-sum(s * s for s in sizes["widths"]) // (rows * target)) <= rows         # ham_slice_width: the slices are 64 columns wide
    tile_cols = lambda W: 64 if W <= 8 else 32                                        # nj_item's TC
    assert [min(tile_cols(9), rows - c) for c in range(0, rows, tile_cols(9))] == [32, 32] and m - rows == 6       # tiles of 32, 32 | 6
    lens = {W: len(windows(cases["widths"]["contigs"], v, cases["widths"]["anchor"])[0][0])
            for W, v in zip(words, (members_of(cases["widths"]["clone"])[k] for k in sorted(members_of(cases["widths"]["clone"]))))}
    assert lens[reg] == 32 * reg and lens[2 * reg] == 64 * reg                        # the last word full: no padding bits in the last chunk
    assert all(32 * (W - 1) < w <= 32 * W for W, w in lens.items()) and sum(w % 32 != 0 for w in lens.values()) == 18
    first = {int(k): i for i, k in reversed(list(enumerate(cases["widths"]["clone"]))) if k >= 0}
    last = {int(k): i for i, k in enumerate(cases["widths"]["clone"]) if k >= 0}
    assert all(last[k] - first[k] + 1 > m for k in first)                             # interleaved
    # rand_*: distances that are not additive on every path of k_nj_join.  A length that is odd has lost bits to nj_half or to
    # nj_floor_div's remainder (every distance is a whole multiple of 2^16)
    assert [sizes[k] for k in ("rand_64", "rand_65", "rand_129", "rand_300")] == [[bound], [bound + 1], [129], [300]]
    assert 129 > bound and 129 % rows == 1                                            # the global path, the last row block a single row
    for k in ("rand_64", "rand_65", "rand_129", "rand_300"):
        res = _model(cases[k])
        ln = res["length"][res["parent"] >= 0]
        odd, loose = int((ln & 1).sum()), int((ln % (1 << 16) != 0).sum())
        assert len(ln) == 2 * sizes[k][0] - 3 and odd >= len(ln) // 4 and loose >= len(ln) // 2, (k, odd, loose)
        assert res["info"]["negative"] == 0 and "N" in "".join(cases[k]["contigs"])
    rounding = ("widths", "rand_64", "rand_65", "rand_129", "rand_300", "random_wild", "many_small")
    for k, c in cases.items():
        res = _model(c)
        assert res["info"]["negative"] == 0, k                                        # no case has a negative branch
        if k not in rounding:                                                         # what the cases above add: nothing is rounded in these,
            assert not (res["length"][res["clone"] >= 0] % (1 << 16)).any(), k        # and the others that round stay below the LDS bound
    assert max(sizes["random_wild"] + sizes["many_small"]) <= 40 < bound
