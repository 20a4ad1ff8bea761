"""The tree model of include/vdjx.h (vdjx_tree) on hand-written cases and against an independent Prim, the window arithmetic, the inputs
`vdjer --trees` derives from the V hits (vdjer_amd/annot.py: tree_inputs), the table writer, the ABI mirror and the command line up to
where a GPU would be needed.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np

from tests import tree_model as T
from tests.test_isotype_cpu import EXE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(rng, n):
    return "".join(rng.choice(list("ACGT"), int(n)))


def _step(s, k):
    """s with position k mod len(s) moved on to the next base"""
    q = k % len(s)
    return s[:q] + "ACGT"[("ACGT".index(s[q]) + 1) % 4] + s[q + 1:]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_distance_is_the_lineage_rule():
    assert T.distance("ACGT", "ACGA") == 1 and T.distance("ACNT", "ACNT") == 1 and T.distance("acgt", "acgt") == 4 and T.distance("AC*T", "ACGT") == 1
    rng = np.random.default_rng(3)
    for L in (5, 37, 300):                                              # the plain loop and the numpy blocks are the same distance
        ws = ["".join(rng.choice(list("ACGTNa*"), L)) for _ in range(9)]
        assert T.distance_matrix(ws).tolist() == [[T.distance(a, b) for b in ws] for a in ws]


def test_kruskal_weight_equals_prim_on_random_clones():
    for seed in range(12):
        rng = np.random.default_rng(700 + seed)
        m, L = int(rng.integers(2, 60)), int(rng.choice([8, 20, 45, 70]))
        f = _rand(rng, L)
        seqs = []
        for _ in range(m):                                              # founder copies with a few substitutions: many equal distances
            s = f
            for q in rng.choice(L, size=int(rng.integers(0, 4)), replace=False).tolist():
                s = _step(s, q)
            seqs.append(s)
        parent, dist, depth, info = T.tree(seqs, [0] * m, [0] * m)
        D = T.distance_matrix(seqs)
        assert info["weight"] == T.prim_weight(D) == int(dist[dist >= 0].sum())
        assert info == dict(members=m, clones=1, largest_clone=m, rounds=(m - 1).bit_length(), edges=m - 1, weight=info["weight"])
        assert (parent < 0).sum() == 1 and parent[0] == -1 and depth[0] == 0
        for i in range(1, m):                                           # every edge carries its distance; depths follow the parents
            assert dist[i] == D[i, parent[i]] and depth[i] == depth[parent[i]] + 1


def test_all_equal_is_a_star_at_the_smallest_index():
    s = "ACGTACGTAC"
    parent, dist, depth, info = T.tree(["TTTTTTTTTT"] + [s] * 6, [-1] + [4] * 6, [0] * 7)
    assert parent.tolist() == [-1, -1, 1, 1, 1, 1, 1] and dist.tolist() == [-1, -1, 0, 0, 0, 0, 0] and depth.tolist() == [-1, 0, 1, 1, 1, 1, 1]
    assert info == dict(members=6, clones=1, largest_clone=6, rounds=3, edges=5, weight=0)
    # rooted elsewhere the star stays a star at the smallest index: the root hangs under it
    parent, dist, depth, _ = T.tree([s] * 5, [0] * 5, [0] * 5, [5, 5, 5, 1, 5])
    assert parent.tolist() == [3, 0, 0, -1, 0] and depth.tolist() == [1, 2, 2, 0, 2]


def test_a_chain_gives_the_chain():
    chain = ["ACGTACGTACGTACGTACGT"]
    for k in range(1, 9):
        chain.append(_step(chain[-1], k))
    assert all(T.distance(chain[k], chain[k + 2]) == 2 for k in range(7))
    order = [4, 0, 8, 2, 6, 1, 7, 3, 5]                                 # item i is chain[order[i]]: index 0 is mid-chain
    seqs = [chain[k] for k in order]
    parent, dist, depth, info = T.tree(seqs, [9] * 9, [0] * 9)
    at = {k: i for i, k in enumerate(order)}
    assert [depth[at[k]] for k in range(9)] == [4, 3, 2, 1, 0, 1, 2, 3, 4] and info["weight"] == 8 and info["rounds"] == 4
    for k in range(9):
        assert parent[at[k]] == (-1 if k == 4 else at[k + 1] if k < 4 else at[k - 1])
    prio = [1] * 9
    prio[at[0]] = 0
    parent, dist, depth, _ = T.tree(seqs, [9] * 9, [0] * 9, prio)
    assert [depth[at[k]] for k in range(9)] == list(range(9)) and dist[at[0]] == -1 and sorted(dist.tolist()) == [-1] + [1] * 8


def test_ties_are_broken_by_the_indices():
    # four members, all pairs at distance 1 except 0-3 (2): the keys (1, 0, 1) (1, 0, 2) (1, 1, 2) (1, 1, 3) (1, 2, 3): Kruskal takes 0-1, 0-2, 1-3
    seqs = ["AAAA", "CAAA", "GAAA", "CAAT"]
    D = T.distance_matrix(seqs)
    assert D[0, 3] == 2 and D[2, 3] == 2 and D[1, 3] == 1
    parent, dist, depth, info = T.tree(seqs, [0] * 4, [0] * 4)
    assert parent.tolist() == [-1, 0, 0, 1] and dist.tolist() == [-1, 1, 1, 1] and depth.tolist() == [0, 1, 1, 2] and info["weight"] == 3


def test_window_arithmetic_at_anchors_0_and_len():
    L = 12
    a = "ACGTACGTACGT"
    # anchors 0 and 5: nothing before the anchor is common, 7 bases from it on: a[0:7] against b[5:12]
    b = "TTTTT" + a[:7]
    assert T.window_of([0, 1], [0, 5], L) == (0, 7) and T.windows([a, b], [0, 1], [0, 5])[0] == [a[:7], a[:7]]
    assert T.tree([a, b], [0, 0], [0, 5])[1].tolist() == [-1, 0]
    # anchors len and 4: 4 bases before the anchor, none from it on: a[8:12] against c[0:4]
    c = a[8:12] + "GGGGGGGG"
    assert T.window_of([0, 1], [L, 4], L) == (4, 0) and T.windows([a, c], [0, 1], [L, 4])[0] == [a[8:], a[8:]]
    assert T.tree([a, c], [1, 1], [L, 4])[1].tolist() == [-1, 0]
    # one member alone keeps its whole contig, wherever its anchor is
    assert T.window_of([0], [0], L) == (0, L) and T.window_of([0], [L], L) == (L, 0) and T.window_of([0], [3], L) == (3, 9)
    # a member anchored at 0 and one at len have nothing in common: the model refuses as vdjx_tree does
    try:
        T.window_of([0, 1], [0, L], L)
    except AssertionError:
        pass
    else:
        raise AssertionError("an empty window was accepted")
    # a difference just outside the common window does not count, one on its first or last position does
    x, y = "AAAA" + "CCCCCCCC", "AAAAT" + "CCCCCCC"
    assert T.tree([x, "G" + x[:-1], y], [0, 0, 0], [4, 5, 4])[1].tolist() == [-1, 0, 1]     # (window: 4 before, 7 after; y differs at its first base after)


def test_items_without_a_clone_and_clone_keys_of_any_size():
    seqs = ["ACGT", "ACGA", "TTTT", "ACGT", "ACGA"]
    parent, dist, depth, info = T.tree(seqs, [2000000000, -1, 7, 2000000000, 7], [0] * 5)
    assert parent.tolist() == [-1, -1, -1, 0, 2] and dist.tolist() == [-1, -1, -1, 0, 4] and depth.tolist() == [0, -1, 0, 1, 1]
    assert info == dict(members=4, clones=2, largest_clone=2, rounds=1, edges=2, weight=4)
    assert T.tree([], [], [])[3] == dict.fromkeys(T.FIELDS, 0)
    assert T.tree(seqs, [-1] * 5, [0] * 5)[3] == dict.fromkeys(T.FIELDS, 0)
    assert T.tree(seqs, [0, 1, 2, 3, 4], [0] * 5)[3] == dict(members=5, clones=5, largest_clone=1, rounds=0, edges=0, weight=0)


def test_table_rows_and_text():
    ids = ["vjf_0_CGT", "vjf_1_x", "vjf_2_CGA", "vjf_3_CGT"]
    contigs = ["AACGTAA", "AAAAAAA", "ACGAAAA", "AACGTAT"]
    clone, anchor, prio = [0, -1, 0, 0], [2, 0, 1, 2], [3, 0, 1, 3]
    parent, dist, depth, info = T.tree(contigs, clone, anchor, prio)
    # window: 1 base before the anchor, 5 from it on: ACGTAA / CGAAAA -> "ACGAAA" / ACGTAT
    assert T.windows(contigs, [0, 2, 3], anchor) == (["ACGTAA", "ACGAAA", "ACGTAT"], (1, 5))
    rows = T.table_rows(ids, contigs, clone, anchor, prio, parent, dist, depth)
    assert rows == [["vjf_0_CGT", "lin_1", "vjf_2_CGA", "1", "1", "1", "3", "1", "6"], ["vjf_1_x"] + [""] * 8,
                    ["vjf_2_CGA", "lin_1", "", "", "0", "1", "1", "0", "6"], ["vjf_3_CGT", "lin_1", "vjf_0_CGT", "1", "2", "0", "3", "1", "6"]]
    text = T.table_text(rows)
    assert text.splitlines()[0].split("\t") == T.COLUMNS and text.count("\n") == 5 and text.splitlines()[2] == "vjf_1_x" + "\t" * 8
    assert T.table_text([]) == "\t".join(T.COLUMNS) + "\n"
    assert T.summary_line(info) == "trees: 3 contigs in 1 lineages (largest 3), 2 edges, total distance 2, 2 rounds"


# ---- vdjer_amd/annot.py ------------------------------------------------------------------------------------------------------------------
def test_tree_inputs_on_hand_made_hits():
    from vdjer_amd import annot
    contigs = ["TTACGTACGGTT", "ACGTACGGTTTT", "TTTTTTTTTTTT", "GGGGACGTACGG"]
    ids = ["vjf_0_ACGTACGG", "vjf_1_ACGTACGG", "vjf_2_ACGTACGG", "vjf_3_ACGTACGG"]
    v = {"mismatches": np.array([3, 0, 9, 1], np.int32), "ins": np.array([1, 0, 9, 0], np.int32), "del": np.array([2, 0, 9, 4], np.int32)}
    anchor, prio = annot.tree_inputs(ids, contigs, v, np.array([0, 0, -1, 5], np.int32))
    assert anchor.dtype == np.int32 and prio.dtype == np.uint32
    assert anchor.tolist() == [2, 0, 0, 4] and prio.tolist() == [6, 0, 0, 5]        # (contig 2 is in no lineage: anchor 0, priority 0)
    parent, dist, depth, info = T.tree(contigs, [0, 0, -1, 5], anchor, prio)
    assert parent.tolist() == [1, -1, -1, -1] and dist.tolist() == [0, -1, -1, -1]   # the member without V mutations is the root


# ---- the ABI mirror ----------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_exports():
    from vdjer_amd import _lib, api
    assert ctypes.sizeof(_lib.TreeInfo) == 32 and [f for f, _ in _lib.TreeInfo._fields_] == T.FIELDS == list(api.Context.TREE_FIELDS)
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    assert re.search(r"\bint vdjx_tree\(vdjx_ctx\* ctx, const char\* contigs, size_t n, int len, const int32_t\* clone, const int32_t\* anchor, const uint32_t\* prio,", header)
    assert "vdjx_tree_info;   /* 32 bytes */" in header
    for word in ("indel", "intermediate nodes", "Newick", "germline sequence as a node"):      # what is not modelled is said
        assert word in header, word
    assert "vdjx_tree" in _lib.SYMBOLS and hasattr(_lib.lib(), "vdjx_tree")


# ---- the command line, up to where a GPU would be needed ---------------------------------------------------------------------------------
def test_cli_trees_needs_lineages(tmp_path):
    for extra in (["--trees", "t.tsv"], ["--trees", "t.tsv", "--airr", "a.tsv"], ["--quant", "q.tsv", "--trees", "t.tsv"]):
        r = _run(tmp_path, extra)
        assert r.returncode != 0 and "--trees" in r.stderr and "it needs --lineages" in r.stderr and "ELAPSED_SECS" not in r.stderr, (extra, r.stderr[-500:])
        assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
        assert not (tmp_path / "t.tsv").exists() and not (tmp_path / "q.tsv").exists() and not (tmp_path / "a.tsv").exists()


def test_cli_usage_names_the_trees_flag(tmp_path):
    r = subprocess.run([EXE, "--help", "x"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--trees <file" in r.stderr
