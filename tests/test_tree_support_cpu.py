"""The jackknife model of include/vdjx.h (vdjx_tree_support): the keep rule against its check value and against vdjer_amd/annot.py's
jackknife_keep, the kept counts, hand-made cases whose supports are known, the table writer, the ABI mirror and the command line up to
where a GPU would be needed.  No GPU."""
import ctypes
import os
import re

import numpy as np

from tests import tree_model as T
from tests import tree_support_model as S
from tests.test_isotype_cpu import _run
from tests.test_tree_cpu import _rand, _step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the keep rule -----------------------------------------------------------------------------------------------------------------------
def test_mix64_check_value():
    assert S.mix64(0) == 0xE220A8397B1DCDAF == S.CHECK
    assert S.mix64(S.M64) < 1 << 64 and S.mix64(1) != S.mix64(0)


def test_jackknife_keep_is_the_models_rule():
    from vdjer_amd import annot
    for w in (1, 31, 32, 33, 486):
        for seed, r in ((1, 1), (7, 16), (0, 1024), (S.M64, 3), (0x123456789ABCDEF0, 100)):
            got = annot.jackknife_keep(seed, r, w)
            assert got.dtype == np.bool_ and got.shape == (w,) and got.tolist() == S.keep(seed, r, w), (w, seed, r)
    # the rule depends on (seed, r, q) only: a shorter window is a prefix of a longer one's
    assert S.keep(5, 2, 486)[:33] == S.keep(5, 2, 33) and S.keep(5, 2, 64) != S.keep(5, 3, 64) and S.keep(5, 2, 64) != S.keep(6, 2, 64)


def test_kept_counts_are_about_half():
    counts = [sum(S.keep(1, r, 486)) for r in range(1, 65)]
    assert all(0 < k < 486 for k in counts), counts
    assert 200 < sum(counts) / 64 < 286                                 # (486 fair bits: 243 +- 11)


# ---- supports that are known -------------------------------------------------------------------------------------------------------------
def test_a_star_of_identical_sequences_has_full_support():
    s = "ACGTACGTACGGTCA"
    seqs = ["T" * 15] + [s] * 7
    clone, anchor = [-1] + [3] * 7, [0] + [4] * 7
    parent = T.tree(seqs, clone, anchor)[0]
    assert parent.tolist() == [-1, -1, 1, 1, 1, 1, 1, 1]
    B = 12
    sup, info = S.support(seqs, clone, anchor, parent, B, 1)
    assert sup.tolist() == [-1, -1] + [B] * 6                            # every replicate's distances are 0: the star at the smallest index
    assert info == dict(members=7, clones=1, largest_clone=7, replicates=B, batches=1, rounds=3, edges=6, matched=6 * B, full=6)


def test_two_families_joined_by_one_long_edge():
    """two families of identical sequences 40 substitutions apart: whatever half of the columns a replicate keeps (a replicate that kept none
    of the 40 would have to lose 40 fair draws), the families stay stars and one edge joins their smallest indices"""
    rng = np.random.default_rng(11)
    a = _rand(rng, 120)
    b = a
    for q in range(40, 80):
        b = _step(b, q)
    seqs = [a, b, a, b, b, a, a, b]
    clone, anchor = [0] * 8, [60] * 8
    parent, dist, _, _ = T.tree(seqs, clone, anchor)
    assert parent.tolist() == [-1, 0, 0, 1, 1, 0, 0, 1] and dist[1] == 40
    B = 20
    sup, info = S.support(seqs, clone, anchor, parent, B, 3)
    assert sup[1] == B and sup.tolist() == [-1] + [B] * 7 and info["full"] == 7 and info["matched"] == 7 * B


def test_one_column_edges_and_the_index_tie_break():
    """three members in a row, one substitution apart each (column 9 between 0 and 1, column 0 between 1 and 2).  By the keys: 0 - 1 is in
    every replicate's tree (where column 9 is deleted, through the index tie-break: the upper bound the header speaks of).  Where column 9
    is deleted 0 and 1 are equal and 2 hangs under the smaller index, 0; so 1 - 2 is there exactly where column 9 is kept"""
    seqs = ["ACGTACGTAC", "ACGTACGTAT", "GCGTACGTAT"]
    parent = T.tree(seqs, [0] * 3, [0] * 3)[0]
    assert parent.tolist() == [-1, 0, 1]
    sup, info = S.support(seqs, [0] * 3, [0] * 3, parent, 64, 1)
    kept9 = sum(1 for r in range(1, 65) if S.keeps(1, r, 9))
    assert 0 < kept9 < 64 and sup.tolist() == [-1, 64, kept9]
    assert info == dict(members=3, clones=1, largest_clone=3, replicates=64, batches=1, rounds=2, edges=2, matched=64 + kept9, full=1)
    # a parent that is not the tree's is counted just the same
    other, _ = S.support(seqs, [0] * 3, [0] * 3, [-1, 0, 0], 64, 1)
    assert other.tolist() == [-1, 64, 64 - kept9]


def test_info_of_nothing_and_batches():
    assert S.support([], [], [], [], 5, 1)[1] == dict.fromkeys(S.FIELDS, 0)                     # (no item: vdjx_tree_support returns at once)
    seqs = ["ACGT", "ACGA", "ACGT"]
    sup, info = S.support(seqs, [0, 1, 2], [0] * 3, [-1] * 3, 5, 1)
    assert sup.tolist() == [-1] * 3 and info["batches"] == 0 and info["clones"] == 3 and info["rounds"] == 0
    for rows, batches in ((S.ROWS, 1), (3, 5), (5, 5), (6, 3), (8, 3), (9, 2), (15, 1), (1, 5)):
        assert S.support(seqs, [0] * 3, [0] * 3, [-1, 0, 0], 5, 1, rows)[1]["batches"] == batches, rows


def test_table_rows_and_summary_line():
    ids = ["vjf_0_CGT", "vjf_1_x", "vjf_2_CGA", "vjf_3_CGT"]
    contigs = ["AACGTAA", "AAAAAAA", "ACGAAAA", "AACGTAT"]
    clone, anchor, prio = [0, -1, 0, 0], [2, 0, 1, 2], [3, 0, 1, 3]
    parent, dist, depth, _ = T.tree(contigs, clone, anchor, prio)
    sup, info = S.support(contigs, clone, anchor, parent, 16, 7)
    rows = S.table_rows(ids, contigs, clone, anchor, prio, parent, dist, depth, sup, 16)
    plain = T.table_rows(ids, contigs, clone, anchor, prio, parent, dist, depth)
    assert [r[:9] for r in rows] == plain and rows[1][9] == "" and rows[2][9] == ""      # no lineage; the root
    assert rows[0][9] == "%.4f" % (sup[0] / 16) and re.fullmatch(r"[01]\.\d{4}", rows[3][9])
    text = S.table_text(rows)
    assert text.splitlines()[0].split("\t") == S.COLUMNS and S.COLUMNS[-2:] == ["window_length", "support"] and text.splitlines()[2] == "vjf_1_x" + "\t" * 9
    assert S.summary_line(info, 7) == (f"tree support: 16 replicates (seed 7), 2 edges, {info['matched']} of 32 kept, {info['full']} in every replicate, 1 batches")


# ---- the ABI mirror ----------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_exports():
    from vdjer_amd import _lib, api
    assert ctypes.sizeof(_lib.TreeSupportInfo) == 48 and ctypes.sizeof(_lib.TreeSupportParams) == 16
    assert [f for f, _ in _lib.TreeSupportInfo._fields_] == S.FIELDS == list(api.Context.TREE_SUPPORT_FIELDS)
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    assert re.search(r"\bint vdjx_tree_support\(vdjx_ctx\* ctx, const char\* contigs, size_t n, int len, const int32_t\* clone, const int32_t\* anchor,", header)
    assert "0xE220A8397B1DCDAF" in header
    for word in ("bipartitions", "bootstrap with replacement", "upper bound"):      # what is not modelled is said
        assert word in header, word
    assert "vdjx_tree_support" in _lib.SYMBOLS and hasattr(_lib.lib(), "vdjx_tree_support")


# ---- the command line, up to where a GPU would be needed ---------------------------------------------------------------------------------
def _refused(r, tmp_path):
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr, r.stderr[-500:]
    assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
    assert not (tmp_path / "t.tsv").exists() and not (tmp_path / "l.tsv").exists()


def test_cli_tree_support_needs_trees(tmp_path):
    for extra in (["--tree-support", "16"], ["--lineages", "l.tsv", "--tree-support", "16"]):
        r = _run(tmp_path, extra)
        _refused(r, tmp_path)
        assert "--tree-support" in r.stderr and "it needs --trees" in r.stderr, (extra, r.stderr[-500:])


def test_cli_tree_seed_needs_tree_support(tmp_path):
    r = _run(tmp_path, ["--lineages", "l.tsv", "--trees", "t.tsv", "--tree-seed", "7"])
    _refused(r, tmp_path)
    assert "--tree-seed" in r.stderr and "it needs --tree-support" in r.stderr, r.stderr[-500:]


def test_cli_tree_support_values_out_of_range(tmp_path):
    base = ["--lineages", "l.tsv", "--trees", "t.tsv"]
    for bad in ("0", "1025", "-1", "16x", "1.5", "", "+4", " 4", "99999999999999999999999"):
        r = _run(tmp_path, base + ["--tree-support", bad])
        _refused(r, tmp_path)
        assert "--tree-support must be a whole decimal number in 1 .. 1024" in r.stderr, (bad, r.stderr[-500:])
    for bad in ("18446744073709551616", "-1", "7x", "", "0x10"):
        r = _run(tmp_path, base + ["--tree-support", "16", "--tree-seed", bad])
        _refused(r, tmp_path)
        assert "--tree-seed must be a whole decimal number below 2^64" in r.stderr, (bad, r.stderr[-500:])


def test_cli_usage_names_the_flags(tmp_path):
    r = _run(tmp_path, ["--tree-support", "16"])
    assert "--tree-support <B" in r.stderr and "--tree-seed <seed" in r.stderr
