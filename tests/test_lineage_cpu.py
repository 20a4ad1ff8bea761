"""The lineage model of include/vdjx.h (vdjx_lineage) on hand-written cases, the inputs `vdjer --lineages` derives from the V/J hits
(vdjer_amd/annot.py: junction_of, lineage_inputs, parse_lineage_dist) on contigs of a committed golden, the table writer, the ABI mirror and
the command line up to where a GPU would be needed.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import golden_util as G
from tests import lineage_model as M
from tests.test_isotype_cpu import EXE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sub(s, at, ch=None):
    """s with position `at` replaced (by ch, or by another ACGT base)"""
    return s[:at] + (ch or ("A" if s[at] != "A" else "C")) + s[at + 1:]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_distance_counts_differences_and_everything_not_acgt():
    assert M.distance("ACGT", "ACGT") == 0 and M.distance("ACGT", "ACGA") == 1 and M.distance("AAAA", "TTTT") == 4
    assert M.distance("ACNT", "ACNT") == 1                              # N against N is a mismatch
    assert M.distance("ACNT", "ACGT") == 1 and M.distance("acgt", "acgt") == 4 and M.distance("AC*T", "ACGT") == 1
    assert M.distance("NNNN", "ACGT") == 4 and M.distance("", "") == 0
    rng = np.random.default_rng(3)
    js = ["".join(rng.choice(list("ACGTNa*"), 37)) for _ in range(9)]      # the matrix the model works on is the same distance
    assert M.distance_matrix(js).tolist() == [[M.distance(a, b) for b in js] for a in js]


def test_chain_of_three_is_one_clone():
    a = "ACGTACGTACGTACGTACGT"                                          # L = 20 at 1500/10000: d <= 3 is linked
    b = _sub(_sub(_sub(a, 0), 1), 2)                                    # a-b: 3
    c = _sub(_sub(_sub(b, 10), 11), 12)                                 # b-c: 3, a-c: 6
    assert (M.distance(a, b), M.distance(b, c), M.distance(a, c)) == (3, 3, 6)
    clone, near, info = M.lineage([a, b, c], [0, 0, 0])
    assert clone.tolist() == [0, 0, 0] and near.tolist() == [3, 3, 3]
    assert info == dict(items=3, buckets=1, largest_bucket=3, clones=1, pairs=3, links=2)
    # without b the two ends are two clones
    clone, near, info = M.lineage([a, c], [0, 0])
    assert clone.tolist() == [0, 1] and near.tolist() == [6, 6] and info["links"] == 0 and info["clones"] == 2


def test_threshold_edge_at_length_20():
    a = "ACGTACGTACGTACGTACGT"
    d3 = _sub(_sub(_sub(a, 3), 7), 15)
    d4 = _sub(d3, 19)
    assert 3 * 10000 <= 1500 * 20 < 4 * 10000                           # 30000 <= 30000: on the boundary
    assert M.lineage([a, d3], [5, 5])[0].tolist() == [0, 0]
    assert M.lineage([a, d4], [5, 5])[0].tolist() == [0, 1]
    assert M.lineage([a, d4], [5, 5], (2000, 10000))[0].tolist() == [0, 0]


def test_num_zero_links_only_identical_acgt_junctions():
    a, n_ = "ACGTACGTAC", "ACGTNCGTAC"
    clone, near, info = M.lineage([a, a, _sub(a, 4), n_, n_], [1] * 5, (0, 10000))
    assert clone.tolist() == [0, 0, 1, 2, 3] and info["links"] == 1     # the two copies with N are at distance 1 from each other
    assert near.tolist() == [1, 1, 1, 1, 1]
    assert M.lineage([a, a], [1, 1], (0, 1))[1].tolist() == [-1, -1]    # all at distance 0: no nearest


def test_num_equal_den_links_a_whole_bucket_and_nothing_across_buckets():
    js = ["AAAAAA", "TTTTTT", "NNNNNN", "cccccc", "AAAAA", "TTTTT", "AAAAAA"]
    grp = [0, 0, 0, 0, 0, 0, 1]
    clone, near, info = M.lineage(js, grp, (7, 7))
    assert clone.tolist() == [0, 0, 0, 0, 1, 1, 2]                      # same group, other length: another bucket; same junction, other group: too
    assert info == dict(items=7, buckets=3, largest_bucket=4, clones=3, pairs=7, links=7)
    assert near.tolist() == [6, 6, 6, 6, 5, 5, -1]


def test_items_without_a_group_take_no_part_and_clones_number_by_first_appearance():
    a, b = "ACGACGACGACG", "TTTTTTTTTTTT"
    js = ["", b, a, "X" * 300, a, b]
    clone, near, info = M.lineage(js, [M.NONE, 3, 3, M.NONE, 3, 3])
    assert clone.tolist() == [-1, 0, 1, -1, 1, 0] and near.tolist() == [-1, 12, 12, -1, 12, 12]
    assert info["items"] == 4 and info["pairs"] == 6 and info["links"] == 2
    assert M.partition(clone) == {frozenset({1, 5}), frozenset({2, 4})}
    assert M.lineage([], [])[2] == dict(items=0, buckets=0, largest_bucket=0, clones=0, pairs=0, links=0)


def test_table_rows_and_text():
    ids = ["vjf_0_AAA", "vjf_1_x", "vjf_2_AAT"]
    clone, near = np.array([0, -1, 0]), np.array([1, -1, 1])
    rows = M.table_rows(ids, ["AAA", "", "AAT"], None, ["V1", "V2", "V1"], ["J1", "", "J1"], clone, near)
    assert rows == [["vjf_0_AAA", "lin_1", "V1", "J1", "3", "0.3333", "2"], ["vjf_1_x", "", "V2", "", "", "", ""], ["vjf_2_AAT", "lin_1", "V1", "J1", "3", "0.3333", "2"]]
    rows = M.table_rows(ids, ["AAA", "", "AAT"], None, ["V1", "V2", "V1"], ["J1", "", "J1"], clone, near, counts=["1.25", "7.00", "2.50"])
    assert [r[-1] for r in rows] == ["3.75", "", "3.75"]
    text = M.table_text(rows, True)
    assert text.splitlines()[0].split("\t") == M.COLUMNS + ["clone_expected_count"] and text.count("\n") == 4
    assert text.splitlines()[2] == "vjf_1_x\t\tV2\t\t\t\t\t"
    assert M.table_text([], False) == "\t".join(M.COLUMNS) + "\n"


# ---- vdjer_amd/annot.py ------------------------------------------------------------------------------------------------------------------
def _hits(genes, ties=None):
    n = len(genes)
    h = dict(gene=np.array(genes, np.int32), n_tied=np.zeros(n, np.int32), tied=np.full((n, 8), -1, np.int32))
    for c, g in enumerate(genes):
        t = (ties or {}).get(c, [g] if g >= 0 else [])
        h["n_tied"][c] = len(t)
        h["tied"][c][:len(t)] = t
    return h


def test_junction_of_and_lineage_inputs_on_golden_contigs():
    from vdjer_amd import annot
    contigs = G.text("vjf_contigs.txt.gz").split()[:8]
    assert len(contigs) == 8 and all(len(s) > 300 for s in contigs)
    cuts = [(100, 45), (100, 45), (200, 2), (50, 256), (0, 3), (len(contigs[5]) - 255, 255), (10, 30), (10, 30)]
    ids = [f"vjf_{c}_{contigs[c][a:a + k]}" for c, (a, k) in enumerate(cuts)]
    ids[6] = "vjf_6_" + "ACGT" * 100                                   # longer than the contig could hold
    ids[7] = "vjf_7"                                                    # no junction in the id
    for c, (a, k) in enumerate(cuts[:6]):
        p, text = annot.junction_of(ids[c], contigs[c])
        assert text == contigs[c][a:a + k] and p == contigs[c].find(text) and 0 <= p <= a
    assert annot.junction_of(ids[6], contigs[6]) == (-1, "ACGT" * 100) and annot.junction_of(ids[7], contigs[7]) == (-1, "")
    assert annot.junction_of("vjf_3_", "ACGT") == (-1, "") and annot.junction_of("a_b_c_d", "xc_dx") == (1, "c_d")
    names = ["IGHV1-69*01", "IGHV1-69D*02", "IGHV3-30-5*01", "IGHJ4*02", "IGHJ6*01"]
    v = _hits([0, 1, 2, 2, 0, 0, 0, -1], {0: [0, 1]})
    j = _hits([3, 3, 4, 4, 3, -1, 3, 3], {4: [3, 4]})
    junctions, group, vgene, jgene = annot.lineage_inputs(ids, contigs, v, j, names)
    #   0, 1: IGHV1-69 (the D allele normalises to it) / IGHJ4 -> group 0; 2: two bases; 3: 256 bases; 4: IGHV1-69 / IGHJ4,IGHJ6 -> group 1;
    #   5: no J call; 6: junction not found; 7: no V call, no junction
    assert group.dtype == np.uint32 and group.tolist() == [0, 0, M.NONE, M.NONE, 1, M.NONE, M.NONE, M.NONE]
    assert junctions == [contigs[0][100:145], contigs[1][100:145], "", "", contigs[4][:3], "", "", ""]
    assert vgene == ["IGHV1-69", "IGHV1-69", "IGHV3-30", "IGHV3-30", "IGHV1-69", "IGHV1-69", "IGHV1-69", ""]
    assert jgene == ["IGHJ4", "IGHJ4", "IGHJ6", "IGHJ6", "IGHJ4,IGHJ6", "", "IGHJ4", "IGHJ4"]
    ok = annot.lineage_inputs(ids[5:6], contigs[5:6], _hits([2]), _hits([4]), names)
    assert ok[1].tolist() == [0] and len(ok[0][0]) == 255               # 255 bases is still eligible
    clone, near, info = M.lineage(junctions, group)
    assert info["items"] == 3 and info["buckets"] == 2 and [int(x) for x in clone >= 0] == [1, 1, 0, 0, 1, 0, 0, 0]


def test_lineage_dist_parsing():
    from vdjer_amd import annot
    good = {"0.15": 1500, "0": 0, "1": 10000, "1.0": 10000, "1.0000": 10000, ".2": 2000, "0.0001": 1, "0.3": 3000, "0.": 0, "1.": 10000, "0.9999": 9999,
            "0.1234": 1234, ".05": 500}
    for text, num in good.items():
        assert annot.parse_lineage_dist(text) == (num, 10000), text
    for bad in ("", ".", "1.0001", "2", "0.12345", "-0.1", "+0.1", "1e-1", "0,15", " 0.15", "0.15 ", "00.15", "0.1.5", "abc", "1.00000", "10", "0x1"):
        with pytest.raises(ValueError):
            annot.parse_lineage_dist(bad)


# ---- the ABI mirror ----------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_exports():
    from vdjer_amd import _lib, annot, api
    assert ctypes.sizeof(_lib.LineageParams) == 8 and ctypes.sizeof(_lib.LineageInfo) == 32
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    assert re.search(r"\bint vdjx_lineage\(vdjx_ctx\*", header)
    assert re.search(r"#define VDJX_LINEAGE_NONE\s+0xFFFFFFFFu", header) and re.search(r"#define VDJX_LINEAGE_MAXLEN\s+255\b", header)
    assert "vdjx_lineage_params;                 /* 8 bytes  */" in header and "vdjx_lineage_info;  /* 32 bytes */" in header
    assert "vdjx_lineage" in _lib.SYMBOLS and hasattr(_lib.lib(), "vdjx_lineage")
    assert annot.LINEAGE_NONE == api.Context.LINEAGE_NONE == M.NONE == 0xFFFFFFFF and annot.LINEAGE_MAXLEN == M.MAXLEN == 255


# ---- the command line, up to where a GPU would be needed ---------------------------------------------------------------------------------
def test_cli_lineage_dist_needs_lineages(tmp_path):
    for extra in (["--lineage-dist", "0.2"], ["--lineage-dist", "0.2", "--airr", "a.tsv"], ["--quant", "q.tsv", "--lineage-dist", "0.15"]):
        r = _run(tmp_path, extra)
        assert r.returncode != 0 and "--lineage-dist" in r.stderr and "--lineages" in r.stderr and "ELAPSED_SECS" not in r.stderr, (extra, r.stderr[-500:])
        assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
        assert not (tmp_path / "q.tsv").exists() and not (tmp_path / "a.tsv").exists()


def test_cli_lineage_dist_must_be_a_decimal_in_range(tmp_path):
    for bad in ("1.0001", "2", "0.12345", "-0.1", "1e-1", "abc", "", ".", "00.15"):
        r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-dist", bad])
        assert r.returncode != 0 and "--lineage-dist must be a decimal in [0, 1]" in r.stderr and "ELAPSED_SECS" not in r.stderr, (bad, r.stderr[-500:])
        assert not (tmp_path / "l.tsv").exists()


def test_cli_usage_names_the_lineage_flags(tmp_path):
    r = subprocess.run([EXE, "--help", "x"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--lineages" in r.stderr and "--lineage-dist" in r.stderr
