"""Without a GPU: vdjx_lineage_distance_table (plain C) against the Python table of tests/lineage_dist_model.py for equality, the model's
own properties (2,000 x Hamming under the uniform table, symmetry, min <= avg, the numpy matrices against the character walk), the proof
that every named case of tests/lineage_dist_cases.py meets its condition in the model -- so that no GPU test passes vacuously --, the
refusals of annot.lineage_distance_table and of the command line, and the ABI mirror."""
import ctypes
import os

import numpy as np
import pytest

from tests import lineage_dist_cases as LC
from tests import lineage_dist_model as LM
from tests import lineage_model as M
from tests.test_isotype_cpu import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the table --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform", "all_equal", "realistic", "realistic_levels", "zeros", "one_big", "seeded", "seeded_small"])
def test_c_table_equals_model(name):
    from vdjer_amd import annot
    w = LC.weights()[name]
    table, info = annot.lineage_distance_table(w)
    mt, mi = LM.distance_table(w)
    assert table.dtype == np.uint16 and table.shape == (1024, 4)
    assert np.array_equal(table, mt), [(m, table[m].tolist(), mt[m].tolist()) for m in np.flatnonzero((table != mt).any(axis=1))[:5]]
    assert info == mi, (info, mi)                                          # the mean bit for bit
    for m in range(1024):
        c = m >> 4 & 3
        assert table[m, c] == 0 and all(table[m, x] >= 1 for x in range(4) if x != c)
    if name in ("uniform", "all_equal", "zeros"):                          # a mismatch under the uniform model costs exactly 1,000
        assert (info["min_cost"], info["max_cost"]) == (1000, 1000)
    if name == "one_big":                                                  # 2^32 - 1 among ones: its cost clamps to 1, the others are the mean
        assert table[LC._index5("AAGCA"), 3] == 1 and (info["min_cost"], info["max_cost"]) == (1, 1000)
    if name.startswith(("realistic", "seeded")):
        assert info["min_cost"] < 1000 < info["max_cost"]


def test_table_ignores_the_centre_column():
    from vdjer_amd import annot
    w = LC.weights()["seeded"].copy()
    base = annot.lineage_distance_table(w)
    for m in range(1024):
        w[m, m >> 4 & 3] = 0xFFFFFFFF
    again = annot.lineage_distance_table(w)
    assert np.array_equal(base[0], again[0]) and base[1] == again[1]


def test_table_refusals(tmp_path):
    from vdjer_amd import annot
    for bad in (np.ones((1024, 3), np.uint32), np.ones(4096, np.uint32), np.ones((1024, 4)), np.full((1024, 4), -1), np.full((1024, 4), 1 << 32)):
        with pytest.raises(ValueError, match="weights of shape"):
            annot.lineage_distance_table(bad)
    good = tmp_path / "t.tsv"
    annot.write_targeting(str(good), LC.weights()["realistic"])
    table, info = annot.lineage_distance_table(str(good))                  # a path: read by read_targeting
    assert np.array_equal(table, LC.tables()["realistic"]) and info == LM.distance_table(LC.weights()["realistic"])[1]
    with pytest.raises(OSError):
        annot.lineage_distance_table(str(tmp_path / "none.tsv"))
    lines = good.read_text().splitlines()
    for change, message in ((lambda ls: ls[:7] + ["AACGX\t1\t1\t1\t1"] + ls[8:], "line 8: expected"), (lambda ls: ls[:7] + ["AAAAC\t1\t1\t1"] + ls[8:], "line 8: expected"),
                            (lambda ls: ls[:7] + [ls[7].rsplit("\t", 1)[0] + "\t4294967296"] + ls[8:], "line 8: expected"),
                            (lambda ls: ls + [ls[3]], "line 1025: the 5-mer AAAAT is given twice"), (lambda ls: ls[:-1], "1023 5-mers")):
        bad = tmp_path / "bad.tsv"
        bad.write_text("\n".join(change(lines)) + "\n")
        with pytest.raises(ValueError, match=message):
            annot.lineage_distance_table(str(bad))
    L = __import__("vdjer_amd._lib", fromlist=["lib"]).lib()
    w, t = np.ones((1024, 4), np.uint32), np.zeros((1024, 4), np.uint16)
    assert L.vdjx_lineage_distance_table(None, t.ctypes.data, None) != 0 and b"vdjx_lineage_distance_table: NULL" in L.vdjx_last_error()
    assert L.vdjx_lineage_distance_table(w.ctypes.data, None, None) != 0
    assert L.vdjx_lineage_distance_table(w.ctypes.data, t.ctypes.data, None) == 0 and t[0].tolist() == [0, 1000, 1000, 1000]      # info may be NULL


# ---- the model's own properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LC.LENGTHS)
def test_uniform_table_is_2000_times_hamming(L):
    js, grp, md, tab = LC.cases()[f"len_{L}_uniform"]
    assert tab == "uniform" and (LC.tables()["uniform"][:, 1:][np.arange(1024) >> 4 & 3 == 0] == 1000).all()
    weird = [s[:len(s) // 2] + "N" + s[len(s) // 2 + 1:] for s in js[:3]] + [js[0].lower(), "N" * L]
    every = js + weird
    for sym in LM.SYMMETRY:
        D, H = LM.distance_matrix(every, LC.tables()["uniform"], sym)
        assert np.array_equal(D, 2000 * M.distance_matrix(every)) and np.array_equal(H, M.distance_matrix(every)), sym
        for a, b in ((0, 1), (0, len(js)), (len(js), len(js) + 1), (len(every) - 1, len(every) - 1)):
            assert LM.distance(every[a], every[b], LC.tables()["uniform"], sym) == 2000 * M.distance(every[a], every[b])
        clone, near, info, walked = LC.models()[f"len_{L}_uniform", sym]
        hclone, hnear, hinfo = M.lineage(js, grp, md)
        assert np.array_equal(clone, hclone) and np.array_equal(near, np.where(hnear >= 0, 2000 * hnear, -1)) and info == hinfo


@pytest.mark.parametrize("L", [3, 4])
def test_shorter_than_five_has_no_5mer(L):
    """under any table a junction of fewer than 5 bases behaves as under the uniform one"""
    js = LC.cases()[f"len_{L}"][0]
    for tab in ("realistic", "extreme"):
        for sym in LM.SYMMETRY:
            assert np.array_equal(LM.distance_matrix(js, LC.tables()[tab], sym)[0], 2000 * M.distance_matrix(js))
    assert not any(LM.reads_5mer(js[0], s, p) for s in js for p in range(L))
    five = LC.cases()["len_5"][0]
    assert {p for s in five for p in range(5) if LM.reads_5mer(five[0], s, p)} <= {2}


@pytest.mark.parametrize("name", ["size_65", "len_33", "len_255_extreme", "placed_70_extreme", "not_acgt_realistic", "not_acgt_extreme", "interleaved_extreme"])
def test_symmetric_min_below_avg_and_matrix_equals_walk(name):
    js, grp, md, tab = LC.cases()[name]
    table = LC.tables()[tab]
    L = max(len(s) for s in js)
    js = [s for s in js if len(s) == L]
    avg, H = LM.distance_matrix(js, table, "avg")
    low, _ = LM.distance_matrix(js, table, "min")
    assert np.array_equal(avg, avg.T) and np.array_equal(low, low.T) and (low <= avg).all() and np.array_equal(H, M.distance_matrix(js))
    assert ((avg == 0) == (H == 0)).all() and ((low == 0) == (H == 0)).all()      # D = 0 iff equal and all ACGT
    if tab == "extreme":
        assert (low < avg).any()
    rng = np.random.default_rng(3)
    for a, b in rng.integers(0, len(js), (150, 2)).tolist():
        assert avg[a, b] == LM.distance(js[a], js[b], table, "avg") == LM.distance(js[b], js[a], table, "avg")
        assert low[a, b] == LM.distance(js[a], js[b], table, "min")


# ---- the named cases meet their conditions ------------------------------------------------------------------------------------------------
def test_tables_are_what_the_cases_need():
    T = LC.tables()
    off = np.arange(4)[None, :] != (np.arange(1024) >> 4 & 3)[:, None]
    assert (T["uniform"][off] == 1000).all() and len(set(T["realistic"][off].tolist())) > 100
    ext = T["extreme"][off]
    assert (ext == 1).sum() > 500 and (ext == 65535).sum() > 500 and ext.min() == 1 and len(set(ext.tolist())) > 1000
    for t in T.values():
        assert (t[~off] == 0).all() and (t[off] >= 1).all()
    assert LM.min_cost(T["uniform"]) == 2000 and LM.min_cost(T["extreme"]) == 2 and LM.min_cost(T["realistic"]) == 2 * int(T["realistic"][off].min()) < 2000


def test_differs_from_hamming_both_ways():
    for name, hamming_links in (("heavier_than_hamming", True), ("lighter_than_hamming", False)):
        js, grp, md, tab = LC.cases()[name]
        assert md == M.DEFAULT and tab == "realistic"
        assert (M.lineage(js, grp, md)[2]["links"] == 1) == hamming_links
        assert (LC.models()[name, "avg"][2]["links"] == 1) != hamming_links, name


def test_symmetry_case_differs():
    a, b = LC.models()["symmetry_matters", "avg"], LC.models()["symmetry_matters", "min"]
    assert M.partition(a[0]) != M.partition(b[0]) and a[2]["clones"] == 4 and b[2]["clones"] == 3 and a[2]["links"] == 1 and b[2]["links"] == 2


def test_largest_d():
    """every position differs; the 251 with a 5-mer cost 65,535 on both sides, the two at either end the mean: the largest D a pair can
    reach.  (The bound the header gives for 32 bits, 255 * 2 * 65,535 = 33,422,850, leaves the ends out of account.)"""
    js, grp, md, tab = LC.cases()["largest_d"]
    want = 251 * 2 * 65535 + 4 * 2000
    for sym in LM.SYMMETRY:
        clone, near, info, walked = LC.models()["largest_d", sym]
        assert near.tolist() == [want, want] and info["links"] == 0 and walked == 2
    assert want == 32906570 < 255 * 2 * 65535 == 33422850 < 1 << 31 and md == (1, 1) and len(js[0]) == 255


@pytest.mark.parametrize("L", LC.PLACED_LENGTHS)
def test_placed_mismatches_reach_ends_and_word_boundaries(L):
    js = LC.cases()[f"placed_{L}_realistic"][0]
    f = js[0]
    at = LC.placed_at(L)
    assert len(js) == 1 + len(at) and sorted(at) == sorted(set(at)) and len(at) == (18 if L == 70 else 15)
    straddles = 0
    for q, s in zip(at, js[1:]):
        assert [p for p in range(L) if s[p] != f[p]] == [q]
        assert LM.reads_5mer(f, s, q) == (2 <= q <= L - 3), q
        if 2 <= q <= L - 3 and (q - 2) // 32 != (q + 2) // 32:                # the 5-mer lies in two words of the packed row
            straddles += 1
            for tab in ("realistic", "extreme"):
                table = LC.tables()[tab]
                assert LM.distance(f, s, table) == int(table[LC._index5(f[q - 2:q + 3])]["ACGT".index(s[q])]) + int(table[LC._index5(s[q - 2:q + 3])]["ACGT".index(f[q])])
    assert straddles == (8 if L == 70 else 7), straddles                       # 30 .. 33 and 62 .. 65 (at L = 67, 65 = L - 2 has no 5-mer)
    for tab in ("realistic", "extreme"):                                       # some placed copies are linked to the founder, some are not
        clone = LC.models()[f"placed_{L}_{tab}", "avg"][0]
        D = LM.distance_matrix(js, LC.tables()[tab])[0][0, 1:]
        assert (D <= 2000).any() and (D > 2000).any() and LC.cases()[f"placed_{L}_{tab}"][2] == (1, L), (tab, D.tolist())
        assert 1 <= len(set(clone.tolist())) < len(js)


def test_other_characters_sit_at_and_beside_the_mismatch():
    js, grp, md, tab = LC.cases()["not_acgt_extreme"]
    f, g, h = js[:3]
    seen = set()
    for s in js[3:]:
        bad = [p for p, ch in enumerate(s) if ch not in "ACGT"]
        assert len(bad) == 1
        base = s[:bad[0]] + s[bad[0]].upper().replace("N", f[bad[0]]) + s[bad[0] + 1:]
        near = 20 if abs(bad[0] - 20) <= 2 else 32
        assert abs(bad[0] - near) <= 2
        seen.add((bad[0] - near, s[bad[0]] == "N", near))
        # the position of the bad character costs the mean on both sides, and it voids the 5-mer of every position within two of it
        for other in (f, g, h):
            for p in range(max(0, bad[0] - 2), min(len(s), bad[0] + 3)):
                assert LM._side(s, other, p, LC.tables()[tab]) == LM.MISS
            assert LM._side(other, s, bad[0], LC.tables()[tab]) == LM.MISS
    assert seen == {(d, n, at) for d in range(-2, 3) for n in (True, False) for at in (20, 32)}
    for name in ("not_acgt_realistic", "not_acgt_extreme"):
        clone, near, info, _ = LC.models()[name, "avg"]
        assert info["items"] == len(js) and 0 < info["links"] < info["pairs"] and (near > 0).all()      # some pairs within D <= 2400, some past it


def test_sizes_lengths_and_the_large_bucket():
    c = LC.cases()
    assert [len(c[f"size_{m}"][0]) for m in LC.SIZES] == LC.SIZES == [1, 2, 63, 64, 65, 129]
    assert LC.LENGTHS == [1, 3, 4, 5, 6, 31, 32, 33, 34, 35, 64, 65, 96, 255] and all({len(s) for s in c[f"len_{L}"][0]} == {L} for L in LC.LENGTHS)
    for m in LC.SIZES[2:]:
        info = LC.models()[f"size_{m}", "avg"][2]
        assert 1 < info["clones"] < info["items"] and info["links"] > 0
    js, grp, md, tab = c[LC.BIG]
    assert len(js) == 4097 and {len(s) for s in js} == {45} and LM.slice_width([4097]) == 128 and js[0] == js[4096]
    for sym in LM.SYMMETRY:
        clone, near, info, walked = LC.models()[LC.BIG, sym]
        assert clone[4096] == clone[0] == 0 and np.bincount(clone).max() >= 100 and info["links"] >= 130 + 4 and (near > 0).all()
        assert 0 < walked < 2 * info["pairs"]                                  # the pre-filter leaves some pairs and walks others
    info = LC.models()["interleaved", "avg"][2]
    assert info["buckets"] == 5 and info["largest_bucket"] == 90 and info["items"] == 276
    assert sorted(LC.permutation()) == list(range(276)) and LC.permutation() != list(range(276))


# ---- the command line, up to where a GPU would be needed ---------------------------------------------------------------------------------
def _refused(r, tmp_path):
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr, r.stderr[-500:]
    assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
    assert not (tmp_path / "l.tsv").exists()


def test_cli_refusals(tmp_path):
    from vdjer_amd import annot
    annot.write_targeting(str(tmp_path / "t.tsv"), LC.weights()["realistic"])
    r = _run(tmp_path, ["--lineage-model", "t.tsv"])
    _refused(r, tmp_path)
    assert "--lineage-model is the distance model of the --lineages table: it needs --lineages <file>" in r.stderr
    r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-symmetry", "min"])
    _refused(r, tmp_path)
    assert "--lineage-symmetry is the symmetry of the --lineage-model distance: it needs --lineage-model <file>" in r.stderr
    for value in ("max", "AVG", ""):
        r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-model", "t.tsv", "--lineage-symmetry", value])
        _refused(r, tmp_path)
        assert f"--lineage-symmetry must be avg (both directions added) or min (twice the cheaper): {value}" in r.stderr
    r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-model", "none.tsv"])
    _refused(r, tmp_path)
    assert "--lineage-model: cannot read none.tsv" in r.stderr
    lines = (tmp_path / "t.tsv").read_text().splitlines()
    for change, message in ((lambda ls: ls[:7] + ["AACGX\t1\t1\t1\t1"] + ls[8:], "--lineage-model: bad.tsv line 8: expected `<5-mer over ACGT> <wA> <wC> <wG> <wT>`"),
                            (lambda ls: ls + [ls[3]], "--lineage-model: bad.tsv line 1025: the 5-mer AAAAT is given twice"),
                            (lambda ls: ls[:-1], "--lineage-model: bad.tsv holds 1023 5-mers, expected every one of the 1024 once")):
        (tmp_path / "bad.tsv").write_text("\n".join(change(lines)) + "\n")
        r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-model", "bad.tsv"])
        _refused(r, tmp_path)
        assert message in r.stderr, r.stderr[-600:]
    # (--targeting's own messages keep their flag's name)
    r = _run(tmp_path, ["--selection", "s.tsv", "--targeting", "none.tsv"])
    assert r.returncode != 0 and "--targeting: cannot read none.tsv" in r.stderr


# ---- the ABI mirror -----------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_documents():
    import inspect
    from vdjer_amd import _lib, api
    assert ctypes.sizeof(_lib.LineageModelParams) == 12 and ctypes.sizeof(_lib.LineageTableInfo) == 16
    for s in ("vdjx_lineage_model", "vdjx_lineage_distance_table"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)
    sig = inspect.signature(api.Context.lineage)
    assert list(sig.parameters)[1:] == ["junctions", "group", "max_dist", "nearest", "table", "symmetry"]
    assert sig.parameters["table"].default is None and sig.parameters["symmetry"].default == "avg" and sig.parameters["max_dist"].default == (1500, 10000)
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text in (header, readme):
        assert "substitution-model (HH_S5F)" not in text and "amino-acid" in text and "padding with N-averaged 5-mers" in text
    assert "--lineage-model" in readme and "--lineage-symmetry" in readme and "lineage_model_walked" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_lin_pairs_model" in design and "profiles/lineage_model_at_size.json" in design
    source = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_lineage.hip")).read()
    assert 'vdjx_prof_scope ps(c, "k_lin_pairs_model")' in source and 'vdjx_prof_scope ps(c, "k_lin_pairs")' in source
