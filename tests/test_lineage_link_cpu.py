"""vdjx_lineage_link without a GPU: the model of tests/lineage_link_model.py on its own -- its clusters refine the single-linkage partition,
every pair inside a complete-linkage cluster is linked, linkage single is tests/lineage_model.py's partition, the handmade cases give the
partitions written beside them in tests/lineage_link_cases.py --, every size case really crossing the boundary it is named for (so that no
device test passes vacuously), the batches, the ABI mirror and the documents, and the command line up to where a GPU would be needed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import lineage_dist_model as LM
from tests import lineage_link_cases as KC
from tests import lineage_link_model as KM
from tests import lineage_model as M
from tests.test_isotype_cpu import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(KC.cases())


def _parts(clone):
    return sorted(sorted(p) for p in M.partition(clone))


# ---- the model on its own ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_clusters_refine_single_linkage(name):
    """the model agglomerates whole buckets: that no cluster crosses two single-linkage components is a result here, not an assumption"""
    single = KC.model(name, "single")[0]
    for linkage in KC.LINKAGES:
        clone, nearest, info, link = KC.model(name, linkage)
        assert ((clone >= 0) == (single >= 0)).all()
        for part in M.partition(clone):
            assert len({int(single[i]) for i in part}) == 1, (name, linkage)
        assert info["clones"] == len(M.partition(clone)) >= link["clones_single"] == len(M.partition(single))
        assert link["merges"] == info["items"] - info["clones"]
        assert nearest.tobytes() == KC.model(name, "single")[1].tobytes()
        first = [min(p) for p in M.partition(clone)]
        assert [int(clone[i]) for i in sorted(first)] == list(range(len(first)))          # numbered by the smallest member


@pytest.mark.parametrize("name", NAMES)
def test_complete_linkage_links_every_pair_inside_a_cluster(name):
    js, grp, (num, den), tab, sym = KC.cases()[name]
    clone = KC.model(name, "complete")[0]
    unit = 1 if tab is None else 2000
    for part in M.partition(clone):
        part = sorted(part)
        for x, a in enumerate(part):
            for b in part[x + 1:]:
                d = M.distance(js[a], js[b]) if tab is None else LM.distance(js[a], js[b], KC.table_of(tab), sym)
                assert d * den <= unit * num * len(js[a]), (name, a, b, d)


@pytest.mark.parametrize("name", NAMES)
def test_linkage_single_is_the_lineage_model(name):
    js, grp, md, tab, sym = KC.cases()[name]
    clone, nearest, info, link = KC.model(name, "single")
    want = M.lineage(js, grp, md) if tab is None else LM.lineage(js, grp, KC.table_of(tab), md, sym)[:3]
    assert clone.tobytes() == want[0].tobytes() and nearest.tobytes() == want[1].tobytes() and info == want[2]
    assert link == dict.fromkeys(KM.LINK_FIELDS, 0)


@pytest.mark.parametrize("name", list(KC.HANDMADE))
def test_handmade_partitions(name):
    for linkage, want in KC.HANDMADE[name].items():
        assert _parts(KC.model(name, linkage)[0]) == want, (name, linkage)


def test_handmade_distances_are_what_the_cases_say():
    d = M.distance
    a, b, c = KC.TIE
    assert (d(a, b), d(b, c), d(a, c)) == (2, 2, 4) and 2 * 10000 <= 1000 * 20 < 3 * 10000
    a, b, c = KC.EQUAL
    assert (d(a, b), d(a, c), d(b, c)) == (1, 2, 3) and 5 * 10000 == 1000 * 25 * 2 and 3 * 10000 > 1000 * 25
    assert _parts(KC.model("tie", "single")[0]) == [[0, 1, 2]] == _parts(KC.model("exact_equality", "single")[0])
    js = KC.cases()["identical_with_n"][0]
    assert d(js[0], js[1]) == 1                               # N never matches, not even N
    assert KC.model("chain_40", "single")[2]["clones"] == 1 and KC.model("chain_40", "complete")[2]["clones"] > 1
    assert KC.model("num_is_den", "complete")[2]["clones"] == 1
    n0 = KC.model("num_0", "complete")
    assert n0[0].tobytes() == KC.model("num_0", "single")[0].tobytes() == KC.model("num_0", "average")[0].tobytes() and n0[3]["merges"] > 0


@pytest.mark.parametrize("m", KC.SIZES)
def test_size_cases_cross_their_boundary(m):
    name = f"size_{m}"
    for linkage in KC.LINKAGES:
        clone, _, info, link = KC.model(name, linkage)
        assert link["largest_component"] == m and link["components"] == 2 and info["largest_bucket"] == m + 5
        assert 1 < info["clones"] < m and link["merges"] > m // 2       # the component is cut, and most of it is merged
    assert KC.model(name, "complete")[0].tobytes() != KC.model(name, "average")[0].tobytes()
    source = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_lineage.hip")).read()
    assert f"#define LINK_LDS_M {KC.LDS_M}u" in source and "#define LINK_THREADS 256u" in source and "#define HAM_ROWS 64u" in open(
        os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_hamming.h")).read()
    assert {63, 64, 65, KC.LDS_M - 1, KC.LDS_M, KC.LDS_M + 1} <= set(KC.SIZES) and max(KC.SIZES) > 256


def test_arithmetic_cases_differ_where_they_should():
    uni, ham = KC.model("table_uniform", "average"), KM.lineage(*KC.cases()["table_uniform"][:3], "average")
    assert uni[0].tobytes() == ham[0].tobytes() and uni[3] == ham[3]            # a uniform table is 2000 x Hamming
    assert (uni[1][uni[1] >= 0] == 2000 * ham[1][ham[1] >= 0]).all()
    for linkage in KC.LINKAGES:
        assert KC.model("table_realistic", linkage)[0].tobytes() != KC.model("table_uniform", linkage)[0].tobytes()
        assert KC.model("table_extreme", linkage)[0].tobytes() != KC.model("table_uniform", linkage)[0].tobytes()
        assert KC.model("table_extreme_min", linkage)[3]["merges"] > 0
    changed = [k for k in range(KC.RANDOM) if KC.model(f"random_{k}", "complete")[0].tobytes() != KC.model(f"random_{k}", "average")[0].tobytes()]
    assert len(changed) >= KC.RANDOM // 2
    assert max(max(np.bincount(np.asarray(grp)[np.asarray(grp) != M.NONE])) for _, grp, *_ in (KC.cases()[f"random_{k}"] for k in range(KC.RANDOM))) <= 220


def test_batches():
    assert KM.batches([]) == 0 and KM.batches([2]) == 1 and KM.batches([2, 2], 8) == 1 and KM.batches([2, 2], 7) == 2
    assert KM.batches([3, 2, 2], 1) == 3 and KM.batches([3, 2, 2], 8) == 2 and KM.batches([2, 2, 3], 8) == 2 and KM.batches([2, 3, 2], 8) == 3
    sizes = KC.component_sizes(KC.BATCHED)
    knob = KC.splitting_knob(KC.BATCHED)
    assert len(sizes) >= 4 and 1 < KM.batches(sizes, knob) < len(sizes) == KM.batches(sizes, 1)
    for k in (1, knob):
        for linkage in KC.LINKAGES:
            got, ref = KC.model(KC.BATCHED, linkage, k), KC.model(KC.BATCHED, linkage)
            assert got[0].tobytes() == ref[0].tobytes() and got[3] == dict(ref[3], batches=KM.batches(sizes, k))


# ---- the ABI mirror and the documents ----------------------------------------------------------------------------------------------------
def test_abi_mirror_and_documents():
    from vdjer_amd import _lib, annot, api
    assert ctypes.sizeof(_lib.LineageLinkParams) == 16 and ctypes.sizeof(_lib.LineageLinkInfo) == 32 and _lib.LineageLinkInfo.cells.offset == 24
    assert [f for f, _ in _lib.LineageLinkParams._fields_] == ["num", "den", "symmetry", "linkage"]
    assert [f for f, _ in _lib.LineageLinkInfo._fields_] == ["components", "largest_component", "merges", "clones_single", "batches", "reserved", "cells"]
    assert "vdjx_lineage_link" in _lib.SYMBOLS and hasattr(_lib.lib(), "vdjx_lineage_link")
    assert list(api.Context.LINEAGE_LINK_FIELDS) == KM.LINK_FIELDS
    assert api.Context.LINEAGE_LINKAGE == annot.LINEAGE_LINKAGE == {n: k for k, n in enumerate(KM.LINKAGE)} and annot.LINEAGE_LINK_NAMES == KM.LINKAGE
    assert annot.LINEAGE_LINK_MAX == KM.MAX_M and [annot.parse_lineage_link(n) for n in KM.LINKAGE] == [0, 1, 2]
    for bad in ("", "Single", "ward", "0"):
        with pytest.raises(ValueError, match="--lineage-link must be single, complete or average"):
            annot.parse_lineage_link(bad)
    sig = inspect.signature(api.Context.lineage_link)
    assert list(sig.parameters)[1:] == list(inspect.signature(api.Context.lineage).parameters)[1:] + ["link"] and sig.parameters["link"].default == "complete"
    assert [sig.parameters[p].default for p in ("max_dist", "nearest", "table", "symmetry")] == [(1500, 10000), True, None, "avg"]
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    assert re.search(r"\bint vdjx_lineage_link\(vdjx_ctx\* ctx, const char\* junctions, const uint64_t\* off, const uint32_t\* group, size_t n,", header)
    for text in ("vdjx_lineage_link_params;   /* 16 bytes */", "vdjx_lineage_link_info;  /* 32 bytes */", "VDJX_LINK_CELLS", "Only linked components need agglomerating",
                 "Everything fits 64 bits", "depends on the caller's order"):
        assert text in header, text
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "--lineage-link" in readme and "VDJX_LINK_CELLS" in readme and "k_link_merge" in design and "profiles/lineage_link_resource_check.md" in design
    for text in (header, readme, design):
        assert "average or complete linkage" not in text and "any linkage other than single" not in text
    source = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_lineage.hip")).read()
    for kname in ("k_link_gather", "k_link_matrix", "k_link_merge"):
        assert f'vdjx_prof_scope ps(c, "{kname}")' in source
    report = open(os.path.join(ROOT, "profiles", "lineage_link_resource_check.md")).read()
    for kname in ("k_lin_pairs", "k_lin_pairs_model", "k_tree_min", "k_link_matrix", "k_link_matrix_model", "k_link_merge"):
        assert kname in report


# ---- the command line, up to where a GPU would be needed ---------------------------------------------------------------------------------
def _refused(r, tmp_path):
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr, r.stderr[-500:]
    assert "Invalid param" not in r.stderr
    assert not (tmp_path / "l.tsv").exists()


def test_cli_refusals(tmp_path):
    for value in KM.LINKAGE:
        r = _run(tmp_path, ["--lineage-link", value])
        _refused(r, tmp_path)
        assert "--lineage-link is the linkage of the --lineages table: it needs --lineages <file>" in r.stderr
    for value in ("ward", "Complete", "1", ""):
        r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-link", value])
        _refused(r, tmp_path)
        assert f"--lineage-link must be single, complete or average: {value}" in r.stderr
    r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-link"])
    assert r.returncode != 0 and "Missing value for param: --lineage-link" in r.stderr and "ELAPSED_SECS" not in r.stderr
    # the other --lineage-* flags keep their refusals beside the new one
    r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-link", "average", "--lineage-dist", "1.5"])
    _refused(r, tmp_path)
    assert "--lineage-dist must be a decimal in [0, 1] with at most four digits after the point: 1.5" in r.stderr
    r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-link", "complete", "--lineage-symmetry", "min"])
    _refused(r, tmp_path)
    assert "--lineage-symmetry is the symmetry of the --lineage-model distance" in r.stderr


def test_cli_help_names_the_flag(tmp_path):
    r = _run(tmp_path, ["--help"])
    assert "--lineage-link <single|complete|average" in r.stderr + r.stdout
