"""Without a GPU: vdjx_consensus_layout and vdjx_consensus_hits (plain C) against the Python model of tests/consensus_model.py on every case
of tests/consensus_cases.py, the ABI mirror, the command line's refusals, and the proof that every case of tests/test_gpu_consensus.py
reaches the edge it is for."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import consensus_cases as CC
from tests import consensus_model as CM
from tests import targeting_cases as TC
from tests import test_gpu_mutation as TM
from tests.test_isotype_cpu import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = CC.P


def _inputs(which):
    if which == "edges":
        return CC.inputs(CC.edge_cases()), CC.edge_model()
    if which == "lone":
        return TC.group_inputs(TC.batch_cases()), CC.lone_model()
    return CC.inputs(CC.big_cases()), CC.big_model()


def hits_equal(got, want, what):
    """annot.consensus_hits' field arrays against the model's hit dicts"""
    for f in got:
        a = np.asarray(got[f], np.int64)
        b = np.array([h[f] for h in want], np.int64).reshape(a.shape)
        assert np.array_equal(a, b), (what, f, np.argwhere(a != b)[:4].tolist())


# ---- the two plain-C functions against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["edges", "lone", "big"])
def test_c_layout_equals_model(which):
    from vdjer_amd import annot
    (ct, v, lim, grp), want = _inputs(which)
    unit, units, cols = annot.consensus_layout(v, len(ct[0]), lim, grp)
    assert unit.dtype == np.int32 and unit.tolist() == want["unit"]
    for f in CM.UNIT:
        assert units[f].tolist() == want["units"][f], (which, f)
    assert cols == want["info"]["columns"] == sum(len(c) for c in want["cons"])
    # limit None is the contigs' length; group None leaves every contig on its own
    free = CM.consensus(ct, v, TM.germs(), None, None)
    unit, units, cols = annot.consensus_layout(v, len(ct[0]))
    assert unit.tolist() == free["unit"] and cols == free["info"]["columns"] and all(units[f].tolist() == free["units"][f] for f in CM.UNIT)
    assert set(free["units"]["group"]) == {-1} and set(free["units"]["members"]) == {1}


@pytest.mark.parametrize("which,freq", [("edges", CM.DEFAULT), ("edges", CC.MOST_COMMON), ("lone", CM.DEFAULT), ("big", CM.DEFAULT)])
def test_c_hits_equal_model(which, freq):
    from vdjer_amd import annot
    (ct, v, lim, grp), want = _inputs(which)
    if freq != CM.DEFAULT:
        want = CC.edge_model(freq)
    contigs, hv = annot.consensus_hits({f: np.array(want["units"][f]) for f in CM.UNIT}, want["cons"], want["germ"])
    mc, mh = CM.hits(want["units"], want["cons"], want["germ"])
    assert contigs == mc and len({len(c) for c in contigs}) == 1
    hits_equal(hv, mh, which)
    # what vh_check asks of a hit, restated: the runs add up to the positions, inside the record and the pseudo-contig
    g = TM.germs()
    for u, h in enumerate(mh):
        if h["gene"] < 0:
            assert h["score"] == 0 and not want["cons"][u].replace("-", "")
            continue
        assert h["score"] >= 1 and h["n_tied"] == 1 and h["ins"] == 0 and h["seq_start"] == 1 and 1 <= h["seq_end"] <= len(contigs[u])
        assert 1 <= h["germ_start"] <= h["germ_end"] <= len(g[h["gene"]])
        if h["n_runs"] <= 64:
            runs = [(r & 15, r >> 4) for r in h["runs"][:h["n_runs"]]]
            assert all(op in (0, 2) and L > 0 for op, L in runs) and all(a[0] != b[0] for a, b in zip(runs, runs[1:])) and runs[0][0] == runs[-1][0] == 0
            assert sum(L for op, L in runs if op == 0) == h["seq_end"] == h["matches"] + h["mismatches"]
            assert sum(L for op, L in runs) == h["germ_end"] - h["germ_start"] + 1 and sum(L for op, L in runs if op == 2) == h["del"]
            assert h["opens"] == sum(op == 2 for op, _ in runs)
        else:
            assert not any(h["runs"])


def test_python_and_c_refusals():
    from vdjer_amd import _lib, annot
    from vdjer_amd._lib import VdjxError
    cs = [c for c in CC.edge_cases() if c["what"] == "thr_3of5"][:2]
    ct, v, lim, grp = CC.inputs(cs)
    bad = lambda **kw: {f: (np.array([kw[f], x[1]]) if f in kw else x) for f, x in v.items()}
    for hv, msg in ((bad(seq_start=0), "contig positions 0 .."), (bad(germ_end=95), "runs hold"), (bad(n_runs=-1), "a run with an op outside 0..2"),
                    (dict(v, runs=np.array([[(90 << 4) | 3] + [0] * 63] * 2)), "a run with an op outside 0..2 or a length of 0")):
        with pytest.raises(VdjxError, match="vdjx_consensus_layout: contig [01]: the V hit") as e:
            annot.consensus_layout(hv, CC.LEN, lim, grp)
        assert msg in str(e.value), str(e.value)
    for lm in (-1, CC.LEN + 1):
        with pytest.raises(VdjxError, match="vdjx_consensus_layout: contig 1: limit"):
            annot.consensus_layout(v, CC.LEN, [CC.LEN, lm], grp)
    with pytest.raises(VdjxError, match="len=4096"):
        annot.consensus_layout(v, 4096)
    with pytest.raises(ValueError):
        annot.consensus_layout(v, CC.LEN, group=[0])
    want = CM.consensus(ct, v, TM.germs(), lim, grp)
    units = {f: np.array(want["units"][f]) for f in CM.UNIT}
    with pytest.raises(ValueError):
        annot.consensus_hits(units, want["cons"], [g[:-1] for g in want["germ"]])
    with pytest.raises(ValueError):
        annot.consensus_hits(units, [c[:-1] for c in want["cons"]], [g[:-1] for g in want["germ"]])
    L = _lib.lib()
    n = ctypes.c_int(0)
    assert L.vdjx_consensus_hits(None, 1, None, None, 0, None, None, ctypes.byref(n)) != 0 and b"vdjx_consensus_hits: NULL argument" in L.vdjx_last_error()
    assert L.vdjx_consensus_hits(None, 0, None, None, 0, None, None, ctypes.byref(n)) == 0 and n.value == 1
    un = np.zeros(1, annot._cons_unit_dtype())
    un["hi"] = 3
    out, hit = np.zeros(8, np.uint8), np.zeros(1, annot._hit_dtype())
    assert L.vdjx_consensus_hits(un.ctypes.data, 1, b"ACG", b"ACG", 2, out.ctypes.data, hit.ctypes.data, ctypes.byref(n)) != 0
    assert b"plen 2 (the longest row has 3 bases" in L.vdjx_last_error() and n.value == 3
    # no unit at all
    unit, units, cols = annot.consensus_layout(CC.hits([dict(v=TM.NONE)] * 3), 40)
    assert unit.tolist() == [-1] * 3 and cols == 0 and all(len(units[f]) == 0 for f in CM.UNIT)
    none, hv = annot.consensus_hits(units, [], [])
    assert none == [] and all(len(hv[f]) == 0 for f in annot.HIT_FIELDS)


# ---- the ABI mirror ------------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_exports():
    from vdjer_amd import _lib, annot, api
    assert ctypes.sizeof(_lib.ConsParams) == 8 and ctypes.sizeof(_lib.ConsUnit) == 32 and ctypes.sizeof(_lib.ConsInfo) == 80
    assert api.Context.CONS_UNIT.itemsize == 32 and annot._cons_unit_dtype() == api.Context.CONS_UNIT and annot._hit_dtype() == api.Context.ANNOT_HIT
    assert [f for f, _ in _lib.ConsInfo._fields_] == list(api.Context.CONS_INFO_FIELDS) == list(CM.INFO)
    assert [f for f, _ in _lib.ConsUnit._fields_] == list(api.Context.CONS_UNIT.names) == list(CM.UNIT) == list(annot.CONS_UNIT_FIELDS)
    for s in ("vdjx_consensus_layout", "vdjx_consensus", "vdjx_consensus_hits"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)
    assert callable(api.Context.consensus) and callable(annot.consensus_layout) and callable(annot.consensus_hits)
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    for word in ("mostMutated / leastMutated / catchAll", "ambiguity codes and stochastic tie-breaking", "inserted bases", "J segment or the junction",
                 "CreateGermlines --cloned's choice among tied V calls", "vdjx_consensus_layout(", "vdjx_consensus_hits(", "VDJX_CONS_CELLS"):
        assert word in header, word
    source = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_consensus.hip")).read()
    assert re.search(r'vdjx_env_num\("VDJX_CONS_CELLS", 1 << 24, 1, 1 << 28\)', source) and f"#define CONS_SHARE {CM.SHARE}" in source
    assert "vh_hit_segments(" in source and "float" not in source.replace("floating point", "") and "double" not in source
    readme = open(os.path.join(ROOT, "README.md")).read()
    for word in ("VDJX_CONS_CELLS", "--consensus-min-freq", "mostMutated"):
        assert word in readme, word


# ---- the command line, up to where a GPU would be needed -----------------------------------------------------------------------------------
def _refused(r, tmp_path):
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr, r.stderr[-500:]
    assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
    assert not (tmp_path / "c.tsv").exists() and not (tmp_path / "l.tsv").exists()


def test_cli_consensus_needs_lineages(tmp_path):
    r = _run(tmp_path, ["--consensus", "c.tsv"])
    _refused(r, tmp_path)
    assert "--consensus is the consensus of every lineage of the --lineages table: it needs --lineages <file>" in r.stderr, r.stderr[-500:]


def test_cli_min_freq_needs_consensus(tmp_path):
    r = _run(tmp_path, ["--lineages", "l.tsv", "--consensus-min-freq", "0.5"])
    _refused(r, tmp_path)
    assert "--consensus-min-freq is the threshold of the --consensus table: it needs --consensus <file>" in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("value", ["1.5", "0.60000", "-0.6", "6e-1", "", "0,6", " 0.6", "10"])
def test_cli_refuses_bad_min_freq(tmp_path, value):
    from vdjer_amd import annot
    r = _run(tmp_path, ["--lineages", "l.tsv", "--consensus", "c.tsv", "--consensus-min-freq", value])
    _refused(r, tmp_path)
    assert f"--consensus-min-freq must be a decimal in [0, 1] with at most four digits after the point: {value}" in r.stderr, r.stderr[-500:]
    with pytest.raises(ValueError):                                   # read exactly as --lineage-dist reads its decimal
        annot.parse_lineage_dist(value)


# ---- the cases reach their edges -------------------------------------------------------------------------------------------------------------
def _col(m, p=P, u=0):
    """(consensus character, cover, best) of record position p of unit u"""
    k = p - m["units"]["lo"][u]
    return m["cons"][u][k], m["cover"][u][k], m["best"][u][k]


def test_threshold_edges():
    g0 = TM.germs()[TM.V0][P]
    x, y = CC.alt(g0, 1), CC.alt(g0, 2)
    _, at6, common = CC.edge("thr_3of5")
    assert _col(at6) == (x, 5, 3) and 3 * 10000 == 6000 * 5          # equality passes
    _, at6, common = CC.edge("thr_5of9")
    assert _col(at6) == ("N", 9, 5) and _col(common) == (x, 9, 5) and at6["info"]["undecided"] == 1
    _, at6, common = CC.edge("thr_5of10")
    assert _col(at6) == ("N", 10, 5) and _col(common) == (x, 10, 5)   # one vote below equality
    _, at6, _ = CC.edge("thr_6of10")
    assert _col(at6) == (x, 10, 6)
    # every other column of these units is the germline's, whatever the threshold
    assert at6["cons"][0][:P] == at6["germ"][0][:P] == TM.germs()[TM.V0][:P] and at6["info"]["undecided"] == 0


def test_tie_edges():
    g0 = TM.germs()[TM.V0][P]
    _, at6, common = CC.edge("tie_germ")
    assert _col(common) == (g0, 4, 2) and _col(at6) == ("N", 4, 2)
    _, at6, common = CC.edge("tie_other")
    assert _col(common) == ("N", 4, 2) and common["info"]["undecided"] == 1
    cs, at6, common = CC.edge("tie_gap")
    assert _col(common) == ("N", 4, 2) and g0 not in {c["contig"][TC._index(CC.PLAIN, P)] for c in cs[2:]}
    assert common["cons"][0][P - 1] == TM.germs()[TM.V0][P - 1] and common["cons"][0][P + 1] == TM.germs()[TM.V0][P + 1]


def test_n_votes_and_holes():
    g0 = TM.germs()[TM.V0][P]
    _, at6, common = CC.edge("n_votes")
    assert _col(common) == (g0, 3, 1) and _col(at6) == ("N", 3, 1)    # N votes raise cover and never win
    _, at6, common = CC.edge("all_n")
    assert _col(common) == ("N", 3, 0) and _col(at6) == ("N", 3, 0) and common["info"]["undecided"] == 1
    _, at6, common = CC.edge("hole")
    assert at6["units"]["lo"] == [0] and at6["units"]["hi"] == [70] and at6["cons"][0][30:40] == "N" * 10 and at6["cover"][0][30:40] == [0] * 10
    assert at6["info"]["undecided"] == 0 and at6["germ"][0] == TM.germs()[TM.V0][:70] and set(at6["cover"][0][:30] + at6["cover"][0][40:]) == {1}


def test_indel_edges():
    rec = TM.germs()[TM.V0]
    _, won, _ = CC.edge("del_won")
    assert won["cons"][0][30:32] == "--" and won["best"][0][30:32] == [2, 2] and won["cover"][0][30:32] == [3, 3]
    _, lost, _ = CC.edge("del_lost")
    assert lost["cons"][0][30:32] == rec[30:32] and lost["best"][0][30:32] == [2, 2]
    _, at, _ = CC.edge("del_at_limit")                                # q == limit: the deletion does not vote
    assert at["units"]["hi"] == [30] and "-" not in at["cons"][0]
    _, below, _ = CC.edge("del_below_limit")                          # q == limit - 1: it votes, and so does the one base after it
    assert below["units"]["hi"] == [33] and below["cons"][0][30:] == "--" + rec[32]
    _, ins, _ = CC.edge("ins")
    assert ins["info"]["inserted"] == 2 and ins["cons"][0] == rec[:71] and ins["info"]["columns"] == 71
    _, cut, _ = CC.edge("ins_cut")
    assert cut["info"]["inserted"] == 1 and cut["units"]["hi"] == [31]


def test_limit_and_record_edges():
    _, m, _ = CC.edge("above_alone")
    assert m["info"]["units"] == 1 and m["units"]["lo"] == m["units"]["hi"] == [0] and m["cons"] == [""] and m["units"]["members"] == [1]
    _, m, _ = CC.edge("above_sister")
    assert m["units"]["members"] == [2] and set(m["cover"][0]) == {1} and m["units"]["hi"] == [90]
    _, m, _ = CC.edge("record_2to1")
    assert m["units"]["gene"] == [TM.V0] and m["units"]["members"] == [2] and m["units"]["off_record"] == [1] and m["unit"] == [0, -1, 0]
    _, m, _ = CC.edge("record_tie")
    assert m["units"]["gene"] == [TM.V0] and TM.V0 < TM.V5 and m["unit"] == [-1, 0] and m["info"]["off_record"] == 1
    _, m, _ = CC.edge("truncated")
    assert m["info"]["truncated"] == 1 and m["info"]["used"] == 1 and m["units"]["members"] == [1]


def test_hits_edges():
    _, m, _ = CC.edge("runs127")
    (pc,), (h,) = CM.hits(m["units"], m["cons"], m["germ"])
    assert h["n_runs"] == 127 and not any(h["runs"]) and h["del"] == 63 and h["seq_end"] == 64 and (h["germ_start"], h["germ_end"]) == (1, 127)
    _, m, _ = CC.edge("end_gaps")
    (pc,), (h,) = CM.hits(m["units"], m["cons"], m["germ"])
    assert m["cons"][0].startswith("--") and m["cons"][0].endswith("---") and m["units"]["lo"] == [10] and m["units"]["hi"] == [45]
    assert (h["germ_start"], h["germ_end"], h["n_runs"], h["del"], h["opens"], h["seq_end"]) == (13, 42, 1, 0, 0, 30) and pc == TM.germs()[TM.V0][12:42]
    _, m, _ = CC.edge("no_base")
    (pc,), (h,) = CM.hits(m["units"], m["cons"], m["germ"])
    assert m["cons"] == ["---"] and h["gene"] == -1 and h["score"] == 0 and pc == "N"


def test_whole_sets():
    m = CC.edge_model()
    assert m["info"]["batches"] == 1 and CC.edge_model(CM.DEFAULT, 1)["info"]["batches"] == m["info"]["units"] > 20
    assert 1 < CC.lone_model(4096)["info"]["batches"] < 10 and CC.lone_model(1)["info"]["batches"] == CC.lone_model()["info"]["units"]
    assert sorted(CC.permutation().tolist()) == list(range(len(CC.edge_cases()))) and CC.permutation().tolist() != list(range(len(CC.edge_cases())))
    lone = CC.lone_model()
    assert lone["info"]["units"] >= TC.SINGLES and lone["units"]["members"].count(1) >= TC.SINGLES
    big = CC.big_model()
    assert big["info"]["units"] == 1 and big["units"]["members"] == [CC.BIG_VOTERS] and big["info"]["large_units"] == 1
    assert (big["units"]["lo"], big["units"]["hi"]) == ([0], [TC.HOT_LEN]) and max(big["cover"][0]) > 40 and "-" not in big["cons"][0]
    diff = sum(a != b for a, b in zip(big["cons"][0], big["germ"][0]))
    assert 40 <= diff <= 62                                           # the shared changes win, the private ones do not


def test_families_lineages_show_lone_voters_and_off_record_members():
    """The CLI test's input: every clone of the e2e_families golden has a V sequence of its own, so contigs of different clones that a
    lineage holds name different records -- the record majority is a tie, the lowest record wins, one member votes and the others are
    off the record.  Here with the V hit of one designed contig per clone taken from the model's traceback against its clone's own record
    (the device's calls are checked against that in tests/test_mutation_cpu.py) and three clones to a group."""
    from tests import families as F
    from tests import mutation_model as M
    from tests.test_mutation_cpu import _v_hits, parsed_records, planted_families
    ids, seqs, recs, planted = planted_families()
    fam = F.build()
    _, classes, germs, _, _ = parsed_records(recs)
    _, _, germs0, _, _ = parsed_records(fam.germline)
    who, _ = F.designed(fam, ids, seqs)
    first = {}
    for c, k in enumerate(who):
        if k is not None and len(fam.clones[k].v_names) == 1:
            first.setdefault(k, c)
    idx = sorted(first.values())[:24]
    own = [[r for r, cl in enumerate(classes) if cl == "V" and germs0[r] == fam.rep.v_germ[who[c]]][0] for c in idx]
    assert len(idx) == 24 and len(set(own)) == len(own)               # a V record of its own per clone
    sub = [seqs[c] for c in idx]
    v, _ = _v_hits(sub, germs, own)
    grp = np.arange(len(idx)) // 3
    res = CM.consensus(sub, v, germs, M.mutation_limit([ids[c] for c in idx], sub), grp)
    assert res["info"]["units"] == 8 and res["units"]["members"] == [1] * 8 and res["units"]["off_record"] == [2] * 8
    assert res["units"]["gene"] == [min(own[3 * u:3 * u + 3]) for u in range(8)] and res["info"]["undecided"] == 0
    assert all(set(cv) == {1} for cv in res["cover"]) and all(len(c) > 100 for c in res["cons"])
