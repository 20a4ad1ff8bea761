"""Without a GPU: vdjx_targeting_model (plain C) against the Python model of tests/targeting_model.py for every written integer, the file
round trip, the command line's refusals, the ABI mirror, and the proof that every case of tests/test_gpu_targeting.py and
tests/test_gpu_targeting_cli.py reaches what it is for."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import mutation_model as M
from tests import selection_cases as SC
from tests import selection_model as S
from tests import targeting_cases as TC
from tests import targeting_model as T
from tests import test_gpu_mutation as TM
from tests.test_isotype_cpu import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model finish ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls,min_sub,min_mut", [("levels", "s", 50, 500), ("levels", "rs", 50, 500), ("rs", "s", 50, 500), ("rs", "rs", 50, 500),
                                                     ("rs", "rs", 1, 1), ("zeros", "s", 50, 500), ("zeros", "rs", 1, 1), ("no_opp", "s", 1, 1),
                                                     ("no_opp", "rs", 1, 1), ("exact", "s", 50, 500), ("exact", "s", 51, 501),
                                                     ("levels", "s", (1 << 32) - 1, (1 << 32) - 1)])
def test_c_finish_equals_model(name, cls, min_sub, min_mut):
    from vdjer_amd import annot
    cnt = TC.finish_counts()[name]
    w, lv = annot.targeting_model(cnt, cls, min_sub, min_mut)
    mw, mlv = T.model(cnt, cls, min_sub, min_mut)
    assert w.dtype == np.uint32 and w.shape == (1024, 4) and lv.dtype == np.uint8 and lv.shape == (1024, 2)
    assert np.array_equal(lv, mlv), np.argwhere(lv != mlv)[:5].tolist()
    assert np.array_equal(w, mw), [(m, w[m].tolist(), mw[m].tolist()) for m in np.flatnonzero((w != mw).any(axis=1))[:5]]
    for m in range(1024):                                             # no 5-mer has a zero row; the centre's entry is 0
        c = m >> 4 & 3
        assert w[m, c] == 0 and all(w[m, x] >= 1 for x in range(4) if x != c)


def test_finish_cases_reach_their_levels():
    fc = TC.finish_counts()
    for cls in ("s", "rs"):
        _, lv = T.model(fc["levels" if cls == "s" else "rs"], cls)
        for t in range(2):
            assert set(lv[:, t].tolist()) == {5, 3, 1, 0}, (cls, t, T.level_counts(lv))
    w, lv = T.model(fc["zeros"])
    assert set(lv.ravel().tolist()) == {0}
    off = [int(w[m, x]) for m in range(1024) for x in range(4) if x != (m >> 4 & 3)]
    assert len(set(off)) == 1 and off[0] == round(1e9 / 1024 / 3)    # every off-centre weight equal
    # observed changes without an opportunity under class s: no level-5 mutability there, with class rs there is
    assert int(fc["no_opp"][0, 0, 5].sum()) >= 1 and int(fc["no_opp"][1, 0, 5].sum()) == 0
    assert T.model(fc["no_opp"], "s", 1, 1)[1][5, 1] != 5 and T.model(fc["no_opp"], "rs", 1, 1)[1][5, 1] == 5
    # a minimum met exactly is met; one below is not
    lv = T.model(fc["exact"], "s", 50, 500)[1]
    assert (lv[0, 0], lv[1, 0], lv[512, 1], lv[513, 1]) == (5, 3, 5, 3)
    lv = T.model(fc["exact"], "s", 51, 501)[1]
    assert lv[0, 0] != 5 and lv[512, 1] != 5


def test_python_refuses_bad_arguments():
    from vdjer_amd import annot
    z = np.zeros((2, 2, 1024, 4), np.uint64)
    for kw in (dict(cls="r"), dict(min_sub=0), dict(min_mut=1 << 32), dict(min_sub=1.5)):
        with pytest.raises(ValueError):
            annot.targeting_model(z, **kw)
    with pytest.raises(ValueError):
        annot.targeting_model(z[0])
    L = __import__("vdjer_amd._lib", fromlist=["lib"]).lib()
    w, lv = np.zeros((1024, 4), np.uint32), np.zeros((1024, 2), np.uint8)
    for cls, a, b in ((2, 1, 1), (0, 0, 1), (0, 1, 0)):
        assert L.vdjx_targeting_model(z.ctypes.data, cls, a, b, w.ctypes.data, lv.ctypes.data) != 0
        assert b"vdjx_targeting_model: " in L.vdjx_last_error()
    assert L.vdjx_targeting_model(None, 0, 1, 1, w.ctypes.data, lv.ctypes.data) != 0 and b"NULL argument" in L.vdjx_last_error()


# ---- the file --------------------------------------------------------------------------------------------------------------------------------
def test_write_targeting_round_trip(tmp_path):
    from vdjer_amd import annot
    w = SC.weights()
    p = tmp_path / "t.tsv"
    annot.write_targeting(str(p), w, comments=("class s", "made by hand"))
    assert np.array_equal(annot.read_targeting(str(p)), w)
    lines = p.read_text().split("\n")
    assert lines[-1] == "" and lines[:2] == ["# class s", "# made by hand"]
    rows = [l.split("\t") for l in lines[2:-1]]
    # the C reader's rules: 1,024 lines of five fields, each 5-mer over ACGT once (here in index order), whole numbers below 2^32
    assert len(rows) == 1024 and [r[0] for r in rows] == [T.kmer(m) for m in range(1024)] and len(set(r[0] for r in rows)) == 1024
    assert all(len(r) == 5 and all(re.fullmatch(r"\d+", x) and int(x) < 1 << 32 for x in r[1:]) for r in rows)
    assert [annot.kmer5(m) for m in (0, 1, 27, 1023)] == ["AAAAA", "AAAAC", "AACGT", "TTTTT"] and T.index5("AACGT") == 27
    # the model's text is that format too
    wm, lv = T.model(TC.finish_counts()["levels"])
    info = dict(units=3, positions=4, obs_s=5, obs_r=6, opp_s=7, opp_r=8)
    (tmp_path / "m.tsv").write_text(T.model_text("x", "s", 50, 500, info, wm, lv))
    assert np.array_equal(annot.read_targeting(str(tmp_path / "m.tsv")), wm)
    with pytest.raises(ValueError):
        annot.write_targeting(str(p), w[:1000])


# ---- the ABI mirror ------------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_exports():
    from vdjer_amd import _lib, api
    assert ctypes.sizeof(_lib.TgtInfo) == 80
    assert [f for f, _ in _lib.TgtInfo._fields_][:-1] == list(api.Context.TGT_INFO_FIELDS) == T.INFO
    for s in ("vdjx_targeting_counts", "vdjx_targeting_model"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)
    assert callable(api.Context.targeting_counts)
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    for word in ("per-sequence normalisation", "N-extended", "multipleMutation", "clonal consensus", "UNION"):
        assert word in header, word
    source = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_target.hip")).read()
    assert re.search(r'vdjx_env_num\("VDJX_TGT_UNITS", 1 << 18, 1, \(1 << 20\) - 1\)', source)
    assert "VDJX_TGT_UNITS" in open(os.path.join(ROOT, "README.md")).read()


# ---- the command line, up to where a GPU would be needed -----------------------------------------------------------------------------------
def _refused(r, tmp_path):
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr, r.stderr[-500:]
    assert "Invalid param" not in r.stderr and "Missing value" not in r.stderr
    assert not (tmp_path / "t.tsv").exists() and not (tmp_path / "c.tsv").exists()


@pytest.mark.parametrize("flag,value,what", [("--targeting-class", "s", "mutation class"), ("--targeting-min-sub", "50", "threshold"),
                                             ("--targeting-min-mut", "500", "threshold"), ("--targeting-counts", "c.tsv", "counts")])
def test_cli_options_need_targeting_model(tmp_path, flag, value, what):
    r = _run(tmp_path, [flag, value])
    _refused(r, tmp_path)
    assert flag in r.stderr and what in r.stderr and "it needs --targeting-model <file>" in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("extra,message", [(["--targeting-class", "r"], "--targeting-class must be s (silent changes only) or rs (silent and replacement): r"),
                                           (["--targeting-class", "sr"], "--targeting-class must be s"),
                                           (["--targeting-min-sub", "0"], "--targeting-min-sub must be a whole decimal number in 1 .. 4294967295: 0"),
                                           (["--targeting-min-sub", "4294967296"], "--targeting-min-sub must be a whole decimal number in 1 .. 4294967295: 4294967296"),
                                           (["--targeting-min-sub", "5.0"], "--targeting-min-sub must be a whole decimal number"),
                                           (["--targeting-min-mut", "0"], "--targeting-min-mut must be a whole decimal number in 1 .. 4294967295: 0"),
                                           (["--targeting-min-mut", "-3"], "--targeting-min-mut must be a whole decimal number"),
                                           (["--targeting-min-mut", "99999999999999999999999"], "--targeting-min-mut must be a whole decimal number")])
def test_cli_refuses_bad_values(tmp_path, extra, message):
    r = _run(tmp_path, ["--targeting-model", "t.tsv"] + extra)
    _refused(r, tmp_path)
    assert message in r.stderr, r.stderr[-500:]


# ---- the GPU cases reach what they are for ---------------------------------------------------------------------------------------------------
def test_count_cases_share_selections_opportunities():
    """with unit weights and every contig a unit of its own, vdjx_selection's expected sums are the opportunities"""
    ct, v, lim = TC.count_inputs()
    cnt, info = TC.count_model()
    sel = S.counts(ct, v, lim, TM.germs(), None, np.ones((1024, 4), np.uint32))
    assert info["opp_s"] == sum(int(x) for x in sel["exp_s"].ravel()) > 100 and info["opp_r"] == sum(int(x) for x in sel["exp_r"].ravel()) > 300
    assert info["obs_s"] + info["obs_r"] > 20 and info["obs_s"] > 0 and info["truncated"] == 1 and info["units"] == info["used"]
    assert int(cnt[:, :, np.arange(1024), np.arange(1024) >> 4 & 3].sum()) == 0           # the centre's entries stay 0
    # positions 2 and L - 3 are the first and last with a 5-mer: the whole-record hits reach them, positions 0, 1, L - 2, L - 1 are never seen
    units, genes, _, _ = T.marks(ct, v, lim, TM.germs())
    for gene in (TM.V5, TM.V3):
        seen = set().union(*(set(bits) for key, bits in units.items() if genes[key] == gene))
        L = len(TM.germs()[gene])
        assert not seen & {0, 1, L - 2, L - 1} and (gene != TM.V5 or {2, L - 3} <= seen), gene
    assert max(p for key, bits in units.items() if genes[key] == TM.V3 for p in bits) >= 2040   # the 2,047-base record: the bitmap's last word


def test_group_cases_reach_their_rule():
    one = lambda what, grouped=True: TC.group_model(what, grouped)[1]
    obs = lambda i: i["obs_s"] + i["obs_r"]
    a, b = one("shared"), one("shared", False)
    assert (obs(a), a["units"]) == (1, 1) and (obs(b), b["units"]) == (2, 2) and b["opp_s"] > a["opp_s"]
    a = one("two_records")
    assert (obs(a), a["units"]) == (2, 2)
    a, b = one("indel_sister"), one("indel_sister", False)
    assert (obs(a), a["units"]) == (1, 1) and obs(b) == 1             # the member beside the insertion never shows it
    cs = [c for c in TC.group_cases() if c["what"] == "indel_sister"]
    ct, v, lim, grp = TC.group_inputs(cs[:1])
    assert obs(T.counts(ct, v, lim, TM.germs(), grp)[1]) == 0
    ct, v, lim, grp = TC.group_inputs(cs[1:])
    sister = T.counts(ct, v, lim, TM.germs(), grp)[1]
    assert obs(sister) == 1 and a["positions"] >= sister["positions"]
    a = one("two_alts")
    cs = [c for c in TC.group_cases() if c["what"] == "two_alts"]
    ct, v, lim, grp = TC.group_inputs(cs[:1])
    alone = T.counts(ct, v, lim, TM.germs(), grp)[1]
    assert obs(a) == 2 and (a["opp_s"], a["opp_r"], a["positions"]) == (alone["opp_s"], alone["opp_r"], alone["positions"])
    a = one("negative")
    assert (obs(a), a["units"]) == (3, 3)
    assert {c["what"] for c in TC.group_cases()} == set(TC.GROUP_NAMES)
    whole = TC.group_model()[1]
    assert whole["units"] == 1 + 2 + 1 + 1 + 3 and sorted(TC.permutation().tolist()) == list(range(len(TC.group_cases())))
    assert TC.permutation().tolist() != list(range(len(TC.group_cases())))


def test_hot_and_batch_cases():
    cnt, info = TC.hot_model()
    assert int(cnt[:, :, 1:].sum()) == 0 and info["units"] == 5 and info["positions"] > 5 * 1500       # every position in 5-mer 0
    assert int(cnt[1, 0, 0].sum()) > 0 and int(cnt[1, 1, 0, 3]) < int(cnt[1, 1, 0, 1])                  # (TAA is a stop: fewer T opportunities)
    assert all(int(cnt[0, k, 0, x]) > 0 or (k, x) == (0, 1) or (k, x) == (0, 3) for k in range(2) for x in range(1, 4))
    _, binfo = TC.batch_model()
    g = TC.group_model()[1]["units"]
    assert binfo["units"] == g + TC.SINGLES and binfo["units"] > 256   # more than one workgroup of k_tgt_count, more than one batch at 1 and 3
    assert binfo["obs_s"] > 50 and binfo["obs_r"] > 200


def test_families_cover_more_than_one_level():
    """The CLI test's input, with the V hit of every designed contig taken from the model's traceback against its clone's own record (the
    device's calls are checked against that in tests/test_mutation_cpu.py): the planted and natural changes are few, so at the defaults
    every 5-mer sits on level 0 or 1, and at minima of 1 some reach 5 and 3 -- the CLI test runs both."""
    from tests import families as F
    from tests.test_mutation_cpu import _v_hits, parsed_records, planted_families
    ids, seqs, recs, planted = planted_families()
    fam = F.build()
    _, classes, germs, _, _ = parsed_records(recs)
    _, _, germs0, _, _ = parsed_records(fam.germline)
    who, _ = F.designed(fam, ids, seqs)
    idx = [c for c, k in enumerate(who) if k is not None and len(fam.clones[k].v_names) == 1][:60]
    own = []
    for c in idx:
        hit = [r for r, cl in enumerate(classes) if cl == "V" and germs0[r] == fam.rep.v_germ[who[c]]]
        own.append(hit[0])
    sub = [seqs[c] for c in idx]
    v, _ = _v_hits(sub, germs, own)
    cnt, info = T.counts(sub, v, M.mutation_limit([ids[c] for c in idx], sub), germs)
    assert info["obs_s"] + info["obs_r"] >= 7 and info["obs_s"] >= 1
    _, lv = T.model(cnt, "rs")
    assert set(lv.ravel().tolist()) <= {0, 1}
    _, lv1 = T.model(cnt, "rs", 1, 1)
    assert len(set(lv1[:, 0].tolist())) >= 3 and len(set(lv1[:, 1].tolist())) >= 3, T.level_counts(lv1)
