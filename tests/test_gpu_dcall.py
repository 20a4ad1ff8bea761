"""vdjx_dcall on the GPU: every vdjx_annot_hit field and the whole score matrix against the integer model of tests/dcall_model.py -- one
call per rows-per-lane count of the per-contig scoring kernel with unequal windows in every workgroup, windows that cut a D record, the
score extremes, the refusals -- and `vdjer --airr --d-calls` on a heavy-chain and a light-chain golden against the model's table.  The
API checks run in child processes, once per knob setting, as tests/test_gpu_annot.py runs them; the model is computed once."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import annot_model as A
from tests import dcall_model as D
from tests import golden_util as G
from tests.test_gpu_annot import KNOBS, RECIPES, _child_env, _mutate, _rand, _vdjer, _write_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEN = 300
LONGEST = [64, 65, 128, 129, 192, 193, 256]                          # both ends of every rows-per-lane count (1 .. 4) of the scoring kernel
EXTREMES = [dict(match=15, mismatch=31, gap_open=31, gap_extend=31, min_score=0), dict(match=1, mismatch=1, gap_open=0, gap_extend=1, min_score=22)]


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_dcall import {fn}; print('DCALL', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("DCALL ")).split(" ", 1)[1])


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def d_set():
    """[(FASTA header, sequence as given)], [cleaned sequence]: records of 37 and 11 .. 36 bases, of 1 and 2 bases, one with N, one in
    lower case, 70 one-base records in a row (the scoring kernel's ring of 32 records in flight at its bound), one of 2,047 bases (so the
    set has several chunks) and, last, a copy of record 0 (a tie across a chunk boundary)"""
    rng = np.random.default_rng(515)
    seqs = [_rand(rng, k) for k in [37] + list(range(11, 37))] + ["G", "CA"]
    with_n = _rand(rng, 30)
    seqs.append(with_n[:14] + "N" + with_n[15:])
    seqs.append(_rand(rng, 25).lower())
    seqs += ["ACGT"[k % 4] for k in range(70)]
    seqs.append(_rand(rng, 2047))
    seqs.append(seqs[0])
    recs = [(f"IGHD{k}*01 x" if k % 2 else f"D{k}", s) for k, s in enumerate(seqs)]
    return recs, [s.upper() for s in seqs]


def _plant(s, at, text):
    assert 0 <= at and at + len(text) <= len(s)
    return s[:at] + text + s[at + len(text):]


@functools.lru_cache(maxsize=None)
def row_calls():
    """per longest window L: (13 contigs of 300 bases, win_start, win_len) -- 13 is no multiple of a workgroup's four waves; every group
    of four holds windows of L, 0, 1, 2 or 37 bases; the starts include 0 and len - win_len"""
    _, recs = d_set()
    rng = np.random.default_rng(616)
    out = {}
    for L in LONGEST:
        ws = [0, LEN - L, 0, LEN - 1, 0, 100, 17, LEN, LEN - L, LEN - 37, 0, (LEN - L) // 2, LEN - 2]
        wl = [L, L, 0, 1, 2, 37, L, 0, L, 37, 1, L, 2]
        ct = [_rand(rng, LEN) for _ in range(13)]
        ct[0] = _plant(ct[0], 9, recs[0])                                            # the whole of record 0: tied with its copy in another chunk
        ct[1] = _plant(ct[1], LEN - L + 20, _mutate(rng, recs[25], 2)[:36])        # a mutated copy
        ct[3] = ct[3][:-1] + "G"
        ct[5] = _plant(ct[5], 105, recs[15][:24])
        long_rec = recs[101]
        ct[6] = _plant(ct[6], 17, long_rec[500:500 + L]) if L in (65, 256) else _plant(ct[6], 30, recs[29])      # inside the 2,047-base record / the record with N
        ct[8] = _plant(ct[8], LEN - 30, recs[20])                                    # ends with the contig
        ct[9] = _plant(ct[9], LEN - 37, recs[30].upper()[:20] + "N")
        ct[12] = ct[12][:-2] + "CA"
        out[L] = (ct, ws, wl)
    return out


@functools.lru_cache(maxsize=None)
def mask_call():
    """windows that cut a planted D record (record 21, 31 bases, at 120 .. 150 of every contig): across the window's 3' end, across its 5'
    end, and the whole record just outside the window on either side -> (contigs, win_start, win_len, the record's index)"""
    _, recs = d_set()
    rng = np.random.default_rng(717)
    r = 21
    assert len(recs[r]) == 31
    ct = [_plant(_rand(rng, LEN), 120, recs[r]) for _ in range(5)]
    ws = [90, 136, 151, 80, 100]
    wl = [45, 60, 50, 40, 80]                                                        # ends at 135 / starts at 136 / starts after / ends before / holds it
    return ct, ws, wl, r


def _cat_calls():
    ct, ws, wl = [], [], []
    for L in LONGEST:
        c, s, l = row_calls()[L]
        ct, ws, wl = ct + c, ws + s, wl + l
    return ct, ws, wl


@functools.lru_cache(maxsize=None)
def models():
    """every model result the device is compared with, computed once (the model is per contig: the seven calls are one model call)"""
    _, recs = d_set()
    ct, ws, wl = _cat_calls()
    h, S = D.dcall(ct, ws, wl, recs)
    rows = {}
    for k, L in enumerate(LONGEST):
        sl = slice(13 * k, 13 * k + 13)
        rows[L] = ({f: v[sl] for f, v in h.items()}, S[sl])
    mc, ms, ml, _ = mask_call()
    c129 = row_calls()[129]
    return dict(rows=rows, mask=D.dcall(mc, ms, ml, recs), extremes=[D.dcall(*c129, recs, p) for p in EXTREMES])


def _pack(dev):
    return dict(d={f: np.asarray(dev["d"][f]).tolist() for f in A.FIELDS}, scores=None if dev["scores"] is None else dev["scores"].tolist(),
                dtype=None if dev["scores"] is None else str(dev["scores"].dtype))


def _device(_):
    from vdjer_amd import api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    with pytest.raises(VdjxError, match="no D set"):
        ctx.dcall(["ACGT" * 10], [0], [10])                           # (VDJX_ESTATE: nothing loaded yet)
    recs, clean = d_set()
    kept0 = ctx.stat("kept_device_bytes")
    info = ctx.dsegment_load(recs + [("IGHV1-2*01", "ACGTACGT"), ("J7", "ACGT")])
    assert info["names"] == [f"IGHD{k}*01" if k % 2 else f"D{k}" for k in range(len(recs))] and info["skipped"] == {"V": 1, "J": 1}
    assert ctx.stat("kept_device_bytes") > kept0                      # (the set is one of the context's kept buffers)
    total = sum(len(s) for s in clean)
    out = dict(rows={}, n_records=len(recs))
    for L in LONGEST:
        ct, ws, wl = row_calls()[L]
        dev = ctx.dcall(ct, ws, wl)
        assert ctx.stat("dcall_cells") == sum(wl) * total, (L, ctx.stat("dcall_cells"))
        again = ctx.dcall(ct, ws, wl)
        for f in A.FIELDS:
            assert np.asarray(again["d"][f]).tobytes() == np.asarray(dev["d"][f]).tobytes(), (L, f)
        assert again["scores"].tobytes() == dev["scores"].tobytes()
        bare = ctx.dcall(ct, ws, wl, scores=False)                    # (out_scores = NULL)
        assert bare["scores"] is None and all(np.asarray(bare["d"][f]).tobytes() == np.asarray(dev["d"][f]).tobytes() for f in A.FIELDS)
        out["rows"][str(L)] = _pack(dev)
    mc, ms, ml, _ = mask_call()
    out["mask"] = _pack(ctx.dcall(mc, ms, ml))
    out["extremes"] = [_pack(ctx.dcall(*row_calls()[129], **p)) for p in EXTREMES]
    # three dispatches a call, whatever n and C are
    ctx.profile(True)
    ctx.profile_reset()
    ctx.dcall(*row_calls()[256])
    out["dispatches"] = {k: v[1] for k, v in ctx.profile_get().items()}
    ctx.profile(False)
    # the germline set and the D set are independent
    rng = np.random.default_rng(77)
    gl = [("V0", _rand(rng, 290)), ("J0", _rand(rng, 50))]
    act = [gl[0][1][10:250] + _rand(rng, 30) + gl[1][1][:45] + _rand(rng, 45) for _ in range(3)]
    ctx.germline_load(gl)
    before = ctx.annotate(act)
    ct, ws, wl = row_calls()[64]
    d0 = ctx.dcall(ct, ws, wl)
    after = ctx.annotate(act)
    assert all(np.asarray(after[c][f]).tobytes() == np.asarray(before[c][f]).tobytes() for c in ("v", "j") for f in A.FIELDS)
    assert d0["scores"].tolist() == out["rows"]["64"]["scores"] and (before["v"]["gene"] >= 0).all()
    # no contig; refusals
    r0 = ctx.dcall([], [], [])
    assert r0["d"]["gene"].shape == (0,) and r0["scores"].shape == (0, len(recs))
    good = ["ACGT" * 75]
    for bad in (dict(min_score=-1), dict(match=0), dict(match=16), dict(mismatch=32), dict(gap_open=-1), dict(gap_extend=32)):
        with pytest.raises(VdjxError):
            ctx.dcall(good, [10], [20], **bad)
    for ws_, wl_ in (([-1], [20]), ([10], [-1]), ([290], [11]), ([300], [1]), ([0], [257]), ([301], [0])):
        with pytest.raises(VdjxError):
            ctx.dcall(good, ws_, wl_)
    assert ctx.dcall(good, [44], [256])["d"]["score"][0] >= 0 and ctx.dcall(good, [300], [0])["d"]["gene"][0] == -1      # (the largest window; an empty one at the end)
    with pytest.raises(VdjxError):
        ctx.dcall(["ACGT" * 5, "ACG" * 5], [0, 0], [4, 4])
    with pytest.raises(VdjxError):
        ctx.dcall((b"ACGTACGTACGTACG\0ACGTACGTACGTACGT", 2, 16), [0, 0], [4, 4])
    with pytest.raises(VdjxError):
        ctx.dcall(["A" * 4096], [0], [4])
    with pytest.raises(VdjxError):
        ctx.dcall((b"A" * (1 << 20), 1 << 20, 1), np.zeros(1 << 20, np.int32), np.zeros(1 << 20, np.int32), scores=False)
    for bad_set in ([("D0", "")], [("D0", "A" * 2048)], [("D0", "ACGT")] * 4097):
        with pytest.raises(VdjxError):
            ctx.dsegment_load(bad_set)
    # an empty D set: no call, score 0
    assert ctx.dsegment_load([("V0", "ACGT")])["names"] == []
    ct, ws, wl = row_calls()[64]
    e = ctx.dcall(ct, ws, wl, min_score=0)
    assert (e["d"]["gene"] == -1).all() and (e["d"]["score"] == 0).all() and (e["d"]["n_tied"] == 0).all() and (e["d"]["tied"] == -1).all()
    assert e["scores"].shape == (13, 0) and ctx.stat("dcall_cells") == 0
    ctx.close()
    return out


def _same(dev, model, what):
    h, Sm = model
    for f in A.FIELDS:
        a, b = np.asarray(dev["d"][f]).astype(np.int64), np.asarray(h[f]).astype(np.int64)
        assert np.array_equal(a, b), (what, f, np.argwhere(a != b)[:5].tolist(), a.ravel()[:14].tolist(), b.ravel()[:14].tolist())
    S = np.asarray(dev["scores"], np.int64).reshape(Sm.shape)
    assert dev["dtype"] == "int32" and np.array_equal(S, Sm), (what, "scores", np.argwhere(S != Sm)[:5].tolist())


@pytest.mark.parametrize("knobs", KNOBS)
def test_dcall_api_vs_model(knobs):
    res = _run_child("_device", "x", _child_env(knobs))
    m = models()
    _, recs = d_set()
    for L in LONGEST:
        _same(res["rows"][str(L)], m["rows"][L], L)
        h = m["rows"][L][0]
        # what the case is there for: the tie across a chunk boundary, the windows at both ends of the contig, the empty windows
        assert h["gene"][0] == 0 and h["n_tied"][0] == 2 and h["tied"][0][:2].tolist() == [0, len(recs) - 1] and h["score"][0] == 74, (L, h["tied"][0])
        assert h["seq_end"][8] == LEN and h["gene"][8] == 20 and h["gene"][1] >= 0 and h["n_runs"][1] > 0
        assert [int(h["gene"][c]) for c in (2, 7)] == [-1, -1] and h["gene"][5] == 15
        if L in (65, 256):
            assert h["gene"][6] == 101 and h["score"][6] == 2 * L and h["seq_start"][6] == 18 and h["seq_end"][6] == 17 + L
    # the masking: a record cut by the window's end scores what lies inside, a record outside nothing of its own
    _same(res["mask"], m["mask"], "mask")
    r = mask_call()[3]
    Sm, full = m["mask"][1][:, r], 2 * len(recs[r])
    assert Sm[4] == full and (Sm[:4] < full).all() and Sm[0] == 2 * 15 and Sm[1] == 2 * 15, Sm
    assert np.asarray(res["mask"]["scores"])[:, r].tolist() == Sm.tolist()
    for k, p in enumerate(EXTREMES):
        _same(res["extremes"][k], m["extremes"][k], p)
    assert (m["extremes"][0][0]["n_tied"] > 8).any()                   # (min_score 0: every one-base record ties)
    assert res["dispatches"] == {"k_dcall_score": 1, "k_dcall_trace": 1}, res["dispatches"]      # (one scoring scope -- score and merge -- and one traceback launch)


# ---- vdjer --airr --d-calls ------------------------------------------------------------------------------------------------------------
def d_records(tag, rep):
    """the class-D records appended to a golden's ig_vdj.fa: for the heavy chain a 14 .. 20-base cut from the middle of the core (the
    bases after the 300 of the V) of three clones, a duplicate of the first cut (a tie: a comma-joined d_call) and five random decoys;
    none for a light chain"""
    if RECIPES[tag].get("chain", "IGH") != "IGH":
        return []
    rng = np.random.default_rng(818)
    cuts = []
    for i in range(3):
        core = rep.clones[i][300:len(rep.clones[i]) - len(rep.j_germ[rep.clone_j[i]])]
        k = min(14 + 3 * i, len(core))
        o = (len(core) - k) // 2
        cuts.append(core[o:o + k])
    seqs = cuts + [cuts[0]] + [_rand(rng, int(rng.integers(11, 38))) for _ in range(5)]
    return [(f"IGHD{k + 1}-1*01" if k % 2 else f"D{k}", s) for k, s in enumerate(seqs)]


@functools.lru_cache(maxsize=None)
def cli_case(tag):
    """(ids, contigs, V/J names, V/J hits, D names, D hits, windows) of a golden's contigs from the models"""
    from vdjer_amd import synth
    rep = synth.make_repertoire(**RECIPES[tag])
    fa = G.text(f"{tag}.contigs.fa.gz").splitlines()
    ids, seqs = [fa[i][1:] for i in range(0, len(fa), 2)], [fa[i + 1] for i in range(0, len(fa), 2)]
    germs = rep.v_germ + rep.j_germ
    names = [f"V{i}" for i in range(len(rep.v_germ))] + [f"J{i}" for i in range(len(rep.j_germ))]
    hits = A.annotate(seqs, germs, ["V"] * len(rep.v_germ) + ["J"] * len(rep.j_germ))
    drec = d_records(tag, rep)
    ws, wl = D.d_window(hits["v"], hits["j"])
    d, _ = D.dcall(seqs, ws, wl, [s for _, s in drec])
    return ids, seqs, names, hits, [n_ for n_, _ in drec], d, (ws, wl)


def _write_d(tag, d):
    from vdjer_amd import synth
    rep = synth.make_repertoire(**RECIPES[tag])
    with open(os.path.join(d, "ref", "ig_vdj.fa"), "a") as f:
        for k, (name, s) in enumerate(d_records(tag, rep)):
            f.write(f">{name} synthetic\n" if k % 2 else f">X{k}|{name}|synthetic\n")
            f.write(s[:7].lower() + "\n" + s[7:] + "\n" if k == 1 else s + "\n")


def _dcalls_line(r):
    return next(l for l in r.stderr.splitlines() if l.startswith("dcalls: "))


def test_vdjer_cli_d_calls_heavy_chain(tmp_path):
    tag = "e2e_mixed"
    ids, seqs, names, hits, d_names, d, (ws, wl) = cli_case(tag)
    want = D.airr_rows(ids, seqs, hits, names, d, d_names)
    col = {k: i for i, k in enumerate(D.AIRR_COLUMNS)}
    assert any(r[col["d_call"]] for r in want) and any("," in r[col["d_call"]] for r in want), [r[col["d_call"]] for r in want]
    _write_inputs(tag, str(tmp_path))
    _write_d(tag, str(tmp_path))
    env = _child_env("shipped")
    r = _vdjer(tmp_path, tag, ["--airr", "a.tsv", "--d-calls"], env)
    head, rows = A.read_table(tmp_path / "a.tsv")
    assert head == D.AIRR_COLUMNS and rows == want
    lines = r.stderr.splitlines()
    a_at = next(i for i, l in enumerate(lines) if l.startswith("airr: "))
    assert lines[a_at + 1] == (f"dcalls: {len(ids)} contigs, {int((wl > 0).sum())} windows, {D.over_window(hits['v'], hits['j'])} over 256 bases, "
                               f"{int((d['gene'] >= 0).sum())} D called against {len(d_names)} D records")
    assert f"skipped: {len(d_names)} D, 0 other" in lines[a_at]
    # without --d-calls: the table and the summary line of --airr as they were, whatever D records the FASTA holds
    plain = tmp_path / "plain"
    plain.mkdir()
    _write_inputs(tag, str(plain))
    _write_d(tag, str(plain))
    r0 = _vdjer(plain, tag, ["--airr", "a.tsv"], env)
    head, rows = A.read_table(plain / "a.tsv")
    assert head == A.AIRR_COLUMNS and rows == A.airr_rows(ids, seqs, hits, names)
    assert not any(l.startswith("dcalls: ") for l in r0.stderr.splitlines())
    assert [l for l in r0.stderr.splitlines() if l.startswith("airr: ")] == [lines[a_at]]
    # one run under the suite's knobs, one germline per scoring launch of vdjx_annotate: the same table
    knobs = tmp_path / "knobs"
    knobs.mkdir()
    _write_inputs(tag, str(knobs))
    _write_d(tag, str(knobs))
    _vdjer(knobs, tag, ["--d-calls", "--airr", "a.tsv"], _child_env("suite", VDJX_ANNOT_PAIRS="3"))
    assert (knobs / "a.tsv").read_bytes() == (tmp_path / "a.tsv").read_bytes()


def test_vdjer_cli_d_calls_light_chain(tmp_path):
    """a ref-dir without D records is no error: no call, np1 is the whole gap between the V and the J hit"""
    tag = "e2e_igk"
    ids, seqs, names, hits, d_names, d, (ws, wl) = cli_case(tag)
    assert d_names == []
    _write_inputs(tag, str(tmp_path))
    r = _vdjer(tmp_path, tag, ["--airr", "a.tsv", "--d-calls"], _child_env("shipped"))
    head, rows = A.read_table(tmp_path / "a.tsv")
    assert head == D.AIRR_COLUMNS and rows == D.airr_rows(ids, seqs, hits, names, d, d_names)
    col = {k: i for i, k in enumerate(D.AIRR_COLUMNS)}
    both = 0
    for c, row in enumerate(rows):
        assert row[col["d_call"]] == "" and row[col["d_cigar"]] == "" and row[col["d_score"]] == "" and row[col["np2"]] == ""
        if row[col["v_sequence_end"]] and row[col["j_sequence_start"]]:
            both += 1
            gap = seqs[c][int(row[col["v_sequence_end"]]):max(int(row[col["j_sequence_start"]]) - 1, int(row[col["v_sequence_end"]]))]
            assert row[col["np1"]] == gap and row[col["np1_length"]] == str(len(gap)) and row[col["np2_length"]] == "0"
    assert both > 0
    assert _dcalls_line(r).endswith("0 D called against 0 D records")
