"""vdjx_isotype on the GPU: every vdjx_annot_hit field and the whole score matrix against the integer model of tests/isotype_model.py
(randomised, and at size on the private repertoire's contigs), and `vdjer --isotypes --clones --cfa` on every e2e golden against the
model's tables.  The API checks run in child processes with timeouts, once per knob setting, as tests/test_gpu_annot.py runs them."""
import os

import numpy as np
import pytest

from tests import annot_model as A
from tests import golden_util as G
from tests import isotype_model as M
from tests import quant_model as Q
from tests.test_gpu_annot import E2E, KNOBS, RECIPES, _argv, _child_env, _mutate, _rand, _vdjer, _write_inputs, at_size_contigs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES = 44
CONST_NAMES = ["IGHM*01", "IGHG1*01", "IGHG2*01", "IGHG4*01", "IGHG3*01", "IGHA1*01", "IGHE*01", "IGHD*01"]


def _run_child(fn, arg, env, timeout=1500):
    import json
    import subprocess
    import sys
    code = f"import json; from tests.test_gpu_isotype import {fn}; print('ISO', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("ISO ")).split(" ", 1)[1])


def _random_case(seed):
    """(contigs, constant records, parameters): len 16 .. 400, tail 16 .. 64 (also above len), 0 .. 60 records of 1 .. 2047 bases with exact
    copies, mutated copies, records holding N and duplicated records (ties, some more than 8 times); tails copied from the records, mutated
    copies of such windows, random tails and tails holding N; random parameters inside vdjx_isotype's ranges"""
    rng = np.random.default_rng(1000 + seed)
    ln = [16, 17, 400, 47, 64, 65][seed] if seed < 6 else int(rng.integers(16, 401))
    tail = [16, 64, 64, 48, 64, 64][seed] if seed < 6 else int(rng.integers(16, 65))
    C = 0 if seed % 11 == 7 else int(rng.integers(1, 61))
    recs = []
    for r in range(C):
        kind = int(rng.integers(0, 10))
        if r and kind == 0:
            recs.append(recs[int(rng.integers(0, r))])                                      # an exact copy: a tie
        elif r and kind == 1:
            recs.append(_mutate(rng, recs[int(rng.integers(0, r))], int(rng.integers(1, 4)))[:2047])
        elif kind == 2:
            recs.append(_rand(rng, rng.integers(1, 6)))
        elif kind == 3 and seed % 4 == 0:
            recs.append(_rand(rng, rng.integers(1500, 2048), "ACGTN" if r % 2 else "ACGT"))
        else:
            recs.append(_rand(rng, rng.integers(20, 400), "ACGTTGCAN" if kind == 4 else "ACGT"))
    if C and seed % 5 == 3:
        recs = (recs + [recs[0]] * 10)[:60]                                                 # more than 8 ties
    if C and seed % 7 == 2:
        recs[-1] = _rand(rng, 2047)
    T = min(tail, ln)
    contigs = []
    for c in range(7):
        t = _rand(rng, T)
        long_enough = [r for r in recs if len(r) >= T]
        if long_enough and c < 5:
            src = long_enough[int(rng.integers(0, len(long_enough)))]
            o = int(rng.integers(0, len(src) - T + 1))
            t = src[o:o + T]
            if c in (1, 2):
                t = (_mutate(rng, t, int(rng.integers(1, 5))) + _rand(rng, T))[:T]
            if c == 3:
                t = t[:T // 2] + "N" + t[T // 2 + 1:]
        elif recs and c == 5:
            t = (recs[0] * T)[:T]
        contigs.append(_rand(rng, ln - T) + t)
    if seed % 3 == 0:
        p = dict(M.DEFAULT, tail=tail)
    else:
        p = dict(match=int(rng.integers(1, 16)), mismatch=int(rng.integers(0, 32)), gap_open=int(rng.integers(0, 32)),
                 gap_extend=int(rng.integers(0, 32)), min_score=int(rng.integers(0, 120)), tail=tail)
        if seed % 3 == 1:
            p.update(match=int(rng.integers(1, 4)), mismatch=int(rng.integers(0, 4)), gap_open=int(rng.integers(0, 4)), gap_extend=int(rng.integers(0, 3)))
    return contigs, recs, p


def _same(dev, model, S, what):
    h, Sm = model
    for f in A.FIELDS:
        a, b = np.asarray(dev["c"][f]).astype(np.int64), np.asarray(h[f]).astype(np.int64)
        assert np.array_equal(a, b), (what, f, np.argwhere(a != b)[:5].tolist(), a.ravel()[:12].tolist(), b.ravel()[:12].tolist())
    if S is not None:
        assert S.dtype == np.int32 and S.shape == Sm.shape and np.array_equal(S.astype(np.int64), Sm), (what, "scores", np.argwhere(S != Sm)[:5].tolist())


def _api_checks(_):
    from vdjer_amd import api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    with pytest.raises(VdjxError, match="no constant set"):
        ctx.isotype(["ACGT" * 10])                                    # (VDJX_ESTATE: nothing loaded yet)
    # a vdjx_annotate call before: the isotype calls in between must not change what it returns
    rng = np.random.default_rng(77)
    gl = [("V0", _rand(rng, 290)), ("V1", _rand(rng, 300)), ("J0", _rand(rng, 50)), ("J1", _rand(rng, 60))]
    act = [gl[c % 2][1][10:250] + _rand(rng, 30) + gl[2 + c % 2][1][:45] + _rand(rng, 45) for c in range(6)]
    ctx.germline_load(gl)
    before = ctx.annotate(act)
    out = dict(cases=0, called=0, traced=0, ties=0, cells=0)
    for seed in range(N_CASES):
        contigs, recs, p = _random_case(seed)
        info = ctx.constant_load([(f"C{k} text", s.lower() if k % 5 == 1 else s) for k, s in enumerate(recs)])
        assert info["names"] == [f"C{k}" for k in range(len(recs))]
        dev = ctx.isotype(contigs, **p)
        model = M.isotype(contigs, recs, p)
        if not recs:
            assert dev["scores"].shape == (len(contigs), 0)
        _same(dev, model, dev["scores"], seed)
        assert ctx.stat("iso_cells") == len(contigs) * min(p["tail"], len(contigs[0])) * sum(len(r) for r in recs)
        again = ctx.isotype(contigs, **p)
        for f in A.FIELDS:
            assert np.asarray(again["c"][f]).tobytes() == np.asarray(dev["c"][f]).tobytes(), (seed, f)
        assert again["scores"].tobytes() == dev["scores"].tobytes()
        bare = ctx.isotype(contigs, scores=False, **p)                # (out_scores = NULL)
        assert bare["scores"] is None
        for f in A.FIELDS:
            assert np.asarray(bare["c"][f]).tobytes() == np.asarray(dev["c"][f]).tobytes(), (seed, f)
        out["cases"] += 1
        out["called"] += int((dev["c"]["gene"] >= 0).sum())
        out["traced"] += int((dev["c"]["n_runs"] > 0).sum())
        out["ties"] += int((dev["c"]["n_tied"] > 1).sum())
        out["cells"] += ctx.stat("iso_cells")
    after = ctx.annotate(act)
    for cls in ("v", "j"):
        for f in A.FIELDS:
            assert np.asarray(after[cls][f]).tobytes() == np.asarray(before[cls][f]).tobytes(), (cls, f)
    assert (before["v"]["gene"] >= 0).all()
    # the germline set and the constant set are independent: a new germline set leaves the isotype call alone
    contigs, recs, p = _random_case(0)
    ctx.constant_load([(f"C{k}", s) for k, s in enumerate(recs)])
    d0 = ctx.isotype(contigs, **p)
    ctx.germline_load([("V0", "ACGT" * 20), ("J0", "TTGCA" * 5)])
    d1 = ctx.isotype(contigs, **p)
    assert all(np.asarray(d0["c"][f]).tobytes() == np.asarray(d1["c"][f]).tobytes() for f in A.FIELDS)
    # no contig; refusals
    r0 = ctx.isotype([])
    assert r0["c"]["gene"].shape == (0,)
    good = ["ACGT" * 20]
    for bad in (dict(tail=15), dict(tail=65), dict(min_score=-1), dict(match=0), dict(match=16), dict(mismatch=32), dict(gap_open=-1),
                dict(gap_extend=32)):
        with pytest.raises(VdjxError):
            ctx.isotype(good, **bad)
    with pytest.raises(VdjxError):
        ctx.isotype(["ACGT" * 5, "ACG" * 5])
    with pytest.raises(VdjxError):
        ctx.isotype((b"ACGTACGTACGTACG\0ACGTACGTACGTACGT", 2, 16))
    with pytest.raises(VdjxError):
        ctx.isotype(["A" * 4096])
    for recs in ([("C0", "")], [("C0", "A" * 2048)], [("C0", "ACGT")] * 4097):
        with pytest.raises(VdjxError):
            ctx.constant_load(recs)
    ctx.constant_load([("C0", "ACGT")] * 4096)                        # (the largest set)
    h = ctx.isotype(["ACGT" * 10], min_score=8)
    assert h["c"]["n_tied"][0] == 4096 and h["c"]["score"][0] == 8 and h["scores"].shape == (1, 4096) and (h["scores"] == 8).all()
    ctx.close()
    return out


@pytest.mark.parametrize("knobs", KNOBS)
def test_isotype_api_vs_model(knobs):
    res = _run_child("_api_checks", "x", _child_env(knobs))
    print(res)
    assert res["cases"] == N_CASES >= 40 and res["called"] > 50 and res["traced"] > 50 and res["ties"] > 5


def at_size_case():
    """the at_size_contigs recipe (2,172 contigs of 360 bases) and 9 records of 1,000 bases: six cut from the J + tail segments of the
    contigs' own clones (three segments each, downstream of the J anchor), three decoys"""
    ids, seqs, rep, clone = at_size_contigs()
    recs = ["".join(rep.j_germ[clone[100 * k + i]][24:] for i in range(3))[:1000] for k in range(6)]
    rng = np.random.default_rng(4)
    recs = recs[:3] + [_rand(rng, 1000)] + recs[3:] + [_rand(rng, 1000), _rand(rng, 1000)]
    assert len(recs) == 9 and all(len(r) == 1000 for r in recs)
    return ids, seqs, recs


def _at_size(_):
    import time
    from vdjer_amd import api
    ids, seqs, recs = at_size_case()
    ctx = api.Context(0)
    ctx.constant_load([(f"C{k}", r) for k, r in enumerate(recs)])
    t0 = time.perf_counter()
    dev = ctx.isotype(seqs)
    wall = time.perf_counter() - t0
    model = M.isotype(seqs, recs)
    _same(dev, model, dev["scores"], "at size")
    called = int((dev["c"]["gene"] >= 0).sum())
    res = dict(contigs=len(seqs), cells=ctx.stat("iso_cells"), score_us=ctx.stat("iso_score_us"), trace_us=ctx.stat("iso_trace_us"),
               called=called, wall_s=round(wall, 4))
    ctx.close()
    return res


def test_isotype_at_size():
    res = _run_child("_at_size", "x", _child_env("shipped"), timeout=2400)
    print(res)
    assert res["contigs"] == 2172 and res["cells"] == 2172 * 48 * 9000 and res["called"] >= 18


# ---- vdjer --isotypes --clones --cfa ---------------------------------------------------------------------------------------------------
def constant_records(rep):
    """the constant FASTA of an e2e golden: the repertoire's J + tail segments downstream of the J anchor (a 360-base contig ends roughly
    90 bases into them), named as constant genes; IGHG2 and IGHG4 are point-mutated copies of IGHG1 -- IGHG2's mutation lies past
    every tail (a tie: one subtype of two genes), IGHG4's inside them (a runner-up score decides)"""
    seg = [j[24:] for j in rep.j_germ]
    assert len(seg) >= 6

    def point(s, q):
        return s[:q] + ("A" if s[q] != "A" else "C") + s[q + 1:]

    seqs = [seg[0], seg[1], point(seg[1], 200), point(seg[1], 40), seg[2], seg[3], seg[4], seg[5]]
    return list(zip(CONST_NAMES, seqs))


def golden_tables(tag, rep, sample, total_count):
    """(isotype rows, clone rows, clone rows without --cfa) of the golden contigs from the models"""
    fa = G.text(f"{tag}.contigs.fa.gz").splitlines()
    ids, seqs = [fa[i][1:] for i in range(0, len(fa), 2)], [fa[i + 1] for i in range(0, len(fa), 2)]
    sids, L, names, a = Q.sam_placements(G.text(f"{tag}.sam.gz"))
    assert sids == ids
    N, _ = Q.quant(a[:, 0], a[:, 1], a[:, 2], len(ids), L)
    germs = rep.v_germ + rep.j_germ
    gnames = [f"V{i}" for i in range(len(rep.v_germ))] + [f"J{i}" for i in range(len(rep.j_germ))]
    vj = A.annotate(seqs, germs, ["V"] * len(rep.v_germ) + ["J"] * len(rep.j_germ))
    recs = constant_records(rep)
    iso, S = M.isotype(seqs, [s for _, s in recs])
    cn = [n_ for n_, _ in recs]
    return (ids, N, M.isotype_rows(ids, seqs, iso, cn), M.clone_rows(sample, ids, seqs, N, vj, gnames, iso, cn, total_count),
            M.clone_rows(sample, ids, seqs, N, vj, gnames, None, None, total_count))


def _write_cfa(rep, d):
    with open(os.path.join(d, "c.fa"), "w") as f:
        for k, (name, s) in enumerate(constant_records(rep)):
            f.write(f">{name} constant\n" if k % 2 else f">X{k}|{name}|synthetic\n")
            f.write((s[:70].lower() + "\n" + s[70:] + "\n") if k == 2 else s + "\n")


@pytest.mark.parametrize("tag", E2E)
def test_vdjer_cli_isotypes_and_clones(tag, tmp_path):
    rep = _write_inputs(tag, str(tmp_path))
    _write_cfa(rep, str(tmp_path))
    ids, N, irows, crows, crows_nocfa = golden_tables(tag, rep, "s7", 1000)
    # every contig with a row in the clone table gets an isotype call (the records cover the tails; the threshold is the model's)
    assert crows and all(r[5] != "N/A" for r in crows), [r[4:6] for r in crows]
    env = _child_env("shipped")
    r = _vdjer(tmp_path, tag, ["--isotypes", "i.tsv", "--clones", "c.tsv", "--cfa", "c.fa", "--sample", "s7", "--total-count", "1000"], env)
    lines = r.stderr.splitlines()
    assert len([l for l in lines if l.startswith("ELAPSED_SECS\t")]) == 17
    last_mark = max(i for i, l in enumerate(lines) if l.startswith("ELAPSED_SECS\t"))
    i_at = next(i for i, l in enumerate(lines) if l.startswith("isotypes: "))
    c_at = next(i for i, l in enumerate(lines) if l.startswith("clones: "))
    assert last_mark < i_at < c_at and not any(l.startswith(("quant: ", "airr: ")) for l in lines)
    head, rows = A.read_table(tmp_path / "i.tsv")
    assert head == M.ISOTYPE_COLUMNS and rows == irows and [r_[0] for r_ in rows] == ids
    head, rows = A.read_table(tmp_path / "c.tsv")
    assert head == M.CLONE_COLUMNS and rows == crows
    assert f"{len(ids)} contigs" in lines[i_at] and f"{len(crows)} rows" in lines[c_at]
    itsv, ctsv = (tmp_path / "i.tsv").read_bytes(), (tmp_path / "c.tsv").read_bytes()
    assert not (tmp_path / "q.tsv").exists() and not (tmp_path / "a.tsv").exists()

    # --quant and --airr alongside: every step once, every table the same values; the default sample name
    both = tmp_path / "both"
    both.mkdir()
    _write_inputs(tag, str(both))
    _write_cfa(rep, str(both))
    _vdjer(both, tag, ["--quant", "q.tsv", "--airr", "a.tsv", "--isotypes", "i.tsv", "--clones", "c.tsv", "--cfa", "c.fa"], env)
    assert (both / "i.tsv").read_bytes() == itsv
    head, rows = A.read_table(both / "c.tsv")
    assert [["s7"] + r_[1:10] + ["1000"] + r_[11:] for r_ in rows] == crows and {r_[0] for r_ in rows} == {"reads"} and {r_[10] for r_ in rows} == {"N/A"}
    qhead, qrows = Q.read_table(both / "q.tsv")
    qcount = {q[0]: q[4] for q in qrows}
    assert [q[4] for q in qrows] == ["%.2f" % x for x in N]
    assert all(r_[3] == qcount[r_[4]] for r_ in rows)
    ahead, arows = A.read_table(both / "a.tsv")
    assert ahead == A.AIRR_COLUMNS + ["expected_count"] and [r_[-1] for r_ in arows] == [q[4] for q in qrows]
    acol = {r_[0]: r_ for r_ in arows}
    assert all(r_[7] == acol[r_[4]][10] and r_[2] == acol[r_[4]][9] for r_ in rows)        # (aa_cdr3 = junction_aa, cdr3 = junction)
    # the AIRR table is what --airr --quant alone writes
    plain = tmp_path / "plain"
    plain.mkdir()
    _write_inputs(tag, str(plain))
    _vdjer(plain, tag, ["--quant", "q.tsv", "--airr", "a.tsv"], env)
    assert (plain / "a.tsv").read_bytes() == (both / "a.tsv").read_bytes() and (plain / "q.tsv").read_bytes() == (both / "q.tsv").read_bytes()

    # --clones without --cfa: isotype N/A
    nocfa = tmp_path / "nocfa"
    nocfa.mkdir()
    _write_inputs(tag, str(nocfa))
    _vdjer(nocfa, tag, ["--clones", "c.tsv", "--sample", "s7", "--total-count", "1000"], env)
    assert A.read_table(nocfa / "c.tsv")[1] == crows_nocfa

    # --isotypes under --gpus 2 (rank 0 calls)
    multi = tmp_path / "two"
    multi.mkdir()
    _write_inputs(tag, str(multi))
    _write_cfa(rep, str(multi))
    _vdjer(multi, tag, ["--gpus", "2", "--isotypes", "i.tsv", "--cfa", "c.fa"], _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert (multi / "i.tsv").read_bytes() == itsv
    assert ctsv


def test_vdjer_cli_isotypes_under_suite_knobs(tmp_path):
    tag = "e2e_mixed"
    rep = _write_inputs(tag, str(tmp_path))
    _write_cfa(rep, str(tmp_path))
    ids, N, irows, crows, _ = golden_tables(tag, rep, "reads", None)
    _vdjer(tmp_path, tag, ["--isotypes", "i.tsv", "--clones", "c.tsv", "--cfa", "c.fa"], _child_env("suite"))
    assert A.read_table(tmp_path / "i.tsv")[1] == irows and A.read_table(tmp_path / "c.tsv")[1] == crows
