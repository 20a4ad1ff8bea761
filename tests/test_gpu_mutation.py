"""vdjx_mutations on the GPU: every row byte, every count and the info against the integer model of tests/mutation_model.py, on handmade
hits (any consistent hit is legal input) at the smallest sizes at which the kernel can go wrong -- the lane striping, the run counts, the
codon frame, indels inside and between codons, the limit, the J clip, the D hit in the gap, a deletion longer than the contig -- the
refusals, and `vdjer --mutations` on three goldens against the model's table.  The API checks run in child processes, once per knob
setting, as tests/test_gpu_dcall.py runs them; the model is computed once."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import annot_model as A
from tests import dcall_model as D
from tests import families as F
from tests import golden_util as G
from tests import mutation_model as M
from tests.test_gpu_annot import KNOBS, _child_env, _vdjer, _write_inputs
from tests.test_mutation_cpu import WANT, designed_pair, parsed_records, planted_families

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEN = 300
CALL = 13                                                            # contigs per call: no multiple of a workgroup's four waves


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_mutation import {fn}; print('MUT', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("MUT ")).split(" ", 1)[1])


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(list(alpha), int(n)))


# ---- the record sets ---------------------------------------------------------------------------------------------------------------------
V0, V1, C1, V2, D0, V3, V4, J0, D1, V5, J1 = range(11)                # the records' indices, as given


@functools.lru_cache(maxsize=None)
def records():
    """[(FASTA header, sequence)] given to germline_load AND dsegment_load (each keeps its classes): V records of 360 bases, of 90 with an
    N, of ONE base, of 2,047 bases, the designed codons of tests/test_mutation_cpu.py and, last of its class, of 60 bases; J records of 48
    and, last of the set, of 30 bases; two D records; a record of another class, so that a gene is not its slot"""
    rng = np.random.default_rng(1919)
    with_n = _rand(rng, 90)
    seqs = {V0: _rand(rng, 360), V1: with_n[:40] + "N" + with_n[41:], C1: "ACGT" * 10, V2: "A", D0: _rand(rng, 20), V3: _rand(rng, 2047),
            V4: designed_pair()[0], J0: _rand(rng, 48), D1: _rand(rng, 12), V5: _rand(rng, 60), J1: _rand(rng, 30)}
    heads = {V0: "V0 x", V1: "X1|IGHV1-1*01|y", C1: "C1", V2: "V2", D0: "IGHD1-1*01", V3: "V3", V4: "V4", J0: "IGHJ1*01", D1: "X|IGHD2-2*01|", V5: "V5",
             J1: "J1"}
    return [(heads[k], seqs[k]) for k in range(11)]


def germs():
    return [s for _, s in records()]


def d_germs():
    return [germs()[D0], germs()[D1]]


# ---- handmade hits -----------------------------------------------------------------------------------------------------------------------
def H(gene=-1, seq_start=0, germ_start=0, ops=(), score=100):
    """a consistent vdjx_annot_hit from its runs [(op, length)]"""
    runs = [(l << 4) | "MID".index(o) for o, l in ops]
    ns, ng = sum(l for o, l in ops if o != "D"), sum(l for o, l in ops if o != "I")
    return dict(gene=gene, score=score if gene >= 0 else 0, n_tied=int(gene >= 0), tied=[gene] + [-1] * 7, seq_start=seq_start,
                seq_end=seq_start + ns - 1 if ops else 0, germ_start=germ_start, germ_end=germ_start + ng - 1 if ops else 0, matches=0,
                mismatches=0, ins=sum(l for o, l in ops if o == "I"), opens=0, n_runs=len(runs),
                runs=(runs if len(runs) <= A.RUNS else []) + [0] * (A.RUNS - (len(runs) if len(runs) <= A.RUNS else 0)),
                **{"del": sum(l for o, l in ops if o == "D")}, ops=list(ops))


NONE = H()


def _lay(ct, h, germ):
    """write the hit's germline bases into the contig along its M runs"""
    p, g = h["seq_start"] - 1, h["germ_start"] - 1
    for o, l in h["ops"]:
        for _ in range(l):
            if o == "M":
                ct[p] = germ[g] if germ[g] in "ACGT" else "A"
            p += o != "D"
            g += o != "I"


def _other(ch):
    return "ACGT"[("ACGT".index(ch.upper()) + 1) % 4] if ch.upper() in "ACGT" else "C"


@functools.lru_cache(maxsize=None)
def cases():
    """[dict(name, contig, v, d, j, limit)]: every case is one contig of 300 bases"""
    rng = np.random.default_rng(2020)
    g, dg = germs(), d_germs()
    out = []

    def case(name, v=NONE, j=NONE, d=NONE, limit=LEN, edits=(), text=None):
        ct = list(_rand(rng, LEN))
        if j["gene"] >= 0 and j["n_runs"] <= A.RUNS and j["score"] > 0:
            _lay(ct, j, g[j["gene"]])
        if d["gene"] >= 0 and d["n_runs"] <= A.RUNS and d["score"] > 0:
            _lay(ct, d, dg[d["gene"]])
        if v["gene"] >= 0 and v["n_runs"] <= A.RUNS and v["score"] > 0:
            _lay(ct, v, g[v["gene"]])
        if text:
            ct[text[0]:text[0] + len(text[1])] = list(text[1])
        for q in edits:                                              # a mismatch at contig index q: another base, or the character given
            q, ch = q if isinstance(q, tuple) else (q, None)
            ct[q] = ch if ch else _other(ct[q])
        assert len(ct) == LEN
        out.append(dict(name=name, contig="".join(ct), v=v, d=d, j=j, limit=limit))

    # the lane striping: cols of 1, 63, 64, 65, 128 and 129 (one run each)
    case("cols1", v=H(V2, 5, 1, [("M", 1)]))
    for L in (63, 64, 65, 128, 129):
        case(f"cols{L}", v=H(V0, 11, 1, [("M", L)]), edits=[10 + 16, 10 + 40, 10 + L - 1])
    # 64 runs, 65 runs (no runs to read: treated as absent), on V and on J
    alt = [("M", 1), ("I", 1), ("M", 1), ("D", 1)] * 16
    case("runs64", v=H(V0, 7, 4, alt), j=H(J0, 120, 1, alt), edits=[6, 8, 10, 119, 121])
    case("runs65_v", v=H(V0, 7, 4, alt + [("M", 1)]), j=H(J0, 120, 2, [("M", 20)]))
    case("runs65_j", v=H(V0, 7, 4, [("M", 50)]), j=H(J0, 120, 2, alt + [("M", 1)]), d=H(0, 70, 1, alt + [("M", 1)]))
    # the frame: germ_start = 1, 2, 0 mod 3 (a partial first codon is skipped), germ_end in the middle of a codon
    for gs in (1, 2, 3, 4):
        case(f"frame{gs}", v=H(V0, 5, gs, [("M", 40)]), edits=[4, 5, 6, 7, 4 + 20, 4 + 38, 4 + 39])
    # germ_end at the record's end: the last V record, the last record of the set (J), the 2,047-base record
    case("ends", v=H(V5, 20, 11, [("M", 50)]), j=H(J1, 80, 5, [("M", 26)]), edits=[19 + 48, 19 + 49, 79 + 25])
    case("end2047", v=H(V3, 1, 2047 - 299, [("M", 300)]), edits=[0, 150, 299])
    # deletions of 1, 2, 3 bases inside a codon (after its first base) and exactly between two codons
    for dl in (1, 2, 3):
        case(f"del{dl}_inside", v=H(V0, 5, 1, [("M", 31), ("D", dl), ("M", 40)]), edits=[4 + 28, 4 + 30, 4 + 31, 4 + 33, 4 + 36])
        case(f"del{dl}_between", v=H(V0, 5, 1, [("M", 30), ("D", dl), ("M", 40)]), edits=[4 + 28, 4 + 30, 4 + 31, 4 + 34])
    # an insertion between bases 1 and 2 of a codon (its mismatch is unclassified), and exactly between two codons (both stay classifiable)
    case("ins_inside", v=H(V0, 5, 1, [("M", 31), ("I", 2), ("M", 40)]), edits=[4 + 33, 4 + 50])
    case("ins_between", v=H(V0, 5, 1, [("M", 30), ("I", 1), ("M", 40)]), edits=[4 + 28, 4 + 32])
    # N and a lower-case base in the contig inside a mismatching codon; an N in the germline record
    case("contig_N", v=H(V0, 5, 1, [("M", 60)]), edits=[(4 + 30, "N"), 4 + 31])
    case("contig_lower", v=H(V0, 5, 1, [("M", 60)]), edits=[(4 + 30, g[V0][30].lower()), 4 + 31])
    case("germ_N", v=H(V1, 5, 1, [("M", 80)]), edits=[4 + 36, 4 + 60])
    # the limit at the first, second and third base of a mismatching codon (contig indices 34, 35, 36), past it, 0 and len
    for lim in (34, 35, 36, 37, 0, LEN):
        case(f"limit{lim}", v=H(V0, 5, 1, [("M", 90)]), limit=lim, edits=[4 + 30, 4 + 32, 4 + 3, 4 + 60])
    # J overlapping V by one base, by the whole of J (not used), the clip landing on an I column, and directly after D columns
    v100 = H(V0, 5, 1, [("M", 100)])                                 # contig positions 5 .. 104
    case("clip1", v=v100, j=H(J0, 104, 3, [("M", 30)]), edits=[110])
    case("clip_all", v=v100, j=H(J0, 80, 3, [("M", 25)]))
    case("clip_on_I", v=v100, j=H(J0, 100, 3, [("M", 3), ("I", 4), ("M", 20)]), edits=[108])
    case("clip_after_D", v=v100, j=H(J0, 100, 3, [("M", 5), ("D", 2), ("M", 20)]), edits=[106])
    case("j_leading_D", v=v100, j=H(J0, 120, 3, [("D", 2), ("M", 20)]))
    # D in the gap: in the middle (with an insertion and a deletion of its own), without a call, abutting V's end, abutting J's start,
    # and outside the gap (not used)
    j150 = H(J0, 150, 1, [("M", 40)])
    dops = [("M", 6), ("D", 2), ("M", 6), ("I", 1), ("M", 4)]         # 17 contig bases
    case("d_middle", v=v100, j=j150, d=H(0, 115, 2, dops), edits=[116, 125, 160])
    case("d_none", v=v100, j=j150, d=H(-1))
    case("d_abuts_v", v=v100, j=j150, d=H(0, 105, 2, dops))
    case("d_abuts_j", v=v100, j=j150, d=H(0, 133, 2, dops))
    case("d_outside", v=v100, j=j150, d=H(1, 100, 1, [("M", 10)]))
    case("d_past_j", v=v100, j=j150, d=H(1, 141, 1, [("M", 10)]))
    case("d_without_j", v=v100, d=H(1, 120, 1, [("M", 10)]))
    # no usable V (no call; a call without a score, whatever else it holds); V only is most of the above
    case("no_v", j=j150)
    case("v_score0", v=dict(H(V0, 5, 1, [("M", 100)], score=0), gene=V0, seq_end=9999), j=j150)
    # a deletion of 250 bases: more columns than the contig has bases
    case("del250", v=H(V3, 3, 10, [("M", 20), ("D", 250), ("M", 200)]), edits=[10, 100, 200])
    # the designed codons: a germline stop, a mutation into a stop, silent, replacement, two changes in one codon
    case("designed", v=H(V4, 8, 1, [("M", 90)]), text=(7, designed_pair()[1]))
    while len(out) % CALL:
        case(f"pad{len(out)}")
    return out


FIELDS = [f for f in A.FIELDS]


def _hits(cs, key):
    """the field dicts api.Context.mutations takes, from the cases' hits"""
    shape = {"tied": (len(cs), A.TIED), "runs": (len(cs), A.RUNS)}
    return {f: np.array([c[key][f] for c in cs], np.int64).reshape(shape.get(f, (len(cs),))) for f in FIELDS}


@functools.lru_cache(maxsize=None)
def model(with_d=True):
    cs = cases()
    return M.mutations([c["contig"] for c in cs], _hits(cs, "v"), _hits(cs, "d") if with_d else None, _hits(cs, "j"), [c["limit"] for c in cs],
                       germs(), d_germs())


def _pack(r):
    return dict(seq=r["seq"], germ=r["germ"], mask=r["mask"], counts={k: np.asarray(v).tolist() for k, v in r["counts"].items()}, info=r["info"])


def _raises(ctx, what, match, cs, **kw):
    from vdjer_amd._lib import VdjxError
    with pytest.raises(VdjxError, match=match):
        ctx.mutations([c["contig"] for c in cs], _hits(cs, "v"), _hits(cs, "j"), **kw)
    return what


def _device(_):
    from vdjer_amd import _lib, api
    from vdjer_amd._lib import VdjxError
    ctx = api.Context(0)
    cs = cases()
    ct = [c["contig"] for c in cs]
    lim = np.array([c["limit"] for c in cs], np.int32)
    v, d, j = _hits(cs, "v"), _hits(cs, "d"), _hits(cs, "j")
    with pytest.raises(VdjxError, match="no germline set"):
        ctx.mutations(ct[:2], {f: x[:2] for f, x in v.items()}, {f: x[:2] for f, x in j.items()})
    ginfo = ctx.germline_load(records())
    assert ginfo["skipped"] == {"C": 1, "D": 2}
    with pytest.raises(VdjxError, match="no D set"):
        ctx.mutations(ct[:2], {f: x[:2] for f, x in v.items()}, {f: x[:2] for f, x in j.items()}, d={f: x[:2] for f, x in d.items()})
    assert ctx.dsegment_load(records())["names"] == ["IGHD1-1*01", "IGHD2-2*01"]
    out = dict(calls=[], calls_no_d=[], n=len(cs))
    ctx.profile(True)
    for with_d in (True, False):
        for a in range(0, len(cs), CALL):
            sl = slice(a, a + CALL)
            args = (ct[sl], {f: x[sl] for f, x in v.items()}, {f: x[sl] for f, x in j.items()})
            kw = dict(d={f: x[sl] for f, x in d.items()} if with_d else None, limit=lim[sl])
            ctx.profile_reset()
            r = ctx.mutations(*args, **kw)
            launches = {k: x[1] for k, x in ctx.profile_get().items()}
            assert launches == {"k_mutations": 1}, launches
            again = ctx.mutations(*args, **kw)
            bare = ctx.mutations(*args, rows=False, **kw)
            assert bare["seq"] is None and bare["germ"] is None and bare["mask"] is None
            for f in M.COUNTS:
                assert r["counts"][f].dtype == np.int32
                assert again["counts"][f].tobytes() == r["counts"][f].tobytes() == bare["counts"][f].tobytes(), (a, f)
            assert again["info"] == r["info"] == bare["info"] and all(again[k] == r[k] for k in ("seq", "germ", "mask"))
            assert ctx.stat("mutations_cols") == int(r["counts"]["cols"].sum())
            out["calls" if with_d else "calls_no_d"].append(_pack(r))
    # every case in one call: one launch whatever n is; limit = NULL is the contig's length
    ctx.profile_reset()
    whole = ctx.mutations(ct, v, j, d=d, limit=lim)
    out["whole_launches"] = {k: x[1] for k, x in ctx.profile_get().items()}
    out["whole"] = _pack(whole)
    ctx.profile(False)
    out["no_limit"] = _pack(ctx.mutations(ct, v, j, d=d))
    # no contig
    r0 = ctx.mutations([], _hits([], "v"), _hits([], "j"))
    assert r0["counts"]["cols"].shape == (0,) and r0["info"] == dict.fromkeys(M.INFO, 0) and r0["seq"] == []
    # the refusals: one call each, the bad hit on contig 1 of two
    good = [c for c in cs if c["name"] == "d_middle"][0]

    def pair(**kw):
        bad = dict(good)
        for k, val in kw.items():
            bad[k] = val
        return [good, bad]

    def hit(h, **kw):
        return dict(h, **kw)

    vh, jh, dh = good["v"], good["j"], good["d"]
    refused = []
    for what, cs2 in (("v gene out of range", pair(v=hit(vh, gene=11))), ("v gene of class J", pair(v=hit(vh, gene=J0))),
                      ("v gene of class C", pair(v=hit(vh, gene=C1))), ("j gene of class V", pair(j=hit(jh, gene=V0))),
                      ("germ_end past the record", pair(v=H(V2, 5, 1, [("M", 2)]))), ("seq_start 0", pair(v=hit(H(V0, 1, 1, [("M", 9)]), seq_start=0, seq_end=8))),
                      ("germ_start 0", pair(v=hit(H(V0, 5, 1, [("M", 9)]), germ_start=0, germ_end=8))),
                      ("seq_end past len", pair(v=H(V0, 290, 1, [("M", 20)]), j=NONE)),
                      ("op 3", pair(v=hit(vh, runs=[(100 << 4) | 3] + [0] * 63))), ("length 0", pair(v=hit(vh, runs=[0] + [0] * 63))),
                      ("M + I", pair(v=hit(vh, seq_end=vh["seq_end"] + 1))), ("M + D", pair(v=hit(vh, germ_end=vh["germ_end"] + 1))),
                      ("j runs", pair(j=hit(jh, seq_end=jh["seq_end"] - 1)))):
        refused.append(_raises(ctx, what, "contig 1", cs2))
    with pytest.raises(VdjxError, match="contig 1"):                 # a D hit of a gene the D set does not hold; D's own run sums
        ctx.mutations([c["contig"] for c in pair()], _hits(pair(), "v"), _hits(pair(), "j"), d=_hits(pair(d=hit(dh, gene=2)), "d"))
    with pytest.raises(VdjxError, match="contig 1"):
        ctx.mutations([c["contig"] for c in pair()], _hits(pair(), "v"), _hits(pair(), "j"), d=_hits(pair(d=hit(dh, germ_end=dh["germ_end"] + 1)), "d"))
    for bad_limit in (-1, LEN + 1):
        refused.append(_raises(ctx, "limit", "contig 1", pair(), limit=[LEN, bad_limit]))
    two = pair()
    with pytest.raises(VdjxError, match="NUL"):
        ctx.mutations((two[0]["contig"].encode() + b"ACG\0" + two[1]["contig"].encode()[4:], 2, LEN), _hits(two, "v"), _hits(two, "j"))
    with pytest.raises(VdjxError, match="len=4096"):
        ctx.mutations(["A" * 4096], _hits([dict(v=NONE, j=NONE)], "v"), _hits([dict(v=NONE, j=NONE)], "j"))
    # strings of unequal length: one preamble behind every call, under each caller's name
    short = [two[0]["contig"], two[1]["contig"][:-1]]
    for who, call in (("vdjx_mutations", lambda: ctx.mutations(short, _hits(two, "v"), _hits(two, "j"))),
                      ("vdjx_selection", lambda: ctx.selection(short, _hits(two, "v"))),
                      ("vdjx_tree", lambda: ctx.tree(short, [0, 0], [0, 0]))):
        with pytest.raises(VdjxError) as err:
            call()
        assert str(err.value) == f"{who}: contigs of unequal length"
    out["unequal"] = 3
    big = 1 << 20                                                    # (the arrays are zero pages until someone reads them: nobody does)
    zero = np.zeros(big, api.Context.ANNOT_HIT)
    rows = np.zeros(big, api.Context.MUT_ROW)
    rc = ctx.L.vdjx_mutations(ctx.h, b"A" * big, big, 1, zero.ctypes.data, None, zero.ctypes.data, None, None, None, None, rows.ctypes.data, None)
    assert rc != 0 and b"2^20" in ctx.L.vdjx_last_error()
    out["refused"] = len(refused)
    ctx.close()
    return out


def _same(dev, rows, counts, sl, what):
    for k in ("seq", "germ", "mask"):
        assert dev[k] == rows[k][sl], (what, k, [(a, b) for a, b in zip(dev[k], rows[k][sl]) if a != b][:2])
    for f in M.COUNTS:
        a, b = np.asarray(dev["counts"][f], np.int64), np.asarray(counts[f][sl], np.int64)
        assert np.array_equal(a, b), (what, f, np.flatnonzero(a != b).tolist(), a.tolist(), b.tolist())


def _info_of(counts, cs, sl, with_d):
    part = {f: np.asarray(counts[f][sl], np.int64) for f in M.COUNTS}
    trunc = sum(sum(1 for key in (("v", "d", "j") if with_d else ("v", "j")) if c[key]["gene"] >= 0 and c[key]["score"] > 0 and c[key]["n_runs"] > A.RUNS)
                for c in cs[sl])
    info = {k: int(part[k].sum()) for k in ("cols", "v_r", "v_s", "v_stop", "v_na", "v_codons")}
    info.update(contigs=len(cs[sl]), aligned=int((part["flags"] & M.F_V > 0).sum()), clipped=int((part["flags"] & M.F_CLIP > 0).sum()), truncated=trunc)
    return info


@pytest.mark.parametrize("knobs", KNOBS)
def test_mutations_api_vs_model(knobs):
    res = _run_child("_device", "x", _child_env(knobs))
    cs = cases()
    assert res["n"] == len(cs) and len(cs) % CALL == 0 and res["refused"] == 15 and res["unequal"] == 3
    for with_d, key in ((True, "calls"), (False, "calls_no_d")):
        rows, counts, info = model(with_d)
        for k, dev in enumerate(res[key]):
            sl = slice(k * CALL, (k + 1) * CALL)
            _same(dev, rows, counts, sl, (key, k))
            assert dev["info"] == _info_of(counts, cs, sl, with_d), (key, k)
    rows, counts, info = model(True)
    _same(res["whole"], rows, counts, slice(None), "whole")
    assert res["whole"]["info"] == info == _info_of(counts, cs, slice(None), True)
    assert res["whole_launches"] == {"k_mutations": 1}
    no_lim = M.mutations([c["contig"] for c in cs], _hits(cs, "v"), _hits(cs, "d"), _hits(cs, "j"), None, germs(), d_germs())
    _same(res["no_limit"], no_lim[0], no_lim[1], slice(None), "no_limit")
    # what the cases are there for, from the model's side (the device equals it)
    at = {c["name"]: k for k, c in enumerate(cs)}

    def got(name, f):
        return int(counts[f][at[name]])

    assert [got(f"cols{L}", "cols") for L in (1, 63, 64, 65, 128, 129)] == [1, 63, 64, 65, 128, 129]
    assert got("runs64", "cols") == 64 + (119 - 54) + 64 and got("runs64", "flags") == M.F_V | M.F_J
    assert got("runs65_v", "flags") == M.F_TRUNC and got("runs65_v", "cols") == 0 and rows["seq"][at["runs65_v"]] == ""
    assert got("runs65_j", "flags") == M.F_V | M.F_TRUNC and got("runs65_j", "cols") == 50 and info["truncated"] == 3
    assert [got(f"frame{gs}", "v_codons") for gs in (1, 2, 3, 4)] == [13, 12, 13, 13]      # (whole codons inside germ_start .. germ_end)
    assert got("frame2", "v_na") == 4 and got("ends", "j_mis") == 1 and got("end2047", "cols") == 300
    assert [got(f"del{dl}_inside", "cols") for dl in (1, 2, 3)] == [72, 73, 74] and got("del3_between", "v_codons") == 23
    assert got("ins_inside", "v_na") == 1 and got("ins_inside", "v_codons") == 22 and got("ins_between", "v_na") == 0 and got("ins_between", "v_codons") == 23
    assert got("ins_between", "v_r") + got("ins_between", "v_s") + got("ins_between", "v_stop") == 2
    assert got("contig_N", "v_na") == 2 and got("contig_lower", "v_na") == 2 and got("germ_N", "v_na") == 1
    assert [got(f"limit{k}", "v_na") for k in (34, 35, 36, 37, 0, LEN)] == [0, 1, 1, 0, 0, 0]
    assert [got(f"limit{k}", "v_codons") for k in (34, 35, 36, 37, 0, LEN)] == [10, 10, 10, 11, 0, 30]
    assert got("clip1", "flags") == M.F_V | M.F_J | M.F_CLIP and got("clip1", "cols") == 100 + 29
    assert got("clip_all", "flags") == M.F_V | M.F_CLIP and got("clip_all", "cols") == 100
    assert got("clip_on_I", "cols") == 100 + 2 + 20 and rows["germ"][at["clip_on_I"]][100:102] == "--"
    assert got("clip_after_D", "cols") == 100 + 20 and "-" not in rows["seq"][at["clip_after_D"]]
    assert got("j_leading_D", "cols") == 100 + 15 + 22 and info["clipped"] == 4
    k = at["d_middle"]
    assert got("d_middle", "flags") == M.F_V | M.F_J | M.F_D and got("d_middle", "cols") == 100 + 45 + 2 + 40
    assert rows["mask"][k][100:147] == "N" * 47 and rows["germ"][k][100:110] == "N" * 10 and "-" in rows["germ"][k][110:129] and "-" in rows["seq"][k][110:129]
    assert got("d_none", "flags") == M.F_V | M.F_J and rows["germ"][at["d_none"]][100:145] == "N" * 45
    assert rows["germ"][at["d_abuts_v"]][100] != "N" and rows["germ"][at["d_abuts_j"]][146] != "N" and got("d_abuts_j", "flags") & M.F_D
    assert not got("d_outside", "flags") & M.F_D and not got("d_past_j", "flags") & M.F_D and got("d_without_j", "flags") == M.F_V
    assert got("no_v", "flags") == 0 and got("v_score0", "flags") == 0 and got("del250", "cols") == 470 > LEN
    assert {f: got("designed", f) for f in ("v_r", "v_s", "v_stop", "v_na", "v_codons")} == dict(v_r=3, v_s=1, v_stop=2, v_na=0, v_codons=30)
    rows_nd, counts_nd, _ = model(False)
    assert int(counts_nd["flags"][k]) == M.F_V | M.F_J and rows_nd["germ"][k][100:145] == "N" * 45


# ---- vdjer --mutations -------------------------------------------------------------------------------------------------------------------
def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [l.split("\t") for l in lines[1:-1]]


def _mut_line(r):
    return [l for l in r.stderr.splitlines() if l.startswith("mutations: ")]


def _families_hits(_):
    """in a child process: the hits of the golden's contigs against the planted records, through api.Context"""
    from vdjer_amd import annot, api
    ids, seqs, recs, _ = planted_families()
    clean = [(h, q.upper()) for h, q, _ in recs]
    ctx = api.Context(0)
    ginfo = ctx.germline_load(clean)
    hits = ctx.annotate(seqs)
    dinfo = ctx.dsegment_load(clean)
    ws, wl = annot.d_window(hits["v"], hits["j"])
    d = ctx.dcall(seqs, ws, wl, scores=False)["d"]
    junctions, group, _, _ = annot.lineage_inputs(ids, seqs, hits["v"], hits["j"], ginfo["names"])
    clone = ctx.lineage(junctions, group)["clone"]
    ctx.close()
    pack = lambda h: {k: np.asarray(x).tolist() for k, x in h.items()}
    return dict(names=ginfo["names"], d_names=dinfo["names"], v=pack(hits["v"]), j=pack(hits["j"]), d=pack(d), clone=clone.tolist())


def _run_families(d, name, extra, env):
    """one run of the e2e_families input with the planted ig_vdj.fa, in a directory of its own"""
    run = d / name
    run.mkdir()
    argv = [os.path.join(ROOT, "vdjer_amd", "vdjer"), "--in", "../reads.txt", "--chain", "IGH", "--ref-dir", "../ref", "--ins", "175", "--t", "1"] + F.FLAGS + extra
    with open(run / "out.sam", "wb") as so:
        r = subprocess.run(argv, cwd=run, stdout=so, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (run / "vdj_contigs.fa").read_text() == G.text(f"{F.TAG}.contigs.fa.gz")
    return run, r


def test_vdjer_cli_mutations_families(tmp_path):
    ids, seqs, recs, planted = planted_families()
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F._write_fasta(str(tmp_path / "ref" / "ig_vdj.fa"), recs)           # the same records with the designed substitutions planted in ten V records
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    env = _child_env("shipped")
    tables = ["--airr", "a.tsv", "--d-calls", "--lineages", "l.tsv"]
    run, r = _run_families(tmp_path, "with", ["--mutations", "m.tsv"] + tables, env)
    plain, r0 = _run_families(tmp_path, "without", tables, env)
    x = _run_child("_families_hits", "x", env)
    v, j, d = ({k: np.asarray(a) for k, a in x[key].items()} for key in "vjd")
    _, _, germs_, _, dg = parsed_records(recs)
    rows, counts, info = M.mutations(seqs, v, d, j, M.mutation_limit(ids, seqs), germs_, dg)
    head, got = _table(run / "m.tsv")
    assert head == M.COLUMNS + ["clone_id"]
    assert got == M.table_rows(ids, {"v": v, "j": j}, x["names"], rows, counts, x["clone"])
    col = {k: i for i, k in enumerate(head)}
    for c, (kind, _, _) in planted.items():                                # the designed contigs show the designed counts
        want = dict(dict(v_r=0, v_s=0, v_stop=0, v_na=0), **WANT[kind])
        assert {f: int(got[c][col["mu_count_" + f]]) for f in want} == want, (c, kind, got[c][6:])
        cod = int(got[c][col["v_germline_codons"]])
        assert got[c][col["mu_freq_v"]] == "%.4f" % ((want["v_r"] + want["v_s"]) / (3 * cod))
    # ten planted clones, the kinds in turn: S R stop RR S R stop RR S R -- and no other contig differs from its germline V
    assert sum(int(row[col["mu_count_v_r"]] or 0) for row in got) == 3 * 1 + 2 * 2 and any(row[col["clone_id"]] for row in got)
    assert info["v_r"] == 7 and info["v_s"] == 3 and info["v_stop"] == 2 and any(int(f) & M.F_D for f in counts["flags"])
    # the AIRR table: the two alignment cells are filled, nothing else moves
    ha, a1 = _table(run / "a.tsv")
    hb, a0 = _table(plain / "a.tsv")
    sa, ga = ha.index("sequence_alignment"), ha.index("germline_alignment")
    assert ha == hb and len(a1) == len(a0) == len(ids)
    for c, (r1, r_) in enumerate(zip(a1, a0)):
        assert r_[sa] == "" and r_[ga] == "" and r1[sa] == rows["seq"][c] and r1[ga] == rows["germ"][c]
        assert [y for k, y in enumerate(r1) if k not in (sa, ga)] == [y for k, y in enumerate(r_) if k not in (sa, ga)]
    assert (run / "l.tsv").read_bytes() == (plain / "l.tsv").read_bytes()
    # the summary line: the last one, the model's sums; none without the flag, and every other line as it was
    lines = r.stderr.splitlines()
    assert lines[-1] == M.summary_line(info) and _mut_line(r) == [lines[-1]] and _mut_line(r0) == []
    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES", "mutations: "))]
    assert keep(lines) == keep(r0.stderr.splitlines())


def test_vdjer_cli_mutations_with_d_records(tmp_path):
    """e2e_mixed with the D records of tests/test_gpu_dcall.py: the D record's bases lie in the germline row between Ns, the mask holds N"""
    from tests.test_gpu_dcall import _write_d, cli_case, d_records
    from vdjer_amd import synth
    from tests.test_gpu_annot import RECIPES
    tag = "e2e_mixed"
    ids, seqs, names, hits, d_names, d, _ = cli_case(tag)
    rep = synth.make_repertoire(**RECIPES[tag])
    germs_ = rep.v_germ + rep.j_germ
    dg = [s_ for _, s_ in d_records(tag, rep)]
    lim = M.mutation_limit(ids, seqs)
    env = _child_env("shipped")
    _write_inputs(tag, str(tmp_path))
    _write_d(tag, str(tmp_path))
    r = _vdjer(tmp_path, tag, ["--airr", "a.tsv", "--d-calls", "--mutations", "m.tsv"], env)
    rows, counts, info = M.mutations(seqs, hits["v"], d, hits["j"], lim, germs_, dg)
    head, got = _table(tmp_path / "m.tsv")
    assert head == M.COLUMNS and got == M.table_rows(ids, hits, names, rows, counts)
    assert r.stderr.splitlines()[-1] == M.summary_line(info)
    with_d = [c for c in range(len(ids)) if int(counts["flags"][c]) & M.F_D]
    assert with_d
    for c in with_d:
        rec = dg[int(d["gene"][c])]
        a, b = int(d["germ_start"][c]) - 1, int(d["germ_end"][c])
        nv = sum(int(q) >> 4 for q in hits["v"]["runs"][c][:int(hits["v"]["n_runs"][c])])
        gap = got[c][4][nv:nv + int(hits["j"]["seq_start"][c]) - 1 - int(hits["v"]["seq_end"][c]) + int(d["del"][c])]
        assert rec[a:b] in gap.replace("-", "") and gap.strip("N") == gap.strip("N").strip() and set(gap.replace("-", "").replace(rec[a:b], "")) <= {"N"}
        assert set(got[c][5][nv:nv + len(gap)]) == {"N"} and got[c][5][:nv] == got[c][4][:nv]
    # without --d-calls the two germline rows are equal; --mutations needs no --airr
    plain = tmp_path / "plain"
    plain.mkdir()
    _write_inputs(tag, str(plain))
    _write_d(tag, str(plain))
    _vdjer(plain, tag, ["--mutations", "m.tsv"], env)
    rows0, counts0, _ = M.mutations(seqs, hits["v"], None, hits["j"], lim, germs_, [])
    head, got0 = _table(plain / "m.tsv")
    assert got0 == M.table_rows(ids, hits, names, rows0, counts0) and all(row[4] == row[5] for row in got0)
    assert not (plain / "a.tsv").exists()
    # one run under the suite's knobs, one germline per scoring launch of vdjx_annotate: the same bytes
    knobs = tmp_path / "knobs"
    knobs.mkdir()
    _write_inputs(tag, str(knobs))
    _write_d(tag, str(knobs))
    _vdjer(knobs, tag, ["--mutations", "m.tsv", "--d-calls", "--airr", "a.tsv"], _child_env("suite", VDJX_ANNOT_PAIRS="3"))
    assert (knobs / "m.tsv").read_bytes() == (tmp_path / "m.tsv").read_bytes() and (knobs / "a.tsv").read_bytes() == (tmp_path / "a.tsv").read_bytes()


def test_vdjer_cli_mutations_light_chain(tmp_path):
    """e2e_igk, a ref-dir without D records: the table equals the model's; alone or beside --airr it is the same table"""
    from tests.test_gpu_dcall import cli_case
    from vdjer_amd import synth
    from tests.test_gpu_annot import RECIPES
    tag = "e2e_igk"
    ids, seqs, names, hits, _, _, _ = cli_case(tag)
    rep = synth.make_repertoire(**RECIPES[tag])
    env = _child_env("shipped")
    _write_inputs(tag, str(tmp_path))
    r = _vdjer(tmp_path, tag, ["--mutations", "m.tsv"], env)
    rows, counts, info = M.mutations(seqs, hits["v"], None, hits["j"], M.mutation_limit(ids, seqs), rep.v_germ + rep.j_germ, [])
    head, got = _table(tmp_path / "m.tsv")
    assert head == M.COLUMNS and got == M.table_rows(ids, hits, names, rows, counts) and info["aligned"] > 0
    assert r.stderr.splitlines()[-1] == M.summary_line(info)
    both = tmp_path / "both"
    both.mkdir()
    _write_inputs(tag, str(both))
    _vdjer(both, tag, ["--airr", "a.tsv", "--mutations", "m.tsv"], env)
    assert (both / "m.tsv").read_bytes() == (tmp_path / "m.tsv").read_bytes()
    ha, a = A.read_table(both / "a.tsv")
    assert ha == A.AIRR_COLUMNS and [row[7] for row in a] == rows["seq"] and [row[8] for row in a] == rows["germ"]
    # an unwritable file is reported as for the other tables
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    from tests.test_gpu_annot import _argv
    bad = subprocess.run([exe] + _argv(tag) + ["--mutations", "no_such_dir/m.tsv"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=600, env=env)
    assert bad.returncode != 0 and "cannot write no_such_dir/m.tsv" in bad.stderr
