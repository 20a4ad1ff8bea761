"""vdjx_quant on the GPU: the contig abundances (RSEM's paired-end EM over map_emit's placements) against the float64 numpy model of
tests/quant_model.py, and `vdjer --quant` on every e2e golden.  Everything runs under both the suite's scorer knobs and the shipped
ones (test_cli_e2e.py::_child_env): the API checks in a child process of each environment, since the knobs are read once per process."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import golden_util as G
from tests import quant_model as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = ["e2e_tiled", "e2e_mixed", "e2e_k25", "e2e_igk", "e2e_igl", "e2e_rl100", "e2e_rl151"]
KNOBS = ["suite", "shipped"]


def _child_env(knobs: str, **extra):
    env = dict(os.environ, **extra)
    if knobs == "shipped":
        env.pop("VDJX_HIT_CHUNK", None)
        env.pop("VDJX_GROUP_MIN", None)
    return env


def _golden_contigs(tag):
    fa = G.text(f"{tag}.contigs.fa.gz").splitlines()
    return [fa[i][1:] for i in range(0, len(fa), 2)], [fa[i + 1] for i in range(0, len(fa), 2)]


def _point(s, pos):
    b = s[pos]
    return s[:pos] + ("ACGT"[("ACGT".index(b) + 1) % 4] if b in "ACGT" else "A") + s[pos + 1:]


def _multi_set(seqs, clones, L=360):
    """the contigs, point variants of each at three positions, and windows of its clone shifted by 1-20 bases: most pairs place on
    several contigs"""
    out = list(seqs)
    for s in seqs:
        out += [_point(s, pos) for pos in (40, 180, 320)]
        for cl in clones:
            at = cl.find(s)
            if at < 0:
                continue
            for sh in (1, 5, 13, 20):
                for a in (at - sh, at + sh):
                    if 0 <= a and a + L <= len(cl):
                        out.append(cl[a:a + L])
            break
    return out


def _triples(offs, pairs):
    contig = np.repeat(np.arange(offs.shape[0] - 1), np.diff(offs).astype(np.int64))
    return pairs["pair_id"].astype(np.int64), contig, pairs["insert"].astype(np.int64)


def _context(pool):
    from vdjer_amd import api
    ctx = api.Context(0)
    p = ctx.pool_load(pool.primary, pool.secondary, pool.rl)
    ctx.read_index_build(p, pool.pair_id, pool.read_num, pool.is_rc, pool.reg_rank, pool.n_pairs)
    return ctx, p


def _api_checks(tag):
    """the checks of one golden case (run in a child process per knob setting)"""
    import ctypes as C
    from vdjer_amd._lib import VdjxError, check
    c = G.Case(tag)
    ctx, p = _context(c.pool)
    ctx.sam_names_load(c.pool.names())
    ids, seqs = _golden_contigs(tag)
    S = _multi_set(seqs, c.clones)
    offs, pairs = ctx.map_emit(S)
    pr, ct, ins = _triples(offs, pairs)
    _, deg = np.unique(pr, return_counts=True)
    assert (deg > 1).sum() > deg.size // 2, ((deg > 1).sum(), deg.size)

    # fixed iteration count: the numpy model to 1e-9
    N, info = ctx.quant(S, tol=0, max_iter=200)
    Nm, im = Q.quant(pr, ct, ins, len(S), 360, tol=0, max_iter=200)
    np.testing.assert_allclose(N, Nm, rtol=1e-9, atol=1e-12)
    assert (info["pairs"], info["alignments"], info["unique_pairs"], info["iterations"]) == (im["pairs"], im["alignments"], im["unique_pairs"], 200)
    assert not info["converged"] and info["eff_len"] == pytest.approx(im["eff_len"], rel=1e-12)
    assert N.sum() == pytest.approx(im["pairs"], rel=1e-9)
    # the default stop rule
    N2, info2 = ctx.quant(S)
    Nm2, im2 = Q.quant(pr, ct, ins, len(S), 360)
    np.testing.assert_allclose(N2, Nm2, rtol=1e-6, atol=1e-9)
    assert abs(info2["iterations"] - im2["iterations"]) <= 1 and info2["converged"] == im2["converged"], (info2, im2)
    # bitwise reproducible
    N3, info3 = ctx.quant(S)
    assert N3.tobytes() == N2.tobytes() and info3 == info2

    # the SAM text of an earlier vdjx_sam_text stays valid, and the next one is the same
    raw, n, ln = ctx.pack_strings(seqs)
    cat, off = ctx._ids(ids, n)
    txt, nb = C.c_char_p(), C.c_uint64()
    check(ctx.L.vdjx_sam_text(ctx.h, raw, n, ln, cat, off.ctypes.data_as(C.c_void_p), C.byref(txt), C.byref(nb)), "vdjx_sam_text")
    addr = C.cast(txt, C.c_void_p).value
    before = bytes((C.c_char * nb.value).from_address(addr))
    ctx.quant(S, max_iter=50)
    assert bytes((C.c_char * nb.value).from_address(addr)) == before
    assert ctx.sam_text_device(seqs, ids) == before
    head = "@HD\tVN:1.4\tSO:unsorted\n" + "".join(f"@SQ\tSN:{i}\tLN:{len(s)}\n" for i, s in zip(ids, seqs))
    assert head + before.decode() == G.text(f"{tag}.sam.gz")

    # edge cases: no contig; contigs no read maps to; a pair placed twice on one contig; refusals
    N0, i0 = ctx.quant([])
    assert N0.shape == (0,) and i0["pairs"] == 0 and i0["iterations"] == 0
    rng = np.random.default_rng(7)
    junk = ["".join(rng.choice(list("ACGT"), 360)) for _ in range(3)]
    Nj, ij = ctx.quant(junk)
    assert Nj.tolist() == [0.0, 0.0, 0.0] and ij["pairs"] == 0 and ij["alignments"] == 0
    Nmix, _ = ctx.quant(seqs + junk, tol=0, max_iter=20)
    assert Nmix[len(seqs):].tolist() == [0.0, 0.0, 0.0]
    # (240 bases with 120 of them again before or after: a read 1 inside the repeated part lies twice on the contig, its mate once --
    # whichever strand read 1 comes from)
    dup = [s[:240] + s[:120] for s in seqs] + [s[120:240] + s[:240] for s in seqs] + [s[120:] + s[120:240] for s in seqs] + [s[240:] + s[120:] for s in seqs]
    o_d, p_d = ctx.map_emit(dup)
    pr_d, ct_d, ins_d = _triples(o_d, p_d)
    # (the reference's quick_map_process_contig places such a pair twice, quick_map3.c:196-232; whatever map_emit returns for these
    # contigs, quant must agree with the model fed by it)
    Nd, idd = ctx.quant(dup, tol=0, max_iter=50)
    Nmd, imd = Q.quant(pr_d, ct_d, ins_d, len(dup), 360, tol=0, max_iter=50)
    np.testing.assert_allclose(Nd, Nmd, rtol=1e-9, atol=1e-12)
    assert idd["pairs"] == imd["pairs"] and idd["alignments"] == imd["alignments"]
    with pytest.raises(VdjxError):
        ctx.quant([seqs[0], seqs[0][:-1]])
    with pytest.raises(VdjxError):
        ctx.quant((b"A" * 359 + b"\0" + b"C" * 360, 2, 360))          # (a shorter contig inside the raw characters)
    with pytest.raises(VdjxError):
        ctx.quant(seqs, max_iter=0)
    with pytest.raises(VdjxError):
        ctx.quant(seqs, tol=-1.0)
    p.free()
    ctx.close()
    return info2


@pytest.mark.parametrize("knobs", KNOBS)
@pytest.mark.parametrize("tag", ["e2e_mixed", "e2e_k25", "e2e_rl151"])
def test_quant_api_multi_mapping_vs_numpy(tag, knobs):
    code = f"import json; from tests.test_gpu_quant import _api_checks; print('QUANT', json.dumps(_api_checks({tag!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=_child_env(knobs))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    info = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("QUANT ")).split(" ", 1)[1])
    assert info["alignments"] > info["pairs"] > 0


def _block_edge_checks(P):
    """e2e_mixed cut down to its first P pairs: with P one below and one above the block of the device-wide scan (vdjx_scan.h) the
    degree scan ends inside its first block or one element into its second, and the pairs no contig places have degree zero"""
    from vdjer_amd import synth
    c = G.Case("e2e_mixed")
    pl = c.pool
    keep = pl.pair_id < P
    npri = pl.primary.shape[0]
    rank = np.argsort(np.argsort(pl.reg_rank[keep], kind="stable"), kind="stable").astype(np.uint32)     # (dense again; a read's two records stay neighbours)
    pool = synth.ReadPool(pl.rl, pl.primary[keep[:npri]], pl.secondary[keep[npri:]], pl.pair_id[keep], pl.read_num[keep], pl.is_rc[keep], rank, P)
    ctx, p = _context(pool)
    _, seqs = _golden_contigs("e2e_mixed")
    S = _multi_set(seqs, c.clones)
    offs, pairs = ctx.map_emit(S)
    pr, ct, ins = _triples(offs, pairs)
    placed = np.unique(pr)
    assert 0 < placed.size < P and int(placed.max()) < P, (placed.size, P)            # some pairs of degree zero
    assert placed.size < placed.max() + 1, "no pair of degree zero before the last placed one"
    N, info = ctx.quant(S, tol=0, max_iter=50)
    Nm, im = Q.quant(pr, ct, ins, len(S), 360, tol=0, max_iter=50)
    np.testing.assert_allclose(N, Nm, rtol=1e-9, atol=1e-12)
    assert (info["pairs"], info["alignments"], info["unique_pairs"]) == (im["pairs"], im["alignments"], im["unique_pairs"])
    assert info["pairs"] == placed.size
    p.free()
    ctx.close()
    return info


@pytest.mark.parametrize("side", [-1, 1])
def test_quant_pair_count_around_a_scan_block(side):
    from tests.scan_shapes import BLOCK
    code = f"import json; from tests.test_gpu_quant import _block_edge_checks; print('QUANT', json.dumps(_block_edge_checks({BLOCK + side})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=_child_env("suite"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    info = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("QUANT ")).split(" ", 1)[1])
    assert info["alignments"] > info["pairs"] > 0


def _write_inputs(c, d):
    os.makedirs(os.path.join(d, "ref"), exist_ok=True)
    c.pool.write_reads_file(os.path.join(d, "reads.txt"))
    with open(os.path.join(d, "ref", "v_region.fa"), "w") as f:
        f.write(">v_region\n" + c.v_region + "\n")
    for fn, codes in (("v_index", c.v_codes), ("j_index", c.j_codes)):
        with open(os.path.join(d, "ref", fn), "w") as f:
            f.write("".join(f"{int(x)}\t0\n" for x in codes))
    open(os.path.join(d, "ref", "ig_vdj.fa"), "w").write(">x\nACGT\n")


def _argv(tag):
    m = G.manifest()
    info = m["e2e"][tag] if tag in m["e2e"] else m["e2e_chains"][tag]
    return ["--in", "reads.txt", "--chain", info.get("chain", "IGH"), "--ref-dir", "ref", "--ins", str(info.get("ins", 175)), "--t", "1"] + info["flags"]


@pytest.mark.parametrize("knobs", KNOBS)
@pytest.mark.parametrize("tag", E2E)
def test_vdjer_cli_quant_table(tag, knobs, tmp_path):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    c = G.Case(tag)
    _write_inputs(c, str(tmp_path))
    r = subprocess.run([exe] + _argv(tag) + ["--quant", "q.tsv"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600, env=_child_env(knobs))
    assert r.returncode == 0, r.stderr[-3000:]
    # the outputs and the stage log are what they are without --quant
    assert (tmp_path / "vdj_contigs.fa").read_text() == G.text(f"{tag}.contigs.fa.gz")
    assert r.stdout == G.text(f"{tag}.sam.gz")
    assert (tmp_path / "vdjer.dot").read_text() == G.text(f"{tag}.dot.gz")
    lines = r.stderr.splitlines()
    marks = [l.split("\t")[1] for l in lines if l.startswith("ELAPSED_SECS\t")]
    assert marks == json.load(open(os.path.join(G.GOLD, "stage_markers.json")))["markers"]
    q_at = next(i for i, l in enumerate(lines) if l.startswith("quant: "))
    assert q_at > max(i for i, l in enumerate(lines) if l.startswith("ELAPSED_SECS\t"))
    # the table: RSEM's columns, one row per contig in vdj_contigs.fa order, expected_count = the model of the golden SAM
    head, rows = Q.read_table(tmp_path / "q.tsv")
    assert head == Q.HEADER
    ids, seqs = _golden_contigs(tag)
    assert [r_[0] for r_ in rows] == ids and [r_[1] for r_ in rows] == ids and all(r_[2] == "360" for r_ in rows)
    sids, L, names, a = Q.sam_placements(G.text(f"{tag}.sam.gz"))
    assert sids == ids
    N, im = Q.quant(a[:, 0], a[:, 1], a[:, 2], len(ids), L)
    assert [r_[4] for r_ in rows] == ["%.2f" % x for x in N]
    assert [r_[3] for r_ in rows] == ["%.2f" % im["eff_len"]] * len(ids)
    assert abs(sum(float(r_[4]) for r_ in rows) - len(set(names))) < 1e-6
    assert abs(sum(float(r_[5]) for r_ in rows) - 1e6) < 0.01 * len(rows) + 1e-6
    assert all(r_[7] == ("100.00" if float(r_[4]) > 0 else "0.00") for r_ in rows)
    assert f"{len(set(names))} pairs placed" in lines[q_at]


def test_vdjer_cli_quant_refuses_gpus_n(tmp_path):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    tag = "e2e_mixed"
    _write_inputs(G.Case(tag), str(tmp_path))
    r = subprocess.run([exe] + _argv(tag) + ["--gpus", "2", "--quant", "q.tsv"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300, env=dict(os.environ, VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="60"))
    assert r.returncode != 0
    assert "--quant runs on one GPU only" in r.stderr
    assert not (tmp_path / "q.tsv").exists() and not (tmp_path / "vdj_contigs.fa").exists()


def _at_size_checks(pairs):
    from tests import midscale_util as M
    from vdjer_amd import synth
    case = M.cases()["mid_cfg1"]
    rep = M.gen.make_rep(case)
    pool = synth.make_reads_cb(rep, pairs, noise_frac=case["noise"], seed=case["seed"] + 13, device="cuda:0").to_host()
    ctx, p = _context(pool)
    # windows of 600 clones at three offsets each, and a point variant of every window
    S = []
    for cl in rep.clones[:600]:
        for a in (60, 75, 90):
            if a + 360 <= len(cl):
                S += [cl[a:a + 360], _point(cl[a:a + 360], 200)]
    offs, pr_ = ctx.map_emit(S)
    pr, ct, ins = _triples(offs, pr_)
    ctx.quant(S, tol=0, max_iter=2)                                         # (warm-up)
    t0 = time.perf_counter()
    N, info = ctx.quant(S, tol=0, max_iter=30)
    t_fixed = time.perf_counter() - t0
    Nm, im = Q.quant(pr, ct, ins, len(S), 360, tol=0, max_iter=30)
    np.testing.assert_allclose(N, Nm, rtol=1e-9, atol=1e-12)
    assert (info["pairs"], info["alignments"]) == (im["pairs"], im["alignments"])
    t0 = time.perf_counter()
    Nd, infod = ctx.quant(S)
    t_def = time.perf_counter() - t0
    p.free()
    ctx.close()
    return dict(pairs=pairs, contigs=len(S), placed_pairs=info["pairs"], alignments=info["alignments"], multi_placed=info["pairs"] - info["unique_pairs"],
                wall_s_30_iterations=round(t_fixed, 4), wall_s_default=round(t_def, 4), iterations_default=infod["iterations"])


def test_quant_one_million_pairs_multi_mapping():
    code = "import json; from tests.test_gpu_quant import _at_size_checks; print('QUANT', json.dumps(_at_size_checks(1_000_000)))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1200,
                       env=_child_env("shipped"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("QUANT ")).split(" ", 1)[1])
    print(res)
    assert res["multi_placed"] > 0 and res["alignments"] > res["placed_pairs"]
