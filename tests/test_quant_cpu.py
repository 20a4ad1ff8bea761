"""CPU checks of the contig-abundance model (tests/quant_model.py, the restatement vdjx_quant is tested against) and of the parts of
`vdjer --quant` that run before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

from tests import golden_util as G
from tests import quant_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = ["e2e_tiled", "e2e_mixed", "e2e_k25", "e2e_igk", "e2e_igl", "e2e_rl100", "e2e_rl151"]


@pytest.mark.parametrize("tag", E2E)
def test_model_on_golden_sam_counts_pairs_per_contig(tag):
    """no golden SAM places a pair twice: every r is 1, so the counts are the pairs per contig exactly, after at most two iterations"""
    ids, L, names, a = Q.sam_placements(G.text(f"{tag}.sam.gz"))
    assert L == 360 and len(ids) > 0 and a.shape[0] > 0
    assert np.unique(a[:, 0]).size == a.shape[0]             # (one placement per pair)
    N, info = Q.quant(a[:, 0], a[:, 1], a[:, 2], len(ids), L)
    assert np.array_equal(N, np.bincount(a[:, 1], minlength=len(ids)).astype(np.float64))
    assert info["pairs"] == len(names) == info["unique_pairs"] == info["alignments"]
    assert info["iterations"] <= 2 and info["converged"]
    assert 0 < info["eff_len"] < L


def _multi_set():
    """three contigs: contig 0 holds pairs placed there alone, contigs 1 and 2 share pairs, contig 3 has none; pair 9 is placed twice
    on contig 1"""
    rows = [(0, 0, 170), (1, 0, 180), (2, 0, 175),                       # unique on 0
            (3, 1, 160), (4, 2, 190), (5, 1, 175),                       # unique on 1 / 2
            (6, 1, 170), (6, 2, 170), (7, 1, 200), (7, 2, 210), (8, 2, 150), (8, 1, 150),
            (9, 1, 120), (9, 1, 300), (10, 0, 175), (10, 1, 176), (10, 2, 177)]
    return np.array(rows, np.int64)


def test_model_invariants_on_multi_mapping_set():
    a = _multi_set()
    N, info = Q.quant(a[:, 0], a[:, 1], a[:, 2], 4, 360, tol=0, max_iter=300)
    assert info["pairs"] == 11 and info["alignments"] == a.shape[0] and info["iterations"] == 300 and not info["converged"]
    assert info["unique_pairs"] == 6
    assert N.sum() == pytest.approx(11, rel=1e-12)                      # every placed pair is shared out in full
    assert N[3] == 0.0                                                   # no placement: stays 0
    assert N[0] >= 3 and N[1] >= 2 and N[2] >= 1                         # unique pairs keep their contig's share
    assert np.all(N[:3] <= np.array([4, 7, 6]))
    # the default stop rule ends early and lands near the fixed point
    Nd, infod = Q.quant(a[:, 0], a[:, 1], a[:, 2], 4, 360)
    assert infod["converged"] and infod["iterations"] < 300
    assert np.allclose(Nd, N, rtol=1e-3)


def test_model_edge_cases():
    N, info = Q.quant([], [], [], 3, 360)
    assert np.array_equal(N, np.zeros(3)) and info["pairs"] == 0 and info["iterations"] == 0
    # one pair, two placements on the same contig: the contig explains one pair
    N, info = Q.quant([0, 0], [1, 1], [150, 250], 2, 360)
    assert N.tolist() == [0.0, 1.0] and info["pairs"] == 1 and info["unique_pairs"] == 0


def test_frag_weights_are_a_distribution():
    g, eff, uniq = Q.frag_weights([0, 1, 1, 2], [175, 175, 180, 200], 360)
    assert uniq == 2
    f = np.arange(50, 401)
    h = np.zeros(351)
    h[175 - 50] += 1
    h[200 - 50] += 1
    Pf = (h + 1) / (h + 1).sum()
    assert eff == pytest.approx(float((Pf * (360 - f + 1))[f <= 360].sum()), rel=1e-12)
    assert g[0] == pytest.approx(Pf[125] / (360 - 175 + 1), rel=1e-15)


def _cli_inputs(d):
    open(os.path.join(d, "reads.txt"), "w").write("P r1 1 0 ACGTACGTAC IIIIIIIIII\nP r1 2 1 ACGTACGTAC IIIIIIIIII\n")
    os.makedirs(os.path.join(d, "ref"), exist_ok=True)
    for fn in ("v_index", "j_index"):
        open(os.path.join(d, "ref", fn), "w").write("1\t0\n")
    open(os.path.join(d, "ref", "v_region.fa"), "w").write(">v\nACGT\n")


def test_cli_quant_refuses_sharded_runs_before_any_gpu_work(tmp_path):
    """`--quant` is one GPU only: with VDJX_FORCE_MGPU (the sharded code path on one rank) the command line stops after parsing,
    with a message and without a table -- no GPU is needed to get there"""
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    assert os.path.exists(exe), "build it: make -C vdjer_amd/csrc/host"
    _cli_inputs(str(tmp_path))
    r = subprocess.run([exe, "--in", "reads.txt", "--chain", "IGH", "--ref-dir", "ref", "--ins", "175", "--quant", "q.tsv"], cwd=tmp_path,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=dict(os.environ, VDJX_FORCE_MGPU="1"))
    assert r.returncode != 0
    assert "--quant runs on one GPU only" in r.stderr
    assert "ELAPSED_SECS" not in r.stderr
    assert not (tmp_path / "q.tsv").exists()


def test_cli_usage_names_quant(tmp_path):
    exe = os.path.join(ROOT, "vdjer_amd", "vdjer")
    r = subprocess.run([exe, "--help", "x"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "--quant" in r.stderr
