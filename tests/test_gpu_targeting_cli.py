"""`vdjer --targeting-model` on the e2e_families golden (with the planted V records of tests/test_mutation_cpu.py, so that some contigs
are mutated) against the files and the stderr line built from tests/targeting_model.py over api's annotation of the same contigs: with
--lineages as the groups, alone, at minima of 1 with both classes, under --gpus 2, fed back into --selection --targeting, and beside the
other tables, whose bytes it must not change."""
import os
import subprocess

import numpy as np
import pytest

from tests import families as F
from tests import mutation_model as M
from tests import targeting_model as T
from tests.test_gpu_annot import _child_env
from tests.test_gpu_mutation import _families_hits, _run_child, _run_families  # noqa: F401  (_families_hits runs in the child)
from tests.test_mutation_cpu import parsed_records, planted_families

pytestmark = pytest.mark.gpu


def _line(r):
    return [l for l in r.stderr.splitlines() if l.startswith("targeting model: ")]


def test_vdjer_cli_targeting_families(tmp_path):
    from vdjer_amd import annot
    ids, seqs, recs, planted = planted_families()
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F._write_fasta(str(tmp_path / "ref" / "ig_vdj.fa"), recs)
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    _, _, germs, _, _ = parsed_records(recs)
    env = _child_env("shipped")
    x = _run_child("_families_hits", "x", env)
    v = {k: np.asarray(a) for k, a in x["v"].items()}
    clone = np.asarray(x["clone"])
    lim = M.mutation_limit(ids, seqs)
    n = len(ids)

    def check(run, r, grouped, cls="s", min_sub=50, min_mut=500, counts_file=True):
        cnt, info = T.counts(seqs, v, lim, germs, clone if grouped else None)
        w, lv = T.model(cnt, cls, min_sub, min_mut)
        assert (run / "t.tsv").read_text() == T.model_text("reads", cls, min_sub, min_mut, info, w, lv)
        assert np.array_equal(annot.read_targeting(str(run / "t.tsv")), w)
        if counts_file:
            assert (run / "c.tsv").read_text() == T.counts_text(cnt, lv)
        assert _line(r) == [T.summary_line(info, cls, lv)] and r.stderr.splitlines()[-1] == _line(r)[0]
        return cnt, info, lv

    # 1. the lineages as groups, at the defaults: few changes, so the model falls back to the centre base and the whole sample
    first, r = _run_families(tmp_path, "first", ["--lineages", "l.tsv", "--targeting-model", "t.tsv", "--targeting-counts", "c.tsv"], env)
    cnt, info, lv = check(first, r, True)
    sizes = np.bincount(clone[clone >= 0])
    print(f"vdjer --targeting-model: {info['used']} of {n} contigs used, {info['units']} units, lineages of up to {int(sizes.max())} contigs, {info}")
    assert info["contigs"] == n and 0 < info["units"] <= info["used"] <= n and info["obs_s"] >= 1 and info["obs_s"] + info["obs_r"] >= 7
    assert set(lv.ravel().tolist()) <= {0, 1} and not (first / "a.tsv").exists()
    # 2. alone (the annotation runs by itself, every contig on its own), both classes, minima of 1: levels 5 and 3 appear
    alone, r = _run_families(tmp_path, "alone", ["--targeting-model", "t.tsv", "--targeting-class", "rs", "--targeting-min-sub", "1", "--targeting-min-mut", "1"], env)
    _, info1, lv1 = check(alone, r, False, "rs", 1, 1, counts_file=False)
    assert info1["units"] == info1["used"] >= info["units"] and not (alone / "c.tsv").exists()
    assert len(set(lv1[:, 0].tolist())) >= 3 and len(set(lv1[:, 1].tolist())) >= 3 and 5 in set(lv1.ravel().tolist())
    # 3. the written model is accepted by --selection --targeting; beside the other tables, whose bytes the new flags do not change
    tables = ["--airr", "a.tsv", "--lineages", "l.tsv", "--mutations", "m.tsv", "--selection", "s.tsv", "--targeting", "../first/t.tsv"]
    new = ["--targeting-model", "t.tsv", "--targeting-counts", "c.tsv", "--targeting-class", "s", "--targeting-min-sub", "50", "--targeting-min-mut", "500"]
    full, rf = _run_families(tmp_path, "full", tables + new, env)
    plain, rp = _run_families(tmp_path, "plain", tables, env)
    check(full, rf, True)
    assert (full / "t.tsv").read_bytes() == (first / "t.tsv").read_bytes() and (full / "c.tsv").read_bytes() == (first / "c.tsv").read_bytes()
    sel = [l for l in rf.stderr.splitlines() if l.startswith("selection: ")]
    assert len(sel) == 1 and "targeting ../first/t.tsv," in sel[0]
    for fn in ("a.tsv", "l.tsv", "m.tsv", "s.tsv", "out.sam", "vdjer.dot", "vdj_contigs.fa"):
        assert (full / fn).read_bytes() == (plain / fn).read_bytes(), fn
    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES", "targeting model: "))]
    assert keep(rf.stderr.splitlines()) == keep(rp.stderr.splitlines()) and _line(rp) == [] and not (plain / "t.tsv").exists()
    # (the selection of the same run does not read the model being written: it stays uniform)
    uni, ru = _run_families(tmp_path, "uniform", ["--lineages", "l.tsv", "--selection", "s.tsv", "--targeting-model", "t.tsv"], env)
    assert any(l.startswith("selection: ") and "targeting uniform," in l for l in ru.stderr.splitlines())
    assert (uni / "s.tsv").read_bytes() != (full / "s.tsv").read_bytes() and (uni / "t.tsv").read_bytes() == (first / "t.tsv").read_bytes()
    # 4. two ranks (on one device): rank 0 writes the same bytes
    two, r2 = _run_families(tmp_path, "two", ["--gpus", "2", "--lineages", "l.tsv", "--targeting-model", "t.tsv", "--targeting-counts", "c.tsv"],
                            _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert any("k-mer table sharded over 2 GPUs" in l for l in r2.stderr.splitlines())
    assert (two / "t.tsv").read_bytes() == (first / "t.tsv").read_bytes() and (two / "c.tsv").read_bytes() == (first / "c.tsv").read_bytes()
    assert _line(r2) == [T.summary_line(info, "s", lv)]
    # an unwritable file is reported as for the other tables
    bad = tmp_path / "bad"
    bad.mkdir()
    argv = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vdjer_amd", "vdjer"), "--in", "../reads.txt", "--chain", "IGH", "--ref-dir", "../ref",
            "--ins", "175", "--t", "1"] + F.FLAGS + ["--targeting-model", "no_such_dir/t.tsv"]
    with open(bad / "out.sam", "wb") as so:
        rb = subprocess.run(argv, cwd=bad, stdout=so, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert rb.returncode != 0 and "cannot write no_such_dir/t.tsv" in rb.stderr
