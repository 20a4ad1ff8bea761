"""`vdjer --lineages --lineage-model` on the e2e_families golden against the table and the stderr lines built from
tests/lineage_dist_model.py over api's annotation of the same contigs: a uniform file (the bytes of a run without the flag), a seeded
realistic file under both symmetries, the clone_id of --airr and --trees, the refusals, and a run without the flag, whose bytes the new
flags must not change."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import annot_model as A
from tests import families as F
from tests import golden_util as G
from tests import lineage_dist_cases as LC
from tests import lineage_dist_model as LM
from tests import lineage_model as M
from tests.test_gpu_annot import _child_env
from tests.test_gpu_tables import _sha, golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vdjer_amd", "vdjer")


def _inputs(_):
    """in a child process: what `vdjer --lineages` derives for the golden's contigs, through api.Context"""
    from vdjer_amd import annot, api
    fam = F.build()
    ids, seqs = golden()
    ctx = api.Context(0)
    ginfo = ctx.germline_load(F.records(fam))
    hits = ctx.annotate(seqs)
    junctions, group, vgene, jgene = annot.lineage_inputs(ids, seqs, hits["v"], hits["j"], ginfo["names"])
    ctx.close()
    return dict(junctions=junctions, group=group.tolist(), vgene=vgene, jgene=jgene)


def _argv(extra):
    return [EXE, "--in", "../reads.txt", "--chain", "IGH", "--ref-dir", "../ref", "--ins", "175", "--t", "1"] + F.FLAGS + extra


def _vdjer(d, name, extra, env):
    run = d / name
    run.mkdir()
    with open(run / "out.sam", "wb") as so:
        r = subprocess.run(_argv(extra), cwd=run, stdout=so, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    info = G.manifest()[F.TAG]                                           # contigs, SAM and graph are the golden's whatever tables are asked for
    assert (run / "vdj_contigs.fa").read_text() == G.text(f"{F.TAG}.contigs.fa.gz")
    assert _sha(run / "out.sam") == info["sam"]["sha256"] and _sha(run / "vdjer.dot") == info["dot"]["sha256"]
    return run, r.stderr.splitlines()


def _lines(lines, prefix):
    return [l for l in lines if l.startswith(prefix)]


def test_vdjer_cli_lineage_model_families(tmp_path):
    from vdjer_amd import annot
    env = _child_env("shipped")
    code = "import json; from tests.test_gpu_lineage_dist_cli import _inputs; print('LINCLI', json.dumps(_inputs(0)))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    x = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("LINCLI ")).split(" ", 1)[1])
    ids, _ = golden()
    n = len(ids)
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    weight = LC.weights()["realistic"]
    annot.write_targeting(str(tmp_path / "uniform.tsv"), np.ones((1024, 4), np.uint32))
    annot.write_targeting(str(tmp_path / "real.tsv"), weight, comments=("seeded",))
    table, tinfo = LM.distance_table(weight)
    uniform, uinfo = LM.distance_table(np.ones((1024, 4), np.uint32))
    ham = M.lineage(x["junctions"], x["group"])
    assert ham[2]["items"] > 20 and ham[2]["pairs"] > 20, ham[2]

    def text(model, rows=LM.table_rows):
        return M.table_text(rows(ids, x["junctions"], x["group"], x["vgene"], x["jgene"], model[0], model[1]), False)

    # without the flag: the table of the Hamming model, no new line
    plain, err0 = _vdjer(tmp_path, "plain", ["--lineages", "l.tsv"], env)
    assert (plain / "l.tsv").read_text() == text(ham, M.table_rows) and _lines(err0, "lineages: ") == [M.summary_line(n, ham[2])]
    assert _lines(err0, "lineage model: ") == []
    # a uniform file: the same bytes, and the new line after the lineages: line
    uni, err = _vdjer(tmp_path, "uniform", ["--lineages", "l.tsv", "--lineage-model", "../uniform.tsv"], env)
    mu = LM.lineage(x["junctions"], x["group"], uniform, M.DEFAULT, "avg")
    assert (uni / "l.tsv").read_bytes() == (plain / "l.tsv").read_bytes() and text(mu) == text(ham, M.table_rows)
    at = err.index(M.summary_line(n, ham[2]))
    assert err[at + 1] == LM.model_line("../uniform.tsv", "avg", uinfo, mu[3], mu[2]) and len(_lines(err, "lineage model: ")) == 1
    assert err[at + 1].startswith("lineage model: ../uniform.tsv, symmetry avg, mean 3.4874, costs 1000 .. 1000, ")
    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES", "lineage model: "))]
    assert keep(err) == keep(err0)
    # the seeded realistic file under both symmetries (and another threshold), with --airr and --trees: every clone_id is the model's
    parts = set()
    for name, extra, sym, md in (("avg", [], "avg", M.DEFAULT), ("min", ["--lineage-symmetry", "min"], "min", M.DEFAULT),
                                 ("tight", ["--lineage-symmetry", "avg", "--lineage-dist", "0.05"], "avg", (500, 10000))):
        run, err = _vdjer(tmp_path, name, ["--lineages", "l.tsv", "--lineage-model", "../real.tsv", "--airr", "a.tsv", "--trees", "t.tsv"] + extra, env)
        model = LM.lineage(x["junctions"], x["group"], table, md, sym)
        hamming = M.lineage(x["junctions"], x["group"], md)
        print(f"vdjer --lineage-model {name}: {model[2]}, walked {model[3]}; Hamming {hamming[2]}")
        assert (run / "l.tsv").read_text() == text(model), name
        at = err.index(M.summary_line(n, model[2], md))
        assert err[at + 1] == LM.model_line("../real.tsv", sym, tinfo, model[3], model[2]), (name, err[at + 1])
        cid = [f"lin_{k + 1}" if k >= 0 else "" for k in model[0].tolist()]
        head, rows = A.read_table(run / "a.tsv")
        assert [r_[head.index("clone_id")] for r_ in rows] == cid, name
        trows = [l.split("\t") for l in (run / "t.tsv").read_text().splitlines()]
        assert trows[0][:2] == ["sequence_id", "clone_id"] and [r_[1] if len(r_) > 1 else "" for r_ in trows[1:]] == cid, name
        parts.add(frozenset(M.partition(model[0])))
        assert model[2]["items"] == ham[2]["items"] and model[2]["pairs"] == ham[2]["pairs"]
    assert len(parts) >= 2                                                  # the runs do not all give one partition
    # two ranks (on one device): rank 0 writes the same table
    two, err = _vdjer(tmp_path, "two", ["--gpus", "2", "--lineages", "l.tsv", "--lineage-model", "../real.tsv"],
                      _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert (two / "l.tsv").read_bytes() == (tmp_path / "avg" / "l.tsv").read_bytes() and len(_lines(err, "lineage model: ")) == 1


@pytest.mark.parametrize("extra,message", [(["--lineage-model", "t.tsv"], "it needs --lineages <file>"),
                                           (["--lineages", "l.tsv", "--lineage-symmetry", "avg"], "it needs --lineage-model <file>"),
                                           (["--lineages", "l.tsv", "--lineage-model", "t.tsv", "--lineage-symmetry", "both"], "--lineage-symmetry must be avg"),
                                           (["--lineages", "l.tsv", "--lineage-model", "none.tsv"], "--lineage-model: cannot read none.tsv"),
                                           (["--lineages", "l.tsv", "--lineage-model", "short.tsv"], "--lineage-model: short.tsv holds 1023 5-mers")])
def test_vdjer_cli_lineage_model_refusals(tmp_path, extra, message):
    """each exits before the first ELAPSED_SECS marker (before any GPU work), with a message, and writes no table"""
    from vdjer_amd import annot
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    run = tmp_path / "run"
    run.mkdir()
    annot.write_targeting(str(run / "t.tsv"), LC.weights()["realistic"])
    (run / "short.tsv").write_text("".join((run / "t.tsv").read_text().splitlines(True)[:-1]))
    r = subprocess.run(_argv(extra), cwd=run, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=_child_env("shipped"))
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr and message in r.stderr, r.stderr[-600:]
    assert not (run / "l.tsv").exists() and not (run / "vdj_contigs.fa").exists()
