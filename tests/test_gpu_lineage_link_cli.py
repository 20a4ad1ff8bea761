"""`vdjer --lineages --lineage-link` on the e2e_families golden: `single` and no flag give identical files and stderr; `complete` and
`average` give the table composed from tests/lineage_link_model.py over api's annotation of the same contigs (annot.lineage_inputs), the
clone_id of --airr and --trees, and the new stderr line after the lineages: line; with --lineage-model and --lineage-symmetry; with --gpus 2.
The runs use --lineage-dist 0.08, found once with the model: there the golden's 92 eligible junctions make 80 lineages under single, 82
under complete and 81 under average linkage (asserted below -- a run where the three agree would show nothing)."""
import json
import os
import subprocess
import sys

import numpy as np

import pytest

from tests import annot_model as A
from tests import families as F
from tests import lineage_dist_cases as LC
from tests import lineage_dist_model as LM
from tests import lineage_link_model as KM
from tests import lineage_model as M
from tests.test_gpu_annot import _child_env
from tests.test_gpu_lineage_dist_cli import _lines, _vdjer
from tests.test_gpu_tables import golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST, MD = "0.08", (800, 10000)


def test_vdjer_cli_lineage_link_families(tmp_path):
    from vdjer_amd import annot
    env = _child_env("shipped")
    env.pop("VDJX_LINK_CELLS", None)
    code = "import json; from tests.test_gpu_lineage_dist_cli import _inputs; print('LINCLI', json.dumps(_inputs(0)))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    x = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("LINCLI ")).split(" ", 1)[1])
    ids, _ = golden()
    n = len(ids)
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    model = {link: KM.lineage(x["junctions"], x["group"], MD, link) for link in KM.LINKAGE}
    parts = {link: M.partition(model[link][0]) for link in KM.LINKAGE}
    assert parts["single"] != parts["complete"] != parts["average"] != parts["single"]       # the linkage changes the golden's lineages at this threshold
    assert [model[link][2]["clones"] for link in KM.LINKAGE] == [80, 82, 81]

    def text(m, rows=M.table_rows):
        return M.table_text(rows(ids, x["junctions"], x["group"], x["vgene"], x["jgene"], m[0], m[1]), False)

    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES"))]
    # no flag and `single`: the same files and the same stderr, no new line
    base = ["--lineages", "l.tsv", "--lineage-dist", DIST, "--airr", "a.tsv", "--trees", "t.tsv"]
    plain, err0 = _vdjer(tmp_path, "plain", base, env)
    single, err1 = _vdjer(tmp_path, "single", base + ["--lineage-link", "single"], env)
    assert (plain / "l.tsv").read_text() == text(model["single"])
    for f in ("l.tsv", "a.tsv", "t.tsv"):
        assert (single / f).read_bytes() == (plain / f).read_bytes(), f
    assert keep(err1) == keep(err0) and _lines(err0, "lineage link: ") == [] and _lines(err0, "lineages: ") == [M.summary_line(n, model["single"][2], MD)]
    # complete and average: the model's table, clone_id everywhere, the new line after the lineages: line
    for link in ("complete", "average"):
        run, err = _vdjer(tmp_path, link, base + ["--lineage-link", link], env)
        m = model[link]
        assert (run / "l.tsv").read_text() == text(m), link
        at = err.index(M.summary_line(n, m[2], MD))
        assert err[at + 1] == KM.link_line(link, m[2], m[3]) and len(_lines(err, "lineage link: ")) == 1, (link, err[at + 1])
        cid = [f"lin_{k + 1}" if k >= 0 else "" for k in m[0].tolist()]
        head, rows = A.read_table(run / "a.tsv")
        assert [r_[head.index("clone_id")] for r_ in rows] == cid, link
        trows = [l.split("\t") for l in (run / "t.tsv").read_text().splitlines()]
        assert [r_[1] if len(r_) > 1 else "" for r_ in trows[1:]] == cid, link
        assert (run / "l.tsv").read_bytes() != (plain / "l.tsv").read_bytes()
        assert [l for l in keep(err) if not l.startswith(("lineages: ", "lineage link: ", "trees: "))] == \
               [l for l in keep(err0) if not l.startswith(("lineages: ", "trees: "))]
    assert err[at + 1].startswith("lineage link: average, ") and err[at + 1].endswith(" merges, 81 lineages of 80 under single linkage, 1 batches")
    # under a distance model, with the symmetry: the line comes after the model's
    weight = LC.weights()["realistic"]
    annot.write_targeting(str(tmp_path / "real.tsv"), weight, comments=("seeded",))
    table, tinfo = LM.distance_table(weight)
    run, err = _vdjer(tmp_path, "model", ["--lineages", "l.tsv", "--lineage-dist", DIST, "--lineage-model", "../real.tsv", "--lineage-symmetry", "min",
                                          "--lineage-link", "complete"], env)
    m = KM.lineage(x["junctions"], x["group"], MD, "complete", table, "min")
    ms = LM.lineage(x["junctions"], x["group"], table, MD, "min")
    assert M.partition(m[0]) != M.partition(ms[0])
    assert (run / "l.tsv").read_text() == text(m, LM.table_rows)
    at = err.index(M.summary_line(n, m[2], MD))
    assert err[at + 1] == LM.model_line("../real.tsv", "min", tinfo, ms[3], m[2]) and err[at + 2] == KM.link_line("complete", m[2], m[3])
    # two ranks (on one device): rank 0 calls and writes the same table
    two, err = _vdjer(tmp_path, "two", ["--gpus", "2", "--lineages", "l.tsv", "--lineage-dist", DIST, "--lineage-link", "complete"],
                      _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert (two / "l.tsv").read_bytes() == (tmp_path / "complete" / "l.tsv").read_bytes() and len(_lines(err, "lineage link: ")) == 1
