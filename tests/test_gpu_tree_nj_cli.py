"""`vdjer --lineages --trees-nj --trees-newick` on the e2e_families golden: the table, the Newick lines and the stderr line are the ones
tests/tree_nj_model.py composes over api's annotation of the same contigs (annot.lineage_inputs, annot.tree_inputs); --trees and
--tree-support write what they write without the new flags; the three refusals; --gpus 2.  The runs use --lineage-dist 0.2, found once
with the model: there the golden has lineages of four and more members and lineages of exactly two (asserted below -- a run with neither
would show nothing)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import families as F
from tests import lineage_model as M
from tests import tree_nj_model as N
from tests.test_gpu_annot import _child_env
from tests.test_gpu_lineage_dist_cli import _argv, _lines, _vdjer
from tests.test_gpu_tables import golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST, MD = "0.2", (2000, 10000)


def _nj_inputs(_):
    """in a child process: what `vdjer --lineages --trees-nj` derives for the golden's contigs, through api.Context"""
    from vdjer_amd import annot, api
    fam = F.build()
    ids, seqs = golden()
    ctx = api.Context(0)
    ginfo = ctx.germline_load(F.records(fam))
    hits = ctx.annotate(seqs)
    junctions, group, _, _ = annot.lineage_inputs(ids, seqs, hits["v"], hits["j"], ginfo["names"])
    anchor, prio = annot.tree_inputs(ids, seqs, hits["v"], np.zeros(len(ids), np.int32))      # (of every contig: the caller masks by lineage)
    ctx.close()
    return dict(junctions=junctions, group=group.tolist(), anchor=anchor.tolist(), prio=prio.tolist())


def test_vdjer_cli_trees_nj_families(tmp_path):
    from vdjer_amd import annot
    env = _child_env("shipped")
    env.pop("VDJX_NJ_CELLS", None)
    code = "import json; from tests.test_gpu_tree_nj_cli import _nj_inputs; print('NJCLI', json.dumps(_nj_inputs(0)))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    x = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("NJCLI ")).split(" ", 1)[1])
    ids, seqs = golden()
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    clone = M.lineage(x["junctions"], x["group"], MD)[0]
    sizes = np.bincount(clone[clone >= 0]).tolist()
    assert max(sizes) >= 4 and 2 in sizes, sizes                                      # inferred nodes and joins, and the one-edge tree
    member = clone >= 0
    anchor, prio = np.where(member, x["anchor"], 0).astype(np.int32), np.where(member, x["prio"], 0).astype(np.uint32)
    want = N.tree_nj(seqs, clone, anchor, prio)
    assert want["info"]["internal"] > 0 and want["info"]["parsimony"] > 0
    table = N.table_text(N.table_rows(ids, seqs, clone, anchor, want))
    newick = N.newick_text(ids, clone, want)
    assert annot.tree_nj_newick(ids, clone, want["parent"], want["length"]) == [l.split("\t", 1)[1] for l in newick.splitlines()]

    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES"))]
    base = ["--lineages", "l.tsv", "--lineage-dist", DIST]
    old = base + ["--trees", "t.tsv", "--tree-support", "8"]
    plain, err0 = _vdjer(tmp_path, "plain", old, env)
    run, err = _vdjer(tmp_path, "nj", old + ["--trees-nj", "n.tsv", "--trees-newick", "n.nwk"], env)
    assert (run / "n.tsv").read_text() == table and (run / "n.nwk").read_text() == newick
    for f in ("l.tsv", "t.tsv"):                                                      # the old tables are what they were
        assert (run / f).read_bytes() == (plain / f).read_bytes(), f
    assert _lines(err0, "trees nj: ") == [] and [l for l in keep(err) if not l.startswith("trees nj: ")] == keep(err0)
    at = next(i for i, l in enumerate(err) if l.startswith("tree support: "))
    assert err[at + 1] == N.summary_line(want["info"]) and len(_lines(err, "trees nj: ")) == 1
    # without --trees: the same table
    alone, err = _vdjer(tmp_path, "alone", base + ["--trees-nj", "n.tsv"], env)
    assert (alone / "n.tsv").read_text() == table and not (alone / "n.nwk").exists() and _lines(err, "trees nj: ") == [N.summary_line(want["info"])]
    assert _lines(err, "trees: ") == []
    # the refusals, each before any GPU work
    for extra, word in [(["--trees-nj", "n.tsv"], "it needs --lineages"), (base + ["--trees-newick", "n.nwk"], "it needs --trees-nj")]:
        d = tmp_path / ("no" + str(len(extra)))
        d.mkdir()
        r = subprocess.run(_argv(extra), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
        assert r.returncode != 0 and word in r.stderr and "ELAPSED_SECS" not in r.stderr and not (d / "n.tsv").exists(), r.stderr[-500:]
    d = tmp_path / "unwritable"
    d.mkdir()
    for extra, name in [(base + ["--trees-nj", "missing/n.tsv"], "missing/n.tsv"), (base + ["--trees-nj", "n.tsv", "--trees-newick", "missing/n.nwk"], "missing/n.nwk")]:
        r = subprocess.run(_argv(extra), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
        assert r.returncode != 0 and f"cannot write {name}" in r.stderr and "trees nj: " not in r.stderr, r.stderr[-500:]
    # two ranks (on one device): rank 0 calls and writes the same files
    two, err = _vdjer(tmp_path, "two", ["--gpus", "2"] + base + ["--trees-nj", "n.tsv", "--trees-newick", "n.nwk"],
                      _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert (two / "n.tsv").read_text() == table and (two / "n.nwk").read_text() == newick and len(_lines(err, "trees nj: ")) == 1
