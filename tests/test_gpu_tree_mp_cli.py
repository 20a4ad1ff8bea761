"""`vdjer --lineages --trees-mp --trees-mp-newick` on the e2e_families golden: the table, the Newick lines and the stderr line are the
ones tests/tree_mp_model.py composes over api's annotation of the same contigs (the inputs of tests/test_gpu_tree_nj_cli.py); a
`--trees-nj` run writes what it writes without the new flags, byte for byte; the refusals; --gpus 2.  --lineage-dist 0.2 as there: the
golden then has lineages of four and more members, which are searched (asserted below)."""
import json
import subprocess
import sys

import numpy as np
import pytest

from tests import families as F
from tests import lineage_model as M
from tests import tree_mp_model as P
from tests.test_gpu_annot import _child_env
from tests.test_gpu_lineage_dist_cli import _argv, _lines, _vdjer
from tests.test_gpu_tables import golden
from tests.test_gpu_tree_nj_cli import DIST, MD, ROOT

pytestmark = pytest.mark.gpu


def test_vdjer_cli_trees_mp_families(tmp_path):
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
    member = clone >= 0
    anchor, prio = np.where(member, x["anchor"], 0).astype(np.int32), np.where(member, x["prio"], 0).astype(np.uint32)
    want = P.tree_mp(seqs, clone, anchor, prio)
    assert want["info"]["searched"] > 0 and want["info"]["candidates"] > 0 and want["info"]["parsimony"] > 0
    table = P.table_text(P.table_rows(ids, seqs, clone, anchor, want))
    newick = P.newick_text(ids, clone, want)
    lengths = annot.tree_mp_lengths(want["parent"], want["mutations"], want["clone"])
    assert np.array_equal(lengths, P.lengths_of(want))
    assert annot.tree_nj_newick(ids, clone, want["parent"], lengths) == [l.split("\t", 1)[1] for l in newick.splitlines()]

    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES"))]
    base = ["--lineages", "l.tsv", "--lineage-dist", DIST]
    old = base + ["--trees", "t.tsv", "--trees-nj", "n.tsv", "--trees-newick", "n.nwk"]
    plain, err0 = _vdjer(tmp_path, "plain", old, env)
    run, err = _vdjer(tmp_path, "mp", old + ["--trees-mp", "m.tsv", "--trees-mp-newick", "m.nwk"], env)
    assert (run / "m.tsv").read_text() == table and (run / "m.nwk").read_text() == newick
    for f in ("l.tsv", "t.tsv", "n.tsv", "n.nwk"):                                    # the old files are what they were
        assert (run / f).read_bytes() == (plain / f).read_bytes(), f
    assert not (plain / "m.tsv").exists()
    assert _lines(err0, "trees mp: ") == [] and [l for l in keep(err) if not l.startswith("trees mp: ")] == keep(err0)
    at = next(i for i, l in enumerate(err) if l.startswith("trees nj: "))
    assert err[at + 1] == P.summary_line(want["info"]) and len(_lines(err, "trees mp: ")) == 1
    # without --trees-nj and --trees: the same table
    alone, err = _vdjer(tmp_path, "alone", base + ["--trees-mp", "m.tsv"], env)
    assert (alone / "m.tsv").read_text() == table and not (alone / "m.nwk").exists() and _lines(err, "trees mp: ") == [P.summary_line(want["info"])]
    assert _lines(err, "trees nj: ") == [] and _lines(err, "trees: ") == []
    # the refusals, each before any GPU work
    for extra, word in [(["--trees-mp", "m.tsv"], "it needs --lineages"), (base + ["--trees-mp-newick", "m.nwk"], "it needs --trees-mp")]:
        d = tmp_path / ("no" + str(len(extra)))
        d.mkdir()
        r = subprocess.run(_argv(extra), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
        assert r.returncode != 0 and word in r.stderr and "ELAPSED_SECS" not in r.stderr and not (d / "m.tsv").exists(), r.stderr[-500:]
    d = tmp_path / "unwritable"
    d.mkdir()
    for extra, name in [(base + ["--trees-mp", "missing/m.tsv"], "missing/m.tsv"), (base + ["--trees-mp", "m.tsv", "--trees-mp-newick", "missing/m.nwk"], "missing/m.nwk")]:
        r = subprocess.run(_argv(extra), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
        assert r.returncode != 0 and f"cannot write {name}" in r.stderr and "trees mp: " not in r.stderr, r.stderr[-500:]
    # two ranks (on one device): rank 0 calls and writes the same files
    two, err = _vdjer(tmp_path, "two", ["--gpus", "2"] + base + ["--trees-mp", "m.tsv", "--trees-mp-newick", "m.nwk"],
                      _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert (two / "m.tsv").read_text() == table and (two / "m.nwk").read_text() == newick and len(_lines(err, "trees mp: ")) == 1
