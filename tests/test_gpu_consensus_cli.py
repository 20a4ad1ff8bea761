"""`vdjer --consensus` on the e2e_families golden (with the planted V records of tests/test_mutation_cpu.py) against what the Python entry
points compose from the same contigs -- Context.consensus over the lineages, annot.consensus_hits, Context.mutations and Context.selection on
the pseudo-contigs -- byte for byte: the table, the stderr line and the two blocks the --selection table gains; beside every other table,
whose bytes it must not change; at --consensus-min-freq 0 alone; and under --gpus 2.  Every clone of this golden has a V sequence of its own,
so its lineages show lone voters and off-record members; a consensus over several voters is tests/test_gpu_consensus.py's ground."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import consensus_model as CM
from tests import families as F
from tests import mutation_model as M
from tests.test_gpu_annot import _child_env
from tests.test_gpu_consensus import _none_hits
from tests.test_gpu_mutation import _run_families, _table
from tests.test_gpu_selection_cli import targeting, v_regions
from tests.test_mutation_cpu import parsed_records, planted_families

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_consensus_cli import {fn}; print('CONS', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("CONS ")).split(" ", 1)[1])


def _sel_rows(level, rid, stat, r, K):
    out = []
    for k in range(K):
        g = lambda f: stat[f][r][k]
        sg = float(g("sigma"))
        sg = 0.0 if -0.00005 < sg < 0.0 else sg
        out.append([level, rid, "v" if K == 1 else ("fwr", "cdr")[k], str(int(g("sequences"))), str(int(g("x"))), str(int(g("n")) - int(g("x"))), str(int(g("exp_r"))),
                    str(int(g("exp_s"))), "%.4f" % sg, "%.2f" % float(g("lower")), "%.2f" % float(g("upper")), "%.4f" % float(g("p_positive"))])
    return out


def _families_consensus(num):
    """in a child process: the table rows, the stderr line and the selection blocks (plain; with regions and weights), through api.Context"""
    from vdjer_amd import annot, api
    ids, seqs, recs, _ = planted_families()
    clean = [(h, q.upper()) for h, q, _ in recs]
    names, classes, germs, _, _ = parsed_records(recs)
    ctx = api.Context(0)
    ginfo = ctx.germline_load(clean)
    hits = ctx.annotate(seqs)
    junctions, group, _, _ = annot.lineage_inputs(ids, seqs, hits["v"], hits["j"], ginfo["names"])
    clone = ctx.lineage(junctions, group)["clone"]
    r = ctx.consensus(seqs, hits["v"], limit=M.mutation_limit(ids, seqs), group=clone, min_freq=(num, 10000), counts=True)
    pc, hv = annot.consensus_hits(r["units"], r["cons"], r["germ"])
    mu = ctx.mutations(pc, hv, _none_hits(len(pc)), rows=False)["counts"]
    rows = CM.table_rows(ids, ginfo["names"], r, mu)
    blocks = {}
    for key, kw in (("plain", {}), ("mapped", dict(cdr=v_regions(names, classes, germs)[1], weight=targeting()[1]))):
        se = ctx.selection(pc, hv, **kw)
        K = 2 if kw else 1
        out = []
        for u, (clone_id, seq_id) in enumerate(CM.unit_ids(ids, r)):
            rid = clone_id or seq_id
            out += _sel_rows("consensus", rid, se["stat"], u, K) if int(se["counts"]["flags"][u]) & 1 else [["consensus", rid] + [""] * 10]
        out += _sel_rows("consensus_sample", "reads", se["stat"], len(pc), K)
        blocks[key] = out
    ctx.close()
    members = np.asarray(r["units"]["members"]).tolist()
    return dict(rows=rows, line=CM.summary_line(r["info"], max(members), num), blocks=blocks, info=r["info"], members=members,
                groups=np.asarray(r["units"]["group"]).tolist(), off=np.asarray(r["units"]["off_record"]).tolist(), clones=int(clone.max()) + 1)


def _line(r):
    return [l for l in r.stderr.splitlines() if l.startswith("consensus: ")]


def test_vdjer_cli_consensus_families(tmp_path):
    ids, seqs, recs, planted = planted_families()
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F._write_fasta(str(tmp_path / "ref" / "ig_vdj.fa"), recs)
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    names, classes, germs, _, _ = parsed_records(recs)
    (tmp_path / "r.tsv").write_text("\n".join(v_regions(names, classes, germs)[0]) + "\n")
    (tmp_path / "t.tsv").write_text("\n".join(targeting()[0]) + "\n")
    env = _child_env("shipped")
    want = _run_child("_families_consensus", 6000, env)
    text = lambda rows: "".join("\t".join(row) + "\n" for row in rows)

    # 1. beside every other table, with regions and a targeting model: the table, the line, the two new blocks; nothing else changes
    tables = ["--airr", "a.tsv", "--lineages", "l.tsv", "--mutations", "m.tsv", "--targeting-model", "tm.tsv", "--selection", "s.tsv", "--v-regions", "../r.tsv",
              "--targeting", "../t.tsv"]
    full, rf = _run_families(tmp_path, "full", tables + ["--consensus", "c.tsv"], env)
    plain, rp = _run_families(tmp_path, "plain", tables, env)
    assert (full / "c.tsv").read_text() == CM.table_text(want["rows"])
    assert _line(rf) == [want["line"]] and rf.stderr.splitlines()[-1] == want["line"]
    info = want["info"]
    print(f"vdjer --consensus: {want['line']}; {want['clones']} lineages, members {sorted(set(want['members']))}, off record {sum(want['off'])}")
    assert info["contigs"] == len(ids) and info["units"] == len(want["rows"]) > want["clones"] > 3 and info["used"] == sum(want["members"]) + info["off_record"]
    assert any(g >= 0 for g in want["groups"]) and any(g < 0 for g in want["groups"]) and info["off_record"] > 0      # lineages and lone contigs; off-record members
    assert set(want["members"]) == {1} and max(want["off"]) >= 1     # (tests/test_consensus_cpu.py: why every lineage here has one voter)
    assert (full / "s.tsv").read_text() == (plain / "s.tsv").read_text() + text(want["blocks"]["mapped"])
    assert [row[2] for row in want["blocks"]["mapped"][-2:]] == ["fwr", "cdr"] and int(want["blocks"]["mapped"][-2][3]) >= 1
    for fn in ("a.tsv", "l.tsv", "m.tsv", "tm.tsv", "out.sam", "vdjer.dot", "vdj_contigs.fa"):
        assert (full / fn).read_bytes() == (plain / fn).read_bytes(), fn
    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES", "consensus: "))]
    assert keep(rf.stderr.splitlines()) == keep(rp.stderr.splitlines()) and _line(rp) == [] and not (plain / "c.tsv").exists()
    head, got = _table(full / "c.tsv")
    assert head == CM.COLUMNS
    col = {k: i for i, k in enumerate(head)}
    for row in got:                                                   # a lone voter's consensus is its own bases: cover 1 throughout
        if row[col["members"]] == "1" and row[col["consensus_alignment"]]:
            assert row[col["min_cover"]] == "1" and len(row[col["consensus_alignment"]]) == int(row[col["germline_end"]]) - int(row[col["germline_start"]]) + 1
    # 2. alone with --lineages (the annotation runs by itself), the most common symbol, one region, uniform weights
    common = _run_child("_families_consensus", 0, env)
    alone, ra = _run_families(tmp_path, "alone", ["--lineages", "l.tsv", "--consensus", "c.tsv", "--consensus-min-freq", "0", "--selection", "s.tsv"], env)
    assert (alone / "c.tsv").read_text() == CM.table_text(common["rows"]) and _line(ra) == [common["line"]] and "min share 0.0000" in common["line"]
    assert (alone / "s.tsv").read_text().endswith(text(common["blocks"]["plain"])) and not (alone / "a.tsv").exists()
    assert (alone / "l.tsv").read_bytes() == (full / "l.tsv").read_bytes()
    # 3. two ranks (on one device): rank 0 writes the same bytes
    two, r2 = _run_families(tmp_path, "two", ["--gpus", "2", "--lineages", "l.tsv", "--consensus", "c.tsv", "--consensus-min-freq", "0.6"],
                            _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert any("k-mer table sharded over 2 GPUs" in l for l in r2.stderr.splitlines())
    assert (two / "c.tsv").read_bytes() == (full / "c.tsv").read_bytes() and _line(r2) == [want["line"]]
    # an unwritable file is reported as for the other tables
    bad = tmp_path / "bad"
    bad.mkdir()
    argv = [os.path.join(ROOT, "vdjer_amd", "vdjer"), "--in", "../reads.txt", "--chain", "IGH", "--ref-dir", "../ref",
            "--ins", "175", "--t", "1"] + F.FLAGS + ["--lineages", "l.tsv", "--consensus", "no_such_dir/c.tsv"]
    with open(bad / "out.sam", "wb") as so:
        rb = subprocess.run(argv, cwd=bad, stdout=so, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert rb.returncode != 0 and "cannot write no_such_dir/c.tsv" in rb.stderr
