"""`vdjer --selection-combine mean` and `--selection-test` on the e2e_families golden (the setup of tests/test_gpu_selection_cli.py: planted
V records, a region map, a targeting model) against tests/selection_conv_model.py: the lineage, sample and consensus_sample rows of the
selection table, the test table and the stderr line; `shared` and the flags absent leave the table and stderr byte for byte what they
were; every other table keeps its bytes; --gpus 2."""
import re

import numpy as np
import pytest

from tests import families as F
from tests import mutation_model as M
from tests import selection_conv_model as CM
from tests import selection_model as S
from tests.test_gpu_annot import _child_env
from tests.test_gpu_mutation import _families_hits, _run_child, _run_families, _table  # noqa: F401  (_families_hits runs in the child)
from tests.test_gpu_selection_cli import _same_table, targeting, v_regions
from tests.test_mutation_cpu import parsed_records, planted_families

pytestmark = pytest.mark.gpu


def _consensus_counts(env):
    """in a child process: the count rows of the consensus pseudo-contigs, as `vdjer --consensus --selection` forms them (regions, weights)"""
    import json
    import subprocess
    import sys

    from tests.test_gpu_consensus_cli import ROOT
    code = ("import json, numpy as np\n"
            "from vdjer_amd import annot, api\n"
            "from tests import mutation_model as M\n"
            "from tests.test_mutation_cpu import parsed_records, planted_families\n"
            "from tests.test_gpu_selection_cli import targeting, v_regions\n"
            "ids, seqs, recs, _ = planted_families()\n"
            "clean = [(h, q.upper()) for h, q, _ in recs]\n"
            "names, classes, germs, _, _ = parsed_records(recs)\n"
            "ctx = api.Context(0)\n"
            "ginfo = ctx.germline_load(clean)\n"
            "hits = ctx.annotate(seqs)\n"
            "junctions, group, _, _ = annot.lineage_inputs(ids, seqs, hits['v'], hits['j'], ginfo['names'])\n"
            "clone = ctx.lineage(junctions, group)['clone']\n"
            "r = ctx.consensus(seqs, hits['v'], limit=M.mutation_limit(ids, seqs), group=clone, min_freq=(6000, 10000), counts=True)\n"
            "pc, hv = annot.consensus_hits(r['units'], r['cons'], r['germ'])\n"
            "se = ctx.selection(pc, hv, cdr=v_regions(names, classes, germs)[1], weight=targeting()[1])\n"
            "ctx.close()\n"
            "print('CSC', json.dumps({f: se['counts'][f].tolist() for f in ('obs_r', 'obs_s', 'exp_r', 'exp_s')}))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("CSC ")).split(" ", 1)[1])


def _with_mean(rows, level, conv):
    """the rows of the selection table with the posterior cells of the `level` rows taken from the convolved model's rows, in order"""
    col = {k: i for i, k in enumerate(S.COLUMNS)}
    out, at = [], 0
    for row in rows:
        row = list(row)
        if row[0] == level:
            p = conv[at // len(conv[0])][at % len(conv[0])]
            at += 1
            assert int(row[col["sequences"]]) == p["sequences"] and int(row[col["obs_r"]]) == p["x"] and int(row[col["exp_r"]]) == p["exp_r"]
            row[col["sigma"]], row[col["p_positive"]] = "%.4f" % float(p["sigma"]), "%.4f" % float(p["p_positive"])
            row[col["sigma_lower"]], row[col["sigma_upper"]] = "%.2f" % p["lower"], "%.2f" % p["upper"]
        out.append(row)
    assert at == sum(len(r) for r in conv) or level != "lineage"
    return out


def _same_test_table(path, want):
    head, got = _table(path)
    assert head == CM.TEST_COLUMNS and len(got) == len(want), (head, len(got), len(want))
    for a, b in zip(got, want):
        assert a[:4] == b[:4], (a, b)
        for x, y in zip(a[4:], b[4:]):
            if y == "":
                assert x == "", (a, b)
            else:
                assert re.fullmatch(r"-?\d+\.\d{4}", x) and abs(float(x) - float(y)) <= 1.0000001e-4, (a, b)


def _combine_line(r):
    return [l for l in r.stderr.splitlines() if l.startswith("selection combine: ")]


def _same_combine_line(r, want):
    got = _combine_line(r)
    lines = r.stderr.splitlines()
    assert len(got) == 1 and lines[lines.index(got[0]) - 1].startswith("selection: "), r.stderr[-600:]      # it follows the selection: line
    num = re.compile(r"(?<=sample sigma )(-?\d+\.\d{4})( -?\d+\.\d{4})?")
    assert num.sub("#", got[0]) == num.sub("#", want), (got[0], want)
    a, b = [float(x) for x in num.search(got[0]).group(0).split()], [float(x) for x in num.search(want).group(0).split()]
    assert len(a) == len(b) and all(abs(x - y) <= 1.0000001e-4 for x, y in zip(a, b)), (got[0], want)


def test_vdjer_cli_selection_combine_families(tmp_path):
    ids, seqs, recs, planted = planted_families()
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F._write_fasta(str(tmp_path / "ref" / "ig_vdj.fa"), recs)
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    names, classes, germs, _, _ = parsed_records(recs)
    rlines, cdr = v_regions(names, classes, germs)
    tlines, w = targeting()
    (tmp_path / "r.tsv").write_text("\n".join(rlines) + "\n")
    (tmp_path / "t.tsv").write_text("\n".join(tlines) + "\n")
    env = _child_env("shipped")
    x = _run_child("_families_hits", "x", env)
    v = {k: np.asarray(a) for k, a in x["v"].items()}
    clone = np.asarray(x["clone"])
    G = int(clone.max()) + 1
    lim = M.mutation_limit(ids, seqs)

    # 1. everything: regions, a targeting model, lineages, the consensus rows, the test table -- beside other tables, whose bytes stay
    tables = ["--airr", "a.tsv", "--lineages", "l.tsv", "--mutations", "m.tsv", "--consensus", "c.tsv"]
    sel = ["--selection", "s.tsv", "--v-regions", "../r.tsv", "--targeting", "../t.tsv"]
    mean, rm = _run_families(tmp_path, "mean", tables + sel + ["--selection-combine", "mean", "--selection-test", "st.tsv"], env)
    shared, rs = _run_families(tmp_path, "shared", tables + sel + ["--selection-combine", "shared", "--selection-test", "st.tsv"], env)
    absent, ra = _run_families(tmp_path, "absent", tables + sel, env)
    cnt = S.counts(seqs, v, lim, germs, cdr, w)
    rows, st = S.table_rows(ids, cnt, 2, clone, G, "reads")
    conv = CM.rows(cnt, 2, clone, G)
    cc = _consensus_counts(env)
    ccnt = {f: np.array(a, dtype=object) for f, a in cc.items()}
    U = len(ccnt["obs_r"])
    cconv = CM.rows(ccnt, 2, None, 0)
    cshared = S.rows(dict(ccnt, flags=np.ones(U, np.int64)), 2, None, 0)[-1]
    head, got = _table(mean / "s.tsv")
    _, base = _table(absent / "s.tsv")
    assert head == S.COLUMNS and len(got) == len(base) == len(rows) + sum(1 for r in base if r[0].startswith("consensus"))
    want = _with_mean(_with_mean(rows, "lineage", conv[:G]), "sample", conv[G:])
    (tmp_path / "head.tsv").write_text("\t".join(head) + "\n" + "".join("\t".join(r) + "\n" for r in got[:len(rows)]))
    _same_table(tmp_path / "head.tsv", want)
    tail_got, tail_base = got[len(rows):], base[len(rows):]
    assert [r for r in tail_got if r[0] == "consensus"] == [r for r in tail_base if r[0] == "consensus"] and U >= 1
    (tmp_path / "tail.tsv").write_text("\t".join(head) + "\n" + "".join("\t".join(r) + "\n" for r in tail_got[-2:]))
    _same_table(tmp_path / "tail.tsv", _with_mean(tail_base[-2:], "consensus_sample", cconv))
    assert any(a != b for a, b in zip(got, base)) and [r[:8] for r in got] == [r[:8] for r in base]
    # the selection: line stays, one line follows it
    inf, cinf = CM.info(conv, G, 2), CM.info(cconv, 0, 2)
    tot = dict(rows=inf["rows"] + cinf["rows"], leaves=inf["leaves"] + cinf["leaves"], combines=inf["combines"] + cinf["combines"],
               levels=max(inf["levels"], cinf["levels"]))
    _same_combine_line(rm, CM.summary_line(tot, 2, conv[-1]))
    sel_line = lambda r: [l for l in r.stderr.splitlines() if l.startswith("selection: ")]
    assert sel_line(rm) == sel_line(ra) and len(sel_line(ra)) == 1 and tot["combines"] > 0 and tot["levels"] >= 2
    # the test table: cdr against fwr per lineage, sample and consensus sample, in the chosen mode's densities
    labels = [("lineage", f"lin_{g + 1}") for g in range(G)] + [("sample", "reads"), ("consensus_sample", "reads")]
    _same_test_table(mean / "st.tsv", CM.test_rows(labels, conv + cconv))
    _same_test_table(shared / "st.tsv", CM.test_rows(labels, st[len(ids):] + [cshared]))
    _, tt = _table(mean / "st.tsv")
    print(f"--selection-test: {sum(r[4] != '' for r in tt)} of {len(tt)} rows compared, sample row {tt[-2]}")
    # shared given explicitly, and the flags absent: the same bytes; every other table keeps its bytes under mean
    assert (shared / "s.tsv").read_bytes() == (absent / "s.tsv").read_bytes() and not (absent / "st.tsv").exists()
    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES"))]
    assert keep(rs.stderr.splitlines()) == keep(ra.stderr.splitlines()) and _combine_line(ra) == [] and _combine_line(rs) == []
    assert [l for l in keep(rm.stderr.splitlines()) if not l.startswith("selection combine: ")] == keep(ra.stderr.splitlines())
    for fn in ("a.tsv", "l.tsv", "m.tsv", "c.tsv", "out.sam", "vdjer.dot", "vdj_contigs.fa"):
        assert (mean / fn).read_bytes() == (absent / fn).read_bytes() == (shared / fn).read_bytes(), fn

    # 2. alone: one region, no lineages, no consensus -- the sample row is the only one that changes
    one, r1 = _run_families(tmp_path, "one", ["--selection", "s.tsv", "--selection-combine", "mean"], env)
    cnt1 = S.counts(seqs, v, lim, germs, None, None)
    rows1, _ = S.table_rows(ids, cnt1, 1, None, 0, "reads")
    conv1 = CM.rows(cnt1, 1, None, 0)
    _same_table(one / "s.tsv", _with_mean(rows1, "sample", conv1))
    _same_combine_line(r1, CM.summary_line(CM.info(conv1, 0, 1), 1, conv1[-1]))
    # regions and lineages without a consensus
    reg, r3 = _run_families(tmp_path, "reg", ["--lineages", "l.tsv", "--selection-test", "st.tsv", "--selection-combine", "mean"] + sel[:4], env)
    cnt3 = S.counts(seqs, v, lim, germs, cdr, None)
    rows3, _ = S.table_rows(ids, cnt3, 2, clone, G, "reads")
    conv3 = CM.rows(cnt3, 2, clone, G)
    _same_table(reg / "s.tsv", _with_mean(_with_mean(rows3, "lineage", conv3[:G]), "sample", conv3[G:]))
    _same_test_table(reg / "st.tsv", CM.test_rows(labels[:-1], conv3))

    # 3. two ranks (on one device): rank 0 writes the same bytes
    two, r2 = _run_families(tmp_path, "two", ["--gpus", "2"] + tables + sel + ["--selection-combine", "mean", "--selection-test", "st.tsv"],
                            _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert any("k-mer table sharded over 2 GPUs" in l for l in r2.stderr.splitlines())
    assert (two / "s.tsv").read_bytes() == (mean / "s.tsv").read_bytes() and (two / "st.tsv").read_bytes() == (mean / "st.tsv").read_bytes()
    assert _combine_line(r2) == _combine_line(rm)
