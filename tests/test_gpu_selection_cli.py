"""`vdjer --selection` on the e2e_families golden (with the planted V records of tests/test_mutation_cpu.py, so that some contigs are
mutated) against the table and the stderr line of tests/selection_model.py: alone, with --lineages, --v-regions and --targeting, under
--gpus 2, and beside every other table, whose bytes it must not change."""
import os
import re

import numpy as np
import pytest

from tests import families as F
from tests import mutation_model as M
from tests import selection_model as S
from tests.test_gpu_annot import _child_env
from tests.test_gpu_mutation import _families_hits, _run_child, _run_families, _table  # noqa: F401  (_families_hits runs in the child)
from tests.test_mutation_cpu import parsed_records, planted_families

pytestmark = pytest.mark.gpu
FLOATS = {"sigma": 1e-4, "sigma_lower": 1e-2, "sigma_upper": 1e-2, "p_positive": 1e-4}


def v_regions(names, classes, germs):
    """a fixed rule over the V records, by name: CDR1 24 bases from a quarter of the record on, CDR2 30 bases from its half on; every
    seventh name has no line (no regions), one line names no record -> (lines, int32[records, 4])"""
    cdr = np.full((len(names), 4), -1, np.int32)
    lines, seen = ["# name cdr1_start cdr1_end cdr2_start cdr2_end", ""], []
    for r, (nm, cl) in enumerate(zip(names, classes)):
        if cl != "V":
            continue
        if nm not in seen:
            seen.append(nm)
            if len(seen) % 7:
                L = len(germs[r])
                lines.append(f"{nm}\t{L // 4}\t{L // 4 + 23} {L // 2}  {L // 2 + 29}")
        if seen.index(nm) % 7 != 6:
            L0 = len(germs[names.index(nm)])
            cdr[r] = (L0 // 4, L0 // 4 + 23, L0 // 2, L0 // 2 + 29)
    lines.append("IGHV99-99*09 1 2 0 0")
    return lines, cdr


def targeting():
    rng = np.random.default_rng(606)
    w = rng.integers(0, 10 ** 7, (1024, 4)).astype(np.uint32)
    lines = ["".join("ACGT"[idx >> s & 3] for s in (8, 6, 4, 2, 0)) + "\t" + "\t".join(str(int(x)) for x in w[idx]) for idx in range(1024)]
    return [l for l in lines], w


def _same_table(path, want):
    head, got = _table(path)
    assert head == S.COLUMNS and len(got) == len(want), (len(got), len(want))
    col = {k: i for i, k in enumerate(head)}
    for a, b in zip(got, want):
        for k, i in col.items():
            if k in FLOATS and b[i] != "":
                assert a[i] != "" and abs(float(a[i]) - float(b[i])) <= FLOATS[k] * 1.0000001 and re.fullmatch(r"-?\d+\.\d{%d}" % (2 if "_" in k and k != "p_positive" else 4), a[i]), (a, b, k)
            else:
                assert a[i] == b[i], (a, b, k)


def _line(r):
    return [l for l in r.stderr.splitlines() if l.startswith("selection: ")]


def _same_line(r, want):
    got = _line(r)
    assert len(got) == 1 and r.stderr.splitlines()[-1] == got[0]
    num = re.compile(r"(?<=sample sigma )(-?\d+\.\d{4})( -?\d+\.\d{4})?")
    assert num.sub("#", got[0]) == num.sub("#", want), (got[0], want)
    a, b = [float(x) for x in num.search(got[0]).group(0).split()], [float(x) for x in num.search(want).group(0).split()]
    assert len(a) == len(b) and all(abs(x - y) <= 1.0000001e-4 for x, y in zip(a, b)), (got[0], want)


def test_vdjer_cli_selection_families(tmp_path):
    ids, seqs, recs, planted = planted_families()
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F._write_fasta(str(tmp_path / "ref" / "ig_vdj.fa"), recs)
    F.write_cfa(fam, str(tmp_path / "c.fa"))
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
    n = len(ids)

    def model(mapped, weighted, grouped, targeting_name="uniform", chunks=0):
        cnt = S.counts(seqs, v, lim, germs, cdr if mapped else None, w if weighted else None)
        K = 2 if mapped else 1
        rows, st = S.table_rows(ids, cnt, K, clone if grouped else None, G if grouped else 0, "reads")
        return cnt, rows, S.summary_line(S.info(cnt, G if grouped else 0, K), st, targeting_name, chunks)

    # 1. alone: the annotation runs by itself; one region, the uniform model, no lineages
    run, r = _run_families(tmp_path, "alone", ["--selection", "s.tsv"], env)
    cnt, rows, line = model(False, False, False)
    _same_table(run / "s.tsv", rows)
    _same_line(r, line)
    assert len(rows) == n + 1 and rows[-1][:3] == ["sample", "reads", "v"] and not (run / "a.tsv").exists()
    assert sum(int(cnt["obs_r"][c].sum()) for c in planted) >= 7 and int(rows[-1][4]) >= 7          # the planted replacements are seen
    # 2. everything: regions, a targeting model, the lineages as groups, beside every other table -- whose bytes stay
    tables = ["--quant", "q.tsv", "--airr", "a.tsv", "--d-calls", "--isotypes", "i.tsv", "--clones", "c.tsv", "--cfa", "../c.fa", "--lineages", "l.tsv",
              "--trees", "t.tsv", "--tree-support", "8", "--mutations", "m.tsv", "--diversity", "dv.tsv", "--diversity-boot", "8"]
    sel = ["--selection", "s.tsv", "--v-regions", "../r.tsv", "--targeting", "../t.tsv"]
    full, rf = _run_families(tmp_path, "full", tables + sel, env)
    plain, rp = _run_families(tmp_path, "plain", tables, env)
    cnt, rows, line = model(True, True, True, "../t.tsv")
    _same_table(full / "s.tsv", rows)
    _same_line(rf, line)
    assert "--v-regions: 1 names match no germline record (the first: IGHV99-99*09)" in rf.stderr
    used = (np.asarray(cnt["flags"]) & S.F_V) > 0
    assert 0 < int(((np.asarray(cnt["flags"]) & S.F_NOREG) > 0).sum()) < n and len(rows) == 2 * int(used.sum()) + int((~used).sum()) + 2 * G + 2
    assert [row[2] for row in rows[-2:]] == ["fwr", "cdr"] and G > 3 and any(row[0] == "lineage" and int(row[3]) >= 1 for row in rows) and int(rows[-2][3]) >= 7
    for fn in ("q.tsv", "a.tsv", "i.tsv", "c.tsv", "l.tsv", "t.tsv", "m.tsv", "dv.tsv", "out.sam", "vdjer.dot", "vdj_contigs.fa"):
        assert (full / fn).read_bytes() == (plain / fn).read_bytes(), fn
    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES", "selection: ", "--v-regions: "))]
    assert keep(rf.stderr.splitlines()) == keep(rp.stderr.splitlines()) and _line(rp) == [] and not (plain / "s.tsv").exists()
    # 3. regions without lineages and a targeting model without regions: the other two shapes of the table
    run, r = _run_families(tmp_path, "regions", sel[:4] + ["--airr", "a.tsv"], env)
    cnt, rows, line = model(True, False, False)
    _same_table(run / "s.tsv", rows)
    _same_line(r, line)
    run, r = _run_families(tmp_path, "weights", sel[:2] + sel[4:] + ["--lineages", "l.tsv"], env)
    cnt, rows, line = model(False, True, True, "../t.tsv")
    _same_table(run / "s.tsv", rows)
    _same_line(r, line)
    # 4. two ranks (on one device): rank 0 writes the same bytes
    two, r2 = _run_families(tmp_path, "two", ["--gpus", "2", "--airr", "a.tsv", "--lineages", "l.tsv"] + sel,
                            _child_env("shipped", VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))
    assert any("k-mer table sharded over 2 GPUs" in l for l in r2.stderr.splitlines())
    assert (two / "s.tsv").read_bytes() == (full / "s.tsv").read_bytes() and _line(r2) == _line(rf)
    # an unwritable file is reported as for the other tables
    bad = tmp_path / "bad"
    bad.mkdir()
    import subprocess
    argv = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vdjer_amd", "vdjer"), "--in", "../reads.txt", "--chain", "IGH", "--ref-dir", "../ref",
            "--ins", "175", "--t", "1"] + F.FLAGS + ["--selection", "no_such_dir/s.tsv"]
    with open(bad / "out.sam", "wb") as so:
        rb = subprocess.run(argv, cwd=bad, stdout=so, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert rb.returncode != 0 and "cannot write no_such_dir/s.tsv" in rb.stderr
