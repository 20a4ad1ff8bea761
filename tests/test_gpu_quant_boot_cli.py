"""`vdjer --quant --lineages --quant-boot 20 --quant-seed 7` on the e2e_families golden: the four bootstrap columns of the quant table against
Context.quant_boot's summary, clone_count_sd of the lineages table against its definition computed from the replicates, the `quant boot:`
line against the API's figures; and a run without the two flags, whose tables are the first run's with the added columns cut.

The `quant:` line of this golden, recorded from a run on the MI355X: see test_vdjer_cli_quant_boot_families."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import families as F
from tests import quant_model as Q
from tests.test_gpu_annot import _child_env
from tests.test_gpu_quant import _context, _golden_contigs
from tests.test_gpu_tables import _vdjer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, SEED = 20, 7
LINE = re.compile(r"quant boot: (\d+) replicates \(seed (\d+)\), (\d+) EM iterations in all \(most (\d+)\), (\d+) stopped at the iteration limit, (\d+) batches")
QLINE = re.compile(r"quant: (\d+) pairs placed \((\d+) once\), (\d+) alignments, (\d+) EM iterations, ")


def _api(_):
    fam = F.build()
    ctx, p = _context(F.pool(fam))
    _, seqs = _golden_contigs(F.TAG)
    res = ctx.quant_boot(seqs, replicates=B, seed=SEED)
    p.free()
    ctx.close()
    return dict(boot=res["boot"].tobytes().hex(), counts=res["counts"].tolist(), info=res["info"], boot_info=res["boot_info"],
                **{k: res[k].tolist() for k in ("mean", "sd", "lower", "upper")})


def test_vdjer_cli_quant_boot_families(tmp_path):
    """The golden's `quant:` line: 51615 pairs placed (51615 once), 51615 alignments -- alignments / pairs = 1: this golden places every
    pair once, on the MI355X as in its SAM.  Every r is then 1.0, a replicate's count is the sum of its pairs' multiplicities and the
    sister contigs trade nothing; the test holds all the same (the replicates differ by their draws, boot_sd and clone_count_sd are
    positive), and the trading of pairs is what tests/test_gpu_quant_boot.py's handmade cases cover."""
    from vdjer_amd import annot
    fam = F.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    env = _child_env("shipped")
    tables = ["--quant", "q.tsv", "--lineages", "l.tsv"]
    d, lines = _vdjer(tmp_path, "boot", tables + ["--quant-boot", str(B), "--quant-seed", str(SEED)], env)
    plain_d, plain_lines = _vdjer(tmp_path, "plain", tables, env)
    code = "import json; from tests.test_gpu_quant_boot_cli import _api; print('QBOOT', json.dumps(_api(0)))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    api = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("QBOOT ")).split(" ", 1)[1])

    # the quant table: RSEM's columns, then the summary of the replicates
    head, rows = Q.read_table(d / "q.tsv")
    n = len(rows)
    assert head == Q.HEADER + ["boot_mean", "boot_sd", "boot_lower", "boot_upper"] and n == len(api["counts"]) > 0
    assert [r_[4] for r_ in rows] == ["%.2f" % x for x in api["counts"]]
    for k, col in enumerate(("mean", "sd", "lower", "upper")):
        assert [r_[8 + k] for r_ in rows] == ["%.2f" % x for x in api[col]], col
    boot = np.frombuffer(bytes.fromhex(api["boot"]), np.float64).reshape(B, n)
    assert any(float(r_[9]) > 0 for r_ in rows)                          # the replicates differ

    # the lineages table: the sd over the replicates of the members' summed replicate counts (unrounded, in contig order)
    lhead, lrows = Q.read_table(d / "l.tsv")
    assert lhead[-2:] == ["clone_expected_count", "clone_count_sd"] and [r_[0] for r_ in lrows] == [r_[0] for r_ in rows]
    clone = [int(r_[1][4:]) - 1 if r_[1] else -1 for r_ in lrows]
    nk = max(clone) + 1
    assert nk > 1
    sums = np.zeros((B, nk))
    for rep in range(B):
        for c, k in enumerate(clone):
            if k >= 0:
                sums[rep, k] += boot[rep, c]
    sd = annot.quant_boot_summary(sums)["sd"]
    for r_, k in zip(lrows, clone):
        assert len(r_) == len(lhead)
        assert r_[-1] == ("%.2f" % sd[k] if k >= 0 else "") and (k >= 0 or r_[-2] == "")
    # (what the column is for: the members of a lineage trade pairs, the lineage keeps them -- the lineage's sd is below the sum of
    # its members' wherever it has more than one)
    msd = np.array(api["sd"])
    multi = [k for k in range(nk) if clone.count(k) > 1]
    assert multi and all(sd[k] <= sum(msd[c] for c in range(n) if clone[c] == k) + 1e-9 for k in multi)

    # stderr: the line follows the quant line and carries the API's figures
    at = next(i for i, l in enumerate(lines) if l.startswith("quant: "))
    m = LINE.fullmatch(lines[at + 1])
    assert m, lines[at:at + 2]
    bi = api["boot_info"]
    assert [int(x) for x in m.groups()] == [B, SEED, bi["iterations"], bi["max_iterations"], B - bi["converged"], bi["batches"]]
    q = QLINE.match(lines[at])
    print(lines[at])
    assert q and int(q.group(3)) >= int(q.group(1)) == api["info"]["pairs"]

    # without the flags: no line, and the same tables with the added columns cut
    assert not any(l.startswith("quant boot: ") for l in plain_lines)
    cut_q = "".join("\t".join(l.split("\t")[:8]) + "\n" for l in (d / "q.tsv").read_text().split("\n")[:-1])
    cut_l = "".join("\t".join(l.split("\t")[:-1]) + "\n" for l in (d / "l.tsv").read_text().split("\n")[:-1])
    assert (plain_d / "q.tsv").read_text() == cut_q
    assert (plain_d / "l.tsv").read_text() == cut_l
