"""`vdjer --lineages --lineage-threshold` on the e2e_families golden and on a second seeded repertoire with large buckets
(tests/threshold_repertoire.py).  A run with the flag prints a threshold T: its lineages table is, byte for byte, that of a run with
--lineage-dist T and no flag; the count column of its file, fed to the model (tests/threshold_model.py), gives the density column, the `#`
lines and the stderr line.  A run without the flag gives the table and the lines of the lineage model, as before.  The same under
--lineage-model with a seeded table and under --gpus 2 on one device."""
import os
import re

import numpy as np
import pytest

from tests import families as F
from tests import lineage_dist_cases as LC
from tests import threshold_cases as TC
from tests import threshold_model as M
from tests import threshold_repertoire as R
from tests.test_gpu_annot import _child_env
from tests.test_gpu_lineage_dist_cli import _argv, _lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHY = {M.FEW: "too few values", M.NO_SCALE: "no scale", M.ONE_MODE: "one mode", M.SHALLOW: "shallow valley"}


def _vdjer(d, name, extra, env):
    import subprocess
    run = d / name
    run.mkdir()
    with open(run / "out.sam", "wb") as so:
        r = subprocess.run(_argv(extra), cwd=run, stdout=so, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return run, r.stderr.splitlines()


def _read(path):
    """t.tsv -> (the `#` lines, counts uint64[N], densities as Python integers)"""
    lines = path.read_text().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert lines[:len(head)] == head and lines[len(head)] == "dist\tcount\tdensity" and len(lines) == len(head) + 1 + M.N
    rows = [l.split("\t") for l in lines[len(head) + 1:]]
    assert [r[0] for r in rows] == ["%.4f" % (g / 10000.0) for g in range(M.N)]
    return head, np.array([int(r[1]) for r in rows], np.uint64), [int(r[2]) for r in rows]


def _expected(model, fallback, passes):
    """the `#` lines and the stderr line for a model result; fallback: the numerator of the --lineage-dist the run was given"""
    i = model["info"]
    used = i["threshold"] if i["status"] == M.FOUND else fallback
    head = [f"# status\t{M.STATUS[i['status']]}", f"# values\t{i['values']}", f"# distinct\t{i['distinct']}", "# bandwidth\t%.3f" % (i["k"] / 1000.0),
            "# peak1\t%.4f\t%.4f\t%d" % (i["p1_first"] / 10000.0, i["p1_last"] / 10000.0, i["y1"]),
            "# peak2\t%.4f\t%.4f\t%d" % (i["p2_first"] / 10000.0, i["p2_last"] / 10000.0, i["y2"]),
            "# valley\t%.4f\t%.4f\t%d" % (i["t_first"] / 10000.0, i["t_last"] / 10000.0, i["m"]), "# threshold\t%.4f" % (used / 10000.0), f"# scale\t{M.FIX}"]
    if i["status"] == M.FOUND:
        line = ("lineage threshold: %d distances in %d bins, bandwidth %.3f, peaks %.4f %.4f, valley %.4f .. %.4f, threshold %.4f, %d pair passes"
                % (i["values"], i["distinct"], i["k"] / 1000.0, i["p1_first"] / 10000.0, i["p2_first"] / 10000.0, i["t_first"] / 10000.0, i["t_last"] / 10000.0,
                   i["threshold"] / 10000.0, passes))
    else:
        line = "lineage threshold: %d distances in %d bins, none (%s), --lineage-dist %.4f stands" % (i["values"], i["distinct"], WHY[i["status"]], fallback / 10000.0)
    return head, line, used


def _check(d, tag, base, env, fallback=1500, base_env=None):
    """the three checks for one set of flags `base`: -> (the model's info, the run's directory)"""
    plain, err0 = _vdjer(d, f"{tag}_plain", base, base_env or env)
    assert _lines(err0, "lineage threshold: ") == [] and not (plain / "t.tsv").exists()
    run, err = _vdjer(d, f"{tag}_thr", base + ["--lineage-threshold", "t.tsv"], env)
    head, counts, dens = _read(run / "t.tsv")
    model = M.threshold(counts)
    passes = 2 if model["info"]["status"] == M.FOUND and model["info"]["threshold"] != fallback else 1
    want_head, want_line, used = _expected(model, fallback, passes)
    print(f"vdjer --lineage-threshold {tag}: {model['info']}")
    assert dens == [int(y) for y in model["density"]] and head == want_head, (head, want_head)
    assert _lines(err, "lineage threshold: ") == [want_line], (_lines(err, "lineage threshold: "), want_line)
    at = [k for k, l in enumerate(err) if l.startswith("lineages: ")]
    assert len(at) == 1 and err[at[0]].endswith(f" lineages at {used}/10000")
    after = err[at[0] + 1:at[0] + 3]
    assert after[0] == want_line or (after[0].startswith("lineage model: ") and after[1] == want_line)       # it follows the lineages: (and lineage model:) line
    # the table is that of --lineage-dist T without the flag; every other line of stderr too
    fixed, errf = _vdjer(d, f"{tag}_dist", [a for a in base if a not in ("--lineage-dist", "0.05")] + ["--lineage-dist", "%.4f" % (used / 10000.0)], base_env or env)
    assert (run / "l.tsv").read_bytes() == (fixed / "l.tsv").read_bytes()
    keep = lambda ls: [l for l in ls if not l.startswith(("ELAPSED_SECS", "VDJX_TIMES", "lineage threshold: ")) and not re.search(r"\d bytes sent by rank", l)]
    assert keep(err) == keep(errf)
    if passes == 2:                                                          # the lineages: line is the second pass', not the first's
        assert keep(err) != keep(err0) and f" lineages at {fallback}/10000" in "\n".join(err0)
    return model["info"], run, plain


@pytest.fixture(scope="module")
def families_dir(tmp_path_factory):
    """the golden's input, written once for the cases below"""
    from vdjer_amd import annot
    d = tmp_path_factory.mktemp("threshold_families")
    fam = F.build()
    F.write_ref_dir(fam, str(d / "ref"))
    F.pool(fam).write_reads_file(str(d / "reads.txt"))
    annot.write_targeting(str(d / "real.tsv"), LC.weights()["realistic"], comments=("seeded",))
    return d


FAMILIES = {"ham": (["--lineages", "l.tsv"], 1500, {}),
            "tight": (["--lineages", "l.tsv", "--lineage-dist", "0.05"], 500, {}),
            "model": (["--lineages", "l.tsv", "--lineage-model", "../real.tsv"], 1500, {}),
            "two": (["--gpus", "2", "--lineages", "l.tsv"], 1500, dict(VDJX_MGPU_ONE_DEVICE="1", VDJX_MGPU_TIMEOUT_S="120"))}
_done = {}


def _families(d, tag):
    """the three checks of a case, made once"""
    if tag not in _done:
        base, fallback, extra = FAMILIES[tag]
        _done[tag] = _check(d, tag, base, _child_env("shipped", **extra), fallback=fallback)
    return _done[tag]


def test_vdjer_cli_lineage_threshold_families(families_dir):
    """Hamming: the designed distances, so what tests/test_threshold_cpu.py found for them"""
    info, run, plain = _families(families_dir, "ham")
    want = TC.model("default", "e2e_families")["info"]
    assert info == want and info["status"] == M.FOUND and info["threshold"] == 996
    assert (run / "l.tsv").read_bytes() != (plain / "l.tsv").read_bytes()    # 0.0996 splits what 0.15 joined


def test_vdjer_cli_lineage_threshold_own_lineage_dist(families_dir):
    """a --lineage-dist of its own is the first pass' threshold and the fallback; the valley does not depend on it"""
    assert _families(families_dir, "tight")[0] == _families(families_dir, "ham")[0]


def test_vdjer_cli_lineage_threshold_under_a_model(families_dir):
    """under a seeded 5-mer table: unit 2000, the same number of distances, a valley of its own"""
    info = _families(families_dir, "model")[0]
    assert info["values"] == _families(families_dir, "ham")[0]["values"] and info["status"] == M.FOUND


def test_vdjer_cli_lineage_threshold_two_ranks(families_dir):
    """two ranks (on one device): rank 0 calls, the same files"""
    info, run, _ = _families(families_dir, "two")
    info1, run1, _ = _families(families_dir, "ham")
    assert info == info1 and (run / "l.tsv").read_bytes() == (run1 / "l.tsv").read_bytes() and (run / "t.tsv").read_bytes() == (run1 / "t.tsv").read_bytes()


def test_vdjer_cli_lineage_threshold_file_that_cannot_be_written(families_dir):
    """handled as --lineages' own: the message, a failed run"""
    import subprocess
    run = families_dir / "unwritable"
    run.mkdir()
    for extra, name in ((["--lineages", "l.tsv", "--lineage-threshold", "none/t.tsv"], "none/t.tsv"), (["--lineages", "none/l.tsv"], "none/l.tsv")):
        r = subprocess.run(_argv(extra), cwd=run, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600, env=_child_env("shipped"))
        assert r.returncode != 0 and f"cannot write {name}" in r.stderr and "lineage threshold: " not in r.stderr, r.stderr[-600:]


def test_vdjer_cli_lineage_threshold_large_buckets(tmp_path):
    """lineages of four and unrelated singles in three buckets: both modes are in the contigs, the valley is found and the pair pass runs twice"""
    env = _child_env("shipped")
    fam = R.build()
    F.write_ref_dir(fam, str(tmp_path / "ref"))
    F.pool(fam).write_reads_file(str(tmp_path / "reads.txt"))
    info, run, _ = _check(tmp_path, "large", ["--lineages", "l.tsv"], env)
    assert info["status"] == M.FOUND and info["threshold"] != 1500           # (so _check saw "2 pair passes" and a table other than the first pass')
    head, counts, _ = _read(run / "t.tsv")
    assert head[0] == "# status\tfound"
    T = info["threshold"]
    assert int(counts[:T].sum()) >= 24 and int(counts[T + 1:].sum()) >= 12                # both modes
    near, length = R.designed_distances(fam)
    print("designed:", M.threshold(M.bins(near, length, 1))["info"])
    rows = [l.split("\t") for l in (run / "l.tsv").read_text().splitlines()[1:]]
    sizes = sorted(int(r[6]) for r in rows if r[1])
    assert sizes.count(4) >= 4 * 8 and sizes.count(1) >= 12                               # lineages of four, singles beside them
