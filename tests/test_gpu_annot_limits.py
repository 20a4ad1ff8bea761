"""vdjx_annotate at the limits only production-sized inputs reach (tests/annot_limit_cases.py; tests/test_annot_cpu.py asserts that each
case meets its condition): a 4,095-base query traced against a 2,047-base record, S at the 16-bit ceiling 15 * 2047, chunks that end
because of their 65,536 columns with ties on both sides of the cut, and hits whose direction bytes take two traceback launches.  Every
field of every hit equals the model's (tests/annot_model.py, annotate(fast=True)) bit for bit, a second call returns the same bytes, and
the counters annot_chunks / annot_score_launches / annot_trace_launches show that the limit was reached.  The device runs in a child
process per test, as in tests/test_gpu_annot.py.

Wall time of each test on one MI355X (the CPU model included, which is most of it; device time from annot_score_us + annot_trace_us):
  test_long_query_long_record       14.1 s   (device: 78 ms and 70 ms for the two parameter sets, 62 ms of each the six tracebacks)
  test_score_at_the_16_bit_ceiling   3.9 s   (device: 37 ms)
  test_chunks_cut_by_columns         8.3 s   (device: 17 ms per record set, five runs)
  test_api_checks_mid_pairs          8.1 s   (test_gpu_annot's _api_checks, whose model is plain Python)
  test_traceback_in_two_launches     7.0 s   (device: 16 ms scoring, 122 ms for the 68 tracebacks in two launches)
The rest is the model: scores() over 4,095 x 2,047 cells per pair and a trace_fast per hit, once per distinct contig."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import annot_limit_cases as L
from tests import annot_model as A
from tests import test_gpu_annot as T
from tests.test_gpu_annot import _child_env, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ["annot_cells", "annot_chunks", "annot_score_launches", "annot_trace_launches", "annot_score_us", "annot_trace_us"]


def _run_child(fn, arg, env, timeout=600):
    code = f"import json; from tests.test_gpu_annot_limits import {fn}; print('ANNOT', json.dumps({fn}({arg!r})))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("ANNOT ")).split(" ", 1)[1])


def _device(names):
    """in the child: every named case under each of its parameter sets, twice (the same bytes) -> {name: [{"v", "j", stats}, ...]}"""
    from vdjer_amd import api
    ctx = api.Context(0)
    out = {}
    for name in names.split(","):
        c = L.CASES[name]()
        info = ctx.germline_load(c["recs"])
        assert not info["skipped"], info["skipped"]
        out[name] = []
        for prm in c["params"]:
            dev = ctx.annotate(c["contigs"], **prm)
            res = {cls: {f: np.asarray(dev[cls][f]).tolist() for f in A.FIELDS} for cls in ("v", "j")}
            res.update({s: ctx.stat(s) for s in STATS})
            again = ctx.annotate(c["contigs"], **prm)
            for cls in ("v", "j"):
                for f in A.FIELDS:
                    assert np.asarray(again[cls][f]).tobytes() == np.asarray(dev[cls][f]).tobytes(), (name, cls, f)
            assert [ctx.stat(s) for s in STATS[:4]] == [res[s] for s in STATS[:4]]
            out[name].append(res)
    ctx.close()
    return out


def _cells(c):
    return len(c["contigs"]) * c["m"] * sum(len(g) for g in c["germs"])


def _us(res):
    return {k: res[k] for k in ("annot_score_us", "annot_trace_us")}


def test_long_query_long_record():
    """4,095 x 2,047: 8.4 M direction bytes per alignment, 6,142 anti-diagonals of up to 32 cells per lane, under the default costs and
    with gap_open = 0"""
    c = L.long_pair()
    dev = _run_child("_device", "long_pair", _child_env("shipped"))["long_pair"]
    for k in range(len(c["params"])):
        print("long_pair", k, _us(dev[k]))
        _same(dev[k], L.model("long_pair", k), ("long_pair", k))
        assert dev[k]["annot_cells"] == _cells(c) and dev[k]["annot_trace_launches"] == 1 and dev[k]["annot_chunks"] == 2
        assert min(np.subtract(dev[k]["v"]["germ_end"], dev[k]["v"]["germ_start"])) >= 1400


def test_score_at_the_16_bit_ceiling():
    """S = 15 * 2047 = 30,705 in the scoring ring's and the traceback's 16-bit H, and three scores just below it"""
    dev = _run_child("_device", "ceiling", _child_env("shipped"))["ceiling"][0]
    print("ceiling", _us(dev))
    _same(dev, L.model("ceiling"), "ceiling")
    v = dev["v"]
    assert v["score"][0] == 30705 and v["matches"][0] == 2047 and v["n_runs"][0] == 1 and v["runs"][0][0] == (2047 << 4)
    assert len(set(v["score"])) == 4 and all(30505 <= s < 30705 for s in v["score"][1:]), v["score"]


SETS = ["column_chunks_A", "column_chunks_B", "column_chunks_A_long", "column_chunks_B_long"]


def _check_ties(dev, name):
    v = dev["v"]
    short = name.endswith("_long")
    assert v["n_tied"][0] == (8 if short else 11) and v["tied"][0] == L.TIED_IN[:8], (name, v["n_tied"], v["tied"][0])
    assert v["n_tied"][4] == v["n_tied"][0] and v["tied"][4] == L.TIED_IN[:8]
    assert v["n_tied"][1] == (1 if short else 2) and v["tied"][1][:2] == (L.TWICE_IN[:1] + [-1] if short else L.TWICE_IN), (name, v["tied"][1])


def test_chunks_cut_by_columns():
    """many records per chunk, the chunk ended by its columns: 65,537 columns make one chunk more than 65,536; ties that lie on both
    sides of the cut, more than eight of them over two chunks; and, with VDJX_ANNOT_PAIRS=100, chunks of 25 records at most and a
    scoring launch that ends between two contig groups of one chunk -- the same bytes as under the shipped knobs"""
    dev = _run_child("_device", ",".join(SETS), _child_env("shipped"))
    for name in SETS:
        c = L.CASES[name]()
        d = dev[name][0]
        print(name, _us(d))
        _same(d, L.model(name), name)
        _check_ties(d, name)
        assert d["annot_chunks"] == L.n_chunks(c["germs"], c["classes"]), (name, d["annot_chunks"])
        assert d["annot_cells"] == _cells(c) and d["annot_score_launches"] == 1 and d["annot_trace_launches"] == 1
    # the number of chunks, in figures: the 32 long records alone are 65,537 columns (two V chunks and the J's) or 65,536 (one and the J's)
    assert [dev[name][0]["annot_chunks"] for name in SETS] == [3, 3, 3, 2]
    capped = _run_child("_device", "column_chunks_A", _child_env("suite", VDJX_ANNOT_PAIRS="100"))["column_chunks_A"][0]
    c = L.column_chunks("A")
    _same(capped, L.model("column_chunks_A"), "A, 100 pairs")
    _check_ties(capped, "column_chunks_A")
    for cls in ("v", "j"):
        for f in A.FIELDS:
            assert capped[cls][f] == dev["column_chunks_A"][0][cls][f], (cls, f)
    assert capped["annot_chunks"] == L.n_chunks(c["germs"], c["classes"], recs=25) == 3
    assert capped["annot_score_launches"] == L.score_launches(len(c["contigs"]), c["germs"], c["classes"], 100) >= 4


def test_api_checks_mid_pairs():
    """test_gpu_annot's API checks with VDJX_ANNOT_PAIRS=40: chunks of up to 10 records, launches of several workgroups"""
    res = T._run_child("_api_checks", "x", _child_env("suite", VDJX_ANNOT_PAIRS="40"))
    assert res["seed1"]["v"] > 0 and res["seed1"]["j"] > 0


def test_traceback_in_two_launches():
    """68 alignments, 34 of them 4,095 x 2,047: the direction bytes of the first 32 fill a launch, the others reuse the buffer from 0"""
    c = L.trace_launches()
    dev = _run_child("_device", "trace_launches", _child_env("shipped"))["trace_launches"][0]
    print("trace_launches", _us(dev))
    model = L.model("trace_launches")
    sizes = L.trace_launch_sizes(model, c["m"], c["germs"])
    assert dev["annot_trace_launches"] == len(sizes) >= 2 and sizes[0] == 32, (dev["annot_trace_launches"], sizes)
    _same(dev, model, "trace_launches")
    assert sum(g >= 0 for cls in ("v", "j") for g in dev[cls]["gene"]) == 68 and dev["annot_cells"] == _cells(c)
