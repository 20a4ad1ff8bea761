"""`vdjer`'s option table (vdjer_amd/csrc/host/vdjer_cli.c) against the hand-written parse() it replaced: the command lines of
tests/cli_corpus.py, each compared with what the binary of the commit before the table answered (tests/golden/cli_refusals.json, recorded
by tests/golden/make_golden_cli.py from that commit's binary and never from this tree's).  No case reaches the GPU.

The rule.  `--help` and every command line with one refusal line: stderr byte for byte.  A command line with several: the usage text byte
for byte behind them, and the refusal lines as the same multiset -- the table reads all values, then walks all requirements, then makes
the checks that are no table rows, where the earlier code went flag group by flag group; within each of the three the order is the earlier
one's.  Which cases that reorders is asserted below, so that a change of the order does not pass unseen."""
import collections
import functools
import json
import os

import pytest

from tests import cli_corpus as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vdjer_amd", "vdjer")
# the several-fault cases whose lines come in another order than before the table: those that mix refused values, requirements and the
# other checks.  A case with lines of one of the three only keeps its order (several_needs_only, nothing, help_as_a_value, ...)
REORDERED = {"several_values_and_needs", "several_across_the_groups", "several_with_the_readers"}


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "cli_refusals.json")))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    assert os.path.exists(EXE), "build it: make -C vdjer_amd/csrc/host"
    d = tmp_path_factory.mktemp("cli")
    C.write_inputs(str(d))
    return d


def test_the_corpus_is_the_recorded_one():
    rec = golden()["cases"]
    assert [c[0] for c in C.cases()] == list(rec)
    for name, argv, env in C.cases():
        assert rec[name]["argv"] == argv and rec[name]["env"] == env, name
    # what the corpus must hold: every requirements row alone, every bound from both sides, a non-number, a wrong word, ...
    names = list(rec)
    assert sum(n.startswith("needs_") and "_without_" in n for n in names) == len(C.REQUIRES) == 32
    assert sum(n.startswith("range_") for n in names) == 9 * len(C.RANGES) and sum(n.startswith("seed_") for n in names) == 7 * len(C.SEEDS)
    assert sum(n.startswith("word_") and "_refuses_both" in n for n in names) == len(C.WORDS) == 4
    assert sum(len(r["stderr"].splitlines()) > 1 and r["usage"] for r in rec.values()) >= 3
    assert golden()["usage"].count("\n\t--") == 62 and "\t--jext <" in golden()["usage"] and "--vf" not in golden()["usage"]


@pytest.mark.parametrize("name", [c[0] for c in C.cases()])
def test_answers_as_before_the_table(inputs, name):
    want = golden()["cases"][name]
    status, err, out = C.run(EXE, str(inputs), want["argv"], want["env"])
    usage = golden()["usage"]
    assert "ELAPSED_SECS" not in err and out == ""
    assert status == want["status"]
    assert err.endswith(usage) == want["usage"]
    head = err[:len(err) - len(usage)] if want["usage"] else err
    if len(want["stderr"].splitlines()) <= 1:
        assert head == want["stderr"]
    else:
        assert collections.Counter(head.splitlines(True)) == collections.Counter(want["stderr"].splitlines(True))
        assert (head != want["stderr"]) == (name in REORDERED), head
    assert sorted(p.name for p in inputs.iterdir()) == ["bad_regions.tsv", "c.fa", "model.tsv", "reads.txt", "ref", "regions.tsv", "short.tsv"]
