#!/usr/bin/env python3
"""The cli_refusals golden: what the `vdjer` of the commit BEFORE the option table (b804045) answers to the command lines of
tests/cli_corpus.py -- exit status and stderr of every case, none of which reaches the GPU.

    python tests/golden/make_golden_cli.py /path/to/that/commit's/vdjer_amd/vdjer

The binary is named on the command line because it is never the one of this tree: the fixture is the record of the hand-written parse()
that tests/test_cli_options_cpu.py holds the table to, and regenerating it from the code under test would make that test vacuous.  Extend
it only by building that commit again (git worktree add, make -C vdjer_amd/csrc && make -C vdjer_amd/csrc/host) and recording from there.

Writes tests/golden/cli_refusals.json: the usage text once ("usage": --help's stderr) and per case its argv, environment, exit status, the
stderr lines before the usage text ("stderr") and whether the usage text follows them ("usage"): stderr is exactly the one plus the other.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import cli_corpus as C  # noqa: E402


def main():
    exe = os.path.abspath(sys.argv[1])
    assert os.path.exists(exe) and os.path.realpath(exe) != os.path.realpath(os.path.join(ROOT, "vdjer_amd", "vdjer")), "name the earlier commit's binary"
    with tempfile.TemporaryDirectory(prefix="vdjx_golden_cli_") as wd:
        C.write_inputs(wd)
        status, usage, out = C.run(exe, wd, ["--help"], {})
        assert status == 0 and out == "" and usage.startswith("vdjer \n\t--in ") and usage.endswith(">\n")
        rec = {}
        for name, argv, env in C.cases():
            status, err, out = C.run(exe, wd, argv, env)
            assert "ELAPSED_SECS" not in err and out == "", (name, err[-300:])
            assert status in (0, 255), (name, status)
            with_usage = err.endswith(usage)
            head = err[:len(err) - len(usage)] if with_usage else err
            assert "vdjer \n" not in head, name
            rec[name] = {"argv": argv, "env": env, "status": status, "stderr": head, "usage": with_usage}
        assert sorted(os.listdir(wd)) == sorted(["reads.txt", "ref", "c.fa", "model.tsv", "short.tsv", "regions.tsv", "bad_regions.tsv"]), "a case wrote a file"
    with open(os.path.join(HERE, "cli_refusals.json"), "w") as f:
        f.write('{"usage": %s,\n "cases": {\n' % json.dumps(usage))                   # a case per line
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rec.items()) + "\n }}\n")
    print(len(rec), "cases,", sum(r["usage"] for r in rec.values()), "with the usage text,", sum(r["status"] == 0 for r in rec.values()), "with status 0")


if __name__ == "__main__":
    main()
