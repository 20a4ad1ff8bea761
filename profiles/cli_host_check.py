#!/usr/bin/env python3
"""Runs every command line of tests/cli_corpus.py through the stand-alone parse() of profiles/cli_host_check.c (built there with
-fsanitize=address,undefined; the build line is in that file):  python profiles/cli_host_check.py ./cli_host_check

A sanitizer report ends its case with another exit status than parse()'s 0 / 255 and with its text on stderr; both are looked for.  Where
the recorded `vdjer` (tests/golden/cli_refusals.json) was refused by parse(), the refusal lines must be the recorded ones; where main()
refused it behind parse(), parse() must have returned 0.  Prints the parsed values of the accepted cases."""
import collections
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cli_corpus as C  # noqa: E402


def main():
    exe = os.path.abspath(sys.argv[1])
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "cli_refusals.json")))
    taken = 0
    with tempfile.TemporaryDirectory() as wd:
        C.write_inputs(wd)
        for name, argv, env in C.cases():
            status, err, out = C.run(exe, wd, argv, env)
            want = gold["cases"][name]
            assert "Sanitizer" not in err and "runtime error" not in err and status in (0, 255), (name, status, err[-2000:])
            in_parse = want["usage"] or name == "chain_unknown"            # the recorded run ended inside parse()
            assert status == (want["status"] if in_parse else 0), (name, status)
            if in_parse and want["status"]:
                head = err[:len(err) - len(gold["usage"])] if want["usage"] else err
                assert collections.Counter(head.splitlines()) == collections.Counter(want["stderr"].splitlines()), name
            if not status and out.startswith("parse 0 "):
                taken += 1
                print(name, out.strip())
    print(f"ok: {len(C.cases())} command lines, {taken} accepted by parse(), no sanitizer report")


if __name__ == "__main__":
    main()
