"""The environment variables of the native code go through one reader (vdjer_amd/csrc/vdjx_env.h): nothing else calls getenv on a
VDJX_* / VDJH_* name, every name the reader is asked for is documented in README.md, and the reader parses as it says."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vdjer_amd", "csrc")
READER = os.path.join(CSRC, "vdjx_env.h")


def _sources():
    for d, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".hip", ".c", ".h", ".cpp", ".hpp")):
                p = os.path.join(d, f)
                with open(p, errors="replace") as fh:
                    yield p, fh.read()


def test_only_the_reader_calls_getenv():
    bad = [(os.path.relpath(p, ROOT), m.group(0)) for p, s in _sources() if p != READER
           for m in re.finditer(r'getenv\s*\(\s*"VDJ[XH]_\w*"', s)]
    assert not bad, bad
    # ... and nothing reads the environment by another route (a name in a variable, a helper of its own)
    other = [os.path.relpath(p, ROOT) for p, s in _sources() if p != READER and re.search(r"\b(secure_)?getenv\s*\(|\benviron\b", s)]
    assert not other, other


def test_every_variable_read_is_in_the_readme():
    names = set()
    for p, s in _sources():
        names.update(re.findall(r'vdjx_env_(?:set|num|str)\s*\(\s*"(\w+)"', s))
    assert len(names) > 30 and all(n.startswith(("VDJX_", "VDJH_")) for n in names), sorted(names)
    with open(os.path.join(ROOT, "README.md")) as fh:
        readme = fh.read()
    missing = sorted(n for n in names if not re.search(r"\b%s\b" % n, readme))
    assert not missing, missing


_PROBE = r'''
#include "vdjx_env.h"
int main(int argc, char** argv) {
	(void) argc;
	printf("%d %lld\n", vdjx_env_set("VDJX_PROBE"), vdjx_env_num("VDJX_PROBE", atoll(argv[1]), atoll(argv[2]), atoll(argv[3])));
	return 0;
}
'''


def test_the_reader_parses_as_documented(tmp_path):
    with open(os.path.join(CSRC, "host", "Makefile")) as fh:
        mk = fh.read()
    cc = os.environ.get("CC") or re.search(r"^CC\s*\?=\s*(\S+)", mk, re.M).group(1)           # the host Makefile's compiler and flags
    cflags = re.search(r"^CFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("-fPIC", "").split()
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_PROBE)
    b = subprocess.run([cc] + cflags + ["-Werror", "-I", CSRC, "-o", str(exe), str(src)], stderr=subprocess.PIPE, text=True)
    assert b.returncode == 0, b.stderr

    def probe(value, dflt, lo, hi):
        env = {k_: v for k_, v in os.environ.items() if k_ != "VDJX_PROBE"}
        if value is not None:
            env["VDJX_PROBE"] = value
        r = subprocess.run([str(exe), str(dflt), str(lo), str(hi)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=30)
        assert r.returncode == 0, r.stderr
        present, num = (int(x) for x in r.stdout.split())
        return present, num, r.stderr

    assert probe(None, 4, 0, 4) == (0, 4, "")                        # unset: the default, nothing said
    assert probe("0", 4, 0, 4) == (1, 0, "")                         # 0 is a value like any other
    assert probe("3", 4, 0, 4) == (1, 3, "")
    assert probe("4", 7, 0, 4) == (1, 4, "") and probe("-2", 7, -5, 4) == (1, -2, "")         # the bounds belong to the range
    assert probe("1000000000", 262144, 1, 0xFFFFFFFF) == (1, 1000000000, "")
    for junk in ("", "12x", "-1", "5", " 3", "+3", "3 ", "0x2", "1e2", "99999999999999999999999"):
        present, num, err = probe(junk, 4, 0, 4)
        assert (present, num) == (1, 4), junk                        # set, and not a number of the range: the default ...
        lines = err.splitlines()
        assert len(lines) == 1 and "VDJX_PROBE" in lines[0] and '"%s"' % junk in lines[0] and "[0, 4]" in lines[0], (junk, err)      # ... and one line that says why
