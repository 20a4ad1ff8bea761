#!/usr/bin/env python3
"""Root scorer (a-7) over the parameters the four dumps of make_golden.py leave out (same rules as make_golden.py: runs only
in the build container, needs oracle/_ref/vdjer_ref = the reference's own sources compiled by oracle/Makefile).

  score_<tag>.tsv.gz   what `vdjer_ref score <v_region.fa> <k> <vk> <thr> <queries>` printed: "<k-mer>\t<0|1>" per query
  score_lines.json     the v-region lines every dump was scored against, by name (inputs drawn here from synth, fixed seeds)

Tags are k<k>v<vk>[m|n]_t<thr> (m: three lines, n: one line with N and lower-case characters; t of -1 is written tm1).
Adds its entries to MANIFEST.json under "score", beside the four of make_golden.py: k, vk, thr, lines (the name in
score_lines.json), n_lines, n, ones.

What the cases are for (seq_score.c:36-48, 118-156):
  * k 50 / 41 / 33 against 32 / 25 / 20 / 17: a window of 2k reference characters on both sides of 64;
  * vk 16 / 15 / 12 / 11 / 8 / 4 / 2, among them k = vk + 1 (one seed offset) and vk 2 (every position of the line is a hit);
  * thresholds 1, k/2, k-5, k-1, k and k+1 (k+1: nothing can reach it); 0 and -1 (row and column 0 hold zeros and are tested
    too: any seed hit accepts) with one pair;
  * three lines [long, exactly 2k+1, medium]: ONE position map for all lines, every hit position applied to every line and
    clamped to len - 2k - 1 (hits far along the long line land on the short line's only window, hits near the end of the
    short line are pulled back to its start);
  * N and lower-case characters in the line while the queries are pure ACGT.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from vdjer_amd import synth  # noqa: E402
from make_golden import REF, gz_write, run_ref  # noqa: E402

# (k, vk, kind, thresholds); kind "" one line, "m" three lines, "n" one line with N / lower case
CASES = [
    (50, 15, "", (25, 45, 51)), (50, 16, "", (1, 49, 50)), (50, 2, "", (45, 49)),
    (33, 11, "", (16, 28, 34)), (32, 11, "", (1, 27, 32)),
    (17, 16, "", (1, 16, 17)), (17, 15, "", (1, 16, 18)),
    (20, 8, "", (0, -1, 10, 15)), (25, 4, "", (20, 24)), (41, 12, "", (20, 36, 40, 42)),
    (50, 16, "m", (25, 45)), (33, 11, "m", (16, 28)), (17, 16, "m", (16, 17)), (20, 8, "m", (10, 15, 21)),
    (32, 11, "n", (16, 27)),
]


def rand_seq(rng, n):
    return "".join("ACGT"[int(i)] for i in rng.integers(0, 4, n))


def make_lines(k, vk, kind, rng, vr):
    if kind == "m":                                         # a short line after a long one; the shortest the scorer accepts
        return [vr[:1500], vr[2000:2000 + 2 * k + 1], vr[3000:3400]]
    n = 600 if vk <= 4 else 3000                            # (vk 2 / 4: every position is a hit, the reference runs a DP for each)
    a = int(rng.integers(0, len(vr) - n))
    line = vr[a:a + n]
    if kind == "n":
        s = list(line)
        for p in rng.integers(0, n, 25):
            s[int(p)] = "N"
        for p in rng.integers(0, n - 8, 12):                # lower-case runs
            ln = int(rng.integers(1, 8))
            s[int(p):int(p) + ln] = [c.lower() for c in s[int(p):int(p) + ln]]
        line = "".join(s)
    return [line]


def acgt_only(rng, s):
    return "".join(c if c in "ACGT" else (c.upper() if c.upper() in "ACGT" else "ACGT"[int(rng.integers(0, 4))]) for c in s)


def make_queries(k, vk, kind, lines, rng):
    qs = []
    for li, line in enumerate(lines):
        n_piece = 6 if len(line) < 4 * k else 100
        for _ in range(n_piece):                            # pieces with 0 .. k/4 substitutions
            st = int(rng.integers(0, len(line) - k + 1))
            q = list(line[st:st + k])
            for _m in range(int(rng.integers(0, k // 4 + 1))):
                q[int(rng.integers(0, k))] = "ACGT"[int(rng.integers(0, 4))]
            qs.append("".join(q))
        for _ in range(n_piece // 3):                       # one deletion / one insertion
            st = int(rng.integers(0, len(line) - k))
            g = line[st:st + k + 1]
            cut = int(rng.integers(2, k - 2))
            qs.append(g[:cut] + g[cut + 1:])
            qs.append((g[:cut] + "ACGT"[int(rng.integers(0, 4))] + g[cut:])[:k])
        qs += [line[:k], line[-k:], line[-k - 5:-5]]
    for _ in range(40):
        qs.append(rand_seq(rng, k))
    return [acgt_only(rng, q) for q in qs]


def tag_of(k, vk, kind, thr):
    return f"k{k}v{vk}{kind}_t{thr if thr >= 0 else 'm' + str(-thr)}"


def main():
    assert os.path.exists(REF), "build the reference first: make -C oracle ref"
    work = tempfile.mkdtemp(prefix="vdjx_golden_score_")
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    vr = synth.make_repertoire(2, seed=4242).v_region
    all_lines = {}
    for ci, (k, vk, kind, thrs) in enumerate(CASES):
        rng = np.random.default_rng(9000 + ci)
        name = f"k{k}v{vk}{kind}"
        lines = make_lines(k, vk, kind, rng, vr)
        assert all(len(l) > 2 * k for l in lines)           # (the reference reads out of bounds otherwise)
        all_lines[name] = lines
        queries = make_queries(k, vk, kind, lines, rng)
        assert all(len(q) == k and set(q) <= set("ACGT") for q in queries)
        with open(os.path.join(work, name + ".fa"), "w") as f:
            f.write("".join(f">line{i}\n{l}\n" for i, l in enumerate(lines)))
        with open(os.path.join(work, name + ".txt"), "w") as f:
            f.write("\n".join(queries) + "\n")
        for thr in thrs:
            r = run_ref(["score", name + ".fa", str(k), str(vk), str(thr), name + ".txt"], work, stdout=subprocess.PIPE)
            assert r.returncode == 0, r.stderr[-2000:]
            rows = [l.split("\t") for l in r.stdout.splitlines()]
            assert [x[0] for x in rows] == queries
            ones = sum(x[1] == "1" for x in rows)
            if thr > k:
                assert ones == 0, (name, thr, ones)
            else:
                assert 0 < ones < len(rows), (name, thr, ones)        # every other dump holds both verdicts
            tag = tag_of(k, vk, kind, thr)
            gz_write(f"score_{tag}.tsv.gz", r.stdout)
            man["score"][tag] = {"k": k, "vk": vk, "thr": thr, "lines": name, "n_lines": len(lines), "n": len(rows), "ones": ones}
            print(tag, "n", len(rows), "ones", ones)
    with open(os.path.join(HERE, "score_lines.json"), "w") as f:
        json.dump(all_lines, f, indent=0, sort_keys=True)
        f.write("\n")
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
