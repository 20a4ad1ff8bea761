"""Query k-mers for the root scorer tests (the recipe of the "score" goldens, tests/golden/make_golden.py): pieces of the v-region
lines with 0 .. k/4 substitutions, pieces with one deletion or insertion, the first and last k characters of every line, random
strings.  Pure ACGT whatever the lines hold (N and lower case in a line are replaced / folded)."""
import numpy as np


def _acgt(rng, s):
    return "".join(c if c in "ACGT" else (c.upper() if c.upper() in "ACGT" else "ACGT"[int(rng.integers(0, 4))]) for c in s)


def random_kmers(rng, n, k):
    return ["".join("ACGT"[int(i)] for i in rng.integers(0, 4, k)) for _ in range(n)]


def pieces(rng, lines, k, n, max_subs):
    """n pieces of k characters from random places of random lines, each with 0 .. max_subs substitutions"""
    out = []
    for _ in range(n):
        line = lines[int(rng.integers(0, len(lines)))]
        st = int(rng.integers(0, len(line) - k + 1))
        q = list(line[st:st + k])
        for _m in range(int(rng.integers(0, max_subs + 1))):
            q[int(rng.integers(0, k))] = "ACGT"[int(rng.integers(0, 4))]
        out.append(_acgt(rng, "".join(q)))
    return out


def queries(rng, lines, k, n):
    """about n queries of k characters over `lines` (every line longer than k)"""
    qs = pieces(rng, lines, k, n // 2, k // 4)
    for _ in range(n // 8):                                 # one deletion, one insertion
        line = lines[int(rng.integers(0, len(lines)))]
        st = int(rng.integers(0, len(line) - k))
        g = line[st:st + k + 1]
        cut = int(rng.integers(1, k))
        qs.append(g[:cut] + g[cut + 1:])
        qs.append((g[:cut] + "ACGT"[int(rng.integers(0, 4))] + g[cut:])[:k])
    for line in lines:
        qs += [line[:k], line[-k:]]
    qs += random_kmers(rng, max(4, n // 4), k)
    qs = [_acgt(rng, q) for q in qs]
    assert all(len(q) == k for q in qs)
    return qs
