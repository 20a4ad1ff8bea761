"""The inputs that take vdjx_annotate to the limits of its engine (vdjer_amd/csrc/vdjx_align.hip), each with the condition it exists for;
tests/test_annot_cpu.py asserts the conditions from the inputs alone (no GPU), tests/test_gpu_annot_limits.py compares the device with
the model on them.  Seeded; every case and every model is computed once per process.

  long_pair        queries of 4,095 bases against records of 2,047: the traceback's 8.4 M cells, diagonals of 32 cells per lane
  ceiling          S = 15 * 2047 = 30,705, the largest H the engine's 16-bit diagonals have to hold
  column_chunks    a chunk of many records that ends because of its columns (65,537 against 65,536), ties on both sides of the cut
  trace_launches   more direction bytes than one traceback launch takes (33 alignments of 4,095 x 2,047 are the fewest)

chunk_sizes() and trace_launch_sizes() restate the engine's two packing rules, so that a case's condition is computed, not assumed."""
import functools

import numpy as np

from tests import annot_model as A

CHUNK_COLS = 65536               # AN_CHUNK_COLS
DIR_BYTES = 256 << 20            # AN_DIR_BYTES
WAVES = 4                        # AN_WAVES: a chunk holds at most VDJX_ANNOT_PAIRS / 4 records


def chunk_sizes(lens, cols=CHUNK_COLS, recs=None):
    """the records per chunk of one class whose records have `lens` bases, in index order: every record takes its bases and a reset column,
    a chunk one more reset column at its end; a chunk grows while columns(x .. y) + 1 <= cols (and while it has fewer than `recs` records)"""
    out, x = [], 0
    while x < len(lens):
        y = x + 1
        while y < len(lens) and (recs is None or y - x < recs) and sum(l + 1 for l in lens[x:y + 1]) + 1 <= cols:
            y += 1
        out.append(y - x)
        x = y
    return out


def n_chunks(germs, classes, cols=CHUNK_COLS, recs=None):
    return sum(len(chunk_sizes([len(g) for g, c in zip(germs, classes) if c == cls], cols, recs)) for cls in "VJ")


def trace_launch_sizes(hits, m, germs, limit=DIR_BYTES):
    """the alignments per traceback launch: the primary hits with S > 0, class V before class J, contigs in order, each m * g direction
    bytes; a launch grows while used + m * g <= limit"""
    out, used = [], 0
    for cls in ("v", "j"):
        for gene, score in zip(hits[cls]["gene"], hits[cls]["score"]):
            if gene < 0 or score <= 0:
                continue
            b = m * len(germs[gene])
            if used and used + b > limit:
                out.append(0)
                used = 0
            if not out:
                out.append(0)
            out[-1] += 1
            used += b
    return out


def score_launches(n, germs, classes, pairs):
    """the scoring launches that hold work: items are (group of up to 4 contigs, chunk), chunk-major; a launch grows while its
    (contig, record) pairs stay <= pairs"""
    launches, acc = 0, 0
    for cls in "VJ":
        for ng in chunk_sizes([len(g) for g, c in zip(germs, classes) if c == cls], recs=max(1, pairs // WAVES)):
            for gr in range(0, n, WAVES):
                pp = min(WAVES, n - gr) * ng
                if acc and acc + pp > pairs:
                    launches, acc = launches + 1, 0
                acc += pp
    return launches + (acc > 0)


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(list(alpha), int(n)))


def _other(rng, ch):
    return "ACGT".replace(ch, "")[int(rng.integers(0, 3))]


def _carrier(rng, s, subs=40, indels=6):
    """s with `subs` substitutions (each to another base) and `indels` indels of 1 .. 3 bases, insertions and deletions in turn, at
    places at least 100 bases apart and 100 from both ends"""
    s = list(s)
    slots = rng.permutation((len(s) - 200) // 100)[:indels]
    for q in rng.choice(len(s), subs, replace=False):
        s[q] = _other(rng, s[q])
    for k, sl in enumerate(sorted(int(x) for x in slots)[::-1]):               # (from the 3' end, so the places stay where they are)
        q, ln = 100 + 100 * sl + int(rng.integers(0, 50)), int(rng.integers(1, 4))
        if k % 2:
            del s[q:q + ln]
        else:
            s[q:q] = list(_rand(rng, ln))
    return "".join(s)


def _fill(rng, parts, m, at):
    """a contig of m bases: random bases with `parts` joined (20 random bases between them) from offset `at`"""
    body = _rand(rng, 20).join(parts)
    assert at + len(body) <= m, (at, len(body), m)
    return _rand(rng, at) + body + _rand(rng, m - at - len(body))


def _case(V, J, contigs, params):
    recs = [(f"V{k}", s) for k, s in enumerate(V)] + [(f"J{k}", s) for k, s in enumerate(J)]
    return dict(recs=recs, germs=[s for _, s in recs], classes=[h[0] for h, _ in recs], contigs=contigs, params=params, m=len(contigs[0]))


M_LONG = 4095
VA, VB = 1, 3                                                                  # the two 2,047-base records of long_pair and trace_launches
P_OPEN0 = dict(A.DEFAULT, gap_open=0)


@functools.lru_cache(maxsize=None)
def long_pair():
    """six contigs of 4,095 bases that carry a 2,047-base V record (40 substitutions, 6 indels) and a J; V records: two of 2,047 bases, three
    short ones, a copy of a short one"""
    rng = np.random.default_rng(4095)
    V = [_rand(rng, 90), _rand(rng, 2047), _rand(rng, 300), _rand(rng, 2047), _rand(rng, 150)]
    V.append(V[2])
    J = [_rand(rng, 30), _rand(rng, 45), _rand(rng, 60)]
    va, vb = V[VA], V[VB]
    contigs = [_fill(rng, [_carrier(rng, va), J[0]], M_LONG, 11), _fill(rng, [_carrier(rng, va), J[1]], M_LONG, 1900),
               _fill(rng, [_carrier(rng, vb), J[2]], M_LONG, 700), _fill(rng, [_carrier(rng, vb), J[0]], M_LONG, 1333),
               _fill(rng, [_carrier(rng, va[-1500:], 20, 4), J[1]], M_LONG, 0)]
    last = _carrier(rng, vb)                                                   # (the J before the V: the V ends with the contig)
    contigs.append(_fill(rng, [J[2], last], M_LONG, M_LONG - len(last) - 20 - len(J[2])))
    assert all(len(c) == M_LONG for c in contigs) and contigs[5].endswith(last)
    return _case(V, J, contigs, [A.DEFAULT, P_OPEN0])


P_CEILING = dict(match=15, mismatch=31, gap_open=31, gap_extend=31, min_v_score=0, min_j_score=0)
M_CEILING = 2100


@functools.lru_cache(maxsize=None)
def ceiling():
    """match = 15 and a 2,047-base record whole in contig 0: S = 30,705; contigs 1 .. 3 lie just below (one base changed, one base
    deleted, the last base missing)"""
    rng = np.random.default_rng(30705)
    va = _rand(rng, 2047)
    V = [_rand(rng, 200), va]
    J = [_rand(rng, 40), _rand(rng, 33)]
    mid = 1023
    tail = _other(rng, va[-1]) + J[0]
    contigs = [_rand(rng, 7) + va + J[0], va[:mid] + _other(rng, va[mid]) + va[mid + 1:] + J[1], va[:mid] + va[mid + 1:] + "T" + J[0],
               va[:2046] + tail]
    contigs = [c + _rand(rng, M_CEILING - len(c)) for c in contigs]
    return _case(V, J, contigs, [P_CEILING])


N_LONG = 32                                                                    # the 2,047-base records of column_chunks
TIED_IN = [3, 8, 12, 20, 25, 28, 30, 31, 32, 33, 34]                           # the records that hold the first stretch
TWICE_IN = [10, 33]                                                            # ... the second: one on each side of every cut
AFTER_IN, BEFORE_IN = 34, 15


@functools.lru_cache(maxsize=None)
def column_chunks(which, shorts=True):
    """nine contigs of 70 bases against 32 V records of 2,047 bases and 3 short ones: 32 * 2048 + 1 = 65,537 columns, one more than a
    chunk takes, so the first chunk ends after record 30 (set "A"); with record 5 one base shorter (set "B") the 32 share a chunk.  A
    stretch of 70 bases lies in eleven records (seven before A's cut, four after it), a second one in one record on each side, a
    third only behind the cut, a fourth only before it.  shorts=False: the 32 long records alone, so that the V class is exactly 65,537
    (two chunks) or 65,536 columns (one chunk) and the number of chunks tells the two apart"""
    rng = np.random.default_rng(65537)
    V = [_rand(rng, 2047) for _ in range(N_LONG)] + [_rand(rng, 180), _rand(rng, 200), _rand(rng, 190)]
    J = [_rand(rng, 30), _rand(rng, 44), _rand(rng, 60)]
    st = [_rand(rng, 70) for _ in range(4)]

    def plant(r, s, at):
        V[r] = V[r][:at] + s + V[r][at + len(s):]

    for r in TIED_IN:
        plant(r, st[0], int(rng.integers(0, 1900)) if r < N_LONG else 5)
    for r in TWICE_IN:
        plant(r, st[1], int(rng.integers(0, 1900)) if r < N_LONG else 110)
    plant(AFTER_IN, st[2], 100)
    plant(BEFORE_IN, st[3], 1500)
    if which == "B":
        V[5] = V[5][:-1]
    if not shorts:
        V = V[:N_LONG]
    sub = list(st[0])
    for q in (9, 33, 61):
        sub[q] = _other(rng, sub[q])
    contigs = [st[0], st[1], st[2], st[3], "".join(sub), st[1][:30] + st[1][31:] + "G", _rand(rng, 26) + J[1], _rand(rng, 70),
               J[2][:50] + _rand(rng, 20)]
    assert all(len(c) == 70 for c in contigs)
    return _case(V, J, contigs, [A.DEFAULT])


N_TRACE = 34


@functools.lru_cache(maxsize=None)
def trace_launches():
    """34 contigs of 4,095 bases with a V hit of 2,047 bases each: 33 such alignments are the fewest whose direction bytes exceed a
    launch (32 take 268,238,880 of 268,435,456).  Contigs 0 .. 30 cycle through long_pair's four whole carriers (Va, Vb, Va, Vb), contigs
    31 .. 33 -- the last alignment of the first launch, the first two of the second -- are carriers of their own"""
    lp = long_pair()
    rng = np.random.default_rng(268435456)
    V, J = [s for (h, s) in lp["recs"] if h[0] == "V"], [s for (h, s) in lp["recs"] if h[0] == "J"]
    cyc = [lp["contigs"][k] for k in CYCLE]
    own = [_fill(rng, [_carrier(rng, V[VB]), J[2]], M_LONG, 444), _fill(rng, [_carrier(rng, V[VA]), J[1]], M_LONG, 1777),
           _fill(rng, [_carrier(rng, V[VB]), J[0]], M_LONG, 901)]
    contigs = [cyc[k % 4] for k in range(N_TRACE - 3)] + own
    assert len(contigs) == N_TRACE and len(set(contigs)) == 7
    return _case(V, J, contigs, [A.DEFAULT])


CASES = {"long_pair": long_pair, "ceiling": ceiling, "column_chunks_A": functools.partial(column_chunks, "A"),
         "column_chunks_B": functools.partial(column_chunks, "B"), "column_chunks_A_long": functools.partial(column_chunks, "A", False),
         "column_chunks_B_long": functools.partial(column_chunks, "B", False), "trace_launches": trace_launches}
CYCLE = (0, 2, 1, 3)                                                           # long_pair's contigs that trace_launches cycles through


@functools.lru_cache(maxsize=None)
def model(name, k=0):
    """A.annotate(..., fast=True) of case `name` under its k-th parameter set (the same arrays for every caller: do not change them)"""
    c = CASES[name]()
    if name == "trace_launches":                                               # (a contig's hits do not depend on the other contigs: the
        lp, own = model("long_pair", 0), c["contigs"][N_TRACE - 3:]            # cycle's are long_pair's, same records, same parameters)
        assert c["germs"] == long_pair()["germs"] and c["params"][k] == long_pair()["params"][0]
        assert [c["contigs"][q] for q in range(4)] == [long_pair()["contigs"][q] for q in CYCLE]
        ho = A.annotate(own, c["germs"], c["classes"], c["params"][k], fast=True)
        rows = [CYCLE[q % 4] for q in range(N_TRACE - 3)]
        h = {cls: {f: np.concatenate([lp[cls][f][rows], ho[cls][f]]) for f in A.FIELDS} for cls in ("v", "j")}
    else:
        h = A.annotate(c["contigs"], c["germs"], c["classes"], c["params"][k], fast=True)
    for cls in h.values():
        for v in cls.values():
            v.setflags(write=False)
    return h
