"""Handmade placements for vdjx_quant_pairs (include/vdjx.h): the cases tests/test_quant_cpu.py and tests/test_gpu_quant_edges.py share,
each built once.  A case is a dict: offs uint64[n + 1], pid uint32[A], ins int16[A] (contig-major, as vdjx_map_emit returns them), n, L,
n_pairs; triples(case) gives the (pair, contig, insert) arrays tests/quant_model.py takes.

The sizes the kernels of vdjer_amd/csrc/vdjx_quant.hip turn on, restated here (the tests assert that the cases sit on them):"""
import functools

import numpy as np

Q_LIGHT = 32                 # a pair with more alignments is reduced by the whole wave (k_q_order, k_q_estep)
Q_CHUNK = 2048               # alignments per workgroup of k_q_mpart
Q_BATCH = 32                 # iterations enqueued between two looks at the stop flag
Q_FIN = 1024                 # threads of k_q_mfin: contig c is thread c % 1024's
WAVE = 64

A_DEGREES = (1, 2, 31, 32, 33, 63, 64, 65, 100)
A_SLOTS = (3, 252, 4100)     # where each of the three runs of A_DEGREES starts among the placed pairs (in id order)
A_BIG = 4097                 # alignments on contig 100
B_SIZES = (0, 1, 255, 0, 256, 257, 0, 0, 2047, 2048, 2049, 4096, 4097, 0)
C_EMPTY = 2                  # the contigs c % 7 == 2 (1024 among them) have no pair of degree 1
E_LENS = (49, 50, 51, 360, 400, 401, 4095)


def _case(contig, pid, ins, n, L, n_pairs, rng):
    """placements in any order -> contig-major, the order inside a contig shuffled"""
    contig, pid, ins = np.asarray(contig, np.int64), np.asarray(pid, np.int64), np.asarray(ins, np.int64)
    o = rng.permutation(contig.size)
    o = o[np.argsort(contig[o], kind="stable")]
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(np.bincount(contig, minlength=n))
    assert pid.size == 0 or (0 <= pid.min() and pid.max() < n_pairs)
    return dict(offs=offs, pid=pid[o].astype(np.uint32), ins=ins[o].astype(np.int16), n=n, L=L, n_pairs=n_pairs)


def triples(case):
    contig = np.repeat(np.arange(case["n"]), np.diff(case["offs"]).astype(np.int64))
    return case["pid"].astype(np.int64), contig, case["ins"].astype(np.int64)


@functools.lru_cache(maxsize=None)
def case_a():
    """101 contigs of 360 bases.  Placed pairs in id order ("slots": the E step gives slot q to thread q, 64 slots a wave, 256 a
    workgroup): three runs of the degrees 1, 2, 31, 32, 33, 63, 64, 65, 100 on distinct random contigs among the first 100 -- at slots
    3.. (heavy and light pairs in one wave), 252.. (32 is the last slot of a workgroup, 33 the first of the next) and 4100.. (the
    grid's last wave, of 28 slots); all other slots are the 4,097 pairs of contig 100, every third of them placed on one more contig.
    Slot q has id 2 q + 1 and n_pairs = 2 * placed + 1: every other id has no placement, ids 0 and n_pairs - 1 among them."""
    rng = np.random.default_rng(4097)
    n_placed = 3 * len(A_DEGREES) + A_BIG
    degree = np.zeros(n_placed, np.int64)
    for s in A_SLOTS:
        degree[s:s + len(A_DEGREES)] = A_DEGREES
    contig, pid = [], []
    k = 0
    for q in range(n_placed):
        if degree[q]:
            on = rng.choice(100, degree[q], replace=False).tolist()
        else:
            on = [100] + ([int(rng.integers(0, 100))] if k % 3 == 0 else [])
            k += 1
        contig += on
        pid += [2 * q + 1] * len(on)
    assert k == A_BIG
    ins = rng.integers(50, 361, len(pid))
    return _case(contig, pid, ins, 101, 360, 2 * n_placed + 1, rng)


@functools.lru_cache(maxsize=None)
def case_b():
    """contigs of B_SIZES alignments, every pair of degree 1 with an insert inside the window: every r is 1.0"""
    rng = np.random.default_rng(2048)
    contig = np.repeat(np.arange(len(B_SIZES)), B_SIZES)
    n_pairs = 3 * contig.size + 2
    pid = 1 + rng.choice(n_pairs - 2, contig.size, replace=False)         # (ids 0 and n_pairs - 1 stay free)
    return _case(contig, pid, rng.integers(50, 361, contig.size), len(B_SIZES), 360, n_pairs, rng)


@functools.lru_cache(maxsize=None)
def case_c(n):
    """n contigs, a pair of degree 1 on each but the c % 7 == 2; five pairs of degree 2 with inserts of 80 and 340 bases: on the two
    last contigs where n <= 1025 (1023 and 1024 at n = 1025: contig 1024 has no other placement and takes the 80s), on contigs of
    index 1024 and more at n = 2049 (-> the contigs that move)"""
    rng = np.random.default_rng(1024 + n)
    contig = [c for c in range(n) if c % 7 != C_EMPTY]
    pid = list(range(1, len(contig) + 1))
    ins = rng.integers(50, 361, len(contig)).tolist()
    if n <= 1025:
        two = [(n - 1, n - 2)] * 5
    else:
        two = [(1024, 1025), (1024, 2048), (1500, 2047), (2048, 1027), (1031, 1030)]
    for k, (lo, hi) in enumerate(two):
        contig += [lo, hi]
        pid += [5000 + k] * 2
        ins += [80, 340]
    moving = sorted({c for t in two for c in t})
    return dict(_case(contig, pid, ins, n, 360, 5006, rng), moving=moving)


@functools.lru_cache(maxsize=None)
def case_d(n_pairs, last_placed):
    """every other id placed (the last one or not), degrees 1 to 3 on five contigs"""
    rng = np.random.default_rng(n_pairs * 2 + last_placed)
    ids = np.arange((n_pairs - 1) % 2 if last_placed else n_pairs % 2, n_pairs, 2)
    deg = rng.integers(1, 4, ids.size)
    pid = np.repeat(ids, deg)
    contig = np.concatenate([rng.choice(5, d, replace=False) for d in deg])
    return _case(contig, pid, rng.integers(50, 361, pid.size), 5, 360, n_pairs, rng)


@functools.lru_cache(maxsize=None)
def case_e(L):
    """inserts from the window's edges and beyond: every one of them alone on a pair of degree 1, and in pairs of degree 3 -- with two
    inserts inside the window, with one, and with none (all three alignments weigh zero)"""
    rng = np.random.default_rng(50 + L)
    edge = [-5, 0, 49, 50, L, L + 1, 400, 401, 32767]
    inside = [f for f in (60, 75, 123, 200, 333) if f <= L] or [50]
    zero = lambda f: not (50 <= f <= min(400, L))                         # noqa: E731
    out = [f for f in edge if zero(f)]
    n = 6
    contig, pid, ins = [], [], []

    def pair(fs):
        k = len(set(pid)) * 2 + 1                                          # (odd ids: every other id has no placement)
        on = rng.choice(n - 1, len(fs), replace=False) + 1                 # (contig 0 has no placement)
        contig.extend(on.tolist())
        pid.extend([k] * len(fs))
        ins.extend(fs)

    for f in edge + inside:
        pair([f])
    for i, f in enumerate(edge):
        pair([f, inside[i % len(inside)], inside[(i + 1) % len(inside)]])
        pair([f, out[i % len(out)], inside[i % len(inside)]])
        pair([f if zero(f) else out[0], out[i % len(out)], out[(i + 2) % len(out)]])
    return _case(contig, pid, ins, n, L, 2 * len(set(pid)) + 1, rng)
