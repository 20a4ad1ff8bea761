"""The pools of tests/test_gpu_part_records.py (k_part_records_g: every gated tuple made once, in the counting pass) and what
tests/test_part_records_pools.py checks about them on the CPU.

A pool is a CIRCLE of bases read at every start: L reads of a random circular sequence of L bases, read s being bases s .. s + rl - 1.
Every k-mer of the circle then stands at every offset of some read, in rl - k + 1 DISTINCT reads -- so it is gated more than once, is seen
in more than one read and survives mf = 2 -- and every read has its reverse-complement record behind it (couples, as the reader writes
them).  Phred 40 throughout but for the bases a pool spoils on purpose (Phred 12: below the gate's 20)."""
import types

import numpy as np

SEED = 20261021
_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b
GOOD, BAD = 40 + 33, 12 + 33


def circle_reads(L, rl, alphabet, rng):
    """[L, rl] ASCII: the L reads of a random circle over `alphabet`."""
    g = np.frombuffer(alphabet.encode(), np.uint8)[rng.integers(0, len(alphabet), L)]
    return g[(np.arange(L)[:, None] + np.arange(rl)[None, :]) % L]


def couples(reads, quals):
    """reads, quals [n, rl] -> records [2n, 2 rl + 1]: read, its reverse complement (qualities reversed), read, ..."""
    n, rl = reads.shape
    rec = np.empty((n, 2, 2 * rl + 1), np.uint8)
    rec[:, :, 0] = ord("0")
    rec[:, 0, 1:1 + rl], rec[:, 0, 1 + rl:] = reads, quals
    rec[:, 1, 1:1 + rl], rec[:, 1, 1 + rl:] = _COMP[reads[:, ::-1]], quals[:, ::-1]
    return np.ascontiguousarray(rec.reshape(2 * n, 2 * rl + 1))


def _pool(records, rl):
    return types.SimpleNamespace(primary=records, secondary=np.zeros((0, 2 * rl + 1), np.uint8), rl=rl)


def make(kind, rl=50):
    """kind:
    clean / clean37   2,048 (+ 37: a short last row of 64) couples over ACGT, all gated; the canonical side changes from offset to offset
    forward / reverse the circle over AC (GT): the first record's k-mer is the smaller (larger) of the two at every offset, whatever the packing
    pieces            every other read has ONE spoiled base, its place moving from read to read: the gated offsets are 0 .. p - k and
                      p + 1 .. rl - k, on one side, the other or both sides of every boundary of 8 or 16 offsets
    dense_head        512 clean couples (a circle of their own), then 1,536 with nothing gated (a circle of their own, base 20 spoiled):
                      the host sizes the round from the pool's mean, a quarter of what the head holds, so the head's rounds do not fit
                      and are retried with half the records, twice
    odd               `clean` without its last record: not a pool of couples, the build takes the form that walks every record
    long              1,024 couples of 100 bases (the long-read instantiation)"""
    rng = np.random.default_rng(SEED)
    if kind == "long":
        rl = 100
    if kind in ("clean", "clean37", "odd", "long", "forward", "reverse", "pieces"):
        L = {"clean37": 2048 + 37, "long": 1024}.get(kind, 2048)
        reads = circle_reads(L, rl, {"forward": "AC", "reverse": "GT"}.get(kind, "ACGT"), rng)
        quals = np.full(reads.shape, GOOD, np.uint8)
        if kind == "pieces":
            s = np.arange(1, L, 2)
            quals[s, (s // 2) % rl] = BAD
        rec = couples(reads, quals)
        return _pool(rec[:-1] if kind == "odd" else rec, rl)
    if kind == "dense_head":
        head = circle_reads(512, rl, "ACGT", rng)
        tail = circle_reads(1536, rl, "ACGT", rng)
        qh, qt = np.full(head.shape, GOOD, np.uint8), np.full(tail.shape, GOOD, np.uint8)
        qt[:, 20] = BAD
        return _pool(np.concatenate([couples(head, qh), couples(tail, qt)]), rl)
    raise ValueError(kind)


def gated_mask(pool, k):
    """[records, rl - k + 1] bool: the offsets whose k bases are all ACGT with Phred >= 20 (include_kmer)."""
    rl = pool.rl
    bad = (pool.primary[:, 1:1 + rl] == ord("N")) | (pool.primary[:, 1 + rl:] < 20 + 33)
    c = np.concatenate([np.zeros((bad.shape[0], 1), np.int64), np.cumsum(bad, axis=1)], axis=1)
    return (c[:, k:] - c[:, :rl - k + 1]) == 0


def forward_is_smaller(pool, k):
    """[couples, rl - k + 1] bool: the k-mer of a couple's FIRST record at an offset is smaller than its reverse complement (A < C < G < T,
    the first base the most significant)."""
    rl = pool.rl
    n = pool.primary.shape[0] // 2
    fwd, rc = pool.primary[0:2 * n:2, 1:1 + rl], pool.primary[1:2 * n:2, 1:1 + rl]
    out = np.zeros((n, rl - k + 1), bool)
    for o in range(rl - k + 1):
        x, y = fwd[:, o:o + k], rc[:, rl - k - o:rl - o]
        d = x != y
        first = d.argmax(axis=1)
        assert d.any(axis=1).all()                       # (k odd: a k-mer is never its own reverse complement)
        i = np.arange(n)
        out[:, o] = x[i, first] < y[i, first]            # (ASCII order of ACGT is the codes' order)
    return out
