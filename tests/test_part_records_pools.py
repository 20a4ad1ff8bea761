"""The pools of tests/test_gpu_part_records.py do what their descriptions say -- checked with the oracle alone, no GPU: every k-mer is
gated at least twice and survives mf = 2 (so a wrong key or instance of any tuple moves a node's first_inst or gated_count), the
intended side of a couple is the canonical one, the spoiled bases split the gated offsets where the listing trips meet."""
import pytest

from oracle import oracle

from tests import part_records_pools as PP

MF, MQ = 2, 60


def _table(pool, k):
    t = oracle.KmerTable(pool, k)
    first, count, multi, _ = t.export()
    return t, first, count, multi


@pytest.mark.parametrize("kind,k", [("clean", 25), ("clean", 35), ("clean", 47), ("clean37", 35), ("forward", 35), ("reverse", 35),
                                    ("pieces", 25), ("pieces", 35), ("dense_head", 35), ("odd", 35), ("long", 35)])
def test_every_kmer_is_gated_twice_and_survives(kind, k):
    pool = PP.make(kind)
    t, first, count, multi = _table(pool, k)
    assert int(count.sum()) == int(PP.gated_mask(pool, k).sum()) > 0          # (no count near the table's cap: the sum is the instances)
    assert count.min() >= 2 and multi.all()
    pre = t.size()
    assert t.prune(MF, MQ) == pre == t.size()


def test_the_canonical_side_is_the_intended_one():
    f = PP.forward_is_smaller(PP.make("forward"), 35)
    assert f.all()
    r = PP.forward_is_smaller(PP.make("reverse"), 35)
    assert not r.any()
    for k in (25, 35, 47):
        m = PP.forward_is_smaller(PP.make("clean"), k)
        # within a read: both sides occur among the offsets of nearly every couple, and the side changes between neighbouring offsets
        assert (m.any(axis=1) & ~m.all(axis=1)).mean() > 0.7
        assert (m[:, 1:] != m[:, :-1]).any(axis=1).mean() > 0.7


def test_the_spoiled_bases_split_the_listing_trips():
    pool = PP.make("pieces")
    for k, steps in ((25, (8, 16)), (35, (8,))):
        g = PP.gated_mask(pool, k)[0::2]                  # the couples' first records
        P = g.shape[1]
        n = g.sum(axis=1)
        assert (n == P).sum() == g.shape[0] // 2          # every other read is clean
        for step in steps:
            # a boundary of the listing (16 offsets a trip; 8 if it is ever halved) with gated offsets on both sides and fewer than all,
            # only before it, and only behind it
            lo, hi = g[:, :step].sum(axis=1), g[:, step:].sum(axis=1)
            part = n < P
            assert (part & (lo > 0) & (hi > 0)).any() and (part & (lo > 0) & (hi == 0)).any() and (part & (lo == 0) & (hi > 0)).any()


def test_the_dense_head_overfills_a_round_sized_from_the_mean():
    pool = PP.make("dense_head")
    g = PP.gated_mask(pool, 35)[0::2].sum(axis=1)
    assert g[:512].tolist() == [16] * 512 and not g[512:].any()
    # the round's room is at most the 6,144 tuples of the 96 KB stage: a round sized for the pool's mean of 4 tuples a couple takes
    # more than 1,024 couples, the head's 512 hold 8,192 tuples, and so do the 512 of the first retry
    assert 512 * 16 > 6144 and g.mean() == 4.0
