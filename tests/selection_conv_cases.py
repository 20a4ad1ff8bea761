"""The handmade vdjx_sel_counts of tests/test_gpu_selconv.py, kept apart so that tests/test_selection_conv_cpu.py can assert, without a GPU,
the conditions under which the GPU test's bounds mean something (a bound that stays small against the row's peak, quantiles that are not
within the bound of their thresholds, the float64 model inside the bound).  Every case: dict(counts, K, group, G)."""
from __future__ import annotations

import numpy as np


def _counts(rows):
    """rows: [(obs_r0, obs_r1, obs_s0, obs_s1, exp_r0, exp_r1, exp_s0, exp_s1)] -> the counts dict Context.selection_convolve takes"""
    a = np.array(rows, dtype=object)
    return dict(obs_r=np.array(a[:, 0:2], np.int32), obs_s=np.array(a[:, 2:4], np.int32), exp_r=np.array(a[:, 4:6], np.uint64),
                exp_s=np.array(a[:, 6:8], np.uint64))


def call_a():
    """K = 2; 13 contigs in groups of 0, 1, 2, 3 and 5 members, one ungrouped contributor and one contig that contributes nothing inside the
    group of 3; the sample row has 12 leaves, a tree of 8 + 4"""
    rng = np.random.default_rng(11)
    group = np.array([4, 2, 3, -1, 4, 1, 3, 4, 3, 2, 4, 3, 4], np.int32)
    rows = []
    for i in range(13):
        if i == 6:                                                 # nothing observed: n = 0 in both regions
            rows.append((0, 0, 0, 0, 5000, 1500, 2500, 700))
            continue
        rows.append((int(rng.integers(0, 7)), int(rng.integers(0, 5)), int(rng.integers(1, 4)), int(rng.integers(0, 3)),
                     int(rng.integers(3000, 9000)), int(rng.integers(800, 2500)), int(rng.integers(1200, 3500)), int(rng.integers(300, 1000))))
    return dict(counts=_counts(rows), K=2, group=group, G=5)


def call_b():
    """K = 1; groups of 6, 7 and 9 members: weights 4 : 2, 4 : (2 : 1) and 8 : 1"""
    rng = np.random.default_rng(12)
    group = np.array([0] * 6 + [1] * 7 + [2] * 9, np.int32)
    group = group[rng.permutation(22)]
    rows = [(int(rng.integers(0, 9)), 0, int(rng.integers(1, 5)), 0, int(rng.integers(3000, 9000)), 0, int(rng.integers(1200, 3500)), 0) for _ in range(22)]
    return dict(counts=_counts(rows), K=1, group=group, G=3)


def call_delta(others=200):
    """K = 1; one group of all nine contigs: a near-delta leaf (n = 1,900) among seven sharp ones, then a flat one (n = 1) -- the block of
    eight meets the flat leaf at weights 8 : 1.  (Seven sharp neighbours, not seven flat ones: the bound of the near-delta leaf doubles at
    each of its three levels, and only a root about as narrow as that leaf keeps the bound under 1e-9 of the root's peak.)"""
    rows = [(950, 0, 950, 0, 4000, 0, 4000, 0)]
    rows += [(others // 2 + 3 * i, 0, others - others // 2 - 3 * i, 0, 4000 + 100 * i, 0, 4000, 0) for i in range(1, 8)]
    rows.append((1, 0, 0, 0, 6000, 0, 2000, 0))
    return dict(counts=_counts(rows), K=1, group=np.zeros(9, np.int32), G=1)


def call_ends():
    """K = 1; group 0: two members whose odds put their peaks on grid point +20.00 (the mass of u = v = 2000: q + 1 would be cell 4001);
    group 1: two on -20.00; group 2: none, the prior"""
    rows = [(400, 0, 0, 0, 1, 0, 1 << 40, 0), (300, 0, 0, 0, 1, 0, 1 << 41, 0)]
    rows += [(0, 0, 400, 0, 1 << 40, 0, 1, 0), (0, 0, 300, 0, 1 << 41, 0, 1, 0)]
    return dict(counts=_counts(rows), K=1, group=np.array([0, 0, 1, 1], np.int32), G=3)


CASES = {"a": call_a, "b": call_b, "delta": call_delta, "ends": call_ends}
