"""Named inputs of vdjx_lineage_threshold, each there for one edge of the model (tests/threshold_model.py), and what each must reach in the
model so that no device test passes vacuously (`reaches`, asserted in tests/test_threshold_cpu.py).

A case is (nearest int32[n], length uint32[n], unit, overrides): the call's parameters are a parameter set (DEFAULT or OTHER) with the
case's overrides on top.  The cases whose edge is a parameter (min_values, the peak_shift cut, the valley guard) are built from the set, so
every case holds under both.  Most are written as counts per bin: with unit 2000 and a length of 5, nearest = v falls into bin v exactly."""
import functools

import numpy as np

from tests import threshold_model as M

G, N = M.G, M.N
TILE = 256                                                  # VDJX_THRESHOLD_TILE: the grid points of a density tile
DEFAULT = dict(M.DEFAULTS)
OTHER = dict(max_k=40, peak_shift=3, valley=(1, 3), min_values=5)
SETS = {"default": DEFAULT, "other": OTHER}
LEN1 = 66                                                   # entries of the k = 1 table: a lone bin reaches 65 grid steps either way


def from_bins(counts):
    """{bin: items} -> a case with unit 2000: every item has length 5 and nearest = its bin"""
    v = np.repeat(np.array(sorted(counts), np.int32), [counts[k] for k in sorted(counts)])
    return v.astype(np.int32), np.full(v.shape, 5, np.uint32), 2000, {}


def sampler(n_near, n_far, seed, p_near=0.04, p_far=0.42):
    """the two-mode sampler: junction lengths 30 .. 69, the distance to the nearest binomial(L, 4 %) for clonal relatives and binomial(L,
    42 %) for unrelated sequences; a distance of 0 is no distance (-1)"""
    rng = np.random.default_rng(seed)
    L = rng.integers(30, 70, n_near + n_far)
    d = np.concatenate([rng.binomial(L[:n_near], p_near), rng.binomial(L[n_near:], p_far)])
    return np.where(d == 0, -1, d).astype(np.int32), L.astype(np.uint32), 1, {}


def families_distances():
    """the designed distances of the e2e_families golden: per eligible contig the smallest non-zero Hamming distance to another junction
    of its (vgene, jgene, length) bucket, from the genes and junctions tests/families.py wrote down (no aligner, no device)"""
    from tests import families as F
    from tests import golden_util as GU
    fam = F.build()
    ids, seqs = F.golden_contigs(GU.text(f"{F.TAG}.contigs.fa.gz"))
    who, _ = F.designed(fam, ids, seqs)
    buckets = {}
    for c, k in enumerate(who):
        if k is not None and fam.clones[k].j_names:
            x = fam.clones[k]
            buckets.setdefault((x.vgene, x.jgene, len(x.junction)), []).append(x.junction)
    near, length = [], []
    for js in buckets.values():
        for i, a in enumerate(js):
            ds = [d for d in (F.hamming(a, b) for j, b in enumerate(js) if j != i) if d > 0]
            near.append(min(ds) if ds else -1)
            length.append(len(a))
    return np.array(near, np.int32), np.array(length, np.uint32), 1, {}


def _guard_pair(valley, past):
    """plateau heights (valley p, peaks q) with den p == num q (on the guard) or == num q + 1 (one step past it)"""
    num, den = valley
    for q in range(2, 200):
        for p in range(1, q):
            if den * p == num * q + (1 if past else 0):
                return p, q
    raise AssertionError(valley)


def _plateaus(p, q):
    """three runs of 140 adjacent bins with q, p and q items each: at k = 1 the middle of each is flat at (items) x (the table's sum)"""
    counts = {}
    for lo, c in ((1000, q), (1140, p), (1280, q)):
        counts.update({v: c for v in range(lo, lo + 140)})
    return from_bins(counts)


def build(P):
    """the cases under parameter set P, in a fixed order"""
    mv, shift = P["min_values"], P["peak_shift"]
    cases = {}
    cases["no_item"] = (np.zeros(0, np.int32), np.zeros(0, np.uint32), 1, {})
    cases["all_none"] = (np.full(20, -1, np.int32), np.zeros(20, np.uint32), 1, {})                    # (the lengths are not read)
    few = from_bins({400: (mv - 1) // 2, 4200: mv - 1 - (mv - 1) // 2})
    cases["min_values_less_1"] = few
    cases["min_values"] = (np.concatenate([few[0], [4200]]).astype(np.int32), np.concatenate([few[1], [5]]).astype(np.uint32), 2000, {})
    cases["one_bin"] = from_bins({1500: 30})
    cases["grid_ends"] = from_bins({0: 40, G: 50})
    clamp = from_bins({300: 30, 9000: 10})
    cases["clamped"] = (np.concatenate([clamp[0], [3 * 2000 * 10 + 7] * 25]).astype(np.int32), np.concatenate([clamp[1], [10] * 25]).astype(np.uint32), 2000, {})
    cases["peak_of_two_points"] = from_bins({3000: 20, 3001: 20, 6000: 30})
    cases["floor_of_zeros"] = from_bins({2000: 20, 7001: 20})
    cases["bump_below_cut"] = from_bins({1000: (2 << shift) - 3, 5000: (2 << shift) + 1, 9000: 2})
    cases["bump_on_cut"] = from_bins({1000: (2 << shift) - 3, 5000: 2 << shift, 9000: 2})
    cases["valley_on_guard"] = _plateaus(*_guard_pair(P["valley"], False))
    cases["valley_past_guard"] = _plateaus(*_guard_pair(P["valley"], True))
    two = from_bins({1500: 30, 6000: 30})
    cases["max_k_1"] = two[:3] + (dict(max_k=1),)
    three = from_bins({1000: 30, 5000: 30, 9000: 30})
    cases["max_k_3_three_modes"] = three[:3] + (dict(max_k=3),)
    cases["largest_bin"] = from_bins({4321: (1 << 20) - 1})
    v = np.arange(N)
    full = 1 + 40 * (abs(v - 600) < 150) + 25 * (abs(v - 4300) < 600)
    cases["every_bin"] = from_bins({int(i): int(c) for i, c in zip(v, full)})
    cases[f"tile_ends_peaks_{TILE}"] = from_bins({4 * TILE: 30, 20 * TILE - 1: 30})
    cases[f"tile_ends_floor_{TILE}"] = from_bins({4 * TILE - LEN1: 30, 20 * TILE - 1 + LEN1: 30})
    cases["sampler_80"] = sampler(20, 60, 3)
    cases["sampler_32000"] = sampler(2000, 30000, 3)
    cases["one_mode_sample"] = sampler(0, 300, 11)
    cases["e2e_families"] = families_distances()
    return cases


@functools.lru_cache(maxsize=None)
def cases(which="default"):
    return build(SETS[which])


def params(which, name):
    return dict(SETS[which], **cases(which)[name][3])


@functools.lru_cache(maxsize=None)
def model(which, name):
    """the model's result for a case under a parameter set, computed once"""
    near, length, unit, _ = cases(which)[name]
    return M.threshold(M.bins(near, length, unit), **params(which, name))


def reaches(which, name):
    """what the case is there for, asserted on the model's result"""
    P = params(which, name)
    r = model(which, name)
    i, peaks = r["info"], r["peaks"]
    st = i["status"]
    if name in ("no_item", "all_none"):
        assert st == M.FEW and i["values"] == 0 and not r["density"].any() and not peaks.any()
    elif name == "min_values_less_1":
        assert st == M.FEW and i["values"] == P["min_values"] - 1 and i["distinct"] == 2 and i["k"] == 0 and not r["density"].any()
    elif name == "min_values":
        assert st != M.FEW and i["values"] == P["min_values"] and r["density"].any()
    elif name == "one_bin":
        assert st == M.ONE_MODE and i["k"] == 1 and i["distinct"] == 1 and (i["p1_first"], i["p1_last"]) == (1500, 1500) and i["threshold"] == 0
    elif name == "grid_ends":
        assert st == M.FOUND and i["k"] == 1 and i["p1_first"] == 0 and i["p2_last"] == G and i["threshold"] == G // 2
    elif name == "clamped":
        assert int(r["hist"][G]) == 25 and M.bin_of(60007, 10, 2000) == G and (20000 * 60007 + 20000) // 40000 > G
    elif name == "peak_of_two_points":
        assert st == M.FOUND and i["k"] == 1 and (i["p1_first"], i["p1_last"]) == (3000, 3001)
    elif name == "floor_of_zeros":
        assert st == M.FOUND and i["m"] == 0 and (i["t_first"], i["t_last"]) == (2000 + LEN1, 7001 - LEN1)
        assert i["threshold"] == (i["t_first"] + i["t_last"]) // 2 and (i["t_first"] + i["t_last"]) % 2 == 1        # (rounded down)
    elif name == "bump_below_cut":
        assert peaks[0].tolist() == [3, 2] and st == M.FOUND and i["k"] == 1 and i["p2_first"] == 5000
    elif name == "bump_on_cut":
        assert peaks[0].tolist() == [3, 3] and i["k"] > 1
    elif name == "valley_on_guard":
        assert st == M.FOUND and i["k"] == 1 and P["valley"][1] * i["m"] == P["valley"][0] * min(i["y1"], i["y2"]) and i["t_last"] > i["t_first"]
    elif name == "valley_past_guard":
        assert st == M.SHALLOW and i["k"] == 1 and i["threshold"] == 0
        assert 0 < P["valley"][1] * i["m"] - P["valley"][0] * min(i["y1"], i["y2"]) <= min(i["y1"], i["y2"]) // 2
    elif name == "max_k_1":
        assert P["max_k"] == 1 and peaks.shape == (1, 2) and st == M.FOUND
    elif name == "max_k_3_three_modes":
        assert P["max_k"] == 3 and st == M.NO_SCALE and i["k"] == 3 and i["peaks"] == 3 and r["density"].any() and i["threshold"] == 0
    elif name == "largest_bin":
        assert i["values"] == (1 << 20) - 1 and i["ymax"] == ((1 << 20) - 1) << 30 and st == M.ONE_MODE
    elif name == "every_bin":
        assert i["distinct"] == N and i["values"] < 1 << 20 and M.kernel(152)[1] < N == M.kernel(153)[1]
    elif name.startswith("tile_ends_peaks"):
        assert st == M.FOUND and i["p1_first"] % TILE == 0 and i["p2_last"] % TILE == TILE - 1
    elif name.startswith("tile_ends_floor"):
        assert st == M.FOUND and i["m"] == 0 and i["t_first"] % TILE == 0 and i["t_last"] % TILE == TILE - 1
    elif name in ("sampler_80", "sampler_32000"):
        assert st == M.FOUND and 1000 <= i["threshold"] <= 2500 and i["values"] > (70 if name == "sampler_80" else 31000)
    elif name == "one_mode_sample":
        assert st == M.SHALLOW and i["values"] == 300
    elif name == "e2e_families":
        assert i["values"] == 21 and int(np.flatnonzero(r["hist"])[0]) == 185 and int(np.flatnonzero(r["hist"])[-1]) == 1250
    else:
        raise AssertionError(name)
