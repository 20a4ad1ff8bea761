"""The cases of tests/rindex_cases.py reach what they are for: shown without a GPU.  The constants of the folding are read out of
vdjx_rindex.hip and vdjx_common.h and every case's class sizes and distinct counts are held to THEM, so that a changed constant fails here
with a message instead of silently missing its route on the GPU; the oracle maps every string of every case to exactly the planted pairs
(and to what the model of rindex_cases makes of the whole pool, position by position); and each of five folds gone wrong, computed in the
model, changes a named pair count.  Why the cases are needed: the largest read-1 class of the pools that
test_read_index_over_couples_equals_the_general_build indexes has 11 members -- no pool of the suite below the 10 M-pair digests left the
small and the wave route."""
import os
import re
from collections import Counter

import pytest

from tests import rindex_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(name):
    with open(os.path.join(ROOT, "vdjer_amd", "csrc", name)) as f:
        return f.read()


def _define(src, name):
    m = re.search(rf"#define {name} (\d+)u?\b", src)
    assert m, f"{name} is no longer a plain #define"
    return int(m.group(1))


@pytest.fixture(scope="module")
def K():
    """the constants as the sources have them"""
    ri, common = _source("vdjx_rindex.hip"), _source("vdjx_common.h")
    k = {n: _define(ri, "RI_" + n) for n in ("FOLD_SMALL", "FOLD_WAVE", "FOLD_SLOTS", "FOLD_BIG_SLOTS", "FOLD_BIG_THREADS", "FM_PER")}
    k["MAXCNT"] = _define(common, "RI_ENT_MAXCNT")
    m = re.search(r"full = s_distinct > RI_FOLD_BIG_SLOTS \* (\d+) / (\d+);", ri)
    assert m, "k_ri_fold_big's `full` is no longer `s_distinct > RI_FOLD_BIG_SLOTS * 3 / 4`"
    k["FULL"] = k["FOLD_BIG_SLOTS"] * int(m.group(1)) // int(m.group(2))
    m = re.search(r"max_giant < (\d+)u \? max_giant : (\d+)u", ri)
    assert m and m.group(1) == m.group(2), "k_ri_fold_big's grid is no longer min(max_giant, 2048)"
    k["GRID"] = int(m.group(1))
    assert "max_giant = n1 / (RI_FOLD_WAVE + 1) + 1" in ri
    assert "s_big[RI_FM_PER / (RI_FOLD_SMALL + 1) + 2]" in ri
    k["S_BIG"] = k["FM_PER"] // (k["FOLD_SMALL"] + 1) + 2
    # the routes: up to SMALL by the members' threads, up to WAVE by a wave, beyond by k_ri_fold_big
    assert "if (m <= RI_FOLD_SMALL) {" in ri and "is_giant = m > RI_FOLD_WAVE; is_big = !is_giant;" in ri and "m > RI_FOLD_SMALL && i == s" in ri
    assert "at += RI_FOLD_BIG_THREADS" in ri
    return k


def test_the_model_has_the_constants_of_the_sources(K):
    mine = dict(FOLD_SMALL=RC.FOLD_SMALL, FOLD_WAVE=RC.FOLD_WAVE, FOLD_SLOTS=RC.FOLD_SLOTS, FOLD_BIG_SLOTS=RC.BIG_SLOTS, FOLD_BIG_THREADS=RC.BIG_THREADS,
                FM_PER=RC.FM_PER, MAXCNT=RC.MAXCNT, FULL=RC.BIG_FULL, GRID=RC.BIG_GRID)
    for n, v in mine.items():
        assert K[n] == v, f"{n}: the sources have {K[n]}, tests/rindex_cases.py has {v}: move the cases with the constant"
    assert K["FOLD_WAVE"] <= K["FOLD_SLOTS"] // 2, "a wave's table can fill"
    assert K["MAXCNT"] == 255 and K["FOLD_WAVE"] <= 2 * K["MAXCNT"], "the wave route's `one entry, or two`"


def _sizes_of(c):
    return Counter(len(c.model.keys.get(cl["seq"], ())) for cl in c.classes)


def _walk(keys, K):
    """(rows that leave unfolded, largest fill of the table) of a giant class: rows of FOLD_BIG_THREADS, the fill read once per row"""
    seen, unfolded = set(), 0
    for at in range(0, len(keys), K["FOLD_BIG_THREADS"]):
        if len(seen) > K["FULL"]:
            unfolded += len(keys[at:at + K["FOLD_BIG_THREADS"]])
        else:
            seen.update(keys[at:at + K["FOLD_BIG_THREADS"]])
    return unfolded, len(seen)


@pytest.mark.parametrize("rl,name", [(rl, n) for rl, names in ((RC.RL, RC.NAMES), (RC.RL_LONG, RC.LONG_NAMES)) for n in names])
def test_case_reaches_its_edge(K, rl, name):
    c = RC.case(name, rl)
    m = c.model
    assert c.what and m.couples and 6 <= len(c.wins) <= 14 and c.pool.n_pairs <= 12100
    S, W, T = K["FOLD_SMALL"], K["FOLD_WAVE"], K["FOLD_BIG_THREADS"]
    for cl in c.classes:                                         # the planted classes are what they were planted as: no base read joined them
        keys = m.keys.get(cl["seq"], [])
        assert len(keys) == cl["members"], (name, cl["what"], len(keys))
        if cl["members"]:
            assert len(set(keys)) == cl["distinct"], (name, cl["what"], len(set(keys)))
        twin = m.keys.get(RC.synth.revcomp(cl["seq"]), [])
        assert len(twin) == cl["members"], (name, cl["what"], "twin")
    sizes = _sizes_of(c)
    if name in ("sizes",) + RC.ORDERS:
        assert sorted(sizes) == sorted(RC.SIZES)
        need = {1, S - 1, S, S + 1, 63, 64, 65, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 1}
        assert need <= set(sizes), f"class sizes {sorted(need - set(sizes))} are missing: both sides of RI_FOLD_SMALL={S}, RI_FOLD_WAVE={W}, the rows of 64 and of {T}"
        for cl in c.classes:
            assert cl["distinct"] >= min(cl["members"], 3)
    if name == "pieces":
        per_route = {}
        for cl in c.classes:
            per_route.setdefault(RC.route(cl["members"]), []).append((cl["members"], sorted(Counter(m.keys[cl["seq"]]).values())))
        mults = lambda r: sorted(x for _, v in per_route[r] for x in v if x > S)          # noqa: E731
        assert mults("giant") == sorted(RC.PIECES), mults("giant")
        assert [-(-n // K["MAXCNT"]) for n in RC.PIECES] == [1, 1, 2, 2, 2, 3, 4]
        assert {254, 255, 256} <= set(mults("wave")) and (W, [W]) in per_route["wave"], "a class of exactly RI_FOLD_WAVE members of one entry: two pieces on the wave route"
        assert all(200 <= n <= W for n, _ in per_route["wave"]) and all(n >= 300 for n, _ in per_route["giant"])
        assert sorted(per_route["small"]) == [(S, [1] * S), (S, [S])]
    if name.startswith("nines"):
        want = {S + 1: 500} if name == "nines" else {S + 1: 10, W + 1: 10}
        assert sizes == want
        assert set(map(len, m.keys.values())) == set(want), "nothing else is a read 1"
    if name == "nines":
        # whatever the numbering of the classes, class starts lie S + 1 members apart: per workgroup of FM_PER members
        n1 = m.r1_members
        starts = Counter(i // K["FM_PER"] for i in range(0, n1, S + 1))
        full = [starts[b] for b in range(n1 // K["FM_PER"])]
        assert n1 == 9000 and set(full) == {K["S_BIG"] - 2, K["S_BIG"] - 1}, full      # 113 or 114 of the 115 places of s_big[]
    if name.startswith("overflow"):
        (cl,) = c.classes
        unfolded, fill = _walk(m.keys[cl["seq"]], K)
        gain = m.entries() - m.entries_folded_minimum()
        n_mapped = sum(RC.OVERFLOW_MAPPED)
        if name == "overflow_tail":
            assert fill == 13 * T > K["FULL"] and unfolded == 6700 - 13 * T + n_mapped
            assert 13 * T <= 6700, "every mapping row lies in the part that leaves unfolded"
        if name == "overflow_head":
            assert fill > K["FULL"] and unfolded == (n_mapped + 6700) % T + 40
        if name == "overflow_at_6144":
            assert fill == K["FULL"] == 12 * T and unfolded == 0 and gain == 0, "exactly RI_FOLD_BIG_SLOTS * 3 / 4 distinct entries: `full` is never taken"
        if name == "overflow_at_6145":
            assert fill == K["FULL"] + 1 and unfolded == 300
            assert len(set(m.keys[cl["seq"]][:12 * T])) == K["FULL"], "the fill is RI_FOLD_BIG_SLOTS * 3 / 4 at a multiple of 512 rows, one more a row later"
        if name != "overflow_at_6144":
            assert gain > 0, "the overflow writes more entries than the folded minimum"
    if name.startswith("giants"):
        n1 = m.r1_members
        giants = sum(len(v) > W for v in m.keys.values())
        assert giants == 6 and n1 // (W + 1) + 1 == 7 and n1 == (6 * (W + 1) if name == "giants" else 7 * (W + 1) - 1)
        # k_ri_fold_big has min(n1 / 257 + 1, GRID) workgroups for at most n1 / 257 giant classes: a workgroup takes a second class
        # (`b += gridDim.x`) only past GRID giant classes = 526,593 read-1 members, which no pool of 12,000 pairs (48,000 records) has
        assert (K["GRID"] + 1) * (W + 1) > 4 * 12100
    if name == "palindrome":
        pal = c.classes[0]["seq"]
        assert pal == RC.synth.revcomp(pal) and len(m.keys[pal]) == 300 > W and m.classes_couples == m.classes_general + 1
        assert sum(k[2] & RC.RC != 0 for k in m.keys[pal]) == 150
        assert all(k[0] == k[1] == pal for k in m.keys[c.classes[1]["seq"]])
    if name == "read2_shapes":
        ks = [k for v in m.keys.values() for k in v]
        assert sum(k[0] is not None and k[1] is None for k in ks) == 2 * 23, "B = none"
        assert sum(k[0] is not None and k[0] == k[1] for k in ks) == 2 * 10, "A = B"
        assert sum(k[0] is None and k[1] is None for k in ks) == 2 * 10 and all(k[2] & (RC.RCA | RC.RCB) == 0 for k in ks if k[0] is None), "an N in read 2"
        n_in_r1 = sum(c.pool.read_num[r] == 1 and "N" in s for r, s in enumerate(m.seq))
        assert n_in_r1 == 2 * 6 and m.r1_members == 2 * 3000 - n_in_r1
    want_order = dict(order_one_run=0, order_second_empty=1, order_first_empty=1, order_permuted=2).get(name, 0 if c.pool.secondary.shape[0] == 0 else 1)
    assert m.rank_order == want_order
    if name == "order_second_empty":
        assert m.n1_first_run == m.r1_members
    if name == "order_first_empty":
        assert m.n1_first_run == 0


def test_the_pools_of_the_couples_test_never_leave_the_wave_route(K):
    """the measured reason for the cases: the largest read-1 class of the three pools of test_read_index_over_couples_equals_the_general_build
    (tests/test_gpu_parity.py) is far below RI_FOLD_WAVE + 1, and a few classes in 5,500 pass RI_FOLD_SMALL (DESIGN §4 quotes the numbers)"""
    from vdjer_amd import synth
    rep = synth.make_repertoire(6, seed=191)
    seen = {}
    for rl in (50, 36, 64):
        pool = synth.make_reads(rep, 6000, noise_frac=0.25, seed=192, rl=rl, err=0.004, n_rate=0.003)
        sizes = [len(v) for v in RC.Model(pool).keys.values()]
        seen[rl] = (max(sizes), sum(n > K["FOLD_SMALL"] for n in sizes), len(sizes))
        assert max(sizes) <= K["FOLD_WAVE"], seen
    assert seen == {50: (11, 20, seen[50][2]), 36: (10, 20, seen[36][2]), 64: (9, 2, seen[64][2])}, seen


@pytest.mark.parametrize("rl,name", [(rl, n) for rl, names in ((RC.RL, RC.NAMES), (RC.RL_LONG, RC.LONG_NAMES)) for n in names])
def test_oracle_maps_the_planted_pairs(rl, name):
    c = RC.case(name, rl)
    verdicts = set()
    for i, (w, (pairs, valid)) in enumerate(zip(c.wins, RC.oracle_results(name, rl))):
        ent, npairs, at = c.model.window(w)
        got = Counter(zip(pairs["pos1"].tolist(), pairs["pos2"].tolist()))
        assert got == at and npairs == len(pairs), (name, i, [(k, got[k], at[k]) for k in set(got) | set(at) if got[k] != at[k]][:5])
        verdicts.add(valid)
    for (i, pos1, pos2), n in c.planted.items():
        pairs = RC.oracle_results(name, rl)[i][0]
        assert int(((pairs["pos1"] == pos1) & (pairs["pos2"] == pos2)).sum()) == n, (name, i, pos1, pos2, n)
    assert sum(c.planted.values()) > 0
    assert verdicts >= set(c.verdicts), (name, verdicts)


# a fold gone wrong -> the cases that must notice
SENSITIVE = [("saturate", "pieces"), ("drop_second", "pieces"), ("lose_unfolded", "overflow_tail"), ("lose_unfolded", "overflow_head"),
             ("lose_unfolded", "overflow_at_6145"), ("no_wave", "sizes"), ("no_wave", "nines"), ("no_wave", "nines_257"), ("first_block", "sizes"),
             ("first_block", "pieces"), ("first_block", "overflow_head"), ("saturate", "sizes"), ("drop_second", "sizes")]


@pytest.mark.parametrize("wrong,name", SENSITIVE)
def test_a_wrong_fold_changes_a_pair_count(wrong, name):
    assert wrong in RC.WRONG
    c = RC.case(name)
    counts = [(i, len(pairs), c.model.window(w, wrong)[1]) for i, (w, (pairs, _)) in enumerate(zip(c.wins, RC.oracle_results(name)))]
    said = "; ".join(f"window {i}: {right} pairs, {bad} under `{wrong}`" for i, right, bad in counts)
    assert any(right != bad for _, right, bad in counts), f"{name}: no window's pair count changes -- {said}"
    print(name, said)


def test_a_wrong_fold_is_covered_for_every_kind():
    assert {w for w, _ in SENSITIVE} == set(RC.WRONG)
