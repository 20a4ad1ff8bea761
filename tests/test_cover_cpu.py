"""The case table of the coverage validator (tests/cover_cases.py) against the oracle alone: every twin has the verdicts (1, 0), every
window takes the path of the kernel it was built for, and the table as a whole reaches every path with a valid and an invalid window.
tests/test_gpu_cover.py then runs k_window_cover on the same windows."""
from collections import Counter

import numpy as np
import pytest

from tests import cover_cases as CC


def _id(t):
    return t[0].name[:-1]


@pytest.mark.parametrize("t", CC.twins(), ids=_id)
def test_twin_has_verdicts_1_and_0(t):
    good, bad = t
    assert (CC.verdict(good), CC.verdict(bad)) == (1, 0), (good, bad)
    if bad.rule2:
        # rule 2 is what refuses the invalid member: with nothing for rule 2 to test it is valid
        assert CC.rule1_alone(bad) == 1 and CC.rule1_alone(good) == 1, (good, bad)
        assert CC.short_of_floor(bad) and not CC.short_of_floor(good), (good, bad)


def test_singles_have_their_verdicts():
    for w in CC.singles():
        if w.expect is not None:
            assert CC.verdict(w) == w.expect, w
    mixed = [CC.verdict(w) for w in CC.singles() if w.family == "mixed"]
    sizes = [len(w.entries) for w in CC.singles() if w.family == "mixed"]
    assert len(mixed) == 70 and 10 <= sum(mixed) <= 60 and sizes.count(0) >= 5 and max(sizes) >= 500 and len({s.bit_length() for s in sizes}) >= 5, (sum(mixed), sorted(sizes))


def test_counting_model_agrees_with_the_oracle_on_rule_2():
    """short_of_floor (a count over rows) and the oracle: where rule 1 passes, the window is valid iff nothing tested is short"""
    n = 0
    for w in CC.all_windows():
        if w.par.floor == 0 or len(w.entries) > 1500 or w.family == "histogram":
            continue
        if CC.rule1_alone(w) == 1:
            j_ok = all(0 <= pos + d <= w.ln + 1023 for pos, d in CC.tested(w))
            assert CC.verdict(w) == (1 if j_ok and not CC.short_of_floor(w) else 0), w
            n += 1
    assert n > 200


def test_every_window_takes_its_path():
    for w in CC.all_windows():
        got = CC.path(w)
        for k, v in w.want.items():
            assert got[k] == v, (w, k, got)


def test_one_short_twins_are_short_at_one_place():
    for name, (target, hole) in CC.ONE_SHORT.items():
        good, bad = next(t for t in CC.twins() if _id(t) == name)
        assert CC.short_of_floor(bad) == [target] and target[1] == hole, (name, target, hole)
        db = CC.path(bad)["db"]
        clo, chi = CC.band(bad.rl, bad.par)
        at = (hole - clo) % db
        assert at in (0, db - 1) or hole == chi - 1, (name, hole)
    batches = {(CC.path(b)["db"], (t[1] - CC.band(b.rl, b.par)[0]) // CC.path(b)["db"]) for (_, b) in CC.twins() if b.family == "batches"
               for t in [CC.ONE_SHORT[b.name[:-1]][0]]}
    assert batches == {(db, k) for db in (22, 8, 6) for k in (0, 1, 3)}, batches


def test_table_reaches_every_path_with_both_verdicts():
    seen = Counter()
    for w in CC.all_windows():
        p, v = CC.path(w), CC.verdict(w)
        if w.par.floor == 0:
            continue
        seen[("priv", p["priv"], v)] += 1
        if w.par.floor == 1 and p["nd"] >= 1:
            seen[("by_bits", p["by_bits"], v)] += 1
        if p["batches"] == 1:
            seen[("batches", 1, v)] += 1
        if p["batches"] >= 3:
            seen[("batches", 3, v)] += 1
        if p["batches"] >= 1 and p["doublings"] >= 2 and (v == 1 or w.rule2):
            seen[("doublings", 2, v)] += 1
        if p["batches"] >= 1 and 2 * len(w.entries) == CC.COVER_CHUNK0 and (v == 1 or w.rule2):
            seen[("fills_first_chunk", 0, v)] += 1                 # the replay ends where done + chunk == all rows, no doubling
            assert p["doublings"] == 0
    for key in [("priv", True), ("priv", False), ("by_bits", True), ("by_bits", False), ("batches", 1), ("batches", 3), ("doublings", 2),
                ("fills_first_chunk", 0)]:
        assert seen[key + (1,)] >= 1 and seen[key + (0,)] >= 1, (key, seen)


def test_chunk_lists_have_the_sizes_of_their_names():
    """the replay counts 2 rows an entry over the whole list: 256 entries fill the first chunk exactly, 257, 512 and 513 take one doubling,
    2,790 three; the 257 list with an entry removed is the invalid list that fills the first chunk exactly"""
    assert CC.COVER_CHUNK0 == 512
    seen = {}
    for good, bad in CC.twins():
        if good.family == "chunks":
            n = int(good.name.split("_")[1])
            assert len(good.entries) == n and len(bad.entries) == n - 1, (good, bad)
            for w in (good, bad):
                p = CC.path(w)
                assert not p["by_bits"] and p["batches"] == 1, w
                seen.setdefault(n, set()).add((2 * len(w.entries), p["doublings"], CC.verdict(w)))
    assert seen[256] == {(512, 0, 1), (510, 0, 0)} and seen[257] == {(514, 1, 1), (512, 0, 0)}, seen
    assert seen[512] == {(1024, 1, 1), (1022, 1, 0)} and seen[513] == {(1026, 1, 1), (1024, 1, 0)}, seen
    assert seen[2790] == {(5580, 3, 1), (5578, 3, 0)}, seen


def test_histogram_twins_carry_thousands_on_one_position():
    for good, bad in CC.twins():
        if good.family == "histogram":
            for w in (good, bad):
                load = Counter()
                for m, a, b in w.entries:
                    load[a] += m
                    load[b] += m
                assert max(load.values()) >= 4 * 2099, w
    assert {(len(g.entries) > 1000, CC.path(g)["priv"]) for g, _ in CC.twins() if g.family == "histogram"} == {(a, b) for a in (True, False) for b in (True, False)}


def test_long_windows_end_at_the_last_position():
    lens = set()
    for good, bad in CC.twins():
        if good.family == "long":
            assert max(max(a, b) for _, a, b in good.entries) == good.ln - good.rl and good.par.e1 == good.ln - 1, good
            lens.add((good.rl, good.ln))
    assert lens == {(rl, ln) for rl in (65, 100, 151, 160) for ln in (1088, 1089, CC.MAP_MAXOFF + rl)}


def test_packed_entries_round_trip():
    for w in CC.all_windows():
        packed = CC.pack(w.entries)
        assert packed.dtype == np.uint64 and CC.unpack(packed) == w.entries, w
    assert CC.unpack(CC.pack([(2 ** 31 - 1, 1024, 1)])) == [(2 ** 31 - 1, 1024, 1)]


def test_sources_split_is_a_partition():
    w = next(w for w in CC.singles() if w.name == "mixed_13")
    for nsrc in (1, 2, 3):
        for how in ("round", "one", "ends"):
            parts = CC.split_sources(w.entries, nsrc, how)
            assert len(parts) == nsrc and sorted(e for p in parts for e in p) == sorted(w.entries)
    assert [len(p) for p in CC.split_sources(w.entries, 3, "one")][:2] == [0, 0] and len(CC.split_sources(w.entries, 3, "ends")[1]) == 0


def test_end_to_end_leg_has_valid_and_invalid_windows():
    """the windows of test_gpu_cover's leg through vdjx_window_score: by the oracle's mapper and coverage test, at least one valid window
    of each length, and an invalid one"""
    from oracle import oracle
    pool, wins = CC.e2e_pool()
    ix = oracle.ReadIndex(pool)
    for ln, ws in wins:
        got = []
        for w in ws:
            pairs, starts = ix.quick_map(w)
            got.append((len(pairs), ix.coverage_is_valid(starts, len(w), CC.E2E_INS, **CC.E2E_PARAMS)))
        assert len(ws[0]) == ln and {v for _, v in got} == {0, 1} and all(n > 20 for n, _ in got), (ln, got)
