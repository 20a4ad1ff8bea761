"""Handmade pair lists for k_window_cover (vdjer_amd/csrc/vdjx_score.hip), the coverage validator behind vdjx_window_cover and
vdjx_window_score: coverage.c:10-130.  No GPU and no pool: a window here is a list of entries (multiplicity, pos1, pos2), as the kernel reads
them, and the oracle (vdjo_coverage_is_valid) gets the rows the reference's mapper would have sorted out of them.

A TWIN is two windows that differ in one thing and have the oracle's verdicts 1 and 0; each family of twins is built for one rule or one
path of the kernel (tests/test_cover_cpu.py holds the verdicts and the paths, tests/test_gpu_cover.py runs the kernel).  SINGLES are windows
without a twin (floor 0, the 70 windows of one call, cases the reference decides one way only).

What the rules leave no room for, found while placing the cases:
  * coverage.c:86-93 (the first in-range first at most eval_start + gap) never decides alone: at eval_start + gap the row `floor` before it
    lies below eval_start, which :96-100 refuses.  The twin stands at eval_start + gap - 1 against eval_start + gap, and eval_start + gap + 1
    is a single.
  * :116-120 asks for a first beyond eval_stop - rl, and firsts end at len - rl: a window with eval_stop >= len is never valid.  So rule 2
    never runs with an evaluation range of more than len - 1 positions (the fewest deltas per batch are 6, at len 1184: 3 are not
    reached), and `pos + delta > len + 1023` never decides (pos + delta <= eval_stop).  Those windows are here as invalid singles, next
    to their valid neighbours.
  * the replay's perm_stride = 1 branch needs 1,000,003 pairs in one window: not reached."""
import ctypes as C
import functools
import os
import re
from collections import namedtuple

import numpy as np

_HIP = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vdjer_amd", "csrc", "vdjx_score.hip")).read()
_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vdjx.h")).read()


def _define(name, text=_HIP):
    (v,) = re.findall(r"^#define %s (\d+)u?\b" % name, text, re.M)
    return int(v)


COV_WORDS = _define("COV_WORDS")
MAP_THREADS = _define("MAP_THREADS")
COVER_CHUNK0 = _define("COVER_CHUNK0")
MAP_MAXOFF = _define("MAP_MAXOFF")
MAX_READ_LEN = _define("VDJX_MAX_READ_LEN", _HDR)

Params = namedtuple("Params", "e0 e1 rs ms lo hi floor")
BASE = Params(52, 411, 35, 48, 175, 175, 1)


class Win:
    """one window: its geometry, its entries and what it is for"""

    def __init__(self, name, family, ln, rl, par, entries, rule2=False, want=None):
        self.name, self.family, self.ln, self.rl, self.par = name, family, ln, rl, par
        self.entries = [tuple(int(x) for x in e) for e in entries]
        self.rule2 = rule2                      # as the invalid member of a twin: rule 2 is what refuses it
        self.want = dict(want or {})            # the path it is meant to take: keys of path()
        check_window(self)

    @property
    def group(self):
        return (self.ln, self.rl, self.par)

    def __repr__(self):
        return "Win(%s, len %d, rl %d, %s, %d entries)" % (self.name, self.ln, self.rl, tuple(self.par), len(self.entries))


def check_window(w):
    """the limits the issue sets, and the ones that keep the kernel inside its arrays"""
    p = w.par
    assert 1 <= w.rl <= MAX_READ_LEN and w.rl < w.ln <= MAP_MAXOFF + w.rl, w.name
    assert 0 <= p.rs <= w.rl and p.ms >= 0 and p.lo <= p.hi and p.floor >= 0 and 1 <= p.e0 < p.e1 and p.e1 - p.e0 + 1 <= COV_WORDS, w.name
    assert all(m >= 1 and 1 <= a <= w.ln - w.rl and 1 <= b <= w.ln - w.rl for m, a, b in w.entries), w.name
    assert 2 * sum(m for m, _, _ in w.entries) < 2 ** 31, w.name


# ---- the packed form
def pack(entries) -> np.ndarray:
    out = np.zeros(len(entries), np.uint64)
    for i, (m, a, b) in enumerate(entries):
        out[i] = (m << 32) | (a << 16) | b
    return out


def unpack(packed):
    return [(int(v) >> 32, (int(v) >> 16) & 0xFFFF, int(v) & 0xFFFF) for v in packed]


# ---- the oracle
def rows(entries) -> np.ndarray:
    """what vdjo_quick_map hands to the coverage test: `mult` times (p1, p2) and (p2, p1), sorted by first, then second"""
    r = []
    for m, a, b in entries:
        r += [(a, b)] * m + [(b, a)] * m
    r.sort()
    return np.array(r, np.int32).reshape(-1, 2)


def oracle_verdict(w, par=None) -> int:
    from oracle import oracle
    p = par or w.par
    if p.floor == 0:
        return 1                                # assembler2_vdj.c:846: the test is not called
    st = np.ascontiguousarray(rows(w.entries))
    return int(oracle.lib().vdjo_coverage_is_valid(w.rl, w.ln, p.e0, p.e1, p.rs, p.lo, p.hi, p.floor, st.ctypes.data_as(C.c_void_p), st.shape[0], p.ms))


@functools.lru_cache(maxsize=None)
def _verdicts():
    return {w.name: oracle_verdict(w) for w in all_windows()}


def verdict(w) -> int:
    """the oracle's verdict, computed once for all windows"""
    return _verdicts()[w.name]


def rule1_alone(w) -> int:
    """the oracle with mate_span 0 and insert_low = insert_high = rl: no (pos, delta) is tested, the verdict is rule 1's"""
    return oracle_verdict(w, w.par._replace(ms=0, lo=w.rl, hi=w.rl))


# ---- the kernel's choice of path, from the parameters
def band(rl, p):
    return p.lo - rl - p.ms // 2, p.hi - rl + p.ms // 2


def path(w) -> dict:
    p, rl = w.par, w.rl
    clo, chi = band(rl, p)
    nd = chi - clo
    nrows = p.e1 - max(0, p.e0 - rl + 1)
    nwb = (nd + 2 * rl + 63) // 64
    by_bits = p.floor == 1 and 1 <= nd <= 64 and nrows >= 1 and nrows * nwb * 2 <= COV_WORDS
    db = COV_WORDS // (p.e1 - p.e0 + 1)
    tot, chunk, done, doublings = 2 * len(w.entries), COVER_CHUNK0, 0, 0
    while done + chunk < tot:                   # all of the list replayed: what an invalid or a just-valid window needs
        done += chunk
        chunk *= 2
        doublings += 1
    return dict(priv=(w.ln + 2) * (MAP_THREADS // 64) <= COV_WORDS, by_bits=by_bits, nd=nd, grid_words=nrows * nwb * 2, db=db,
                batches=0 if (by_bits or nd <= 0) else -(-nd // db), doublings=doublings)


def tested(w):
    """the (pos, delta) that mate_coverage_is_valid looks at (coverage.c:25-38), were no verdict to end its loop"""
    p = w.par
    clo, chi = band(w.rl, p)
    out, mate_low, pos = [], 0, p.e0
    while mate_low < p.e1 and pos < p.e1:
        mate_low = pos + clo
        mate_high = min(pos + chi, p.e1 + 1) if pos + chi > p.e1 else pos + chi
        out += [(pos, j - pos) for j in range(mate_low, mate_high)]
        pos += 1
    return out


def short_of_floor(w):
    """NOT the reference (that is the oracle alone): a helper to place cases and to show that an invalid member is refused by rule 2 at
    the (pos, delta) it was built for.  Where it and the oracle disagree, tests/test_cover_cpu.py fails.
    The tested (pos, delta) that fewer than `floor` rows cover, by counting: a row (f, s) covers iff f in (pos - rl, pos] and
    s in (pos + delta - rl, pos + delta], that is at the positions [max(f, s - delta), min(f, s - delta) + rl)"""
    rl, p = w.rl, w.par
    clo, chi = band(rl, p)
    t = np.array(tested(w), np.int64).reshape(-1, 2)
    if t.shape[0] == 0:
        return []
    mult = {}
    for m, a, b in w.entries:
        mult[(a, b)] = mult.get((a, b), 0) + m
        mult[(b, a)] = mult.get((b, a), 0) + m
    nd, npos = chi - clo, p.e1 - p.e0
    diff = np.zeros((nd, npos + 1), np.int64)
    if mult:
        uniq = sorted(mult)
        f = np.array([u[0] for u in uniq], np.int64)[:, None]
        s = np.array([u[1] for u in uniq], np.int64)[:, None]
        mm = np.broadcast_to(np.array([mult[u] for u in uniq], np.int64)[:, None], (len(uniq), nd))
        v = s - np.arange(clo, chi, dtype=np.int64)[None, :]
        lo = np.clip(np.maximum(f, v), p.e0, p.e1)
        hi = np.clip(np.minimum(f, v) + rl, p.e0, p.e1)
        ok = lo < hi
        col = np.broadcast_to(np.arange(nd)[None, :], lo.shape)
        np.add.at(diff, (col[ok], lo[ok] - p.e0), mm[ok])
        np.add.at(diff, (col[ok], hi[ok] - p.e0), -mm[ok])
    cov = np.cumsum(diff, axis=1)
    short = cov[t[:, 1] - clo, t[:, 0] - p.e0] < p.floor
    return [(int(a), int(b)) for a, b in t[short]]


# ---- builders
def spread(rl, p):
    """mate offsets with which reads at every gap-th position cover every delta of the band: one offset d serves the deltas
    [d - rs, d + rs] at every position (gap = rl - rs)"""
    clo, chi = band(rl, p)
    ds = [clo + p.rs]
    while ds[-1] + p.rs + 1 < chi:
        ds.append(min(ds[-1] + 2 * p.rs + 1, chi - p.rs - 1))
    return ds


def tiled(rl, ln, p, ds=None, step=None, mult=None, anchor=1, last=None, copies=1):
    """reads at anchor, anchor + step, ... with a mate at every offset of ds that fits the window (a read without one is paired with itself)"""
    step = step or (rl - p.rs)
    ds = spread(rl, p) if ds is None else ds
    mult = max(p.floor, 1) if mult is None else mult
    out = []
    for q in range(anchor, (last or ln - rl) + 1, step):
        mates = [q + d for d in ds if 1 <= q + d <= (last or ln - rl)] or [q]
        out += [(mult, q, s) for s in mates] * copies
    return out


def firsts(counts, far):
    """a list with the given first positions {pos: copies} below `far`: every one paired with `far`"""
    return [(m, q, far) for q, m in sorted(counts.items()) if m > 0]


def split_sources(entries, nsrc, how):
    """the list as `nsrc` parts: `round` deals the entries out, `one` gives everything to the last source, `ends` to the first and last"""
    parts = [[] for _ in range(nsrc)]
    for i, e in enumerate(entries):
        parts[{"round": i % nsrc, "one": nsrc - 1, "ends": 0 if i % 2 == 0 else nsrc - 1}[how]].append(e)
    return parts


TWINS, SINGLES = [], []


def twin(family, name, good, bad, rule2=False, want=None):
    """good and bad: (ln, rl, par, entries)"""
    a = Win(name + "+", family, *good, want=want)
    b = Win(name + "-", family, *bad, rule2=rule2, want=want)
    TWINS.append((a, b))


def single(family, name, ln, rl, par, entries, expect, want=None):
    w = Win(name, family, ln, rl, par, entries, want=want)
    w.expect = expect
    SINGLES.append(w)


NO_RULE2 = dict(ms=0, lo=50, hi=50)             # (rl 50) nd 0: nothing tested


def _floor0():
    for nm, ent in (("empty", []), ("one", [(1, 10, 20)]), ("step16", tiled(50, 600, BASE, step=16))):
        single("floor0", "floor0_" + nm, 600, 50, BASE._replace(floor=0), ent, 1)


def _tiny():
    """coverage.c:106-120 on lists of 0, 1 and 2 entries (rule 2 tests nothing)"""
    p = Params(13, 70, 35, 0, 50, 50, 1)        # gap 15, firsts up to 36 are walked, the last must lie beyond 20
    single("tiny", "tiny_empty", 120, 50, p, [], 0)
    twin("tiny", "tiny_1_last_beyond", (120, 50, p, [(1, 12, 21)]), (120, 50, p, [(1, 12, 20)]))          # > e1 - rl against ==
    twin("tiny", "tiny_1_index0", (120, 50, p, [(1, 3, 40)]), (120, 50, p, [(1, 40, 41)]))                # the walk ends at row 1 / at row 0: `i > 0`
    twin("tiny", "tiny_1_i_above_floor", (120, 50, p, [(1, 3, 40)]), (120, 50, p, [(2, 3, 40)]))          # i == floor: :111 not asked; i > floor: asked
    p2 = p._replace(e0=10)
    twin("tiny", "tiny_2_last_beyond", (120, 50, p2, [(1, 5, 12), (1, 12, 21)]), (120, 50, p2, [(1, 5, 12), (1, 12, 20)]))
    twin("tiny", "tiny_2_all_walked", (120, 50, p2, [(1, 5, 20), (1, 12, 35)]), (120, 50, p2, [(1, 5, 20), (1, 12, 36)]))      # clamp to the last row, :111 on it


def _rule1():
    """each sub-rule at its edge, rule 2 testing nothing.  rl 50, gap 15, firsts walked up to vmax = 377"""
    rl, ln, far = 50, 600, 540
    for fl in (1, 2, 3):
        p = BASE._replace(floor=fl, **NO_RULE2)
        base = {45 + 15 * k: fl for k in range(24)}          # 45, 60, ..., 390: the first row beyond vmax = 377 is 390's
        for how in ("mult", "distinct"):
            def lst(c):
                e = firsts(c, far)
                return e if how == "mult" else [(1, q, f) for m, q, f in e for _ in range(m)]
            tag = "rule1_f%d_%s_" % (fl, how)
            # :80-84 rows below e0: floor - 1 against floor
            twin("rule1", tag + "before_e0", (ln, rl, p, lst(base)), (ln, rl, p, lst({**base, 45: fl - 1})))
            # :96-100 consecutive firsts gap against gap + 1 apart, in the middle
            stretched = {(q if q < 200 else q + 1): m for q, m in base.items()}
            twin("rule1", tag + "gap", (ln, rl, p, lst(base)), (ln, rl, p, lst(stretched)))
            # ... and one copy short at one position: the row `floor` back is then two positions back
            twin("rule1", tag + "copies", (ln, rl, p, lst(base)), (ln, rl, p, lst({**base, 195: fl - 1})))
            # the stretched step around vmax: the step INTO the first row beyond vmax still counts (:111-113), the next one does not
            for k, nm in ((0, "at_vmax"), (1, "into_stop_row")):
                top = 377 + k
                c_bad = {top - 16 - 15 * j: fl for j in range(23)}
                c_bad.update({top: fl, top + 15: fl})
                c_good = {q + 1 if q < top else q: m for q, m in c_bad.items()}
                twin("rule1", tag + nm, (ln, rl, p, lst(c_good)), (ln, rl, p, lst(c_bad)))
            c = {378 - 15 * j: fl for j in range(23)}          # 378 is the first row beyond vmax; what follows is free
            twin("rule1", tag + "past_stop_row", (ln, rl, p, lst({**c, 420: fl})), (ln, rl, p, lst({**{q - 1: m for q, m in c.items()}, 393: fl, 420: fl})))
    # :86-93 the first in-range first: e0 + gap - 1 is the last that can be valid
    p = BASE._replace(**NO_RULE2)
    def first_at(v):
        return firsts({51: 1, **{v + 15 * k: 1 for k in range(24)}}, far)
    twin("rule1", "rule1_first_in_range", (ln, rl, p, first_at(66)), (ln, rl, p, first_at(67)))
    single("rule1", "rule1_first_in_range_plus1", ln, rl, p, first_at(68), 0)


def _histogram():
    """the first-position histogram: private per wave up to len 1022, shared atomics from 1023; thousands of increments on one position,
    from one entry and from many; the count decides (floor 2100: one copy short in the middle)"""
    rl, fl = 50, 2100
    for ln in (1022, 1023):
        p = Params(52, 120, 35, 0, rl, rl, fl)                # firsts walked up to 86, the last beyond 70
        far = ln - rl                                       # the histogram's top position
        base = {45: fl, 60: fl, 75: fl, 90: fl}
        for how in ("mult", "distinct"):
            def lst(c):
                e = firsts(c, far)
                return e if how == "mult" else [(1, q, f) for m, q, f in e for _ in range(m)]
            twin("histogram", "hist_%d_%s" % (ln, how), (ln, rl, p, lst(base)), (ln, rl, p, lst({**base, 60: fl - 1})), want=dict(priv=ln == 1022))


def _long():
    """windows of 1088 bases and more with reads over 64: hf[] up to len + 1.  Every first is walked (eval_stop = len - 1), so the entry
    count hf[len] places the last row, and the last row decides: at len - rl (beyond eval_stop - rl) or one lower"""
    for rl in (65, 100, 151, 160):
        for ln in sorted({1088, 1089, MAP_MAXOFF + rl}):
            for fl in (1, 2):
                # gap 15; deltas [90, 110), mates 90 on: a read's mate covers them at its own position and the next 14 or more
                p = Params(ln - 400, ln - 1, rl - 15, 20, rl + 100, rl + 100, fl)
                good = tiled(rl, ln, p, ds=[90], anchor=(ln - rl) % 15 or 15)
                bad = tiled(rl, ln, p, ds=[90], anchor=(ln - rl - 1) % 15 or 15, last=ln - rl - 1)
                assert max(a for _, a, _ in good) == ln - rl and max(b for _, _, b in good) == ln - rl
                twin("long", "long_rl%d_len%d_f%d" % (rl, ln, fl), (ln, rl, p, good), (ln, rl, p, bad), want=dict(priv=False, by_bits=fl == 1))


def _edge_lists(rl, ln, p, which):
    """reads at every gap-th position whose mates cover the band exactly / miss its first or last delta by one"""
    clo, chi = band(rl, p)
    if which == "low":
        return tiled(rl, ln, p, ds=[clo + p.rs]), tiled(rl, ln, p, ds=[clo + p.rs + 1])
    return tiled(rl, ln, p, ds=[chi - p.rs - 1]), tiled(rl, ln, p, ds=[chi - p.rs - 2])


def _forms():
    """bit grid against difference arrays: the band's width around 64, 1 and 0; the grid's size around COV_WORDS; the same at floor 2"""
    rl, ln = 50, 600
    for ms in (64, 65, 66):
        for fl in (1, 2):
            p = BASE._replace(ms=ms, floor=fl)
            nd = 2 * (ms // 2)
            for which in ("low", "high"):
                g, b = _edge_lists(rl, ln, p, which)
                twin("forms", "forms_ms%d_f%d_%s" % (ms, fl, which), (ln, rl, p, g), (ln, rl, p, b), rule2=True, want=dict(nd=nd, by_bits=fl == 1 and nd <= 64))
    for fl in (1, 2):
        p = BASE._replace(ms=1, lo=175, hi=176, floor=fl)                  # one delta: 125
        twin("forms", "forms_nd1_f%d_low" % fl, (ln, rl, p, tiled(rl, ln, p, ds=[160])), (ln, rl, p, tiled(rl, ln, p, ds=[161])), rule2=True, want=dict(nd=1, by_bits=fl == 1))
        twin("forms", "forms_nd1_f%d_high" % fl, (ln, rl, p, tiled(rl, ln, p, ds=[90])), (ln, rl, p, tiled(rl, ln, p, ds=[89])), rule2=True, want=dict(nd=1, by_bits=fl == 1))
        for ms in (0, 1):                                                 # no delta: rule 1's verdict, whatever the mates
            p = BASE._replace(ms=ms, floor=fl)
            twin("forms", "forms_nd0_ms%d_f%d" % (ms, fl), (ln, rl, p, tiled(rl, ln, p, ds=[300], step=15)), (ln, rl, p, tiled(rl, ln, p, ds=[300], step=16)), want=dict(nd=0, by_bits=False))
    # the grid's size: rows x words x 2 against COV_WORDS.  rl 100, 4 words a row: 1024 rows fill it exactly, 1025 go to the difference
    # arrays; rl 151, 5 words a row: 819 rows are the most that fit, 820 do not
    for rl, nrows, fit in ((100, 1024, True), (100, 1025, False), (151, 819, True), (151, 820, False)):
        ln = MAP_MAXOFF + rl
        e0 = rl + 20
        for fl in (1, 2):
            p = Params(e0, nrows + e0 - rl + 1, 60, 16, rl + 120, rl + 120, fl)     # deltas 112 .. 127; mates 67 on reach 127, mates 66 on do not
            g, b = _edge_lists(rl, ln, p, "high")
            twin("forms", "forms_grid_rl%d_%drows_f%d" % (rl, nrows, fl), (ln, rl, p, g), (ln, rl, p, b), rule2=True,
                 want=dict(by_bits=fit and fl == 1, grid_words=nrows * (4 if rl == 100 else 5) * 2))


def _smear():
    """one (pos, delta) tested (eval_stop = eval_start + clo, one delta), rule 1 met by reads paired with themselves, which cover nothing
    (clo >= rl); the only covering entry has its read and its mate at the ends of what counts, and at distances that are multiples of 64"""
    for rl in (36, 50, 64, 65, 128, 151):
        e0, clo = rl + 10, rl + 20
        e1 = e0 + clo
        ln = e1 + rl + 40
        for fl in (1, 2):
            p = Params(e0, e1, rl - 15, 0, rl + clo, rl + clo + 1, fl)
            fill = tiled(rl, ln, p, ds=[])
            def w(f, s):
                return (ln, rl, p, fill + [(fl, f, s)])
            tag = "smear_rl%d_f%d_" % (rl, fl)
            want = dict(nd=1, by_bits=fl == 1)
            twin("smear", tag + "read_first", w(e0 - rl + 1, e1), w(e0 - rl, e1), rule2=True, want=want)
            twin("smear", tag + "read_last", w(e0, e1 - rl + 1), w(e0 + 1, e1 - rl + 1), rule2=True, want=want)
            twin("smear", tag + "mate_first", w(e0, e1 - rl + 1), w(e0, e1 - rl), rule2=True, want=want)
            twin("smear", tag + "mate_last", w(e0 - rl + 1, e1), w(e0 - rl + 1, e1 + 1), rule2=True, want=want)
            for t in (64, 128):
                if t < rl:
                    twin("smear", tag + "t%d_mate_first" % t, w(e0 - t, e1 - rl + 1), w(e0 - t, e1 - rl), rule2=True, want=want)
                    twin("smear", tag + "t%d_mate_last" % t, w(e0 - t, e1), w(e0 - t, e1 + 1), rule2=True, want=want)


def _one_short(name, ln, rl, p, at, hole, want):
    """a twin whose invalid member is short at ONE tested (pos, delta) = (at, hole).  An entry (f, s) covers the square of positions
    f .. f + rl - 1 and mate positions j = pos + delta in s .. s + rl - 1.  Reads rl apart (read_span 0: that is the gap) split the
    positions into columns: below `at` the columns at - rl, at - 2 rl, ..., above it at + 1, at + 1 + rl, ..., each with mates rl apart
    over every j tested in it; at `at` itself a read whose mates end at j - 1 and begin at j + 1.  The valid member has (at, at + hole)"""
    clo, chi = band(rl, p)
    fl, top, j_short = p.floor, ln - rl, at + hole
    ent = []

    def column(f):
        s = f + clo
        while True:
            ent.append((fl, f, min(s, top)))
            if s >= top or s + rl - 1 >= f + rl + chi - 2:
                break
            s += rl

    for f in range(at - rl, 0, -rl):
        column(f)
    for f in range(at + 1, top + 1, rl):
        column(f)
    if hole > clo:
        for s in range(j_short - rl, at + clo - rl, -rl):
            ent.append((fl, at, s))
    for s in range(j_short + 1, at + chi, rl):
        ent.append((fl, at, s))
    ent.append((fl, top, top))                  # a last first beyond eval_stop - rl; paired with itself it covers nothing (clo > rl)
    twin("batches", name, (ln, rl, p, ent + [(fl, at, j_short)]), (ln, rl, p, ent), rule2=True, want=want)
    assert short_of_floor(TWINS[-1][1]) == [(at, hole)], (name, short_of_floor(TWINS[-1][1])[:6])


ONE_SHORT = {}       # name of the twin -> (the one (pos, delta) its invalid member leaves uncovered, the delta meant)


def _batches():
    """difference arrays in batches of 22, 8 and 6 deltas (an evaluation range of more than len - 1 positions is never valid: 3 are not
    reached); the one (pos, delta) short of the floor in the first, a middle and the last batch, at the first and the last delta of a batch,
    at a low and at a high position"""
    for rl, ln, e0, e1, db in ((50, 600, 52, 411, 22), (100, 1124, 52, 1051, 8), (160, 1184, 13, 1183, 6)):
        nd = 3 * db + 2                                            # 3 batches and a short one
        lo = 2 * rl + 40
        p = Params(e0, e1, 0, nd - (nd % 2), lo, lo + (nd % 2), 2)
        clo, chi = band(rl, p)
        assert chi - clo == nd and COV_WORDS // (e1 - e0 + 1) == db and clo > rl
        high = 5 + rl * ((min(e1 - chi, ln - rl - chi - 1) - 5) // rl)
        for b, nm in ((0, "first"), (1, "middle"), (3, "last")):
            for k, nm2 in ((0, "first_delta"), (db - 1, "last_delta")):
                hole = min(clo + b * db + k, chi - 1)              # (the last batch is short)
                for at, nm3 in ((5 + rl, "lowpos"), (high, "highpos")):
                    name = "batches_db%d_%s_%s_%s" % (db, nm, nm2, nm3)
                    _one_short(name, ln, rl, p, at, hole, dict(db=db, batches=4, by_bits=False))
                    ONE_SHORT[name] = ((at, hole), hole)


def _chunks():
    """lists of which every entry is needed: a read at EVERY position whose mate covers one (pos, delta) alone (one delta tested, the mate at
    its far end, the read at its far end), `floor` entries a position; whole, and with the first, a middle and the last entry removed.
    The list holds nothing else -- n entries are 2 n rows of the replay, which counts its chunks over all rows (in a scattered order: where
    an entry stands in the list plays no part), so 256 entries fill the first chunk of COVER_CHUNK0 = 512 rows exactly and 257 need a
    second.  Rule 1 is met by the same entries: reads at the consecutive positions 5 .. e1 - 75, mates at 80 .. e1, `floor` rows each
    (one fewer at one position in the invalid member: the row `floor` back is then still the position before)"""
    rl, rs, clo, e0 = 36, 21, 40, 40
    for n, fl in ((256, 2), (257, 2), (512, 2), (513, 2), (2790, 3)):
        npos = -(-n // fl)
        e1 = e0 + clo + npos - 1
        ln = e1 + rl + 4
        p = Params(e0, e1, rs, 0, rl + clo, rl + clo + 1, fl)
        assert e0 + clo <= e1 - clo - rl + 1 + (rl - rs)            # the mates' positions go on where the reads' end: no step above the gap
        need = []
        for k in range(npos):
            pos = e0 + k
            here = fl if k < npos - 1 else n - fl * (npos - 1)                 # the last position takes the rest: fewer entries, the same sum
            need += [(fl - here + 1 if i == 0 else 1, pos - rl + 1, pos + clo) for i in range(here)]
        assert len(need) == n
        for cut, nm in ((0, "first"), (n // 2, "middle"), (n - 1, "last")):
            twin("chunks", "chunks_%d_%s" % (n, nm), (ln, rl, p, need), (ln, rl, p, need[:cut] + need[cut + 1:]), rule2=True,
                 want=dict(by_bits=False, batches=1))


def _bounds():
    """pos + delta outside the reference's array (coverage.c:46: j < 0 or j > len + 1023 is invalid); eval_stop beyond the window"""
    rl, ln = 50, 600
    for fl in (1, 2):
        # deltas -10 .. 29, mates at the reads' own positions: eval_start 11 tests j = 1 first, eval_start 9 tests j = -1
        p = Params(11, 411, 35, 40, 60, 60, fl)
        ent = tiled(rl, ln, p, ds=[0])
        twin("bounds", "bounds_negative_f%d" % fl, (ln, rl, p, ent), (ln, rl, p._replace(e0=9), ent), rule2=True, want=dict(by_bits=fl == 1))
        # eval_stop: len - 1 is the last that can be valid; len, and len + 1030 (where pos + delta would pass len + 1023), are not
        p = BASE._replace(e1=ln - 1, ms=30, floor=fl)               # deltas 110 .. 139
        ent = tiled(rl, ln, p, ds=[105], anchor=10)                 # 10, 25, ..., 550: the mate at 550 serves the last tested positions
        twin("bounds", "bounds_e1_len_f%d" % fl, (ln, rl, p, ent), (ln, rl, p._replace(e1=ln), ent))
        single("bounds", "bounds_e1_far_f%d" % fl, ln, rl, p._replace(e1=ln + 1030), ent, 0)


def _clamp():
    """mate_high stops at eval_stop + 1 (coverage.c:36-38) and the last evaluated position tests j = eval_stop alone (:25): no mate
    reaches beyond eval_stop = 411; with eval_stop 412 the same list is one base short"""
    rl, ln = 50, 600
    for fl in (1, 2):
        p = Params(52, 411, 35, 30, 170, 170, fl)                  # deltas 105 .. 134, mates 105 on
        ent = tiled(rl, ln, p, ds=[105], anchor=362 % 15, last=362)     # reads and mates up to eval_stop - rl + 1: they end at eval_stop
        ent += [(fl, 377, 377), (fl, 392, 392)]                     # firsts for rule 1 under either eval_stop; no tested position sees them
        twin("clamp", "clamp_f%d" % fl, (ln, rl, p, ent), (ln, rl, p._replace(e1=412), ent), rule2=True, want=dict(by_bits=fl == 1))


def _inserts():
    """insert_low < insert_high: the same list under (150, 200) and under (100, 250)"""
    rl, ln = 50, 600
    for fl in (1, 2):
        p = BASE._replace(lo=150, hi=200, floor=fl)                # deltas 76 .. 173: two mates a read
        ent = tiled(rl, ln, p)
        twin("inserts", "inserts_f%d" % fl, (ln, rl, p, ent), (ln, rl, p._replace(lo=100, hi=250), ent), rule2=True, want=dict(by_bits=False))
    p = BASE._replace(lo=165, hi=185, ms=40)                       # 60 deltas: the grid
    ent = tiled(rl, ln, p)
    twin("inserts", "inserts_grid", (ln, rl, p, ent), (ln, rl, p._replace(lo=164), ent), rule2=True, want=dict(by_bits=True))


def _issue_examples():
    """the examples of the issue's text, on reads at every step-th position with mates 125 on"""
    rl, ln = 50, 600
    def t(step, mult=1):
        return tiled(rl, ln, BASE, ds=[125], step=step, mult=mult)
    twin("examples", "ex_step", (ln, rl, BASE, t(15)), (ln, rl, BASE, t(16)))
    p2 = BASE._replace(floor=2)
    twin("examples", "ex_multiplicity", (ln, rl, p2, t(14, 2)), (ln, rl, p2, t(14, 1)))
    twin("examples", "ex_mate_span", (ln, rl, BASE._replace(ms=71), t(15)), (ln, rl, BASE._replace(ms=72), t(15)), rule2=True, want=dict(by_bits=False))
    hole10 = [e for e in tiled(rl, ln, BASE, ds=[125], step=5) if not 201 <= e[1] <= 210 and not 201 <= e[2] <= 210]
    hole30 = [e for e in tiled(rl, ln, BASE, ds=[125], step=5) if not 201 <= e[1] <= 230 and not 201 <= e[2] <= 230]
    twin("examples", "ex_hole", (ln, rl, BASE, hole10), (ln, rl, BASE, hole30))


def _mixed():
    """70 windows of one geometry for one call: sizes from 0 to some hundred entries, valid and invalid"""
    rl, ln = 50, 600
    for i in range(70):
        if i % 9 == 0:
            ent = []
        else:
            ent = tiled(rl, ln, BASE, ds=[120 + i % 11], step=11 + i % 6, copies=1 + (i % 7) * (i % 5))
            if i % 4 == 1:
                ent = ent[: len(ent) // 2]
        single("mixed", "mixed_%02d" % i, ln, rl, BASE, ent, None)


@functools.lru_cache(maxsize=None)
def _built():
    assert not TWINS and not SINGLES
    for f in (_floor0, _tiny, _rule1, _histogram, _long, _forms, _smear, _batches, _chunks, _bounds, _clamp, _inserts, _issue_examples, _mixed):
        f()
    names = [w.name for t in TWINS for w in t] + [w.name for w in SINGLES]
    assert len(names) == len(set(names))
    return True


def all_windows():
    _built()
    return [w for t in TWINS for w in t] + list(SINGLES)


def twins():
    _built()
    return list(TWINS)


def singles():
    _built()
    return list(SINGLES)


def groups():
    """(len, rl, params) -> its windows, in order"""
    out = {}
    for w in all_windows():
        out.setdefault(w.group, []).append(w)
    return out


# ---- the end-to-end leg: reads of 151 bases tiled over one transcript
E2E_RL, E2E_LENS = 151, (1088, 1089, 1175)
E2E_PARAMS = dict(e0=160, e1=1000, rs=136, ms=20, floor=1)          # gap 15
E2E_INS = 251                                                   # mates 100 on: deltas 90 .. 109


@functools.lru_cache(maxsize=None)
def e2e_pool():
    """-> (pool, windows): one random transcript of 1,400 bases; a pair at every 15th position up to 900 (read 1 as it stands, read 2 the
    reverse complement of the transcript 100 bases on).  Windows that start at 0 and 7 see the tiling through their evaluation range, the
    ones that start at 200 see it end before"""
    from vdjer_amd import synth
    rng = np.random.default_rng(20240611)
    t = "".join(rng.choice(list("ACGT"), 1400))
    rl = E2E_RL
    qs = list(range(0, 901, 15))
    base = synth.make_reads(synth.make_repertoire(1, seed=5), len(qs), noise_frac=0.0, seed=6, rl=rl, ins_mean=rl + 40.0, err=0.0, n_rate=0.0)
    recs = base.primary.copy()
    assert base.secondary.shape[0] == 0 and recs.shape[0] == 4 * len(qs)
    for j in range(0, recs.shape[0], 4):                         # a pair's records: read 1, its reverse complement, read 2, its reverse complement
        q = qs[int(base.pair_id[j])]
        r1, r2 = t[q:q + rl], synth.revcomp(t[q + 100:q + 100 + rl])
        for k, s in enumerate((r1, synth.revcomp(r1), r2, synth.revcomp(r2))):
            assert int(base.pair_id[j + k]) == int(base.pair_id[j]) and int(base.read_num[j + k]) == 1 + k // 2 and int(base.is_rc[j + k]) == k % 2
            recs[j + k, 1:1 + rl] = np.frombuffer(s.encode(), np.uint8)
    pool = synth.ReadPool(rl, recs, base.secondary.copy(), base.pair_id.copy(), base.read_num.copy(), base.is_rc.copy(), base.reg_rank.copy(), base.n_pairs)
    wins = [(ln, [t[s:s + ln] for s in (0, 7, 200)]) for ln in E2E_LENS]
    return pool, wins
