"""Handmade pools for the read index (vdjx_read_index_build, vdjer_amd/csrc/vdjx_rindex.hip) and a plain model of what it folds, shared by
tests/test_rindex_cpu.py (which proves without a GPU that every case reaches what it is for) and tests/test_gpu_rindex.py.

A pool is a small synth.make_reads pool (n_rate 0) whose first pairs -- in registration order, which falls on both of its runs, primary and
secondary -- are overwritten.  A pair is four consecutive records: read 1, its reverse complement, read 2, its reverse complement.  A "class
of m" is m pairs whose read 1 is w[a:a+rl] of a window w at an offset a where no other record of the pool reads that sequence; a mapping
read 2 is revcomp(w[b:b+rl]), a filler read 2 a seeded random string.  (The reverse complements of the m read 1s are a class of m of their
own: every planted class has a twin that the reverse complement of the window hits.)

The model is plain Python over the records: per read sequence its read-1 members in registration order, each with the key (sequence of the
pair's read-2 record A, of B, flags) of its entry; fold() turns a class's keys into the weighted entries the device writes, route by route;
window() evaluates the entries of the classes along a string the way quick_map3.c:188-266 pairs reads.  Everything is seeded and computed
once per process."""
from __future__ import annotations

import dataclasses
import functools
from collections import Counter

import numpy as np

from vdjer_amd import synth

# what vdjx_rindex.hip and vdjx_common.h define (tests/test_rindex_cpu.py reads them out of the sources and compares)
FOLD_SMALL, FOLD_WAVE, FOLD_SLOTS, BIG_SLOTS, BIG_THREADS, FM_PER, MAXCNT = 8, 256, 512, 8192, 512, 1024, 255
BIG_FULL = BIG_SLOTS * 3 // 4                   # more distinct entries than this: the rest of the class leaves unfolded
BIG_GRID = 2048                                 # k_ri_fold_big's workgroups at most
RC, RCA, RCB = 2, 4, 8                          # flags of an entry: is_rc of the read-1 record, of the read-2 records A and B
MIN_INSERT, MAX_INSERT = 50, 400                # quick_map3.c:23-24
WRONG = ("saturate", "drop_second", "lose_unfolded", "no_wave", "first_block")          # the wrong folds of fold()
WLEN = 486


def pieces(n):
    """a multiplicity in pieces of at most MAXCNT (the field has 8 bits)"""
    return [MAXCNT] * (n // MAXCNT) + ([n % MAXCNT] if n % MAXCNT else [])


def fold(keys, wrong=None):
    """[(key, multiplicity)]: the weighted entries of a class whose members hold `keys` in CSR (registration) order.  wrong: one of WRONG,
    a fold gone wrong in that way (the sensitivity checks of tests/test_rindex_cpu.py)"""
    m = len(keys)
    unfolded = []
    if m <= FOLD_SMALL:                          # a thread per member: no piece can pass 8
        return list(Counter(keys).items())
    if m <= FOLD_WAVE:                           # one wave, a table that cannot fill
        if wrong == "no_wave":
            return []
        folded = Counter(keys)
    else:                                        # k_ri_fold_big: rows of BIG_THREADS members, the fill of the table read once per row
        folded = Counter()
        rows = keys[:BIG_THREADS] if wrong == "first_block" else keys
        for at in range(0, len(rows), BIG_THREADS):
            if len(folded) > BIG_FULL:
                unfolded += rows[at:at + BIG_THREADS]
            else:
                folded.update(rows[at:at + BIG_THREADS])
        if wrong == "lose_unfolded":
            unfolded = []
    out = [(k, 1) for k in unfolded]
    for k, n in folded.items():
        ps = pieces(n)
        if wrong == "saturate":
            ps = ps[:1]
        if wrong == "drop_second":
            ps = ps[:1] + ps[2:]
        out += [(k, x) for x in ps]
    return out


def route(members):
    """which way a class of `members` is folded"""
    return "small" if members <= FOLD_SMALL else "wave" if members <= FOLD_WAVE else "giant"


class Model:
    """the read index of a pool, in plain Python"""

    def __init__(self, pool):
        rl = self.rl = pool.rl
        recs = np.concatenate([pool.primary, pool.secondary])
        self.seq = [row.tobytes().decode() for row in recs[:, 1:1 + rl]]
        R = len(self.seq)
        pid, rnum, isrc, reg = (x.tolist() for x in (pool.pair_id, pool.read_num, pool.is_rc, pool.reg_rank))
        r2 = {}
        for r in range(R):
            if rnum[r] == 2:
                r2.setdefault(pid[r], []).append((reg[r], r))
        for v in r2.values():
            v.sort()
            assert len(v) <= 2
        rows = {}
        for r in range(R):
            if rnum[r] == 1 and "N" not in self.seq[r] and pid[r] < pool.n_pairs:
                ab = [x[1] for x in r2.get(pid[r], [])] + [None, None]
                sa, sb = (None if x is None or "N" in self.seq[x] else self.seq[x] for x in ab[:2])
                fl = (RC if isrc[r] else 0) | (RCA if sa is not None and isrc[ab[0]] else 0) | (RCB if sb is not None and isrc[ab[1]] else 0)
                rows.setdefault(self.seq[r], []).append((reg[r], r, (sa, sb, fl)))
        self.keys = {s: [x[2] for x in sorted(v)] for s, v in rows.items()}          # class -> the keys of its members in CSR order
        self.r1_members = sum(len(v) for v in self.keys.values())
        clean = {s for s in self.seq if "N" not in s}
        self.classes_general = len(clean)
        self.classes_couples = 2 * len({min(s, synth.revcomp(s)) for s in clean})     # a key's sequence and its reverse complement
        self.couples = R % 2 == 0 and all(self.seq[r + 1] == synth.revcomp(self.seq[r]) for r in range(0, R, 2))
        descents = sum(reg[r] < reg[r - 1] for r in range(1, R))
        self.rank_order = min(descents, 2)          # 0 as recorded, 1 two runs (a merge), 2 a sort by rank
        self.n1_first_run = None
        if descents == 1:                           # the read-1 members before the record at which the second run starts (k_ri_split's n1p)
            cut = next(r for r in range(1, R) if reg[r] < reg[r - 1])
            self.n1_first_run = sum(rnum[r] == 1 and "N" not in self.seq[r] for r in range(cut))
        self._folded = {}

    def folded(self, s, wrong=None):
        if (s, wrong) not in self._folded:
            self._folded[(s, wrong)] = fold(self.keys[s], wrong)
        return self._folded[(s, wrong)]

    def entries(self, wrong=None):
        """read_index_r1_distinct: the weighted entries of all classes"""
        return sum(len(self.folded(s, wrong)) for s in self.keys)

    def entries_folded_minimum(self):
        """... if no class overflowed: sum of ceil(multiplicity / 255)"""
        return sum(len(pieces(n)) for ks in self.keys.values() for n in Counter(ks).values())

    def window(self, w, wrong=None):
        """(entries that map, pairs, {(pos1, pos2): pairs}) of a string: the entries of the class at every offset but the last
        (quick_map3.c:200) against the last offset at which either read-2 sequence of the entry occurs (on a tie the record registered
        last: B)"""
        rl = self.rl
        last = {}
        for i in range(len(w) - rl):
            last[w[i:i + rl]] = i + 1
        ent = pairs = 0
        at = Counter()
        for i in range(len(w) - rl):
            s = w[i:i + rl]
            if s not in self.keys:
                continue
            for (sa, sb, fl), mult in self.folded(s, wrong):
                la, lb = last.get(sa, 0) if sa else 0, last.get(sb, 0) if sb else 0
                if not (la or lb):
                    continue
                which = 1 if lb and lb >= la else 0
                best = lb if which else la
                if bool(fl & RC) == bool(fl & (RCB if which else RCA)):
                    continue
                if not MIN_INSERT <= abs(i + 1 - best) + rl <= MAX_INSERT:
                    continue
                ent += 1
                pairs += mult
                at[(i + 1, best)] += mult
        return ent, pairs, at


@dataclasses.dataclass(eq=False)
class Case:
    name: str
    what: str                  # the edge the case is for
    rl: int
    pool: synth.ReadPool
    wins: list                 # the strings (all WLEN long) that are scored and mapped
    planted: dict              # (index into wins, pos1, pos2) -> pairs planted there
    classes: list              # [dict(seq, members, distinct, what)]: the planted classes and what the CPU test holds them to
    verdicts: tuple = (0, 1)   # the coverage verdicts its windows must show (a pool without base reads covers no window)

    @functools.cached_property
    def model(self):
        return Model(self.pool)


@functools.lru_cache(maxsize=None)
def _rep():
    rep = synth.make_repertoire(6, seed=191)
    wins = rep.windows()
    assert all(w and len(w) == WLEN for w in wins)
    return rep, wins


class _Plant:
    """a make_reads pool whose first `room` pairs (in registration order) are given to the case: random pairs until they are planted"""

    def __init__(self, rl, n_pairs, room, noise=0.25, seed=192, shallow_first=True):
        self.rl = rl
        self.rep, wins = _rep()
        self.wins = list(wins)
        base = self.base = synth.make_reads(self.rep, n_pairs, noise_frac=noise, seed=seed, rl=rl, n_rate=0)
        self.n_primary = base.primary.shape[0]
        self.recs = np.concatenate([base.primary, base.secondary])
        self.pair_id = base.pair_id.copy()
        self.n_pairs = n_pairs
        self.first = [0] * n_pairs                                  # a pair's first record
        for j in range(0, self.recs.shape[0], 4):
            self.first[int(base.pair_id[j])] = j
        self.rng = np.random.default_rng(seed + 1000 + rl)
        self.room = room
        self.next = 0
        for _ in range(room):
            self.put(self.filler(), self.filler())
        self.next = 0
        self.taken = {row.tobytes().decode() for row in self.recs[:, 1:1 + rl]}
        self.planted = Counter()
        self.classes = []
        self.rc_of = []                                             # windows whose reverse complement is scored too
        self.noff = WLEN - rl
        nw = len(self.wins)
        order = list(range(nw - 1, -1, -1)) if shallow_first else list(range(nw))      # (clone 0 is the deepest: its offsets are nearly all read)
        # shallow first: the sites go round the windows; else window 0 is tiled offset by offset before the next one
        self._scan = ((wi, a) for a in range(2, self.noff - 1, 3) for wi in order[:-1]) if shallow_first else ((wi, a) for wi in order for a in range(2, self.noff - 1))

    def filler(self):
        return "".join("ACGT"[int(x)] for x in self.rng.integers(0, 4, self.rl))

    def put(self, r1, r2):
        """the next pair of the room: read 1, its reverse complement, read 2, its reverse complement"""
        assert self.next < self.room
        j = self.first[self.next]
        for q, s in enumerate((r1, synth.revcomp(r1), r2, synth.revcomp(r2))):
            self.recs[j + q, 1:1 + self.rl] = np.frombuffer(s.encode(), np.uint8)
        self.next += 1
        return j

    def add_window(self, w):
        assert len(w) == WLEN
        self.wins.append(w)
        return len(self.wins) - 1

    def site(self, wi=None, a=None):
        """(window, offset a): no record of the pool reads w[a:a+rl] or its reverse complement, and no earlier site does"""
        while True:
            if wi is None or a is None:
                w_, a_ = next(self._scan)
            else:
                w_, a_ = wi, a
            s = self.wins[w_][a_:a_ + self.rl]
            if s in self.taken or synth.revcomp(s) in self.taken or s == synth.revcomp(s):
                assert wi is None, "the given site is read by the base pool"
                continue
            self.taken.update((s, synth.revcomp(s)))
            return w_, a_

    def targets(self, wi, a, n):
        """n offsets b whose read w[b:b+rl] occurs once in the window and pairs with a read at a (the insert within 50 .. 400)"""
        w, out = self.wins[wi], []
        for d in (125, 100, 75, 150, 60, 90, 110, 135, 85, 140):
            b = a + d if a + d <= self.noff - 1 else a - d
            t = w[b:b + self.rl] if b >= 0 else ""
            if b >= 0 and w.find(t) == b and w.rfind(t) == b and MIN_INSERT <= d + self.rl <= MAX_INSERT:
                out.append(b)
            if len(out) == n:
                return out
        raise AssertionError((wi, a, n))

    def plant(self, rows, what, n_targets=None, wi=None, a=None, r1=None):
        """a class: rows[i] >= 0 -- the pair's read 2 maps at target rows[i] of the site --, -1 a filler read 2, a string: that read 2.
        In this order (= registration order)"""
        wi, a = self.site(wi, a) if r1 is None else (wi, a)
        w = self.wins[wi]
        seq = w[a:a + self.rl] if r1 is None else r1
        nt = n_targets if n_targets is not None else 1 + max([x for x in rows if isinstance(x, int)] + [-1])
        tg = self.targets(wi, a, nt) if nt else []
        keys = set()
        for x in rows:
            if isinstance(x, str):
                r2 = x
            elif x < 0:
                r2 = self.filler()
            else:
                r2 = synth.revcomp(w[tg[x]:tg[x] + self.rl])
                self.planted[(wi, a + 1, tg[x] + 1)] += 1
            keys.add(r2)
            self.put(seq, r2)
        if wi not in self.rc_of and wi < 6:
            self.rc_of.append(wi)
        self.classes.append(dict(seq=seq, members=len(rows), distinct=len(keys), what=what, window=wi, a=a, targets=tg))
        return tg

    def shuffled(self, counts, fillers=0):
        rows = [k for k, n in enumerate(counts) for _ in range(n)] + [-1] * fillers
        return [rows[i] for i in self.rng.permutation(len(rows))]

    def pool(self, extra_pairs=0):
        b = self.base
        return synth.ReadPool(self.rl, self.recs[:self.n_primary].copy(), self.recs[self.n_primary:].copy(), self.pair_id.copy(), b.read_num.copy(),
                              b.is_rc.copy(), b.reg_rank.copy(), self.n_pairs + extra_pairs)

    def case(self, name, what, verdicts=(0, 1), extra_pairs=0, rc_windows=2):
        assert self.next <= self.room
        wins = self.wins + [synth.revcomp(self.wins[i]) for i in self.rc_of[:rc_windows]] + [self.filler_window()]
        return Case(name, what, self.rl, self.pool(extra_pairs), wins, dict(self.planted), self.classes, verdicts)

    def filler_window(self):
        return "".join("ACGT"[int(x)] for x in self.rng.integers(0, 4, WLEN))        # nothing maps to it


def _shares(m):
    """a class of m: three mapping read 2s in unequal shares (about 1/2, 1/3, 1/6) and a few fillers"""
    fillers = 0 if m < 7 else 1 if m < 16 else 3
    rest = m - fillers
    c = rest // 6
    b = rest // 3 if rest > 2 else rest // 2
    return [n for n in (rest - b - c, b, c) if n], fillers


SIZES = (1, 2, 7, 8, 9, 10, 63, 64, 65, 255, 256, 257, 258, 511, 512, 513, 1025)


def _sizes(rl):
    p = _Plant(rl, 8000, sum(SIZES))
    for m in SIZES:
        sh, f = _shares(m)
        p.plant(p.shuffled(sh, f), f"class of {m}: {route(m)} route")
    return p.case("sizes", "classes on both sides of 8 and of 256, of the wave's rows of 64 and of k_ri_fold_big's rows of 512")


PIECES = (254, 255, 256, 509, 510, 511, 766)


def _pieces(rl):
    giants = ([766, 509, 254], 3), ([511, 256], 0), ([510, 255], 45)
    waves = ([254], 2), ([255], 0), ([256], 0), ([100, 100], 0)
    smalls = ([8], 0), ([1, 1, 1], 5)
    p = _Plant(rl, 8000, sum(sum(c) + f for c, f in giants + waves + smalls))
    for c, f in giants + waves + smalls:
        m = sum(c) + f
        p.plant(p.shuffled(c, f), f"{route(m)} route, class of {m}: entries repeated {c} times, {f} others")
    return p.case("pieces", "multiplicities of 254 ... 766 in 1 ... 4 pieces of at most 255, on every route that has them; 8 equal and 8 distinct members on the small one")


def _nines(rl, with_giants=False):
    """classes of exactly 9 members and nothing else as read 1 (no base reads): however the classes are numbered, every 1,024 members hold
    113 or 114 class starts -- s_big[] at its limit"""
    if with_giants:
        sizes = [9, 257] * 10
        p = _Plant(rl, sum(sizes), sum(sizes), noise=0.0, shallow_first=False)
        for m in sizes:
            sh, f = _shares(m)
            p.plant(p.shuffled(sh, f), f"class of {m}: {route(m)} route")
        return p.case("nines_257", "classes of 9 and of 257 in turns: the starts of wave and giant classes share workgroups of k_ri_fold_members", verdicts=(0,))
    p = _Plant(rl, 4500, 4500, noise=0.0, shallow_first=False)
    for _ in range(500):
        p.plant(p.shuffled([5, 3], 1), "class of 9: wave route")
    return p.case("nines", "500 classes of 9 (and their 500 twins), no other read 1: 113 or 114 starts of wave classes per workgroup of k_ri_fold_members")


OVERFLOW_MAPPED = (600, 255, 256)


def _overflow(rl, variant):
    m = list(OVERFLOW_MAPPED)
    mapped = [k for k, n in enumerate(m) for _ in range(n)]
    if variant == "tail":          # the table passes BIG_FULL distinct entries before the mapping rows arrive: they leave unfolded
        rows, n, what = [-1] * 6700 + mapped, 12000, "6,700 distinct fillers, then 600 + 255 + 256 mapping pairs: the mapping rows leave unfolded"
    elif variant == "head":        # the mapping rows are folded, the last fillers -- and 40 more pairs of the first mapping read 2 -- leave unfolded
        rows, n, what = mapped + [-1] * 6700 + [0] * 40, 12000, "the mapping pairs first (folded), the fillers after, 40 more mapping pairs last (unfolded)"
    elif variant == "at_6144":     # exactly BIG_FULL distinct entries: `full` is never taken
        rows, n, what = [0] + [-1] * (BIG_FULL - 1) + [0] * 812, 9000, "6,144 distinct entries at a multiple of 512 rows, 812 repeats after: nothing leaves unfolded"
    else:                          # one more: the row after the one that made it 6,145 leaves unfolded
        rows, n, what = [0] + [-1] * BIG_FULL + [0] * 811, 9000, "6,145 distinct entries one row of 512 later: the last 300 repeats leave unfolded"
    p = _Plant(rl, n, len(rows))
    p.plant(rows, "giant route with overflow: " + what, n_targets=3)
    return p.case("overflow_" + variant, what)


def _giants(rl, below):
    """no base reads: the read-1 members are three classes of 257 and their twins, n1 = 6 * 257 and k_ri_fold_big gets n1 / 257 + 1 = 7
    workgroups for 6 giant classes; `below`: a class of 128 and its twin more, n1 = 7 * 257 - 1, still 7 workgroups.  (A second turn of a
    workgroup -- `b += gridDim.x` -- needs more than BIG_GRID = 2,048 giant classes, 526,593 read-1 members: tests/test_rindex_cpu.py)"""
    sizes = [257, 257, 257] + ([128] if below else [])
    p = _Plant(rl, sum(sizes), sum(sizes), noise=0.0, shallow_first=False)
    for m in sizes:
        sh, f = _shares(m)
        p.plant(p.shuffled(sh, f), f"class of {m}: {route(m)} route")
    return p.case("giants_below" if below else "giants", "as many giant classes as k_ri_fold_big has workgroups, less one" + (", n1 just below a multiple of 257" if below else ""),
                  verdicts=(0,))


def _palindromic(rng, rl):
    half = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, rl // 2))
    return half + synth.revcomp(half)


def _palindrome(rl):
    assert rl % 2 == 0
    p = _Plant(rl, 3000, 170)
    pal = _palindromic(p.rng, rl)
    w = p.filler_window()
    wi = p.add_window(w[:100] + pal + w[100 + rl:])
    # 150 pairs: both records of read 1 are members of the one class (300: giant), half of them with the flag RC
    p.plant(p.shuffled([100, 47], 3), "a read 1 that is its own reverse complement, 150 pairs = 300 members: giant route", wi=wi, a=100, r1=pal)
    # ... and the same read as read 2 (both read-2 records of the pair are equal: A = B)
    p.classes[-1].update(members=300, distinct=10)                   # (every read 2 once with the flag RC and once without)
    p.plant([pal] * 20, "read 2 is its own reverse complement: the pair's read-2 records are of one class", wi=wi, a=300)
    p.planted[(wi, 301, 101)] += 20
    c = p.case("palindrome", "a read that is its own reverse complement as read 1 (one class of both records under the couples build too) and as read 2")
    c.wins.insert(-1, synth.revcomp(c.wins[wi]))
    return c


def _read2_shapes(rl):
    assert rl % 2 == 0
    p = _Plant(rl, 3000, 60)
    first = p.next
    p.plant([0] * 12, "pairs with one read-2 record, the reverse complement (B = none): map in the window")
    p.plant([0] * 11, "pairs with one read-2 record, the read as it is (B = none): map in the window's reverse complement")
    pal = _palindromic(p.rng, rl)
    w = p.filler_window()
    wi = p.add_window(w[:150] + pal + w[150 + rl:])
    p.plant([pal] * 10, "pairs whose two read-2 records are equal", wi=wi, a=40)
    p.planted[(wi, 41, 151)] += 10
    # a read 2 holding an N is in no class: the entry's mate classes are none, the pair never maps; five clean pairs of the class do
    at = p.next
    wi4, a4 = p.site()
    tg = p.plant([0] * 15, "ten of fifteen pairs with an N in read 2: left out of the table, their class reads as none", wi=wi4, a=a4, r1=p.wins[wi4][a4:a4 + rl])
    for k in range(10):
        j = p.first[at + k]
        p.recs[j + 2, 1 + 7 + k] = ord("N")
        p.recs[j + 3, rl - 7 - k] = ord("N")
    p.planted[(wi4, a4 + 1, tg[0] + 1)] -= 10
    p.classes[-1]["distinct"] = 2                                     # (the mapping read 2; none, none)
    # a read 1 holding an N is never a member
    at = p.next
    wi5, a5 = p.site()
    p.plant([0] * 6, "pairs with an N in read 1: never members", wi=wi5, a=a5, r1=p.wins[wi5][a5:a5 + rl])
    for k in range(6):
        j = p.first[at + k]
        p.recs[j, 1 + 3 + k] = ord("N")
        p.recs[j + 1, rl - 3 - k] = ord("N")
    del p.planted[(wi5, a5 + 1, p.classes[-1]["targets"][0] + 1)]
    p.classes[-1]["members"] = 0
    # one read-2 record of a pair goes to a pair of its own (a pair id past the pool's), which has no read 1
    extra = 0
    for k in range(12):
        p.pair_id[p.first[first + k] + 2] = p.n_pairs + extra
        extra += 1
    for k in range(11):
        p.pair_id[p.first[first + 12 + k] + 3] = p.n_pairs + extra
        extra += 1
    c0 = p.classes[1]
    del p.planted[(c0["window"], c0["a"] + 1, c0["targets"][0] + 1)]           # (these map in the reverse complement of the window only)
    return p.case("read2_shapes", "pairs with one read-2 record, with two equal ones, with an N in read 2 or in read 1", extra_pairs=extra, rc_windows=6)


def _relaid(c, name, what, pri, sec):
    """the records pri then sec of c's pool: a layout of its own with every record's pair, read number, orientation and rank"""
    pool = c.pool
    recs = np.concatenate([pool.primary, pool.secondary])
    idx = np.concatenate([pri, sec]).astype(np.int64)
    assert sorted(idx.tolist()) == list(range(recs.shape[0]))
    new = synth.ReadPool(pool.rl, recs[pri].copy(), recs[sec].copy(), pool.pair_id[idx].copy(), pool.read_num[idx].copy(), pool.is_rc[idx].copy(),
                         pool.reg_rank[idx].copy(), pool.n_pairs)
    return Case(name, what, c.rl, new, c.wins, c.planted, c.classes, c.verdicts)


def _order(rl, variant):
    """the `sizes` pool laid out another way, every record with the rank it has there"""
    c = case("sizes", rl)
    pool = c.pool
    R = pool.n_records
    by_rank = np.argsort(pool.reg_rank, kind="stable")
    none = np.zeros(0, np.int64)
    # the read-2 couples of every fifth pair
    some = by_rank[(pool.read_num[by_rank] == 2) & (pool.pair_id[by_rank] % 5 == 0)]
    rest = by_rank[~((pool.read_num[by_rank] == 2) & (pool.pair_id[by_rank] % 5 == 0))]
    if variant == "one_run":
        return _relaid(c, "order_one_run", "all records in the primary pool by rank: the members are in registration order as recorded", by_rank, none)
    if variant == "second_empty":
        return _relaid(c, "order_second_empty", "two runs, the second without read-1 members: a merge with n1p == n1", rest, some)
    if variant == "first_empty":
        return _relaid(c, "order_first_empty", "two runs, the first without read-1 members: a merge with n1p == 0", some, rest)
    rng = np.random.default_rng(77)
    npri = pool.primary.shape[0]

    def couples(lo, hi):
        k = rng.permutation((hi - lo) // 2)
        return (lo + np.stack([2 * k, 2 * k + 1], 1).reshape(-1)).astype(np.int64)

    return _relaid(c, "order_permuted", "the couples permuted inside the pools: the members are sorted by rank", couples(0, npri), couples(npri, R))


_MAKERS = {
    "sizes": _sizes, "pieces": _pieces, "nines": _nines, "nines_257": lambda rl: _nines(rl, True),
    "overflow_tail": lambda rl: _overflow(rl, "tail"), "overflow_head": lambda rl: _overflow(rl, "head"),
    "overflow_at_6144": lambda rl: _overflow(rl, "at_6144"), "overflow_at_6145": lambda rl: _overflow(rl, "at_6145"),
    "giants": lambda rl: _giants(rl, False), "giants_below": lambda rl: _giants(rl, True),
    "palindrome": _palindrome, "read2_shapes": _read2_shapes,
    "order_one_run": lambda rl: _order(rl, "one_run"), "order_second_empty": lambda rl: _order(rl, "second_empty"),
    "order_first_empty": lambda rl: _order(rl, "first_empty"), "order_permuted": lambda rl: _order(rl, "permuted"),
}
NAMES = tuple(_MAKERS)
OVERFLOWS = tuple(n for n in NAMES if n.startswith("overflow"))
ORDERS = ("sizes",) + tuple(n for n in NAMES if n.startswith("order_"))       # `sizes` is the layout as made: two runs
LONG_NAMES = ("sizes", "pieces") + OVERFLOWS                                   # the long-read build (rl 100)
RL, RL_LONG = 50, 100
INS = 175
BUILDS = {"couples": (RL, NAMES), "general": (RL, NAMES), "long": (RL_LONG, LONG_NAMES)}


@functools.lru_cache(maxsize=None)
def case(name, rl=RL):
    c = _MAKERS[name](rl)
    assert all(len(w) == WLEN for w in c.wins)
    return c


@functools.lru_cache(maxsize=None)
def oracle_results(name, rl=RL):
    """per string of the case: (pairs of the oracle's quick_map, its coverage verdict)"""
    from oracle import oracle
    c = case(name, rl)
    ix = oracle.ReadIndex(c.pool)
    out = []
    for w in c.wins:
        pairs, starts = ix.quick_map(w)
        out.append((pairs, ix.coverage_is_valid(starts, len(w), INS)))
    return out
