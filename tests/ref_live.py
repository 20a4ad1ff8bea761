"""The compiled reference as a live yardstick (oracle/_ref/vdjer_ref: the reference's own sources, compiled by `make -C oracle ref`
and driven by oracle/ref_harness.cpp).  No test in here: tests/test_oracle_vs_reference_live.py pins the oracle to it,
tests/test_gpu_vs_reference_live.py the HIP stages, and tests/golden/make_golden_edges.py writes the edges_* fixtures with it, so that
the pin also holds where the binary is absent.

  graph / map_windows / score   run one sub-command in a temporary directory and parse what the reference's own functions dumped
  put_read                      write a forward record AND its reverse-complement twin: a reads file holds forward records only and the
                                reader derives the twin, so an edit of one row alone cannot be expressed in it
  draw_graph / draw_map / draw_score, make_pool / make_map_case
                                configurations from a seed, the same for the CPU and the GPU tests
  EDGE_GRAPH / EDGE_MAP, edge_graph_case / edge_map_case
                                the fixed configurations of the fixtures and their loaders (the recipe is read from edges.json)

A configuration is a plain dict (it goes into edges.json as it is): rl, clones, pairs, noise, err, n_rate, seed (make_repertoire's;
make_reads takes seed + 1, the edits draw from [seed, 2, i], the windows from [seed, 3]), edits (names of EDITS, applied in order)
and the flags k / mf / mq, or ins / wlen / e0 / e1 / rs / ms / rf.
"""
import gzip
import hashlib
import json
import os
import re
import subprocess
import tempfile

import numpy as np

from vdjer_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "vdjer_ref")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SKIP_REASON = "oracle/_ref/vdjer_ref is not built (make -C oracle ref, where the reference's sources are)"


def available():
    return os.path.exists(REF_BIN)


class RefError(RuntimeError):
    """the reference binary failed or printed something else than it should: an error of the run, never a reason to skip"""


# ---------------------------------------------------------------------------------------------- running the binary
def _run(args, cwd, timeout, stdout=subprocess.DEVNULL):
    r = subprocess.run([REF_BIN] + [str(a) for a in args], cwd=cwd, stdout=stdout, stderr=subprocess.PIPE, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RefError(f"vdjer_ref {args[0]} ended with {r.returncode}: {r.stderr[-2000:]}")
    return r


def _inputs(d, rep, pool):
    synth.write_ref_dir(rep, os.path.join(d, "ref"))
    pool.write_reads_file(os.path.join(d, "reads.txt"))
    return ["--in", "reads.txt", "--chain", "IGH", "--ref-dir", "ref"]


def _tsv(path):
    with open(path) as f:
        return [l.rstrip("\n").split("\t") for l in f if l.strip()]


def node_rows(rows):
    """(id, k-mer, freq, has_v, has_j, to, from) per line of a nodes dump"""
    return [(int(r[0]), r[1], int(r[2]), int(r[3]), int(r[4]), [int(x) for x in r[5].split(",") if x],
             [int(x) for x in (r[6] if len(r) > 6 else "").split(",") if x]) for r in rows]


def graph(rep, pool, k, mf, mq, timeout=60, keep_text=False):
    """build_pre_graph, prune_pre_graph and build_graph2 over both pools: (pre-prune size, {surviving k-mer: count}, node rows).
    keep_text: also the two dumps as the binary wrote them (make_golden_edges.py stores them)."""
    with tempfile.TemporaryDirectory(prefix="vdjx_live_") as d:
        r = _run(["graph", "out"] + _inputs(d, rep, pool) + ["--ins", 175, "--k", k, "--mf", mf, "--mq", mq], d, timeout)
        m = re.search(r"HARNESS_GRAPH\tpre=(\d+)\tsurvivors=(\d+)\tnodes=(\d+)", r.stderr)
        if not m:
            raise RefError(f"vdjer_ref graph printed no HARNESS_GRAPH line: {r.stderr[-2000:]}")
        surv_rows, rows = _tsv(os.path.join(d, "out.survivors.tsv")), _tsv(os.path.join(d, "out.nodes.tsv"))
        texts = (open(os.path.join(d, "out.survivors.tsv")).read(), open(os.path.join(d, "out.nodes.tsv")).read()) if keep_text else None
    surv = {a: int(b) for a, b in surv_rows}
    nodes = node_rows(rows)
    if (len(surv_rows), len(surv), len(nodes)) != (int(m.group(2)), int(m.group(2)), int(m.group(3))):
        raise RefError(f"vdjer_ref graph: {len(surv_rows)} survivor rows and {len(nodes)} node rows for {m.group(0)!r}")
    return (int(m.group(1)), surv, nodes) + ((texts,) if keep_text else ())


def map_windows(rep, pool, wins, ins, e0, e1, rs, ms, rf, timeout=60, keep_text=False):
    """quick_map_process_contig and coverage_is_valid per window: [{valid, n, pairs, starts}] (parse_map's rows)"""
    from tests.test_oracle_vs_golden import parse_map
    with tempfile.TemporaryDirectory(prefix="vdjx_live_") as d:
        with open(os.path.join(d, "windows.txt"), "w") as f:
            f.write("\n".join(wins) + "\n")
        r = _run(["map", "windows.txt"] + _inputs(d, rep, pool) + ["--ins", ins, "--e0", e0, "--e1", e1, "--rs", rs, "--ms", ms, "--rf", rf],
                 d, timeout, stdout=subprocess.PIPE)
    out = parse_map(None, text=r.stdout)
    if len(out) != len(wins) or any(w["n"] != len(w["pairs"]) for w in out):
        raise RefError(f"vdjer_ref map: {len(out)} W rows for {len(wins)} windows (or P rows that do not add up): {r.stderr[-2000:]}")
    return (out, r.stdout) if keep_text else out


def score(lines, k, vk, thr, queries, timeout=60):
    """score_seq per query against the v-region lines: the verdicts"""
    with tempfile.TemporaryDirectory(prefix="vdjx_live_") as d:
        with open(os.path.join(d, "v.fa"), "w") as f:
            f.write("".join(f">line{i}\n{l}\n" for i, l in enumerate(lines)))
        with open(os.path.join(d, "q.txt"), "w") as f:
            f.write("\n".join(queries) + "\n")
        r = _run(["score", "v.fa", k, vk, thr, "q.txt"], d, timeout, stdout=subprocess.PIPE)
    rows = [l.split("\t") for l in r.stdout.splitlines()]
    if [x[0] for x in rows] != list(queries):
        raise RefError(f"vdjer_ref score: {len(rows)} rows for {len(queries)} queries")
    return [int(x[1]) for x in rows]


# ---------------------------------------------------------------------------------------------- pools
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in ("AT", "TA", "CG", "GC"):
    _COMP[ord(_a)] = ord(_b)


def _bytes(x, n):
    a = np.frombuffer(x.encode(), np.uint8) if isinstance(x, str) else np.asarray(x, np.uint8)
    assert a.shape[-1] == n, (a.shape, n)
    return a


def put_reads(pool, which, fwd_rows, seqs, quals):
    """put_read over many rows at once: seqs / quals are uint8 [n, rl] (or one row for all)"""
    arr = pool.primary if which == "primary" else pool.secondary
    rl = pool.rl
    fwd_rows = np.asarray(fwd_rows, np.int64)
    rec = fwd_rows + (0 if which == "primary" else pool.primary.shape[0])
    # forward records sit on even registration ranks, their twins on the next: what write_reads_file writes and the reader derives
    assert (pool.reg_rank[rec] % 2 == 0).all() and (pool.reg_rank[rec + 1] == pool.reg_rank[rec] + 1).all()
    s, q = np.broadcast_to(seqs, (len(fwd_rows), rl)), np.broadcast_to(quals, (len(fwd_rows), rl))
    arr[fwd_rows, 0] = arr[fwd_rows + 1, 0] = ord("0")
    arr[fwd_rows, 1:1 + rl] = s
    arr[fwd_rows, 1 + rl:] = q
    arr[fwd_rows + 1, 1:1 + rl] = _COMP[s[:, ::-1]]
    arr[fwd_rows + 1, 1 + rl:] = q[:, ::-1]


def put_read(pool, which, fwd_row, seq, qual):
    """the forward record `fwd_row` of pool.primary / pool.secondary and, in the next row, its reverse complement with the
    qualities reversed (bam_read.c:206-244)"""
    put_reads(pool, which, [fwd_row], _bytes(seq, pool.rl)[None, :], _bytes(qual, pool.rl)[None, :])


def _rand_bases(rng, shape):
    return synth.ACGT[rng.integers(0, 4, shape)]


def _edit_dup(pool, rng, c):
    """a third of the primary records twice, in whole couples (identical reads: the distinct-read rule, A2:349-352)"""
    m = (pool.primary.shape[0] // 3) & ~1
    pool.primary[m:2 * m] = pool.primary[:m]


def _edit_scramble(pool, rng, c):
    """qualities around the Phred-20 gate on 50 reads"""
    n = pool.primary.shape[0] // 2
    for r in rng.integers(0, max(n, 1), 50 if n else 0):
        put_read(pool, "primary", 2 * int(r), pool.primary[2 * int(r), 1:1 + pool.rl].copy(), rng.integers(33, 75, pool.rl, dtype=np.uint8))


LADDER_SUMS = (213, 214)


def ladder_reads(c):
    """Two k-mers whose quality sums end at 213 and at 214 exactly (A2:354-361: a sum that would reach 214 is stored as 255, so the
    first passes --mq 213 only and the second every --mq): per k-mer six distinct reads that start with it, each with one quality
    throughout (40, 40, 40, 40, 33 and 20 or 21: the record's first k qualities are then the k-mer's, A2:337-339, on both strands).
    Returns ([core], [(seq, qual)]); a pure function of the configuration."""
    rng = np.random.default_rng([c["seed"], 4])
    rl, k = c["rl"], c["k"]
    cores, reads = [], []
    for total in LADDER_SUMS:
        core = _rand_bases(rng, k)
        cores.append(core.tobytes().decode())
        for q in (40, 40, 40, 40, 33, total - 193):
            reads.append((np.concatenate([core, _rand_bases(rng, rl - k)]), np.full(rl, 33 + q, np.uint8)))
    return cores, reads


def _edit_ladders(pool, rng, c):
    _, reads = ladder_reads(c)
    assert pool.primary.shape[0] >= 2 * len(reads)
    for i, (s, q) in enumerate(reads):
        put_read(pool, "primary", 2 * i, s, q)


def _edit_tandem(pool, rng, c):
    """reads that run round short cycles (poly-A, (AC)n, (ACG)n, ...) and leave them, every ninth couple"""
    rl = pool.rl
    units = ["A", "AC", "ACG", "ACGTT", "T", "GGC"]
    for i, row in enumerate(range(0, pool.primary.shape[0] - 1, 18)):
        u = units[i % len(units)]
        ph = int(rng.integers(0, len(u)))
        tail = rl // 2 if i % 11 == 0 else rl // 5
        seq = (u * (rl + 5))[ph:ph + rl - tail] + _rand_bases(rng, tail).tobytes().decode()
        put_read(pool, "primary", row, seq, "I" * rl)


def _edit_all_n(pool, rng, c):
    rows = np.arange(0, pool.primary.shape[0] - 1, 14)
    put_reads(pool, "primary", rows, np.full((1, pool.rl), ord("N"), np.uint8), pool.primary[rows, 1 + pool.rl:].copy())


def _edit_hash_q(pool, rng, c):
    """reads of quality 2 throughout ('#'), every fifth couple of the secondary pool and every eleventh of the primary"""
    for which, arr, step in (("secondary", pool.secondary, 10), ("primary", pool.primary, 22)):
        rows = np.arange(0, arr.shape[0] - 1, step)
        put_reads(pool, which, rows, arr[rows, 1:1 + pool.rl].copy(), np.full((1, pool.rl), ord("#"), np.uint8))


def _edit_secondary_only(pool, rng, c):
    w = 2 * pool.rl + 1
    return synth.ReadPool(pool.rl, np.zeros((0, w), np.uint8), np.concatenate([pool.primary, pool.secondary]), pool.pair_id, pool.read_num,
                          pool.is_rc, pool.reg_rank, pool.n_pairs)


def _edit_hot(pool, rng, c):
    """c["hot_reads"] distinct reads around one string of c["hot_len"] bases: its k-mers (and their reverse complements) pass the
    frequency cap MAX_FREQUENCY - 1 = 32765 (A2:66, 345-347; the nodes' too, A2:261-265).  The random flanks have quality 2, so
    that no k-mer reaches into them (the dump stays small) while the reads stay distinct."""
    rl, n, hl = pool.rl, c["hot_reads"], c["hot_len"]
    left = (rl - hl) // 2
    S = _rand_bases(rng, (n, rl))
    S[:, left:left + hl] = _rand_bases(rng, hl)[None, :]
    Q = np.full((1, rl), ord("#"), np.uint8)
    Q[:, left:left + hl] = ord("I")
    put_reads(pool, "primary", 2 * np.arange(n), S, Q)


EDITS = {"dup": _edit_dup, "scramble": _edit_scramble, "ladders": _edit_ladders, "tandem": _edit_tandem, "all_n": _edit_all_n,
         "hash_q": _edit_hash_q, "secondary_only": _edit_secondary_only, "hot": _edit_hot}


def make_pool(c):
    """(repertoire, pool) of a configuration"""
    rep = synth.make_repertoire(c["clones"], seed=c["seed"])
    kw = dict(ins_mean=float(c["ins"]), ins_lo=c["ins"] - 55, ins_hi=c["ins"] + 65) if "ins" in c else {}
    pool = synth.make_reads(rep, c["pairs"], noise_frac=c["noise"], seed=c["seed"] + 1, rl=c["rl"], err=c["err"], n_rate=c["n_rate"], **kw)
    for i, e in enumerate(c.get("edits", [])):
        pool = EDITS[e](pool, np.random.default_rng([c["seed"], 2, i]), c) or pool
    return rep, pool


def codes(rep):
    return (np.array(sorted({synth.seq_to_int(a) for a in rep.v_anchors}), dtype=np.uint32),
            np.array(sorted({synth.seq_to_int(a) for a in rep.j_anchors}), dtype=np.uint32))


def pool_sha(pool):
    return hashlib.sha256(pool.primary.tobytes() + b"|" + pool.secondary.tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------- draws
GRAPH_MODES = ("le32", "gt32", "long", "even_k", "k46_50", "mq_edges")
MQ_EDGES = (213, 214, 215, 254, 255, 300)      # the ">= 214 reads as 255" rule from both sides, the largest value below the clamp, the clamp (A2:1514-1516)


def draw_graph(rng, mode, it=0):
    """le32 / gt32 / long as tests/test_gpu_fuzz.py draws them (at most 32 offsets per read, more, the word-per-32-bases records);
    even_k: the build that cannot pair a k-mer with its mirror image, on reads of at most 64 bases (the pools the other form takes);
    k46_50: the 24-byte tuples; mq_edges: MQ_EDGES in turn (configuration `it` takes MQ_EDGES[it % 6]) over pools that hold the
    two ladder k-mers.  Pools of 200 ... 1,500 pairs over 1 ... 5 clones, so that the reference takes a fraction of a second."""
    if mode == "long":
        rl = int(rng.integers(65, 161))
    elif mode == "k46_50":
        rl = int(rng.choice([50, 50, 64, 75, 100, 151]))
    else:
        rl = int(rng.choice([36, 40, 50, 50, 50, 64]))
    k = int(rng.integers(8, min(50, rl) + 1))
    if mode == "gt32" and rl - k + 1 <= 32:
        k = max(8, rl - 32 - int(rng.integers(0, 8)))
    if mode == "le32" and rl - k + 1 > 32:
        k = min(50, rl - 31 + int(rng.integers(0, 10)))
    if mode == "even_k":
        k = max(8, k & ~1)
    if mode == "k46_50":
        k = int(rng.integers(46, 51))
    c = dict(rl=rl, k=k, mf=int(rng.integers(1, 5)), mq=int(rng.choice([20, 40, 60, 90, 120, 214, 254, 300])),
             clones=int(rng.integers(1, 6)), pairs=int(rng.integers(200, 1501)), noise=float(rng.choice([0.0, 0.1, 0.3, 0.6])),
             err=float(rng.choice([0.0, 0.002, 0.01, 0.03])), n_rate=float(rng.choice([0.0, 0.002, 0.02])),
             seed=int(rng.integers(0, 1 << 30)), edits=[])
    if rng.random() < 0.3:
        c["edits"].append("dup")
    if rng.random() < 0.3:
        c["edits"].append("scramble")
    if mode == "mq_edges":                                  # deep enough for sums of 214 and more, and room for the ladders' twelve reads
        c.update(mq=MQ_EDGES[it % len(MQ_EDGES)], clones=min(c["clones"], 2), pairs=max(c["pairs"], 800), noise=min(c["noise"], 0.3))
        c["edits"].append("ladders")
    return c


def draw_map(rng):
    """the recipes of test_scorers_random_... and test_coverage_floor_one_random_... (tests/test_gpu_fuzz.py): read length, window
    length, insert size (the pool's fragments follow it), evaluation range, spans on both sides of the 64 deltas one word holds
    and every floor"""
    rl = int(rng.choice([36, 50, 50, 64, 75, 100, 151]))
    wlen = int(rng.integers(rl + 160, rl + 520))
    ins = int(rng.integers(rl + 60, rl + 220))
    e0 = int(rng.integers(1, max(2, wlen // 2)))
    e1 = int(rng.integers(e0 + 5, max(e0 + 6, wlen - rl // 2)))
    return dict(rl=rl, wlen=wlen, ins=ins, e0=e0, e1=e1, rs=int(rng.integers(10, rl)), ms=int(rng.choice([10, 30, 48, 48, 63, 64, 65, 90])),
                rf=int(rng.integers(0, 4)), clones=int(rng.integers(1, 6)), pairs=int(rng.integers(200, 1501)),
                noise=float(rng.choice([0.0, 0.2])), err=float(rng.choice([0.0, 0.002, 0.004])), n_rate=0.001, seed=int(rng.integers(0, 1 << 30)), edits=[])


def make_map_case(c):
    """(repertoire, pool, windows): three slices of every clone, one in five reverse-complemented, and one random string LAST"""
    rep, pool = make_pool(c)
    rng = np.random.default_rng([c["seed"], 3])
    wins = []
    for t in rep.clones:
        for _ in range(3):
            st = int(rng.integers(0, len(t) - c["wlen"] + 1))
            w = t[st:st + c["wlen"]]
            wins.append(w if rng.random() < 0.8 else synth.revcomp(w))
    wins.append(_rand_bases(rng, c["wlen"]).tobytes().decode())
    return rep, pool, wins


def draw_score(rng, it):
    """the recipe of test_root_scorer_random_configurations_vs_oracle: k 3 ... 50, vk 2 ... 16 (one in five at or next to k <= vk), one to
    four lines of 2k+1 to a few thousand characters with an N or a lower-case character now and then, three thresholds -1 ... k+1"""
    from tests import root_queries as Q
    k = int(rng.integers(3, 51))
    vk = int(rng.integers(2, 17))
    if it % 5 == 4:
        k = max(3, vk - int(rng.integers(0, 3))) if it % 10 == 4 else min(50, vk + 1)
    n_lines = int(rng.integers(1, 5))
    vr = synth.make_repertoire(2, seed=int(rng.integers(0, 1 << 30))).v_region
    cap = 3000 if vk > 6 else max(2 * k + 1, min(3000, 1_500_000 // (n_lines * 2 * k * k)))
    lines = []
    for _ in range(n_lines):
        ln = 2 * k + 1 if rng.random() < 0.25 else int(rng.integers(2 * k + 1, cap + 1))
        a = int(rng.integers(0, len(vr) - ln))
        line = list(vr[a:a + ln])
        if rng.random() < 0.3:
            for p_ in rng.integers(0, ln, int(rng.integers(1, 5))):
                line[int(p_)] = "N" if rng.random() < 0.7 else line[int(p_)].lower()
        lines.append("".join(line))
    return dict(it=it, k=k, vk=vk, lines=lines, queries=Q.queries(rng, lines, k, 240), thrs=[int(t) for t in rng.integers(-1, k + 2, 3)])


# ---------------------------------------------------------------------------------------------- the fixtures' configurations
def _g(rl, k, mf, mq, seed, clones=2, pairs=900, noise=0.2, err=0.004, n_rate=0.002, edits=(), **kw):
    return dict(rl=rl, k=k, mf=mf, mq=mq, clones=clones, pairs=pairs, noise=noise, err=err, n_rate=n_rate, seed=seed, edits=list(edits), **kw)


_MQ = dict(rl=50, k=25, mf=2, seed=707, clones=1, pairs=500, edits=("scramble", "ladders"))
# one configuration per edge the dumps of make_golden.py leave out; each holds what its name says and little else
EDGE_GRAPH = {
    "even_k34": _g(50, 34, 2, 60, 701), "k48": _g(50, 48, 2, 60, 702, clones=1, pairs=1500), "k12": _g(50, 12, 3, 90, 703, pairs=400),
    "rl36_k25": _g(36, 25, 2, 60, 704), "rl64_k30_dup": _g(64, 30, 2, 60, 705, edits=("dup",)),
    "rl100_k35": _g(100, 35, 2, 90, 706, pairs=600), "rl151_k50_mf4": _g(151, 50, 4, 60, 708, pairs=500),
    "reads_with_n": _g(50, 35, 2, 60, 709, n_rate=0.02, pairs=1500),
    "mq213": _g(mq=213, **_MQ), "mq214": _g(mq=214, **_MQ), "mq215": _g(mq=215, **_MQ), "mq254": _g(mq=254, **_MQ),
    "mq255": _g(mq=255, **_MQ), "mq300": _g(mq=300, **_MQ),
    # the handmade pools
    "tandem_k25": _g(50, 25, 3, 90, 711, pairs=1200, edits=("tandem",)), "tandem_k34": _g(50, 34, 2, 60, 711, pairs=1200, edits=("tandem",)),
    "all_n": _g(50, 35, 2, 60, 712, pairs=700, edits=("all_n",)), "hash_q": _g(50, 35, 2, 60, 713, pairs=700, noise=0.5, edits=("hash_q",)),
    "k_eq_rl50": _g(50, 50, 2, 60, 714, clones=1, pairs=1500),
    "secondary_only": _g(50, 35, 3, 90, 716, pairs=1200, noise=0.3, edits=("secondary_only",)),
    "hot_k35": _g(50, 35, 3, 90, 717, clones=1, pairs=45000, err=0.002, n_rate=0.001, edits=("hot",), hot_reads=34000, hot_len=36),
    "hot_k34": _g(50, 34, 3, 90, 717, clones=1, pairs=45000, err=0.002, n_rate=0.001, edits=("hot",), hot_reads=34000, hot_len=36),
}
HANDMADE = ["tandem_k25", "tandem_k34", "all_n", "hash_q", "k_eq_rl50", "secondary_only", "hot_k35", "hot_k34"]


def _m(rl, wlen, ins, e0, e1, rs, ms, rf, seed, clones=2, pairs=700):
    return dict(rl=rl, wlen=wlen, ins=ins, e0=e0, e1=e1, rs=rs, ms=ms, rf=rf, clones=clones, pairs=pairs, noise=0.1, err=0.002, n_rate=0.001,
                seed=seed, edits=[])


EDGE_MAP = {
    "ms90": _m(50, 486, 175, 52, 411, 35, 90, 1, 801),                     # past the 64 deltas of one word: the difference arrays
    "rf0_e_rs": _m(50, 400, 160, 20, 300, 25, 48, 0, 802),                 # floor 0 (no validation), e0 / e1 / rs off their defaults
    "rf3_rl100_ins300": _m(100, 520, 300, 60, 430, 60, 65, 3, 803, clones=1, pairs=900),
    "rl36_ms64_ins130": _m(36, 300, 130, 10, 250, 20, 64, 2, 804, clones=1),
}


def edge_conditions(tag, c, pre, surv, nodes):
    """what each fixture is there for (asserted where it is made and wherever it is used)"""
    if tag.startswith("k_eq_rl"):                           # one k-mer per record, and a k-mer of two DISTINCT reads would be shorter than they are: all pruned
        assert pre >= 100 and not nodes
    else:
        assert len(nodes) >= 1
    if tag.startswith("hot"):
        assert max(r[2] for r in nodes) == 32765 == max(surv.values())
    if tag.startswith("mq"):                                # the ladder k-mers sit where they were put
        at213, at214 = ladder_reads(c)[0]
        assert (at213 in surv) == (c["mq"] <= 213) and at214 in surv


def timeout_of(c):
    return 120 if c.get("hot_reads") else 60


def edges():
    with open(os.path.join(GOLD, "edges.json")) as f:
        return json.load(f)


def _gz(name):
    with gzip.open(os.path.join(GOLD, name), "rt") as f:
        return f.read()


def _pool_of_fixture(info):
    rep, pool = make_pool(info["recipe"])
    # a change of synth (or of the edits above) is not a parity failure: say so before anything is compared
    assert pool_sha(pool) == info["sha256"], "the recipe no longer gives the pool the dump was made from: regenerate tests/golden/edges_* (make_golden_edges.py)"
    return rep, pool


def edge_graph_case(tag):
    """(configuration, repertoire, pool, pre-prune size, survivors, node rows) of tests/golden/edges_<tag>.*"""
    info = edges()["graph"][tag]
    rep, pool = _pool_of_fixture(info)
    surv = {r[0]: int(r[1]) for r in (l.split("\t") for l in _gz(f"edges_{tag}.survivors.tsv.gz").splitlines())}
    nodes = node_rows([l.split("\t") for l in _gz(f"edges_{tag}.nodes.tsv.gz").splitlines()])
    assert (len(surv), len(nodes)) == (info["survivors"], info["nodes"])
    return info["recipe"], rep, pool, info["pre"], surv, nodes


def edge_map_case(tag):
    """(configuration, repertoire, pool, windows, parse_map's rows) of tests/golden/edges_map_<tag>.txt.gz"""
    from tests.test_oracle_vs_golden import parse_map
    info = edges()["map"][tag]
    rep, pool, wins = make_map_case(info["recipe"])
    assert pool_sha(pool) == info["sha256"], "the recipe no longer gives the pool the dump was made from: regenerate tests/golden/edges_* (make_golden_edges.py)"
    ref = parse_map(None, text=_gz(f"edges_map_{tag}.txt.gz"))
    assert len(ref) == len(wins) == info["windows"] and sum(w["valid"] for w in ref) == info["valid"] and sum(w["n"] for w in ref) == info["pairs"]
    return info["recipe"], rep, pool, wins, ref
