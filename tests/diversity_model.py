"""The model of vdjx_diversity (include/vdjx.h) in plain Python: the draw rule, a replicate's counts (one draw at a time, and a numpy
path for many), the Hill numbers summed with math.fsum, mean and sd in replicate order, the info, the tolerance the device's float64
results are held to -- and the rows of `vdjer --diversity` with its stderr line, to predict the command line's bytes.  Nothing here is
shared with the device code, with vdjer_amd/annot.py or with vdjer_main.c."""
import math

import numpy as np

M64 = (1 << 64) - 1
CHECK = 0xE220A8397B1DCDAF                                  # mix64(0)
CELLS = 1 << 28                                             # counters of a batch: VDJX_DIV_CELLS' default
LDS_CLONES = 16384                                          # the largest C of the LDS histogram: VDJX_DIV_LDS_CLONES' default
PATH_LDS, PATH_GLOBAL = 1, 2
FIELDS = ["clones", "weighted", "weight", "depth", "replicates", "batches", "path"]
COLUMNS = ["q", "d_observed", "d", "d_sd", "d_lower", "d_upper", "e", "e_lower", "e_upper"]
Z95 = 1.959963984540054
EPS = 2.0 ** -52


def mix64(x):
    """splitmix64's output step, in 64-bit wrap-around arithmetic"""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def orders():
    """`vdjer`'s grid: k / 10.0 for k = 0 .. 40"""
    return [k / 10.0 for k in range(41)]


def draw(seed, r, i, W):
    """t of draw i (0 .. N - 1) of replicate r (1 .. B): the high half of mix64(mix64(seed) + (r << 32 | i)) * W"""
    return (mix64((mix64(seed) + ((r << 32) | i)) & M64) * W) >> 64


def cumulative(weight):
    cum = [0]
    for w in weight:
        cum.append(cum[-1] + int(w))
    return cum


def counts_plain(weight, N, seed, r):
    """one replicate, one draw at a time: the draw falls on the clone k with cum[k] <= t < cum[k + 1]"""
    cum = cumulative(weight)
    out = [0] * len(weight)
    for i in range(N):
        t = draw(seed, r, i, cum[-1])
        k = next(k for k in range(len(weight)) if cum[k] <= t < cum[k + 1])
        out[k] += 1
    return out


def _mix64_np(x):
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _mulhi_np(u, W):
    """the high half of u * W, u a uint64 array, W < 2^64, from 32-bit halves"""
    lo32 = np.uint64(0xFFFFFFFF)
    s = np.uint64(32)
    u0, u1 = u & lo32, u >> s
    w0, w1 = np.uint64(W & 0xFFFFFFFF), np.uint64(W >> 32)
    mid = u1 * w0 + ((u0 * w0) >> s)                        # < 2^64: (2^32 - 1)^2 + 2^32 - 1
    mid2 = u0 * w1 + (mid & lo32)
    return u1 * w1 + (mid >> s) + (mid2 >> s)


def counts(weight, N, seed, r):
    """one replicate with numpy -> int64[C]; the same rule as counts_plain (tests/test_diversity_cpu.py compares the two)"""
    cum = cumulative(weight)
    W = cum[-1]
    assert 0 < W < 1 << 63 and 1 <= N < 1 << 31 and 1 <= r <= 4096 and 0 <= seed <= M64
    with np.errstate(over="ignore"):
        x = np.arange(N, dtype=np.uint64) + np.uint64((mix64(seed) + (r << 32)) & M64)      # (i < 2^32: r << 32 | i = (r << 32) + i)
        t = _mulhi_np(_mix64_np(x), W)
    k = np.searchsorted(np.array(cum, np.uint64), t, side="right") - 1
    return np.bincount(k, minlength=len(weight)).astype(np.int64)


def hill(values, total, q):
    """the Hill number of order q of p_k = values[k] / total over the values > 0; the sums with math.fsum"""
    ps = [int(v) / int(total) for v in values if int(v) > 0]
    if q == 0.0:
        return float(len(ps))
    if q == 1.0:
        return math.exp(-math.fsum(p * math.log(p) for p in ps))
    return math.fsum(p ** q for p in ps) ** (1.0 / (1.0 - q))


def mean_sd(d):
    """over the replicates (rows of d), summed in replicate order; sd with n - 1, 0 for one replicate"""
    B, Q = len(d), len(d[0])
    mean, sd = [], []
    for j in range(Q):
        s = 0.0
        for r in range(B):
            s += d[r][j]
        m = s / B
        v = 0.0
        for r in range(B):
            v += (d[r][j] - m) * (d[r][j] - m)
        mean.append(m)
        sd.append(math.sqrt(v / (B - 1)) if B > 1 else 0.0)
    return mean, sd


def diversity(weight, N, q=None, replicates=200, seed=1, cells=CELLS, lds_clones=LDS_CLONES):
    """-> dict(observed, mean, sd: float64[Q]; d: float64[B, Q]; counts: int64[B, C]; info)"""
    q = orders() if q is None else [float(x) for x in q]
    C = len(weight)
    assert 0 < C < 1 << 20 and 1 <= replicates <= 4096 and 1 <= N < 1 << 31 and 1 <= len(q) <= 64
    assert all(0.0 <= x <= 16.0 and not 0.0 < abs(x - 1.0) < 1.0 / 64.0 for x in q)
    W = sum(int(w) for w in weight)
    cs = np.stack([counts(weight, N, seed, r) for r in range(1, replicates + 1)])
    d = [[hill(row, N, x) for x in q] for row in cs.tolist()]
    mean, sd = mean_sd(d)
    per_batch = min(replicates, max(1, cells // C))
    info = dict(clones=C, weighted=sum(1 for w in weight if int(w) > 0), weight=W, depth=N, replicates=replicates, batches=-(-replicates // per_batch),
                path=PATH_LDS if C <= lds_clones else PATH_GLOBAL)
    return dict(observed=np.array([hill(weight, W, x) for x in q]), mean=np.array(mean), sd=np.array(sd), d=np.array(d), counts=cs, info=info)


def rel_tol(q, m):
    """the relative tolerance of a device Hill number against this model, m the clones drawn (of weight, for `observed`): a sum of m
    positive terms in any order is within (m - 1) eps; the rounding of p, magnified by q <= 16, and sixteen ulps each for pow, log and exp
    are the 64; 1 / |1 - q| is what the outer power magnifies the sum's error by, ln m what exp(-sum) does (the sum is at most ln m)"""
    if q == 0.0:
        return 0.0
    if q == 1.0:
        return (m + 64) * EPS * max(1.0, math.log(m))
    return (m + 64) * EPS * max(1.0, 1.0 / abs(1.0 - q))


# ---- `vdjer --diversity` -------------------------------------------------------------------------------------------------------------------
def hundredths(cell):
    """a printed expected_count cell ("12.34") as integer hundredths, digit by digit"""
    whole, point, frac = cell.partition(".")
    assert point == "." and len(frac) == 2 and (whole + frac).isdigit(), cell
    return int(whole) * 100 + int(frac)


def weights(clone, cells):
    """-> (weights, lineage numbers): a lineage's weight is the sum of its members' printed expected_count cells in hundredths; lineages of
    weight 0 and contigs in no lineage (clone < 0) are left out; ascending lineage number"""
    sums = {}
    for k, cell in zip(clone, cells):
        if int(k) >= 0:
            sums[int(k)] = sums.get(int(k), 0) + hundredths(cell)
    keep = sorted(k for k, w in sums.items() if w > 0)
    return [sums[k] for k in keep], keep


def default_depth(weight):
    """the lineages' total expected pairs rounded half up, at least 1"""
    return max(1, (sum(weight) + 50) // 100)


def table_rows(q, observed, mean, sd):
    rows = []
    d0 = mean[0]
    assert q[0] == 0.0
    for j, x in enumerate(q):
        lo, hi = max(mean[j] - Z95 * sd[j], 0.0), mean[j] + Z95 * sd[j]
        rows.append(["%.1f" % x] + ["%.4f" % v for v in (observed[j], mean[j], sd[j], lo, hi, mean[j] / d0, lo / d0, hi / d0)])
    return rows


def table_text(rows):
    return "".join("\t".join(r) + "\n" for r in [COLUMNS] + rows)


def summary_line(n_lineages, weight, N, replicates, seed, mean, batches):
    """mean: the 41-order grid's (None when no lineage has weight)"""
    W = sum(weight)
    d0, d1, d2 = (mean[0], mean[10], mean[20]) if mean is not None else (0.0, 0.0, 0.0)
    return (f"diversity: {len(weight)} lineages with weight of {n_lineages}, {W // 100}.{W % 100:02d} expected pairs, depth {N}, {replicates} replicates "
            f"(seed {seed}), richness {d0:.2f}, shannon {d1:.4f}, simpson {d2:.4f}, {batches} batches")
