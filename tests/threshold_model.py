"""The model of vdjx_lineage_threshold (include/vdjx.h) restated in Python: whole numbers only past the kernel tables, which call the same
libm exp with the same argument expression as the C helper.

The definitions are the plain ones (`kernel`, `bins`, `density_plain`, `peaks_of`, `threshold`).  numpy holds the arrays, and every value
in them is an exact integer: counts below 2^20, weights up to 2^30, sums below 2^50 in uint64 -- nothing rounds, nothing wraps.
`density_plain` costs (non-zero bins) x (grid) per bandwidth, which is minutes for an input with thousands of bins, so `density` switches
to `density_fft` from FFT_FROM bins on: the same sums by FFT over the two 15-bit limbs of the weights.  A limb's convolution is below 2^36,
and its float64 result lies within a small fraction of the whole number it stands for (asserted on every call: below 1/16), so rounding
gives that number.
tests/test_threshold_cpu.py compares the two forms on sparse and dense inputs."""
import functools
import math

import numpy as np

G = 10000
N = G + 1
FIX = 1 << 30
MAX_K = 200
DEFAULTS = dict(max_k=200, peak_shift=5, valley=(1, 2), min_values=10)
STATUS = ("found", "too few values", "no scale", "one mode", "shallow valley")
FOUND, FEW, NO_SCALE, ONE_MODE, SHALLOW = range(5)
INFO_FIELDS = ("values", "distinct", "status", "k", "peaks_all", "peaks", "p1_first", "p1_last", "p2_first", "p2_last", "t_first", "t_last",
               "threshold", "y1", "y2", "m", "ymax")
FFT_FROM = 48


@functools.lru_cache(maxsize=None)
def kernel(k):
    """-> (uint32[N], len): w[d] = floor(FIX exp(-(double)(d d) / (double)(200 k k)) + 0.5) up to the first 0, zeros from there"""
    assert 1 <= k <= MAX_K
    w = np.zeros(N, np.uint32)
    den = float(200 * k * k)
    reach = min(N, 66 * k + 8)                                               # (the first 0 comes at about 65.6 k: asserted below)
    xs = [int(math.floor(float(FIX) * math.exp(-float(d * d) / den) + 0.5)) for d in range(reach)]
    n = xs.index(0) if 0 in xs else reach
    assert n == N or n < reach
    w[:n] = xs[:n]
    w.setflags(write=False)
    return w, n


def bin_of(nearest, length, unit):
    return min(G, (2 * G * nearest + unit * length) // (2 * unit * length))


def bins(nearest, length, unit):
    """-> c: uint64[N]; an item with nearest < 0 takes no part and its length is not read"""
    d, L = np.asarray(nearest, np.int64), np.asarray(length, np.int64)
    assert d.shape == L.shape and d.ndim == 1 and (d >= -1).all() and (d < 1 << 31).all() and 1 <= int(unit) <= 1 << 20
    part = d >= 0
    d, L = d[part], L[part]
    assert ((L >= 1) & (L <= 255)).all()
    ul = int(unit) * L                                                      # (below 2^28; 2 G d + ul below 2^47: int64 holds it)
    v = np.minimum(G, (2 * G * d + ul) // (2 * ul))
    return np.bincount(v, minlength=N).astype(np.uint64)


def density_plain(c, k):
    """Y[g] = the sum over v of c[v] w[|g - v|], bin by bin"""
    w, n = kernel(k)
    w64 = w.astype(np.uint64)
    y = np.zeros(N, np.uint64)
    for v in np.flatnonzero(c):
        v = int(v)
        lo, hi = max(0, v - (n - 1)), min(G, v + (n - 1))                   # the g with a weight
        y[v:hi + 1] += c[v] * w64[:hi + 1 - v]
        if lo < v:
            y[lo:v] += c[v] * w64[v - lo:0:-1]
    return y


_SIZE = 32768                                                               # >= 2 N - 1


def density_fft(c, k, fc=None):
    w, _ = kernel(k)
    assert int(c.sum()) < 1 << 20
    if fc is None:
        fc = np.fft.rfft(c.astype(np.float64), _SIZE)
    full = np.concatenate([w[:0:-1], w]).astype(np.int64)                  # w[|j - G|] for j = 0 .. 2 G
    y = np.zeros(N, np.uint64)
    for part, shift in ((full & 32767, 0), (full >> 15, 15)):               # (the high limb of w[0] = 2^30 is 2^15)
        r = np.fft.irfft(fc * np.fft.rfft(part.astype(np.float64), _SIZE), _SIZE)[G:2 * G + 1]
        whole = np.rint(r)
        assert float(np.abs(r - whole).max()) < 1.0 / 16 and whole.min() >= 0 and whole.max() < 2.0 ** 36
        y += whole.astype(np.uint64) << np.uint64(shift)
    return y


def density(c, k, fc=None):
    return density_plain(c, k) if np.count_nonzero(c) < FFT_FROM else density_fft(c, k, fc)


def peaks_of(y, peak_shift):
    """the runs of equal Y that are peaks -> (peaks_all, [(first, last, Y) of the counted ones, ascending], ymax)"""
    start = np.concatenate([[0], np.flatnonzero(y[1:] != y[:-1]) + 1])
    last = np.concatenate([start[1:] - 1, [G]])
    v = y[start]
    before = np.concatenate([[True], v[1:] > v[:-1]])                       # greater than the run before it, or there is none
    after = np.concatenate([v[:-1] > v[1:], [True]])
    peak = (v > 0) & before & after
    ymax = int(y.max())
    counted = peak & ((v << np.uint64(peak_shift)) >= np.uint64(ymax))      # (Y < 2^50, shift <= 13)
    return int(peak.sum()), [(int(start[i]), int(last[i]), int(v[i])) for i in np.flatnonzero(counted)], ymax


def threshold(c, max_k=200, peak_shift=5, valley=(1, 2), min_values=10):
    """-> dict(hist uint32[N], density uint64[N], peaks uint32[max_k, 2], info dict) from the counts c"""
    assert 1 <= max_k <= MAX_K and 0 <= peak_shift <= 13 and 1 <= valley[1] <= 10 ** 6 and 0 <= valley[0] <= valley[1] and min_values >= 1
    c = np.asarray(c, np.uint64)
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["values"], info["distinct"] = int(c.sum()), int(np.count_nonzero(c))
    out = dict(hist=c.astype(np.uint32), density=np.zeros(N, np.uint64), peaks=np.zeros((max_k, 2), np.uint32), info=info)
    if info["values"] < min_values:
        info["status"] = FEW
        return out
    fc = np.fft.rfft(c.astype(np.float64), _SIZE) if info["distinct"] >= FFT_FROM else None
    rows, ks = {}, None
    for k in range(1, max_k + 1):
        y = density(c, k, fc)
        n_all, counted, ymax = peaks_of(y, peak_shift)
        out["peaks"][k - 1] = (n_all, len(counted))
        if ks is None and len(counted) <= 2:                                # k*: the smallest such k
            ks = k
        if k == ks or k == max_k:
            rows[k] = (y, n_all, counted, ymax)
    status = None
    if ks is None:
        ks, status = max_k, NO_SCALE
    y, n_all, counted, ymax = rows[ks]
    out["density"] = y
    info.update(k=ks, peaks_all=n_all, peaks=len(counted), ymax=ymax)
    info.update(p1_first=counted[0][0], p1_last=counted[0][1], y1=counted[0][2])
    if len(counted) >= 2:
        info.update(p2_first=counted[1][0], p2_last=counted[1][1], y2=counted[1][2])
    if status is None and len(counted) == 1:
        status = ONE_MODE
    if status is None:
        a, b = counted[0][1], counted[1][0]
        between = [int(x) for x in y[a + 1:b]]
        m = min(between)
        at = [a + 1 + i for i, x in enumerate(between) if x == m]
        info.update(t_first=at[0], t_last=at[-1], m=m)
        if valley[1] * m <= valley[0] * min(counted[0][2], counted[1][2]):
            status = FOUND
            info["threshold"] = (at[0] + at[-1]) // 2
        else:
            status = SHALLOW
    info["status"] = status
    return out


def macs(c, max_k):
    """the terms of the density pass with a weight: for every bin and every k the g within len_k - 1 of it"""
    total = 0
    lens = [kernel(k)[1] for k in range(1, max_k + 1)]
    for v in np.flatnonzero(c):
        v = int(v)
        total += sum(min(G, v + n - 1) - max(0, v - (n - 1)) + 1 for n in lens)
    return total
