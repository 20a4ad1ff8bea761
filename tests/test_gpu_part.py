"""The LDS-staged partition pass of the k-mer build (vdjer_amd/csrc/vdjx_part.h) on its own, through vdjx_part_u64: the streaming
kernel and its host helper as the build instantiates them (8-byte elements with paired loads and holes, 16-byte elements with their own
load and store; one level, and two levels with the second inside the segments of the first) against numpy.  The starts must be the
exclusive cumsum of the buckets' counts, exactly; every bucket's slice of the output must hold the elements of that bucket, each once
and whole (placement inside a bucket is arbitrary by design).  The sizes sit around ROUND, the elements of one round of a workgroup,
which follows the header's constants.  All cases run in one child process with a timeout, as tests/test_gpu_scan.py does; a wrong result
is reported for its own case."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_H = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_part.h")).read()


def _define(name):
    (v,) = re.findall(r"^#define %s (\d+)u?\b" % name, _H, re.M)
    return int(v)


THREADS, MAXB = _define("PART_THREADS"), _define("PART_MAXB")
ROUND = {b: _define("PART_LDS_BYTES") // b // THREADS * THREADS for b in (8, 16)}      # 16,384 items, 8,192 tuples
HOLE = 0xFFFFFFFFFFFFFFFF


def _case(name, eb, n, nb=37, kind="uniform", levels=1, fine_bits=0, slices=1, wgs=1):
    return dict(id=f"{name}-{eb}B-n{n}-nb{nb}-{kind}" + (f"-{nb >> fine_bits}x2^{fine_bits}x{slices}" if levels == 2 else f"-wg{wgs}"),
                eb=eb, n=n, nb=nb, kind=kind, levels=levels, fine_bits=fine_bits, slices=slices, wgs=wgs)


def _cases():
    out = []
    for eb in (8, 16):
        R = ROUND[eb]
        # one workgroup: no element, less than a pair, an odd tail, a round that is exactly full, a last round of one element
        out += [_case("one", eb, n) for n in (0, 1, 2, 3, R - 1, R, R + 1, 3 * R + 7)]
        # four workgroups: shares are whole rounds, so R + 1 leaves two of them nothing
        out += [_case("shared", eb, n, wgs=4) for n in (R + 1, 9 * R + 5)]
        out += [_case("buckets", eb, 2 * R + 5, nb=nb) for nb in (1, 2, 3, MAXB - 1, MAXB)]
        out += [_case("buckets", eb, 2 * R + 5, nb=MAXB, kind="first"), _case("buckets", eb, 2 * R + 5, nb=MAXB, kind="last"),
                _case("buckets", eb, MAXB, nb=MAXB, kind="each"), _case("buckets", eb, 2 * R + 5, nb=MAXB - 1, kind="sawtooth")]
        for coarse, fine_bits, slices in ((2, 1, 8), (3, 10, 8), (64, 5, 8), (1024, 1, 2)):
            out.append(_case("two", eb, 4 * R + 3, nb=coarse << fine_bits, levels=2, fine_bits=fine_bits, slices=slices, wgs=4))
        out += [_case("two", eb, 4 * R + 3, nb=64 << 5, kind="one_segment", levels=2, fine_bits=5, slices=8, wgs=4),
                _case("two", eb, 4 * R + 3, nb=64 << 5, kind="thin_segment", levels=2, fine_bits=5, slices=8, wgs=4)]
    R = ROUND[8]
    out += [_case("holes", 8, 2 * R + 5, kind="every_second", wgs=2), _case("holes", 8, R + 3, kind="all_holes"),
            _case("holes", 8, 2 * R + 5, kind="last_hole"),
            _case("holes", 8, 4 * R + 3, nb=64 << 5, kind="every_second", levels=2, fine_bits=5, slices=8, wgs=4)]
    return out


def _input(c):
    """(n, eb / 8) words: bucket << 40 | the element's index in the first word, a tag of the index in the second"""
    n, nb, kind = c["n"], c["nb"], c["kind"]
    rng = np.random.default_rng(7 * n + nb)
    i = np.arange(n, dtype=np.uint64)
    b = rng.integers(0, nb, n, dtype=np.uint64)
    if kind == "first":
        b[:] = 0
    elif kind == "last":
        b[:] = nb - 1
    elif kind in ("each", "sawtooth"):
        b = i % np.uint64(nb)
    elif kind == "one_segment":                     # coarse segment 40 of 64 holds everything
        b = (np.uint64(40) << np.uint64(c["fine_bits"])) | (b & np.uint64((1 << c["fine_bits"]) - 1))
    elif kind == "thin_segment":                    # three elements in coarse segment 5, for eight slices
        seg = b >> np.uint64(c["fine_bits"])
        b[seg == 5] += np.uint64(1 << c["fine_bits"])
        b[[11, n // 2, n - 1]] = (np.uint64(5) << np.uint64(c["fine_bits"])) | np.array([0, 7, 31], np.uint64)
    a = np.empty((n, c["eb"] // 8), np.uint64)
    a[:, 0] = (b << np.uint64(40)) | i
    if c["eb"] == 16:
        a[:, 1] = (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    if kind == "every_second":
        a[1::2, 0] = HOLE
    elif kind == "all_holes":
        a[:, 0] = HOLE
    elif kind == "last_hole":
        a[-1, 0] = HOLE
    return a


def _sorted_rows(a):
    return a[np.lexsort(tuple(a[:, j] for j in range(a.shape[1] - 1, -1, -1)))]


def _reference(c, a):
    """the kept elements and the expected starts"""
    kept = a[a[:, 0] != HOLE] if c["eb"] == 8 else a
    bucket = (kept[:, 0] >> np.uint64(40)).astype(np.int64)
    assert kept.shape[0] == c["n"] - (int((a[:, 0] == HOLE).sum()) if c["eb"] == 8 else 0) and (bucket < c["nb"]).all(), "the test's own input"
    starts = np.zeros(c["nb"] + 1, np.uint64)
    np.cumsum(np.bincount(bucket, minlength=c["nb"]), out=starts[1:])
    return kept, starts


def _differs(c, a, starts, out):
    kept, ref_starts = _reference(c, a)
    bad = np.flatnonzero(starts.astype(np.uint64) != ref_starts)
    if bad.size:
        return f"{bad.size} of {c['nb'] + 1} starts differ, first at {int(bad[0])}: {int(starts[bad[0]])} != {int(ref_starts[bad[0]])}"
    got = out[:kept.shape[0]]
    # every slice holds elements of its own bucket only, and the elements are the input's, each once and whole: with the starts
    # right, that is "the sorted slice of every bucket equals the sorted elements of that bucket"
    where = np.repeat(np.arange(c["nb"], dtype=np.uint64), np.diff(ref_starts).astype(np.int64))
    bad = np.flatnonzero((got[:, 0] >> np.uint64(40)) != where)
    if bad.size:
        return f"{bad.size} of {got.shape[0]} elements lie in another bucket's slice, first at {int(bad[0])}: {int(got[bad[0], 0]):#x} in bucket {int(where[bad[0]])}"
    bad = np.flatnonzero((_sorted_rows(got) != _sorted_rows(kept)).any(axis=1))
    if bad.size:
        return f"{bad.size} of {got.shape[0]} elements are not the input's (sorted), first at {int(bad[0])}"
    return None


REFUSALS = {            # one per rule of the entry: (elem_bytes, nb, levels, fine_bits, slices, workgroups, bucket of the one element)
    "elem_bytes": (4, 8, 1, 0, 1, 1, 0), "levels": (8, 8, 3, 0, 1, 1, 0), "nb_zero": (8, 0, 1, 0, 1, 1, 0),
    "nb_above_1024": (8, MAXB + 1, 1, 0, 1, 1, 0), "coarse_above_1024": (8, (MAXB + 1) << 1, 2, 1, 8, 1, 0),
    "nb_not_coarse_times_fine": (8, 5, 2, 1, 8, 1, 0), "fine_bits": (8, 1 << 11, 2, 11, 8, 1, 0), "slices": (16, 8, 2, 1, 0, 1, 0),
    "workgroups": (16, 8, 1, 0, 1, 0, 0), "bucket": (8, 8, 1, 0, 1, 1, 8),
}


def _child():
    """every case on the device: prints 'PART {case id: None or what differs}'"""
    import ctypes as C
    from vdjer_amd import api
    ctx = api.Context(0)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    res = {}
    for c in _cases():
        a = _input(c)
        starts = np.full(c["nb"] + 1, 0xA5A5A5A5, np.uint32)
        out = np.full(a.shape, 0xA5A5A5A5A5A5A5A5, np.uint64)
        rc = ctx.L.vdjx_part_u64(ctx.h, ptr(a), c["n"], c["eb"], c["nb"], c["levels"], c["fine_bits"], c["slices"], c["wgs"], ptr(starts), ptr(out))
        res[c["id"]] = f"rc {rc}: {ctx.L.vdjx_last_error().decode(errors='replace')}" if rc else _differs(c, a, starts, out)
    for name, (eb, nb, levels, fine_bits, slices, wgs, bucket) in REFUSALS.items():
        a = np.full((1, 2), bucket << 40, np.uint64)
        starts, out = np.zeros(max(nb, 1) + 1, np.uint32), np.zeros((1, 2), np.uint64)
        rc = ctx.L.vdjx_part_u64(ctx.h, ptr(a), 1, eb, nb, levels, fine_bits, slices, wgs, ptr(starts), ptr(out))
        res[f"refused-{name}"] = None if rc != 0 else "accepted"
    ctx.close()
    print("PART", json.dumps(res))


@pytest.fixture(scope="module")
def results():
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_part import _child; _child()"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("PART ")).split(" ", 1)[1])


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["id"])
def test_partition_against_numpy(results, case):
    assert results[case["id"]] is None, results[case["id"]]


def test_partition_refuses_bad_arguments(results):
    bad = {k: v for k, v in results.items() if k.startswith("refused-") and v is not None}
    assert not bad and sum(k.startswith("refused-") for k in results) == len(REFUSALS), bad
