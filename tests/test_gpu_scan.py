"""The exclusive prefix sum of the device code (vdjer_amd/csrc/vdjx_scan.h) on its own, through vdjx_scan_u32: both forms (one launch,
three launches) and both output widths against numpy.cumsum in uint64, all n + 1 elements compared exactly.  The sizes sit around the
one-launch tile W and the device-wide block B (tests/scan_shapes.py reads them from the header).  All cases run in one child process
with a timeout, as the other API checks of the suite do (a fault in one call therefore fails every case of the module, with the child's
output); a wrong result is reported for its own case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.scan_shapes import BLOCK as B, TILE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sizes(launches, u64):
    W = TILE[u64]
    if launches == 1:
        return [0, 1, 63, 64, 65, 1023, 1024, 1025, W - 1, W, W + 1, 2 * W + 5]
    return [0, 1, B - 1, B, B + 1, 1024 * B - 1, 1024 * B + 1, W * B + B + 1]      # (the last: the top-level scan crosses a tile)


def _cases():
    out = []
    for launches in (1, 3):
        for u64 in (False, True):
            out += [(launches, u64, n, "random") for n in _sizes(launches, u64)]
            # a wrong out[n] and a dropped carry: nothing but zeros, and nothing but the last element, over several tiles / blocks
            n = 2 * TILE[u64] + 5 if launches == 1 else 1024 * B + 1
            out += [(launches, u64, n, "zeros"), (launches, u64, n, "last")]
    return out


def _id(case):
    launches, u64, n, kind = case
    return f"{launches}-{'u64' if u64 else 'u32'}-{n}-{kind}"


def _counts(u64, n, kind):
    rng = np.random.default_rng(1000 * n + u64)
    if kind != "random":
        a = np.zeros(n, np.uint32)
        if kind == "last":
            a[-1] = 0xFFFFFFFF
        return a
    if u64:
        # counts up to 2^32 - 1: the sum passes 2^32 inside the first wave, inside the first tile and at about every second element after
        a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        a[:3] = 0xFFFFFFFF
        return a
    return rng.integers(0, max(2, 0xFFFFFFFF // max(n, 1)), n, dtype=np.uint64).astype(np.uint32)      # the total stays below 2^32


def _child():
    """every case on the device: prints 'SCAN {case id: None or what differs}'"""
    import ctypes as C
    from vdjer_amd import api
    ctx = api.Context(0)
    res = {}
    for case in _cases():
        launches, u64, n, kind = case
        a = _counts(u64, n, kind)
        ref = np.zeros(n + 1, np.uint64)
        np.cumsum(a, dtype=np.uint64, out=ref[1:])
        if not u64 and int(ref[-1]) >= 1 << 32:                          # (of the reference: the 4-byte sums must not have to wrap)
            res[_id(case)] = f"the reference total {int(ref[-1])} does not fit 32 bits: the test's counts are wrong"
            continue
        out = np.full(n + 1, 0xA5A5A5A5, np.uint64 if u64 else np.uint32)
        rc = ctx.L.vdjx_scan_u32(ctx.h, a.ctypes.data_as(C.c_void_p), n, int(u64), launches, out.ctypes.data_as(C.c_void_p))
        if rc:
            res[_id(case)] = f"rc {rc}: {ctx.L.vdjx_last_error().decode(errors='replace')}"
            continue
        bad = np.flatnonzero(out.astype(np.uint64) != ref)
        res[_id(case)] = None if bad.size == 0 else f"{bad.size} of {n + 1} differ, first at {int(bad[0])}: {int(out[bad[0]])} != {int(ref[bad[0]])}"
    # refusals
    one = np.zeros(2, np.uint32)
    for n, launches in ((1 << 31, 1), (1, 2), (1, 0)):
        rc = ctx.L.vdjx_scan_u32(ctx.h, one.ctypes.data_as(C.c_void_p), n, 0, launches, one.ctypes.data_as(C.c_void_p))
        res[f"refused-{n}-{launches}"] = None if rc != 0 else "accepted"
    ctx.close()
    print("SCAN", json.dumps(res))


@pytest.fixture(scope="module")
def results():
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_scan import _child; _child()"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("SCAN ")).split(" ", 1)[1])


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_scan_against_numpy_cumsum(results, case):
    assert results[_id(case)] is None, results[_id(case)]


def test_scan_refuses_bad_arguments(results):
    bad = {k: v for k, v in results.items() if k.startswith("refused-") and v is not None}
    assert not bad and sum(k.startswith("refused-") for k in results) == 3, bad
