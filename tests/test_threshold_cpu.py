"""vdjx_lineage_threshold without a GPU: the C kernel tables against the model's for every bandwidth, the model's two density forms against
each other, every named case of tests/threshold_cases.py reaching what it is there for (so that no device test passes vacuously), the
designed distances of the e2e_families golden, the refusals of the Python helpers, the ABI mirror and the command line up to where a GPU
would be needed."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tests import threshold_cases as TC
from tests import threshold_model as M
from tests.test_isotype_cpu import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(TC.cases("default"))


# ---- the kernel tables --------------------------------------------------------------------------------------------------------------------
def test_c_kernel_tables_equal_the_model():
    from vdjer_amd import annot
    total = 0
    for k in range(1, M.MAX_K + 1):
        w, n = annot.threshold_kernel(k)
        mw, mn = M.kernel(k)
        assert w.dtype == np.uint32 and w.shape == (M.N,) and n == mn and w.tobytes() == mw.tobytes(), k
        assert int(w[0]) == M.FIX and (w[:n] > 0).all() and not w[n:].any() and (np.diff(w.astype(np.int64)) <= 0).all(), k
        total += n
    assert M.kernel(1)[1] == TC.LEN1 == 66 and M.kernel(152)[1] < M.N == M.kernel(153)[1]          # len is about 65.6 k
    assert 1_200_000 < total < 1_300_000                                                            # the entries uploaded at max_k = 200
    L = __import__("vdjer_amd._lib", fromlist=["lib"]).lib()
    for k in (0, -1, 201):
        with pytest.raises(Exception, match="vdjx_threshold_kernel: k"):
            annot.threshold_kernel(k)
    assert L.vdjx_threshold_kernel(5, None, None) == -1 and b"NULL table" in L.vdjx_last_error()
    w = np.zeros(M.N, np.uint32)
    assert L.vdjx_threshold_kernel(5, w.ctypes.data_as(ctypes.c_void_p), None) == 0 and w.tobytes() == M.kernel(5)[0].tobytes()      # len may be NULL
    for bad in (1.5, "3", 1 << 40):
        with pytest.raises(ValueError):
            annot.threshold_kernel(bad)


def test_model_density_forms_agree():
    """the bin-by-bin sums and the FFT over 15-bit limbs give the same whole numbers: sparse, dense, the largest counts"""
    rng = np.random.default_rng(5)
    sparse = np.zeros(M.N, np.uint64)
    sparse[rng.integers(0, M.N, 50)] = rng.integers(1, 3000, 50).astype(np.uint64)
    dense = rng.integers(1, 100, M.N).astype(np.uint64)
    heavy = np.zeros(M.N, np.uint64)
    heavy[[0, 1, 4999, M.G]] = np.array([262143, 262143, 262144, 262144], np.uint64)                # 2^20 - 2 values in four bins
    for c, ks in ((sparse, (1, 2, 9, 77, 153, 200)), (dense, (1, 30, 200)), (heavy, (1, 100, 200))):
        for k in ks:
            a, b = M.density_plain(c, k), M.density_fft(c, k)
            assert a.dtype == b.dtype == np.uint64 and np.array_equal(a, b), k
    # and the definition itself, term by term in Python integers, at a few points
    w = [int(x) for x in M.kernel(9)[0]]
    y = M.density_plain(sparse, 9)
    for g in (0, 1, 4999, 5000, M.G):
        assert int(y[g]) == sum(int(sparse[v]) * w[abs(g - v)] for v in np.flatnonzero(sparse))


def test_model_bins_round_half_up_and_clamp():
    from vdjer_amd import annot
    assert M.bin_of(0, 40, 1) == 0 and M.bin_of(3, 40, 1) == 750 and M.bin_of(1, 3, 1) == 3333 and M.bin_of(2, 3, 1) == 6667
    assert M.bin_of(1, 16, 1) == 625 and M.bin_of(1, 32, 1) == 313                                   # 312.5 rounds up
    assert M.bin_of(40, 40, 1) == M.G and M.bin_of(2 ** 31 - 1, 1, 1) == M.G and M.bin_of(2000 * 255, 255, 2000) == M.G
    rng = np.random.default_rng(2)
    L = rng.integers(1, 256, 500)
    d = rng.integers(-1, 300, 500)
    for unit in (1, 7, 2000):
        du = np.where(d < 0, -1, d * unit + rng.integers(0, unit, 500))     # (in the call's unit; -1 stays -1)
        v = annot.threshold_bins(du, L, unit)
        want = [M.bin_of(int(x), int(l), unit) if x >= 0 else -1 for x, l in zip(du, L)]
        assert v.dtype == np.int32 and v.tolist() == want and min(want) == -1 and max(want) == M.G
        assert np.array_equal(np.bincount(v[v >= 0], minlength=M.N).astype(np.uint64), M.bins(du, L, unit))
    assert annot.threshold_bins([(1 << 31) - 1], [255], 1 << 20).tolist() == [M.bin_of((1 << 31) - 1, 255, 1 << 20)]      # the largest operands
    assert annot.threshold_bins([-1, 5], [0, 50], 1).tolist() == [-1, 1000]                           # (a length that is not read)


def test_python_helper_refusals():
    from vdjer_amd import annot
    for near, length, unit in (([-2], [10], 1), ([1], [0], 1), ([1], [256], 1), ([1], [10], 0), ([1], [10], (1 << 20) + 1), ([1, 2], [10], 1),
                               ([1 << 31], [10], 1), ([1], [10], 1.0)):
        with pytest.raises(ValueError):
            annot.threshold_bins(near, length, unit)
    with pytest.raises(ValueError):
        annot.threshold_bins(np.zeros(1 << 20, np.int32), np.ones(1 << 20, np.uint32), 1)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(TC.SETS))
@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_what_it_is_for(which, name):
    assert list(TC.cases(which)) == NAMES
    near, length, unit, over = TC.cases(which)[name]
    assert near.dtype == np.int32 and length.dtype == np.uint32 and near.shape == length.shape and len(near) < 1 << 20
    TC.reaches(which, name)
    r = TC.model(which, name)
    i = r["info"]
    assert r["hist"].dtype == np.uint32 and r["density"].dtype == np.uint64 and r["peaks"].shape == (TC.params(which, name)["max_k"], 2)
    assert i["values"] == int(r["hist"].sum()) == int((near >= 0).sum()) and i["distinct"] == int(np.count_nonzero(r["hist"]))
    assert (i["threshold"] != 0) <= (i["status"] == M.FOUND) and int(r["density"].max()) < 1 << 50
    if i["status"] in (M.FOUND, M.SHALLOW):                                  # k* is the smallest k with at most two counted peaks
        assert (r["peaks"][:i["k"] - 1, 1] > 2).all() and r["peaks"][i["k"] - 1].tolist() == [i["peaks_all"], 2]
        assert i["p1_last"] < i["t_first"] <= i["threshold"] or i["status"] == M.SHALLOW
        assert i["p1_last"] < i["t_first"] <= i["t_last"] < i["p2_first"]


def test_cases_cover_every_status_and_both_density_forms():
    seen = {TC.model(w, n)["info"]["status"] for w in TC.SETS for n in NAMES}
    assert seen == {M.FOUND, M.FEW, M.NO_SCALE, M.ONE_MODE, M.SHALLOW}
    distinct = [TC.model("default", n)["info"]["distinct"] for n in NAMES]
    assert min(d for d in distinct if d) < M.FFT_FROM <= max(distinct) == M.N
    assert TC.TILE == __import__("vdjer_amd._lib", fromlist=["x"]).THRESHOLD_TILE and f"tile_ends_peaks_{TC.TILE}" in NAMES
    assert TC.DEFAULT == dict(max_k=200, peak_shift=5, valley=(1, 2), min_values=10) and all(TC.OTHER[k] != TC.DEFAULT[k] for k in TC.DEFAULT)


def test_e2e_families_designed_distances():
    """the 21 designed distances of the golden's contigs, 185 .. 1250 ten-thousandths: what the model decides is what `vdjer
    --lineage-threshold` must print for them (tests/test_gpu_threshold_cli.py)"""
    near, length, unit, _ = TC.cases("default")["e2e_families"]
    v = sorted(M.bin_of(int(d), int(L), 1) for d, L in zip(near, length) if d >= 0)
    assert unit == 1 and len(near) > 80 and len(v) == 21 and v[0] == 185 and v[-1] == 1250
    i = TC.model("default", "e2e_families")["info"]
    print("e2e_families:", i)
    assert i["status"] == M.FOUND and i["k"] == 9 and i["threshold"] == 996 and (i["t_first"], i["t_last"]) == (996, 996)
    assert (i["p1_first"], i["p2_first"]) == (226, 1250) and i["threshold"] != 1500           # the command line makes a second pair pass


def test_macs_of_the_worst_case():
    """every bin non-zero under 200 bandwidths: the 1.6 x 10^10 multiply-adds of the issue's estimate"""
    lens = [M.kernel(k)[1] for k in range(1, 201)]
    total = sum(sum(min(M.G, v + n - 1) - max(0, v - (n - 1)) + 1 for n in lens) for v in (0, 5000, M.G))
    assert total == M.macs(np.array([1 if v in (0, 5000, M.G) else 0 for v in range(M.N)], np.uint64), 200)
    full = 0
    for n in lens:                                                            # (the sum over all v of the g within n - 1 of v)
        full += M.N * (2 * n - 1) - n * (n - 1) if n < M.N else M.N * M.N
    assert 1.2e10 < full < 1.8e10


# ---- the ABI mirror ------------------------------------------------------------------------------------------------------------------------
def test_abi_mirror_and_documents():
    from vdjer_amd import _lib, annot, api
    assert ctypes.sizeof(_lib.ThresholdParams) == 20 and ctypes.sizeof(_lib.ThresholdInfo) == 88
    assert [f for f, _ in _lib.ThresholdParams._fields_] == ["max_k", "peak_shift", "valley_num", "valley_den", "min_values"]
    assert [f for f, _ in _lib.ThresholdInfo._fields_] == ["values", "distinct", "status", "k", "peaks_all", "peaks", "p1_first", "p1_last", "p2_first", "p2_last",
                                                           "t_first", "t_last", "threshold", "reserved", "y1", "y2", "m", "ymax"]
    assert _lib.ThresholdInfo.y1.offset == 56
    for s in ("vdjx_lineage_threshold", "vdjx_threshold_kernel"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)
    assert _lib.THRESHOLD_STATUS == M.STATUS == api.Context.THRESHOLD_STATUS and (_lib.THRESHOLD_GRID, _lib.THRESHOLD_MAX_K) == (M.G, M.MAX_K) and annot.THRESHOLD_GRID == M.G
    assert tuple(f for f in api.Context.THRESHOLD_FIELDS) == M.INFO_FIELDS
    sig = inspect.signature(api.Context.lineage_threshold)
    assert list(sig.parameters)[1:] == ["nearest", "length", "unit", "max_k", "peak_shift", "valley", "min_values"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[3:]] == [1, 200, 5, (1, 2), 10]
    header = open(os.path.join(ROOT, "include", "vdjx.h")).read()
    for text in ("#define VDJX_THRESHOLD_GRID  10000u", "#define VDJX_THRESHOLD_MAX_K 200", f"#define VDJX_THRESHOLD_TILE  {TC.TILE}u", "/* 20 bytes */", "/* 88 bytes */",
                 "#define VDJX_THRESHOLD_SHALLOW  4u"):
        assert text in header, text
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "--lineage-threshold" in readme and "threshold_macs" in readme and "k_thr_density" in design and "profiles/threshold_resource_check.md" in design
    for text in (header, readme, design):
        assert "a threshold chosen automatically." not in text and "vdjx_lineage_threshold" in text
    source = open(os.path.join(ROOT, "vdjer_amd", "csrc", "vdjx_threshold.hip")).read()
    for kname in ("k_thr_hist", "k_thr_number", "k_thr_compact", "k_thr_density", "k_thr_peaks"):
        assert f'vdjx_prof_scope ps(c, "{kname}")' in source
    report = open(os.path.join(ROOT, "profiles", "threshold_resource_check.md")).read()
    for kname in ("k_thr_hist", "k_thr_compact", "k_thr_density", "k_thr_peaks", "k_scan_one"):
        assert kname in report


# ---- the command line, up to where a GPU would be needed -----------------------------------------------------------------------------------
def test_cli_refusals(tmp_path):
    r = _run(tmp_path, ["--lineage-threshold", "t.tsv"])
    assert r.returncode != 0 and "ELAPSED_SECS" not in r.stderr and "Invalid param" not in r.stderr
    assert "--lineage-threshold chooses the threshold of the --lineages table: it needs --lineages <file>" in r.stderr
    assert not (tmp_path / "t.tsv").exists() and not (tmp_path / "l.tsv").exists()
    r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-threshold"])
    assert r.returncode != 0 and "Missing value for param: --lineage-threshold" in r.stderr and "ELAPSED_SECS" not in r.stderr
    # --lineage-dist keeps its own refusals beside the new flag
    r = _run(tmp_path, ["--lineages", "l.tsv", "--lineage-threshold", "t.tsv", "--lineage-dist", "1.5"])
    assert r.returncode != 0 and "--lineage-dist must be a decimal in [0, 1] with at most four digits after the point: 1.5" in r.stderr
    assert "ELAPSED_SECS" not in r.stderr and not (tmp_path / "t.tsv").exists()


def test_cli_help_names_the_flag(tmp_path):
    r = _run(tmp_path, ["--help"])
    assert r.returncode == 0
    line = [l for l in (r.stderr + r.stdout).splitlines() if l.strip().startswith("--lineage-threshold")]
    assert len(line) == 1 and "--lineages" in line[0] and "--lineage-dist stands" in line[0]
