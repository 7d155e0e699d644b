"""CPU-only tests of the non-uniform FFT's host side: the companion library
libmhfeat_nufft.so (include/mhfeat_nufft.h) builds, loads and exports exactly its header's
entry points; grid parameters equal the reference's (tests/golden/make_golden_nufft.py);
every invalid request is rejected before any device call; the Python drop-in
``generic.frequency.nufft`` keeps the reference's errors and has no CPU path."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def LX():
    import __graft_entry__
    __graft_entry__.build()
    from pymhealth_amd import _lib_nufft
    return _lib_nufft.lib()


def test_exports_every_header_symbol(LX):
    from pymhealth_amd import _lib_nufft
    hdr = open(os.path.join(ROOT, "include", "mhfeat_nufft.h")).read()
    decls = set(re.findall(r"^\s*MHFX_API\s+(?:const\s+)?\w+\*?\s+\*?(mhfx_\w+)\(", hdr, re.M))
    assert decls == {"mhfx_version", "mhfx_last_error", "mhfx_nufft_grid_params",
                     "mhfx_nufft1d1_workspace", "mhfx_nufft1d1"}
    assert set(_lib_nufft.EXPORTS) == decls
    for name in decls:
        assert hasattr(LX, name), name
    assert LX.mhfx_version() == _lib_nufft.MHFX_ABI_VERSION
    assert int(re.search(r"#define MHFX_ABI_VERSION (\d+)", hdr).group(1)) == _lib_nufft.MHFX_ABI_VERSION
    for k in ("MHFX_DTYPE_F64", "MHFX_DTYPE_C128", "MHFX_OUT_COMPLEX", "MHFX_OUT_POWER"):
        assert int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) == getattr(_lib_nufft, k), k
    lines = subprocess.run(["nm", "-D", "--defined-only", _lib_nufft.LIB_PATH], capture_output=True,
                           text=True).stdout.splitlines()
    funcs = {ln.split()[-1] for ln in lines if len(ln.split()) == 3 and ln.split()[1] == "T"}
    assert funcs == decls, funcs ^ decls
    # the transform is libmhfeat.so's: linked, not compiled in again
    dyn = subprocess.run(["readelf", "-d", _lib_nufft.LIB_PATH], capture_output=True, text=True).stdout
    assert "libmhfeat.so" in dyn and "$ORIGIN" in dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", _lib_nufft.LIB_PATH], capture_output=True,
                         text=True).stdout
    assert "mhf_fft" in und and "mhf_fft_workspace" in und


def test_grid_params_match_reference_table(LX):
    """(Msp, Mr, tau) of the C entry point and of the Python function equal the reference's
    _compute_grid_params on both sides of eps = 1e-11: integers exactly, tau bit for bit."""
    from pymhealth_amd.generic.frequency import nufft
    t = np.load(os.path.join(GOLDEN, "nufft_grid_params.npz"))
    assert len(t["M"]) >= 20 and (t["eps"] > 1e-11).any() and (t["eps"] <= 1e-11).any()
    for M, eps, Msp, Mr, tau in zip(t["M"], t["eps"], t["Msp"], t["Mr"], t["tau"]):
        a, b, c = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_double()
        assert LX.mhfx_nufft_grid_params(int(M), float(eps), ctypes.byref(a), ctypes.byref(b),
                                         ctypes.byref(c)) == 0
        assert (a.value, b.value) == (Msp, Mr), (M, eps)
        assert np.float64(c.value).tobytes() == np.float64(tau).tobytes(), (M, eps)
        pm, pr, pt = nufft._compute_grid_params(int(M), float(eps))
        assert isinstance(pm, int) and isinstance(pr, int)
        assert (pm, pr) == (Msp, Mr), (M, eps)
        assert np.float64(pt).tobytes() == np.float64(tau).tobytes(), (M, eps)
    assert nufft._compute_grid_params(256, 1e-15)[:2] == (14, 768)
    assert LX.mhfx_nufft_grid_params(256, 1e-15, None, None, None) == 0
    for M, eps in ((1, 1e-15), (0, 1e-15), (16, 1e-33), (16, 1e-1), (16, 0.5), (16, float("nan"))):
        assert LX.mhfx_nufft_grid_params(M, eps, None, None, None) == -1, (M, eps)
        assert LX.mhfx_last_error()
    LX.mhfx_nufft_grid_params(16, 0.5, None, None, None)
    assert b"1e-33 < eps < 1e-1" in LX.mhfx_last_error()
    assert LX.mhfx_nufft_grid_params(1 << 29, 1e-15, None, None, None) == -2    # Mr > 2^30


def _call(L, **kw):
    """mhfx_nufft1d1 on fake (never dereferenced) device pointers."""
    from pymhealth_amd import _lib_nufft
    a = dict(x=4096, c=8192, cdt=_lib_nufft.MHFX_DTYPE_F64, n=1000, starts=12288, ends=16384,
             B=10, min_len=1, M=16, df=1.0, eps=1e-15, iflag=1, mode=_lib_nufft.MHFX_OUT_COMPLEX,
             out=20480, ld=16, ws=1 << 20, wsn=None)
    a.update(kw)
    if a["wsn"] is None:
        a["wsn"] = max(L.mhfx_nufft1d1_workspace(a["M"], a["eps"], a["B"]), 0)
    p = lambda v: ctypes.c_void_p(v) if v else None   # noqa: E731
    return L.mhfx_nufft1d1(p(a["x"]), p(a["c"]), a["cdt"], a["n"], p(a["starts"]), p(a["ends"]),
                           a["B"], a["min_len"], a["M"], a["df"], a["eps"], a["iflag"], a["mode"],
                           p(a["out"]), a["ld"], p(a["ws"]), a["wsn"], None)


def test_argument_validation_without_gpu(LX):
    """Every invalid request is rejected on the host, with a message, before any launch."""
    need = LX.mhfx_nufft1d1_workspace(16, 1e-15, 10)
    assert need > 0
    bad = [dict(M=1), dict(M=0), dict(eps=1e-34), dict(eps=0.1), dict(eps=0.2),
           dict(cdt=0), dict(cdt=7), dict(mode=2), dict(mode=-1),
           dict(ld=15),                    # out_ld is the row pitch: < M
           dict(B=20, ld=10),              # out_ld < n_segments (and < M)
           dict(wsn=need - 1), dict(ws=0), dict(wsn=0),
           dict(ends=0),                   # starts without ends
           dict(starts=0),                 # ends without starts
           dict(starts=0, ends=0),         # no bounds: one segment only (B = 10)
           dict(x=0), dict(c=0), dict(out=0), dict(n=-1), dict(B=-1), dict(df=float("inf"))]
    for b in bad:
        rc = _call(LX, **b)
        assert rc == -1, (b, rc)
        assert LX.mhfx_last_error(), b
    _call(LX, wsn=need - 1)
    assert b"workspace too small" in LX.mhfx_last_error()
    assert _call(LX, B=0) == 0             # nothing to do: no device call
    assert LX.mhfx_last_error() == b""
    assert LX.mhfx_nufft1d1_workspace(16, 1e-15, 0) == 0
    assert LX.mhfx_nufft1d1_workspace(1, 1e-15, 4) == -1
    assert LX.mhfx_nufft1d1_workspace(16, 0.5, 4) == -1
    assert LX.mhfx_nufft1d1_workspace(16, 1e-15, -1) == -1
    # grids (Mr = 48 complex128 per segment) plus the transform's own workspace
    from pymhealth_amd import _lib
    L = _lib.lib()
    assert need >= 10 * 48 * 16 + L.mhf_fft_workspace(48, 10)
    # at most 256 MiB of grid at a time: the workspace stops growing with the batch
    big = LX.mhfx_nufft1d1_workspace(256, 1e-15, 10 ** 6)
    assert big == LX.mhfx_nufft1d1_workspace(256, 1e-15, 10 ** 7)


def test_nufftfreqs():
    from pymhealth_amd.generic.frequency import nufft
    assert nufft.nufftfreqs(5).tolist() == [-2, -1, 0, 1, 2]
    assert nufft.nufftfreqs(4, 0.5).tolist() == [-1.0, -0.5, 0.0, 0.5]
    assert nufft.nufftfreqs(4).tolist() == [-2, -1, 0, 1]


def test_python_argument_errors():
    """The reference's errors, raised before any device work (so also without a GPU)."""
    from pymhealth_amd.generic.frequency import nufft
    x, c = np.linspace(0, 1, 8), np.ones(8)
    for eps in (1e-33, 1e-1, 0.5, 1e-40):
        with pytest.raises(ValueError, match=re.escape("eps must satisfy 1e-33 < eps < 1e-1.")):
            nufft.nufft1d1(x, c, 8, eps=eps)
        with pytest.raises(ValueError, match=re.escape("eps must satisfy 1e-33 < eps < 1e-1.")):
            nufft._compute_grid_params(8, eps)
    with pytest.raises(ValueError, match="M must be >= 2"):
        nufft.nufft1d1(x, c, 1)
    with pytest.raises(ValueError, match="M must be >= 2"):
        nufft.nufft1d1_segments(x, c, [0], [8], 1)
    with pytest.raises(ZeroDivisionError):
        nufft.nufft1d1(np.zeros(0), np.zeros(0), 8)
    with pytest.raises(ValueError, match="same length"):
        nufft.nufft1d1(x, c[:7], 8)
    with pytest.raises(ValueError, match="same length"):
        nufft.nufft1d1_segments(x, c[:7], [0], [8], 8)


def test_mhealth_alias_has_nufft():
    import pymhealth_amd
    pymhealth_amd.install_mhealth_alias()
    from mhealth.generic.frequency import nufft  # noqa: F401
    from mhealth.generic.frequency.nufft import nufft1d1, nufftfreqs, _compute_grid_params  # noqa: F401
    import mhealth.generic.frequency as fq
    assert fq.nufft is nufft and nufft is pymhealth_amd.generic.frequency.nufft


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pymhealth_amd.generic.frequency import nufft
    x, c = np.linspace(0, 1, 8), np.ones(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nufft.nufft1d1(x, c, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nufft.nufft1d1_segments(x, c, [0, 2], [8, 6], 8, power=True)
