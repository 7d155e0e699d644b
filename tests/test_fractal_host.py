"""CPU-only tests of the DFA / Hurst host side: the companion library libmhfeat_fractal.so
(include/mhfeat_fractal.h) builds, loads and exports exactly its header's entry points, and
leaves the other two libraries' exports as they were; every invalid request is rejected
before any device call; the sub-window step equals the reference's expression; the Python
features resolve as the reference's call forms; every fixture
(tests/golden/make_golden_fractal.py) is within the 1e-12 conditioning cap of its
long-double restatement."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CAP = 1e-12


@pytest.fixture(scope="module")
def LR():
    import __graft_entry__
    __graft_entry__.build()
    from pymhealth_amd import _lib_fractal
    return _lib_fractal.lib()


def _exported(path):
    lines = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True,
                           text=True).stdout.splitlines()
    return {ln.split()[-1] for ln in lines if len(ln.split()) == 3 and ln.split()[1] == "T"}


def _declared(header, api, prefix):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"^\s*%s\s+(?:const\s+)?\w+\*?\s+\*?(%s\w+)\(" % (api, prefix), hdr, re.M))


def test_exports_every_header_symbol(LR):
    from pymhealth_amd import _lib_fractal
    hdr = open(os.path.join(ROOT, "include", "mhfeat_fractal.h")).read()
    decls = _declared("mhfeat_fractal.h", "MHFR_API", "mhfr_")
    assert decls == {"mhfr_version", "mhfr_last_error", "mhfr_dfa_step", "mhfr_dfa", "mhfr_hurst"}
    assert set(_lib_fractal.EXPORTS) == decls
    for name in decls:
        assert hasattr(LR, name), name
    assert _exported(_lib_fractal.LIB_PATH) == decls
    assert LR.mhfr_version() == _lib_fractal.MHFR_ABI_VERSION
    assert int(re.search(r"#define MHFR_ABI_VERSION (\d+)", hdr).group(1)) == LR.mhfr_version()
    for k in ("MHFR_DTYPE_F32", "MHFR_DTYPE_F64", "MHFR_OUT_EXPONENT", "MHFR_OUT_FLUCT",
              "MHFR_MAX_SEGMENT", "MHFR_MAX_SCALES", "MHFR_MAX_LAGS"):
        assert int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) == getattr(_lib_fractal, k), k
    assert _lib_fractal.MHFR_MAX_SEGMENT >= 8192
    from pymhealth_amd import _lib
    assert (_lib_fractal.MHFR_DTYPE_F32, _lib_fractal.MHFR_DTYPE_F64) == (_lib.MHF_DTYPE_F32,
                                                                          _lib.MHF_DTYPE_F64)
    for k, v in (("MHFR_EINVAL", 1), ("MHFR_EUNSUPPORTED", 2), ("MHFR_EDEVICE", 3)):
        assert int(re.search(r"#define %s \(-(\d+)\)" % k, hdr).group(1)) == v
    # self-contained: it links neither of the other two libraries
    dyn = subprocess.run(["readelf", "-d", _lib_fractal.LIB_PATH], capture_output=True, text=True).stdout
    assert "libmhfeat.so" not in dyn and "libmhfeat_nufft.so" not in dyn


def test_other_libraries_exports_unchanged(LR):
    """libmhfeat.so (ABI 7) and libmhfeat_nufft.so (ABI 1) export what their headers declare
    and their bindings list — nothing of this library leaked into them."""
    from pymhealth_amd import _lib, _lib_nufft
    L, LX = _lib.lib(), _lib_nufft.lib()
    main = _exported(_lib.LIB_PATH)
    assert main == set(_lib.EXPORTS) == _declared("mhfeat.h", "MHF_API", "mhf_")
    nufft = _exported(_lib_nufft.LIB_PATH)
    assert nufft == set(_lib_nufft.EXPORTS) == _declared("mhfeat_nufft.h", "MHFX_API", "mhfx_")
    assert nufft == {"mhfx_version", "mhfx_last_error", "mhfx_nufft_grid_params",
                     "mhfx_nufft1d1_workspace", "mhfx_nufft1d1"}
    assert not any(s.startswith("mhfr_") for s in main | nufft)
    assert (L.mhf_version(), LX.mhfx_version()) == (7, 1)


def _i64(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int64))


def _ptr(v):
    return ctypes.c_void_p(v) if v else None


def _dfa(L, **kw):
    """mhfr_dfa on fake (never dereferenced) device pointers."""
    a = dict(x=4096, dt=1, n=1000, starts=8192, ends=12288, B=10, min_len=1, max_len=300,
             scales=[4, 8, 16], ns=None, order=1, overlap=0.0, mode=0, out=16384, ld=1)
    a.update(kw)
    sc = None if a["scales"] is None else _i64(a["scales"])
    ns = a["ns"] if a["ns"] is not None else (0 if sc is None else len(sc))
    return L.mhfr_dfa(_ptr(a["x"]), a["dt"], a["n"], _ptr(a["starts"]), _ptr(a["ends"]), a["B"],
                      a["min_len"], a["max_len"], None if sc is None else sc.ctypes.data, ns,
                      a["order"], a["overlap"], a["mode"], _ptr(a["out"]), a["ld"], None)


def _hurst(L, **kw):
    a = dict(x=4096, dt=1, n=1000, starts=8192, ends=12288, B=10, min_len=1, max_len=300,
             lags=list(range(2, 64)), nl=None, mode=0, out=16384, ld=1)
    a.update(kw)
    lg = None if a["lags"] is None else _i64(a["lags"])
    nl = a["nl"] if a["nl"] is not None else (0 if lg is None else len(lg))
    return L.mhfr_hurst(_ptr(a["x"]), a["dt"], a["n"], _ptr(a["starts"]), _ptr(a["ends"]), a["B"],
                        a["min_len"], a["max_len"], None if lg is None else lg.ctypes.data, nl,
                        a["mode"], _ptr(a["out"]), a["ld"], None)


COMMON_BAD = [dict(dt=2), dict(dt=-1), dict(mode=2), dict(mode=-1), dict(B=-1), dict(n=-1),
              dict(ends=0),                    # starts without ends
              dict(starts=0),                  # ends without starts
              dict(starts=0, ends=0),          # no bounds: one segment only (B = 10)
              dict(out=0), dict(x=0), dict(ld=0), dict(max_len=-1)]


def test_dfa_argument_validation_without_gpu(LR):
    """Every invalid request is rejected on the host, with a message, before any launch."""
    from pymhealth_amd import _lib_fractal
    bad = COMMON_BAD + [
        dict(order=0), dict(order=4), dict(order=-1),
        dict(scales=[2, 8, 16]),               # 2 < order + 2 = 3
        dict(scales=[4, 8, 16], order=3),      # 4 < 5
        dict(scales=[3, 8], order=2),          # 3 < 4
        dict(scales=[0, 8]), dict(scales=[-4, 8]),
        dict(scales=[8]), dict(scales=[]), dict(scales=None, ns=3), dict(ns=1),
        dict(overlap=100.0), dict(overlap=-1.0), dict(overlap=150.0), dict(overlap=float("nan")),
        dict(mode=1, ld=2),                    # F(w) rows need out_ld >= n_scales = 3
    ]
    for b in bad:
        rc = _dfa(LR, **b)
        assert rc == -1, (b, rc)
        assert LR.mhfr_last_error(), b
    _dfa(LR, scales=[2, 8, 16])
    assert b"order + 2" in LR.mhfr_last_error()
    _dfa(LR, overlap=100.0)
    assert b"[0, 100)" in LR.mhfr_last_error()
    # beyond the limits: unsupported, not invalid
    assert _dfa(LR, max_len=_lib_fractal.MHFR_MAX_SEGMENT + 1) == -2
    assert b"MHFR_MAX_SEGMENT" in LR.mhfr_last_error()
    assert _dfa(LR, scales=list(range(4, 4 + 65))) == -2
    assert LR.mhfr_last_error()
    # a good request with nothing to do clears the error and touches no device
    assert _dfa(LR, B=0) == 0
    assert LR.mhfr_last_error() == b""
    assert _dfa(LR, B=0, max_len=_lib_fractal.MHFR_MAX_SEGMENT, scales=list(range(5, 5 + 64)),
                order=3, overlap=99.9, mode=1, ld=64) == 0


def test_hurst_argument_validation_without_gpu(LR):
    from pymhealth_amd import _lib_fractal
    bad = COMMON_BAD + [
        dict(lags=[0, 2, 4]), dict(lags=[-1, 2]), dict(lags=[3]), dict(lags=[]),
        dict(lags=None, nl=4), dict(nl=1),
        dict(mode=1, ld=61),                   # tau rows need out_ld >= n_lags = 62
    ]
    for b in bad:
        rc = _hurst(LR, **b)
        assert rc == -1, (b, rc)
        assert LR.mhfr_last_error(), b
    _hurst(LR, lags=[0, 2, 4])
    assert b"lag 0" in LR.mhfr_last_error()
    assert _hurst(LR, max_len=_lib_fractal.MHFR_MAX_SEGMENT + 1) == -2
    assert b"MHFR_MAX_SEGMENT" in LR.mhfr_last_error()
    assert _hurst(LR, lags=list(range(1, 130))) == -2
    assert LR.mhfr_last_error()
    assert _hurst(LR, B=0) == 0
    assert LR.mhfr_last_error() == b""
    assert _hurst(LR, B=0, lags=list(range(1, 129)), mode=1, ld=128,
                  max_len=_lib_fractal.MHFR_MAX_SEGMENT) == 0


def test_step_equals_reference_expression(LR):
    """max(int(w * (100 - overlap) / 100), 1) (timedom.py:226) — the Python helper and the
    library's host computation, over scales and overlaps including 12.5, 33.3 and 99."""
    from pymhealth_amd import engine
    overlaps = [0, 0.0, 1, 10, 12.5, 25, 33.3, 50, 50.0, 66.6, 75, 90, 99, 99.5, 99.99]
    scales = list(range(1, 130)) + [255, 256, 257, 1000, 1024, 4095, 4096, 8192, 16384]
    for ov in overlaps:
        for w in scales:
            want = max(int(w * (100 - ov) / 100), 1)
            assert engine.dfa_step(w, ov) == want, (w, ov)
            assert LR.mhfr_dfa_step(w, float(ov)) == want, (w, ov)
    assert engine.dfa_step(4, 99) == 1 and engine.dfa_step(64, 12.5) == 56
    assert engine.dfa_step(np.int64(16), np.float64(33.3)) == 10
    for w, ov in ((0, 0.0), (-3, 0.0), (8, 100.0), (8, -0.5), (8, float("nan"))):
        assert LR.mhfr_dfa_step(w, ov) == -1
        assert LR.mhfr_last_error()


def test_features_resolve_like_the_reference_call_forms():
    from pymhealth_amd import features
    from pymhealth_amd.feature import SegmentFeature, resolve
    from pymhealth_amd.generic import timedom
    f = resolve(functools.partial(timedom.dfa, windows=[4, 8, 16]))
    assert isinstance(f, SegmentFeature) and f.kind == "dfa"
    assert f.params == {"windows": [4, 8, 16], "o": 1, "overlap": 0}
    g = resolve(functools.partial(timedom.dfa, windows=[5, 11, 16], o=2, overlap=50))
    assert (g.params["windows"], g.params["o"], g.params["overlap"]) == ([5, 11, 16], 2, 50)
    p = resolve(functools.partial(timedom.dfa, [4, 8], 3))          # positional, as dfa(x, windows, o)
    assert (p.params["windows"], p.params["o"]) == ([4, 8], 3)
    h = resolve(timedom.hurst)
    assert h is timedom.hurst and h.kind == "hurst" and h.params == {"lags": None}
    hl = resolve(functools.partial(timedom.hurst, lags=[1, 2, 4]))
    assert hl.params == {"lags": [1, 2, 4]}
    assert resolve(features.dfa([4, 8, 16], o=2)).params["o"] == 2
    assert features.hurst().params == {"lags": None} and features.hurst([2, 3]).params == {"lags": [2, 3]}
    assert "dfa" in features.__all__ and "hurst" in features.__all__
    for name in ("dfa", "hurst", "o1fit", "o1fit_multiple"):
        assert name in timedom.__all__ and callable(getattr(timedom, name))
    assert timedom.dfa.__name__ == "dfa" and timedom.hurst.__name__ == "hurst"
    # the original objects are not modified by binding
    assert timedom.dfa.params["windows"] is None
    with pytest.raises(TypeError):
        resolve(functools.partial(timedom.dfa, windows=[4, 8], bogus=1))
    with pytest.raises(TypeError):
        resolve(functools.partial(timedom.hurst, [2, 3], lags=[2, 3]))


def test_unbound_dfa_raises_typeerror_naming_the_partial_form():
    from pymhealth_amd.generic import timedom
    from pymhealth_amd.util.windows import (indices_rolling_apply, nonuniform_rolling_apply,
                                            rolling_apply)
    for make in (lambda: rolling_apply(timedom.dfa, 128, 64),
                 lambda: rolling_apply([np.mean, timedom.dfa], 128, 64),
                 lambda: rolling_apply({"a": timedom.dfa}, 128, 64),
                 lambda: indices_rolling_apply(timedom.dfa),
                 lambda: nonuniform_rolling_apply(timedom.dfa),
                 lambda: rolling_apply(functools.partial(timedom.dfa, o=2), 128, 64)):
        with pytest.raises(TypeError, match=r"functools\.partial\(timedom\.dfa, windows="):
            make()
    # bound forms build without a GPU
    assert callable(rolling_apply(functools.partial(timedom.dfa, windows=[4, 8, 16]), 128, 64))
    assert callable(rolling_apply(timedom.hurst, 128, 64))
    assert callable(nonuniform_rolling_apply([np.mean, timedom.hurst]))


def test_2d_record_raises_the_existing_error():
    from pymhealth_amd.generic import timedom
    from pymhealth_amd.util.windows import rolling_apply
    x = np.zeros((400, 3), np.float32)
    with pytest.raises(TypeError, match="hurst not defined on 2-D windows"):
        rolling_apply(timedom.hurst, 128, 64)(x)
    with pytest.raises(TypeError, match="dfa not defined on 2-D windows"):
        rolling_apply(functools.partial(timedom.dfa, windows=[4, 8]), 128, 64)(x)


def test_mhealth_alias_has_the_four_functions():
    import pymhealth_amd
    from pymhealth_amd.generic import timedom
    pymhealth_amd.install_mhealth_alias()
    import mhealth.generic.timedom as t
    assert t is timedom
    from mhealth.generic.timedom import dfa, hurst, o1fit, o1fit_multiple
    assert dfa is timedom.dfa and hurst is timedom.hurst
    assert o1fit is timedom.o1fit and o1fit_multiple is timedom.o1fit_multiple


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pymhealth_amd.generic import timedom
    x = np.random.default_rng(0).standard_normal(300)
    with pytest.raises(RuntimeError, match="no CPU path"):
        timedom.hurst(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        timedom.dfa(x, [4, 8, 16])
    with pytest.raises(RuntimeError, match="no CPU path"):
        timedom.o1fit(x, x)


def _pairs(d):
    """(name, reference values, long-double values) of every checked quantity of a fixture."""
    out = []
    for k in d.files:
        if k.endswith("__ld"):
            base = k[:-4]
            out.append((k, d[base + ("__alpha" if base + "__alpha" in d.files else "__H")], d[k]))
        elif k.endswith("_ld"):
            out.append((k, d[k[:-3]], d[k]))
    return out


@pytest.mark.parametrize("name", ["dfa", "hurst", "segments", "rolling", "o1fit"])
def test_fixtures_within_conditioning_cap(name):
    """|reference - long double| <= 1e-12 for every stored value (relative for o1fit, whose
    intercepts are not O(1)); the files stay under 100 KB and avoid the keys by which
    tests/golden_cases.py classifies the other fixtures."""
    path = os.path.join(GOLDEN, "fractal_%s.npz" % name)
    assert os.path.getsize(path) < 100 * 1024
    d = np.load(path)
    assert not {"wsize", "fs", "indices"} & set(d.files)
    pairs = _pairs(d)
    assert pairs
    for key, ref, ld in pairs:
        ref, ld = np.asarray(ref, np.float64), np.asarray(ld, np.float64)
        ok = np.isfinite(ref)
        assert ok.any() and (np.isfinite(ld) == ok).all(), key
        scale = np.abs(ld[ok]) if name == "o1fit" else 1.0
        assert (np.abs(ref[ok] - ld[ok]) <= CAP * scale).all(), (key, np.abs(ref[ok] - ld[ok]).max())
    if name == "dfa":
        assert len(d["max_segment__x"]) == 16384
        assert len(d["n4133__x"]) % 256 != 0
    if name == "segments":
        assert len(d["x"]) == 6000 and 250 <= len(d["starts"]) <= 350
        assert (d["starts"] < 0).any() and (d["ends"] > len(d["x"])).any()
        assert (d["ends"] <= d["starts"]).any() and np.isnan(d["dfa"]).any()
