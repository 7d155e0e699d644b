"""ctypes binding of libmhfeat_fractal.so (include/mhfeat_fractal.h), the companion
library that holds detrended fluctuation analysis and the Hurst exponent.

Like ``_lib``: one compute path, the HIP kernels of the library. If it is missing, or no
GPU is visible, the entry points raise — there is no CPU fallback. The library stands
alone (it links neither libmhfeat.so nor libmhfeat_nufft.so).
"""
import ctypes
import os
import threading

from . import _lib

LIB_PATH = os.path.join(_lib.HERE, "libmhfeat_fractal.so")

MHFR_ABI_VERSION = 1   # include/mhfeat_fractal.h MHFR_ABI_VERSION
MHFR_DTYPE_F32 = 0
MHFR_DTYPE_F64 = 1
MHFR_OUT_EXPONENT = 0
MHFR_OUT_FLUCT = 1
MHFR_MAX_SEGMENT = 16384
MHFR_MAX_SCALES = 64
MHFR_MAX_LAGS = 128

ERRORS = _lib.ERRORS

EXPORTS = ("mhfr_version", "mhfr_last_error", "mhfr_dfa_step", "mhfr_dfa", "mhfr_hurst")

_lock = threading.Lock()
_libr = None


def lib():
    """Load libmhfeat_fractal.so once (after torch, whose HIP runtime it shares)."""
    global _libr
    if _libr is not None:
        return _libr
    with _lock:
        if _libr is not None:
            return _libr
        import torch  # noqa: F401  (the HIP runtime the library binds to)
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "pymhealth_amd: %s is not built. Build it with `make -C %s` or "
                "`python -c 'import __graft_entry__ as g; g.build()'`."
                % (LIB_PATH, os.path.join(_lib.HERE, "csrc")))
        L = ctypes.CDLL(LIB_PATH)
        i64, i32, vp, f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
        L.mhfr_version.restype = ctypes.c_int
        L.mhfr_version.argtypes = []
        L.mhfr_last_error.restype = ctypes.c_char_p
        L.mhfr_last_error.argtypes = []
        if L.mhfr_version() != MHFR_ABI_VERSION:
            raise ImportError("pymhealth_amd: %s has ABI %d, this package needs %d; rebuild it "
                              "(make -C %s)" % (LIB_PATH, L.mhfr_version(), MHFR_ABI_VERSION,
                                                os.path.join(_lib.HERE, "csrc")))
        L.mhfr_dfa_step.restype = i64
        L.mhfr_dfa_step.argtypes = [i64, f64]
        L.mhfr_dfa.restype = ctypes.c_int
        L.mhfr_dfa.argtypes = [vp, i32, i64, vp, vp, i64, i64, i64, vp, i32, i32, f64, i32, vp, i64, vp]
        L.mhfr_hurst.restype = ctypes.c_int
        L.mhfr_hurst.argtypes = [vp, i32, i64, vp, vp, i64, i64, i64, vp, i32, i32, vp, i64, vp]
        _libr = L
        return _libr


def check(rc):
    if rc != 0:
        msg = lib().mhfr_last_error().decode(errors="replace")
        raise ERRORS.get(rc, RuntimeError)("libmhfeat_fractal: %s (code %d)" % (msg, rc))
