"""ctypes binding of libmhfeat_nufft.so (include/mhfeat_nufft.h), the companion library
that holds the non-uniform FFT.

Like ``_lib``: one compute path, the HIP kernels of the library. If it is missing, or no
GPU is visible, the entry points raise — there is no CPU fallback. The library is linked
against libmhfeat.so (``mhf_fft``), which is loaded first.
"""
import ctypes
import os
import threading

from . import _lib

LIB_PATH = os.path.join(_lib.HERE, "libmhfeat_nufft.so")

MHFX_ABI_VERSION = 1   # include/mhfeat_nufft.h MHFX_ABI_VERSION
MHFX_DTYPE_F64 = 1
MHFX_DTYPE_C128 = 4
MHFX_OUT_COMPLEX = 0
MHFX_OUT_POWER = 1

ERRORS = _lib.ERRORS

EXPORTS = ("mhfx_version", "mhfx_last_error", "mhfx_nufft_grid_params",
           "mhfx_nufft1d1_workspace", "mhfx_nufft1d1")

_lock = threading.Lock()
_libx = None


def lib():
    """Load libmhfeat_nufft.so once (after libmhfeat.so, and so after torch)."""
    global _libx
    if _libx is not None:
        return _libx
    with _lock:
        if _libx is not None:
            return _libx
        _lib.lib()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "pymhealth_amd: %s is not built. Build it with `make -C %s` or "
                "`python -c 'import __graft_entry__ as g; g.build()'`."
                % (LIB_PATH, os.path.join(_lib.HERE, "csrc")))
        L = ctypes.CDLL(LIB_PATH)
        i64, i32, vp, f64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
        L.mhfx_version.restype = ctypes.c_int
        L.mhfx_version.argtypes = []
        L.mhfx_last_error.restype = ctypes.c_char_p
        L.mhfx_last_error.argtypes = []
        if L.mhfx_version() != MHFX_ABI_VERSION:
            raise ImportError("pymhealth_amd: %s has ABI %d, this package needs %d; rebuild it "
                              "(make -C %s)" % (LIB_PATH, L.mhfx_version(), MHFX_ABI_VERSION,
                                                os.path.join(_lib.HERE, "csrc")))
        L.mhfx_nufft_grid_params.restype = ctypes.c_int
        L.mhfx_nufft_grid_params.argtypes = [i64, f64, ctypes.POINTER(i32), ctypes.POINTER(i64),
                                             ctypes.POINTER(f64)]
        L.mhfx_nufft1d1_workspace.restype = i64
        L.mhfx_nufft1d1_workspace.argtypes = [i64, f64, i64]
        L.mhfx_nufft1d1.restype = ctypes.c_int
        L.mhfx_nufft1d1.argtypes = [vp, vp, i32, i64, vp, vp, i64, i64, i64, f64, f64, i32, i32,
                                    vp, i64, vp, i64, vp]
        _libx = L
        return _libx


def check(rc):
    if rc != 0:
        msg = lib().mhfx_last_error().decode(errors="replace")
        raise ERRORS.get(rc, RuntimeError)("libmhfeat_nufft: %s (code %d)" % (msg, rc))
