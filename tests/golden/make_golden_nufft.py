#!/usr/bin/env python3
"""Generate the non-uniform FFT fixtures ``tests/golden/nufft_*.npz`` from the REFERENCE
itself (``mhealth.generic.frequency.nufft``, src/mhealth/generic/frequency/nufft.py).

Test infrastructure only, like ``make_golden.py``: run with the interpreter that has numba
and the reference's ``src`` directory on the path, under the same in-memory numba shim,
never on the GPU box::

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference>/src \
        python3.9 tests/golden/make_golden_nufft.py tests/golden

The reference's ``@jit`` functions fall back to object mode here (``np.fft`` has no numba
lowering), i.e. they run as the Python they are written as, on ``numpy.fft``.

Every case is the smallest shape at which one code path of the device version can go
wrong; each file holds the inputs, the arguments and the reference's output ``F``.
``LONG_N`` spans three of the gridding kernel's 1024-sample staging chunks plus a
remainder (kChunk, pymhealth_amd/csrc/nufft.hip).
"""
import os
import sys
import types
import warnings

import numpy as np

# ---------------------------------------------------------------- numba shim (in memory)
_m = types.ModuleType("numba.np.ufunc._internal")
_m.PyUFunc_None, _m.PyUFunc_Zero, _m.PyUFunc_One, _m.PyUFunc_ReorderableNone = -1, 0, 1, -2


class _DUFunc:  # placeholder type; DUFunc is never instantiated here
    pass


def _fromfunc(*a, **k):
    raise RuntimeError("numba ufunc builder unavailable under the shim")


_m._DUFunc, _m.fromfunc = _DUFunc, _fromfunc
sys.modules["numba.np.ufunc._internal"] = _m
np.MachAr = type("MachAr", (), {})
_real_version, np.__version__ = np.__version__, "1.20.3"
import numba  # noqa: E402,F401
np.__version__ = _real_version

warnings.simplefilter("ignore")
from mhealth.generic.frequency import nufft as ref  # noqa: E402

LONG_N = 3 * 1024 + 77


def rr_times(rng, n):
    """Beat times of an RR series of about 0.8 +- 0.1 s."""
    return np.cumsum(0.8 + 0.1 * rng.standard_normal(n))


def cases(rng):
    def cplx(n):
        return rng.standard_normal(n) + 1j * rng.standard_normal(n)
    t300 = rr_times(rng, 300)
    yield "rr300_m256", t300, rng.standard_normal(300), 256, 1.0, 1e-15, 1
    yield "cplx300_m256_neg", t300, cplx(300), 256, 1.0, 1e-15, -1
    yield "odd255_eps1e-6", t300, rng.standard_normal(300), 255, 1.0, 1e-6, 1
    yield "wrap_n2_m5", np.array([0.3, 5.9]), cplx(2), 5, 1.0, 1e-12, 1
    yield "n37_m16_df", rr_times(rng, 37), rng.standard_normal(37), 16, 0.5, 1e-15, 1
    yield "unsorted_neg", rng.uniform(-50, 50, 200), rng.standard_normal(200), 32, 1.0, 1e-15, 1
    yield "n1_m8", np.array([1.25]), np.array([0.75]), 8, 1.0, 1e-15, 1
    yield "on_grid", 2 * np.pi * np.arange(48) / 48, rng.standard_normal(48), 16, 1.0, 1e-15, 1
    yield "eps_coarse", rng.uniform(0, 20, 64), rng.standard_normal(64), 12, 1.0, 0.05, 1
    yield "m1024", t300, rng.standard_normal(300), 1024, 0.01, 1e-15, -1
    yield "m6000_n50", rr_times(rng, 50), rng.standard_normal(50), 6000, 0.001, 1e-15, 1
    yield "long_segment", rr_times(rng, LONG_N), rng.standard_normal(LONG_N), 16, 1.0, 1e-15, 1


def segments_case(rng):
    """One 2000-point record, 12 segments: overlapping ones, an empty one, one of length 2
    (below min_len = 3), one of length 1, one of 1500. Rows: the reference called per
    segment (zeros where it cannot be: the empty segment)."""
    n, M = 2000, 64
    x = rr_times(rng, n)
    c = 0.8 + 0.1 * rng.standard_normal(n)
    starts = np.array([0, 100, 150, 400, 400, 700, 900, 901, 250, 1000, 1990, 1700], np.int64)
    ends = np.array([300, 400, 450, 400, 402, 701, 1200, 1201, 1750, 1300, 2000, 2000], np.int64)
    F = np.zeros((len(starts), M), np.complex128)
    for b, (s, e) in enumerate(zip(starts, ends)):
        if e > s:
            F[b] = ref.nufft1d1(x[s:e], c[s:e], M, 1.0, 1e-15, 1)
    length = ends - starts
    return dict(x=x, c=c, starts=starts, ends=ends, M=M, df=1.0, eps=1e-15, iflag=1, F=F,
                min_len=3, nan_rows=length < 3, empty_rows=length <= 0)


def grid_param_table():
    pairs = [(2, 1e-15), (5, 1e-12), (8, 1e-15), (12, 0.05), (16, 1e-15), (16, 1e-6), (32, 1e-11),
             (32, 1.0000001e-11), (64, 9.9e-12), (64, 1e-10), (255, 1e-6), (256, 1e-15),
             (256, 1e-3), (1000, 1e-8), (1024, 1e-15), (1024, 1e-20), (4096, 1e-30), (6000, 1e-15),
             (7, 0.099), (3, 2e-33), (100003, 1e-13), (1 << 20, 1e-15)]
    rows = [ref._compute_grid_params(M, eps) for M, eps in pairs]
    return dict(M=np.array([p[0] for p in pairs], np.int64),
                eps=np.array([p[1] for p in pairs], np.float64),
                Msp=np.array([r[0] for r in rows], np.int64),
                Mr=np.array([r[1] for r in rows], np.int64),
                tau=np.array([r[2] for r in rows], np.float64))


def main(out_dir):
    rng = np.random.default_rng(20250307)
    for name, x, c, M, df, eps, iflag in cases(rng):
        F = ref.nufft1d1(x, c, M, df, eps, iflag)
        assert F.shape == (M,) and F.dtype == np.complex128
        np.savez_compressed(os.path.join(out_dir, "nufft_%s.npz" % name), x=x, c=c, M=M, df=df,
                            eps=eps, iflag=iflag, F=F)
    np.savez_compressed(os.path.join(out_dir, "nufft_segments.npz"), **segments_case(rng))
    np.savez_compressed(os.path.join(out_dir, "nufft_grid_params.npz"), **grid_param_table())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__)))
