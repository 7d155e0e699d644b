#!/usr/bin/env python3
"""Time the batched non-uniform FFT (mhfx_nufft1d1) on the MI355X.

Workload (default): 1e5 segments x 300 samples of one RR-like record, M = 256,
eps = 1e-15 (Mr = 768, so mhf_fft runs Bluestein over 2048 points), power output.

HIP events around each call on the current stream, after ``--warmup`` untimed calls; the
median, minimum and maximum of ``--runs`` (>= 10) calls are printed as one JSON line. The
workspace is allocated once, outside the timed region, as a caller of the C-ABI would.
``fft_ms`` is mhf_fft alone on a batch of the same grids, in the library's own batches;
the split into gridding / transform / deconvolution kernels comes from a kernel trace of
this script (``rocprofv3 --kernel-trace --stats -- python tools/nufft_time.py --runs 10``,
a run of its own: tracing slows the host), summed by kernel name.

There is no CPU path: without a GPU the script fails.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--segments", type=int, default=100000)
    ap.add_argument("--points", type=int, default=300)
    ap.add_argument("--M", type=int, default=256)
    ap.add_argument("--eps", type=float, default=1e-15)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--complex-out", action="store_true", help="complex128 rows, not |F|^2")
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs must be >= 10 (the median of fewer calls is not reported)")

    import torch
    if not torch.cuda.is_available():
        sys.exit("nufft_time: no GPU (torch.cuda.is_available() is False); nothing is measured")
    from pymhealth_amd import _lib, _lib_nufft
    L, LX = _lib.lib(), _lib_nufft.lib()

    # one record; segment b = points [b * step, b * step + points): overlapping RR windows
    rng = np.random.default_rng(0)
    step = 30
    n = (a.segments - 1) * step + a.points
    t = torch.from_numpy(np.cumsum(0.8 + 0.1 * rng.standard_normal(n))).cuda()
    c = torch.from_numpy(0.8 + 0.1 * rng.standard_normal(n)).cuda()
    starts = torch.arange(a.segments, dtype=torch.int64, device="cuda") * step
    ends = starts + a.points
    df = 2 * np.pi / 256
    out = torch.empty((a.segments, a.M), dtype=torch.complex128 if a.complex_out else torch.float64,
                      device="cuda")
    nws = LX.mhfx_nufft1d1_workspace(a.M, a.eps, a.segments)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731

    def call():
        _lib_nufft.check(LX.mhfx_nufft1d1(
            p(t), p(c), _lib_nufft.MHFX_DTYPE_F64, n, p(starts), p(ends), a.segments, 1, a.M, df,
            a.eps, 1, _lib_nufft.MHFX_OUT_COMPLEX if a.complex_out else _lib_nufft.MHFX_OUT_POWER,
            p(out), a.M, p(ws), nws, ctypes.c_void_p(stream)))

    # the transform alone: the same number of Mr-point rows, in the library's batches
    Msp, Mr, tau = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_double()
    LX.mhfx_nufft_grid_params(a.M, a.eps, ctypes.byref(Msp), ctypes.byref(Mr), ctypes.byref(tau))
    Mr = Mr.value
    batch = max(1, min(a.segments, (256 << 20) // (16 * Mr)))
    grids = torch.randn((batch, Mr), dtype=torch.complex128, device="cuda")
    nfw = L.mhf_fft_workspace(Mr, batch)
    fws = torch.empty(nfw, dtype=torch.uint8, device="cuda")

    def fft_only():
        for b0 in range(0, a.segments, batch):
            nb = min(batch, a.segments - b0)
            _lib.check(L.mhf_fft(p(grids), p(grids), Mr, nb, _lib.MHF_FFT_BACKWARD, 1.0 / Mr, p(fws),
                                 nfw, ctypes.c_void_p(stream)))

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    total, fft = timed(call), timed(fft_only)
    assert bool(torch.isfinite(out).all()), "non-finite output"
    med = float(np.median(total))
    print(json.dumps({
        "workload": "nufft1d1_segments", "segments": a.segments, "points": a.points, "M": a.M,
        "eps": a.eps, "Msp": Msp.value, "Mr": Mr, "out": "complex128" if a.complex_out else "power",
        "runs": a.runs, "warmup": a.warmup, "workspace_MiB": round(nws / 2 ** 20, 1),
        "total_ms": {"median": round(med, 3), "min": round(min(total), 3), "max": round(max(total), 3)},
        "fft_ms": {"median": round(float(np.median(fft)), 3), "min": round(min(fft), 3),
                   "max": round(max(fft), 3)},
        "segments_per_s": round(a.segments / (med * 1e-3)),
        "samples_per_s": round(a.segments * a.points / (med * 1e-3))}))


if __name__ == "__main__":
    main()
