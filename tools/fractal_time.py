#!/usr/bin/env python3
"""Time the batched DFA and Hurst kernels (mhfr_dfa / mhfr_hurst) on the MI355X.

Workloads:
  A (default)  1e5 segments x 300 samples of one RR-like record (overlapping windows, step
               30), DFA scales 4 .. 64 (12 of them), order 1, overlap 0; default Hurst lags.
  B (--workload B)  1e4 segments x 4096 samples (step 512), the same scales and lags.
  --segments / --points / --step describe another workload of the same kind ("custom").

HIP events around each call on the current stream, after ``--warmup`` untimed calls; the
median, minimum and maximum of ``--runs`` (>= 10) calls are printed as one JSON line per
workload, with the cost model of DESIGN (fp64 operations and LDS reads of the fitting loops)
and the rate it implies. ``--lib PATH`` times another build of the library (e.g. one
compiled with -DMHFR_PAD_ABOVE=0) with the same script.

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

SCALES = [4, 5, 6, 8, 10, 13, 16, 20, 25, 32, 45, 64]
WORKLOADS = {"A": (100000, 300, 30), "B": (10000, 4096, 512)}


def dfa_model(points, scales, order, overlap, dfa_step):
    """fp64 operations and LDS reads (8 B each) of one segment's fitting loops: per sample of
    a sub-window, pass 1 is 1 read, order + 1 multiply-adds and the basis recurrence, pass 2
    1 read, the same basis, the fit and the squared residual."""
    basis = {1: 1, 2: 3, 3: 6}[order]                 # flops to get t and p2, p3
    per = 2 * (basis + 2 * (order + 1)) + 3           # both passes + (y - fit)^2 accumulate
    samples = 0
    for w in scales:
        s = dfa_step(w, overlap)
        samples += ((points - w) // s + 1) * w
    return samples * per, samples * 2


def hurst_model(points, lags):
    """Pass 1: 2 reads, 2 flops per difference; pass 2: 2 reads, 4 flops."""
    diffs = sum(points - l for l in lags)
    return diffs * 6, diffs * 4


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workload", choices=["A", "B", "both"], default="both")
    ap.add_argument("--segments", type=int, default=None)
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--order", type=int, default=1)
    ap.add_argument("--overlap", type=float, default=0.0)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libmhfeat_fractal.so to time")
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs must be >= 10 (the median of fewer calls is not reported)")

    import torch
    if not torch.cuda.is_available():
        sys.exit("fractal_time: no GPU (torch.cuda.is_available() is False); nothing is measured")
    from pymhealth_amd import _lib_fractal, engine
    if a.lib:
        _lib_fractal.LIB_PATH = os.path.abspath(a.lib)
    L = _lib_fractal.lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    scales = np.array(SCALES, np.int64)
    lags = np.arange(2, 64).astype(np.int64)

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

    names = ["A", "B"] if a.workload == "both" else [a.workload]
    if a.segments or a.points:
        if not (a.segments and a.points) or a.points > _lib_fractal.MHFR_MAX_SEGMENT:
            ap.error("a custom workload needs --segments and --points (<= MHFR_MAX_SEGMENT)")
        WORKLOADS["custom"] = (a.segments, a.points, a.step or max(a.points // 8, 1))
        names = ["custom"]
    for name in names:
        segments, points, step = WORKLOADS[name]
        rng = np.random.default_rng(0)
        n = (segments - 1) * step + points
        x = torch.from_numpy(800 + 50 * np.sin(np.arange(n) * 0.3) + 20 * rng.standard_normal(n)).cuda()
        starts = torch.arange(segments, dtype=torch.int64, device="cuda") * step
        ends = starts + points
        out = torch.empty(segments, dtype=torch.float64, device="cuda")

        def dfa():
            _lib_fractal.check(L.mhfr_dfa(p(x), _lib_fractal.MHFR_DTYPE_F64, n, p(starts), p(ends),
                                          segments, 1, points, scales.ctypes.data, len(scales), a.order,
                                          a.overlap, _lib_fractal.MHFR_OUT_EXPONENT, p(out), 1,
                                          ctypes.c_void_p(stream)))

        def hurst():
            _lib_fractal.check(L.mhfr_hurst(p(x), _lib_fractal.MHFR_DTYPE_F64, n, p(starts), p(ends),
                                            segments, 1, points, lags.ctypes.data, len(lags),
                                            _lib_fractal.MHFR_OUT_EXPONENT, p(out), 1,
                                            ctypes.c_void_p(stream)))

        res = {"workload": name, "segments": segments, "points": points, "scales": SCALES,
               "order": a.order, "overlap": a.overlap, "runs": a.runs, "warmup": a.warmup,
               "lib": os.path.relpath(_lib_fractal.LIB_PATH, ROOT)}
        for key, fn, model in (("dfa", dfa, dfa_model(points, SCALES, a.order, a.overlap, engine.dfa_step)),
                               ("hurst", hurst, hurst_model(points, lags))):
            ms = timed(fn)
            assert bool(torch.isfinite(out).all()), "non-finite output"
            med = float(np.median(ms))
            flops, reads = model
            res[key] = {"ms": {"median": round(med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3)},
                        "segments_per_s": round(segments / (med * 1e-3)),
                        "model_gflop": round(segments * flops / 1e9, 2),
                        "model_lds_gb": round(segments * reads * 8 / 1e9, 2),
                        "tflops_fp64": round(segments * flops / (med * 1e-3) / 1e12, 3),
                        "lds_tb_per_s": round(segments * reads * 8 / (med * 1e-3) / 1e12, 3)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
