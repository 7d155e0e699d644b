#!/usr/bin/env python3
"""Generate the DFA / Hurst fixtures ``tests/golden/fractal_*.npz`` from the REFERENCE
itself (``mhealth.generic.timedom``, src/mhealth/generic/timedom.py:196-299).

Test infrastructure only, like ``make_golden_nufft.py``: run with the interpreter that has
numba and the reference's ``src`` directory on the path, under the same in-memory numba
shim, never on the GPU box::

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference>/src \
        python3.9 tests/golden/make_golden_fractal.py tests/golden

Every value is the reference's own function on float64 input; the ``@jit`` ones are called
through ``.py_func`` where the object is a numba dispatcher, i.e. as the Python they are
written as. ``dfa`` keeps F(w) in a closure: it is captured by wrapping ``np.polyfit``
during the call and recording the ``y`` of the final degree-1 fit (log F); the same wrap
of ``o1fit`` records log tau of ``hurst``.

Conditioning check: every case is also evaluated by a long-double restatement (Gram-Schmidt
residuals, centred slope); the generator stores that value and asserts
``|ref - longdouble| <= 1e-12``. A case that fails is ill-conditioned and must be replaced
by another one; the cap is never widened.

Inputs are stored as what they are made from where that is smaller: a series that is a
sum of integer-valued parts is kept as int16 / int32 and widened by the tests, so that the
longest record (MHFR_MAX_SEGMENT samples) stays well under 100 KB.
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
from mhealth.generic import timedom as ref  # noqa: E402

MAX_SEGMENT = 16384          # include/mhfeat_fractal.h MHFR_MAX_SEGMENT
CAP = 1e-12
LD = np.longdouble
DEFAULT_LAGS = np.arange(2, 64)
TAU_ROWS = 40


def _py(f):
    return getattr(f, "py_func", f)


# o1fit_multiple and hurst call the module's o1fit: as written, not as compiled
ref.o1fit = _py(ref.o1fit)


# ---------------------------------------------------------------- the reference, with F / tau
def ref_dfa(x, windows, o=1, overlap=0):
    """(exponent, F) of the reference's dfa: F from the y of its final np.polyfit."""
    seen = []
    real = np.polyfit

    def spy(px, py, deg, *a, **k):
        if deg == 1 and np.ndim(py) == 1 and not k.get("full"):
            seen.append(np.array(py, dtype=np.float64))
        return real(px, py, deg, *a, **k)

    np.polyfit = spy
    try:
        alpha = float(_py(ref.dfa)(x, windows, o, overlap))
    finally:
        np.polyfit = real
    assert len(seen) == 1 and len(seen[0]) == len(windows)
    return alpha, np.exp(seen[0])


def ref_hurst(x, lags=None):
    """(H, tau) of the reference's hurst: tau from the y its o1fit receives."""
    seen = []
    real = ref.o1fit

    def spy(px, py):
        seen.append(np.array(py, dtype=np.float64))
        return _py(real)(px, py)

    ref.o1fit = spy
    try:
        h = float(_py(ref.hurst)(x) if lags is None else _py(ref.hurst)(x, np.asarray(lags)))
    finally:
        ref.o1fit = real
    assert len(seen) == 1
    return h, np.exp(seen[0])


# ---------------------------------------------------------------- long-double restatements
def ld_dfa(x, windows, o=1, overlap=0):
    x = x.astype(LD)
    xp = np.cumsum(x - x.mean())
    N = len(xp)
    F = []
    for w in windows:
        s = max(int(w * (100 - overlap) / 100), 1)
        t = (np.arange(w).astype(LD) - LD(w - 1) / 2) / LD(w)
        Q = []
        for k in range(o + 1):
            v = t ** k
            for _ in range(2):
                for q in Q:
                    v = v - (q @ v) * q
            Q.append(v / np.sqrt(v @ v))
        nseg = (N - w) // s + 1
        acc = LD(0)
        for k in range(nseg):
            y = xp[k * s:k * s + w]
            r = y.copy()
            for q in Q:
                r = r - (q @ y) * q
            acc += np.sqrt((r @ r) / w)
        F.append(acc / nseg)
    lw = np.log(np.array(windows, dtype=LD))
    lf = np.log(np.array(F, dtype=LD))
    lw0 = lw - lw.mean()
    return float((lw0 @ (lf - lf.mean())) / (lw0 @ lw0))


def ld_hurst(x, lags=None):
    lags = DEFAULT_LAGS if lags is None else np.asarray(lags)
    x = x.astype(LD)
    tau = []
    for l in lags:
        d = x[l:] - x[:-l]
        d = d - d.mean()
        tau.append(np.sqrt(np.sqrt((d @ d) / len(d))))
    lx = np.log(lags.astype(LD))
    ly = np.log(np.array(tau, dtype=LD))
    lx0 = lx - lx.mean()
    return float(2 * (lx0 @ (ly - ly.mean())) / (lx0 @ lx0))


def ld_o1fit(x, y):
    x, y = x.astype(LD), y.astype(LD)
    x0 = x - x.mean()
    b = (x0 @ (y - y.mean())) / (x0 @ x0)
    return float(y.mean() - b * x.mean()), float(b)


# ---------------------------------------------------------------- inputs
def rr_ms(rng, n):
    """RR intervals in whole milliseconds (a respiratory swing plus noise around 800 ms)."""
    return np.round(800 + 50 * np.sin(np.arange(n) * 0.3) + 20 * rng.standard_normal(n)).astype(np.int16)


def walk_int(rng, n):
    """A random walk of integer steps (-3 .. 3)."""
    return np.cumsum(rng.integers(-3, 4, n)).astype(np.int32)


def dfa_cases(rng):
    """name -> (x, windows, o, overlap); each the smallest shape that takes one path."""
    rr = rr_ms(rng, 300)
    c = {"rr300": (rr, [4, 8, 16, 32, 64], 1, 0),
         "o2": (rr, [5, 11, 16, 32], 2, 0),
         "o3": (rr, [5, 11, 16, 32], 3, 0),
         "ov50": (rr, [4, 8, 16, 32, 64], 1, 50),
         "ov12p5": (rr, [4, 8, 16, 32, 64], 1, 12.5),
         "ov99": (rr, [4, 8, 16, 32], 1, 99),
         "o3_ov50": (rr, [5, 11, 16, 32], 3, 50)}
    for n in (252, 256, 260):          # 63 / 64 / 65 sub-windows of scale 4: the wave boundary
        c["n%d" % n] = (rng.standard_normal(n), [4, 8], 1, 0)
    c["n1025"] = (walk_int(rng, 1025), [16, 512, 1024], 1, 0)     # 1024: one sub-window, 512: two
    c["offset"] = (1e4 + rng.standard_normal(300), [4, 8, 16, 32, 64], 1, 0)
    c["walk"] = (walk_int(rng, 1024), [4, 8, 16, 32, 64, 128], 2, 0)
    c["max_segment"] = (rr_ms(rng, MAX_SEGMENT), [4, 16, 64, 256, 1024], 1, 0)
    c["n4133"] = (rr_ms(rng, 4133), [4, 8, 16, 32, 64], 1, 0)     # not a multiple of the block
    c["len_eq_max_scale"] = (rng.standard_normal(64), [4, 8, 16, 32, 64], 1, 0)
    return c


def hurst_cases(rng):
    """name -> (x, lags or None)."""
    c = {"n65": (rng.standard_normal(65), None),           # two elements at lag 63
         "rr300": (rr_ms(rng, 300), None),
         "walk1024": (walk_int(rng, 1024), None),
         "white300": (rng.standard_normal(300), None),
         "offset300": (1e4 + rng.standard_normal(300), None),
         "custom_lags": (walk_int(rng, 300), [1, 2, 4, 8, 16]),
         "n4133": (rr_ms(rng, 4133), None)}
    return c


def segments_case(rng):
    """One record of 6000 samples, about 300 segments of length 40 .. 400 with negative and
    clipped bounds, overlapping, empty and too-short ones. Rows hold the reference's value on
    the Python slice x[s:e]; NaN where the rules of include/mhfeat_fractal.h say so."""
    n, nseg = 6000, 300
    x = rr_ms(rng, n)
    xf = x.astype(np.float64)
    length = rng.integers(40, 401, nseg)
    starts = rng.integers(0, n - 400, nseg)
    ends = starts + length
    starts[0], ends[0] = 0, 300
    starts[-1], ends[-1] = n - 350, n
    starts[5], ends[5] = -400, -100           # negative bounds
    starts[6], ends[6] = n - 200, n + 500     # clipped at the end: 200 samples
    starts[7], ends[7] = -7000, 150           # clipped at the start: 150 samples (raw length 7150)
    starts[8], ends[8] = 1000, 1000           # empty
    starts[9], ends[9] = 1200, 1100           # end before start
    starts[10], ends[10] = 2000, 2020         # too short for every feature
    starts[11], ends[11] = 2000, 2064         # 64: dfa finite, hurst NaN (needs 65)
    starts[12], ends[12] = 2000, 2065         # 65: both finite
    starts[13], ends[13] = 2000, 2063         # 63: both NaN
    starts[14], ends[14] = 3000, 3090         # below min_len = 100
    dfa_w, min_len = [4, 8, 16, 32, 64], 100
    dfa = np.full(nseg, np.nan)
    F = np.full((nseg, len(dfa_w)), np.nan)
    hurst = np.full(nseg, np.nan)
    tau = np.full((TAU_ROWS, len(DEFAULT_LAGS)), np.nan)    # of the first rows only (file size)
    dfa_ld, hurst_ld = dfa.copy(), hurst.copy()
    clipped = np.zeros(nseg, np.int64)
    for b, (s, e) in enumerate(zip(starts, ends)):
        seg = xf[int(s):int(e)]
        clipped[b] = len(seg)
        if e - s < 1 or len(seg) == 0:
            continue
        if len(seg) >= max(dfa_w):
            dfa[b], F[b] = ref_dfa(seg, dfa_w)
            dfa_ld[b] = ld_dfa(seg, dfa_w)
        if len(seg) >= DEFAULT_LAGS.max() + 2:
            hurst[b], t = ref_hurst(seg)
            if b < TAU_ROWS:
                tau[b] = t
            hurst_ld[b] = ld_hurst(seg)
    raw = ends - starts
    short = raw < min_len                      # rows that min_len = 100 turns into NaN
    return dict(x=x, starts=starts.astype(np.int64), ends=ends.astype(np.int64), clipped=clipped,
                dfa_windows=np.array(dfa_w, np.int64), dfa=dfa, dfa_F=F, dfa_ld=dfa_ld,
                hurst=hurst, hurst_tau=tau, hurst_ld=hurst_ld, min_len=min_len, short=short)


def rolling_case(rng):
    """rolling_apply(., 128, 64) and nonuniform windows over one record: the reference's value
    per window."""
    n, W, S = 1500, 128, 64
    x = rr_ms(rng, n)
    xf = x.astype(np.float64)
    dfa_w = [4, 8, 16, 32]
    nw = 1 + (n - W) // S
    dfa = np.array([ref_dfa(xf[i * S:i * S + W], dfa_w)[0] for i in range(nw)])
    hurst = np.array([ref_hurst(xf[i * S:i * S + W])[0] for i in range(nw)])
    dfa_ld = np.array([ld_dfa(xf[i * S:i * S + W], dfa_w) for i in range(nw)])
    hurst_ld = np.array([ld_hurst(xf[i * S:i * S + W]) for i in range(nw)])
    mean = np.array([xf[i * S:i * S + W].mean() for i in range(nw)])
    # an RR index: beat times in ms; windows of 90 s every 45 s hold about 112 beats, fewer
    # across a gap of missing beats
    t = np.cumsum(x.astype(np.int64))
    t[700:] += 60000
    t[1100:] += 80000
    nu_w, nu_s = 90000, 45000
    begin = np.arange(t[0], t[-1], nu_s)
    si = np.searchsorted(t, begin, "left")
    ei = np.searchsorted(t, begin + nu_w, "left")
    nu = np.full(len(begin), np.nan)
    nu_ld = nu.copy()
    for i, (s, e) in enumerate(zip(si, ei)):
        if e - s >= DEFAULT_LAGS.max() + 2:
            nu[i] = ref_hurst(xf[s:e])[0]
            nu_ld[i] = ld_hurst(xf[s:e])
    assert np.isnan(nu).any() and np.isfinite(nu).sum() >= 5
    return dict(x=x, W=W, S=S, dfa_windows=np.array(dfa_w, np.int64), dfa=dfa, hurst=hurst,
                dfa_ld=dfa_ld, hurst_ld=hurst_ld, mean=mean, index=t, nu_wsize=nu_w, nu_wstep=nu_s,
                nu_starts=si.astype(np.int64), nu_ends=ei.astype(np.int64), nu_hurst=nu, nu_hurst_ld=nu_ld)


def o1fit_case(rng):
    x = np.log(np.arange(2, 64))
    ys = np.stack([(0.3 + 0.1 * k) * x + 0.5 * k + 0.05 * rng.standard_normal(len(x))
                   for k in range(5)], 1)
    one = np.array(_py(ref.o1fit)(x, ys[:, 0]), np.float64)
    multi = np.asarray(_py(ref.o1fit_multiple)(x, ys), np.float64)
    ld = np.array([ld_o1fit(x, ys[:, k]) for k in range(ys.shape[1])])
    assert multi.shape == (5, 2) and (np.abs(multi - ld) <= CAP * np.abs(ld)).all()
    assert (one == multi[0]).all()
    return dict(x=x, ys=ys, one=one, multi=multi, multi_ld=ld)


def main(out_dir):
    rng = np.random.default_rng(20251019)
    d = {}
    for name, (x, windows, o, overlap) in dfa_cases(rng).items():
        xf = np.asarray(x, np.float64)
        alpha, F = ref_dfa(xf, windows, o, overlap)
        ld = ld_dfa(xf, windows, o, overlap)
        assert np.isfinite(alpha) and abs(alpha - ld) <= CAP, (name, alpha, ld)
        d.update({name + "__x": x, name + "__windows": np.array(windows, np.int64), name + "__o": o,
                  name + "__overlap": float(overlap), name + "__alpha": alpha, name + "__F": F,
                  name + "__ld": ld})
    np.savez_compressed(os.path.join(out_dir, "fractal_dfa.npz"), **d)
    d = {}
    for name, (x, lags) in hurst_cases(rng).items():
        xf = np.asarray(x, np.float64)
        h, tau = ref_hurst(xf, lags)
        ld = ld_hurst(xf, lags)
        assert np.isfinite(h) and abs(h - ld) <= CAP, (name, h, ld)
        d.update({name + "__x": x, name + "__lags": np.asarray(DEFAULT_LAGS if lags is None else lags, np.int64),
                  name + "__default": lags is None, name + "__H": h, name + "__tau": tau, name + "__ld": ld})
    np.savez_compressed(os.path.join(out_dir, "fractal_hurst.npz"), **d)
    for name, case in (("segments", segments_case(rng)), ("rolling", rolling_case(rng))):
        for k in [k for k in case if k.endswith("_ld")]:
            a, b = case[k[:-3]], case[k]
            ok = np.isfinite(a)
            assert (np.isfinite(b) == ok).all() and (np.abs(a[ok] - b[ok]) <= CAP).all(), (name, k)
        np.savez_compressed(os.path.join(out_dir, "fractal_%s.npz" % name), **case)
    np.savez_compressed(os.path.join(out_dir, "fractal_o1fit.npz"), **o1fit_case(rng))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__)))
