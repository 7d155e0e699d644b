"""Drop-in for ``mhealth.generic.frequency.nufft`` (nufft.py:36-99): the type-1
non-uniform FFT of irregularly sampled series (an RR tachogram, phone-sensor samples)

    F_k = (1/N) sum_j c_j exp(+-i k df x_j),   k = nufftfreqs(M)

on the MI355X (``mhfx_nufft1d1``, include/mhfeat_nufft.h: gather gridding, ``mhf_fft``,
deconvolution; pymhealth_amd/csrc/nufft.hip).

``nufft1d1(x, c, M, df, eps, iflag)`` keeps the reference's signature: numpy in gives a
complex128 numpy array, a CUDA tensor in gives a CUDA tensor. ``nufft1d1_segments`` is
the batched form for windows of one record: row b is ``nufft1d1(x[s:e], c[s:e], ...)``
for the bounds ``util.windows.get_indices`` yields, in one device call; with
``power=True`` it returns ``|F|^2``, ready for ``spectrum.power_band`` /
``peak_frequency`` with ``freqs = nufftfreqs(M, df) / (2 pi)``.

``x`` is computed in float64: integer or datetime ticks and float32 are widened first.
(On float32 ``x`` the reference computes ``x * df`` and the wrapped positions in fp32,
so this drop-in is the more accurate of the two there.)
"""
import numpy as np

_EPS_MSG = "eps must satisfy 1e-33 < eps < 1e-1."


def nufftfreqs(M, df=1):
    """The frequency range used in nufft for M frequency bins (nufft.py:36-39)."""
    return df * np.arange(-(M // 2), M - (M // 2))


def _compute_grid_params(M, eps):
    """(Msp, Mr, tau) from eps following Dutt & Rokhlin (nufft.py:42-52)."""
    if eps <= 1E-33 or eps >= 1E-1:
        raise ValueError(_EPS_MSG)
    ratio = 2 if eps > 1E-11 else 3
    Msp = int(-np.log(eps) / (np.pi * (ratio - 1) / (ratio - 0.5)) + 0.5)
    Mr = max(ratio * M, 2 * Msp)
    lambda_ = Msp / (ratio * (ratio - 0.5))
    tau = np.pi * lambda_ / M ** 2
    return Msp, Mr, tau


def _check(x, c, M, eps):
    if not (1E-33 < eps < 1E-1):
        raise ValueError(_EPS_MSG)
    if int(M) < 2:
        # the reference's Ftau[-(M // 2):] is the whole grid for M = 1 (Mr + 1 values out)
        raise ValueError("M must be >= 2")
    if len(x) != len(c):
        raise ValueError("x and c must have the same length")


def _hand_back(out, *arrs):
    """numpy in, numpy out; a tensor among the inputs: a tensor on the first one's device."""
    import torch
    for a in arrs:
        if isinstance(a, torch.Tensor):
            return out if out.device == a.device else out.to(a.device)
    return out.cpu().numpy()


def nufft1d1(x, c, M, df=1.0, eps=1E-15, iflag=1):
    """Fast non-uniform Fourier transform, type 1 (nufft.py:79-99): complex128, length M,
    bins in ``nufftfreqs(M, df)`` order; ``iflag >= 0`` gives exp(+i k x)."""
    _check(x, c, M, eps)
    if len(x) == 0:
        raise ZeroDivisionError("division by zero")    # the reference's 1 / N
    from ...engine import nufft1d1 as dev
    out = dev(x, c, None, None, M, df, eps, iflag)[0]
    return _hand_back(out, x, c)


def nufft1d1_segments(x, c, starts, ends, M, df=1.0, eps=1E-15, iflag=1, min_len=1,
                      power=False):
    """``nufft1d1(x[s:e], c[s:e], M, df, eps, iflag)`` for every segment ``(s, e)`` of
    ``zip(starts, ends)`` in one device call: a ``(B, M)`` array, complex128 or, with
    ``power``, float64 ``|F|^2``. An empty segment, or one shorter than ``min_len``, is a
    row of NaN (the indexed-window convention, util.windows.indices_rolling_apply)."""
    _check(x, c, M, eps)
    from ...engine import nufft1d1 as dev
    out = dev(x, c, starts, ends, M, df, eps, iflag, min_len=min_len, power=power)
    return _hand_back(out, x, c)


__all__ = ["nufftfreqs", "nufft1d1", "nufft1d1_segments"]
