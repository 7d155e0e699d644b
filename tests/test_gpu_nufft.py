"""GPU tests of the non-uniform FFT (``generic.frequency.nufft``, mhfx_nufft1d1) against
fixtures made by running the reference itself (tests/golden/make_golden_nufft.py).

Bound: max |F_dev - F_ref| <= 1e-12 x max |F_ref| per row — the project's bound for its fp64
transform against the reference's (README, mhf_fft row). A reordered fp64 restatement of
the algorithm on the CPU (gather in sample order, closed-form exponentials, numpy's FFT)
differs from the reference by at most 1.1e-15 x max |F_ref| over these cases, and the
device FFT (Bluestein for Mr = 3 M) adds its own rounding, so the bound has margin but
is not loose. Power: |F|^2 has twice the relative error: 2e-12 x max |F_ref|^2.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-12
CASES = ["rr300_m256", "cplx300_m256_neg", "odd255_eps1e-6", "wrap_n2_m5", "n37_m16_df",
         "unsorted_neg", "n1_m8", "on_grid", "eps_coarse", "m1024", "m6000_n50", "long_segment"]


@pytest.fixture(scope="module")
def nf():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    from pymhealth_amd import _lib_nufft
    _lib_nufft.lib()
    from pymhealth_amd.generic.frequency import nufft
    return nufft


def _load(name):
    d = np.load(os.path.join(GOLDEN, "nufft_%s.npz" % name))
    return {k: (d[k] if d[k].ndim else d[k].item()) for k in d.files}


@pytest.fixture(scope="module")
def seg():
    return _load("segments")


def _bits(t):
    """The int64 bit patterns of a float64 / complex128 tensor or array (NaN compare equal)."""
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int64).cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rel(F, ref):
    return float(np.abs(F - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", CASES)
def test_parity_with_reference(nf, name):
    d = _load(name)
    F = nf.nufft1d1(d["x"], d["c"], d["M"], d["df"], d["eps"], d["iflag"])
    assert isinstance(F, np.ndarray) and F.dtype == np.complex128 and F.shape == (d["M"],)
    err = _rel(F, d["F"])
    print("nufft %s: max|dF| / max|F| = %.3e" % (name, err))
    assert err <= TOL, (name, err)


def test_long_segment_spans_staging_chunks():
    """The fixture's length is 3 staging chunks of the gridding kernel plus a remainder."""
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "pymhealth_amd", "csrc", "nufft.hip")).read()
    import re
    chunk = int(re.search(r"constexpr int kChunk = (\d+);", src).group(1))
    n = len(_load("long_segment")["x"])
    assert n >= 3 * chunk and n % chunk != 0


@pytest.mark.parametrize("min_len", [3, 1])
def test_segments_match_reference_rows(nf, seg, min_len):
    """Row b = the reference called on segment b; NaN rows (both parts) are exactly the empty
    segment and those shorter than min_len."""
    length = seg["ends"] - seg["starts"]
    nan_rows = seg["nan_rows"] if min_len == seg["min_len"] else seg["empty_rows"]
    assert (nan_rows == ((length < min_len) | (length <= 0))).all()
    assert nan_rows.any() and seg["empty_rows"].any() and (length == 1).any() and (length == 1500).any()
    F = nf.nufft1d1_segments(seg["x"], seg["c"], seg["starts"], seg["ends"], seg["M"], seg["df"],
                             seg["eps"], seg["iflag"], min_len=min_len)
    assert isinstance(F, np.ndarray) and F.dtype == np.complex128
    assert F.shape == (len(length), seg["M"])
    assert (np.isnan(F.real).all(axis=1) == nan_rows).all()
    assert (np.isnan(F.imag).all(axis=1) == nan_rows).all()
    assert not np.isnan(F[~nan_rows].view(np.float64)).any()
    for b in np.nonzero(~nan_rows)[0]:
        err = _rel(F[b], seg["F"][b])
        print("nufft segments row %d (len %d): %.3e" % (b, length[b], err))
        assert err <= TOL, (b, err)


def test_deterministic_and_batch_independent(nf, seg):
    """The same bits run to run, and every row of a batch equals the single-segment call on
    its slice bit for bit."""
    dev = "cuda"
    x, c = torch.from_numpy(seg["x"]).to(dev), torch.from_numpy(seg["c"]).to(dev)
    args = (seg["M"], seg["df"], seg["eps"], seg["iflag"])
    A = nf.nufft1d1_segments(x, c, seg["starts"], seg["ends"], *args)
    B = nf.nufft1d1_segments(x, c, seg["starts"], seg["ends"], *args)
    assert A.is_cuda and A.dtype == torch.complex128 and _same_bits(A, B)
    for b, (s, e) in enumerate(zip(seg["starts"].tolist(), seg["ends"].tolist())):
        if e > s:
            assert _same_bits(A[b], nf.nufft1d1(x[s:e], c[s:e], *args)), b
    # a row does not depend on its position in the batch, nor on the batch
    perm = np.arange(len(seg["starts"]))[::-1].copy()
    P = nf.nufft1d1_segments(x, c, seg["starts"][perm], seg["ends"][perm], *args)
    assert _same_bits(P, A[torch.from_numpy(perm).to(dev)])

    d = _load("rr300_m256")
    x, c = torch.from_numpy(d["x"]).to(dev), torch.from_numpy(d["c"]).to(dev)
    args = (d["M"], d["df"], d["eps"], d["iflag"])
    one = nf.nufft1d1(x, c, *args)
    assert _same_bits(one, nf.nufft1d1(x, c, *args))
    starts, ends = np.array([0, 10, 0, 150, 0]), np.array([300, 200, 150, 300, 300])
    R = nf.nufft1d1_segments(x, c, starts, ends, *args)
    assert _same_bits(R[0], one) and _same_bits(R[4], one)
    for b in (1, 2, 3):
        assert _same_bits(R[b], nf.nufft1d1(x[starts[b]:ends[b]], c[starts[b]:ends[b]], *args)), b


def test_power_mode(nf, seg):
    args = (seg["x"], seg["c"], seg["starts"], seg["ends"], seg["M"], seg["df"], seg["eps"], seg["iflag"])
    F = nf.nufft1d1_segments(*args, min_len=3)
    P = nf.nufft1d1_segments(*args, min_len=3, power=True)
    assert P.dtype == np.float64 and P.shape == F.shape
    assert _same_bits(P, F.real * F.real + F.imag * F.imag)
    keep = ~seg["nan_rows"]
    assert (np.isnan(P).all(axis=1) == seg["nan_rows"]).all()
    for b in np.nonzero(keep)[0]:
        ref = np.abs(seg["F"][b]) ** 2
        err = float(np.abs(P[b] - ref).max() / ref.max())
        print("nufft power row %d: %.3e" % (b, err))
        assert err <= 2 * TOL, (b, err)


def test_input_kinds(nf):
    d = _load("n37_m16_df")
    args = (d["M"], d["df"], d["eps"], d["iflag"])
    x, c = d["x"], d["c"]
    base = nf.nufft1d1(x, c, *args)
    xt, ct = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    T = nf.nufft1d1(xt, ct, *args)
    assert T.is_cuda and T.dtype == torch.complex128 and _same_bits(T, base)
    # float32 and integer positions / weights: computed on their float64 widening
    x32, c32 = x.astype(np.float32), c.astype(np.float32)
    assert _same_bits(nf.nufft1d1(x32, c32, *args),
                      nf.nufft1d1(x32.astype(np.float64), c32.astype(np.float64), *args))
    ticks = (x * 1000).astype(np.int64)
    assert _same_bits(nf.nufft1d1(ticks, c, d["M"], 1e-3), nf.nufft1d1(ticks.astype(np.float64), c, d["M"], 1e-3))
    assert _same_bits(nf.nufft1d1(torch.from_numpy(ticks).cuda(), ct, d["M"], 1e-3),
                      nf.nufft1d1(ticks.astype(np.float64), c, d["M"], 1e-3))
    dt = ticks.astype("datetime64[ms]")
    assert _same_bits(nf.nufft1d1(dt, c, d["M"], 1e-3), nf.nufft1d1(ticks.astype(np.float64), c, d["M"], 1e-3))
    # complex64 weights widen to complex128
    cc = (c + 1j * c[::-1]).astype(np.complex64)
    assert _same_bits(nf.nufft1d1(x, cc, *args), nf.nufft1d1(x, cc.astype(np.complex128), *args))
    # a side stream
    from pymhealth_amd import engine
    s = torch.cuda.Stream()
    S = engine.nufft1d1(xt, ct, None, None, *args, stream=s.cuda_stream)
    s.synchronize()
    assert _same_bits(S[0], base)
    with pytest.raises(ZeroDivisionError):
        nf.nufft1d1(xt[:0], ct[:0], 8)


def test_rr_band_power_end_to_end(nf):
    """RR windows -> nufft1d1_segments(power=True) -> spectrum.peak_frequency / power_band,
    all on the device, against an fp64 direct sum on the CPU."""
    from pymhealth_amd import spectrum
    n, M, df = 1500, 256, 2 * np.pi / 200          # bins 1/200 Hz apart, up to 0.64 Hz
    t, rr = np.empty(n), np.empty(n)
    now = 0.0
    for i in range(n):   # 0.1 Hz (LF) modulation and a weaker 0.25 Hz (HF) one
        rr[i] = 0.8 + 0.05 * np.sin(2 * np.pi * 0.1 * now) + 0.02 * np.sin(2 * np.pi * 0.25 * now)
        now += rr[i]
        t[i] = now
    c = rr - rr.mean()
    starts = np.arange(0, n - 300 + 1, 100)
    ends = starts + 300
    k = np.arange(1, M - M // 2)                   # the positive-frequency bins
    freqs = nf.nufftfreqs(M, df) / (2 * np.pi)
    pos = slice(M // 2 + 1, M)
    assert np.array_equal(nf.nufftfreqs(M)[pos], k)
    direct = np.empty((len(starts), len(k)))
    for b, (s, e) in enumerate(zip(starts, ends)):
        direct[b] = np.abs(np.exp(1j * np.outer(k * df, t[s:e])) @ c[s:e] / (e - s)) ** 2
    top2 = np.sort(direct, axis=1)[:, -2:]
    assert (top2[:, 1] >= 1.01 * top2[:, 0]).all()          # no near-tie at the top
    want_peak = freqs[pos][direct.argmax(axis=1)]
    assert np.allclose(want_peak, 0.1)

    P = nf.nufft1d1_segments(torch.from_numpy(t).cuda(), torch.from_numpy(c).cuda(), starts, ends,
                             M, df, power=True)
    assert P.is_cuda and P.shape == (len(starts), M)
    fpos = torch.from_numpy(freqs[pos].copy()).cuda()
    peak = spectrum.peak_frequency(P[:, pos], fpos).cpu().numpy()
    assert np.array_equal(peak, want_peak)
    for lo, hi in ((0.04, 0.15), (0.15, 0.4)):
        band = spectrum.power_band(P[:, pos], fpos, lo, hi).cpu().numpy()
        want = direct[:, (freqs[pos] >= lo) & (freqs[pos] <= hi)].sum(axis=1)
        # every bin within 2e-12 x the row's largest power; at most 50 bins in a band
        assert (np.abs(band - want) <= 50 * 2 * TOL * direct.max(axis=1)).all()
    lf = spectrum.power_band(P[:, pos], fpos, 0.04, 0.15).cpu().numpy()
    hf = spectrum.power_band(P[:, pos], fpos, 0.15, 0.4).cpu().numpy()
    assert (lf > 2 * hf).all()
