"""GPU tests of detrended fluctuation analysis and the Hurst exponent (``timedom.dfa`` /
``timedom.hurst``, mhfr_dfa / mhfr_hurst of libmhfeat_fractal.so) against fixtures made by
running the reference itself (tests/golden/make_golden_fractal.py).

Bound: |dev - ref| <= 1e-11 absolute on exponents (values are O(1)) and 1e-11 x the
reference value on F(w) and tau. Rationale: the reference is within 2.3e-14 of a long-double
evaluation on these kinds of input (each fixture stores that value and is held to 1e-12 by
tests/test_fractal_host.py); a device result with a different but fixed fp64 summation order
over at most 16384 terms should land in the 1e-14 .. 1e-13 range; 1e-11 leaves about two
orders of margin for that and is still ten times tighter than the project's fp64-vs-reference
bar (1e-10, README float64 spectral row). ``o1fit`` / ``o1fit_multiple``: 1e-10 relative (the
uncentred normal-equation formula amplifies a reordered sum). Every test prints the figure
it asserts; DESIGN and the README row record the measured maxima.
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-11

DFA_CASES = ["rr300", "o2", "o3", "ov50", "ov12p5", "ov99", "o3_ov50", "n252", "n256", "n260",
             "n1025", "offset", "walk", "max_segment", "n4133", "len_eq_max_scale"]
HURST_CASES = ["n65", "rr300", "walk1024", "white300", "offset300", "custom_lags", "n4133"]


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    from pymhealth_amd import _lib_fractal, engine
    _lib_fractal.lib()
    return engine


def _file(name):
    return np.load(os.path.join(GOLDEN, "fractal_%s.npz" % name))


@pytest.fixture(scope="module")
def dfa_fx():
    return _file("dfa")


@pytest.fixture(scope="module")
def hurst_fx():
    return _file("hurst")


@pytest.fixture(scope="module")
def seg():
    d = _file("segments")
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def roll():
    d = _file("rolling")
    return {k: d[k] for k in d.files}


def _case(d, name):
    pre = name + "__"
    return {k[len(pre):]: (d[k] if d[k].ndim else d[k].item()) for k in d.files if k.startswith(pre)}


def _bits(t):
    """The int64 bit patterns of a float64 tensor or array (NaNs compare equal)."""
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    assert t.dtype == torch.float64
    return t.contiguous().view(torch.int64).cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------- DFA
@pytest.mark.parametrize("name", DFA_CASES)
def test_dfa_parity_with_reference(eng, dfa_fx, name):
    from pymhealth_amd.generic import timedom
    c = _case(dfa_fx, name)
    x = np.asarray(c["x"], np.float64)
    windows = [int(w) for w in c["windows"]]
    alpha = timedom.dfa(x, windows, c["o"], c["overlap"])
    F = eng.dfa(x, None, None, windows, c["o"], c["overlap"], fluctuations=True).cpu().numpy()[0]
    err_a = abs(alpha - c["alpha"])
    err_f = float(np.max(np.abs(F - c["F"]) / c["F"]))
    print("dfa %s: |d alpha| = %.3e, max |dF| / F = %.3e, |alpha - long double| = %.3e (reference: %.3e)"
          % (name, err_a, err_f, abs(alpha - c["ld"]), abs(c["alpha"] - c["ld"])))
    assert isinstance(alpha, float) and F.shape == (len(windows),)
    assert err_a <= TOL, (name, err_a)
    assert err_f <= TOL, (name, err_f)


def test_dfa_fixture_shapes_cover_the_paths(dfa_fx):
    """The fixtures are the shapes the kernel can go wrong at: 63 / 64 / 65 sub-windows (the
    wave boundary), one and two sub-windows, the smallest scale o + 2, a step clamped to 1, the
    longest segment the library takes and a length that is no multiple of the workgroup."""
    from pymhealth_amd import _lib_fractal, engine
    for n, k in ((252, 63), (256, 64), (260, 65)):
        assert (len(dfa_fx["n%d__x" % n]) - 4) // 4 + 1 == k
    assert len(dfa_fx["n1025__x"]) == 1025 and list(dfa_fx["n1025__windows"][-2:]) == [512, 1024]
    assert min(dfa_fx["o3__windows"]) == int(dfa_fx["o3__o"]) + 2 == 5
    assert engine.dfa_step(4, float(dfa_fx["ov99__overlap"])) == 1
    assert len(dfa_fx["max_segment__x"]) == _lib_fractal.MHFR_MAX_SEGMENT
    assert len(dfa_fx["n4133__x"]) % 256 != 0


def test_dfa_length_equal_to_largest_scale_and_one_less(eng, dfa_fx):
    c = _case(dfa_fx, "len_eq_max_scale")
    x, windows = c["x"], [int(w) for w in c["windows"]]
    assert len(x) == max(windows)
    st = torch.tensor([0, 0, 1], device="cuda")
    en = torch.tensor([64, 63, 64], device="cuda")
    out = eng.dfa(x, st, en, windows).cpu().numpy()
    assert abs(out[0] - c["alpha"]) <= TOL
    assert np.isnan(out[1]) and np.isnan(out[2])
    F = eng.dfa(x, st, en, windows, fluctuations=True).cpu().numpy()
    assert np.isfinite(F[0]).all() and np.isnan(F[1:]).all()


def test_segment_longer_than_max_len_is_nan_not_a_fault(eng, dfa_fx):
    """The C contract: max_len is the caller's bound; a segment that is in fact longer gives a
    NaN row (nothing is read or staged beyond max_len)."""
    import ctypes
    from pymhealth_amd import _lib_fractal
    L = _lib_fractal.lib()
    x = torch.from_numpy(np.asarray(dfa_fx["rr300__x"], np.float64)).cuda()
    st = torch.tensor([0, 0, 100], device="cuda")
    en = torch.tensor([300, 200, 300], device="cuda")
    sc = np.array([4, 8, 16, 32, 64], np.int64)
    lg = np.arange(2, 64).astype(np.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    _lib_fractal.check(L.mhfr_dfa(p(x), 1, 300, p(st), p(en), 3, 1, 200, sc.ctypes.data, 5, 1, 0.0,
                                  0, p(out[0]), 1, stream))
    _lib_fractal.check(L.mhfr_hurst(p(x), 1, 300, p(st), p(en), 3, 1, 200, lg.ctypes.data, 62, 0,
                                    p(out[1]), 1, stream))
    got = out.cpu().numpy()
    assert np.isnan(got[:, 0]).all() and np.isfinite(got[:, 1:]).all()
    assert abs(got[0, 1] - float(eng.dfa(x[:200], None, None, sc)[0])) == 0.0


def test_rows_do_not_depend_on_max_len(eng, seg):
    """max_len sizes the LDS and picks the profile's layout (padded above 1024 samples against
    bank conflicts); it moves addresses, not the order of any sum: the same bits for every
    max_len that admits the segment, on both sides of the layout threshold."""
    import ctypes
    import re
    from pymhealth_amd import _lib_fractal
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "pymhealth_amd", "csrc", "fractal.hip")).read()
    above = int(re.search(r"#define MHFR_PAD_ABOVE (\d+)", src).group(1))
    L = _lib_fractal.lib()
    x = torch.from_numpy(seg["x"].astype(np.float64)).cuda()
    st = torch.from_numpy(seg["starts"][:40]).cuda()
    en = torch.from_numpy(seg["ends"][:40]).cuda()
    sc = np.array([5, 8, 11, 16, 32, 64], np.int64)
    lg = np.arange(2, 64).astype(np.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = {}
    for max_len in (400, above, above + 1, 5000, _lib_fractal.MHFR_MAX_SEGMENT):
        for order, overlap in ((1, 0.0), (3, 50.0)):
            out = torch.zeros((40, 6), dtype=torch.float64, device="cuda")
            _lib_fractal.check(L.mhfr_dfa(p(x), 1, len(x), p(st), p(en), 40, 1, max_len, sc.ctypes.data,
                                          6, order, overlap, 1, p(out), 6, stream))
            rows.setdefault(("dfa", order), []).append(out)
        out = torch.zeros((40, 62), dtype=torch.float64, device="cuda")
        _lib_fractal.check(L.mhfr_hurst(p(x), 1, len(x), p(st), p(en), 40, 1, max_len, lg.ctypes.data,
                                        62, 1, p(out), 62, stream))
        rows.setdefault(("hurst", 0), []).append(out)
    for key, outs in rows.items():
        assert torch.isfinite(outs[0]).any(), key
        for o in outs[1:]:
            assert _same_bits(outs[0], o), key


def test_constant_and_nonfinite_segments_are_nan(eng):
    x = np.full(300, 812.0)
    y = np.random.default_rng(3).standard_normal(300)
    y[150] = np.nan
    z = y.copy()
    z[150] = np.inf
    for v in (x, y, z):
        assert np.isnan(float(eng.dfa(v, None, None, [4, 8, 16, 32])[0]))
        assert np.isnan(float(eng.hurst(v, None, None)[0]))
        assert np.isnan(eng.dfa(v, None, None, [4, 8, 16, 32], fluctuations=True).cpu().numpy()).all()
        assert np.isnan(eng.hurst(v, None, None, tau=True).cpu().numpy()).all()
    with pytest.raises(NotImplementedError, match="MHFR_MAX_SEGMENT"):
        eng.hurst(np.zeros(16385), None, None)
    with pytest.raises(ValueError, match=r"order \+ 2"):
        eng.dfa(y, None, None, [2, 8])


# ------------------------------------------------------------------------------- Hurst
@pytest.mark.parametrize("name", HURST_CASES)
def test_hurst_parity_with_reference(eng, hurst_fx, name):
    from pymhealth_amd.generic import timedom
    c = _case(hurst_fx, name)
    x = np.asarray(c["x"], np.float64)
    lags = None if c["default"] else [int(v) for v in c["lags"]]
    H = timedom.hurst(x) if lags is None else timedom.hurst(x, np.asarray(lags))
    tau = eng.hurst(x, None, None, lags, tau=True).cpu().numpy()[0]
    err_h = abs(H - c["H"])
    err_t = float(np.max(np.abs(tau - c["tau"]) / c["tau"]))
    print("hurst %s: |dH| = %.3e, max |d tau| / tau = %.3e, |H - long double| = %.3e (reference: %.3e)"
          % (name, err_h, err_t, abs(H - c["ld"]), abs(c["H"] - c["ld"])))
    assert isinstance(H, float) and tau.shape == (len(c["lags"]),)
    assert err_h <= TOL, (name, err_h)
    assert err_t <= TOL, (name, err_t)


def test_hurst_needs_largest_lag_plus_two(eng, hurst_fx):
    x = np.asarray(hurst_fx["n65__x"], np.float64)
    assert len(x) == 65
    out = eng.hurst(x, [0, 0, 1], [65, 64, 65]).cpu().numpy()
    assert abs(out[0] - float(hurst_fx["n65__H"])) <= TOL
    assert np.isnan(out[1]) and np.isnan(out[2])
    from pymhealth_amd.generic import timedom
    assert np.isnan(timedom.hurst(x[:64]))


# ------------------------------------------------------------------------------- both
def test_float32_record_gives_the_bits_of_its_float64_copy(eng, seg):
    x32 = seg["x"].astype(np.float32) + np.float32(0.37)
    x64 = x32.astype(np.float64)
    st, en = seg["starts"][:40], seg["ends"][:40]
    for f in (lambda x: eng.dfa(x, st, en, seg["dfa_windows"]),
              lambda x: eng.dfa(x, st, en, [5, 11, 16], 2, 50.0, fluctuations=True),
              lambda x: eng.hurst(x, st, en),
              lambda x: eng.hurst(x, st, en, tau=True)):
        a, b = f(x32), f(x64)
        assert torch.isfinite(a).any() and _same_bits(a, b)


def _nan_rows(seg, need, min_len):
    raw = seg["ends"] - seg["starts"]
    return (raw < max(min_len, 1)) | (seg["clipped"] < max(need, 1))


@pytest.mark.parametrize("min_len", [1, 100])
def test_segments_match_reference_rows(eng, seg, min_len):
    """About 300 segments of one record (negative and clipped bounds, overlapping, empty and
    too-short ones): every row within the bound of the reference's per-segment value, NaN rows
    exactly where the rules say."""
    x = seg["x"].astype(np.float64)
    windows = seg["dfa_windows"]
    a = eng.dfa(x, seg["starts"], seg["ends"], windows, min_len=min_len).cpu().numpy()
    F = eng.dfa(x, seg["starts"], seg["ends"], windows, min_len=min_len, fluctuations=True).cpu().numpy()
    h = eng.hurst(x, seg["starts"], seg["ends"], min_len=min_len).cpu().numpy()
    tau = eng.hurst(x, seg["starts"], seg["ends"], min_len=min_len, tau=True).cpu().numpy()
    nan_d = _nan_rows(seg, int(windows.max()), min_len)
    nan_h = _nan_rows(seg, 63 + 2, min_len)
    assert nan_d.any() and nan_h.any() and not nan_d.all()
    if min_len == 1:
        assert (nan_d != nan_h).any()          # the 64-sample segment: dfa finite, hurst NaN
    assert np.array_equal(np.isnan(a), nan_d) and np.array_equal(np.isnan(h), nan_h)
    assert np.array_equal(np.isnan(F).all(1), nan_d) and np.array_equal(np.isnan(F).any(1), nan_d)
    assert np.array_equal(np.isnan(tau).all(1), nan_h) and np.array_equal(np.isnan(tau).any(1), nan_h)
    # the fixture holds the reference wherever the slice admits it (min_len = 1)
    assert np.array_equal(np.isnan(seg["dfa"]), _nan_rows(seg, int(windows.max()), 1))
    assert np.array_equal(np.isnan(seg["hurst"]), _nan_rows(seg, 65, 1))
    ea = np.abs(a - seg["dfa"])[~nan_d].max()
    eh = np.abs(h - seg["hurst"])[~nan_h].max()
    ef = (np.abs(F - seg["dfa_F"]) / seg["dfa_F"])[~nan_d].max()
    rows = len(seg["hurst_tau"])
    keep = ~nan_h[:rows]
    et = (np.abs(tau[:rows] - seg["hurst_tau"]) / seg["hurst_tau"])[keep].max()
    print("segments min_len %d: |d alpha| %.3e, |dH| %.3e, |dF|/F %.3e, |d tau|/tau %.3e"
          % (min_len, ea, eh, ef, et))
    assert keep.sum() >= 10
    assert max(ea, eh, ef, et) <= TOL, (ea, eh, ef, et)


def test_rows_are_deterministic_and_batch_independent(eng, seg):
    """The same bits run to run, and alone (its own call, its own max_len) as inside the batch."""
    x = torch.from_numpy(seg["x"].astype(np.float64)).cuda()
    st, en = seg["starts"], seg["ends"]
    windows = seg["dfa_windows"]
    runs = [(eng.dfa(x, st, en, windows), eng.dfa(x, st, en, windows, fluctuations=True),
             eng.hurst(x, st, en), eng.hurst(x, st, en, tau=True)) for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert _same_bits(a, b)
    n = len(st)
    rows = sorted({0, n - 1, 5, 6, 7, 8, 11, 12, 13} | set(range(20, n, 23)))
    assert len(rows) >= 10
    finite = 0
    for b in rows:
        s1, e1 = st[b:b + 1], en[b:b + 1]
        alone = (eng.dfa(x, s1, e1, windows), eng.dfa(x, s1, e1, windows, fluctuations=True),
                 eng.hurst(x, s1, e1), eng.hurst(x, s1, e1, tau=True))
        for a, full in zip(alone, runs[0]):
            assert _same_bits(a, full[b:b + 1]), b
        finite += int(torch.isfinite(alone[0]).all())
        # and as a plain series: the slice itself, bounds None
        s, e, _ = slice(int(st[b]), int(en[b])).indices(len(x))
        if e > s and en[b] - st[b] >= 1:
            assert _same_bits(eng.hurst(x[s:e], None, None), runs[0][2][b:b + 1]), b
    assert finite >= 8


def test_rolling_apply_matches_reference_windows(eng, roll):
    from pymhealth_amd.generic import timedom
    from pymhealth_amd.util.windows import rolling_apply
    W, S = int(roll["W"]), int(roll["S"])
    x = roll["x"].astype(np.float64)
    fd = functools.partial(timedom.dfa, windows=[int(w) for w in roll["dfa_windows"]])
    h = rolling_apply(timedom.hurst, W, S)(x)
    d = rolling_apply(fd, W, S)(x)
    assert isinstance(h, np.ndarray) and h.dtype == np.float64 and h.shape == roll["hurst"].shape
    assert isinstance(d, np.ndarray) and d.dtype == np.float64 and d.shape == roll["dfa"].shape
    eh, ed = np.abs(h - roll["hurst"]).max(), np.abs(d - roll["dfa"]).max()
    print("rolling_apply: |dH| %.3e, |d alpha| %.3e over %d windows" % (eh, ed, len(h)))
    assert eh <= TOL and ed <= TOL
    xt = torch.from_numpy(x).cuda()
    ht, dt = rolling_apply(timedom.hurst, W, S)(xt), rolling_apply(fd, W, S)(xt)
    assert ht.is_cuda and dt.is_cuda and ht.dtype == torch.float64
    assert _same_bits(ht, h) and _same_bits(dt, d)
    # a float32 record: float64 output (np.zeros((nw,))), the value of its float64 copy
    h32 = rolling_apply(timedom.hurst, W, S)(x.astype(np.float32))
    assert h32.dtype == np.float64 and _same_bits(h32, h)       # whole milliseconds: exact in fp32
    assert rolling_apply(timedom.hurst, 2000, 64)(x).shape == (0,)


def test_mixed_list_and_dict(eng, roll):
    """[np.mean, hurst, dfa]: mean goes through its fused launch unchanged; each fractal feature
    equals its own single run, bit for bit."""
    from pymhealth_amd.generic import timedom
    from pymhealth_amd.util.windows import rolling_apply
    W, S = int(roll["W"]), int(roll["S"])
    x = roll["x"].astype(np.float64)
    fd = functools.partial(timedom.dfa, windows=[4, 8, 16, 32], o=2, overlap=50)
    m, h, d = rolling_apply([np.mean, timedom.hurst, fd], W, S)(x)
    assert _same_bits(m, rolling_apply(np.mean, W, S)(x))
    assert _same_bits(h, rolling_apply(timedom.hurst, W, S)(x))
    assert _same_bits(d, rolling_apply(fd, W, S)(x))
    assert np.abs(m - roll["mean"]).max() <= 1e-9
    out = rolling_apply({"mean": np.mean, "H": timedom.hurst, "alpha": fd}, W, S)(x)
    assert isinstance(out, dict) and list(out) == ["mean", "H", "alpha"]
    assert _same_bits(out["mean"], m) and _same_bits(out["H"], h) and _same_bits(out["alpha"], d)
    xt = torch.from_numpy(x).cuda()
    mt, ht, dt = rolling_apply((np.mean, timedom.hurst, fd), W, S)(xt)
    assert _same_bits(mt, m) and _same_bits(ht, h) and _same_bits(dt, d)


def test_nonuniform_rolling_apply_on_an_rr_index(eng, roll):
    """Windows of 90 s over beat times: NaN exactly in the windows with too few beats."""
    from pymhealth_amd.generic import timedom
    from pymhealth_amd.util.windows import indices_rolling_apply, nonuniform_rolling_apply
    x = roll["x"].astype(np.float64)
    got = nonuniform_rolling_apply(timedom.hurst)(roll["index"], x, int(roll["nu_wsize"]),
                                                  int(roll["nu_wstep"]))
    ref = roll["nu_hurst"]
    assert got.dtype == np.float64 and got.shape == ref.shape
    short = (roll["nu_ends"] - roll["nu_starts"]) < 65
    assert short.any() and np.array_equal(np.isnan(got), short) and np.array_equal(np.isnan(ref), short)
    err = np.abs(got - ref)[~short].max()
    print("nonuniform hurst: |dH| %.3e" % err)
    assert err <= TOL
    ind = np.stack([roll["nu_starts"], roll["nu_ends"]])
    m, h = nonuniform_rolling_apply([np.mean, timedom.hurst])(roll["index"], x, int(roll["nu_wsize"]),
                                                              int(roll["nu_wstep"]))
    assert _same_bits(h, got)
    assert _same_bits(m, indices_rolling_apply(np.mean)(ind, x))
    # min_window_len, and the record's dtype for a float32 record (np.zeros(n, arr.dtype))
    h100 = indices_rolling_apply(timedom.hurst, 100)(ind, x)
    assert np.array_equal(np.isnan(h100), (roll["nu_ends"] - roll["nu_starts"]) < 100)
    assert indices_rolling_apply(timedom.hurst)(ind, x.astype(np.float32)).dtype == np.float32


def test_o1fit_and_o1fit_multiple(eng):
    from pymhealth_amd.generic import timedom
    d = _file("o1fit")
    A, b = timedom.o1fit(d["x"], d["ys"][:, 0])
    assert isinstance(A, float) and isinstance(b, float)
    multi = timedom.o1fit_multiple(d["x"], d["ys"])
    assert isinstance(multi, np.ndarray) and multi.shape == (5, 2) and multi.dtype == np.float64
    e1 = np.abs(np.array([A, b]) - d["one"]) / np.abs(d["one"])
    em = np.abs(multi - d["multi"]) / np.abs(d["multi"])
    print("o1fit: max rel %.3e, o1fit_multiple: max rel %.3e" % (e1.max(), em.max()))
    assert e1.max() <= 1e-10 and em.max() <= 1e-10
    assert (np.abs(d["multi"] - d["multi_ld"]) <= 1e-12 * np.abs(d["multi_ld"])).all()
    mt = timedom.o1fit_multiple(torch.from_numpy(d["x"]).cuda(), torch.from_numpy(d["ys"]).cuda())
    assert mt.is_cuda and _same_bits(mt, multi)


def test_mhealth_alias_exposes_the_new_objects(eng, hurst_fx):
    import pymhealth_amd
    from pymhealth_amd.generic import timedom
    pymhealth_amd.install_mhealth_alias()
    import mhealth.generic.timedom as t
    assert t.dfa is timedom.dfa and t.hurst is timedom.hurst
    assert t.o1fit is timedom.o1fit and t.o1fit_multiple is timedom.o1fit_multiple
    x = np.asarray(hurst_fx["rr300__x"], np.float64)
    assert abs(t.hurst(x) - float(hurst_fx["rr300__H"])) <= TOL
