/*
 * mhfeat_fractal.h — C-ABI of the companion library libmhfeat_fractal.so: the scaling
 * exponents of the reference's generic.timedom on the MI355X,
 *
 *     dfa(x, windows, o=1, overlap=0)        src/mhealth/generic/timedom.py:196-235
 *     hurst(x, lags=np.arange(2, 64))        src/mhealth/generic/timedom.py:238-259
 *
 * for one series or for many segments [starts[b], ends[b]) of one record in a single
 * call (fixed windows, or RR-interval windows: the bounds of mhf_window_bounds plug in
 * directly). One workgroup per segment, the segment in LDS, fp64 throughout.
 *
 * DFA: profile y = cumsum(x - mean(x)); for every scale w the sub-windows y[k s : k s + w],
 * k = 0 .. (N - w) // s with s = max(int(w (100 - overlap) / 100), 1), are detrended by a
 * least-squares polynomial of order o; F(w) = mean_k sqrt(rss_k / w) — the MEAN of the
 * per-window RMS values, as the reference computes it — and the result is the slope of
 * log F(w) against log w. Hurst: tau(l) = sqrt(std(x[l:] - x[:-l])) (population std; its
 * square root), result 2 b with b the gradient of o1fit(log l, log tau).
 *
 * A library of its own, with its own ABI version: include/mhfeat.h, include/mhfeat_nufft.h
 * and the exports of the other two libraries are unchanged.
 *
 * Conventions, as in mhfeat.h: plain C types only; the caller owns every buffer; no
 * workspace is needed and nothing is allocated; stream-ordered and asynchronous, no host
 * read-back; 0 on success or a negative MHFR_E* code, the message of the last error on
 * the calling thread from mhfr_last_error(). Every argument is checked before any launch.
 */
#ifndef MHFEAT_FRACTAL_H
#define MHFEAT_FRACTAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHFR_ABI_VERSION 1

/* Built with -fvisibility=hidden; only these entry points are exported. */
#if defined(__GNUC__) || defined(__clang__)
#define MHFR_API __attribute__((visibility("default")))
#else
#define MHFR_API
#endif

/* Error codes (the values of MHF_OK / MHF_EINVAL / MHF_EUNSUPPORTED / MHF_EDEVICE). */
#define MHFR_OK 0
#define MHFR_EINVAL (-1)
#define MHFR_EUNSUPPORTED (-2)
#define MHFR_EDEVICE (-3)

/* dtype of the record x (the values of MHF_DTYPE_F32 / MHF_DTYPE_F64). float32 samples
 * are widened exactly; all arithmetic is fp64, so a float32 record gives the bits of its
 * float64 copy. */
#define MHFR_DTYPE_F32 0
#define MHFR_DTYPE_F64 1

/* what a row of `out` holds */
#define MHFR_OUT_EXPONENT 0 /* one double: the scaling / Hurst exponent                   */
#define MHFR_OUT_FLUCT 1    /* n_scales doubles F(w) (dfa), n_lags doubles tau (hurst)    */

/* Limits. A segment lives in LDS as fp64, long ones padded by one double per 32 against
 * bank conflicts: 16384 samples are 132 KiB of the CU's 160 KiB, which leaves room for the
 * kernels' reduction scratch. */
#define MHFR_MAX_SEGMENT 16384
#define MHFR_MAX_SCALES 64
#define MHFR_MAX_LAGS 128

MHFR_API int mhfr_version(void);
MHFR_API const char* mhfr_last_error(void);

/* The step between sub-windows of scale w: max(int(w * (100 - overlap) / 100), 1), the
 * reference's expression in double arithmetic (timedom.py:226). -1 for w < 1 or an
 * overlap outside [0, 100). */
MHFR_API int64_t mhfr_dfa_step(int64_t scale, double overlap);

/* Common arguments of mhfr_dfa and mhfr_hurst.
 *
 *   x            device, n_points samples, contiguous, float32 or float64 (x_dtype).
 *   starts, ends device int64 arrays of n_segments bounds: segment b is x[s:e] with
 *                Python slice semantics (negative counts from the end, clipped to
 *                [0, n_points]), the contract of mhf_indexed_window_features. Both NULL:
 *                one segment [0, n_points) (n_segments must be 1).
 *   min_len      a segment with ends[b] - starts[b] < min_len, or empty, gives a NaN row.
 *   max_len      the caller's upper bound on the (clipped) segment length; it sizes the
 *                dynamic LDS. MHFR_EUNSUPPORTED above MHFR_MAX_SEGMENT. A segment that is
 *                in fact longer gives a NaN row; nothing is read out of bounds.
 *   out_mode     MHFR_OUT_EXPONENT or MHFR_OUT_FLUCT.
 *   out          device float64; row b starts at element b * out_ld. out_ld >= the row
 *                length (1, or n_scales / n_lags).
 *
 * NaN rows (every element of the row): a segment shorter than the largest scale (dfa: the
 * reference raises) or than the largest lag + 2 (hurst: at lag + 1 the one difference has
 * std 0 and the reference returns a non-finite value); any F(w) or tau that is zero or
 * not finite (a constant segment); a sample that is not finite.
 *
 * Deterministic: a row is the same bits on every run, alone or inside any batch, and for
 * any max_len that admits it (fixed workgroup shape, fixed summation orders, no atomics). */

/* Detrended fluctuation analysis.
 *   scales       HOST array of n_scales window sizes, 2 <= n_scales <= MHFR_MAX_SCALES,
 *                every scale >= order + 2 (below that the reference's lstsq returns no
 *                residual).
 *   order        of the detrending polynomial, 1..3.
 *   overlap      percentage overlap between sub-windows, in [0, 100). */
MHFR_API int mhfr_dfa(const void* x, int32_t x_dtype, int64_t n_points, const int64_t* starts,
                      const int64_t* ends, int64_t n_segments, int64_t min_len, int64_t max_len,
                      const int64_t* scales, int32_t n_scales, int32_t order, double overlap,
                      int32_t out_mode, double* out, int64_t out_ld, void* hip_stream);

/* Hurst exponent.
 *   lags         HOST array of n_lags time lags, 2 <= n_lags <= MHFR_MAX_LAGS, every
 *                lag >= 1 (the reference's default: 2 .. 63). */
MHFR_API int mhfr_hurst(const void* x, int32_t x_dtype, int64_t n_points, const int64_t* starts,
                        const int64_t* ends, int64_t n_segments, int64_t min_len, int64_t max_len,
                        const int64_t* lags, int32_t n_lags, int32_t out_mode, double* out,
                        int64_t out_ld, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MHFEAT_FRACTAL_H */
