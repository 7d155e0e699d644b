/*
 * mhfeat_nufft.h — C-ABI of the companion library libmhfeat_nufft.so: the type-1
 * non-uniform FFT of irregularly sampled series on the MI355X.
 *
 * Replaces the reference's Gaussian-gridding NUFFT
 *
 *     nufft1d1(x, c, M, df=1.0, eps=1e-15, iflag=1)   src/mhealth/generic/frequency/nufft.py:79-99
 *
 *     F_k = (1/N) sum_j c_j exp(+-i k df x_j),   k = -(M//2) .. M - (M//2) - 1
 *
 * for one series or for many segments [starts[b], ends[b]) of one record in a single
 * call (RR-interval windows: the bounds of mhf_window_bounds plug in directly). Three
 * stages per call: the gridding kernel spreads every sample onto a fine grid of Mr cells
 * (nufft.py:55-76), mhf_fft of libmhfeat.so transforms the grids (the library links
 * against it; nothing of it is compiled twice), and the deconvolution kernel picks the M
 * bins and divides the Gaussian out (nufft.py:95-99).
 *
 * A library of its own, with its own ABI version: include/mhfeat.h and the exports of
 * libmhfeat.so are unchanged, so callers of MHF_ABI_VERSION 7 see no difference.
 *
 * Conventions, as in mhfeat.h: plain C types only; the caller owns every buffer, the
 * workspace included (device memory, 256-B aligned, sized by mhfx_nufft1d1_workspace(),
 * untouched until the stream reaches the end of the call); stream-ordered and
 * asynchronous, no host read-back; 0 on success or a negative MHFX_E* code, the message
 * of the last error on the calling thread from mhfx_last_error().
 */
#ifndef MHFEAT_NUFFT_H
#define MHFEAT_NUFFT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHFX_ABI_VERSION 1

/* Built with -fvisibility=hidden; only these entry points are exported. */
#if defined(__GNUC__) || defined(__clang__)
#define MHFX_API __attribute__((visibility("default")))
#else
#define MHFX_API
#endif

/* Error codes (the values of MHF_OK / MHF_EINVAL / MHF_EUNSUPPORTED / MHF_EDEVICE). */
#define MHFX_OK 0
#define MHFX_EINVAL (-1)
#define MHFX_EUNSUPPORTED (-2)
#define MHFX_EDEVICE (-3)

/* dtype of the weights c */
#define MHFX_DTYPE_F64 1    /* float64 (== MHF_DTYPE_F64)          */
#define MHFX_DTYPE_C128 4   /* complex128, interleaved (re, im)    */

/* what a row of `out` holds */
#define MHFX_OUT_COMPLEX 0  /* M complex128 values F_k             */
#define MHFX_OUT_POWER 1    /* M float64 values re(F_k)^2 + im(F_k)^2 */

MHFX_API int mhfx_version(void);
MHFX_API const char* mhfx_last_error(void);

/* _compute_grid_params(M, eps) (nufft.py:42-52) on the host: the half-width Msp of the
 * Gaussian in cells, the fine grid size Mr = max(ratio * M, 2 * Msp) and the Gaussian's
 * tau, ratio = 2 for eps > 1e-11 and 3 otherwise. MHFX_EINVAL unless 1e-33 < eps < 1e-1
 * (the reference's ValueError) and M >= 2 (for M = 1 the reference's slice Ftau[-0:]
 * returns Mr + 1 values); MHFX_EUNSUPPORTED when Mr exceeds mhf_fft's 2^30. Any output
 * pointer may be NULL. */
MHFX_API int mhfx_nufft_grid_params(int64_t M, double eps, int32_t* Msp, int64_t* Mr, double* tau);

/* Bytes of workspace mhfx_nufft1d1 needs for these arguments: the grids of as many
 * segments as are transformed at a time (all of them up to 256 MiB of grid, at least
 * one) plus mhf_fft_workspace() for that batch. -1 on arguments mhfx_nufft1d1 rejects. */
MHFX_API int64_t mhfx_nufft1d1_workspace(int64_t M, double eps, int64_t n_segments);

/* Type-1 NUFFT of n_segments segments of one record.
 *
 *   x            device, n_points float64 sample positions (any order, any sign).
 *   c            device, n_points weights: float64 (MHFX_DTYPE_F64) or complex128.
 *   starts, ends device int64 arrays of n_segments bounds: segment b is x[s:e], c[s:e]
 *                with Python slice semantics (negative counts from the end, clipped to
 *                [0, n_points]), the contract of mhf_indexed_window_features. Both NULL:
 *                one segment [0, n_points) (n_segments must be 1).
 *   min_len      a segment with ends[b] - starts[b] < min_len, or empty, gives a row of
 *                NaN (both parts); the reference raises ZeroDivisionError on empty input.
 *   M, df, eps   number of bins, frequency step and accuracy of nufft1d1; M >= 2.
 *   iflag        >= 0: exp(+i k df x) (numpy's ifft of the grid); < 0: exp(-i k df x).
 *   out          device; row b starts at element b * out_ld (elements: complex128 for
 *                MHFX_OUT_COMPLEX, float64 for MHFX_OUT_POWER), bins in nufftfreqs(M)
 *                order. out_ld >= M.
 *
 * Deterministic: a row is the same bits on every run, alone or inside any batch (gather
 * gridding, contributions added in sample order, no atomics). A sample position that is
 * not finite makes its row NaN (the reference raises). */
MHFX_API int mhfx_nufft1d1(const double* x, const void* c, int32_t c_dtype, int64_t n_points,
                           const int64_t* starts, const int64_t* ends, int64_t n_segments,
                           int64_t min_len, int64_t M, double df, double eps, int32_t iflag,
                           int32_t out_mode, void* out, int64_t out_ld, void* workspace,
                           int64_t workspace_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MHFEAT_NUFFT_H */
