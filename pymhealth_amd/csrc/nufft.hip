// nufft.hip — libmhfeat_nufft.so: the type-1 non-uniform FFT of include/mhfeat_nufft.h.
//
// The reference (src/mhealth/generic/frequency/nufft.py:36-99) spreads every sample onto a
// fine grid of Mr cells with a Gaussian of half-width Msp cells (build_grid_fast, a serial
// scatter), transforms the grid (numpy ifft, or fft / Mr) and divides the Gaussian's
// transform out of the M central bins.
//
// MI355X form, fp64 throughout, three stream-ordered stages per batch of segments:
//   * nufft_grid_kernel — the scatter restated as a GATHER, so that it needs no atomics and
//     every cell is summed in one fixed order. One workgroup per (segment, block of cells).
//     The workgroup stages the segment's samples in LDS in chunks of kChunk (wrapped
//     position, base cell, weight: 28 B per sample); each lane owns cells g = g_lo + lane,
//     + 256, ... and walks the staged samples in index order: sample p with base cell m
//     contributes to g iff (g - m) mod Mr is in [-Msp, Msp - 1], with weight
//     exp(-(xi - j hx)^2 / (4 tau)) — the closed form of the reference's E1 E2^j E3[|j|].
//     A cell's sum therefore depends on nothing but its segment's samples: the same bits on
//     every run, in any batch and under any split of the cells over workgroups.
//   * mhf_fft (libmhfeat.so, linked — fft.hip is not compiled twice) on the grids in place,
//     1 / Mr folded into its `scale`.
//   * nufft_deconv_kernel — bins k = -(M // 2) .. M - (M // 2) - 1 from Ftau[k mod Mr], times
//     (1 / N) sqrt(pi / tau) exp(tau k^2); complex128 or re^2 + im^2.
// Built with -ffp-contract=off like the rest of the product: the power output is then the
// plain product-sum of the complex output, bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/mhfeat.h"
#include "../../include/mhfeat_nufft.h"

namespace mhfx {
namespace {

typedef double2 cplx;

constexpr int kThreads = 256;
constexpr int kChunk = 1024;                       // samples staged in LDS at a time (28 KiB)
constexpr int kMaxCellsPerBlock = 4096;            // 16 cells per lane
constexpr int64_t kGridBytes = int64_t(256) << 20; // grids transformed at a time
constexpr int64_t kMaxMr = int64_t(1) << 30;       // mhf_fft's limit

thread_local char g_err[512] = "";

int set_error(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

// numpy's float divmod (npy_divmod) for b > 0: the remainder has b's sign (Python `%`), the
// quotient is the floor. The reference applies it twice per sample (nufft.py:66-67).
__device__ __forceinline__ void np_divmod(double a, double b, double* q, double* r) {
    double mod = fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0) {
        if (mod < 0.0) {
            mod += b;
            div -= 1.0;
        }
    } else {
        mod = 0.0;
    }
    double fl;
    if (div != 0.0) {
        fl = floor(div);
        if (div - fl > 0.5) fl += 1.0;
    } else {
        fl = copysign(0.0, a / b);
    }
    *q = fl;
    *r = mod;
}

// arr[s:e] of n samples: Python slice bounds (mhf_indexed_window_features' contract)
__device__ __forceinline__ bool segment_bounds(const int64_t* starts, const int64_t* ends, int64_t seg,
                                               int64_t n, int64_t min_len, int64_t* s0, int64_t* e0) {
    const int64_t si = starts ? starts[seg] : 0, ei = starts ? ends[seg] : n;
    int64_t s = si < 0 ? si + n : si, e = ei < 0 ? ei + n : ei;
    s = s < 0 ? 0 : (s > n ? n : s);
    e = e < 0 ? 0 : (e > n ? n : e);
    *s0 = s;
    *e0 = e;
    return (ei - si >= min_len) && e > s;
}

struct GridArgs {
    const double* x;
    const double* c;          // float64, or interleaved complex128
    const int64_t* starts;
    const int64_t* ends;
    int64_t n_points, min_len, seg0;
    cplx* ftau;               // (segments of this batch) x Mr
    int32_t Mr, Msp, cells_per_block, cell_blocks;
    double df, hx, q4;        // hx = 2 pi / Mr, q4 = 0.25 / tau
};

template <bool kComplex>
__global__ void __launch_bounds__(kThreads) nufft_grid_kernel(GridArgs a) {
    __shared__ double s_xi[kChunk];
    __shared__ double s_cr[kChunk];
    __shared__ double s_ci[kComplex ? kChunk : 1];
    __shared__ int32_t s_m[kChunk];
    const int64_t b = blockIdx.x / a.cell_blocks;
    const int32_t cb = static_cast<int32_t>(blockIdx.x - b * a.cell_blocks);
    const int32_t Mr = a.Mr, Msp = a.Msp;
    const int32_t g_lo = cb * a.cells_per_block;
    const int32_t g_hi = g_lo + a.cells_per_block < Mr ? g_lo + a.cells_per_block : Mr;
    cplx* row = a.ftau + b * Mr;
    int64_t s0, e0;
    const bool keep = segment_bounds(a.starts, a.ends, a.seg0 + b, a.n_points, a.min_len, &s0, &e0);
    if (!keep) {   // the deconvolution writes NaN; the transform still reads the row
        for (int32_t g = g_lo + threadIdx.x; g < g_hi; g += kThreads) row[g] = cplx{0.0, 0.0};
        return;
    }
    const double two_pi = 2.0 * M_PI;
    for (int64_t p0 = s0; p0 < e0; p0 += kChunk) {
        const int32_t cnt = e0 - p0 < kChunk ? static_cast<int32_t>(e0 - p0) : kChunk;
        for (int32_t i = threadIdx.x; i < cnt; i += kThreads) {
            double q, xi, unused;
            np_divmod(a.x[p0 + i] * a.df, two_pi, &unused, &xi);   // xi = (x df) % 2 pi, in [0, 2 pi]
            np_divmod(xi, a.hx, &q, &unused);                      // q = xi // hx
            if (!(q >= 0.0 && q <= static_cast<double>(Mr))) q = 0.0;   // non-finite x: NaN weights below
            const int32_t m = 1 + static_cast<int32_t>(q);              // 1 .. Mr + 1
            s_xi[i] = xi - a.hx * static_cast<double>(m);
            s_m[i] = m >= Mr ? m - Mr : m;                              // m mod Mr
            if (kComplex) {
                s_cr[i] = a.c[2 * (p0 + i)];
                s_ci[i] = a.c[2 * (p0 + i) + 1];
            } else {
                s_cr[i] = a.c[p0 + i];
            }
        }
        __syncthreads();
        for (int32_t g = g_lo + threadIdx.x; g < g_hi; g += kThreads) {
            cplx acc = p0 == s0 ? cplx{0.0, 0.0} : row[g];
            for (int32_t p = 0; p < cnt; ++p) {
                int32_t t = g - s_m[p] + Msp;        // (g - m + Msp) mod Mr, one wrap either way
                t += t < 0 ? Mr : 0;
                t -= t >= Mr ? Mr : 0;
                if (t < 2 * Msp) {
                    const double d = s_xi[p] - static_cast<double>(t - Msp) * a.hx;
                    const double w = exp(-(d * d) * a.q4);
                    acc.x += s_cr[p] * w;
                    if (kComplex) acc.y += s_ci[p] * w;
                }
            }
            row[g] = acc;
        }
        __syncthreads();
    }
}

struct DeconvArgs {
    const cplx* ftau;
    const int64_t* starts;
    const int64_t* ends;
    int64_t n_points, min_len, seg0, nseg, M, Mr;
    double tau, sq;           // sq = sqrt(pi / tau)
    void* out;
    int64_t out_ld;
    int32_t power;
};

__global__ void __launch_bounds__(kThreads) nufft_deconv_kernel(DeconvArgs a) {
    const int64_t total = a.nseg * a.M;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t b = i / a.M, t = i - b * a.M;
        int64_t s0, e0;
        const bool keep = segment_bounds(a.starts, a.ends, a.seg0 + b, a.n_points, a.min_len, &s0, &e0);
        double re = __builtin_nan(""), im = re;
        if (keep) {
            const int64_t k = t - a.M / 2;
            const cplx F = a.ftau[b * a.Mr + (k < 0 ? k + a.Mr : k)];
            // (1 / N) * sqrt(pi / tau) * exp(tau * k ** 2) * Ftau2, left to right (nufft.py:99)
            const double f = ((1.0 / static_cast<double>(e0 - s0)) * a.sq) *
                             exp(a.tau * static_cast<double>(k * k));
            re = F.x * f;
            im = F.y * f;
        }
        const int64_t at = (a.seg0 + b) * a.out_ld + t;
        if (a.power) static_cast<double*>(a.out)[at] = re * re + im * im;
        else static_cast<cplx*>(a.out)[at] = cplx{re, im};
    }
}

int64_t round256(int64_t b) { return (b + 255) & ~int64_t(255); }

struct Plan {
    int32_t Msp;
    int64_t Mr, segs, grid_bytes, fft_bytes;   // segs: segments transformed at a time
    double tau;
};

int grid_params(int64_t M, double eps, int32_t* Msp, int64_t* Mr, double* tau) {
    if (!(eps > 1e-33 && eps < 1e-1)) return set_error(MHFX_EINVAL, "eps must satisfy 1e-33 < eps < 1e-1.");
    if (M < 2) return set_error(MHFX_EINVAL, "M must be >= 2");
    if (M > kMaxMr) return set_error(MHFX_EUNSUPPORTED, "the fine grid must have at most 2^30 cells");
    const int ratio = eps > 1e-11 ? 2 : 3;
    const int32_t msp = static_cast<int32_t>(-log(eps) / (M_PI * (ratio - 1) / (ratio - 0.5)) + 0.5);
    const int64_t mr = ratio * M > 2 * msp ? ratio * M : 2 * msp;
    if (mr > kMaxMr) return set_error(MHFX_EUNSUPPORTED, "the fine grid must have at most 2^30 cells");
    const double lambda = msp / (ratio * (ratio - 0.5));
    if (Msp) *Msp = msp;
    if (Mr) *Mr = mr;
    if (tau) *tau = M_PI * lambda / static_cast<double>(M * M);
    return MHFX_OK;
}

int make_plan(int64_t M, double eps, int64_t n_segments, Plan* p) {
    if (n_segments < 0) return set_error(MHFX_EINVAL, "n_segments must be >= 0");
    const int rc = grid_params(M, eps, &p->Msp, &p->Mr, &p->tau);
    if (rc != MHFX_OK) return rc;
    int64_t segs = kGridBytes / (p->Mr * static_cast<int64_t>(sizeof(cplx)));
    if (segs < 1) segs = 1;
    if (segs > n_segments) segs = n_segments;
    p->segs = segs;
    p->grid_bytes = round256(segs * p->Mr * static_cast<int64_t>(sizeof(cplx)));
    p->fft_bytes = segs > 0 ? mhf_fft_workspace(p->Mr, segs) : 0;
    if (p->fft_bytes < 0) return set_error(MHFX_EUNSUPPORTED, "mhf_fft_workspace rejects this grid size");
    return MHFX_OK;
}

}  // namespace
}  // namespace mhfx

using namespace mhfx;

extern "C" int mhfx_version(void) { return MHFX_ABI_VERSION; }

extern "C" const char* mhfx_last_error(void) { return g_err; }

extern "C" int mhfx_nufft_grid_params(int64_t M, double eps, int32_t* Msp, int64_t* Mr, double* tau) {
    set_error(MHFX_OK, "");
    return grid_params(M, eps, Msp, Mr, tau);
}

extern "C" int64_t mhfx_nufft1d1_workspace(int64_t M, double eps, int64_t n_segments) {
    set_error(MHFX_OK, "");
    Plan p;
    if (make_plan(M, eps, n_segments, &p) != MHFX_OK) return -1;
    return n_segments == 0 ? 0 : p.grid_bytes + round256(p.fft_bytes);
}

extern "C" int mhfx_nufft1d1(const double* x, const void* c, int32_t c_dtype, int64_t n_points,
                             const int64_t* starts, const int64_t* ends, int64_t n_segments,
                             int64_t min_len, int64_t M, double df, double eps, int32_t iflag,
                             int32_t out_mode, void* out, int64_t out_ld, void* workspace,
                             int64_t workspace_bytes, void* hip_stream) {
    set_error(MHFX_OK, "");
    Plan p;
    const int prc = make_plan(M, eps, n_segments, &p);
    if (prc != MHFX_OK) return prc;
    if (c_dtype != MHFX_DTYPE_F64 && c_dtype != MHFX_DTYPE_C128)
        return set_error(MHFX_EINVAL, "c_dtype must be MHFX_DTYPE_F64 or MHFX_DTYPE_C128");
    if (out_mode != MHFX_OUT_COMPLEX && out_mode != MHFX_OUT_POWER)
        return set_error(MHFX_EINVAL, "out_mode must be MHFX_OUT_COMPLEX or MHFX_OUT_POWER");
    if (n_points < 0) return set_error(MHFX_EINVAL, "n_points must be >= 0");
    if ((starts == nullptr) != (ends == nullptr))
        return set_error(MHFX_EINVAL, "starts and ends must both be given, or both be NULL");
    if (!starts && n_segments > 1)
        return set_error(MHFX_EINVAL, "n_segments must be 1 when starts and ends are NULL");
    if (!(df == df) || std::isinf(df)) return set_error(MHFX_EINVAL, "df must be finite");
    if (n_segments == 0) return MHFX_OK;
    if (out_ld < M) return set_error(MHFX_EINVAL, "out_ld must be >= M (elements between rows of out)");
    if (!out) return set_error(MHFX_EINVAL, "null out");
    if (n_points > 0 && (!x || !c)) return set_error(MHFX_EINVAL, "null x or c");
    const int64_t need = p.grid_bytes + round256(p.fft_bytes);
    if (!workspace || workspace_bytes < need) {
        char msg[160];
        snprintf(msg, sizeof(msg), "nufft workspace too small: %lld bytes needed "
                 "(mhfx_nufft1d1_workspace), %lld given", (long long)need, (long long)workspace_bytes);
        return set_error(MHFX_EINVAL, msg);
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 15)
        return set_error(MHFX_EINVAL, "workspace must be 16-byte aligned");

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    cplx* ftau = static_cast<cplx*>(workspace);
    void* fft_ws = static_cast<char*>(workspace) + p.grid_bytes;
    const int32_t Mr = static_cast<int32_t>(p.Mr);
    for (int64_t seg0 = 0; seg0 < n_segments; seg0 += p.segs) {
        const int64_t nb = n_segments - seg0 < p.segs ? n_segments - seg0 : p.segs;
        // cells per workgroup: up to 16 per lane; fewer when that leaves the chip idle (a
        // cell's sum does not depend on which workgroup owns it)
        int32_t cpb = kMaxCellsPerBlock;
        while (cpb > kThreads && nb * ((Mr + cpb - 1) / cpb) < 1024) cpb /= 2;
        GridArgs g;
        g.x = x;
        g.c = static_cast<const double*>(c);
        g.starts = starts;
        g.ends = ends;
        g.n_points = n_points;
        g.min_len = min_len;
        g.seg0 = seg0;
        g.ftau = ftau;
        g.Mr = Mr;
        g.Msp = p.Msp;
        g.cells_per_block = cpb;
        g.cell_blocks = (Mr + cpb - 1) / cpb;
        g.df = df;
        g.hx = 2 * M_PI / static_cast<double>(p.Mr);
        g.q4 = 0.25 / p.tau;
        const unsigned blocks = static_cast<unsigned>(nb * g.cell_blocks);
        if (c_dtype == MHFX_DTYPE_C128)
            hipLaunchKernelGGL(nufft_grid_kernel<true>, dim3(blocks), dim3(kThreads), 0, s, g);
        else
            hipLaunchKernelGGL(nufft_grid_kernel<false>, dim3(blocks), dim3(kThreads), 0, s, g);
        const int frc = mhf_fft(reinterpret_cast<const double*>(ftau), reinterpret_cast<double*>(ftau), p.Mr,
                                nb, iflag < 0 ? MHF_FFT_FORWARD : MHF_FFT_BACKWARD,
                                1.0 / static_cast<double>(p.Mr), fft_ws, p.fft_bytes, s);
        if (frc != MHF_OK) {
            char msg[400];
            snprintf(msg, sizeof(msg), "mhf_fft: %s", mhf_last_error());
            return set_error(frc, msg);
        }
        DeconvArgs d;
        d.ftau = ftau;
        d.starts = starts;
        d.ends = ends;
        d.n_points = n_points;
        d.min_len = min_len;
        d.seg0 = seg0;
        d.nseg = nb;
        d.M = M;
        d.Mr = p.Mr;
        d.tau = p.tau;
        d.sq = sqrt(M_PI / p.tau);
        d.out = out;
        d.out_ld = out_ld;
        d.power = out_mode == MHFX_OUT_POWER;
        int64_t db = (nb * M + kThreads - 1) / kThreads;
        if (db > 65536) db = 65536;
        hipLaunchKernelGGL(nufft_deconv_kernel, dim3(static_cast<unsigned>(db)), dim3(kThreads), 0, s, d);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MHFX_OK : set_error(MHFX_EDEVICE, hipGetErrorString(e));
}
