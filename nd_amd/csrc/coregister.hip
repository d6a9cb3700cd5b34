// nd_amd/csrc/coregister.hip -- Coregistration (nd/warp.py:1104-1163): sub-pixel alignment of every
// date of a stack to a reference date, as scikit-image 0.18 computes it.
//
// Shifts (skimage.registration.phase_cross_correlation(C11[t], C11[ref], upsample_factor=u)):
//   stage C11 planar -> R2C FFT of every date (hipFFT, batched) -> cross-power P_t = F_t conj(F_ref)
//   -> C2R -> per-date argmax |cc| (first index in C order) -> whole-pixel shift; for u > 1 the
//   upsampled matrix DFT of conj(P_t) around it, in complex128, split into an x pass over the stored
//   half spectrum (a missing column is the conjugate of a stored one: P[-j, -c] = conj(P[j, c])) and
//   a y pass, then argmax |CC| and the final shift.  Shifts stay in device memory.
// Warp (skimage.transform.warp(v[t], AffineTransform(translation=(s_col, s_row)), order=3), mode
// 'constant', cval 0, clip=True): per-(variable, date) min / max with NaN propagation, per-date row
// and column tables of the sample coordinates (formed in the array's own precision, as skimage does
// with float32 data), then the Catmull-Rom bicubic from an LDS tile, the clip to the plane's input
// range and the cval-preserve rule.
#include <hipfft/hipfft.h>

#include <map>
#include <math.h>
#include <mutex>
#include <tuple>

#include "common.hpp"
#include "dispatch.hpp"

namespace nd_amd {

// ================================================================================ hipFFT plan cache
#define ND_FFT_CHECK(expr)                                                                   \
    do {                                                                                     \
        hipfftResult _r = (expr);                                                            \
        if (_r != HIPFFT_SUCCESS) {                                                          \
            ::nd_amd::set_error("%s failed: hipfft status %d (%s:%d)", #expr, (int)_r,       \
                                __FILE__, __LINE__);                                         \
            return ND_AMD_EHIP;                                                              \
        }                                                                                    \
    } while (0)

// (device, stream, ny, nx, batch, dtype, inverse) -> plan.  rocFFT builds its kernels on a plan's
// first use; the cache keeps that cost to the first call of a shape on a stream.  The stream is part
// of the key: a plan's stream is set once, when the plan is made, and never changed, and its
// auto-allocated work area belongs to that stream alone.  The transforms run after g_plan_mu is
// released, so a plan shared between streams could be retargeted by one host thread between another
// thread's fft_plan and its hipfftExec*, and two streams would share one work area.  Plans live as
// long as the process: a caller that makes and destroys streams without end grows the cache.
static std::mutex g_plan_mu;
static std::map<std::tuple<int, hipStream_t, int, int, int, int, int>, hipfftHandle> g_plans;

static int fft_plan(int ny, int nx, int batch, int dtype, bool inverse, hipStream_t stream, hipfftHandle *out)
{
    int dev = 0;
    ND_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_plan_mu);
    const auto key = std::make_tuple(dev, stream, ny, nx, batch, dtype, inverse ? 1 : 0);
    auto it = g_plans.find(key);
    if (it == g_plans.end()) {
        hipfftHandle h;
        int n[2] = {ny, nx};
        const hipfftType type = dtype == ND_AMD_F32 ? (inverse ? HIPFFT_C2R : HIPFFT_R2C)
                                                    : (inverse ? HIPFFT_Z2D : HIPFFT_D2Z);
        ND_FFT_CHECK(hipfftPlanMany(&h, 2, n, nullptr, 1, 0, nullptr, 1, 0, type, batch));
        const hipfftResult r = hipfftSetStream(h, stream);
        if (r != HIPFFT_SUCCESS) {
            hipfftDestroy(h);
            ND_FFT_CHECK(r);
        }
        it = g_plans.emplace(key, h).first;
    }
    *out = it->second;
    return ND_AMD_OK;
}

// ================================================================================ shifts
template <typename T> struct Cplx;
template <> struct Cplx<float> { typedef float2 type; };
template <> struct Cplx<double> { typedef double2 type; };

// Strided C11 -> planar (k, ny, nx) staging buffer (layouts the copy engine or relayout do not cover)
template <typename T>
__global__ void __launch_bounds__(256) coreg_gather_kernel(const T *__restrict__ in, T *__restrict__ out, int64_t k,
                                                           int64_t ny, int64_t nx, int64_t st, int64_t sy, int64_t sx)
{
    const int64_t n = k * ny * nx;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t t = e / (ny * nx), p = e - t * ny * nx, y = p / nx, x = p - y * nx;
        out[e] = in[t * st + y * sy + x * sx];
    }
}

// P_t = F_t conj(F_ref): numpy's complex product src_freq * target_freq.conj(), in the spectra's type
template <typename C>
__device__ inline C cross_power(C a, C b)
{
    C p;
    p.x = a.x * b.x - a.y * (-b.y);
    p.y = a.x * (-b.y) + a.y * b.x;
    return p;
}

template <typename T>
__global__ void __launch_bounds__(256) coreg_crosspower_kernel(const typename Cplx<T>::type *__restrict__ F,
                                                               typename Cplx<T>::type *__restrict__ P,
                                                               int64_t nspec, int64_t total, int64_t ref)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
        P[e] = cross_power(F[e], F[ref * nspec + e % nspec]);
}

struct ArgMax {
    double v;       // |value|
    int64_t i;      // C-order index
    int nan;        // a NaN was seen
};

__device__ inline void argmax_merge(ArgMax &a, const ArgMax &b)
{
    if (b.v > a.v || (b.v == a.v && b.i < a.i)) {
        a.v = b.v;
        a.i = b.i;
    }
    a.nan |= b.nan;
}

__device__ inline ArgMax block_argmax(ArgMax m)
{
    __shared__ double sv[256];
    __shared__ int64_t si[256];
    __shared__ int sn[256];
    const int tid = threadIdx.x;
    sv[tid] = m.v;
    si[tid] = m.i;
    sn[tid] = m.nan;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            ArgMax a{sv[tid], si[tid], sn[tid]}, b{sv[tid + s], si[tid + s], sn[tid + s]};
            argmax_merge(a, b);
            sv[tid] = a.v;
            si[tid] = a.i;
            sn[tid] = a.nan;
        }
        __syncthreads();
    }
    ArgMax r{sv[0], si[0], sn[0]};
    __syncthreads();
    return r;
}

// per-date argmax |cc| over ny * nx (the C2R output: unnormalised, a common positive factor);
// partials per block at part[t * nblk + b]
template <typename T>
__global__ void __launch_bounds__(256) coreg_argmax_kernel(const T *__restrict__ cc, int64_t n, ArgMax *part)
{
    const int t = blockIdx.y, nblk = gridDim.x;
    const T *src = cc + (int64_t)t * n;
    ArgMax m{-1.0, INT64_MAX, 0};
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)nblk * 256) {
        const double v = fabs((double)src[e]);
        if (isnan(v)) m.nan = 1;
        else if (v > m.v) {           // ascending e per thread: the first of equal values stays
            m.v = v;
            m.i = e;
        }
    }
    m = block_argmax(m);
    if (threadIdx.x == 0) part[(int64_t)t * nblk + blockIdx.x] = m;
}

struct DatePeak {
    double s_r, s_c;       // whole-pixel shifts
    double off_r, off_c;   // sample_region_offset = dftshift - s * u
    int nan;
};

// one block per date: reduce the partials, whole-pixel shift, offsets of the upsampled region;
// with u == 1 also the final shifts
__global__ void __launch_bounds__(256) coreg_peak_kernel(const ArgMax *part, int nblk, int64_t ny, int64_t nx, int u,
                                                         int64_t ref, DatePeak *peaks, double *shifts, int32_t *status)
{
    const int t = blockIdx.x;
    ArgMax m{-1.0, INT64_MAX, 0};
    for (int b = threadIdx.x; b < nblk; b += 256) argmax_merge(m, part[(int64_t)t * nblk + b]);
    m = block_argmax(m);
    if (threadIdx.x != 0) return;
    int64_t pr = 0, pc = 0;
    if (m.i != INT64_MAX) {
        pr = m.i / nx;
        pc = m.i - pr * nx;
    }
    double sr = (double)pr, sc = (double)pc;
    if (sr > trunc((double)ny / 2.0)) sr -= (double)ny;
    if (sc > trunc((double)nx / 2.0)) sc -= (double)nx;
    DatePeak p;
    const double R = ceil((double)u * 1.5), d = trunc(R / 2.0);
    p.s_r = sr;
    p.s_c = sc;
    p.off_r = d - sr * (double)u;
    p.off_c = d - sc * (double)u;
    p.nan = m.nan;
    peaks[t] = p;
    if (u == 1) {
        shifts[2 * t] = (ny == 1 || t == ref) ? 0.0 : sr;
        shifts[2 * t + 1] = (nx == 1 || t == ref) ? 0.0 : sc;
        status[t] = (t == ref) ? 0 : m.nan;
    }
}

// numpy.fft.fftfreq(n, u)[c] = (c < (n - 1) / 2 + 1 ? c : c - n) * (1.0 / (n * u))
__device__ inline double fftfreq(int64_t c, int64_t n, double u)
{
    const int64_t npos = (n - 1) / 2 + 1;
    const double val = 1.0 / ((double)n * u);
    return (double)(c < npos ? c : c - n) * val;
}

// exp(-2 pi i (i - off) f) as numpy forms it: theta = (-2 pi) * ((i - off) * f), one rounding each
__device__ inline double2 dft_kernel(double i, double off, double f)
{
    const double th = (-2.0 * M_PI) * ((i - off) * f);
    double s, c;
    sincos(th, &s, &c);
    return make_double2(c, s);
}

// Tables of every date (R = upsampled region size):
//   kxa[c][i], c < nh               kernel along x at the stored column c
//   kxb[c][i], 1 <= c <= nx - nh    kernel along x at the missing column nx - c
//   ky[j][a], kyr[j][a]             kernel along y at row j and at row (ny - j) % ny
struct DftTables {
    double2 *kxa, *kxb, *ky, *kyr;
    int64_t kxa_n, kxb_n, ky_n;     // elements per date
};

__global__ void __launch_bounds__(256) coreg_dft_tables_kernel(DftTables tb, const DatePeak *peaks, int64_t ny,
                                                               int64_t nx, int R, int u)
{
    const int t = blockIdx.y;
    const DatePeak p = peaks[t];
    const double du = (double)u;
    const int64_t nxa = tb.kxa_n, nxb = tb.kxb_n, nyy = tb.ky_n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nxa + nxb + 2 * nyy; e += (int64_t)gridDim.x * 256) {
        if (e < nxa) {
            const int64_t c = e / R, i = e - c * R;
            tb.kxa[t * nxa + e] = dft_kernel((double)i, p.off_c, fftfreq(c, nx, du));
        } else if (e < nxa + nxb) {
            const int64_t f = e - nxa, c = f / R, i = f - c * R;
            tb.kxb[t * nxb + f] = c == 0 ? make_double2(0.0, 0.0)
                                         : dft_kernel((double)i, p.off_c, fftfreq(nx - c, nx, du));
        } else {
            const bool refl = e - nxa - nxb >= nyy;
            const int64_t f = (e - nxa - nxb) - (refl ? nyy : 0), j = f / R, a = f - j * R;
            const int64_t row = refl ? (ny - j) % ny : j;
            (refl ? tb.kyr : tb.ky)[t * nyy + f] = dft_kernel((double)a, p.off_r, fftfreq(row, ny, du));
        }
    }
}

__device__ inline double2 cmul(double2 a, double2 b)
{
    return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
__device__ inline double2 cmulconj(double2 a, double2 b)    // a * conj(b)
{
    return make_double2(fma(a.x, b.x, a.y * b.y), fma(a.y, b.x, -a.x * b.y));
}

// x pass of the upsampled DFT, 64 rows j x 16 MI region columns i of one date per block:
//   A[j][i] = sum_{c < nh} kxa[c][i] conj(P[j][c]),   B[j][i] = sum_{1 <= c <= nx - nh} kxb[c][i] P[j][c]
// P recomputed from the spectra (the arithmetic of coreg_crosspower_kernel), widened to complex128
// as numpy's tensordot does.  Thread: 4 rows x MI columns.
constexpr int DX_ROWS = 64, DX_CK = 16;

template <typename T, int MI>
__global__ void __launch_bounds__(256) coreg_dft_x_kernel(const typename Cplx<T>::type *__restrict__ F, int64_t ref,
                                                          DftTables tb, double2 *A, double2 *B, int64_t ny,
                                                          int64_t nx, int64_t nh, int R)
{
    __shared__ double2 ps[DX_ROWS][DX_CK + 1];
    __shared__ double2 ka[DX_CK][16 * MI], kb[DX_CK][16 * MI];
    const int t = blockIdx.z, tid = threadIdx.x, ti = tid & 15, tj = tid >> 4;
    const int64_t j0 = (int64_t)blockIdx.y * DX_ROWS;
    const int i0 = blockIdx.x * 16 * MI;
    const int64_t nspec = ny * nh;
    const typename Cplx<T>::type *Ft = F + (int64_t)t * nspec, *Fr = F + ref * nspec;
    const double2 *kxa = tb.kxa + t * tb.kxa_n, *kxb = tb.kxb + t * tb.kxb_n;
    double2 a[4][MI], b[4][MI];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int m = 0; m < MI; ++m) a[q][m] = b[q][m] = make_double2(0.0, 0.0);
    const int64_t nb = nx - nh;      // missing columns: nx - c for c = 1 .. nb
    for (int64_t c0 = 0; c0 < nh; c0 += DX_CK) {
        __syncthreads();
        for (int e = tid; e < DX_ROWS * DX_CK; e += 256) {
            const int r = e / DX_CK, cc = e - r * DX_CK;
            const int64_t j = j0 + r, c = c0 + cc;
            double2 v = make_double2(0.0, 0.0);
            if (j < ny && c < nh) {
                const typename Cplx<T>::type p = cross_power(Ft[j * nh + c], Fr[j * nh + c]);
                v = make_double2((double)p.x, (double)p.y);
            }
            ps[r][cc] = v;
        }
        for (int e = tid; e < DX_CK * 16 * MI; e += 256) {
            const int cc = e / (16 * MI), ii = e - cc * (16 * MI);
            const int64_t c = c0 + cc;
            const int i = i0 + ii;
            ka[cc][ii] = (c < nh && i < R) ? kxa[c * R + i] : make_double2(0.0, 0.0);
            kb[cc][ii] = (c >= 1 && c <= nb && i < R) ? kxb[c * R + i] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        for (int cc = 0; cc < DX_CK; ++cc) {
            double2 p[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) p[q] = ps[tj + 16 * q][cc];
#pragma unroll
            for (int m = 0; m < MI; ++m) {
                const double2 wa = ka[cc][ti + 16 * m], wb = kb[cc][ti + 16 * m];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double2 ua = cmulconj(wa, p[q]), ub = cmul(wb, p[q]);
                    a[q][m].x += ua.x;
                    a[q][m].y += ua.y;
                    b[q][m].x += ub.x;
                    b[q][m].y += ub.y;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t j = j0 + tj + 16 * q;
#pragma unroll
        for (int m = 0; m < MI; ++m) {
            const int i = i0 + ti + 16 * m;
            if (j < ny && i < R) {
                A[((int64_t)t * ny + j) * R + i] = a[q][m];
                B[((int64_t)t * ny + j) * R + i] = b[q][m];
            }
        }
    }
}

// y pass: |CC[a][i]| = |sum_j ky[j][a] A[j][i] + kyr[j][a] B[j][i]|  (the conj numpy applies after
// the DFT does not change the modulus).  One block per (a, date); R <= 256 lanes over i, the
// 256 / R lane groups split j and are summed in a fixed order.
__global__ void __launch_bounds__(256) coreg_dft_y_kernel(DftTables tb, const double2 *A, const double2 *B,
                                                          double *mag, int64_t ny, int R)
{
    __shared__ double2 part[256];
    const int a = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int ng = 256 / R, g = tid / R, i = tid - g * R;
    const double2 *ky = tb.ky + t * tb.ky_n, *kyr = tb.kyr + t * tb.ky_n;
    const double2 *At = A + (int64_t)t * ny * R, *Bt = B + (int64_t)t * ny * R;
    double2 s = make_double2(0.0, 0.0);
    if (g < ng) {
        for (int64_t j = g; j < ny; j += ng) {
            const double2 u1 = cmul(ky[j * R + a], At[j * R + i]), u2 = cmul(kyr[j * R + a], Bt[j * R + i]);
            s.x += u1.x + u2.x;
            s.y += u1.y + u2.y;
        }
    }
    part[tid] = s;
    __syncthreads();
    if (tid < R) {
        double2 tot = part[tid];
        for (int gg = 1; gg < ng; ++gg) {
            tot.x += part[gg * R + tid].x;
            tot.y += part[gg * R + tid].y;
        }
        mag[((int64_t)t * R + a) * R + tid] = hypot(tot.x, tot.y);
    }
}

// one block per date: argmax |CC| (first in C order; a NaN anywhere is what makes skimage raise)
__global__ void __launch_bounds__(256) coreg_refine_kernel(const double *mag, const DatePeak *peaks, int R, int u,
                                                           int64_t ny, int64_t nx, int64_t ref, double *shifts,
                                                           int32_t *status)
{
    const int t = blockIdx.x;
    const double *m = mag + (int64_t)t * R * R;
    ArgMax best{-1.0, INT64_MAX, 0};
    for (int e = threadIdx.x; e < R * R; e += 256) {
        const double v = m[e];
        const ArgMax c = isnan(v) ? ArgMax{-1.0, INT64_MAX, 1} : ArgMax{v, (int64_t)e, 0};
        argmax_merge(best, c);
    }
    best = block_argmax(best);
    if (threadIdx.x != 0) return;
    const DatePeak p = peaks[t];
    const double d = trunc(ceil((double)u * 1.5) / 2.0);
    const int64_t pa = best.i == INT64_MAX ? 0 : best.i / R, pi = best.i == INT64_MAX ? 0 : best.i % R;
    const double sr = p.s_r + ((double)pa - d) / (double)u, sc = p.s_c + ((double)pi - d) / (double)u;
    shifts[2 * t] = (ny == 1 || t == ref) ? 0.0 : sr;
    shifts[2 * t + 1] = (nx == 1 || t == ref) ? 0.0 : sc;
    status[t] = t == ref ? 0 : (best.nan | p.nan);
}

struct ShiftLayout {
    size_t stage, spec, spec2, partials, peaks, kxa, kxb, ky, kyr, A, B, mag, total;
    int nblk, R;
};

static ShiftLayout shift_layout(int dtype, int64_t k, int64_t ny, int64_t nx, int u)
{
    ShiftLayout L;
    const size_t es = dtype == ND_AMD_F32 ? 4 : 8;
    const int64_t nh = nx / 2 + 1, n = ny * nx;
    L.R = u > 1 ? (int)ceil(u * 1.5) : 0;
    const int64_t nb = n / (256 * 16);
    L.nblk = (int)(nb < 1 ? 1 : (nb > 256 ? 256 : nb));
    size_t off = 0;
    auto put = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    const size_t R = (size_t)L.R;
    L.stage = put(k * n * es);                       // planar C11, then the C2R output
    L.spec = put(k * ny * nh * 2 * es);              // F_t
    L.spec2 = put(k * ny * nh * 2 * es);             // P_t, consumed by the C2R
    L.partials = put(k * L.nblk * sizeof(ArgMax));
    L.peaks = put(k * sizeof(DatePeak));
    L.kxa = put(k * nh * R * 16);
    L.kxb = put(k * (nx - nh + 1) * R * 16);
    L.ky = put(k * ny * R * 16);
    L.kyr = put(k * ny * R * 16);
    L.A = put(k * ny * R * 16);
    L.B = put(k * ny * R * 16);
    L.mag = put(k * R * R * 8);
    L.total = off;
    return L;
}

static int grid1(int64_t n)
{
    const int64_t b = ceil_div(n, 256);
    return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

template <typename T>
static int coreg_shifts_impl(const void *c11, int64_t k, int64_t ny, int64_t nx, int64_t st, int64_t sy,
                             int64_t sx, int64_t ref, int u, double *shifts, int32_t *status, void *workspace,
                             hipStream_t stream)
{
    typedef typename Cplx<T>::type C;
    const int dtype = sizeof(T) == 4 ? ND_AMD_F32 : ND_AMD_F64;
    const ShiftLayout L = shift_layout(dtype, k, ny, nx, u);
    char *ws = static_cast<char *>(workspace);
    T *stage = reinterpret_cast<T *>(ws + L.stage);
    C *F = reinterpret_cast<C *>(ws + L.spec), *P = reinterpret_cast<C *>(ws + L.spec2);
    ArgMax *part = reinterpret_cast<ArgMax *>(ws + L.partials);
    DatePeak *peaks = reinterpret_cast<DatePeak *>(ws + L.peaks);
    const int64_t n = ny * nx, nh = nx / 2 + 1;
    KernelTimer timer(ND_AMD_KERNEL_COREG_SHIFTS, stream);
    // 1. C11 planar
    if (sx == 1 && sy == nx && st == n) {
        ND_HIP_CHECK(hipMemcpyAsync(stage, c11, (size_t)(k * n) * sizeof(T), hipMemcpyDeviceToDevice, stream));
    } else if (st == 1 && sx == k && sy == nx * k && (k | 1) * (int64_t)sizeof(T) <= 48 * 1024) {
        const int rc = nd_amd_relayout_planar(c11, stage, dtype, n, k, 1, n, stream);
        if (rc != ND_AMD_OK) return rc;
    } else {
        hipLaunchKernelGGL((coreg_gather_kernel<T>), dim3(grid1(k * n)), dim3(256), 0, stream,
                           static_cast<const T *>(c11), stage, k, ny, nx, st, sy, sx);
        ND_HIP_CHECK(hipGetLastError());
    }
    // 2. spectra of every date, cross-power against the reference, back to the correlation
    hipfftHandle fwd, inv;
    int rc = fft_plan((int)ny, (int)nx, (int)k, dtype, false, stream, &fwd);
    if (rc != ND_AMD_OK) return rc;
    rc = fft_plan((int)ny, (int)nx, (int)k, dtype, true, stream, &inv);
    if (rc != ND_AMD_OK) return rc;
    if (dtype == ND_AMD_F32)
        ND_FFT_CHECK(hipfftExecR2C(fwd, reinterpret_cast<float *>(stage), reinterpret_cast<hipfftComplex *>(F)));
    else
        ND_FFT_CHECK(hipfftExecD2Z(fwd, reinterpret_cast<double *>(stage), reinterpret_cast<hipfftDoubleComplex *>(F)));
    hipLaunchKernelGGL((coreg_crosspower_kernel<T>), dim3(grid1(k * ny * nh)), dim3(256), 0, stream, F, P, ny * nh,
                       k * ny * nh, ref);
    ND_HIP_CHECK(hipGetLastError());
    if (dtype == ND_AMD_F32)
        ND_FFT_CHECK(hipfftExecC2R(inv, reinterpret_cast<hipfftComplex *>(P), reinterpret_cast<float *>(stage)));
    else
        ND_FFT_CHECK(hipfftExecZ2D(inv, reinterpret_cast<hipfftDoubleComplex *>(P), reinterpret_cast<double *>(stage)));
    // 3. whole-pixel peak
    hipLaunchKernelGGL((coreg_argmax_kernel<T>), dim3(L.nblk, (unsigned)k), dim3(256), 0, stream, stage, n, part);
    ND_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(coreg_peak_kernel, dim3((unsigned)k), dim3(256), 0, stream, part, L.nblk, ny, nx, u, ref,
                       peaks, shifts, status);
    ND_HIP_CHECK(hipGetLastError());
    if (u == 1) return ND_AMD_OK;
    // 4. upsampled DFT around the peak
    const int R = L.R;
    DftTables tb;
    tb.kxa = reinterpret_cast<double2 *>(ws + L.kxa);
    tb.kxb = reinterpret_cast<double2 *>(ws + L.kxb);
    tb.ky = reinterpret_cast<double2 *>(ws + L.ky);
    tb.kyr = reinterpret_cast<double2 *>(ws + L.kyr);
    tb.kxa_n = nh * R;
    tb.kxb_n = (nx - nh + 1) * R;
    tb.ky_n = ny * R;
    const int64_t ntab = tb.kxa_n + tb.kxb_n + 2 * tb.ky_n;
    hipLaunchKernelGGL(coreg_dft_tables_kernel, dim3((unsigned)ceil_div(ntab, 256 * 4), (unsigned)k), dim3(256), 0,
                       stream, tb, peaks, ny, nx, R, u);
    ND_HIP_CHECK(hipGetLastError());
    double2 *A = reinterpret_cast<double2 *>(ws + L.A), *B = reinterpret_cast<double2 *>(ws + L.B);
    const int mi = (R + 15) / 16;
    const int MI = mi > 5 ? 4 : mi;            // region columns per block: 16 MI
    const dim3 gx((unsigned)ceil_div(R, 16 * MI), (unsigned)ceil_div(ny, DX_ROWS), (unsigned)k);
    auto dft_x = [&](auto M) {
        hipLaunchKernelGGL((coreg_dft_x_kernel<T, decltype(M)::value>), gx, dim3(256), 0, stream, F, ref, tb, A,
                           B, ny, nx, nh, R);
    };
    if (!pick_eq<1, 2, 3, 4>(MI, dft_x)) dft_x(int_c<5>{});
    ND_HIP_CHECK(hipGetLastError());
    double *mag = reinterpret_cast<double *>(ws + L.mag);
    hipLaunchKernelGGL(coreg_dft_y_kernel, dim3((unsigned)R, (unsigned)k), dim3(256), 0, stream, tb, A, B, mag, ny, R);
    ND_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(coreg_refine_kernel, dim3((unsigned)k), dim3(256), 0, stream, mag, peaks, R, u, ny, nx, ref,
                       shifts, status);
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

// ================================================================================ warp
// Catmull-Rom as skimage's cubic_interpolation computes it for the array type: in double for float64;
// for float32 the two differences of taps in float, the rest in double, the result rounded to float.
__device__ inline double cubic(double x, double f0, double f1, double f2, double f3)
{
    return f1 + 0.5 * x * (f2 - f0 + x * (2.0 * f0 - 5.0 * f1 + 4.0 * f2 - f3 + x * (3.0 * (f1 - f2) + f3 - f0)));
}
__device__ inline float cubic(float x, float f0, float f1, float f2, float f3)
{
    const double xd = x, d20 = (double)(f2 - f0), d12 = (double)(f1 - f2);
    const double a = (double)f0, b = (double)f1, c = (double)f2, d = (double)f3;
    return (float)(b + 0.5 * xd * (d20 + xd * (2.0 * a - 5.0 * b + 4.0 * c - d + xd * (3.0 * d12 + d - a))));
}

// numpy's clip (NaN in the value or a bound gives NaN), then the cval-preserve rule of skimage's
// _clip_warp_output: when 0 lies outside [lo, hi] (or they are NaN) exact zeros stay 0.
template <typename T>
__device__ inline T clip_preserve(T v, double lo, double hi)
{
    const bool zero = v == (T)0;
    const bool preserve = !(lo <= 0.0 && 0.0 <= hi);
    T r;
    if (isnan(v) || isnan(lo) || isnan(hi)) r = (T)NAN;
    else r = (T)fmin(fmax((double)v, lo), hi);
    return (preserve && zero) ? (T)0 : r;
}

// Per-date sample coordinates: coord = (T)i + (T)shift in T (skimage casts its matrix to the image's
// dtype and forms x = 1 * c + 0 * r + tx in that type), floor and fraction.  A coordinate beyond
// the plane by more than the kernel's reach is clamped (all its taps read 0 either way); a
// non-finite shift counts as 0 (callers of nd_amd_coregister_shifts see the date's status).
template <typename T>
__global__ void __launch_bounds__(256) coreg_warp_tables_kernel(const double *shifts, int64_t nr, int64_t nc,
                                                                int32_t *ri, T *rf, int32_t *ci, T *cf)
{
    const int t = blockIdx.y;
    const double s0 = shifts[2 * t], s1 = shifts[2 * t + 1];
    const T sr = isfinite(s0) ? (T)s0 : (T)0, sc = isfinite(s1) ? (T)s1 : (T)0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nr + nc; e += (int64_t)gridDim.x * 256) {
        const bool row = e < nr;
        const int64_t i = row ? e : e - nr, n = row ? nr : nc;
        T v = (T)i + (row ? sr : sc);
        if (!(v >= (T)-4)) v = (T)-4;
        if (v > (T)(n + 4)) v = (T)(n + 4);
        const T f = floor(v);
        if (row) {
            ri[t * nr + i] = (int32_t)f;
            rf[t * nr + i] = v - f;
        } else {
            ci[t * nc + i] = (int32_t)f;
            cf[t * nc + i] = v - f;
        }
    }
}

struct Planes {
    const void *in[ND_AMD_COREG_MAX_VARS];
    void *out[ND_AMD_COREG_MAX_VARS];
};

struct MinMax {
    double lo, hi;
};

__device__ inline double nanmin(double a, double b) { return (isnan(a) || isnan(b)) ? NAN : fmin(a, b); }
__device__ inline double nanmax(double a, double b) { return (isnan(a) || isnan(b)) ? NAN : fmax(a, b); }

// min / max of every (variable, date) plane, NaN-propagating, partials per block at
// part[(variable * k + date) * nblk + block].  (t, r, c): grid.y = variable * k + date.
template <typename T>
__global__ void __launch_bounds__(256) coreg_minmax_planar_kernel(const Planes pl, int64_t k, int64_t n, MinMax *part)
{
    __shared__ double slo[256], shi[256];
    const int p = blockIdx.y, v = p / (int)k, t = p - v * (int)k, nblk = gridDim.x, tid = threadIdx.x;
    const T *src = static_cast<const T *>(pl.in[v]) + (int64_t)t * n;
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t e = (int64_t)blockIdx.x * 256 + tid; e < n; e += (int64_t)nblk * 256) {
        const double x = (double)src[e];
        lo = nanmin(lo, x);
        hi = nanmax(hi, x);
    }
    slo[tid] = lo;
    shi[tid] = hi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            slo[tid] = nanmin(slo[tid], slo[tid + s]);
            shi[tid] = nanmax(shi[tid], shi[tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) part[(int64_t)p * nblk + blockIdx.x] = MinMax{slo[0], shi[0]};
}

// (r, c, t): thread = (pixel lane, date) with dates fastest, so a wave reads a contiguous span;
// grid.y = variable, dates in groups of up to 256.
template <typename T>
__global__ void __launch_bounds__(256) coreg_minmax_pm_kernel(const Planes pl, int64_t k, int64_t npix, MinMax *part)
{
    __shared__ double slo[256], shi[256];
    const int v = blockIdx.y, nblk = gridDim.x, tid = threadIdx.x;
    const T *src = static_cast<const T *>(pl.in[v]);
    for (int64_t t0 = 0; t0 < k; t0 += 256) {
        const int kk = (int)(k - t0 < 256 ? k - t0 : 256), per = 256 / kk;
        const int g = tid / kk, tt = tid - g * kk;
        double lo = INFINITY, hi = -INFINITY;
        if (g < per) {
            for (int64_t p = (int64_t)blockIdx.x * per + g; p < npix; p += (int64_t)nblk * per) {
                const double x = (double)src[p * k + t0 + tt];
                lo = nanmin(lo, x);
                hi = nanmax(hi, x);
            }
        }
        slo[tid] = lo;
        shi[tid] = hi;
        __syncthreads();
        if (tid < kk) {
            for (int gg = 1; gg < per; ++gg) {
                lo = nanmin(lo, slo[gg * kk + tid]);
                hi = nanmax(hi, shi[gg * kk + tid]);
            }
            part[((int64_t)v * k + t0 + tid) * nblk + blockIdx.x] = MinMax{lo, hi};
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) coreg_minmax_final_kernel(const MinMax *part, int nblk, int64_t nplanes,
                                                                 MinMax *mm)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nplanes) return;
    double lo = INFINITY, hi = -INFINITY;
    for (int b = 0; b < nblk; ++b) {
        const MinMax m = part[p * nblk + b];
        lo = nanmin(lo, m.lo);
        hi = nanmax(hi, m.hi);
    }
    mm[p] = MinMax{lo, hi};
}

struct WarpArgs {
    Planes pl;
    const int32_t *ri, *ci;
    const void *rf, *cf;
    const MinMax *mm;
    int64_t k, nr, nc, ref;
};

template <typename T>
__device__ inline T tap(const T *src, int64_t r, int64_t c, int64_t nr, int64_t nc)
{
    return (r >= 0 && r < nr && c >= 0 && c < nc) ? src[r * nc + c] : (T)0;
}

// Planar (t, r, c): one block = 16 output rows x 64 output columns of one (variable, date) plane.
// The taps (rows ri[r] - 1 .. ri[r] + 2, columns ci[c] - 1 .. ci[c] + 2: the integer part of the
// shift is folded into those addresses) are staged in LDS, 0 outside the plane; the column cubic of
// every staged row is formed once (rounded to T, as skimage keeps it) and the row cubic reads 4 of
// them.  A tile whose coordinates spread wider than the staging buffer (only where T = float can no
// longer resolve the fraction) reads its taps from global memory.
constexpr int WT_ROWS = 16, WT_COLS = 64, WT_HMAX = WT_ROWS + 8, WT_WMAX = WT_COLS + 8, WT_Q = WT_ROWS / 4;

template <typename T>
__global__ void __launch_bounds__(256) coreg_warp_planar_kernel(const WarpArgs a)
{
    __shared__ T tile[WT_HMAX][WT_WMAX];
    __shared__ T hs[WT_HMAX][WT_COLS];
    const int p = blockIdx.z, v = p / (int)a.k, t = p - v * (int)a.k, tid = threadIdx.x;
    const int64_t n = a.nr * a.nc;
    const T *src = static_cast<const T *>(a.pl.in[v]) + (int64_t)t * n;
    T *dst = static_cast<T *>(a.pl.out[v]) + (int64_t)t * n;
    const int64_t cb = (int64_t)blockIdx.x * WT_COLS, rb = (int64_t)blockIdx.y * WT_ROWS;
    const int x = tid & 63, yq = tid >> 6;
    const int64_t c = cb + x;
    if (t == a.ref) {          // the reference date is left as it is
        for (int q = 0; q < WT_Q; ++q) {
            const int64_t r = rb + yq + 4 * q;
            if (r < a.nr && c < a.nc) dst[r * a.nc + c] = src[r * a.nc + c];
        }
        return;
    }
    const int32_t *ri = a.ri + (int64_t)t * a.nr, *ci = a.ci + (int64_t)t * a.nc;
    const T *rf = static_cast<const T *>(a.rf) + (int64_t)t * a.nr;
    const T *cf = static_cast<const T *>(a.cf) + (int64_t)t * a.nc;
    const MinMax mm = a.mm[p];
    const int64_t ce = (cb + WT_COLS < a.nc ? cb + WT_COLS : a.nc) - 1;
    const int64_t re = (rb + WT_ROWS < a.nr ? rb + WT_ROWS : a.nr) - 1;
    const int64_t cl = (int64_t)ci[cb] - 1, rl = (int64_t)ri[rb] - 1;
    const int64_t W = (int64_t)ci[ce] + 3 - cl, H = (int64_t)ri[re] + 3 - rl;
    if (W <= WT_WMAX && H <= WT_HMAX) {
        for (int e = tid; e < H * W; e += 256) {
            const int rr = e / (int)W, cc = e - rr * (int)W;
            tile[rr][cc] = tap(src, rl + rr, cl + cc, a.nr, a.nc);
        }
        __syncthreads();
        for (int e = tid; e < H * WT_COLS; e += 256) {
            const int rr = e / WT_COLS, xx = e - rr * WT_COLS;
            const int64_t cx = cb + xx;
            if (cx < a.nc) {
                const int b = (int)(ci[cx] - 1 - cl);
                hs[rr][xx] = cubic(cf[cx], tile[rr][b], tile[rr][b + 1], tile[rr][b + 2], tile[rr][b + 3]);
            }
        }
        __syncthreads();
        if (c < a.nc) {
#pragma unroll
            for (int q = 0; q < WT_Q; ++q) {
                const int64_t r = rb + yq + 4 * q;
                if (r < a.nr) {
                    const int b = (int)(ri[r] - 1 - rl);
                    const T o = cubic(rf[r], hs[b][x], hs[b + 1][x], hs[b + 2][x], hs[b + 3][x]);
                    dst[r * a.nc + c] = clip_preserve(o, mm.lo, mm.hi);
                }
            }
        }
    } else if (c < a.nc) {
        for (int q = 0; q < WT_Q; ++q) {
            const int64_t r = rb + yq + 4 * q;
            if (r >= a.nr) continue;
            const int64_t r0 = ri[r], c0 = ci[c];
            T f[4];
            for (int i = 0; i < 4; ++i)
                f[i] = cubic(cf[c], tap(src, r0 - 1 + i, c0 - 1, a.nr, a.nc), tap(src, r0 - 1 + i, c0, a.nr, a.nc),
                             tap(src, r0 - 1 + i, c0 + 1, a.nr, a.nc), tap(src, r0 - 1 + i, c0 + 2, a.nr, a.nc));
            dst[r * a.nc + c] = clip_preserve(cubic(rf[r], f[0], f[1], f[2], f[3]), mm.lo, mm.hi);
        }
    }
}

// (r, c, t): one thread per output element, dates fastest (a wave writes a contiguous span); the 16
// taps of a date are read where they lie (neighbouring pixels are k elements apart, served by the
// caches).  Correct for any shift; its speed is reported, not tuned.
template <typename T>
__device__ inline T tap_pm(const T *src, int64_t r, int64_t c, int64_t t, int64_t nr, int64_t nc, int64_t k)
{
    return (r >= 0 && r < nr && c >= 0 && c < nc) ? src[(r * nc + c) * k + t] : (T)0;
}

template <typename T>
__global__ void __launch_bounds__(256) coreg_warp_pm_kernel(const WarpArgs a)
{
    const int v = blockIdx.y;
    const T *src = static_cast<const T *>(a.pl.in[v]);
    T *dst = static_cast<T *>(a.pl.out[v]);
    const int64_t total = a.nr * a.nc * a.k;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t p = e / a.k, t = e - p * a.k, r = p / a.nc, c = p - r * a.nc;
        if (t == a.ref) {
            dst[e] = src[e];
            continue;
        }
        const int64_t r0 = a.ri[t * a.nr + r], c0 = a.ci[t * a.nc + c];
        const T fr = static_cast<const T *>(a.rf)[t * a.nr + r], fc = static_cast<const T *>(a.cf)[t * a.nc + c];
        T f[4];
        for (int i = 0; i < 4; ++i)
            f[i] = cubic(fc, tap_pm(src, r0 - 1 + i, c0 - 1, t, a.nr, a.nc, a.k),
                         tap_pm(src, r0 - 1 + i, c0, t, a.nr, a.nc, a.k),
                         tap_pm(src, r0 - 1 + i, c0 + 1, t, a.nr, a.nc, a.k),
                         tap_pm(src, r0 - 1 + i, c0 + 2, t, a.nr, a.nc, a.k));
        const MinMax mm = a.mm[(int64_t)v * a.k + t];
        dst[e] = clip_preserve(cubic(fr, f[0], f[1], f[2], f[3]), mm.lo, mm.hi);
    }
}

struct WarpLayout {
    size_t ri, ci, rf, cf, part, mm, total;
    int nblk;
};

static WarpLayout warp_layout(int dtype, int nvars, int64_t k, int64_t nr, int64_t nc, int layout)
{
    WarpLayout L;
    const size_t es = dtype == ND_AMD_F32 ? 4 : 8;
    const int64_t n = nr * nc;
    const int64_t per = layout == ND_AMD_LAYOUT_PLANAR ? n : n * k;
    const int64_t nb = per / (256 * 32);
    L.nblk = (int)(nb < 1 ? 1 : (nb > 512 ? 512 : nb));
    if (layout == ND_AMD_LAYOUT_PLANAR) {
        // fewer blocks per plane once the planes are many: their number alone fills the device
        const int64_t planes = (int64_t)nvars * k, cap = 8192 / planes;
        if (L.nblk > cap) L.nblk = (int)(cap < 1 ? 1 : cap);
    }
    size_t off = 0;
    auto put = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    L.ri = put(k * nr * 4);
    L.ci = put(k * nc * 4);
    L.rf = put(k * nr * es);
    L.cf = put(k * nc * es);
    L.part = put((size_t)nvars * k * L.nblk * sizeof(MinMax));
    L.mm = put((size_t)nvars * k * sizeof(MinMax));
    L.total = off;
    return L;
}

template <typename T>
static int warp_impl(const void *const *in, void *const *out, int nvars, int64_t k, int64_t nr, int64_t nc,
                     int layout, const double *shifts, int64_t ref, void *workspace, hipStream_t stream)
{
    const int dtype = sizeof(T) == 4 ? ND_AMD_F32 : ND_AMD_F64;
    const WarpLayout L = warp_layout(dtype, nvars, k, nr, nc, layout);
    char *ws = static_cast<char *>(workspace);
    WarpArgs a;
    for (int v = 0; v < ND_AMD_COREG_MAX_VARS; ++v) {
        a.pl.in[v] = v < nvars ? in[v] : nullptr;
        a.pl.out[v] = v < nvars ? out[v] : nullptr;
    }
    a.ri = reinterpret_cast<const int32_t *>(ws + L.ri);
    a.ci = reinterpret_cast<const int32_t *>(ws + L.ci);
    a.rf = ws + L.rf;
    a.cf = ws + L.cf;
    a.mm = reinterpret_cast<const MinMax *>(ws + L.mm);
    a.k = k;
    a.nr = nr;
    a.nc = nc;
    a.ref = ref;
    KernelTimer timer(ND_AMD_KERNEL_COREG_WARP, stream);
    hipLaunchKernelGGL((coreg_warp_tables_kernel<T>), dim3((unsigned)ceil_div(nr + nc, 256), (unsigned)k), dim3(256), 0,
                       stream, shifts, nr, nc, reinterpret_cast<int32_t *>(ws + L.ri), reinterpret_cast<T *>(ws + L.rf),
                       reinterpret_cast<int32_t *>(ws + L.ci), reinterpret_cast<T *>(ws + L.cf));
    ND_HIP_CHECK(hipGetLastError());
    MinMax *part = reinterpret_cast<MinMax *>(ws + L.part);
    if (layout == ND_AMD_LAYOUT_PLANAR)
        hipLaunchKernelGGL((coreg_minmax_planar_kernel<T>), dim3(L.nblk, (unsigned)(nvars * k)), dim3(256), 0, stream,
                           a.pl, k, nr * nc, part);
    else
        hipLaunchKernelGGL((coreg_minmax_pm_kernel<T>), dim3(L.nblk, (unsigned)nvars), dim3(256), 0, stream, a.pl, k,
                           nr * nc, part);
    ND_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(coreg_minmax_final_kernel, dim3((unsigned)ceil_div(nvars * k, 256)), dim3(256), 0, stream, part,
                       L.nblk, (int64_t)nvars * k, reinterpret_cast<MinMax *>(ws + L.mm));
    ND_HIP_CHECK(hipGetLastError());
    if (layout == ND_AMD_LAYOUT_PLANAR)
        hipLaunchKernelGGL((coreg_warp_planar_kernel<T>),
                           dim3((unsigned)ceil_div(nc, WT_COLS), (unsigned)ceil_div(nr, WT_ROWS), (unsigned)(nvars * k)),
                           dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((coreg_warp_pm_kernel<T>), dim3(grid1(nr * nc * k), (unsigned)nvars), dim3(256), 0, stream, a);
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

static bool shapes_ok(int64_t k, int64_t ny, int64_t nx)
{
    return k >= 1 && ny >= 1 && nx >= 1 && k <= 65535 && ny < (1 << 30) && nx < (1 << 30) && ny * nx <= INT32_MAX;
}

}  // namespace nd_amd

using namespace nd_amd;

extern "C" size_t nd_amd_coregister_shifts_workspace_bytes(int dtype, int64_t k, int64_t ny, int64_t nx,
                                                           int upsampling)
{
    if ((dtype != ND_AMD_F32 && dtype != ND_AMD_F64) || !shapes_ok(k, ny, nx) || upsampling < 1 ||
        upsampling > ND_AMD_COREG_MAX_UPSAMPLING)
        return 0;
    return shift_layout(dtype, k, ny, nx, upsampling).total;
}

extern "C" int nd_amd_coregister_shifts(const void *c11, int dtype, int64_t k, int64_t ny, int64_t nx,
                                        int64_t stride_t, int64_t stride_y, int64_t stride_x, int64_t reference,
                                        int upsampling, double *shifts, int32_t *status, void *workspace,
                                        size_t workspace_bytes, void *hip_stream)
{
    if (dtype != ND_AMD_F32 && dtype != ND_AMD_F64) {
        set_error("nd_amd_coregister_shifts: dtype must be ND_AMD_F32 or ND_AMD_F64, got %d", dtype);
        return ND_AMD_EINVAL;
    }
    if (!shapes_ok(k, ny, nx)) {
        set_error("nd_amd_coregister_shifts: bad or unsupported shape k=%lld ny=%lld nx=%lld", (long long)k,
                  (long long)ny, (long long)nx);
        return ND_AMD_EINVAL;
    }
    if (reference < 0 || reference >= k) {
        set_error("nd_amd_coregister_shifts: reference %lld outside [0, %lld)", (long long)reference, (long long)k);
        return ND_AMD_EINVAL;
    }
    if (upsampling < 1 || upsampling > ND_AMD_COREG_MAX_UPSAMPLING) {
        set_error("nd_amd_coregister_shifts: upsampling must be in [1, %d], got %d", ND_AMD_COREG_MAX_UPSAMPLING,
                  upsampling);
        return ND_AMD_EINVAL;
    }
    if (!c11 || !shifts || !status) {
        set_error("nd_amd_coregister_shifts: null pointer");
        return ND_AMD_EINVAL;
    }
    if (!workspace || workspace_bytes < shift_layout(dtype, k, ny, nx, upsampling).total ||
        ((uintptr_t)workspace & 255)) {
        set_error("nd_amd_coregister_shifts: workspace missing, too small or not 256-byte aligned");
        return ND_AMD_EWORKSPACE;
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int rc = ND_AMD_EINVAL;
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        rc = coreg_shifts_impl<T>(c11, k, ny, nx, stride_t, stride_y, stride_x, reference, upsampling, shifts,
                                  status, workspace, stream);
    });
    return rc;
}

extern "C" size_t nd_amd_warp_translate_workspace_bytes(int dtype, int nvars, int64_t k, int64_t nr, int64_t nc,
                                                        int layout)
{
    if ((dtype != ND_AMD_F32 && dtype != ND_AMD_F64) || nvars < 1 || nvars > ND_AMD_COREG_MAX_VARS ||
        !shapes_ok(k, nr, nc) || (layout != ND_AMD_LAYOUT_PLANAR && layout != ND_AMD_LAYOUT_PIXEL_MAJOR))
        return 0;
    return warp_layout(dtype, nvars, k, nr, nc, layout).total;
}

extern "C" int nd_amd_warp_translate(const void *const *in, void *const *out, int nvars, int dtype, int64_t k,
                                     int64_t nr, int64_t nc, int layout, const double *shifts, int64_t reference,
                                     void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (dtype != ND_AMD_F32 && dtype != ND_AMD_F64) {
        set_error("nd_amd_warp_translate: dtype must be ND_AMD_F32 or ND_AMD_F64, got %d", dtype);
        return ND_AMD_EINVAL;
    }
    if (layout != ND_AMD_LAYOUT_PLANAR && layout != ND_AMD_LAYOUT_PIXEL_MAJOR) {
        set_error("nd_amd_warp_translate: layout must be ND_AMD_LAYOUT_PLANAR or ND_AMD_LAYOUT_PIXEL_MAJOR");
        return ND_AMD_EINVAL;
    }
    if (nvars < 1 || nvars > ND_AMD_COREG_MAX_VARS || !shapes_ok(k, nr, nc) || (int64_t)nvars * k > 65535) {
        set_error("nd_amd_warp_translate: bad or unsupported shape (nvars=%d k=%lld nr=%lld nc=%lld)", nvars,
                  (long long)k, (long long)nr, (long long)nc);
        return ND_AMD_EINVAL;
    }
    if (reference < -1 || reference >= k) {
        set_error("nd_amd_warp_translate: reference %lld outside [-1, %lld)", (long long)reference, (long long)k);
        return ND_AMD_EINVAL;
    }
    if (!in || !out || !shifts) {
        set_error("nd_amd_warp_translate: null pointer");
        return ND_AMD_EINVAL;
    }
    for (int v = 0; v < nvars; ++v) {
        if (!in[v] || !out[v]) {
            set_error("nd_amd_warp_translate: null plane pointer (variable %d)", v);
            return ND_AMD_EINVAL;
        }
        if (in[v] == out[v]) {
            set_error("nd_amd_warp_translate: output %d is its input (the warp never writes its input)", v);
            return ND_AMD_EINVAL;
        }
    }
    if (!workspace || workspace_bytes < warp_layout(dtype, nvars, k, nr, nc, layout).total ||
        ((uintptr_t)workspace & 255)) {
        set_error("nd_amd_warp_translate: workspace missing, too small or not 256-byte aligned");
        return ND_AMD_EWORKSPACE;
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int rc = ND_AMD_EINVAL;
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        rc = warp_impl<T>(in, out, nvars, k, nr, nc, layout, shifts, reference, workspace, stream);
    });
    return rc;
}
