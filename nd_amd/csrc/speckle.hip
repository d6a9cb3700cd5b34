// nd_amd/csrc/speckle.hip -- adaptive speckle filters on detected (intensity) stacks.  include/nd_amd.h has the
// definition, which is this project's: the reference has no counterpart.
//
//   nd_amd_speckle_lee             the local-statistics filter of Lee 1980 / Kuan et al. 1985, per plane
//   nd_amd_speckle_multitemporal   the temporal filter of Quegan & Yu 2001 over k dates of up to 4 variables
//
// Both rest on the window sums S1 (of x) and S2 (of x * x) around every pixel, formed in float64 exactly as the
// definition brackets them: the row sums h1 / h2 of a source row with taps ascending, then the sum of the w row sums
// with rows ascending.  A block of 256 lanes owns a tile of TY x 64 outputs.  It stages the tile plus R halo rows and
// columns of the source in LDS with the reflect index map applied while staging (so nothing later branches on a
// border), forms h1 / h2 ONCE per staged (row, column) into LDS as doubles, and then every lane adds the w row sums of
// its outputs and evaluates the formula.  Lanes run along x; the 4 waves of a block take rows 4 apart.  w = 3, 5, 7, 9
// and 11 have unrolled instantiations, other widths loop with the same order of additions.
// The multitemporal filter needs r = sum over the dates of x / m at every pixel before it can write anything:
//   general form   pass 1 walks a tile through all planes and leaves r in a float64 workspace plane, pass 2 forms m
//                  again for every plane and writes: two reads and one write of the stack
//   hot form       k * C <= 32: a block of 8 x 64 outputs keeps every m[c, t] of its two pixels per lane in registers
//                  (statically indexed: the loop over the planes is unrolled over the templated bound and guarded by
//                  p < k * C), finishes r and writes all planes without reading the stack again
// Both forms do the same operations in the same order on every pixel, so they give the same bits.
// Strides are arbitrary (in elements), so crops and (y, x, time) data are read where they lie; the latter without
// coalescing: the filter classes bring such data to the planar layout first (kernels.relayout_planar).
#include "borders.hpp"
#include "common.hpp"
#include "dispatch.hpp"

using namespace nd_amd;

namespace {

constexpr int SP_TX = ND_AMD_SPECKLE_TILE_X;        // outputs along x: one wave
constexpr int SP_TY = ND_AMD_SPECKLE_TILE_Y;        // output rows of a tile
constexpr int SP_TY_HOT = ND_AMD_SPECKLE_HOT_TILE_Y;    // the same in the one-launch multitemporal form
constexpr int SP_WAVES = 4;
constexpr int SP_THREADS = SP_TX * SP_WAVES;
constexpr int SP_MAX_W = ND_AMD_SPECKLE_MAX_W;
constexpr int SP_MAX_VARS = ND_AMD_SPECKLE_MAX_VARIABLES;
constexpr int SP_HOT_MAX = ND_AMD_SPECKLE_HOT_MAX_PLANES;
constexpr int64_t SP_MAX_PIXELS = (int64_t)1 << 31;
constexpr int64_t SP_MAX_BLOCKS = ((int64_t)1 << 31) - 1;

static_assert(SP_TX == 64, "lanes of a wave run along x");
static_assert(SP_TY % SP_WAVES == 0 && SP_TY_HOT % SP_WAVES == 0, "the waves of a block take rows SP_WAVES apart");

struct SpArgs {
    const void *src[SP_MAX_VARS];
    void *dst[SP_MAX_VARS];
    double *work;                                   // multitemporal, general form: r, (ny, nx) contiguous
    int64_t nplanes, ny, nx;                        // planes of a variable (Lee: the batch; multitemporal: k)
    int64_t ssp, ssy, ssx, dsp, dsy, dsx;           // strides in elements: plane, y, x
    uint32_t tiles_x, tiles_y;
    int w, nvar;
    double n, cu2, kuan, count;                     // w * w, 1 / looks, 1 + cu2, k * C
};

// a variable's base pointer by a select chain: the argument struct is never indexed at run time
template <class T>
__device__ __forceinline__ const T *sp_src(const SpArgs &a, int c)
{
    const void *p = c == 0 ? a.src[0] : c == 1 ? a.src[1] : c == 2 ? a.src[2] : a.src[3];
    return reinterpret_cast<const T *>(p);
}
template <class T>
__device__ __forceinline__ T *sp_dst(const SpArgs &a, int c)
{
    void *p = c == 0 ? a.dst[0] : c == 1 ? a.dst[1] : c == 2 ? a.dst[2] : a.dst[3];
    return reinterpret_cast<T *>(p);
}

// where the block's LDS arrays lie for a tile of TY rows: h1, h2 (SQ only), then the staged source
template <class T, int TY, bool SQ>
struct SpLds {
    double *h1, *h2;
    T *stage;
    int sw;                                         // staged columns: SP_TX + 2 R
    __device__ SpLds(unsigned char *base, int w)
    {
        const int rows = TY + (w - 1);
        h1 = reinterpret_cast<double *>(base);
        h2 = h1 + (SQ ? rows * SP_TX : 0);
        stage = reinterpret_cast<T *>(h2 + rows * SP_TX);
        sw = SP_TX + (w - 1);
    }
};

template <class T, bool SQ>
size_t sp_lds_bytes(int ty, int w)
{
    const size_t rows = (size_t)ty + (w - 1);
    return rows * SP_TX * sizeof(double) * (SQ ? 2 : 1) + rows * (SP_TX + (w - 1)) * sizeof(T);
}

// Stage rows [y0 - R, y0 + live + R) x columns [x0 - R, x0 + 64 + R) of `plane`, reflected, and form their row sums.
// `live` is the number of tile rows inside the plane, the same in every lane.  Ends behind a barrier: h1 / h2 and the
// staged samples may be read by any lane.  Starts with one: the previous plane's readers are done.
template <class T, int W, bool SQ>
__device__ __forceinline__ void sp_row_sums(const T *plane, int64_t sy, int64_t sx, int64_t ny, int64_t nx,
                                            int64_t y0, int64_t x0, int live, int w, T *stage, double *h1,
                                            double *h2, int sw)
{
    const int ww = W > 0 ? W : w, R = ww / 2;
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int rows = live + 2 * R;
    // the lane's two staged columns (sw <= 64 + 30 < 128)
    const int64_t c0 = reflect_line(x0 - R + lane, nx) * sx;
    const int64_t c1 = lane + SP_TX < sw ? reflect_line(x0 - R + lane + SP_TX, nx) * sx : 0;
    __syncthreads();
    for (int r = wave; r < rows; r += SP_WAVES) {
        const T *row = plane + reflect_line(y0 - R + r, ny) * sy;
        stage[r * sw + lane] = row[c0];
        if (lane + SP_TX < sw) stage[r * sw + lane + SP_TX] = row[c1];
    }
    __syncthreads();
    for (int r = wave; r < rows; r += SP_WAVES) {
        const T *s = stage + r * sw + lane;
        double a = 0.0, b = 0.0;
        if constexpr (W > 0) {
#pragma unroll
            for (int d = 0; d < W; d++) {
                const double v = (double)s[d];
                a = a + v;
                if (SQ) b = b + v * v;
            }
        } else {
            for (int d = 0; d < ww; d++) {
                const double v = (double)s[d];
                a = a + v;
                if (SQ) b = b + v * v;
            }
        }
        h1[r * SP_TX + lane] = a;
        if (SQ) h2[r * SP_TX + lane] = b;
    }
    __syncthreads();
}

// the sum of the w row sums above and below output row i of the tile, rows ascending
template <int W>
__device__ __forceinline__ double sp_col_sum(const double *h, int i, int lane, int w)
{
    const double *p = h + i * SP_TX + lane;
    double s = 0.0;
    if constexpr (W > 0) {
#pragma unroll
        for (int d = 0; d < W; d++) s = s + p[d * SP_TX];
    } else {
        for (int d = 0; d < w; d++) s = s + p[d * SP_TX];
    }
    return s;
}

struct SpTile {
    int64_t y0, x0, plane;
    int live;                                       // tile rows inside the plane
    bool col;                                       // this lane's column is inside the plane
};

template <int TY>
__device__ __forceinline__ SpTile sp_tile(const SpArgs &a)
{
    SpTile t;
    const uint32_t b = blockIdx.x;
    const uint32_t bx = b % a.tiles_x, q = b / a.tiles_x;
    t.x0 = (int64_t)bx * SP_TX;
    t.y0 = (int64_t)(q % a.tiles_y) * TY;
    t.plane = q / a.tiles_y;
    t.live = a.ny - t.y0 < TY ? (int)(a.ny - t.y0) : TY;
    t.col = t.x0 + threadIdx.x < a.nx;
    return t;
}

template <class T, int W>
__global__ __launch_bounds__(SP_THREADS) void speckle_lee_kernel(SpArgs a, int kuan)
{
    extern __shared__ __align__(16) unsigned char nd_smem_speckle[];
    const int w = W > 0 ? W : a.w, R = w / 2;
    const SpLds<T, SP_TY, true> l(nd_smem_speckle, w);
    const SpTile t = sp_tile<SP_TY>(a);
    const int lane = threadIdx.x, wave = threadIdx.y;
    const T *plane = reinterpret_cast<const T *>(a.src[0]) + t.plane * a.ssp;
    sp_row_sums<T, W, true>(plane, a.ssy, a.ssx, a.ny, a.nx, t.y0, t.x0, t.live, w, l.stage, l.h1, l.h2, l.sw);
    if (!t.col) return;
    T *out = reinterpret_cast<T *>(a.dst[0]) + t.plane * a.dsp + (t.x0 + lane) * a.dsx;
    for (int i = wave; i < t.live; i += SP_WAVES) {
        const double s1 = sp_col_sum<W>(l.h1, i, lane, w), s2 = sp_col_sum<W>(l.h2, i, lane, w);
        const double x = (double)l.stage[(i + R) * l.sw + lane + R];
        const double m = s1 / a.n;
        const double v = s2 / a.n - m * m;
        const double q = ((m * m) * a.cu2) / v;
        double b = 1.0 - q;
        if (kuan) b = b / a.kuan;
        b = (v > 0.0 && b > 0.0) ? b : 0.0;
        out[(t.y0 + i) * a.dsy] = (T)(m + b * (x - m));
    }
}

// general form, pass 1: r of every pixel of the tile into the workspace plane
template <class T, int W>
__global__ __launch_bounds__(SP_THREADS) void speckle_mt_ratio_kernel(SpArgs a)
{
    extern __shared__ __align__(16) unsigned char nd_smem_speckle[];
    constexpr int PX = SP_TY / SP_WAVES;
    const int w = W > 0 ? W : a.w, R = w / 2;
    const SpLds<T, SP_TY, false> l(nd_smem_speckle, w);
    const SpTile t = sp_tile<SP_TY>(a);
    const int lane = threadIdx.x, wave = threadIdx.y;
    double r[PX];
#pragma unroll
    for (int u = 0; u < PX; u++) r[u] = 0.0;
    for (int64_t d = 0; d < a.nplanes; d++)
        for (int c = 0; c < a.nvar; c++) {
            sp_row_sums<T, W, false>(sp_src<T>(a, c) + d * a.ssp, a.ssy, a.ssx, a.ny, a.nx, t.y0, t.x0, t.live, w,
                                     l.stage, l.h1, l.h1, l.sw);
#pragma unroll
            for (int u = 0; u < PX; u++) {
                const int i = wave + u * SP_WAVES;
                if (i < t.live) {
                    const double m = sp_col_sum<W>(l.h1, i, lane, w) / a.n;
                    r[u] = r[u] + (double)l.stage[(i + R) * l.sw + lane + R] / m;
                }
            }
        }
    if (!t.col) return;
#pragma unroll
    for (int u = 0; u < PX; u++) {
        const int i = wave + u * SP_WAVES;
        if (i < t.live) a.work[(t.y0 + i) * a.nx + t.x0 + lane] = r[u];
    }
}

// general form, pass 2: one plane of one variable per block, plane index = date * nvar + variable
template <class T, int W>
__global__ __launch_bounds__(SP_THREADS) void speckle_mt_apply_kernel(SpArgs a)
{
    extern __shared__ __align__(16) unsigned char nd_smem_speckle[];
    const int w = W > 0 ? W : a.w;
    const SpLds<T, SP_TY, false> l(nd_smem_speckle, w);
    const SpTile t = sp_tile<SP_TY>(a);
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int64_t d = t.plane / a.nvar;
    const int c = (int)(t.plane % a.nvar);
    sp_row_sums<T, W, false>(sp_src<T>(a, c) + d * a.ssp, a.ssy, a.ssx, a.ny, a.nx, t.y0, t.x0, t.live, w, l.stage,
                             l.h1, l.h1, l.sw);
    if (!t.col) return;
    T *out = sp_dst<T>(a, c) + d * a.dsp + (t.x0 + lane) * a.dsx;
    for (int i = wave; i < t.live; i += SP_WAVES) {
        const double m = sp_col_sum<W>(l.h1, i, lane, w) / a.n;
        const double r = a.work[(t.y0 + i) * a.nx + t.x0 + lane];
        out[(t.y0 + i) * a.dsy] = (T)((m * r) / a.count);
    }
}

// hot form: k * C <= KMAX planes, every m of the lane's pixels kept in registers between the two walks
template <class T, int W, int KMAX>
__global__ __launch_bounds__(SP_THREADS) void speckle_mt_hot_kernel(SpArgs a)
{
    extern __shared__ __align__(16) unsigned char nd_smem_speckle[];
    constexpr int PX = SP_TY_HOT / SP_WAVES;
    const int w = W > 0 ? W : a.w, R = w / 2;
    const SpLds<T, SP_TY_HOT, false> l(nd_smem_speckle, w);
    const SpTile t = sp_tile<SP_TY_HOT>(a);
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int planes = (int)a.nplanes * a.nvar;
    double m[PX][KMAX], r[PX];
#pragma unroll
    for (int u = 0; u < PX; u++) r[u] = 0.0;
    {
        int64_t d = 0;
        int c = 0;
#pragma unroll
        for (int p = 0; p < KMAX; p++) {
            if (p < planes) {
                sp_row_sums<T, W, false>(sp_src<T>(a, c) + d * a.ssp, a.ssy, a.ssx, a.ny, a.nx, t.y0, t.x0, t.live, w,
                                         l.stage, l.h1, l.h1, l.sw);
#pragma unroll
                for (int u = 0; u < PX; u++) {
                    const int i = wave + u * SP_WAVES;
                    if (i < t.live) {
                        m[u][p] = sp_col_sum<W>(l.h1, i, lane, w) / a.n;
                        r[u] = r[u] + (double)l.stage[(i + R) * l.sw + lane + R] / m[u][p];
                    }
                }
                if (++c == a.nvar) {
                    c = 0;
                    d++;
                }
            }
        }
    }
    if (!t.col) return;
    int64_t d = 0;
    int c = 0;
#pragma unroll
    for (int p = 0; p < KMAX; p++) {
        if (p < planes) {
            T *out = sp_dst<T>(a, c) + d * a.dsp + (t.x0 + lane) * a.dsx;
#pragma unroll
            for (int u = 0; u < PX; u++) {
                const int i = wave + u * SP_WAVES;
                if (i < t.live) out[(t.y0 + i) * a.dsy] = (T)((m[u][p] * r[u]) / a.count);
            }
            if (++c == a.nvar) {
                c = 0;
                d++;
            }
        }
    }
}

// what the two entries check alike; fills the geometry of `a`.  *empty: nothing to write
int sp_common(const char *fn, int dtype, int64_t nplanes, int64_t ny, int64_t nx, const int64_t *ss,
              const int64_t *ds, int w, SpArgs &a, bool &empty)
{
    empty = false;
    if (dtype != ND_AMD_F32 && dtype != ND_AMD_F64) {
        set_error("%s: dtype must be ND_AMD_F32 or ND_AMD_F64, got %d", fn, dtype);
        return ND_AMD_EINVAL;
    }
    if (nplanes < 0 || ny < 0 || nx < 0) {
        set_error("%s: negative size planes=%lld ny=%lld nx=%lld", fn, (long long)nplanes, (long long)ny,
                  (long long)nx);
        return ND_AMD_EINVAL;
    }
    if (!ss || !ds) {
        set_error("%s: src_strides or dst_strides is null", fn);
        return ND_AMD_EINVAL;
    }
    for (int d = 0; d < 3; d++)
        if (ss[d] < 0 || ds[d] < 0) {
            set_error("%s: negative stride (source %lld, destination %lld at axis %d of plane, y, x)", fn,
                      (long long)ss[d], (long long)ds[d], d);
            return ND_AMD_EINVAL;
        }
    if (w < 1) {
        set_error("%s: w must be positive, got %d", fn, w);
        return ND_AMD_EINVAL;
    }
    if (w % 2 == 0 || w > SP_MAX_W) {
        set_error("%s: w = %d: odd windows up to %d are served", fn, w, SP_MAX_W);
        return ND_AMD_EUNSUPPORTED;
    }
    if (ny > 0 && nx >= SP_MAX_PIXELS / ny + (SP_MAX_PIXELS % ny != 0)) {
        set_error("%s: planes of 2^31 pixels or more are not served (%lld x %lld)", fn, (long long)ny, (long long)nx);
        return ND_AMD_EUNSUPPORTED;
    }
    if (nplanes == 0 || ny == 0 || nx == 0) {
        empty = true;
        return ND_AMD_OK;
    }
    for (int c = 0; c < SP_MAX_VARS; c++) {
        a.src[c] = nullptr;
        a.dst[c] = nullptr;
    }
    a.work = nullptr;
    a.nplanes = nplanes; a.ny = ny; a.nx = nx;
    a.ssp = ss[0]; a.ssy = ss[1]; a.ssx = ss[2];
    a.dsp = ds[0]; a.dsy = ds[1]; a.dsx = ds[2];
    a.w = w; a.nvar = 1;
    a.n = (double)(w * w);
    a.cu2 = 0.0; a.kuan = 1.0; a.count = 1.0;
    return ND_AMD_OK;
}

// tiles of `ty` rows, `batch` of them per tile position, as one 1-D grid
int sp_grid(const char *fn, SpArgs &a, int ty, int64_t batch, unsigned &blocks)
{
    const int64_t bx = ceil_div(a.nx, SP_TX), by = ceil_div(a.ny, ty);
    if (bx * by > SP_MAX_BLOCKS / batch) {
        set_error("%s: %lld x %lld x %lld blocks are more than one launch holds", fn, (long long)bx, (long long)by,
                  (long long)batch);
        return ND_AMD_EUNSUPPORTED;
    }
    a.tiles_x = (uint32_t)bx;
    a.tiles_y = (uint32_t)by;
    blocks = (unsigned)(bx * by * batch);
    return ND_AMD_OK;
}

// f(T, W): the data's type and the window's instantiation (0 = the loop form)
template <class F>
void sp_pick(int dtype, int w, F &&f)
{
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        auto g = [&](auto W) { f(T{}, W); };
        if (!pick_eq<3, 5, 7, 9, 11>(w, g)) g(int_c<0>{});
    });
}

template <class Kernel, class... Args>
hipError_t sp_launch(Kernel *kernel, unsigned blocks, size_t lds, hipStream_t stream, Args... args)
{
    // on every launch that needs it: the attribute belongs to the current device's function object
    hipError_t e = lds > 64 * 1024 ? allow_dynamic_lds(kernel, lds) : hipSuccess;
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(SP_TX, SP_WAVES), lds, stream, args...);
    return hipGetLastError();
}

bool sp_hot(int64_t k, int nvar) { return k <= SP_HOT_MAX / nvar; }

}  // namespace

extern "C" int nd_amd_speckle_lee(const void *src, void *dst, int dtype, int64_t nplanes, int64_t ny, int64_t nx,
                                  const int64_t *src_strides, const int64_t *dst_strides, int w, double cu2,
                                  int method, void *hip_stream)
{
    const char *fn = "nd_amd_speckle_lee";
    SpArgs a;
    bool empty = false;
    if (method != ND_AMD_SPECKLE_LEE && method != ND_AMD_SPECKLE_KUAN) {
        set_error("%s: method must be ND_AMD_SPECKLE_LEE or ND_AMD_SPECKLE_KUAN, got %d", fn, method);
        return ND_AMD_EINVAL;
    }
    if (!(cu2 > 0.0) || !(cu2 <= 1.7976931348623157e308)) {
        set_error("%s: cu2 = 1 / looks must be positive and finite, got %g", fn, cu2);
        return ND_AMD_EINVAL;
    }
    int rc = sp_common(fn, dtype, nplanes, ny, nx, src_strides, dst_strides, w, a, empty);
    if (rc != ND_AMD_OK || empty) return rc;
    if (!src || !dst) {
        set_error("%s: src or dst is null", fn);
        return ND_AMD_EINVAL;
    }
    a.src[0] = src;
    a.dst[0] = dst;
    a.cu2 = cu2;
    a.kuan = 1.0 + cu2;
    unsigned blocks = 0;
    rc = sp_grid(fn, a, SP_TY, nplanes, blocks);
    if (rc != ND_AMD_OK) return rc;

    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    hipError_t e = hipSuccess;
    KernelTimer timer(ND_AMD_KERNEL_SPECKLE, stream);
    sp_pick(dtype, w, [&](auto t, auto W) {
        using T = decltype(t);
        e = sp_launch(&speckle_lee_kernel<T, decltype(W)::value>, blocks, sp_lds_bytes<T, true>(SP_TY, w), stream, a,
                      method == ND_AMD_SPECKLE_KUAN ? 1 : 0);
    });
    ND_HIP_CHECK(e);
    return ND_AMD_OK;
}

extern "C" size_t nd_amd_speckle_multitemporal_workspace_bytes(int64_t ny, int64_t nx, int64_t k, int nvar)
{
    if (ny <= 0 || nx <= 0 || k <= 0 || nvar < 1 || nvar > SP_MAX_VARS) return 0;
    if (nx >= SP_MAX_PIXELS / ny + (SP_MAX_PIXELS % ny != 0)) return 0;
    return sp_hot(k, nvar) ? 0 : (size_t)ny * (size_t)nx * sizeof(double);
}

extern "C" int nd_amd_speckle_multitemporal(const void *const *src, void *const *dst, int nvar, int dtype, int64_t k,
                                            int64_t ny, int64_t nx, const int64_t *src_strides,
                                            const int64_t *dst_strides, int w, void *workspace,
                                            size_t workspace_bytes, void *hip_stream)
{
    const char *fn = "nd_amd_speckle_multitemporal";
    SpArgs a;
    bool empty = false;
    if (nvar < 1) {
        set_error("%s: nvar must be positive, got %d", fn, nvar);
        return ND_AMD_EINVAL;
    }
    if (nvar > SP_MAX_VARS) {
        set_error("%s: %d variables, at most %d are filtered jointly", fn, nvar, SP_MAX_VARS);
        return ND_AMD_EUNSUPPORTED;
    }
    int rc = sp_common(fn, dtype, k, ny, nx, src_strides, dst_strides, w, a, empty);
    if (rc != ND_AMD_OK || empty) return rc;
    if (!src || !dst) {
        set_error("%s: src or dst is null", fn);
        return ND_AMD_EINVAL;
    }
    for (int c = 0; c < nvar; c++) {
        if (!src[c] || !dst[c]) {
            set_error("%s: src[%d] or dst[%d] is null", fn, c, c);
            return ND_AMD_EINVAL;
        }
        a.src[c] = src[c];
        a.dst[c] = dst[c];
    }
    if (k > SP_MAX_BLOCKS / nvar) {
        set_error("%s: k * nvar = %lld * %d reaches 2^31", fn, (long long)k, nvar);
        return ND_AMD_EUNSUPPORTED;
    }
    a.nvar = nvar;
    a.count = (double)(k * nvar);
    const bool hot = sp_hot(k, nvar);
    const size_t need = nd_amd_speckle_multitemporal_workspace_bytes(ny, nx, k, nvar);
    if (!hot && (!workspace || workspace_bytes < need)) {
        set_error("%s: the two-pass form (k * nvar = %lld > %d) needs a workspace of %zu bytes, got %zu", fn,
                  (long long)(k * nvar), SP_HOT_MAX, need, workspace_bytes);
        return ND_AMD_EWORKSPACE;
    }
    a.work = reinterpret_cast<double *>(workspace);

    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    hipError_t e = hipSuccess;
    unsigned blocks = 0;
    KernelTimer timer(ND_AMD_KERNEL_SPECKLE, stream);
    if (hot) {
        rc = sp_grid(fn, a, SP_TY_HOT, 1, blocks);
        if (rc != ND_AMD_OK) return rc;
        sp_pick(dtype, w, [&](auto t, auto W) {
            using T = decltype(t);
            const size_t lds = sp_lds_bytes<T, false>(SP_TY_HOT, w);
            pick_le<8, SP_HOT_MAX>((int)(k * nvar), [&](auto KMAX) {
                e = sp_launch(&speckle_mt_hot_kernel<T, decltype(W)::value, decltype(KMAX)::value>, blocks, lds,
                              stream, a);
            });
        });
        ND_HIP_CHECK(e);
        return ND_AMD_OK;
    }
    rc = sp_grid(fn, a, SP_TY, k * nvar, blocks);   // the larger grid first: both must fit
    if (rc != ND_AMD_OK) return rc;
    const unsigned apply_blocks = blocks;
    rc = sp_grid(fn, a, SP_TY, 1, blocks);
    if (rc != ND_AMD_OK) return rc;
    sp_pick(dtype, w, [&](auto t, auto W) {
        using T = decltype(t);
        const size_t lds = sp_lds_bytes<T, false>(SP_TY, w);
        e = sp_launch(&speckle_mt_ratio_kernel<T, decltype(W)::value>, blocks, lds, stream, a);
        if (e == hipSuccess)
            e = sp_launch(&speckle_mt_apply_kernel<T, decltype(W)::value>, apply_blocks, lds, stream, a);
    });
    ND_HIP_CHECK(e);
    return ND_AMD_OK;
}
