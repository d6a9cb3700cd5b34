// nd_amd/csrc/resample.hip -- stacks brought onto another rotation-free grid (nd.warp.Resample / Reprojection within
// one coordinate system, nd/warp.py:872-1017).  include/nd_amd.h has the definition, which is this project's.
//
//   nd_amd_resample           out[i, j] = T(sum_r wy[r, i] * (sum_q wx[q, j] * double(src[sy[i] + r, sx[j] + q]))), else fill
//   nd_amd_resample_nearest   out[i, j] = src[sy[i], sx[j]] as a raw word of 1, 2, 4 or 8 bytes, else fill
//   nd_amd_resample_check_table   is every (start, count) of a device table inside its axis?  (synchronises)
//
// The kernels do no coordinate arithmetic: which taps exist and what they weigh is decided on the host, once per axis
// (start[m], count[m], weights[taps][m] tap-major), and shared with the restatement the tests compare with.  One lane
// owns one output element at a time and walks its row taps outside and its column taps inside, which is the definition's
// order.  A block is 256 lanes along the destination's fastest axis, and every lane writes 4 consecutive output rows of
// its column one after the other: the column's table entry, its weights and its address arithmetic are paid once for
// the four, and a wave lies in one output row, so its row table entries are wave-uniform.  Where neither table has
// more than K = 2, 3 or 4 taps the column weights stay in registers and the K x K source elements of an output
// are fetched without a branch between the loads, all in flight together (taps beyond a run repeat its last one and
// are left out of the sums); longer runs are read tap by tap.  The fastest axis is x, or, for a (y, x, time) stack whose
// inner stride is the smaller one in the destination, x and time flattened: such a wave reads and writes runs
// contiguous along time.  The source is read through the caches, without LDS staging: neighbouring lanes and a lane's
// consecutive rows share their lines there.
// An entry of a table that points outside the source makes its output `fill`: nothing outside the source extent the
// caller states is read, whatever the tables hold.
#include "common.hpp"
#include "dispatch.hpp"

#include <string.h>

using namespace nd_amd;

namespace {

constexpr int RS_LANES = 64;                        // along the fast axis: one wave
constexpr int RS_WAVES = 4;                         // waves per block, side by side along the fast axis
constexpr int RS_ROWS = 4;                          // output rows a lane writes, one after the other
constexpr int RS_MAX_TAPS = ND_AMD_RESAMPLE_MAX_TAPS;
constexpr int64_t RS_MAX_PIXELS = (int64_t)1 << 31;
constexpr int64_t RS_MAX_BLOCKS = ((int64_t)1 << 31) - 1;

struct RsArgs {
    const void *src;
    void *dst;
    const int32_t *start_y, *count_y, *start_x, *count_x;
    const double *wy, *wx;
    int64_t nplanes, inner;                         // batch and inner axis
    int64_t sny, snx, ssp, ssy, ssx, ssl;           // source extent and strides (elements)
    int64_t dny, dnx, dsp, dsy, dsx, dsl;           // destination
    int64_t fast;                                   // elements of one output row along the lanes: dnx or dnx * inner
    uint32_t bpr, rgroups;                          // blocks per output row, groups of RS_ROWS rows
    int taps_y, taps_x;
};

struct RsWhere {
    int64_t p, i0, j, l;                            // i0: the first of the block's RS_ROWS output rows
    bool live;
};

// the output column of this lane.  INNER: the lanes run over (x, inner) flattened, inner fastest.
template <bool INNER>
__device__ __forceinline__ RsWhere rs_where(const RsArgs &a)
{
    RsWhere w;
    const uint32_t b = blockIdx.x;
    const uint32_t bf = b % a.bpr, t = b / a.bpr;
    const uint32_t ig = t % a.rgroups, pl = t / a.rgroups;
    w.i0 = (int64_t)ig * RS_ROWS;
    const int64_t f = ((int64_t)bf * RS_WAVES + threadIdx.y) * RS_LANES + threadIdx.x;
    w.live = f < a.fast;
    if (INNER) {
        w.p = pl;
        if (a.fast <= (int64_t)0xffffffffll) {
            w.j = (uint32_t)f / (uint32_t)a.inner;
            w.l = (uint32_t)f % (uint32_t)a.inner;
        } else {
            w.j = f / a.inner;
            w.l = f % a.inner;
        }
    } else {
        w.j = f;
        w.p = pl / (uint32_t)a.inner;
        w.l = pl % (uint32_t)a.inner;
    }
    return w;
}

// a run of `count` taps from `start` lies in [0, n) and in the table's `taps` rows
__device__ __forceinline__ bool rs_run_ok(int32_t start, int32_t count, int64_t n, int taps)
{
    return count > 0 && count <= taps && start >= 0 && (int64_t)start + count <= n;
}

// K > 0: both tables have at most K taps.  A lane keeps its column weights in registers and fetches the K x K source
// elements of an output without a branch between the loads (taps beyond a run repeat its last one and are left out
// of the sums), so that they are all in flight together.  K == 0: any number of taps, read one by one.
template <class T, int K, bool INNER>
__global__ __launch_bounds__(RS_LANES * RS_WAVES) void resample_kernel(RsArgs a, T fill)
{
    const RsWhere w = rs_where<INNER>(a);
    if (!w.live) return;
    const int32_t x0 = a.start_x[w.j];
    int32_t cx = a.count_x[w.j];
    const bool xok = rs_run_ok(x0, cx, a.snx, a.taps_x);
    if (!xok) cx = 0;
    // what the lane's RS_ROWS outputs share: its column of the source and of the destination, its column weights
    const T *col = reinterpret_cast<const T *>(a.src) + (w.p * a.ssp + (int64_t)(xok ? x0 : 0) * a.ssx + w.l * a.ssl);
    T *ocol = reinterpret_cast<T *>(a.dst) + (w.p * a.dsp + w.j * a.dsx + w.l * a.dsl);
    const double *wx = a.wx + w.j;
    constexpr int KK = K > 0 ? K : 1;
    double wq[KK];
    int64_t qoff[KK];
    if constexpr (K > 0) {
#pragma unroll
        for (int q = 0; q < K; q++) {
            const int qq = q < cx ? q : (cx > 0 ? cx - 1 : 0);
            wq[q] = wx[(int64_t)qq * a.dnx];
            qoff[q] = (int64_t)qq * a.ssx;
        }
    }
    const int rows = a.dny - w.i0 < RS_ROWS ? (int)(a.dny - w.i0) : RS_ROWS;
    for (int k = 0; k < rows; k++) {
        const int64_t i = w.i0 + k;                 // wave-uniform, and so is the row's table entry
        const int32_t y0 = a.start_y[i], cy = a.count_y[i];
        T *out = ocol + i * a.dsy;
        if (!xok || !rs_run_ok(y0, cy, a.sny, a.taps_y)) {
            *out = fill;
            continue;
        }
        const T *row = col + (int64_t)y0 * a.ssy;
        const double *wy = a.wy + i;
        double acc = 0.0;
        if constexpr (K > 0) {
            T v[KK][KK];
            double wr[KK];
#pragma unroll
            for (int r = 0; r < K; r++) {
                const int rr = r < cy ? r : cy - 1;
                wr[r] = wy[(int64_t)rr * a.dny];
                const T *from = row + (int64_t)rr * a.ssy;
#pragma unroll
                for (int q = 0; q < K; q++) v[r][q] = from[qoff[q]];
            }
#pragma unroll
            for (int r = 0; r < K; r++) {
                double h = 0.0;
#pragma unroll
                for (int q = 0; q < K; q++) {
                    const double t = h + wq[q] * (double)v[r][q];
                    h = q < cx ? t : h;
                }
                const double t = acc + wr[r] * h;
                acc = r < cy ? t : acc;
            }
        } else {
            for (int r = 0; r < cy; r++) {
                double h = 0.0;
                for (int q = 0; q < cx; q++) h = h + wx[(int64_t)q * a.dnx] * (double)row[(int64_t)q * a.ssx];
                acc = acc + *wy * h;
                row += a.ssy;
                wy += a.dny;
            }
        }
        *out = (T)acc;
    }
}

template <class W, bool INNER>
__global__ __launch_bounds__(RS_LANES * RS_WAVES) void resample_nearest_kernel(RsArgs a, W fill)
{
    const RsWhere w = rs_where<INNER>(a);
    if (!w.live) return;
    const int32_t x0 = a.start_x[w.j], cx = a.count_x[w.j];
    const bool xok = rs_run_ok(x0, cx, a.snx, 1);
    const W *col = reinterpret_cast<const W *>(a.src) + (w.p * a.ssp + (int64_t)(xok ? x0 : 0) * a.ssx + w.l * a.ssl);
    W *ocol = reinterpret_cast<W *>(a.dst) + (w.p * a.dsp + w.j * a.dsx + w.l * a.dsl);
    const int rows = a.dny - w.i0 < RS_ROWS ? (int)(a.dny - w.i0) : RS_ROWS;
    for (int k = 0; k < rows; k++) {
        const int64_t i = w.i0 + k;
        const int32_t y0 = a.start_y[i], cy = a.count_y[i];
        W v = fill;
        if (xok && rs_run_ok(y0, cy, a.sny, 1)) v = col[(int64_t)y0 * a.ssy];
        ocol[i * a.dsy] = v;
    }
}

// flag |= 1 where an entry of the table is neither outside (count 0) nor a run inside [0, n) of at most `taps`
__global__ __launch_bounds__(256) void resample_check_kernel(const int32_t *start, const int32_t *count, int64_t m,
                                                            int64_t n, int taps, int *flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const int32_t c = count[t];
    if (c != 0 && !rs_run_ok(start[t], c, n, taps)) atomicOr(flag, 1);
}

// what the two entries check alike.  -> ND_AMD_OK with *empty set where there is nothing to write
int rs_common(const char *fn, const void *src, void *dst, int64_t nplanes, int64_t inner, int64_t sny, int64_t snx,
              const int64_t *ss, int64_t dny, int64_t dnx, const int64_t *ds, const int32_t *start_y,
              const int32_t *count_y, const int32_t *start_x, const int32_t *count_x, RsArgs &a, bool &inner_fast,
              bool &empty)
{
    empty = false;
    if (nplanes < 0 || inner < 0 || sny < 0 || snx < 0 || dny < 0 || dnx < 0) {
        set_error("%s: negative size nplanes=%lld inner=%lld source=(%lld, %lld) destination=(%lld, %lld)", fn,
                  (long long)nplanes, (long long)inner, (long long)sny, (long long)snx, (long long)dny,
                  (long long)dnx);
        return ND_AMD_EINVAL;
    }
    if (!ss || !ds) {
        set_error("%s: src_strides or dst_strides is null", fn);
        return ND_AMD_EINVAL;
    }
    for (int d = 0; d < 4; d++)
        if (ss[d] < 0 || ds[d] < 0) {
            set_error("%s: negative stride (source %lld, destination %lld at axis %d of plane, y, x, inner)", fn,
                      (long long)ss[d], (long long)ds[d], d);
            return ND_AMD_EINVAL;
        }
    if ((sny > 0 && snx >= RS_MAX_PIXELS / sny + (RS_MAX_PIXELS % sny != 0)) ||
        (dny > 0 && dnx >= RS_MAX_PIXELS / dny + (RS_MAX_PIXELS % dny != 0))) {
        set_error("%s: rasters of 2^31 pixels or more per plane are not served (source %lld x %lld, destination "
                  "%lld x %lld)", fn, (long long)sny, (long long)snx, (long long)dny, (long long)dnx);
        return ND_AMD_EUNSUPPORTED;
    }
    if (nplanes > 0 && inner >= RS_MAX_PIXELS / nplanes + (RS_MAX_PIXELS % nplanes != 0)) {
        set_error("%s: nplanes * inner = %lld * %lld reaches 2^31", fn, (long long)nplanes, (long long)inner);
        return ND_AMD_EUNSUPPORTED;
    }
    if (nplanes == 0 || inner == 0 || dny == 0 || dnx == 0) {
        empty = true;
        return ND_AMD_OK;
    }
    if (!src || !dst || !start_y || !count_y || !start_x || !count_x) {
        set_error("%s: null pointer among src, dst and the tables' start and count", fn);
        return ND_AMD_EINVAL;
    }
    // lanes along the inner axis where that is the closer one in the destination
    inner_fast = inner > 1 && ds[3] < ds[2];
    a.src = src; a.dst = dst;
    a.start_y = start_y; a.count_y = count_y; a.start_x = start_x; a.count_x = count_x;
    a.wy = nullptr; a.wx = nullptr;
    a.nplanes = nplanes; a.inner = inner;
    a.sny = sny; a.snx = snx; a.ssp = ss[0]; a.ssy = ss[1]; a.ssx = ss[2]; a.ssl = ss[3];
    a.dny = dny; a.dnx = dnx; a.dsp = ds[0]; a.dsy = ds[1]; a.dsx = ds[2]; a.dsl = ds[3];
    a.fast = inner_fast ? dnx * inner : dnx;        // below 2^62
    const int64_t bpr = ceil_div(a.fast, RS_LANES * RS_WAVES), rgroups = ceil_div(dny, RS_ROWS);
    const int64_t outer = inner_fast ? nplanes : nplanes * inner;
    if (bpr > RS_MAX_BLOCKS || bpr * rgroups > RS_MAX_BLOCKS || bpr * rgroups > RS_MAX_BLOCKS / outer) {
        set_error("%s: %lld x %lld x %lld blocks are more than one launch holds", fn, (long long)bpr,
                  (long long)rgroups, (long long)outer);
        return ND_AMD_EUNSUPPORTED;
    }
    a.bpr = (uint32_t)bpr; a.rgroups = (uint32_t)rgroups;
    a.taps_y = 1; a.taps_x = 1;
    return ND_AMD_OK;
}

unsigned rs_blocks(const RsArgs &a, bool inner_fast)
{
    return (unsigned)((int64_t)a.bpr * a.rgroups * (inner_fast ? a.nplanes : a.nplanes * a.inner));
}

}  // namespace

extern "C" int nd_amd_resample(const void *src, void *dst, int dtype, int64_t nplanes, int64_t inner, int64_t src_ny,
                               int64_t src_nx, const int64_t *src_strides, int64_t dst_ny, int64_t dst_nx,
                               const int64_t *dst_strides, const int32_t *start_y, const int32_t *count_y,
                               const double *weights_y, int taps_y, const int32_t *start_x, const int32_t *count_x,
                               const double *weights_x, int taps_x, double fill, void *hip_stream)
{
    const char *fn = "nd_amd_resample";
    if (dtype != ND_AMD_F32 && dtype != ND_AMD_F64) {
        set_error("%s: dtype must be ND_AMD_F32 or ND_AMD_F64, got %d", fn, dtype);
        return ND_AMD_EINVAL;
    }
    if (taps_y < 0 || taps_x < 0) {
        set_error("%s: negative tap count (%d, %d)", fn, taps_y, taps_x);
        return ND_AMD_EINVAL;
    }
    if (taps_y > RS_MAX_TAPS || taps_x > RS_MAX_TAPS) {
        set_error("%s: %d x %d taps, at most %d on an axis are served", fn, taps_y, taps_x, RS_MAX_TAPS);
        return ND_AMD_EUNSUPPORTED;
    }
    RsArgs a;
    bool inner_fast = false, empty = false;
    const int rc = rs_common(fn, src, dst, nplanes, inner, src_ny, src_nx, src_strides, dst_ny, dst_nx, dst_strides,
                             start_y, count_y, start_x, count_x, a, inner_fast, empty);
    if (rc != ND_AMD_OK || empty) return rc;
    if (!weights_y || !weights_x) {
        set_error("%s: weights_y or weights_x is null", fn);
        return ND_AMD_EINVAL;
    }
    a.wy = weights_y; a.wx = weights_x;
    a.taps_y = taps_y; a.taps_x = taps_x;

    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    const dim3 grid(rs_blocks(a, inner_fast)), block(RS_LANES, RS_WAVES);
    KernelTimer timer(ND_AMD_KERNEL_RESAMPLE, stream);
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        pick(inner_fast, [&](auto INNER) {
            auto launch = [&](auto KT) {
                hipLaunchKernelGGL((resample_kernel<T, decltype(KT)::value, decltype(INNER)::value>), grid, block, 0,
                                   stream, a, (T)fill);
            };
            if (!pick_le<2, 3, 4>(taps_y > taps_x ? taps_y : taps_x, launch)) launch(int_c<0>{});
        });
    });
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_resample_nearest(const void *src, void *dst, int elem_size, int64_t nplanes, int64_t inner,
                                       int64_t src_ny, int64_t src_nx, const int64_t *src_strides, int64_t dst_ny,
                                       int64_t dst_nx, const int64_t *dst_strides, const int32_t *start_y,
                                       const int32_t *count_y, const int32_t *start_x, const int32_t *count_x,
                                       const void *fill, void *hip_stream)
{
    const char *fn = "nd_amd_resample_nearest";
    if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) {
        set_error("%s: elem_size must be 1, 2, 4 or 8 bytes, got %d", fn, elem_size);
        return ND_AMD_EINVAL;
    }
    if (!fill) {
        set_error("%s: fill is null", fn);
        return ND_AMD_EINVAL;
    }
    RsArgs a;
    bool inner_fast = false, empty = false;
    const int rc = rs_common(fn, src, dst, nplanes, inner, src_ny, src_nx, src_strides, dst_ny, dst_nx, dst_strides,
                             start_y, count_y, start_x, count_x, a, inner_fast, empty);
    if (rc != ND_AMD_OK || empty) return rc;
    if (((uintptr_t)src | (uintptr_t)dst) & (uintptr_t)(elem_size - 1)) {
        set_error("%s: src and dst must be aligned to the element's %d bytes", fn, elem_size);
        return ND_AMD_EINVAL;
    }
    uint64_t fill_bits = 0;
    memcpy(&fill_bits, fill, (size_t)elem_size);    // little-endian: the low bytes are the element

    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    const dim3 grid(rs_blocks(a, inner_fast)), block(RS_LANES, RS_WAVES);
    KernelTimer timer(ND_AMD_KERNEL_RESAMPLE, stream);
    pick(inner_fast, [&](auto INNER) {
        auto launch = [&](auto BYTES) {
            constexpr int B = decltype(BYTES)::value;
            using W = std::conditional_t<B == 1, uint8_t, std::conditional_t<B == 2, uint16_t,
                      std::conditional_t<B == 4, uint32_t, uint64_t>>>;
            hipLaunchKernelGGL((resample_nearest_kernel<W, decltype(INNER)::value>), grid, block, 0, stream, a,
                               (W)fill_bits);
        };
        pick_eq<1, 2, 4, 8>(elem_size, launch);
    });
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_resample_check_table(const int32_t *start, const int32_t *count, int64_t m, int64_t n, int taps,
                                           void *hip_stream)
{
    const char *fn = "nd_amd_resample_check_table";
    if (m < 0 || n < 0 || taps < 0) {
        set_error("%s: negative size m=%lld n=%lld taps=%d", fn, (long long)m, (long long)n, taps);
        return ND_AMD_EINVAL;
    }
    if (m >= RS_MAX_PIXELS || n >= RS_MAX_PIXELS) {
        set_error("%s: axes of 2^31 samples or more are not served (m=%lld n=%lld)", fn, (long long)m, (long long)n);
        return ND_AMD_EUNSUPPORTED;
    }
    if (taps > RS_MAX_TAPS) {
        set_error("%s: %d taps, at most %d on an axis are served", fn, taps, RS_MAX_TAPS);
        return ND_AMD_EUNSUPPORTED;
    }
    if (m == 0) return ND_AMD_OK;
    if (!start || !count) {
        set_error("%s: start or count is null", fn);
        return ND_AMD_EINVAL;
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    int *flag = nullptr, host = 0;
    ND_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&flag), sizeof(int)));
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(resample_check_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, stream, start, count,
                           m, n, taps, flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(flag);
    ND_HIP_CHECK(e);
    if (host) {
        set_error("%s: count / start out of range: a run must be empty (count 0) or lie in [0, %lld) with at most %d "
                  "taps", fn, (long long)n, taps);
        return ND_AMD_EINVAL;
    }
    return ND_AMD_OK;
}
