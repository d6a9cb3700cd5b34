// nd_amd/csrc/temporal.hip -- per-pixel statistics along the series of a stack: count, sum, mean, the second moment
// and what derives from it, minimum and maximum with their dates, the median and percentiles.
// include/nd_amd.h has the definition ("Statistics along time"); tests/temporal_ref.py restates it bit for bit.
//
// One lane owns one pixel; a block is one wave of 64 pixels that are neighbours along the kept dim with the smaller
// stride.  Every floating-point result is a function of the pixel's own series in date order, so the three forms and
// the two ways of reading give the same bits:
//
//   register form   k <= TS_REG_MAX<T>: the series sits in KP = 8, 16, 32 or 64 registers by static index, padded with
//                   NaN.  The moments take both passes from the registers.  For the order statistics the values become
//                   order-preserving keys (NaN and padding: the largest key), a bitonic network of compare-exchanges
//                   with constant indices sorts them, and a rank is read by a tree of selects.
//   LDS form        k <= TS_LDS_MAX<T>: the wave's series lie in LDS as [date][lane], the lane's column rotated by the
//                   date so that a lane walking its column and a wave writing one pixel's dates both touch 64 different
//                   banks.  Each lane sorts its own column there (the same network, run-time indices) after the moments
//                   have been taken from it in date order.
//   streaming form  no order statistic asked for and k beyond the register form: two walks over memory, the second
//                   only if m2 or what derives from it is wanted.  (A contiguous series that fits the LDS form's tile
//                   goes through that form instead, which then sorts nothing.)
//
//   reading         direct: each lane loads its own elements date by date; (time, y, x) data are coalesced that way,
//                   crops and steps are merely correct.  staged: series stride 1 and pixels k apart ((y, x, time)
//                   data): the wave's run of 64 * k contiguous elements is loaded with consecutive lanes on consecutive
//                   elements and handed to its owners through LDS; nothing is transposed in memory.
// No kernel indexes a private array at run time.
#include <math.h>
#include <string.h>

#include "common.hpp"
#include "dispatch.hpp"

using namespace nd_amd;

namespace {

constexpr int TS_LANES = 64;                        // pixels of a block: one wave
constexpr int TS_MAXQ = 8;                          // percentiles of one launch
constexpr int TS_LDS_BYTES = 64 * 1024;             // what a block's tile may take
constexpr int64_t TS_MAX_BLOCKS = ((int64_t)1 << 26) - 1;   // a launch holds fewer than 2^32 threads, 64 to a block
// the forms; TS_FORM_AUTO is the library's own choice and all that the public entry passes
enum { TS_FORM_AUTO = 0, TS_FORM_REGISTER = 1, TS_FORM_LDS = 2, TS_FORM_STREAM = 3 };

template <class T> struct TsLimits;
template <> struct TsLimits<float> { static constexpr int reg = ND_AMD_TEMPORAL_REG_MAX_F32; };
template <> struct TsLimits<double> { static constexpr int reg = ND_AMD_TEMPORAL_REG_MAX_F64; };
static_assert(ND_AMD_TEMPORAL_LDS_MAX_F32 * TS_LANES * sizeof(float) <= TS_LDS_BYTES, "a float32 tile must fit");
static_assert(ND_AMD_TEMPORAL_LDS_MAX_F64 * TS_LANES * sizeof(double) <= TS_LDS_BYTES, "a float64 tile must fit");

struct TsArgs {
    const void *x;
    int64_t st, s_slow, s_fast;                     // element strides: series, the rows of lanes, the lanes
    int64_t o_slow, o_fast;                         // the same two in the outputs, which are (ny, nx) contiguous
    int64_t nfast, blocks_per_row, plane;           // plane: ny * nx, the pitch of the percentile planes
    int k, kpad;                                    // kpad: rows of the LDS form's tile: k, or a power of two >= k to sort
    int skipna, ddof, nq;
    double q[TS_MAXQ];
    int32_t *count, *nan_count, *argmin, *argmax;
    double *sum, *mean, *m2, *var, *std, *cv;
    void *mn, *mx, *median, *pct;
};

// ---- order-preserving keys: a < b as values iff key(a) < key(b) as unsigned integers; NaN is the largest key
template <class T> struct TsKey;
template <> struct TsKey<float> {
    typedef uint32_t U;
    static __device__ __forceinline__ U enc(float v)
    {
        const U u = __float_as_uint(v);
        return v != v ? ~(U)0 : ((u >> 31) ? ~u : (u | 0x80000000u));
    }
    static __device__ __forceinline__ float dec(U k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
};
template <> struct TsKey<double> {
    typedef uint64_t U;
    static __device__ __forceinline__ U enc(double v)
    {
        const U u = (U)__double_as_longlong(v);
        return v != v ? ~(U)0 : ((u >> 63) ? ~u : (u | 0x8000000000000000ull));
    }
    static __device__ __forceinline__ double dec(U k)
    {
        return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
    }
};

template <class T> __device__ __forceinline__ T ts_value(typename TsKey<T>::U bits);
template <> __device__ __forceinline__ float ts_value<float>(uint32_t bits) { return __uint_as_float(bits); }
template <> __device__ __forceinline__ double ts_value<double>(uint64_t bits) { return __longlong_as_double((long long)bits); }

template <class T> __device__ __forceinline__ T ts_nan();
template <> __device__ __forceinline__ float ts_nan<float>() { return __uint_as_float(0x7fc00000u); }
template <> __device__ __forceinline__ double ts_nan<double>() { return __longlong_as_double(0x7ff8000000000000ll); }

// where date t of the block's pixel p lies in the tile
__device__ __forceinline__ int ts_at(int t, int p) { return t * TS_LANES + ((p + t) & (TS_LANES - 1)); }

// ---- what a lane keeps of its series
template <class T> struct TsMoments {
    int n, nans, amin, amax, first_nan;
    double sum, mean, m2;
    T mn, mx;
};

template <class T> __device__ __forceinline__ void ts_clear(TsMoments<T> &m)
{
    m.n = m.nans = 0;
    m.amin = m.amax = m.first_nan = -1;
    m.sum = m.m2 = 0.0;
    m.mean = 0.0;
    m.mn = m.mx = ts_nan<T>();
}

// the first walk, date t
template <class T> __device__ __forceinline__ void ts_first(TsMoments<T> &m, T x, int t, bool skipna)
{
    const bool isnan = x != x;
    if (isnan) {
        if (m.nans == 0) m.first_nan = t;
        ++m.nans;
    } else {
        if (m.amin < 0 || x < m.mn) { m.mn = x; m.amin = t; }
        if (m.amax < 0 || x > m.mx) { m.mx = x; m.amax = t; }
    }
    if (!isnan || !skipna) {
        ++m.n;
        m.sum = m.sum + (double)x;
    }
}

// the second walk
template <class T> __device__ __forceinline__ void ts_second(TsMoments<T> &m, T x, bool skipna)
{
    if (x == x || !skipna) {
        const double d = (double)x - m.mean;
        m.m2 = m.m2 + d * d;
    }
}

__device__ __forceinline__ bool ts_wants_second(const TsArgs &a) { return a.m2 || a.var || a.std || a.cv; }
__device__ __forceinline__ bool ts_wants_order(const TsArgs &a) { return a.median || a.nq > 0; }

template <class T> __device__ __forceinline__ void ts_write_moments(const TsArgs &a, int64_t o, TsMoments<T> &m)
{
    if (!a.skipna && m.nans > 0) {                  // NaN enters as it is: it is the extreme, at its first date
        m.mn = m.mx = ts_nan<T>();
        m.amin = m.amax = m.first_nan;
    }
    if (a.count) a.count[o] = m.n;
    if (a.nan_count) a.nan_count[o] = m.nans;
    if (a.sum) a.sum[o] = m.sum;
    if (a.mean) a.mean[o] = m.mean;
    if (a.mn) reinterpret_cast<T *>(a.mn)[o] = m.mn;
    if (a.mx) reinterpret_cast<T *>(a.mx)[o] = m.mx;
    if (a.argmin) a.argmin[o] = m.amin;
    if (a.argmax) a.argmax[o] = m.amax;
    if (a.m2) a.m2[o] = m.m2;
    if (a.var || a.std || a.cv) {
        const int dof = m.n - a.ddof;
        const double var = dof > 0 ? m.m2 / (double)dof : (double)ts_nan<double>();
        const double sd = sqrt(var);
        if (a.var) a.var[o] = var;
        if (a.std) a.std[o] = sd;
        if (a.cv) a.cv[o] = sd / m.mean;
    }
}

// the median and the percentiles of the n sorted values that at(rank) reads; bad: the result is NaN
template <class T, class At> __device__ __forceinline__ void ts_write_order(const TsArgs &a, int64_t o, int n, bool bad, At at)
{
    if (a.median) {
        T r = ts_nan<T>();
        if (!bad) {
            if (n & 1) {
                r = at((n - 1) >> 1);
            } else {
                const T lo = at((n >> 1) - 1), hi = at(n >> 1);
                r = (lo + hi) / T(2);
            }
        }
        reinterpret_cast<T *>(a.median)[o] = r;
    }
    for (int j = 0; j < a.nq; ++j) {
        T r = ts_nan<T>();
        if (!bad) {
            const T q = T(a.q[j]) / T(100);
            const T last = T(n - 1);
            const T vi = last * q;
            int lo, hi;
            if (vi >= last) {
                lo = hi = n - 1;
            } else {
                lo = (int)floor(vi);
                if (lo > n - 1) lo = n - 1;
                if (lo < 0) lo = 0;
                hi = lo + 1 < n ? lo + 1 : n - 1;
            }
            const T g = T((double)vi - (double)lo);
            const T A = at(lo), B = at(hi);
            const T d = B - A;
            r = A + d * g;
            if (g >= T(0.5)) r = B - d * (T(1) - g);
        }
        reinterpret_cast<T *>(a.pct)[(int64_t)j * a.plane + o] = r;
    }
}

// ---- the block's place: its row of lanes, the lane's pixel, whether there is one, and the offsets of its data
struct TsPlace {
    int64_t slow, fast0, in, out;
    int nvalid;
    bool active;
};

__device__ __forceinline__ TsPlace ts_place(const TsArgs &a)
{
    TsPlace p;
    p.slow = (int64_t)blockIdx.x / a.blocks_per_row;
    p.fast0 = ((int64_t)blockIdx.x % a.blocks_per_row) * TS_LANES;
    const int64_t left = a.nfast - p.fast0;
    p.nvalid = (int)(left < TS_LANES ? left : TS_LANES);
    p.active = (int)threadIdx.x < p.nvalid;
    const int64_t fast = p.fast0 + threadIdx.x;
    p.in = p.slow * a.s_slow + fast * a.s_fast;
    p.out = p.slow * a.o_slow + fast * a.o_fast;
    return p;
}

// the wave's run of nvalid * k contiguous elements into the tile, consecutive lanes on consecutive elements
// (the tile holds bit patterns: the LDS form turns them into keys where they lie)
template <class U> __device__ __forceinline__ void ts_stage_run(const TsArgs &a, const TsPlace &p, U *tile)
{
    const U *run = reinterpret_cast<const U *>(a.x) + p.slow * a.s_slow + p.fast0 * a.s_fast;
    const int total = p.nvalid * a.k;
    int pixel = (int)threadIdx.x / a.k, t = (int)threadIdx.x % a.k;
    const int dp = TS_LANES / a.k, dt = TS_LANES % a.k;
    for (int i = threadIdx.x; i < total; i += TS_LANES) {
        tile[ts_at(t, pixel)] = run[i];
        pixel += dp;
        t += dt;
        if (t >= a.k) { t -= a.k; ++pixel; }
    }
}

// ---- the register form
constexpr int ts_log2(int n) { return n <= 1 ? 0 : 1 + ts_log2(n >> 1); }

// the bitonic network on N = 2^L registers; the loops count exponents so that all of them unroll and every index is a
// constant
template <class U, int N> __device__ __forceinline__ void ts_sort_registers(U (&key)[N])
{
    constexpr int L = ts_log2(N);
#pragma unroll
    for (int ls = 1; ls <= L; ++ls) {
#pragma unroll
        for (int lt = ls - 1; lt >= 0; --lt) {
#pragma unroll
            for (int c = 0; c < N / 2; ++c) {
                const int stride = 1 << lt, size = 1 << ls;
                const int i = ((c & ~(stride - 1)) << 1) | (c & (stride - 1)), j = i | stride;
                const bool less = key[i] < key[j];
                const U lo = less ? key[i] : key[j], hi = less ? key[j] : key[i];
                const bool up = (i & size) == 0;
                key[i] = up ? lo : hi;
                key[j] = up ? hi : lo;
            }
        }
    }
}

// key[r] by a tree of selects on the bits of r: written without a loop, because the compiler turns a loop of
// `i == r ? key[i] : v` back into the run-time index it stands for, and the array then leaves the registers
template <class U, int N, int LO, int CNT> __device__ __forceinline__ U ts_pick_tree(const U (&key)[N], int r)
{
    if constexpr (CNT == 1) {
        return key[LO];
    } else {
        const U a = ts_pick_tree<U, N, LO, CNT / 2>(key, r), b = ts_pick_tree<U, N, LO + CNT / 2, CNT / 2>(key, r);
        return (r & (CNT / 2)) ? b : a;
    }
}

template <class U, int N> __device__ __forceinline__ U ts_pick(const U (&key)[N], int r)
{
    return ts_pick_tree<U, N, 0, N>(key, r);
}

template <class T, int KP, bool STAGED>
__global__ __launch_bounds__(TS_LANES) void temporal_register_kernel(TsArgs a)
{
    typedef typename TsKey<T>::U U;
    const TsPlace p = ts_place(a);
    T v[KP];
    if constexpr (STAGED) {
        extern __shared__ __align__(16) unsigned char ts_tile_raw[];
        U *tile = reinterpret_cast<U *>(ts_tile_raw);
        ts_stage_run<U>(a, p, tile);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < KP; ++t) {
            v[t] = ts_nan<T>();
            if (t < a.k && p.active) v[t] = ts_value<T>(tile[ts_at(t, threadIdx.x)]);
        }
    } else {
        const T *x = reinterpret_cast<const T *>(a.x) + p.in;
#pragma unroll
        for (int t = 0; t < KP; ++t) {
            v[t] = ts_nan<T>();
            if (t < a.k && p.active) v[t] = x[(int64_t)t * a.st];
        }
    }
    if (!p.active) return;
    const bool skipna = a.skipna != 0;
    TsMoments<T> m;
    ts_clear(m);
#pragma unroll
    for (int t = 0; t < KP; ++t)
        if (t < a.k) ts_first(m, v[t], t, skipna);
    m.mean = m.sum / (double)m.n;
    if (ts_wants_second(a)) {
#pragma unroll
        for (int t = 0; t < KP; ++t)
            if (t < a.k) ts_second(m, v[t], skipna);
    }
    const int n = a.k - m.nans;
    const bool bad = n == 0 || (!skipna && m.nans > 0);
    ts_write_moments(a, p.out, m);
    if (!ts_wants_order(a)) return;
    U key[KP];
#pragma unroll
    for (int t = 0; t < KP; ++t) key[t] = TsKey<T>::enc(v[t]);
    ts_sort_registers<U, KP>(key);
    ts_write_order<T>(a, p.out, n, bad, [&](int r) { return TsKey<T>::dec(ts_pick<U, KP>(key, r)); });
}

// ---- the LDS form
template <class T, bool STAGED>
__global__ __launch_bounds__(TS_LANES) void temporal_lds_kernel(TsArgs a)
{
    typedef typename TsKey<T>::U U;
    extern __shared__ __align__(16) unsigned char ts_tile_raw[];
    U *tile = reinterpret_cast<U *>(ts_tile_raw);       // bit patterns first, keys later
    const TsPlace p = ts_place(a);
    const int lane = threadIdx.x;
    if constexpr (STAGED) {
        ts_stage_run<U>(a, p, tile);
    } else {
        if (p.active) {
            const U *x = reinterpret_cast<const U *>(a.x) + p.in;
            for (int t = 0; t < a.k; ++t) tile[ts_at(t, lane)] = x[(int64_t)t * a.st];
        }
    }
    __syncthreads();
    if (!p.active) return;
    // from here on a lane touches its own column only
    const bool skipna = a.skipna != 0;
    TsMoments<T> m;
    ts_clear(m);
    for (int t = 0; t < a.k; ++t) ts_first(m, ts_value<T>(tile[ts_at(t, lane)]), t, skipna);
    m.mean = m.sum / (double)m.n;
    if (ts_wants_second(a))
        for (int t = 0; t < a.k; ++t) ts_second(m, ts_value<T>(tile[ts_at(t, lane)]), skipna);
    const int n = a.k - m.nans;
    const bool bad = n == 0 || (!skipna && m.nans > 0);
    ts_write_moments(a, p.out, m);
    if (!ts_wants_order(a)) return;
    U *key = tile;
    for (int t = 0; t < a.k; ++t) key[ts_at(t, lane)] = TsKey<T>::enc(ts_value<T>(tile[ts_at(t, lane)]));
    for (int t = a.k; t < a.kpad; ++t) key[ts_at(t, lane)] = ~(U)0;
    const int half = a.kpad >> 1;
    for (int size = 2; size <= a.kpad; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int c = 0; c < half; ++c) {
                const int i = ((c & ~(stride - 1)) << 1) | (c & (stride - 1)), j = i | stride;
                const U ki = key[ts_at(i, lane)], kj = key[ts_at(j, lane)];
                const bool swap = ((i & size) == 0) == (kj < ki);
                if (swap) {
                    key[ts_at(i, lane)] = kj;
                    key[ts_at(j, lane)] = ki;
                }
            }
        }
    }
    ts_write_order<T>(a, p.out, n, bad, [&](int r) { return TsKey<T>::dec(key[ts_at(r, lane)]); });
}

// ---- the streaming form: the moments of a series of any length
template <class T>
__global__ __launch_bounds__(TS_LANES) void temporal_stream_kernel(TsArgs a)
{
    const TsPlace p = ts_place(a);
    if (!p.active) return;
    const T *x = reinterpret_cast<const T *>(a.x) + p.in;
    const bool skipna = a.skipna != 0;
    TsMoments<T> m;
    ts_clear(m);
    for (int t = 0; t < a.k; ++t) ts_first(m, x[(int64_t)t * a.st], t, skipna);
    m.mean = m.sum / (double)m.n;
    if (ts_wants_second(a))
        for (int t = 0; t < a.k; ++t) ts_second(m, x[(int64_t)t * a.st], skipna);
    ts_write_moments(a, p.out, m);
}

// ---- host
int ts_next_pow2(int k)
{
    int p = 2;
    while (p < k) p <<= 1;
    return p;
}

template <class T>
int ts_launch(const char *fn, TsArgs a, int form, bool staged, bool order, hipStream_t stream, int64_t nblocks)
{
    const dim3 grid((unsigned)nblocks), block(TS_LANES);
    if (form == TS_FORM_REGISTER) {
        const size_t lds = staged ? (size_t)a.k * TS_LANES * sizeof(T) : 0;
        bool ok = false;
        pick(staged, [&](auto S) {
            ok = pick_le<8, 16, 32, 64>(a.k, [&](auto KP) {
                if constexpr (decltype(KP)::value <= TsLimits<T>::reg)
                    hipLaunchKernelGGL((temporal_register_kernel<T, decltype(KP)::value, decltype(S)::value>), grid,
                                       block, lds, stream, a);
            });
        });
        if (!ok) {
            set_error("%s: internal: no register form for k = %d", fn, a.k);
            return ND_AMD_EINTERNAL;
        }
    } else if (form == TS_FORM_LDS) {
        a.kpad = order ? ts_next_pow2(a.k) : a.k;           // the network wants a power of two; the moments want k rows
        const size_t lds = (size_t)a.kpad * TS_LANES * sizeof(T);
        pick(staged, [&](auto S) {
            hipLaunchKernelGGL((temporal_lds_kernel<T, decltype(S)::value>), grid, block, lds, stream, a);
        });
    } else {
        hipLaunchKernelGGL((temporal_stream_kernel<T>), grid, block, 0, stream, a);
    }
    return ND_AMD_OK;
}

// what both entries do; `form`: TS_FORM_AUTO, or the one form a test asks for
int ts_entry(const char *fn, const void *x, int dtype, int64_t k, int64_t ny, int64_t nx, const int64_t *strides,
             int skipna, int ddof, const double *percentiles, int npercentiles, int32_t *count, int32_t *nan_count,
             double *sum, double *mean, void *min, void *max, int32_t *argmin, int32_t *argmax, double *m2, double *var,
             double *std, double *cv, void *median, void *percentile_out, int form, void *hip_stream)
{
    bool empty = false;
    int rc = check_dtype(fn, dtype);
    if (rc == ND_AMD_OK) rc = check_shape(fn, ny, nx, 1, &empty);
    if (rc != ND_AMD_OK) return rc;
    if (k < 1 || k > 0x7fffffffLL) {
        set_error("%s: the series needs 1 to 2^31 - 1 dates, got %lld", fn, (long long)k);
        return ND_AMD_EINVAL;
    }
    rc = check_strides(fn, "strides", strides);
    if (rc == ND_AMD_OK) rc = check_plane_pixels(fn, ny, nx);
    if (rc != ND_AMD_OK) return rc;
    if (ddof < 0) {
        set_error("%s: ddof must not be negative, got %d", fn, ddof);
        return ND_AMD_EINVAL;
    }
    if (npercentiles < 0 || (npercentiles > 0 && (!percentiles || !percentile_out))) {
        set_error("%s: %d percentiles need their list and their output", fn, npercentiles);
        return ND_AMD_EINVAL;
    }
    for (int j = 0; j < npercentiles; ++j)
        if (!(percentiles[j] >= 0.0 && percentiles[j] <= 100.0)) {
            set_error("%s: percentile %d is %g: outside [0, 100]", fn, j, percentiles[j]);
            return ND_AMD_EINVAL;
        }
    if (form < TS_FORM_AUTO || form > TS_FORM_STREAM) {
        set_error("%s: unknown form %d", fn, form);
        return ND_AMD_EINVAL;
    }
    const bool order = median || npercentiles > 0;
    const int reg_max = dtype == ND_AMD_F64 ? ND_AMD_TEMPORAL_REG_MAX_F64 : ND_AMD_TEMPORAL_REG_MAX_F32;
    const int lds_max = dtype == ND_AMD_F64 ? ND_AMD_TEMPORAL_LDS_MAX_F64 : ND_AMD_TEMPORAL_LDS_MAX_F32;
    const bool choose = form == TS_FORM_AUTO;
    if (choose)
        form = k <= reg_max ? TS_FORM_REGISTER : (order ? TS_FORM_LDS : TS_FORM_STREAM);
    if ((form == TS_FORM_REGISTER && k > reg_max) || (form == TS_FORM_LDS && k > lds_max)
        || (form == TS_FORM_STREAM && order)) {
        set_error("%s: %s of %lld dates are not served%s (register form: %d, LDS form: %d dates)", fn,
                  order ? "order statistics" : "series", (long long)k,
                  form == TS_FORM_STREAM ? " by the streaming form" : "", reg_max, lds_max);
        return ND_AMD_EUNSUPPORTED;
    }
    if (empty) return ND_AMD_OK;
    if (!x) {
        set_error("%s: null data pointer", fn);
        return ND_AMD_EINVAL;
    }
    if (!count && !nan_count && !sum && !mean && !min && !max && !argmin && !argmax && !m2 && !var && !std && !cv
        && !order)
        return ND_AMD_OK;

    TsArgs a;
    memset(&a, 0, sizeof a);
    a.x = x;
    a.st = strides[0];
    // lanes along the kept dim with the smaller stride; a dim of one element has none to speak of
    const bool along_x = ny == 1 || (nx != 1 && strides[2] <= strides[1]);
    int64_t nslow;
    if (along_x) {
        a.s_slow = strides[1]; a.s_fast = strides[2]; a.o_slow = nx; a.o_fast = 1; a.nfast = nx; nslow = ny;
    } else {
        a.s_slow = strides[2]; a.s_fast = strides[1]; a.o_slow = 1; a.o_fast = nx; a.nfast = ny; nslow = nx;
    }
    if (along_x && a.s_slow == a.nfast * a.s_fast) {        // rows back to back: one row, no block cut at a row's end
        a.nfast *= nslow;
        nslow = 1;
    }
    a.blocks_per_row = ceil_div(a.nfast, TS_LANES);
    const int64_t nblocks = a.blocks_per_row * nslow;
    if (nblocks > TS_MAX_BLOCKS) {
        set_error("%s: %lld blocks are more than one launch holds", fn, (long long)nblocks);
        return ND_AMD_EUNSUPPORTED;
    }
    a.plane = ny * nx;
    a.k = (int)k;
    a.skipna = skipna != 0;
    a.ddof = ddof;
    a.count = count; a.nan_count = nan_count; a.argmin = argmin; a.argmax = argmax;
    a.sum = sum; a.mean = mean; a.m2 = m2; a.var = var; a.std = std; a.cv = cv;
    a.mn = min; a.mx = max; a.median = median;
    // the staged reading: a pixel's series is contiguous and the lanes' pixels follow one another
    const bool contiguous = k > 1 && a.st == 1 && a.s_fast == k;
    // the moments of a long contiguous series that fits the tile go through it: the streaming form would read
    // (y, x, time) memory with every lane on a cache line of its own
    if (choose && form == TS_FORM_STREAM && contiguous && k <= lds_max) form = TS_FORM_LDS;
    const bool staged = form != TS_FORM_STREAM && contiguous;
    const size_t esize = dtype == ND_AMD_F64 ? sizeof(double) : sizeof(float);

    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    KernelTimer timer(ND_AMD_KERNEL_TEMPORAL, stream);
    // TS_MAXQ percentiles per launch; everything else comes from the first
    for (int q0 = 0; q0 == 0 || q0 < npercentiles; q0 += TS_MAXQ) {
        a.nq = npercentiles - q0 < TS_MAXQ ? npercentiles - q0 : TS_MAXQ;
        for (int j = 0; j < a.nq; ++j) a.q[j] = percentiles[q0 + j];
        a.pct = a.nq > 0 ? reinterpret_cast<unsigned char *>(percentile_out) + (size_t)q0 * (size_t)a.plane * esize : nullptr;
        if (q0 > 0) {
            a.count = a.nan_count = a.argmin = a.argmax = nullptr;
            a.sum = a.mean = a.m2 = a.var = a.std = a.cv = nullptr;
            a.mn = a.mx = a.median = nullptr;
        }
        rc = dtype == ND_AMD_F64 ? ts_launch<double>(fn, a, form, staged, order, stream, nblocks)
                                 : ts_launch<float>(fn, a, form, staged, order, stream, nblocks);
        if (rc != ND_AMD_OK) return rc;
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

}  // namespace

extern "C" int nd_amd_temporal_stats(const void *x, int dtype, int64_t k, int64_t ny, int64_t nx, const int64_t *strides,
                                     int skipna, int ddof, const double *percentiles, int npercentiles,
                                     int32_t *count, int32_t *nan_count, double *sum, double *mean, void *min, void *max,
                                     int32_t *argmin, int32_t *argmax, double *m2, double *var, double *std, double *cv,
                                     void *median, void *percentile_out, void *hip_stream)
{
    return ts_entry("nd_amd_temporal_stats", x, dtype, k, ny, nx, strides, skipna, ddof, percentiles, npercentiles, count,
                    nan_count, sum, mean, min, max, argmin, argmax, m2, var, std, cv, median, percentile_out,
                    TS_FORM_AUTO, hip_stream);
}

// For the tests that hold the forms to the same bits, and for nothing else: the same call with one form named (1
// register, 2 LDS, 3 streaming; ND_AMD_EUNSUPPORTED where that form does not serve the request).  It is in no header
// and no part of the C ABI; nd_amd.kernels.temporal_stats reaches it through its private `_form` argument.
extern "C" int nd_amd_temporal_stats_in_form(const void *x, int dtype, int64_t k, int64_t ny, int64_t nx,
                                             const int64_t *strides, int skipna, int ddof, const double *percentiles,
                                             int npercentiles, int32_t *count, int32_t *nan_count, double *sum,
                                             double *mean, void *min, void *max, int32_t *argmin, int32_t *argmax,
                                             double *m2, double *var, double *std, double *cv, void *median,
                                             void *percentile_out, int form, void *hip_stream)
{
    return ts_entry("nd_amd_temporal_stats_in_form", x, dtype, k, ny, nx, strides, skipna, ddof, percentiles,
                    npercentiles, count, nan_count, sum, mean, min, max, argmin, argmax, m2, var, std, cv, median,
                    percentile_out, form, hip_stream);
}
