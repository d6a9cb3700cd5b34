// nd_amd/csrc/rgb.hip -- percentile-stretched RGB composites (nd.visualize.to_rgb, nd/visualize.py:176-193)
//
//   nd_amd_rgb_limits   np.nanpercentile(channel, pmin), np.nanpercentile(channel, pmax) of every channel
//                       plane of a batch, as numpy 2.2.6 computes them in the data type (include/nd_amd.h).
//   nd_amd_rgb_compose  (channel - minval) / (maxval - minval) * 255 -> clip -> uint8, three bytes a pixel.
//
// The percentile is an exact order-statistic selection, not a sort.  A value maps to an unsigned key that
// orders like the value (sign bit flipped for positive values, all bits for negative ones); NaNs are
// dropped.  Pass 0 histograms the leading 11 bits of every key of every plane; rgb_select_kernel turns the
// plane's count n into the (at most four) wanted ranks -- lo and hi of both percentiles -- and picks the
// bucket of each; every later pass histograms the next digit of the keys that carry one of the chosen
// prefixes (ranks that share a prefix share a histogram).  float32: 11 + 11 + 10 bits, three reads of the
// planes; float64: 11 + 11 + 11 + 11 + 10 + 10, six.  The last select call has the full keys and forms
// the interpolation on the device, so nothing returns to the host between the passes.
//
// Atomic contention (SAR intensities are close to exponentially distributed: most keys of a plane fall
// into a dozen leading-digit bins; a constant plane is the extreme):
//   * a lane carries (bin, count) across its loop and only issues an LDS atomic when the bin changes, so
//     a constant run costs one atomic per lane, not one per element;
//   * the block's LDS histogram is kept in COPIES interleaved copies, copy = lane % COPIES: lanes of a
//     wave that hit the same bin land in different banks instead of serialising on one address;
//   * a block adds only its non-zero bins to the plane's global histogram (one atomic per bin and block).
#include "common.hpp"
#include "dispatch.hpp"

using namespace nd_amd;

namespace {

constexpr int RGB_BINS = 2048;          // bins of one histogram (11 bits; the 10-bit passes use half)
constexpr int RGB_SLOTS = 4;            // histograms per plane and pass: one per distinct prefix
constexpr int RGB_HIST_THREADS = 512;
constexpr int RGB_LDS_WORDS = 16384;    // 64 KiB: 1 x 2048 x 8 copies (pass 0), 4 x 2048 x 2 copies (later)
constexpr int RGB_MAX_PASSES = 6;

struct RgbPlanes {
    const void *num[3];
    const void *den[3];                 // null: the channel is num itself, else num / den
    int nchan;
    int64_t nframes, ny, nx;
    int64_t st, sy, sx;                 // element strides of frame, row, column (shared by all planes)
    int vec;                            // planes are contiguous and 16-byte aligned: 4-element loads
};

struct RgbStretch {
    double vmin[3], vmax[3];
    int given;                          // bit 2c: vmin[c] given, bit 2c + 1: vmax[c] given
};

struct RgbSelState {
    long long n;                        // non-NaN values of the plane
    long long rank[4];                  // wanted rank, relative to the start of its prefix
    unsigned long long prefix[4];       // key digits fixed so far, per rank
    unsigned long long uprefix[4];      // the distinct prefixes; slot[r] indexes them
    int slot[4];
    int nslot;                          // 0: empty plane, nothing to select
    double g[2];                        // interpolation weight of pmin / pmax (a value of T)
};

template <typename T> struct RgbKey;
template <> struct RgbKey<float> {
    typedef uint32_t U;
    static __device__ __forceinline__ U enc(float v)
    {
        const U u = __float_as_uint(v);
        return (u >> 31) ? ~u : (u | 0x80000000u);
    }
    static __device__ __forceinline__ float dec(unsigned long long k64)
    {
        const U k = (U)k64;
        return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
    }
};
template <> struct RgbKey<double> {
    typedef uint64_t U;
    static __device__ __forceinline__ U enc(double v)
    {
        const U u = (U)__double_as_longlong(v);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double dec(unsigned long long k)
    {
        return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
    }
};

__device__ __forceinline__ void load4(const float *p, float v[4])
{
    const float4 q = *reinterpret_cast<const float4 *>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void load4(const double *p, double v[4])
{
    const double2 a = *reinterpret_cast<const double2 *>(p);
    const double2 b = *reinterpret_cast<const double2 *>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}

// kernel arguments are selected, not indexed: a run-time index into a by-value struct would be served from a
// scratch copy of it
__device__ __forceinline__ const void *rgb_pick(const void *const p[3], int c)
{
    return c == 0 ? p[0] : (c == 1 ? p[1] : p[2]);
}

// values of the elements i .. i + 3 of one channel plane (flat index y * nx + x); only the first `m` exist
template <typename T>
__device__ __forceinline__ void load_channel4(const RgbPlanes &a, const T *num, const T *den, int64_t i, int m,
                                              T v[4])
{
    if (a.vec && m == 4) {
        load4(num + i, v);
        if (den) {
            T d[4];
            load4(den + i, d);
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = v[j] / d[j];
        }
        return;
    }
    int64_t y = i / a.nx, x = i - y * a.nx;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = T(0);
        if (j < m) {
            const int64_t off = y * a.sy + x * a.sx;
            v[j] = num[off];
            if (den) v[j] = v[j] / den[off];
            if (++x == a.nx) { x = 0; y++; }
        }
    }
}

// ---- digit histogram of one pass -----------------------------------------------------------------------
// grid (plane, chunk): the planes of one frame run side by side, so the quotient channel finds C11 and C22
// in the cache behind the two plain channels.
template <typename T, bool FIRST>
__global__ __launch_bounds__(RGB_HIST_THREADS) void rgb_hist_kernel(RgbPlanes a, const RgbSelState *state,
                                                                    uint32_t *hist, int shift, int bits,
                                                                    int64_t chunk)
{
    typedef typename RgbKey<T>::U U;
    constexpr int COPIES = FIRST ? 8 : 2;
    __shared__ uint32_t lds[RGB_LDS_WORDS];
    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    int nslot = 1;
    U up0 = 0, up1 = 0, up2 = 0, up3 = 0;
    if (!FIRST) {
        const RgbSelState &s = state[p];
        nslot = s.nslot;
        if (nslot == 0) return;
        up0 = (U)s.uprefix[0]; up1 = (U)s.uprefix[1]; up2 = (U)s.uprefix[2]; up3 = (U)s.uprefix[3];
    }
    for (int e = tid; e < RGB_LDS_WORDS; e += RGB_HIST_THREADS) lds[e] = 0;
    __syncthreads();

    const int frame = p / a.nchan, c = p - frame * a.nchan;
    const void *dp = rgb_pick(a.den, c);
    const T *num = reinterpret_cast<const T *>(rgb_pick(a.num, c)) + frame * a.st;
    const T *den = dp ? reinterpret_cast<const T *>(dp) + frame * a.st : nullptr;
    const int64_t n = a.ny * a.nx;
    const int64_t i0 = (int64_t)blockIdx.y * chunk;
    const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    const U dmask = (U(1) << bits) - 1;
    const int copy = tid & (COPIES - 1);

    int cur = -1;
    uint32_t cnt = 0;
    // one element: its bin (or none), merged into the lane's running (bin, count)
    auto count = [&](T v) {
        if (!(v == v)) return;
        const U key = RgbKey<T>::enc(v);
        int idx = -1;
        if (FIRST) {
            idx = (int)(key >> shift) * COPIES + copy;
        } else {
            const U pre = (key >> shift) >> bits;
            const int d = (int)((key >> shift) & dmask);
            int s = -1;
            if (pre == up0) s = 0;
            else if (nslot > 1 && pre == up1) s = 1;
            else if (nslot > 2 && pre == up2) s = 2;
            else if (nslot > 3 && pre == up3) s = 3;
            if (s >= 0) idx = (s * RGB_BINS + d) * COPIES + copy;
        }
        if (idx < 0) return;
        if (idx == cur) {
            cnt++;
        } else {
            if (cnt) atomicAdd(&lds[cur], cnt);
            cur = idx;
            cnt = 1;
        }
    };
    // (two groups a step with both loads issued before counting was measured too: no gain, 2.18 against 2.15 ms
    //  for pass 1 of the 24 x 4096 x 4096 float32 stack)
    for (int64_t i = i0 + (int64_t)tid * 4; i < i1; i += RGB_HIST_THREADS * 4) {
        const int m = i1 - i < 4 ? (int)(i1 - i) : 4;
        T v[4];
        load_channel4<T>(a, num, den, i, m, v);
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (j < m) count(v[j]);
    }
    if (cnt) atomicAdd(&lds[cur], cnt);
    __syncthreads();

    uint32_t *h = hist + (int64_t)p * (RGB_SLOTS * RGB_BINS);
    const int nbin = (FIRST ? 1 : nslot) * RGB_BINS;
    for (int e = tid; e < nbin; e += RGB_HIST_THREADS) {
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < COPIES; k++) sum += lds[e * COPIES + k];
        if (sum) atomicAdd(&h[e], sum);
    }
}

// ---- rank bookkeeping between the passes -----------------------------------------------------------------
// One block per plane.  Pass 0 first turns the plane's count into ranks; every pass then finds, per rank, the
// bin its rank falls into and makes the rank relative to that bin; the last pass forms the limits.
template <typename T>
__global__ __launch_bounds__(256) void rgb_select_kernel(RgbSelState *state, const uint32_t *hist, int pass,
                                                         int npass, int bits, double pmin, double pmax,
                                                         T *limits, long long *counts)
{
    __shared__ unsigned long long part[256];
    __shared__ RgbSelState s;
    __shared__ int sel_bin[4];
    __shared__ long long sel_rank[4];
    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t *h = hist + (int64_t)p * (RGB_SLOTS * RGB_BINS);
    constexpr int PER = RGB_BINS / 256;

    if (tid == 0) s = state[p];
    __syncthreads();

    if (pass == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < PER; k++) t += h[tid * PER + k];
        part[tid] = t;
        __syncthreads();
        if (tid == 0) {
            unsigned long long n = 0;
            for (int k = 0; k < 256; k++) n += part[k];
            s.n = (long long)n;
            s.nslot = n ? 1 : 0;
            const double pq[2] = {pmin, pmax};
            for (int j = 0; j < 2; j++) {
                long long lo = 0, hi = 0;
                T g = T(0);
                if (n) {
                    const T q = T(pq[j]) / T(100);
                    const T last = T((long long)n - 1);
                    const T vi = last * q;
                    if (vi >= last) {                       // numpy: index -1 for both neighbours
                        lo = hi = (long long)n - 1;
                    } else {
                        lo = (long long)floor(vi);
                        if (lo > (long long)n - 1) lo = (long long)n - 1;
                        hi = lo + 1 < (long long)n ? lo + 1 : (long long)n - 1;
                    }
                    g = T((double)vi - (double)lo);         // numpy subtracts the integer index in double
                }
                s.rank[2 * j] = lo;
                s.rank[2 * j + 1] = hi;
                s.g[j] = (double)g;
            }
            for (int r = 0; r < 4; r++) {
                s.prefix[r] = 0;
                s.uprefix[r] = 0;
                s.slot[r] = 0;
            }
        }
        __syncthreads();
    }

    if (s.nslot > 0) {
        for (int r = 0; r < 4; r++) {
            const uint32_t *hs = h + s.slot[r] * RGB_BINS;
            uint32_t c[PER];
            unsigned long long t = 0;
#pragma unroll
            for (int k = 0; k < PER; k++) {
                c[k] = hs[tid * PER + k];
                t += c[k];
            }
            part[tid] = t;
            __syncthreads();
            unsigned long long before = 0;
            for (int k = 0; k < tid; k++) before += part[k];
            const unsigned long long want = (unsigned long long)s.rank[r];
            if (want >= before && want < before + t) {
                bool done = false;
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    if (!done && want < before + c[k]) {
                        sel_bin[r] = tid * PER + k;
                        sel_rank[r] = (long long)(want - before);
                        done = true;
                    }
                    if (!done) before += c[k];
                }
            }
            __syncthreads();
        }
    }

    if (tid == 0) {
        if (s.nslot > 0) {
            int nslot = 0;
            for (int r = 0; r < 4; r++) {
                s.prefix[r] = (s.prefix[r] << bits) | (unsigned long long)sel_bin[r];
                s.rank[r] = sel_rank[r];
                int found = -1;
                for (int q = 0; q < r; q++)
                    if (s.prefix[q] == s.prefix[r]) { found = s.slot[q]; break; }
                if (found < 0) {
                    found = nslot++;
                    s.uprefix[found] = s.prefix[r];
                }
                s.slot[r] = found;
            }
            s.nslot = nslot;
        }
        state[p] = s;
        if (pass == npass - 1) {
            for (int j = 0; j < 2; j++) {
                T res = T(NAN);
                if (s.nslot > 0) {
                    const T A = RgbKey<T>::dec(s.prefix[2 * j]);
                    const T B = RgbKey<T>::dec(s.prefix[2 * j + 1]);
                    const T g = T(s.g[j]);
                    const T d = B - A;
                    res = A + d * g;
                    if (g >= T(0.5)) res = B - d * (T(1) - g);
                }
                limits[2 * (int64_t)p + j] = res;
            }
            counts[p] = s.n;
        }
    }
}

// ---- composite ---------------------------------------------------------------------------------------------
template <typename T> struct RgbScale {
    T mn, span;
    bool on;
};

template <typename T>
__device__ __forceinline__ RgbScale<T> rgb_scale(const T *limits, const RgbStretch &st, int64_t plane, int c)
{
    RgbScale<T> r;
    const bool gmin = (st.given >> (2 * c)) & 1, gmax = (st.given >> (2 * c + 1)) & 1;
    if (gmin && gmax) {                   // two Python numbers: compared and subtracted in double
        r.on = st.vmax[c] > st.vmin[c];
        r.mn = T(st.vmin[c]);
        r.span = T(st.vmax[c] - st.vmin[c]);
    } else {
        const T lo = gmin ? T(st.vmin[c]) : limits[2 * plane];
        const T hi = gmax ? T(st.vmax[c]) : limits[2 * plane + 1];
        r.on = hi > lo;
        r.mn = lo;
        r.span = hi - lo;
    }
    return r;
}

template <typename T> __device__ __forceinline__ uint32_t rgb_byte(T v, const RgbScale<T> &s)
{
    if (s.on) v = (v - s.mn) / s.span * T(255);
    double d = (double)v;
    if (!(d == d)) return 0;
    d = d < 0.0 ? 0.0 : (d > 255.0 ? 255.0 : d);
    return (uint32_t)d;
}

// One lane: four consecutive pixels, twelve bytes, three dwords.  `framewise` (ny * nx a multiple of 4):
// grid (groups of a frame, frame), every group lies in one frame.  Otherwise the batch is one flat run of
// pixels, a group may straddle two frames and the last one may be short (byte stores).
template <typename T>
__global__ __launch_bounds__(256) void rgb_compose_kernel(RgbPlanes a, const T *limits, RgbStretch st,
                                                          const uint8_t *mask, uint8_t *out, int framewise)
{
    const int64_t n = a.ny * a.nx;
    const int64_t grp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t b[4][3];
    int valid = 4;
    int64_t g0;                                    // first pixel of the group in the flat batch
    if (framewise) {
        const int64_t i = grp * 4;
        if (i >= n) return;
        const int64_t f = blockIdx.y;
        g0 = f * n + i;
        bool keep[4] = {true, true, true, true};
        if (mask) {
            if (((uintptr_t)mask & 3) == 0) {
                const uint32_t w = *reinterpret_cast<const uint32_t *>(mask + i);
#pragma unroll
                for (int j = 0; j < 4; j++) keep[j] = ((w >> (8 * j)) & 0xffu) != 0;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) keep[j] = mask[i + j] != 0;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (c < a.nchan) {
                const RgbScale<T> s = rgb_scale<T>(limits, st, f * a.nchan + c, c);
                const T *num = reinterpret_cast<const T *>(a.num[c]) + f * a.st;
                const T *den = a.den[c] ? reinterpret_cast<const T *>(a.den[c]) + f * a.st : nullptr;
                T v[4];
                load_channel4<T>(a, num, den, i, 4, v);
#pragma unroll
                for (int j = 0; j < 4; j++) b[j][c] = keep[j] ? rgb_byte<T>(v[j], s) : 0u;
            }
        }
    } else {
        const int64_t total = a.nframes * n;
        g0 = grp * 4;
        if (g0 >= total) return;
        if (total - g0 < 4) valid = (int)(total - g0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            b[j][0] = b[j][1] = b[j][2] = 0;
            if (j < valid) {
                const int64_t f = (g0 + j) / n, i = (g0 + j) - f * n;
                const bool keep = mask ? mask[i] != 0 : true;
                const int64_t y = i / a.nx, x = i - y * a.nx;
                const int64_t off = f * a.st + y * a.sy + x * a.sx;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    if (c < a.nchan) {
                        const RgbScale<T> s = rgb_scale<T>(limits, st, f * a.nchan + c, c);
                        T v = reinterpret_cast<const T *>(a.num[c])[off];
                        if (a.den[c]) v = v / reinterpret_cast<const T *>(a.den[c])[off];
                        b[j][c] = keep ? rgb_byte<T>(v, s) : 0u;
                    }
                }
            }
        }
    }
    if (a.nchan == 1) {
#pragma unroll
        for (int j = 0; j < 4; j++) b[j][1] = b[j][2] = b[j][0];
    }
    if (valid == 4) {
        uint32_t *o = reinterpret_cast<uint32_t *>(out) + (g0 >> 2) * 3;
        o[0] = b[0][0] | (b[0][1] << 8) | (b[0][2] << 16) | (b[1][0] << 24);
        o[1] = b[1][1] | (b[1][2] << 8) | (b[2][0] << 16) | (b[2][1] << 24);
        o[2] = b[2][2] | (b[3][0] << 8) | (b[3][1] << 16) | (b[3][2] << 24);
    } else {
        for (int j = 0; j < valid; j++)
            for (int c = 0; c < 3; c++) out[(g0 + j) * 3 + c] = (uint8_t)b[j][c];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------
struct RgbPasses {
    int n;
    int shift[RGB_MAX_PASSES], bits[RGB_MAX_PASSES];
};

RgbPasses rgb_passes(int dtype)
{
    RgbPasses ps;
    if (dtype == ND_AMD_F32) {
        ps.n = 3;
        const int b[3] = {11, 11, 10};
        for (int i = 0, top = 32; i < 3; i++) { top -= b[i]; ps.shift[i] = top; ps.bits[i] = b[i]; }
    } else {
        ps.n = 6;
        const int b[6] = {11, 11, 11, 11, 10, 10};
        for (int i = 0, top = 64; i < 6; i++) { top -= b[i]; ps.shift[i] = top; ps.bits[i] = b[i]; }
    }
    return ps;
}

size_t rgb_align(size_t v) { return (v + 255) & ~(size_t)255; }

size_t rgb_state_bytes(int64_t planes) { return rgb_align((size_t)planes * sizeof(RgbSelState)); }

size_t rgb_hist_bytes(int64_t planes) { return (size_t)planes * RGB_SLOTS * RGB_BINS * sizeof(uint32_t); }

const int64_t RGB_MAX_PLANE = (int64_t)1 << 31;        // 32-bit bin counts
const int64_t RGB_MAX_PLANES = 65535;

// common argument checks of the two calls; fills `a`.  No HIP call is made here.
int rgb_check_planes(const char *fn, const void *const *num, const void *const *den, int nchan, int dtype,
                     int64_t nframes, int64_t ny, int64_t nx, int64_t st, int64_t sy, int64_t sx, RgbPlanes &a)
{
    if (dtype != ND_AMD_F32 && dtype != ND_AMD_F64) {
        set_error("%s: dtype must be ND_AMD_F32 or ND_AMD_F64, got %d", fn, dtype);
        return ND_AMD_EINVAL;
    }
    if (nchan != 1 && nchan != 3) {
        set_error("%s: a frame has 1 or 3 channels, got %d", fn, nchan);
        return ND_AMD_EINVAL;
    }
    if (nframes < 0 || ny < 0 || nx < 0 || (ny > 0 && nx > RGB_MAX_PLANE / ny) || nframes * nchan > RGB_MAX_PLANES) {
        set_error("%s: bad or unsupported shape nframes=%lld ny=%lld nx=%lld", fn, (long long)nframes,
                  (long long)ny, (long long)nx);
        return ND_AMD_EINVAL;
    }
    if (st < 0 || sy < 0 || sx < 0) {
        set_error("%s: negative stride (%lld, %lld, %lld)", fn, (long long)st, (long long)sy, (long long)sx);
        return ND_AMD_EINVAL;
    }
    const bool empty = nframes == 0 || ny == 0 || nx == 0;
    const size_t esz = dtype == ND_AMD_F32 ? 4 : 8;
    if (!empty && !num) {
        set_error("%s: null pointer", fn);
        return ND_AMD_EINVAL;
    }
    a.nchan = nchan;
    a.nframes = nframes; a.ny = ny; a.nx = nx;
    a.st = st; a.sy = sy; a.sx = sx;
    a.vec = (sx == 1 && sy == nx && (st * esz) % 16 == 0) ? 1 : 0;
    for (int c = 0; c < 3; c++) {
        a.num[c] = c < nchan && num ? num[c] : nullptr;
        a.den[c] = c < nchan && den ? den[c] : nullptr;
        if (c >= nchan) continue;
        if (!empty && !a.num[c]) {
            set_error("%s: null plane pointer (channel %d)", fn, c);
            return ND_AMD_EINVAL;
        }
        if (((uintptr_t)a.num[c] % esz) || ((uintptr_t)a.den[c] % esz)) {
            set_error("%s: channel %d is not aligned to its element size", fn, c);
            return ND_AMD_EINVAL;
        }
        if (((uintptr_t)a.num[c] % 16) || ((uintptr_t)a.den[c] % 16)) a.vec = 0;
    }
    return ND_AMD_OK;
}

template <typename T>
int rgb_limits_launch(const RgbPlanes &a, double pmin, double pmax, T *limits, long long *counts, void *workspace,
                      size_t used_bytes, hipStream_t stream)
{
    const int dtype = sizeof(T) == 4 ? ND_AMD_F32 : ND_AMD_F64;
    const RgbPasses ps = rgb_passes(dtype);
    const int64_t planes = a.nframes * a.nchan;
    const int64_t n = a.ny * a.nx;
    RgbSelState *state = reinterpret_cast<RgbSelState *>(workspace);
    uint32_t *hist0 = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(workspace) + rgb_state_bytes(planes));
    const size_t hist_words = (size_t)planes * RGB_SLOTS * RGB_BINS;

    KernelTimer timer(ND_AMD_KERNEL_RGB_LIMITS, stream);
    ND_HIP_CHECK(hipMemsetAsync(workspace, 0, used_bytes, stream));
    // about 4096 blocks over the batch, none smaller than 16 Ki elements; chunks are multiples of the 2048
    // elements one block iteration covers, so every 4-element group of a chunk but the plane's last is whole
    int64_t per_plane = ceil_div(4096, planes);
    const int64_t most = ceil_div(n, 16384);
    if (per_plane > most) per_plane = most;
    if (per_plane < 1) per_plane = 1;
    const int64_t chunk = ceil_div(ceil_div(n, per_plane), RGB_HIST_THREADS * 4) * (RGB_HIST_THREADS * 4);
    const dim3 grid((unsigned)planes, (unsigned)(n ? ceil_div(n, chunk) : 1));
    for (int d = 0; d < ps.n; d++) {
        uint32_t *hist = hist0 + (size_t)d * hist_words;
        if (n > 0)
            pick(d == 0, [&](auto FIRST) {
                hipLaunchKernelGGL((rgb_hist_kernel<T, decltype(FIRST)::value>), grid, dim3(RGB_HIST_THREADS), 0,
                                   stream, a, state, hist, ps.shift[d], ps.bits[d], chunk);
            });
        hipLaunchKernelGGL((rgb_select_kernel<T>), dim3((unsigned)planes), dim3(256), 0, stream, state, hist, d,
                           ps.n, ps.bits[d], pmin, pmax, limits, counts);
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

template <typename T>
int rgb_compose_launch(const RgbPlanes &a, const T *limits, const RgbStretch &st, const uint8_t *mask, uint8_t *out,
                       hipStream_t stream)
{
    const int64_t n = a.ny * a.nx;
    const int framewise = (n % 4 == 0) ? 1 : 0;
    dim3 grid;
    if (framewise)
        grid = dim3((unsigned)ceil_div(n / 4, 256), (unsigned)a.nframes);
    else {
        const int64_t blocks = ceil_div(ceil_div(a.nframes * n, 4), 256);
        if (blocks > 0x7fffffff) {
            set_error("nd_amd_rgb_compose: %lld frames of %lld pixels (not a multiple of 4) exceed one launch",
                      (long long)a.nframes, (long long)n);
            return ND_AMD_EINVAL;
        }
        grid = dim3((unsigned)blocks);
    }
    KernelTimer timer(ND_AMD_KERNEL_RGB_COMPOSE, stream);
    hipLaunchKernelGGL((rgb_compose_kernel<T>), grid, dim3(256), 0, stream, a, limits, st, mask, out, framewise);
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

}  // namespace

extern "C" size_t nd_amd_rgb_limits_workspace_bytes(int dtype, int64_t nplanes)
{
    if ((dtype != ND_AMD_F32 && dtype != ND_AMD_F64) || nplanes <= 0 || nplanes > RGB_MAX_PLANES) return 0;
    return rgb_state_bytes(nplanes) + (size_t)rgb_passes(dtype).n * rgb_hist_bytes(nplanes);
}

extern "C" int nd_amd_rgb_limits(const void *const *num, const void *const *den, int nchan, int dtype,
                                 int64_t nframes, int64_t ny, int64_t nx, int64_t stride_frame, int64_t stride_y,
                                 int64_t stride_x, double pmin, double pmax, void *limits, int64_t *counts,
                                 void *workspace, size_t workspace_bytes, void *hip_stream)
{
    RgbPlanes a;
    const int rc = rgb_check_planes("nd_amd_rgb_limits", num, den, nchan, dtype, nframes, ny, nx, stride_frame,
                                    stride_y, stride_x, a);
    if (rc != ND_AMD_OK) return rc;
    if (!(pmin >= 0.0 && pmin <= 100.0) || !(pmax >= 0.0 && pmax <= 100.0)) {
        set_error("nd_amd_rgb_limits: percentiles must be in the range [0, 100], got pmin=%g pmax=%g", pmin, pmax);
        return ND_AMD_EINVAL;
    }
    if (nframes == 0) return ND_AMD_OK;
    if (!limits || !counts) {
        set_error("nd_amd_rgb_limits: null pointer");
        return ND_AMD_EINVAL;
    }
    const size_t need = nd_amd_rgb_limits_workspace_bytes(dtype, nframes * nchan);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 255)) {
        set_error("nd_amd_rgb_limits: workspace missing, too small or not 256-byte aligned");
        return ND_AMD_EWORKSPACE;
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    int rcl = ND_AMD_EINVAL;
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        rcl = rgb_limits_launch<T>(a, pmin, pmax, reinterpret_cast<T *>(limits),
                                   reinterpret_cast<long long *>(counts), workspace, need, stream);
    });
    return rcl;
}

extern "C" int nd_amd_rgb_compose(const void *const *num, const void *const *den, int nchan, int dtype,
                                  int64_t nframes, int64_t ny, int64_t nx, int64_t stride_frame, int64_t stride_y,
                                  int64_t stride_x, const void *limits, const double *vmin, const double *vmax,
                                  const uint8_t *mask, uint8_t *out, void *hip_stream)
{
    RgbPlanes a;
    const int rc = rgb_check_planes("nd_amd_rgb_compose", num, den, nchan, dtype, nframes, ny, nx, stride_frame,
                                    stride_y, stride_x, a);
    if (rc != ND_AMD_OK) return rc;
    if (!limits && (!vmin || !vmax)) {
        set_error("nd_amd_rgb_compose: limits is null, so both vmin and vmax must be given");
        return ND_AMD_EINVAL;
    }
    if (nframes == 0 || ny == 0 || nx == 0) return ND_AMD_OK;
    if (!out || ((uintptr_t)out & 3)) {
        set_error("nd_amd_rgb_compose: out is null or not 4-byte aligned");
        return ND_AMD_EINVAL;
    }
    RgbStretch st;
    st.given = 0;
    for (int c = 0; c < 3; c++) {
        st.vmin[c] = vmin && c < nchan ? vmin[c] : 0.0;
        st.vmax[c] = vmax && c < nchan ? vmax[c] : 0.0;
        if (vmin && c < nchan) st.given |= 1 << (2 * c);
        if (vmax && c < nchan) st.given |= 1 << (2 * c + 1);
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    int rcl = ND_AMD_EINVAL;
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        rcl = rgb_compose_launch<T>(a, reinterpret_cast<const T *>(limits), st, mask, out, stream);
    });
    return rcl;
}
