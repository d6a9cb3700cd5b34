// nd_amd/csrc/zonal.hip -- statistics of the zones of a label map, and their way back onto the pixels.
// include/nd_amd.h has the definition ("Statistics of zones"); tests/zonal_ref.py restates it bit for bit.
//
//   nd_amd_zonal_keys    every pixel's zone rank (int32; n = no zone) from a label plane of any map type
//   nd_amd_zonal_stats   count, nan_count, sum, min, max, m2 of every (plane, zone) through the inverted index
//                        (perm, offsets) that the CALLER builds from the keys: a stable sort and a search
//   nd_amd_zonal_paint   a (plane, zone) table painted back onto the pixels of its zones
//
// A segmented reduction without a floating-point atomic.  Zone z's pixels are perm[offsets[z] .. offsets[z + 1]), in
// raster order because the sort is stable: its sequence, positions 0 .. m - 1.  Every floating-point sum is formed in
// ONE TREE, a function of the zone's own sequence alone:
//
//   chunk     64 consecutive positions, one per lane, summed by the aligned pairwise tree: lane l with l ^ 1, then
//             ^ 2 ... ^ 32.  A position that is absent (behind the zone's end) or skipped (NaN) does not take part:
//             a (+) absent = a, not a + 0.0 -- so a group of 8 lanes serving a zone of 8 pixels forms the same bits
//             as a whole wave.
//   segment   64 chunks (4096 positions), their sums added sequentially in order, a chunk without a participant left out
//   zone      its segments' sums added sequentially in order, a segment without a participant left out
//
// m2 uses the same tree over (c - mean) * (c - mean), one rounding for the difference and one for the product
// (-ffp-contract=off), mean = sum / count in one IEEE division.  min and max are exact in any order.
//
// The kernels.  A wave is the unit of work; a block is four independent waves.
//   stats     waves 0 .. ceil(n / 8) - 1 take 8 consecutive zones each and serve those of at most 8 pixels together,
//             one per group of 8 lanes.  The next n waves take one zone each, if it has more than 8 pixels: a zone of
//             at most 64 pixels in one chunk with its values kept in registers between the two sums, a larger one by
//             its FIRST segment.  The waves behind them take one block of 4096 sorted positions each: at most one
//             later segment (s >= 1) of any zone starts inside such a block (two starts of one zone lie 4096 apart,
//             and a zone that begins behind a start has its own second segment 4096 behind its beginning), found by
//             a binary search in offsets.  So the grid is ceil(n / 8) + n + ceil(npix / 4096) waves, known to the
//             host without reading anything back; a wave that finds nothing to do ends at once.
//             A wave reads its 64 entries of perm once per chunk and walks the planes with them (eight loads in
//             flight); plane p's running sums live in lane p, 64 planes at a time.  A zone of one segment is finished
//             by its wave, the second sum over the same pixels included.  A segment of a longer zone goes to a slot of
//             the workspace: slot j for the later segment that starts in block j, slot nblocks + j for the first
//             segment of the (only) zone of more than 4096 pixels that begins in block j.
//   fold      one lane per (zone, plane) adds the slots of a zone of several segments in order
//   m2        the second sum of those zones, one wave per block of positions again (the wave of a zone's segment 1
//             takes segment 0 as well), and the fold once more
//   keys, paint   one lane per pixel
// No kernel holds a private array; perm entries and offsets are range-checked, so a wrong index reads nothing.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "common.hpp"
#include "dispatch.hpp"

using namespace nd_amd;

namespace {

constexpr int ZN_CHUNK = 64;                        // positions of a chunk: one per lane
constexpr int ZN_SEG = 4096;                        // positions of a segment: 64 chunks
constexpr int ZN_GROUP = 8;                         // lanes of a sub-wave group, and zones of a wave
constexpr int ZN_WAVES = 4;                         // waves of a block
constexpr int ZN_BATCH = 64;                        // planes whose running sums a wave keeps, one per lane
constexpr int ZN_LOADS = 8;                         // planes whose values a lane loads before it sums them
constexpr int ZN_PX = 256;                          // lanes of a block of the keys / paint / fold kernels
constexpr int64_t ZN_MAX_BLOCKS = ((int64_t)1 << 31) - 1;

struct ZnArgs {
    const void *values;
    int64_t sp, sy, sx;                             // strides in elements: plane, y, x
    int64_t nplanes, nx, npix, n, nblocks;          // nblocks: ceil(npix / ZN_SEG)
    const int32_t *perm;
    const int64_t *offsets;
    int64_t *count, *nan_count;                     // outputs (nplanes, n), each may be null
    double *sum, *mn, *mx, *m2;
    double *tsum;                                   // sum and count of the zones of several segments, for the mean:
    int64_t *tcnt;                                  //   the outputs, or the workspace where they are null
    double *s_sum, *s_min, *s_max, *s_m2;           // slots [2 * nblocks][nplanes]
    int32_t *s_cnt, *s_nan;
};

__device__ __forceinline__ bool zn_any(uint64_t mask, int base, int d)
{
    const uint64_t g = d >= 64 ? ~0ull : ((1ull << d) - 1ull);
    return ((mask >> base) & g) != 0;
}

// the aligned pairwise sum over the lanes of `mask` inside every aligned group of `group` lanes; every lane of a
// group that has a participant holds the group's sum afterwards (a + b and b + a are the same bits)
__device__ __forceinline__ double zn_tree_sum(double v, uint64_t mask, int group)
{
    const int lane = threadIdx.x;
    for (int d = 1; d < group; d <<= 1) {
        const double o = __shfl_xor(v, d);
        const int mine = lane & ~(d - 1);
        const bool a = zn_any(mask, mine, d), b = zn_any(mask, mine ^ d, d);
        v = (a && b) ? v + o : (b ? o : v);
    }
    return v;
}

__device__ __forceinline__ double zn_tree_min(double v, int group)
{
    for (int d = 1; d < group; d <<= 1) v = fmin(v, __shfl_xor(v, d));
    return v;
}

__device__ __forceinline__ double zn_tree_max(double v, int group)
{
    for (int d = 1; d < group; d <<= 1) v = fmax(v, __shfl_xor(v, d));
    return v;
}

// a zone's extent in perm, cut to what perm holds
__device__ __forceinline__ void zn_extent(const ZnArgs &a, int64_t z, int64_t *o0, int64_t *m)
{
    int64_t lo = a.offsets[z], hi = a.offsets[z + 1];
    lo = lo < 0 ? 0 : (lo > a.npix ? a.npix : lo);
    hi = hi < lo ? lo : (hi > a.npix ? a.npix : hi);
    *o0 = lo;
    *m = hi - lo;
}

// the element offset of the pixel at perm[at], *present cleared where the entry is no pixel of the plane
__device__ __forceinline__ int64_t zn_pixel(const ZnArgs &a, int64_t at, bool *present)
{
    const int32_t idx = *present ? a.perm[at] : 0;
    if ((uint32_t)idx >= (uint64_t)a.npix) {
        *present = false;
        return 0;
    }
    const int32_t nx = (int32_t)a.nx;
    return (int64_t)(idx / nx) * a.sy + (int64_t)(idx % nx) * a.sx;
}

// ---- zones of one chunk: one zone per aligned group of `group` lanes (8, or 64: the whole wave), every statistic
// from registers.  `active`: the lane's group has a zone to serve; every lane of the wave walks the planes
template <class T>
__device__ __forceinline__ void zn_small(const ZnArgs &a, int64_t z, bool active, int group)
{
    const int lane = threadIdx.x, l = lane & (group - 1), gbase = lane - l;
    const uint64_t gm = group >= 64 ? ~0ull : ((1ull << group) - 1ull);
    int64_t o0 = 0, m = 0;
    if (active) zn_extent(a, z, &o0, &m);
    bool present = active && l < m;
    const int64_t eoff = zn_pixel(a, o0 + l, &present);
    const T *v = reinterpret_cast<const T *>(a.values);
    const bool writer = active && l == 0;
    for (int64_t p = 0; p < a.nplanes; ++p) {
        T x = T(0);
        if (present) x = v[p * a.sp + eoff];
        const bool part = present && x == x;
        const uint64_t mask = __ballot(part), nmask = __ballot(present && x != x);
        const int cnt = __popcll((mask >> gbase) & gm), nans = __popcll((nmask >> gbase) & gm);
        const double c = (double)x;
        double s = zn_tree_sum(c, mask, group);
        s = cnt ? s : 0.0;
        const int64_t at = p * a.n + z;
        if (a.m2) {
            const double mean = s / (double)cnt;
            const double t = c - mean;
            double r = zn_tree_sum(t * t, mask, group);
            r = cnt ? r : 0.0;
            if (writer) a.m2[at] = r;
        }
        if (a.mn) {
            const double r = zn_tree_min(part ? c : (double)INFINITY, group);
            if (writer) a.mn[at] = cnt ? r : (double)NAN;
        }
        if (a.mx) {
            const double r = zn_tree_max(part ? c : -(double)INFINITY, group);
            if (writer) a.mx[at] = cnt ? r : (double)NAN;
        }
        if (writer) {
            if (a.sum) a.sum[at] = s;
            if (a.count) a.count[at] = cnt;
            if (a.nan_count) a.nan_count[at] = nans;
        }
    }
}

// what lane p keeps of plane pb + p along a segment
struct ZnAcc {
    double sum, mn, mx, m2;
    int cnt, nan, cnt2;
};

__device__ __forceinline__ void zn_clear(ZnAcc &c)
{
    c.sum = c.m2 = 0.0;
    c.mn = (double)INFINITY;
    c.mx = -(double)INFINITY;
    c.cnt = c.nan = c.cnt2 = 0;
}

// ---- a segment: `len` positions from perm[base] on, `np` planes from plane pb on, chunk by chunk.  SECOND: the sum
// of squares around `mean` (lane p's is plane pb + p's), else count, nan, sum, min, max
template <class T, bool SECOND>
__device__ __forceinline__ void zn_walk(const ZnArgs &a, int64_t base, int len, int64_t pb, int np, double mean,
                                        ZnAcc &acc)
{
    const int lane = threadIdx.x;
    const T *v = reinterpret_cast<const T *>(a.values) + pb * a.sp;
    for (int c0 = 0; c0 < len; c0 += ZN_CHUNK) {
        bool present = c0 + lane < len;
        const int64_t eoff = zn_pixel(a, base + c0 + lane, &present);
        for (int p0 = 0; p0 < np; p0 += ZN_LOADS) {
            T xs[ZN_LOADS];
#pragma unroll
            for (int k = 0; k < ZN_LOADS; ++k) {
                xs[k] = T(0);
                if (present && p0 + k < np) xs[k] = v[(int64_t)(p0 + k) * a.sp + eoff];
            }
#pragma unroll
            for (int k = 0; k < ZN_LOADS; ++k) {
                const int p = p0 + k;
                if (p >= np) break;                 // (wave-uniform)
                const T x = xs[k];
                const bool part = present && x == x;
                const uint64_t mask = __ballot(part);
                const double c = (double)x;
                if constexpr (!SECOND) {
                    const uint64_t nmask = __ballot(present && x != x);
                    const double s = zn_tree_sum(c, mask, ZN_CHUNK);
                    const double lo = zn_tree_min(part ? c : (double)INFINITY, ZN_CHUNK);
                    const double hi = zn_tree_max(part ? c : -(double)INFINITY, ZN_CHUNK);
                    if (lane == p) {
                        if (mask) {
                            acc.sum = acc.cnt ? acc.sum + s : s;
                            acc.mn = fmin(acc.mn, lo);
                            acc.mx = fmax(acc.mx, hi);
                        }
                        acc.cnt += __popcll(mask);
                        acc.nan += __popcll(nmask);
                    }
                } else {
                    const double mu = __shfl(mean, p);
                    const double t = c - mu;
                    const double s = zn_tree_sum(t * t, mask, ZN_CHUNK);
                    if (lane == p && mask) {
                        acc.m2 = acc.cnt2 ? acc.m2 + s : s;
                        acc.cnt2 += __popcll(mask);
                    }
                }
            }
        }
    }
}

// ---- the first segment of a zone of more than 64 pixels, by the whole wave
template <class T>
__device__ __forceinline__ void zn_first(const ZnArgs &a, int64_t z)
{
    const int lane = threadIdx.x;
    int64_t o0, m;
    zn_extent(a, z, &o0, &m);
    const bool single = m <= ZN_SEG;
    const int len = (int)(single ? m : ZN_SEG);
    for (int64_t pb = 0; pb < a.nplanes; pb += ZN_BATCH) {
        const int np = (int)(a.nplanes - pb < ZN_BATCH ? a.nplanes - pb : ZN_BATCH);
        ZnAcc acc;
        zn_clear(acc);
        zn_walk<T, false>(a, o0, len, pb, np, 0.0, acc);
        if (single) {
            const double s = acc.cnt ? acc.sum : 0.0;
            if (a.m2) zn_walk<T, true>(a, o0, len, pb, np, s / (double)acc.cnt, acc);
            if (lane < np) {
                const int64_t at = (pb + lane) * a.n + z;
                if (a.count) a.count[at] = acc.cnt;
                if (a.nan_count) a.nan_count[at] = acc.nan;
                if (a.sum) a.sum[at] = s;
                if (a.mn) a.mn[at] = acc.cnt ? acc.mn : (double)NAN;
                if (a.mx) a.mx[at] = acc.cnt ? acc.mx : (double)NAN;
                if (a.m2) a.m2[at] = acc.cnt2 ? acc.m2 : 0.0;
            }
        } else if (lane < np) {
            const int64_t at = (a.nblocks + o0 / ZN_SEG) * a.nplanes + pb + lane;
            a.s_sum[at] = acc.sum;
            a.s_min[at] = acc.mn;
            a.s_max[at] = acc.mx;
            a.s_cnt[at] = acc.cnt;
            a.s_nan[at] = acc.nan;
        }
    }
}

// the later segment (s >= 1) that starts inside block j of the sorted positions: its zone, where it starts and its
// length; false if there is none
__device__ __forceinline__ bool zn_later_segment(const ZnArgs &a, int64_t j, int64_t *zone, int64_t *start, int *len,
                                                 int64_t *segment)
{
    const int64_t q = j * ZN_SEG;
    int64_t total = a.offsets[a.n];
    total = total > a.npix ? a.npix : total;
    if (q >= total) return false;
    int64_t lo = 0, hi = a.n - 1;                   // the last zone whose offset is <= q
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.offsets[mid] <= q) lo = mid; else hi = mid - 1;
    }
    int64_t o0, m;
    zn_extent(a, lo, &o0, &m);
    if (q < o0 || q >= o0 + m) return false;
    const int64_t s = (q - o0 + ZN_SEG - 1) / ZN_SEG;
    const int64_t at = s * ZN_SEG;
    if (s == 0 || at >= m) return false;
    *zone = lo;
    *start = o0 + at;
    *len = (int)(m - at < ZN_SEG ? m - at : ZN_SEG);
    *segment = s;
    return true;
}

template <class T>
__global__ __launch_bounds__(ZN_CHUNK * ZN_WAVES) void zonal_stats_kernel(ZnArgs a, int64_t zone_waves)
{
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * ZN_WAVES + threadIdx.y;
    if (w < zone_waves) {
        // the zones of at most 8 pixels, 8 consecutive zones together, one per group of lanes
        const int64_t z = w * ZN_GROUP + lane / ZN_GROUP;
        bool small = false;
        if (z < a.n) {
            int64_t o0, m;
            zn_extent(a, z, &o0, &m);
            small = m <= ZN_GROUP;
        }
        if (__ballot(small)) zn_small<T>(a, z, small, ZN_GROUP);
        return;
    }
    if (w < zone_waves + a.n) {
        // a larger zone: one chunk, or its first segment
        const int64_t zz = w - zone_waves;
        int64_t o0, m;
        zn_extent(a, zz, &o0, &m);
        if (m <= ZN_GROUP) return;
        if (m <= ZN_CHUNK) zn_small<T>(a, zz, true, ZN_CHUNK);
        else zn_first<T>(a, zz);
        return;
    }
    const int64_t j = w - zone_waves - a.n;
    if (j >= a.nblocks) return;
    int64_t z, start, s;
    int len;
    if (!zn_later_segment(a, j, &z, &start, &len, &s)) return;
    for (int64_t pb = 0; pb < a.nplanes; pb += ZN_BATCH) {
        const int np = (int)(a.nplanes - pb < ZN_BATCH ? a.nplanes - pb : ZN_BATCH);
        ZnAcc acc;
        zn_clear(acc);
        zn_walk<T, false>(a, start, len, pb, np, 0.0, acc);
        if (lane < np) {
            const int64_t at = j * a.nplanes + pb + lane;
            a.s_sum[at] = acc.sum;
            a.s_min[at] = acc.mn;
            a.s_max[at] = acc.mx;
            a.s_cnt[at] = acc.cnt;
            a.s_nan[at] = acc.nan;
        }
    }
}

// ---- m2 of the zones of several segments: the wave of block j takes the later segment that starts there, and
// segment 0 as well where that is segment 1
template <class T>
__global__ __launch_bounds__(ZN_CHUNK * ZN_WAVES) void zonal_m2_kernel(ZnArgs a)
{
    const int lane = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * ZN_WAVES + threadIdx.y;
    if (j >= a.nblocks) return;
    int64_t z, start, s;
    int len;
    if (!zn_later_segment(a, j, &z, &start, &len, &s)) return;
    for (int64_t pb = 0; pb < a.nplanes; pb += ZN_BATCH) {
        const int np = (int)(a.nplanes - pb < ZN_BATCH ? a.nplanes - pb : ZN_BATCH);
        double mean = 0.0;
        if (lane < np) mean = a.tsum[(pb + lane) * a.n + z] / (double)a.tcnt[(pb + lane) * a.n + z];
        ZnAcc acc;
        zn_clear(acc);
        zn_walk<T, true>(a, start, len, pb, np, mean, acc);
        if (lane < np) a.s_m2[j * a.nplanes + pb + lane] = acc.m2;
        if (s == 1) {
            const int64_t o0 = start - ZN_SEG;
            zn_clear(acc);
            zn_walk<T, true>(a, o0, ZN_SEG, pb, np, mean, acc);
            if (lane < np) a.s_m2[(a.nblocks + o0 / ZN_SEG) * a.nplanes + pb + lane] = acc.m2;
        }
    }
}

// ---- fold: the segments of a zone of several, in order.  SECOND: m2, else the other five
template <bool SECOND>
__global__ __launch_bounds__(ZN_PX) void zonal_fold_kernel(ZnArgs a, int64_t items)
{
    const int64_t t = (int64_t)blockIdx.x * ZN_PX + threadIdx.x;
    if (t >= items) return;
    const int64_t z = t / a.nplanes, p = t % a.nplanes;
    int64_t o0, m;
    zn_extent(a, z, &o0, &m);
    if (m <= ZN_SEG) return;
    const int64_t nseg = (m + ZN_SEG - 1) / ZN_SEG;
    const int64_t out = p * a.n + z;
    int64_t at = (a.nblocks + o0 / ZN_SEG) * a.nplanes + p;
    int64_t cnt = a.s_cnt[at];
    if constexpr (SECOND) {
        double m2 = a.s_m2[at];
        for (int64_t s = 1; s < nseg; ++s) {
            at = ((o0 + s * ZN_SEG) / ZN_SEG) * a.nplanes + p;
            const int c = a.s_cnt[at];
            const double v = a.s_m2[at];
            if (c) m2 = cnt ? m2 + v : v;
            cnt += c;
        }
        a.m2[out] = cnt ? m2 : 0.0;
    } else {
        int64_t nans = a.s_nan[at];
        double sum = a.s_sum[at], lo = a.s_min[at], hi = a.s_max[at];
        for (int64_t s = 1; s < nseg; ++s) {
            at = ((o0 + s * ZN_SEG) / ZN_SEG) * a.nplanes + p;
            const int c = a.s_cnt[at];
            const double v = a.s_sum[at];
            if (c) {
                sum = cnt ? sum + v : v;
                lo = fmin(lo, a.s_min[at]);
                hi = fmax(hi, a.s_max[at]);
            }
            cnt += c;
            nans += a.s_nan[at];
        }
        sum = cnt ? sum : 0.0;
        a.tsum[out] = sum;
        a.tcnt[out] = cnt;
        if (a.nan_count) a.nan_count[out] = nans;
        if (a.mn) a.mn[out] = cnt ? lo : (double)NAN;
        if (a.mx) a.mx[out] = cnt ? hi : (double)NAN;
    }
}

// ---- keys
// the label as an int64 if it is one: integers as they are, floating values where they are whole and in range
template <class T>
__device__ __forceinline__ bool zn_label(T v, int64_t *out)
{
    if constexpr (std::is_floating_point<T>::value) {
        if (!(v >= (T)-9223372036854775808.0 && v < (T)9223372036854775808.0) || v != trunc(v)) return false;
        *out = (int64_t)v;
    } else {
        *out = (int64_t)v;
    }
    return true;
}

template <class T>
__global__ __launch_bounds__(ZN_PX) void zonal_keys_kernel(const T *labels, int64_t sy, int64_t sx, int64_t nx, int64_t npix,
                                                           const int64_t *ids, int64_t n, int32_t *keys)
{
    const int64_t i = (int64_t)blockIdx.x * ZN_PX + threadIdx.x;
    if (i >= npix) return;
    int64_t v, key = n;
    if (zn_label<T>(labels[(i / nx) * sy + (i % nx) * sx], &v)) {
        if (!ids) {
            if (v >= 1 && v <= n) key = v - 1;
        } else {
            int64_t lo = 0, hi = n;                 // the first id that is >= v
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (ids[mid] < v) lo = mid + 1; else hi = mid;
            }
            if (lo < n && ids[lo] == v) key = lo;
        }
    }
    keys[i] = (int32_t)key;
}

// ---- paint.  PLANE_FAST: consecutive lanes take the planes of one pixel ((y, x, time) memory), else the pixels of one
// plane
template <class T, bool PLANE_FAST>
__global__ __launch_bounds__(ZN_PX) void zonal_paint_kernel(const int32_t *keys, const double *table, int64_t nplanes,
                                                            int64_t nx, int64_t npix, int64_t n, const T *src,
                                                            int64_t ssp, int64_t ssy, int64_t ssx, T *dst, int64_t dsp,
                                                            int64_t dsy, int64_t dsx, double fill)
{
    const int64_t t = (int64_t)blockIdx.x * ZN_PX + threadIdx.x;
    if (t >= npix * nplanes) return;
    const int64_t i = PLANE_FAST ? t / nplanes : t % npix, p = PLANE_FAST ? t % nplanes : t / npix;
    const int64_t y = i / nx, x = i % nx;
    const int32_t key = keys[i];
    T v;
    if ((uint32_t)key < (uint64_t)n) v = (T)table[p * n + key];
    else if (src) v = src[p * ssp + y * ssy + x * ssx];
    else v = (T)fill;
    dst[p * dsp + y * dsy + x * dsx] = v;
}

// ---- host
struct ZnPlan {
    size_t sum_off, min_off, max_off, m2_off, cnt_off, nan_off, tsum_off, tcnt_off, bytes;
    int64_t nblocks;
};

ZnPlan zn_plan(int64_t nplanes, int64_t ny, int64_t nx, int64_t n)
{
    ZnPlan p;
    p.nblocks = ceil_div(ny * nx, ZN_SEG);
    const size_t slots = (size_t)2 * (size_t)p.nblocks * (size_t)nplanes;
    const size_t d = align256(slots * sizeof(double)), i = align256(slots * sizeof(int32_t));
    const size_t t = align256((size_t)nplanes * (size_t)n * sizeof(double));
    p.sum_off = 0;
    p.min_off = p.sum_off + d;
    p.max_off = p.min_off + d;
    p.m2_off = p.max_off + d;
    p.cnt_off = p.m2_off + d;
    p.nan_off = p.cnt_off + i;
    p.tsum_off = p.nan_off + i;
    p.tcnt_off = p.tsum_off + t;
    p.bytes = p.tcnt_off + t;
    return p;
}

int zn_blocks(const char *fn, int64_t items, int64_t per_block, unsigned *blocks)
{
    const int64_t b = ceil_div(items, per_block);
    if (b > ZN_MAX_BLOCKS) {
        set_error("%s: %lld blocks are more than one launch holds: pass fewer planes per call", fn, (long long)b);
        return ND_AMD_EUNSUPPORTED;
    }
    *blocks = (unsigned)b;
    return ND_AMD_OK;
}

// what the three entries check alike, in this order; *empty: nothing to do
int zn_check(const char *fn, int64_t nplanes, int64_t ny, int64_t nx, int64_t n, bool *empty)
{
    int rc = check_shape(fn, ny, nx, nplanes, empty);
    if (rc == ND_AMD_OK) rc = check_plane_pixels(fn, ny, nx);
    if (rc == ND_AMD_OK) rc = check_zone_count(fn, n);
    return rc;
}

template <int D> struct zn_type;
template <> struct zn_type<ND_AMD_F32> { using type = float; };
template <> struct zn_type<ND_AMD_F64> { using type = double; };
template <> struct zn_type<ND_AMD_I64> { using type = int64_t; };
template <> struct zn_type<ND_AMD_I32> { using type = int32_t; };
template <> struct zn_type<ND_AMD_U8> { using type = uint8_t; };

}  // namespace

extern "C" int nd_amd_zonal_keys(const void *labels, int dtype, int64_t ny, int64_t nx, const int64_t *label_strides,
                                 const int64_t *ids, int64_t n, int32_t *keys, void *hip_stream)
{
    const char *fn = "nd_amd_zonal_keys";
    bool empty = false;
    int rc = check_region_dtype(fn, dtype);
    if (rc == ND_AMD_OK) rc = zn_check(fn, 1, ny, nx, n, &empty);
    if (rc != ND_AMD_OK || empty) return rc;
    rc = check_strides2(fn, "label_strides", label_strides);
    if (rc != ND_AMD_OK) return rc;
    if (!labels || !keys) {
        set_error("%s: labels or keys is null", fn);
        return ND_AMD_EINVAL;
    }
    unsigned blocks = 0;
    rc = zn_blocks(fn, ny * nx, ZN_PX, &blocks);
    if (rc != ND_AMD_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    KernelTimer timer(ND_AMD_KERNEL_ZONAL, stream);
    pick_eq<ND_AMD_F32, ND_AMD_F64, ND_AMD_I64, ND_AMD_I32, ND_AMD_U8>(dtype, [&](auto D) {
        using T = typename zn_type<decltype(D)::value>::type;
        hipLaunchKernelGGL((zonal_keys_kernel<T>), dim3(blocks), dim3(ZN_PX), 0, stream,
                           reinterpret_cast<const T *>(labels), label_strides[0], label_strides[1], nx, ny * nx, ids, n,
                           keys);
    });
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" size_t nd_amd_zonal_workspace_bytes(int64_t nplanes, int64_t ny, int64_t nx, int64_t n)
{
    const char *fn = "nd_amd_zonal_workspace_bytes";
    if (nplanes <= 0 || ny <= 0 || nx <= 0 || n <= 0 || check_plane_pixels(fn, ny, nx) != ND_AMD_OK
        || check_zone_count(fn, n) != ND_AMD_OK)
        return 0;
    return zn_plan(nplanes, ny, nx, n).bytes;
}

extern "C" int nd_amd_zonal_stats(const void *values, int dtype, int64_t nplanes, int64_t ny, int64_t nx,
                                  const int64_t *strides, const int32_t *perm, const int64_t *offsets, int64_t n,
                                  int64_t *count, int64_t *nan_count, double *sum, double *min, double *max,
                                  double *m2, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    const char *fn = "nd_amd_zonal_stats";
    bool empty = false;
    int rc = check_dtype(fn, dtype);
    if (rc == ND_AMD_OK) rc = zn_check(fn, nplanes, ny, nx, n, &empty);
    if (rc != ND_AMD_OK || empty || n == 0) return rc;
    rc = check_strides(fn, "strides", strides);
    if (rc != ND_AMD_OK) return rc;
    if (!values || !perm || !offsets) {
        set_error("%s: values, perm or offsets is null", fn);
        return ND_AMD_EINVAL;
    }
    if (!count && !nan_count && !sum && !min && !max && !m2) return ND_AMD_OK;
    const ZnPlan plan = zn_plan(nplanes, ny, nx, n);
    if (!workspace || workspace_bytes < plan.bytes) {
        set_error("%s: needs a workspace of %zu bytes, got %zu", fn, plan.bytes, workspace ? workspace_bytes : (size_t)0);
        return ND_AMD_EWORKSPACE;
    }
    const int64_t zone_waves = ceil_div(n, ZN_GROUP);
    unsigned stat_blocks = 0, fold_blocks = 0, m2_blocks = 0;
    rc = zn_blocks(fn, zone_waves + n + plan.nblocks, ZN_WAVES, &stat_blocks);
    // (n < 2^31: the product overflows nothing where nplanes passes this cap)
    if (rc == ND_AMD_OK) rc = zn_blocks(fn, n * (nplanes > ((int64_t)1 << 31) ? (int64_t)1 << 31 : nplanes), ZN_PX, &fold_blocks);
    if (rc == ND_AMD_OK) rc = zn_blocks(fn, plan.nblocks, ZN_WAVES, &m2_blocks);
    if (rc != ND_AMD_OK) return rc;

    unsigned char *w = reinterpret_cast<unsigned char *>(workspace);
    ZnArgs a;
    a.values = values;
    a.sp = strides[0]; a.sy = strides[1]; a.sx = strides[2];
    a.nplanes = nplanes; a.nx = nx; a.npix = ny * nx; a.n = n; a.nblocks = plan.nblocks;
    a.perm = perm;
    a.offsets = offsets;
    a.count = count; a.nan_count = nan_count; a.sum = sum; a.mn = min; a.mx = max; a.m2 = m2;
    a.tsum = sum ? sum : reinterpret_cast<double *>(w + plan.tsum_off);
    a.tcnt = count ? count : reinterpret_cast<int64_t *>(w + plan.tcnt_off);
    a.s_sum = reinterpret_cast<double *>(w + plan.sum_off);
    a.s_min = reinterpret_cast<double *>(w + plan.min_off);
    a.s_max = reinterpret_cast<double *>(w + plan.max_off);
    a.s_m2 = reinterpret_cast<double *>(w + plan.m2_off);
    a.s_cnt = reinterpret_cast<int32_t *>(w + plan.cnt_off);
    a.s_nan = reinterpret_cast<int32_t *>(w + plan.nan_off);

    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    KernelTimer timer(ND_AMD_KERNEL_ZONAL, stream);
    const bool several = a.npix > ZN_SEG;           // a zone of several segments can exist
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        hipLaunchKernelGGL((zonal_stats_kernel<T>), dim3(stat_blocks), dim3(ZN_CHUNK, ZN_WAVES), 0, stream, a,
                           zone_waves);
        if (!several) return;
        hipLaunchKernelGGL((zonal_fold_kernel<false>), dim3(fold_blocks), dim3(ZN_PX), 0, stream, a, n * nplanes);
        if (!m2) return;
        hipLaunchKernelGGL((zonal_m2_kernel<T>), dim3(m2_blocks), dim3(ZN_CHUNK, ZN_WAVES), 0, stream, a);
        hipLaunchKernelGGL((zonal_fold_kernel<true>), dim3(fold_blocks), dim3(ZN_PX), 0, stream, a, n * nplanes);
    });
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_zonal_paint(const int32_t *keys, const double *table, int64_t nplanes, int64_t ny, int64_t nx,
                                  int64_t n, const void *src, const int64_t *src_strides, void *dst,
                                  const int64_t *dst_strides, int dtype, double fill, void *hip_stream)
{
    const char *fn = "nd_amd_zonal_paint";
    bool empty = false;
    int rc = check_dtype(fn, dtype);
    if (rc == ND_AMD_OK) rc = zn_check(fn, nplanes, ny, nx, n, &empty);
    if (rc != ND_AMD_OK || empty) return rc;
    rc = check_strides(fn, "dst_strides", dst_strides);
    if (rc == ND_AMD_OK && src) rc = check_strides(fn, "src_strides", src_strides);
    if (rc != ND_AMD_OK) return rc;
    if (!keys || !dst || (n > 0 && !table)) {
        set_error("%s: keys, table or dst is null", fn);
        return ND_AMD_EINVAL;
    }
    unsigned blocks = 0;
    if (nplanes > ZN_MAX_BLOCKS / ceil_div(ny * nx, ZN_PX)) {
        set_error("%s: more blocks than one launch holds: paint fewer planes per call", fn);
        return ND_AMD_EUNSUPPORTED;
    }
    rc = zn_blocks(fn, ny * nx * nplanes, ZN_PX, &blocks);
    if (rc != ND_AMD_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    KernelTimer timer(ND_AMD_KERNEL_ZONAL, stream);
    const int64_t ss[3] = {src ? src_strides[0] : 0, src ? src_strides[1] : 0, src ? src_strides[2] : 0};
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        pick(dst_strides[0] < dst_strides[2], [&](auto PF) {
            hipLaunchKernelGGL((zonal_paint_kernel<T, decltype(PF)::value>), dim3(blocks), dim3(ZN_PX), 0, stream, keys,
                               table, nplanes, nx, ny * nx, n, reinterpret_cast<const T *>(src), ss[0], ss[1], ss[2],
                               reinterpret_cast<T *>(dst), dst_strides[0], dst_strides[1], dst_strides[2], fill);
        });
    });
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}
