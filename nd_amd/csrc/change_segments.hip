// nd_amd/csrc/change_segments.hip -- direction of each detected change and the segment means, on gfx950.
//
// EXTENSION (no reference counterpart; tests/change_segments_ref.py restates the definition in numpy).  Given
// the planes an omnibus test reads and a change map c[y, x, t] (non-zero: date t opens a new segment, the
// meaning of nd/_change.pyx:253; c[.., 0] is ignored), per pixel and in double, in date order:
//   l = 0; s_p = 0; m = 0
//   t >= 1 and c[t] != 0:  mean_p = s_p / m;  d_p = (double)x_p[t] - mean_p;  direction[t] = code(d)
//                          means_p[l .. t-1] = (T)mean_p;  l = t; s_p = 0; m = 0          else direction[t] = 0
//   s_p = s_p + (double)x_p[t];  m = m + 1
//   means_p[l .. k-1] = (T)(s_p / m)
// code(d): the Loewner order of the difference, 1 positive definite, 2 negative definite, 3 anything else
// (indefinite, semi-definite, singular, NaN) -- Canty's bmap coding; by leading principal minors, the
// operations bracketed as direction_code writes them (the library is built with -ffp-contract=off).
//
// One kernel, change_segments_kernel<T, P, DIRECTION, MEANS>; the number of planes names the structure
// (1..3 intensities, 4 = C2, 9 = C3).  One lane per pixel, x fastest across the lanes: every plane access of a
// date is a row piece of 64 consecutive elements when stride_x == 1 (any strides are served; time-fastest
// data are transposed one level up).  The walk over the dates is in lockstep across the wave and keeps the
// running sums only -- nothing grows with k.
//
// The means.  A lane knows a segment's mean only when the segment closes, and the lanes of a wave close at
// different dates.  The forward walk stores the mean at the segment's LAST date only (the lanes closing at
// date t write date t - 1 in one masked store; every lane writes date k - 1); a backward walk, again in
// lockstep, picks that value up at each segment's last date (unless the segment is that one date) and stores
// it to the segment's other dates.  Every element of `means` is written exactly once and at most one value per
// segment and plane is read back: P sizeof(T) (2 k + segments) bytes per pixel and the map bytes, against the
// definition's 2 P k sizeof(T) + 2 k.  (DESIGN-EXPERIMENTS.md has the forms this was measured against.)
//
// The map bytes.  Map and direction are (y, x, time), time fastest: the rows of a wave's pixels are 64 k
// contiguous bytes.  Dates are taken in chunks of 32: the chunk's map bytes come in as 4-byte words of
// consecutive lanes, become one bit per date and pass through a wave-private LDS image to the lane that owns
// the row (a 32-bit mask per lane); the chunk's codes (two bits per date) leave the same way.  This needs
// k % 4 == 0 and a 4-byte aligned span; anything else takes per-lane byte accesses.  No block-wide barrier:
// a wave only reads the image it wrote (LDS operations of a wave complete in order).
#include "common.hpp"
#include "dispatch.hpp"
#include "memops.hpp"

namespace nd_amd {

constexpr int kCsThreads = 256;
constexpr int kCsChunk = 32;         // dates per chunk: one bit (map) / two bits (codes) per date in a register
constexpr int kCsUnroll = 4;         // dates whose loads are issued together (half as many beyond 32 bytes per date)
constexpr int kCsPitch = kCsChunk / 4 + 1;                 // words per row of the image: odd, so conflict-free
constexpr int kCsImgWords = 64 * kCsPitch;

template <typename T, int P>
struct SegArgs {
    const T *pl[P];
    T *mn[P];
    const uint8_t *change;
    int8_t *direction;
    int64_t nx, sy, sx, st, k, blocks_per_row;
};

// ---- the Loewner order of a difference -------------------------------------------------------------------
template <int P>
__device__ __forceinline__ int direction_code(const double (&d)[P])
{
    if constexpr (P <= 3) {
        bool pos = true, neg = true;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            pos = pos && d[c] > 0.0;
            neg = neg && d[c] < 0.0;
        }
        return pos ? 1 : (neg ? 2 : 3);
    } else if constexpr (P == 4) {                             // [C11, C12re, C12im, C22]
        const double a = d[0];
        const double det = (d[0] * d[3]) - ((d[1] * d[1]) + (d[2] * d[2]));
        return (a > 0.0 && det > 0.0) ? 1 : ((a < 0.0 && det > 0.0) ? 2 : 3);
    } else {                                                   // [C11, C22, C33, C12, C13, C23 re / im]
        static_assert(P == 9, "structures: 1..3 intensities, C2 (4 planes), C3 (9 planes)");
        const double d11 = d[0], d22 = d[1], d33 = d[2];
        const double r12 = d[3], i12 = d[4], r13 = d[5], i13 = d[6], r23 = d[7], i23 = d[8];
        const double n12 = r12 * r12 + i12 * i12;
        const double n13 = r13 * r13 + i13 * i13;
        const double n23 = r23 * r23 + i23 * i23;
        const double m1 = d11;
        const double m2 = (d11 * d22) - n12;
        const double tr = ((r12 * r23) - (i12 * i23)) * r13 + ((r12 * i23) + (i12 * r23)) * i13;
        const double m3 = (((d11 * d22) * d33) + (2.0 * tr)) - (((d11 * n23) + (d22 * n13)) + (d33 * n12));
        return (m1 > 0.0 && m2 > 0.0 && m3 > 0.0) ? 1 : ((m1 < 0.0 && m2 > 0.0 && m3 < 0.0) ? 2 : 3);
    }
}

// ---- the map bytes of dates [t0, t0 + tc) of the wave's wnp pixels -> one bit per date, per lane -------------
// wc: the first byte of the wave's rows.  words: k % 4 == 0 and wc 4-byte aligned (then t0 and tc are
// multiples of 4 as well).
__device__ __forceinline__ uint32_t load_map_bits(const uint8_t *wc, const int64_t k, const int64_t t0, const int tc,
                                                  const int wnp, const int lane, const bool words, uint32_t *img)
{
    uint32_t bits = 0u;
    if (words) {
        const int wpc = tc >> 2, n = wnp * wpc;
        for (int i = lane; i < n; i += 64) {
            const int r = i / wpc, w = i - r * wpc;
            const uint32_t v = *reinterpret_cast<const uint32_t *>(wc + ((int64_t)r * k + t0 + 4 * w));
            // the top bit of every non-zero byte, then those four bits side by side
            const uint32_t h = (v | ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
            img[r * kCsPitch + w] = (((h >> 7) * 0x00204081u) >> 21) & 0xFu;
        }
        wave_lds_fence();
        for (int w = 0; w < wpc; ++w) bits |= img[lane * kCsPitch + w] << (4 * w);
        wave_lds_fence();                                      // the image may be written again behind this
        if (lane >= wnp) bits = 0u;
    } else if (lane < wnp) {
        const uint8_t *p = wc + ((int64_t)lane * k + t0);
        for (int j = 0; j < tc; ++j) bits |= (p[j] != 0 ? 1u : 0u) << j;
    }
    return bits;
}

// ---- the codes of dates [t0, t0 + tc), two bits per date in dc, to the wave's rows of `direction` -----------
__device__ __forceinline__ void store_codes(int8_t *wd, const int64_t k, const int64_t t0, const int tc, const int wnp,
                                            const int lane, const bool words, uint32_t *img, const uint64_t dc)
{
    if (words) {
        const int wpc = tc >> 2, n = wnp * wpc;
        for (int w = 0; w < wpc; ++w) {
            const uint32_t c = (uint32_t)(dc >> (8 * w)) & 0xFFu;                  // four codes -> four bytes
            img[lane * kCsPitch + w] = (c & 0x03u) | ((c & 0x0Cu) << 6) | ((c & 0x30u) << 12) | ((c & 0xC0u) << 18);
        }
        wave_lds_fence();
        for (int i = lane; i < n; i += 64) {
            const int r = i / wpc, w = i - r * wpc;
            *reinterpret_cast<uint32_t *>(wd + ((int64_t)r * k + t0 + 4 * w)) = img[r * kCsPitch + w];
        }
        wave_lds_fence();
    } else if (lane < wnp) {
        int8_t *p = wd + ((int64_t)lane * k + t0);
        for (int j = 0; j < tc; ++j) p[j] = (int8_t)((dc >> (2 * j)) & 3ull);
    }
}

template <typename T, int P, bool DIRECTION, bool MEANS>
__global__ void __launch_bounds__(kCsThreads) change_segments_kernel(const SegArgs<T, P> g)
{
    __shared__ uint32_t lds_img[(kCsThreads / 64) * kCsImgWords];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t b = blockIdx.x;
    const int64_t row = b / g.blocks_per_row;
    const int64_t wpx0 = (b - row * g.blocks_per_row) * (int64_t)kCsThreads + (tid & ~63);
    const int64_t wleft = g.nx - wpx0;
    if (wleft <= 0) return;                                    // (no block-wide barrier below)
    const int wnp = wleft > 64 ? 64 : (int)wleft;
    const bool in = lane < wnp;
    const int64_t k = g.k, st = g.st;
    const int64_t off0 = row * g.sy + (in ? wpx0 + lane : g.nx - 1) * g.sx;       // idle lanes re-read the last pixel
    const int64_t wrow0 = (row * g.nx + wpx0) * k;             // the wave's rows of the map and of direction
    const uint8_t *wc = g.change + wrow0;
    int8_t *wd = DIRECTION ? g.direction + wrow0 : nullptr;
    uint32_t *img = lds_img + (tid >> 6) * kCsImgWords;
    const bool cwords = (k & 3) == 0 && ((uintptr_t)wc & 3) == 0;
    const bool dwords = DIRECTION && (k & 3) == 0 && ((uintptr_t)wd & 3) == 0;

    // ---- forward: the sums of the open segment; codes; each closed segment's mean at its last date --------
    double s[P], m = 0.0;
#pragma unroll
    for (int p = 0; p < P; ++p) s[p] = 0.0;
    uint32_t cm = 0u;
    int64_t t0 = 0;
    // (the loads of the next dates are issued before the current ones are worked on: loads and stores return in
    //  order, and a load waited for behind this group's stores would wait for those stores as well)
    constexpr int kU = P * sizeof(T) > 32 ? kCsUnroll / 2 : kCsUnroll;
    T v[kU][P], vn[kU][P];
    auto load_dates = [&](T(&dst)[kU][P], const int64_t first) {
#pragma unroll
        for (int jj = 0; jj < kU; ++jj) {
            const int64_t t = first + jj < k ? first + jj : k - 1;
            const int64_t off = off0 + t * st;
#pragma unroll
            for (int p = 0; p < P; ++p) dst[jj][p] = __builtin_nontemporal_load(g.pl[p] + off);
        }
    };
    load_dates(v, 0);
    for (;; t0 += kCsChunk) {
        const int tc = k - t0 > kCsChunk ? kCsChunk : (int)(k - t0);
        cm = load_map_bits(wc, k, t0, tc, wnp, lane, cwords, img);
        if (t0 == 0) cm &= ~1u;                                // nothing lies before date 0
        uint64_t dc = 0ull;
        for (int j0 = 0; j0 < tc; j0 += kU) {
            load_dates(vn, t0 + j0 + kU);
#pragma unroll
            for (int jj = 0; jj < kU; ++jj) {
                const int j = j0 + jj;
                if (j < tc) {
                    if ((cm >> j) & 1u) {
                        const int64_t off = off0 + (t0 + j - 1) * st;
                        double d[P];
#pragma unroll
                        for (int p = 0; p < P; ++p) {
                            const double mean = s[p] / m;
                            d[p] = (double)v[jj][p] - mean;
                            if (MEANS) g.mn[p][off] = (T)mean;
                            s[p] = 0.0;
                        }
                        m = 0.0;
                        if (DIRECTION) dc |= (uint64_t)direction_code<P>(d) << (2 * j);
                    }
#pragma unroll
                    for (int p = 0; p < P; ++p) s[p] = s[p] + (double)v[jj][p];
                    m = m + 1.0;
                }
            }
#pragma unroll
            for (int jj = 0; jj < kU; ++jj)
#pragma unroll
                for (int p = 0; p < P; ++p) v[jj][p] = vn[jj][p];
        }
        if (DIRECTION) store_codes(wd, k, t0, tc, wnp, lane, dwords, img, dc);
        if (t0 + kCsChunk >= k) break;
    }
    if (!MEANS) return;
    if (in) {
        const int64_t off = off0 + (k - 1) * st;
#pragma unroll
        for (int p = 0; p < P; ++p) g.mn[p][off] = (T)(s[p] / m);
    }

    // ---- backward: a segment's value, found at its last date, goes to its other dates -------------------------
    // (t0 and cm are the last chunk's; a lane reads back only what it stored itself)
    T carry[P];
#pragma unroll
    for (int p = 0; p < P; ++p) carry[p] = (T)0;
    bool last = true;                                          // date k - 1 closes a segment
    for (;; t0 -= kCsChunk) {
        const int tc = k - t0 > kCsChunk ? kCsChunk : (int)(k - t0);
        if (t0 + kCsChunk < k) {
            cm = load_map_bits(wc, k, t0, tc, wnp, lane, cwords, img);
            if (t0 == 0) cm &= ~1u;
        }
        if (in) {
            for (int j = tc - 1; j >= 0; --j) {
                const int64_t off = off0 + (t0 + j) * st;
                const bool opens = ((cm >> j) & 1u) != 0u;     // date t opens a segment: t - 1 is a last date
                if (!last) {
#pragma unroll
                    for (int p = 0; p < P; ++p) g.mn[p][off] = carry[p];
                } else if (!opens && t0 + j > 0) {             // (a one-date segment has nothing to carry)
#pragma unroll
                    for (int p = 0; p < P; ++p) carry[p] = g.mn[p][off];
                }
                last = opens;
            }
        }
        if (t0 == 0) break;
    }
}

// =========================================================================================
// host side
template <typename T, int P>
static int change_segments_impl(const void *const planes[], int64_t ny, int64_t nx, int64_t k, int64_t sy, int64_t sx,
                                int64_t st, const uint8_t *change, int8_t *direction, void *const means[],
                                hipStream_t stream)
{
    SegArgs<T, P> g;
    for (int p = 0; p < P; ++p) {
        g.pl[p] = static_cast<const T *>(planes[p]);
        g.mn[p] = means ? static_cast<T *>(means[p]) : nullptr;
    }
    g.change = change;
    g.direction = direction;
    RowWalk rw;
    if (const int rc = row_walk("nd_amd_change_segments", ny, nx, sy, sx, false, kCsThreads, &rw)) return rc;
    g.nx = rw.nx;
    g.sy = sy;
    g.sx = sx;
    g.st = st;
    g.k = k;
    g.blocks_per_row = rw.blocks_per_row;
    const dim3 grid((unsigned)rw.nblocks()), block(kCsThreads);
    KernelTimer timer(ND_AMD_KERNEL_CHANGE_SEGMENTS, stream);
    pick(direction != nullptr, [&](auto D) {
        pick(means != nullptr, [&](auto M) {
            // (the entry point admits no call that asks for neither)
            if constexpr (decltype(D)::value || decltype(M)::value)
                hipLaunchKernelGGL((change_segments_kernel<T, P, decltype(D)::value, decltype(M)::value>), grid,
                                   block, 0, stream, g);
        });
    });
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

}  // namespace nd_amd

using namespace nd_amd;

extern "C" int nd_amd_change_segments(const void *const planes[], int nplanes, int structure, int dtype, int64_t ny,
                                      int64_t nx, int64_t k, int64_t stride_y, int64_t stride_x, int64_t stride_t,
                                      const uint8_t *change, int8_t *direction, void *const means[], void *hip_stream)
{
    constexpr const char *entry = "nd_amd_change_segments";
    if (const int rc = check_dtype(entry, dtype)) return rc;
    if (structure != ND_AMD_STRUCT_DIAG && structure != ND_AMD_STRUCT_C2 && structure != ND_AMD_STRUCT_C3) {
        set_error("nd_amd_change_segments: structure must be ND_AMD_STRUCT_DIAG, _C2 or _C3, got %d", structure);
        return ND_AMD_EINVAL;
    }
    if (structure == ND_AMD_STRUCT_DIAG ? (nplanes < 1 || nplanes > 3)
                                        : nplanes != (structure == ND_AMD_STRUCT_C2 ? 4 : 9)) {
        set_error("nd_amd_change_segments: %s, got %d",
                  structure == ND_AMD_STRUCT_DIAG ? "ND_AMD_STRUCT_DIAG takes one to three planes"
                  : structure == ND_AMD_STRUCT_C2 ? "ND_AMD_STRUCT_C2 takes four planes"
                                                  : "ND_AMD_STRUCT_C3 takes nine planes",
                  nplanes);
        return ND_AMD_EINVAL;
    }
    bool empty;
    if (const int rc = check_shape(entry, ny, nx, k, &empty)) return rc;
    if (!direction && !means) {
        set_error("nd_amd_change_segments: neither direction nor means is asked for");
        return ND_AMD_EINVAL;
    }
    if (empty) return ND_AMD_OK;
    if (const int rc = check_planes(entry, planes, nplanes, change)) return rc;
    for (int p = 0; means && p < nplanes; ++p)
        if (!means[p]) {
            set_error("nd_amd_change_segments: means plane %d is null", p);
            return ND_AMD_EINVAL;
        }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int rc = ND_AMD_EINVAL;
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        auto run = [&](auto P) {
            rc = change_segments_impl<T, decltype(P)::value>(planes, ny, nx, k, stride_y, stride_x, stride_t,
                                                             change, direction, means, stream);
        };
        if (!pick_eq<1, 2, 3, 4>(nplanes, run)) run(int_c<9>{});     // (nine planes: C3, checked above)
    });
    return rc;
}
