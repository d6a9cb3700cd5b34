// nd_amd/csrc/omnibus_diag.hip -- OmnibusTest for intensity-only stacks (pol = 'diag') on gfx950.
//
// EXTENSION: the block-diagonal case of Conradsen et al.'s omnibus test -- q independent 1 x 1 blocks,
// q = 1, 2 or 3 real intensity channels (Sentinel-1 GRD: VV, VH; a single-channel stack: one plane).
// The algorithm is the reference's (nd/_change.pyx:46-77, 133-151, 224-257) with p replaced by q and the
// determinant of a date by the product of its intensities, in the arithmetic of the generic-p oracle
// (oracle/nd_oracle_impl.h:150-200), T the data type:
//   det_i = x_1i * x_2i * ...            left to right in T           (q = 1: x_1i itself)
//   prod  = prod * (double)det_i          in double, in time order
//   s_c   = s_c + x_ci                    in T, in time order
//   dets  = s_1 * s_2 * ...               left to right in T
//   logQ  = n ((T(q) T(j)) ln j + ln prod - j ln dets)                  in double
//   z     = T((-2 T(rho)) logQ),  P = T(P1 + omega2 T(T(P2) - T(P1))),  change where P > alpha
//   f = q (j - 1),  rho = host_rho(1, j, n),  omega2 = q host_omega2(1, j, n, rho) < 0
// (additivity of Box's expansion over independent blocks).  n is a double: equivalent numbers of looks
// of detected products are not integers.
//
// Regime -> kernel:
//   alpha <  0.75 and k q sizeof(T) <= 192 B (k >= 2):  omnibus_diag_fused_kernel, ONE launch.  A lane stages
//       its pixel's series in LDS once (a column of a wave-private image: no barrier, no bank conflict at any
//       per-lane date) and runs the exact search from there; the wave's rows of the map leave as 16-byte pieces.
//       192 B per pixel = 48 KB per block of 256 pixels plus the table: three blocks per CU.
//   everything else:  pass A (omnibus_diag_global_kernel) streams the planes once, decides the whole-series
//       test per pixel by zlo / zhi or exactly in between, zero-fills the map and lists the pixels that fire;
//       pass B (omnibus_diag_search_kernel) searches the listed pixels exactly, one lane per pixel, reading
//       the series from the planes -- any k.
// Every form evaluates a test the same way (diag_fires): the f32-log2 screen against zlo_a / zhi_a, and in
// between the exact statistic and, inside [zlo, zhi], the chi-square pair.
#include "dispatch.hpp"
#include "omnibus_common.hpp"
#include "omnibus_search.hpp"

namespace nd_amd {

constexpr int kDgThreads = 256;
constexpr int kDgShards = 128;
constexpr int kDgCounterStride = 32;
constexpr int kDgChunk = 8;          // dates per load chunk in pass A and in the staging of the fused form
constexpr int kDgFusedBytes = 192;   // bytes of series per pixel up to which the one-launch form is used
constexpr double kDgFusedAlpha = 0.75;
constexpr size_t kDgCounterBytes = (size_t)kDgShards * kDgCounterStride * sizeof(uint32_t);

// (the running state DiagAccum<T, Q>, z_stat / z_approx over it and the table views: omnibus_search.hpp)

// P of the test whose statistic is z.  chisq_pair's upper form sums Q(a, x) = t_{a-1} (1 + (a-1)/x + ...) over
// the factors >= 1 and starts that sum at 1 -- right for every a >= 1, but at a = 1/2 (f = 1: one channel, two
// dates) Q(1/2, x) is erfc(sqrt x) alone.  The dual- and full-pol tests never meet f = 1 (f = 4 (j - 1),
// 9 (j - 1)), so the shared routine stays as it is and that one case is finished here.
template <typename T>
__device__ __forceinline__ T diag_P(const T z, const int a2, const OmniTabEntry &e)
{
    double zd[1] = {(double)z}, P1[1], P2[1];
    chisq_pair<1>(zd, a2, e.lgam, P1, P2);
    if (a2 == 1 && zd[0] >= 3.0 && zd[0] < INFINITY) {      // x >= a + 1
        const double x = 0.5 * zd[0];
        const double ta = exp(fma(0.5, log(x), -x) - e.lgam);
        const double qa = erfc(sqrt(x));
        P1[0] = 1.0 - qa;
        P2[0] = 1.0 - (qa + ta + ta * (x * inv_half(3)));
    }
    return combine_P<T>(P1[0], P2[0], e.omega2);
}

// exact_verdict (omnibus_common.hpp) with diag_P behind it
template <typename T>
__device__ __forceinline__ bool diag_verdict(const T z, const int a2, const OmniTabEntry &e, const double alpha)
{
    const double zd = (double)z;
    int verdict = !(zd >= e.zlo) ? 0 : ((zd > e.zhi && zd < INFINITY) ? 1 : 2);
    if (verdict == 2) verdict = ((double)diag_P<T>(z, a2, e) > alpha) ? 1 : 0;
    return verdict == 1;
}

// Does the test over the jj dates folded into A fire?  The screen first: z_approx is within aerr of the exact
// double statistic (make_entry, omnibus_tables.hip), NaN or infinite exactly when that is; only between zlo_a and zhi_a the
// exact statistic is formed and decided by zlo / zhi or the chi-square pair.  (test_f64 of omnibus_search.hpp with
// this family's own exact tail: diag_verdict for f = 1, the view's own copy of the full entry, and no wave-uniform
// branch in front of it.)
template <typename T, int Q, typename Tab>
__device__ __forceinline__ bool diag_fires(const DiagAccum<T, Q> &A, const int jj, const double nlooks,
                                           const double alpha, const Tab &tab)
{
    const double za = z_approx(A, jj, nlooks, tab.m2rho(jj), tab.pklogk(jj));
    bool fires = (za > tab.zhi_a(jj)) && (za < INFINITY);
    const bool inband = (za >= tab.zlo_a(jj)) && !fires;
    if (inband) {
        const OmniTabEntry e = tab.entry(jj);
        fires = diag_verdict<T>(z_stat(A, jj, nlooks, e.m2rho, e.pklogk), DiagAccum<T, Q>::kDof * (jj - 1), e, alpha);
    }
    return fires;
}

// The sequential search of nd/_change.pyx:224-257 for one pixel, one sweep per segment: the dates of ts[l:]
// are folded once in time order; every prefix of j >= 2 dates is the marginal test over j dates (asked until
// the first one fires), the whole of it the global test of the segment (:241-242) -- which is also its last
// marginal test, so r = (k - l) - 1 where no shorter one fires.  fetch(t, v): the pixel's values of date t;
// fire(t): a change at date t (:252).
template <typename T, int Q, typename Tab, typename Fetch, typename Fire>
__device__ __forceinline__ void diag_search(const int k, const bool active, const double nlooks, const double alpha,
                                            const Tab &tab, Fetch fetch, Fire fire)
{
    // (spelled out, not through Sweep of omnibus_search.hpp: with it the fused and the search kernels spill one or
    //  two scalar registers more -- profiles/omnibus_search_codeobj.txt)
    int l = 0;
    bool done = !active || k < 2;
    while (!done) {
        DiagAccum<T, Q> A;
        A.reset();
        int fire_at = -1;
        bool gfires = false;
        for (int t0 = l; t0 < k; t0 += 4) {
            T v[4][Q];
#pragma unroll
            for (int u = 0; u < 4; ++u) fetch(t0 + u < k ? t0 + u : k - 1, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + u;
                if (t < k) {
                    A.step(v[u]);
                    const int jj = t - l + 1;
                    const bool last = (t == k - 1);
                    if (jj >= 2 && (fire_at < 0 || last)) {
                        const bool f = diag_fires<T, Q>(A, jj, nlooks, alpha, tab);
                        if (f && fire_at < 0) fire_at = t;
                        if (last) gfires = f;
                    }
                }
            }
        }
        if (gfires) {
            fire(fire_at);                    // :252
            l = fire_at;                      // :255
            if (l >= k - 1) done = true;      // :256
        } else {
            done = true;                      // :241-242
        }
    }
}

template <typename T>
struct DiagArgs {
    const T *pl[3];
    int64_t nx, nrows, sy, sx, st, blocks_per_row;
    int64_t nx_orig;          // pixels per row of the raster (list entries are y * nx_orig + x)
    int k, write_tab;
    double nlooks, alpha;
    OmniTabEntry e;           // the whole-series test's constants
    uint8_t *change;
    T *z_out, *p_out;
    uint32_t *flag_count, *flag_idx;
    uint32_t seg;
    OmniTabEntry *tab_dev;
};

// ---- pass A: the whole-series test, streamed -----------------------------------------------------------
template <typename T, int Q, bool STATS>
__global__ void __launch_bounds__(kDgThreads) omnibus_diag_global_kernel(const DiagArgs<T> g, const OmniTab tab)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t b = blockIdx.x;
    const int64_t row = b / g.blocks_per_row;
    const int64_t bx = b - row * g.blocks_per_row;
    const int64_t bpx0 = bx * (int64_t)kDgThreads;
    const int64_t x0 = bpx0 + tid;
    const int k = g.k;
    const bool in = x0 < g.nx;

    if (g.write_tab && b == 0)
        for (int j = tid; j <= k; j += kDgThreads) g.tab_dev[j] = tab.e[j];

    DiagAccum<T, Q> A;
    A.reset();
    {
        const int64_t xc = in ? x0 : g.nx - 1;                // idle lanes re-read the last pixel
        const int64_t off0 = row * g.sy + xc * g.sx;
        for (int t0 = 0; t0 < k; t0 += kDgChunk) {
            T v[kDgChunk][Q];
#pragma unroll
            for (int tt = 0; tt < kDgChunk; ++tt) {
                const int t = t0 + tt < k ? t0 + tt : k - 1;
                const int64_t off = off0 + (int64_t)t * g.st;
#pragma unroll
                for (int c = 0; c < Q; ++c) v[tt][c] = __builtin_nontemporal_load(g.pl[c] + off);
            }
#pragma unroll
            for (int tt = 0; tt < kDgChunk; ++tt)
                if (t0 + tt < k) A.step(v[tt]);
        }
    }

    bool flag;
    if (STATS) {
        const T z = z_stat(A, k, g.nlooks, g.e.m2rho, g.e.pklogk);
        const T P = diag_P<T>(z, Q * (k - 1), g.e);
        flag = in && ((double)P > g.alpha);
        if (in) {
            const int64_t pix = row * g.nx + x0;
            if (g.z_out) g.z_out[pix] = z;
            if (g.p_out) g.p_out[pix] = P;
        }
    } else {
        const TabOne one{g.e};
        flag = in && diag_fires<T, Q>(A, k, g.nlooks, g.alpha, one);
    }
    flag = flag && k >= 2;                                    // a single date has no change to place

    const unsigned shard = (unsigned)(b % kDgShards);
    if (__any(flag)) {
        const unsigned slot = wave_claim(flag, g.flag_count + shard * kDgCounterStride, lane);
        if (flag) g.flag_idx[(size_t)shard * g.seg + slot] = (uint32_t)(row * g.nx + x0);
    }

    // zero-fill this block's slice of the change map (np.zeros, nd/_change.pyx:275; issued last, never waited on)
    {
        const int64_t left = g.nx - bpx0;
        const int npx = left > kDgThreads ? kDgThreads : (int)left;
        zero_fill_span<kDgThreads, int64_t>(g.change + (row * g.nx + bpx0) * (int64_t)k, (int64_t)npx * k, tid);
    }
}

// ---- pass B: the exact search over the listed pixels, any k ----------------------------------------------
template <typename T, int Q>
__global__ void __launch_bounds__(64) omnibus_diag_search_kernel(const DiagArgs<T> s)
{
    const int lane = threadIdx.x;
    const int k = s.k;
    const unsigned shard = blockIdx.x % kDgShards;
    const unsigned lblock = blockIdx.x / kDgShards, nlblock = gridDim.x / kDgShards;
    const uint32_t n = s.flag_count[shard * kDgCounterStride];
    const uint32_t *list = s.flag_idx + (size_t)shard * s.seg;
    const TabGlobal tab{s.tab_dev};
    for (uint32_t base = lblock * 64u; base < n; base += nlblock * 64u) {
        const uint32_t idx = base + (uint32_t)lane;
        const bool active = idx < n;
        const int64_t pix = active ? (int64_t)list[idx] : 0;
        const int64_t row = pix / s.nx_orig, col = pix - row * s.nx_orig;
        const int64_t off = row * s.sy + col * s.sx;
        uint8_t *res = s.change + pix * (int64_t)k;           // the row was zero-filled by pass A
        diag_search<T, Q>(
            k, active, s.nlooks, s.alpha, tab,
            [&](const int t, T(&v)[Q]) {
#pragma unroll
                for (int c = 0; c < Q; ++c) v[c] = s.pl[c][off + (int64_t)t * s.st];
            },
            [&](const int t) { res[t] = 1; });
    }
}

// ---- the one-launch form for short series ----------------------------------------------------------------
// LDS: [table: 8 (k + 1) doubles][per wave: k Q rows of 64 values, value (t, c) of the lane's pixel at
// ((t Q + c) 64 + lane)].  A lane reads only what it wrote, so the image needs no barrier; the one barrier is
// for the table.  k <= 48 (float32) / 24 (float64) dates: the changes of a pixel are bits of one 64-bit word.
template <typename T, int Q, bool STATS>
__global__ void __launch_bounds__(kDgThreads) omnibus_diag_fused_kernel(const DiagArgs<T> g, const OmniTab tab)
{
    extern __shared__ __align__(16) unsigned char nd_smem_diag[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int k = g.k, kp = k + 1;
    double *tl = reinterpret_cast<double *>(nd_smem_diag);
    T *ser = reinterpret_cast<T *>(nd_smem_diag + (size_t)kp * sizeof(OmniTabEntry)) + (size_t)(tid >> 6) * (k * Q * 64);
    const int64_t b = blockIdx.x;
    const int64_t row = b / g.blocks_per_row;
    const int64_t bx = b - row * g.blocks_per_row;
    const int64_t bpx0 = bx * (int64_t)kDgThreads;
    const int64_t x0 = bpx0 + tid;
    const bool in = x0 < g.nx;

    // the table into LDS: entry j (wave-uniform: scalar loads from the argument segment) by wave j mod 4, its
    // eight fields by the wave's first eight lanes
    {
        const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll 1
        for (int j = w; j <= k; j += kDgThreads / 64) {
            const OmniTabEntry e = tab.e[j];
            const double f = lane == 0 ? e.m2rho : lane == 1 ? e.pklogk : lane == 2 ? e.omega2 : lane == 3 ? e.lgam
                           : lane == 4 ? e.zlo : lane == 5 ? e.zlo_a : lane == 6 ? e.zhi : e.zhi_a;
            if (lane < 8) tl[lane * kp + j] = f;
        }
    }
    {
        const int64_t xc = in ? x0 : g.nx - 1;                // idle lanes re-read the last pixel
        const int64_t off0 = row * g.sy + xc * g.sx;
        for (int t0 = 0; t0 < k; t0 += kDgChunk) {
            T v[kDgChunk][Q];
#pragma unroll
            for (int tt = 0; tt < kDgChunk; ++tt) {
                const int t = t0 + tt < k ? t0 + tt : k - 1;
                const int64_t off = off0 + (int64_t)t * g.st;
#pragma unroll
                for (int c = 0; c < Q; ++c) v[tt][c] = __builtin_nontemporal_load(g.pl[c] + off);
            }
#pragma unroll
            for (int tt = 0; tt < kDgChunk; ++tt)
                if (t0 + tt < k) {
#pragma unroll
                    for (int c = 0; c < Q; ++c) ser[((t0 + tt) * Q + c) * 64 + lane] = v[tt][c];
                }
        }
    }
    __syncthreads();
    const TabLds tv{tl, kp};
    auto fetch = [&](const int t, T(&v)[Q]) {
#pragma unroll
        for (int c = 0; c < Q; ++c) v[c] = ser[(t * Q + c) * 64 + lane];
    };
    if (STATS) {
        DiagAccum<T, Q> A;
        A.reset();
        for (int t = 0; t < k; ++t) {
            T v[Q];
            fetch(t, v);
            A.step(v);
        }
        const T z = z_stat(A, k, g.nlooks, g.e.m2rho, g.e.pklogk);
        const T P = diag_P<T>(z, Q * (k - 1), g.e);
        if (in) {
            const int64_t pix = row * g.nx + x0;
            if (g.z_out) g.z_out[pix] = z;
            if (g.p_out) g.p_out[pix] = P;
        }
    }
    unsigned long long mask = 0ull;
    diag_search<T, Q>(k, in, g.nlooks, g.alpha, tv, fetch, [&](const int t) { mask |= 1ull << t; });

    // the wave's rows of the map: 64 k contiguous bytes, through the wave's own image (every lane of the wave
    // is through with its series here: LDS operations of a wave complete in order)
    const int64_t wpx0 = bpx0 + (tid & ~63);
    const int64_t wleft = g.nx - wpx0;
    const int wnp = wleft > 64 ? 64 : (wleft > 0 ? (int)wleft : 0);
    uint8_t *wob = g.change + (row * g.nx + wpx0) * (int64_t)k;
    wave_lds_fence();
    if (change_rows_wave_ok(wob, k, wnp)) {
        store_change_rows_wave(wob, reinterpret_cast<uint32_t *>(ser), k, mask, lane);
    } else if (in) {
        uint8_t *res = wob + (int64_t)lane * k;
        for (int t = 0; t < k; ++t) res[t] = (uint8_t)((mask >> t) & 1ull);
    }
}

// =========================================================================================
// host side
// =========================================================================================
// workspace: [counters][per-j table][pixel lists: kDgShards x seg x u32]
struct DiagWorkspace {
    size_t off_count, off_tab, off_idx, total;
    uint32_t seg;
};
static DiagWorkspace diag_layout(int64_t npix, int64_t ny, int64_t k)
{
    DiagWorkspace w;
    // (a row may end inside a block: at most ceil(npix / 256) + ny blocks of <= 256 entries)
    const int64_t nb = ceil_div(npix, kDgThreads) + ny;
    w.seg = (uint32_t)((ceil_div(nb, kDgShards) + 1) * kDgThreads);
    w.off_count = 0;
    w.off_tab = align256(kDgCounterBytes);
    w.off_idx = w.off_tab + align256((size_t)(k + 1) * sizeof(OmniTabEntry));
    w.total = w.off_idx + align256((size_t)w.seg * kDgShards * sizeof(uint32_t));
    return w;
}

template <typename T, int Q>
static int omnibus_diag_impl(const void *const planes[], int64_t ny, int64_t nx, int64_t k, int64_t sy, int64_t sx,
                             int64_t st, double n_looks, double alpha, uint8_t *change, void *z_out, void *p_out,
                             void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const int64_t npix = ny * nx;
    const DiagWorkspace w = diag_layout(npix, ny, k);
    if (const int rc = check_workspace("nd_amd_omnibus_diag", workspace, workspace_bytes, w.total)) return rc;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const std::vector<OmniTabEntry> htab = get_table((int)k, n_looks, alpha, dtype_of<T>(), OmniFamily{1, Q});
    OmniTab tab;
    OmniTabEntry *tab_dev = reinterpret_cast<OmniTabEntry *>(ws + w.off_tab);
    bool tab_in_args;
    ND_HIP_CHECK(stage_table(htab, k, &tab, tab_dev, stream, &tab_in_args));

    DiagArgs<T> g;
    for (int c = 0; c < 3; ++c) g.pl[c] = static_cast<const T *>(planes[c < Q ? c : 0]);
    RowWalk rw;
    if (const int rc = row_walk("nd_amd_omnibus_diag", ny, nx, sy, sx, false, kDgThreads, &rw)) return rc;
    g.nx = rw.nx;
    g.nrows = rw.nrows;
    g.nx_orig = nx;
    g.sy = sy;
    g.sx = sx;
    g.st = st;
    g.blocks_per_row = rw.blocks_per_row;
    g.k = (int)k;
    g.write_tab = tab_in_args ? 1 : 0;
    g.nlooks = n_looks;
    g.alpha = alpha;
    g.e = htab[(size_t)k];
    g.change = change;
    g.z_out = static_cast<T *>(z_out);
    g.p_out = static_cast<T *>(p_out);
    g.flag_count = reinterpret_cast<uint32_t *>(ws + w.off_count);
    g.tab_dev = tab_dev;
    g.flag_idx = reinterpret_cast<uint32_t *>(ws + w.off_idx);
    g.seg = w.seg;
    const bool stats = z_out != nullptr || p_out != nullptr;
    const dim3 grid((unsigned)rw.nblocks()), block(kDgThreads);

    // (The launches are timed under the dual-pol test's timer ids -- OMNIBUS_FUSED, _GLOBAL, _SEARCH, reported as
    //  omnibus_c2_* -- as the full-pol unit does: the ids name the role of a launch in an omnibus call, and one call
    //  runs one family.)
    // low thresholds fire on nearly every pixel: the search runs inside the one launch where the series fit
    const bool fused = k >= 2 && k * Q * (int64_t)sizeof(T) <= kDgFusedBytes && alpha < kDgFusedAlpha;
    if (fused) {
        const size_t lds = (size_t)(k + 1) * sizeof(OmniTabEntry) + (size_t)k * Q * kDgThreads * sizeof(T);
        KernelTimer timer(ND_AMD_KERNEL_OMNIBUS_FUSED, stream);
        pick(stats, [&](auto S) {
            hipLaunchKernelGGL((omnibus_diag_fused_kernel<T, Q, decltype(S)::value>), grid, block, lds, stream, g, tab);
        });
        ND_HIP_CHECK(hipGetLastError());
        return ND_AMD_OK;
    }

    ND_HIP_CHECK(hipMemsetAsync(g.flag_count, 0, kDgCounterBytes, stream));
    {
        KernelTimer timer(ND_AMD_KERNEL_OMNIBUS_GLOBAL, stream);
        pick(stats, [&](auto S) {
            hipLaunchKernelGGL((omnibus_diag_global_kernel<T, Q, decltype(S)::value>), grid, block, 0, stream, g, tab);
        });
        ND_HIP_CHECK(hipGetLastError());
    }
    if (k >= 2) {
        const int64_t per_shard = shard_blocks(npix, kDgShards, 64, 64);
        KernelTimer timer(ND_AMD_KERNEL_OMNIBUS_SEARCH, stream);
        hipLaunchKernelGGL((omnibus_diag_search_kernel<T, Q>), dim3((unsigned)(per_shard * kDgShards)), dim3(64), 0,
                           stream, g);
        ND_HIP_CHECK(hipGetLastError());
    }
    return ND_AMD_OK;
}

}  // namespace nd_amd

using namespace nd_amd;

extern "C" size_t nd_amd_omnibus_diag_workspace_bytes(int dtype, int nch, int64_t ny, int64_t nx, int64_t k)
{
    if ((dtype != ND_AMD_F32 && dtype != ND_AMD_F64) || nch < 1 || nch > 3 || ny < 0 || nx < 0 || k < 0) return 0;
    return diag_layout(ny * nx, ny, k).total;
}

extern "C" int nd_amd_omnibus_diag(const void *const planes[], int nch, int dtype, int64_t ny, int64_t nx, int64_t k,
                                   int64_t stride_y, int64_t stride_x, int64_t stride_t, double n_looks, double alpha,
                                   uint8_t *change, void *z_out, void *p_out, void *workspace, size_t workspace_bytes,
                                   void *hip_stream)
{
    constexpr const char *entry = "nd_amd_omnibus_diag";
    if (const int rc = check_dtype(entry, dtype)) return rc;
    if (nch < 1 || nch > 3) {
        set_error("nd_amd_omnibus_diag: one to three intensity channels, got %d", nch);
        return ND_AMD_EINVAL;
    }
    bool empty;
    if (const int rc = check_shape(entry, ny, nx, k, &empty)) return rc;
    if (!(n_looks > 0.0) || !(n_looks < INFINITY)) {
        set_error("nd_amd_omnibus_diag: n_looks must be positive and finite, got %g", n_looks);
        return ND_AMD_EINVAL;
    }
    if (empty) return ND_AMD_OK;
    if (const int rc = check_planes(entry, planes, nch, change)) return rc;
    if (const int rc = check_pixel_index(entry, ny, nx)) return rc;
    if (k > 0x7fffffffLL / 3) {
        set_error("nd_amd_omnibus_diag: k = %lld exceeds the supported number of dates", (long long)k);
        return ND_AMD_EUNSUPPORTED;
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int rc = ND_AMD_EINVAL;
    pick(dtype == ND_AMD_F64, [&](auto F64) {
        using T = std::conditional_t<decltype(F64)::value, double, float>;
        pick_eq<1, 2, 3>(nch, [&](auto Q) {
            rc = omnibus_diag_impl<T, decltype(Q)::value>(planes, ny, nx, k, stride_y, stride_x, stride_t, n_looks,
                                                          alpha, change, z_out, p_out, workspace, workspace_bytes,
                                                          stream);
        });
    });
    return rc;
}
