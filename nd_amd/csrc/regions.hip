// nd_amd/csrc/regions.hip -- connected regions of per-pixel maps.  include/nd_amd.h has the definition ("Regions of
// a map"), which scipy.ndimage.label pins: labels number the regions in raster order of their first pixel.
//
//   nd_amd_label_regions    labels, an optional area plane and the number of regions of every plane
//   nd_amd_region_sizes     the pixel count of every label, from a labelling
//   nd_amd_sieve_regions    the map with the regions below a minimum size replaced
//
// A union-find over the raster.  A pixel's parent is the in-plane index i * nx + j of another pixel of its region, never
// a larger one than its own, so a region's root is its smallest index: its first pixel in raster order.  That makes
// the result independent of the order in which the links are made.
//
//   local     a block of 4 waves labels a tile of 32 x 64 pixels in LDS: a wave takes a row, one ballot gives every
//             pixel the start of its run along x, and the links to the row above are made with the lock-free atomicMin
//             union on the LDS parents (a link that the lane to the left makes as well is left to it).  The tile's
//             parents go to the int32 parent plane as in-plane indices.
//   seam      one lane per pixel below or right of a tile edge: the same union on the parent plane across the edge
//   flatten   every pixel's parent becomes its root; the roots of every 1024 pixels are counted, and with a size
//             plane every pixel adds 1 at its root (integer atomicAdd; lanes of a wave that share a root add once, and
//             so do the waves of a block that each hold one root)
//   scan      one block per plane turns the block counts into exclusive prefix counts: the numbering
//   number    a root's parent becomes -(rank + 1)
//   write     labels and area, or the sieved map, with the caller's strides
//
// Every pass is a launch of its own, and no block waits for another.  Every loop is bounded: a find walks strictly
// downwards, so it ends within `n` steps among n pixels; a union that fails continues with a strictly smaller pair,
// so it ends within 2 n rounds.  A loop that reaches its bound, or an index that leaves the plane, sets the give-up
// word, which the entry reads back: ND_AMD_EINTERNAL.
// Strides are arbitrary (in elements): crops and (y, x, time) maps are read and written where they lie; only the
// local pass reads the map (the seam pass again where by_value compares values), only the write pass writes.
#include <limits.h>
#include <string.h>

#include <type_traits>

#include "common.hpp"
#include "dispatch.hpp"

using namespace nd_amd;

namespace {

constexpr int RG_TX = 64;                           // a tile: one wave along x
constexpr int RG_TY = 32;
constexpr int RG_WAVES = 4;
constexpr int RG_TILE = RG_TX * RG_TY;
constexpr int RG_SCAN = 1024;                       // pixels of a block of the flatten / number passes
constexpr int RG_PX = 256;                          // pixels of a block of the seam / write passes
constexpr int32_t RG_BG = INT_MIN;                  // the parent of a background pixel
constexpr int64_t RG_MAX_BLOCKS = ((int64_t)1 << 31) - 1;

struct RgArgs {
    const void *src;
    int64_t ssp, ssy, ssx;                          // strides in elements: plane, y, x
    int32_t *parent;                                // (nplanes, ny * nx)
    int32_t *cnt;                                   // the same, pixels per root; null where no sizes are asked for
    int32_t *giveup;
    int64_t nplanes, ny, nx, npix;
    uint32_t tiles_x, tiles_y;
    uint64_t bg;                                    // the background element's bytes
};

template <class T>
__device__ __forceinline__ T rg_value(uint64_t bits)
{
    T v;
    __builtin_memcpy(&v, &bits, sizeof(T));
    return v;
}

template <class T>
__device__ __forceinline__ bool rg_fg(T v, T bg)
{
    return v != bg && v == v;
}

// the root of x among n pixels, -1 (and the give-up word) where the walk leaves the plane or does not end
__device__ __forceinline__ int32_t rg_find(int32_t *L, int32_t x, int64_t n, int32_t *giveup)
{
    if ((uint32_t)x < (uint64_t)n)
        for (int64_t it = 0; it <= n; ++it) {
            const int32_t p = __atomic_load_n(L + x, __ATOMIC_RELAXED);
            if (p == x) return x;
            if (p < 0 || p > x) break;
            x = p;
        }
    *giveup = 1;
    return -1;
}

__device__ __forceinline__ void rg_union(int32_t *L, int32_t a, int32_t b, int64_t n, int32_t *giveup)
{
    for (int64_t it = 0; it < 2 * n + 2; ++it) {
        a = rg_find(L, a, n, giveup);
        b = rg_find(L, b, n, giveup);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;                                    // a had a parent by then, old < a: go on from there
    }
    *giveup = 1;
}

// ---- local: a tile labelled in LDS
template <class T, int CONN, bool BYV>
__global__ __launch_bounds__(RG_TX * RG_WAVES) void regions_local_kernel(RgArgs a)
{
    using K = std::conditional_t<BYV, T, uint8_t>;  // what two pixels are compared by: the value, or foreground
    __shared__ K key[RG_TILE];
    __shared__ int32_t par[RG_TILE];
    const int lane = threadIdx.x, wave = threadIdx.y;
    const uint32_t b = blockIdx.x;
    const uint32_t bx = b % a.tiles_x, q = b / a.tiles_x;
    const int64_t x0 = (int64_t)bx * RG_TX, y0 = (int64_t)(q % a.tiles_y) * RG_TY;
    const int64_t plane = q / a.tiles_y;
    const T bg = rg_value<T>(a.bg);
    const K kbg = [&] { if constexpr (BYV) return bg; else return (uint8_t)0; }();
    const T *src = reinterpret_cast<const T *>(a.src) + plane * a.ssp;
    const int64_t x = x0 + lane;
    const bool col = x < a.nx;

    auto fg = [&](K k) { if constexpr (BYV) return rg_fg<T>(k, bg); else return k != 0; };
    auto joined = [&](K k, K other) {               // k is foreground
        if constexpr (BYV) return rg_fg<T>(other, bg) && k == other; else return other != 0;
    };

    for (int r = wave; r < RG_TY; r += RG_WAVES) {
        const int64_t y = y0 + r;
        K k = kbg;
        if (col && y < a.ny) {
            const T v = src[y * a.ssy + x * a.ssx];
            if (rg_fg<T>(v, bg)) {
                if constexpr (BYV) k = v; else k = 1;
            }
        }
        key[r * RG_TX + lane] = k;
    }
    __syncthreads();
    // runs along x: a pixel's first parent is the start of its run
    for (int r = wave; r < RG_TY; r += RG_WAVES) {
        const int p = r * RG_TX + lane;
        const K k = key[p];
        const bool f = fg(k);
        const bool link = f && lane > 0 && joined(k, key[p - (lane > 0 ? 1 : 0)]);
        const uint64_t starts = ~__ballot(link);    // bit 0 is always set
        const uint64_t below = starts & ((2ull << lane) - 1ull);
        const int start = 63 - __clzll((long long)below);
        par[p] = f ? r * RG_TX + start : RG_BG;
    }
    __syncthreads();
    // links to the row above
    for (int r = wave; r < RG_TY; r += RG_WAVES) {
        if (r == 0) continue;                       // (wave-uniform)
        const int p = r * RG_TX + lane;
        const K k = key[p];
        const bool f = fg(k);
        const K up = key[p - RG_TX];
        const K left = key[p - (lane > 0 ? 1 : 0)], upleft = key[p - RG_TX - (lane > 0 ? 1 : 0)];
        const bool ju = f && joined(k, up);
        const bool jl = f && lane > 0 && joined(k, left);
        const uint64_t U = __ballot(ju);
        // the lane to the left links the same two runs
        const bool same = jl && ((U >> (lane > 0 ? lane - 1 : 0)) & 1ull) && fg(up) && joined(up, upleft);
        if (ju && !same) rg_union(par, p, p - RG_TX, RG_TILE, a.giveup);
        if constexpr (CONN == 8) {
            // a diagonal link adds nothing where the pixel is joined to the one above or beside it
            if (f && !ju) {
                if (lane > 0 && !jl && joined(k, upleft)) rg_union(par, p, p - RG_TX - 1, RG_TILE, a.giveup);
                if (lane < RG_TX - 1 && !joined(k, key[p + 1]) && joined(k, key[p - RG_TX + 1]))
                    rg_union(par, p, p - RG_TX + 1, RG_TILE, a.giveup);
            }
        }
    }
    __syncthreads();
    int32_t *parent = a.parent + plane * a.npix;
    int32_t *cnt = a.cnt ? a.cnt + plane * a.npix : nullptr;
    for (int r = wave; r < RG_TY; r += RG_WAVES) {
        const int64_t y = y0 + r;
        if (!col || y >= a.ny) continue;
        const int p = r * RG_TX + lane;
        int32_t g = RG_BG;
        if (par[p] != RG_BG) {
            const int32_t root = rg_find(par, p, RG_TILE, a.giveup);
            // (a failed find leaves the pixel a root of its own: in the plane, and the entry fails anyway)
            const int rr = root < 0 ? p : root;
            g = (int32_t)((y0 + rr / RG_TX) * a.nx + x0 + rr % RG_TX);
        }
        parent[y * a.nx + x] = g;
        if (cnt) cnt[y * a.nx + x] = 0;
    }
}

// ---- seam: the links across the tile edges, one lane per pixel below a horizontal or right of a vertical edge
template <class T, int CONN, bool BYV>
__global__ __launch_bounds__(RG_PX) void regions_seam_kernel(RgArgs a, int64_t row_items, int64_t items,
                                                             uint32_t blocks_per_plane)
{
    const int64_t plane = blockIdx.x / blocks_per_plane;
    const int64_t i = (int64_t)(blockIdx.x % blocks_per_plane) * RG_PX + threadIdx.x;
    if (i >= items) return;
    int32_t *L = a.parent + plane * a.npix;
    const T *src = reinterpret_cast<const T *>(a.src) + plane * a.ssp;
    auto link = [&](int64_t y, int64_t x, int64_t y2, int64_t x2) {
        const int32_t p = (int32_t)(y * a.nx + x), q = (int32_t)(y2 * a.nx + x2);
        if (L[p] == RG_BG || L[q] == RG_BG) return;
        if constexpr (BYV) {
            if (!(src[y * a.ssy + x * a.ssx] == src[y2 * a.ssy + x2 * a.ssx])) return;
        }
        rg_union(L, p, q, a.npix, a.giveup);
    };
    if (i < row_items) {
        const int64_t s = i / a.nx, x = i % a.nx, y = (s + 1) * RG_TY;
        link(y, x, y - 1, x);
        if constexpr (CONN == 8) {
            if (x > 0) link(y, x, y - 1, x - 1);
            if (x < a.nx - 1) link(y, x, y - 1, x + 1);
        }
    } else {
        const int64_t j = i - row_items;
        const int64_t s = j / a.ny, y = j % a.ny, x = (s + 1) * RG_TX;
        link(y, x, y, x - 1);
        if constexpr (CONN == 8) {
            if (y > 0) link(y, x, y - 1, x - 1);
            if (y < a.ny - 1) link(y, x, y + 1, x - 1);
        }
    }
}

// the sum of one value per wave over the block's 16 waves, and what the waves before this one hold
__device__ __forceinline__ int rg_block_offsets(int wave_total, int *lds, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                // the previous use of lds is over
    if (lane == 0) lds[wave] = wave_total;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RG_SCAN / 64; w++) {
        const int v = lds[w];
        before += w < wave ? v : 0;
        all += v;
    }
    *total = all;
    return before;
}

// `n` added at cnt[root] for the lanes with `on`; lanes that share a root add once
__device__ __forceinline__ void rg_count(int32_t *cnt, bool on, int32_t root)
{
    const int lane = threadIdx.x & 63;
    bool pending = on;
    for (int it = 0; it < 4; ++it) {
        const uint64_t m = __ballot(pending);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const int32_t r0 = __shfl(root, leader);
        const bool mine = pending && root == r0;
        const uint64_t g = __ballot(mine);
        if (lane == leader) atomicAdd(cnt + r0, __popcll(g));
        pending = pending && !mine;
    }
    if (pending) atomicAdd(cnt + root, 1);
}

// the same over a block of RG_SCAN lanes: a wave whose lanes all share one root hands its count to wave 0, which
// adds once per root among the 16 -- inside a large region one atomicAdd per 1024 pixels
__device__ __forceinline__ void rg_count_block(int32_t *cnt, bool on, int32_t root, int32_t *lds_root, int *lds_n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(on);
    int32_t r0 = -1;
    bool uniform = false;
    if (m) {
        r0 = __shfl(root, __ffsll((long long)m) - 1);
        uniform = __ballot(on && root != r0) == 0;
    }
    if (!uniform) rg_count(cnt, on, root);          // (wave-uniform)
    if (lane == 0) {
        lds_root[wave] = uniform ? r0 : -1;
        lds_n[wave] = uniform ? __popcll(m) : 0;
    }
    __syncthreads();
    if (wave != 0) return;
    const int32_t r = lane < RG_SCAN / 64 ? lds_root[lane] : -1;
    const int c = lane < RG_SCAN / 64 ? lds_n[lane] : 0;
    bool pending = r >= 0;
    for (int it = 0; it < RG_SCAN / 64; ++it) {     // every round serves its leader at least
        const uint64_t mm = __ballot(pending);
        if (!mm) break;
        const int leader = __ffsll((long long)mm) - 1;
        const int32_t rr = __shfl(r, leader);
        const bool mine = pending && r == rr;
        int s = mine ? c : 0;
#pragma unroll
        for (int d = RG_SCAN / 128; d > 0; d >>= 1) s += __shfl_xor(s, d);
        if (lane == leader) atomicAdd(cnt + rr, s);
        pending = pending && !mine;
    }
}

// ---- flatten: parent = root; roots per block; sizes per root
__global__ __launch_bounds__(RG_SCAN) void regions_flatten_kernel(RgArgs a, int32_t *blocksum, uint32_t blocks_per_plane)
{
    __shared__ int lds[RG_SCAN / 64];
    __shared__ int32_t lds_root[RG_SCAN / 64];
    __shared__ int lds_n[RG_SCAN / 64];
    const int64_t plane = blockIdx.x / blocks_per_plane;
    const int64_t i = (int64_t)(blockIdx.x % blocks_per_plane) * RG_SCAN + threadIdx.x;
    int32_t *L = a.parent + plane * a.npix;
    bool f = false;
    int32_t root = -1;
    if (i < a.npix && L[i] != RG_BG) {
        root = rg_find(L, (int32_t)i, a.npix, a.giveup);
        if (root >= 0) {
            f = true;
            if (root != (int32_t)i) __atomic_store_n(L + i, root, __ATOMIC_RELAXED);
        }
    }
    if (a.cnt) rg_count_block(a.cnt + plane * a.npix, f, root, lds_root, lds_n);
    if (blocksum) {
        int total;
        rg_block_offsets(__popcll(__ballot(f && root == (int32_t)i)), lds, &total);
        if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
    }
}

// ---- scan: a plane's block counts -> exclusive prefix counts, and the plane's number of regions
__global__ __launch_bounds__(RG_SCAN) void regions_scan_kernel(int32_t *blocksum, uint32_t blocks_per_plane,
                                                               int64_t *counts)
{
    __shared__ int lds[RG_SCAN / 64];
    const int lane = threadIdx.x & 63;
    int32_t *s = blocksum + (int64_t)blockIdx.x * blocks_per_plane;
    int carry = 0;
    for (uint32_t base = 0; base < blocks_per_plane; base += RG_SCAN) {
        const uint32_t i = base + threadIdx.x;
        const int v = i < blocks_per_plane ? s[i] : 0;
        int x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(x, d);
            if (lane >= d) x += t;
        }
        int total;
        const int before = rg_block_offsets(__shfl(x, 63), lds, &total);
        if (i < blocks_per_plane) s[i] = carry + before + x - v;
        carry += total;
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// ---- number: a root's parent becomes -(rank + 1)
__global__ __launch_bounds__(RG_SCAN) void regions_number_kernel(RgArgs a, const int32_t *blocksum,
                                                                 uint32_t blocks_per_plane)
{
    __shared__ int lds[RG_SCAN / 64];
    const int lane = threadIdx.x & 63;
    const int64_t plane = blockIdx.x / blocks_per_plane;
    const int64_t i = (int64_t)(blockIdx.x % blocks_per_plane) * RG_SCAN + threadIdx.x;
    int32_t *L = a.parent + plane * a.npix;
    const bool root = i < a.npix && L[i] == (int32_t)i;
    const uint64_t m = __ballot(root);
    int total;
    const int before = rg_block_offsets(__popcll(m), lds, &total);
    if (root) L[i] = -(blocksum[blockIdx.x] + before + __popcll(m & ((1ull << lane) - 1ull)) + 1);
}

struct RgOut {
    int32_t *labels, *area;
    int64_t lsp, lsy, lsx, asp, asy, asx;
};

// ---- write: labels and area
__global__ __launch_bounds__(RG_PX) void regions_write_kernel(RgArgs a, RgOut o, uint32_t blocks_per_plane)
{
    const int64_t plane = blockIdx.x / blocks_per_plane;
    const int64_t i = (int64_t)(blockIdx.x % blocks_per_plane) * RG_PX + threadIdx.x;
    if (i >= a.npix) return;
    const int32_t *L = a.parent + plane * a.npix;
    const int32_t v = L[i];
    int32_t label = 0, area = 0;
    if (v != RG_BG) {
        int64_t root = i;
        int32_t code = v;
        if (v >= 0) {
            root = v;
            code = v < a.npix ? L[v] : 0;
        }
        if (code < 0 && code != RG_BG) {
            label = -code;
            if (o.area) area = a.cnt[plane * a.npix + root];
        } else {
            *a.giveup = 1;
        }
    }
    const int64_t y = i / a.nx, x = i % a.nx;
    o.labels[plane * o.lsp + y * o.lsy + x * o.lsx] = label;
    if (o.area) o.area[plane * o.asp + y * o.asy + x * o.asx] = area;
}

// ---- write: the sieved map.  E is an unsigned type of the element's size: values are copied bit for bit
template <class E>
__global__ __launch_bounds__(RG_PX) void regions_sieve_kernel(RgArgs a, E *dst, int64_t dsp, int64_t dsy, int64_t dsx,
                                                              int64_t min_size, uint64_t fill, uint32_t blocks_per_plane)
{
    const int64_t plane = blockIdx.x / blocks_per_plane;
    const int64_t i = (int64_t)(blockIdx.x % blocks_per_plane) * RG_PX + threadIdx.x;
    if (i >= a.npix) return;
    const int64_t y = i / a.nx, x = i % a.nx;
    E val = reinterpret_cast<const E *>(a.src)[plane * a.ssp + y * a.ssy + x * a.ssx];
    if (a.parent) {                                 // null: min_size <= 1, a copy
        const int32_t v = a.parent[plane * a.npix + i];
        if (v != RG_BG) {
            if ((uint32_t)v < (uint64_t)a.npix) {
                if ((int64_t)a.cnt[plane * a.npix + v] < min_size) val = (E)fill;
            } else {
                *a.giveup = 1;
            }
        }
    }
    dst[plane * dsp + y * dsy + x * dsx] = val;
}

// ---- sizes[offsets[plane] + label - 1] += 1 over a labelling
__global__ __launch_bounds__(RG_PX) void regions_sizes_kernel(const int32_t *labels, int64_t lsp, int64_t lsy, int64_t lsx,
                                                              int64_t nx, int64_t npix, const int64_t *offsets,
                                                              int32_t *sizes, int64_t nsizes, uint32_t blocks_per_plane)
{
    const int64_t plane = blockIdx.x / blocks_per_plane;
    const int64_t i = (int64_t)(blockIdx.x % blocks_per_plane) * RG_PX + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int64_t slot = -1;
    if (i < npix) {
        const int32_t l = labels[plane * lsp + (i / nx) * lsy + (i % nx) * lsx];
        if (l > 0) {
            slot = offsets[plane] + l - 1;
            if (slot < 0 || slot >= nsizes) slot = -1;      // not a label of this labelling: counted nowhere
        }
    }
    bool pending = slot >= 0;
    for (int it = 0; it < 4; ++it) {
        const uint64_t m = __ballot(pending);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const int64_t s0 = __shfl(slot, leader);
        const bool mine = pending && slot == s0;
        const uint64_t g = __ballot(mine);
        if (lane == leader) atomicAdd(sizes + s0, __popcll(g));
        pending = pending && !mine;
    }
    if (pending) atomicAdd(sizes + slot, 1);
}

// ---- host
struct RgPlan {
    size_t parent_off, cnt_off, sums_off, bytes;
    int64_t scan_blocks;                            // per plane
};

RgPlan rg_plan(int64_t nplanes, int64_t ny, int64_t nx, bool sizes)
{
    RgPlan p;
    const size_t plane = align256((size_t)nplanes * (size_t)ny * (size_t)nx * sizeof(int32_t));
    p.scan_blocks = ceil_div(ny * nx, RG_SCAN);
    p.parent_off = align256(sizeof(int32_t));       // the give-up word comes first
    p.cnt_off = p.parent_off + plane;
    p.sums_off = p.cnt_off + (sizes ? plane : 0);
    p.bytes = p.sums_off + align256((size_t)nplanes * (size_t)p.scan_blocks * sizeof(int32_t));
    return p;
}

template <int D> struct rg_type;
template <> struct rg_type<ND_AMD_F32> { using type = float; };
template <> struct rg_type<ND_AMD_F64> { using type = double; };
template <> struct rg_type<ND_AMD_I64> { using type = int64_t; };
template <> struct rg_type<ND_AMD_I32> { using type = int32_t; };
template <> struct rg_type<ND_AMD_U8> { using type = uint8_t; };

// f(T, CONN, BYV)
template <class F>
void rg_pick(int dtype, int connectivity, bool by_value, F &&f)
{
    pick_eq<ND_AMD_F32, ND_AMD_F64, ND_AMD_I64, ND_AMD_I32, ND_AMD_U8>(dtype, [&](auto D) {
        using T = typename rg_type<decltype(D)::value>::type;
        pick_eq<4, 8>(connectivity, [&](auto CONN) { pick(by_value, [&](auto BYV) { f(T{}, CONN, BYV); }); });
    });
}

// what the three entries check alike, in this order; *empty: nothing to do
int rg_check(const char *fn, int dtype, int connectivity, int64_t nplanes, int64_t ny, int64_t nx, bool *empty)
{
    int rc = check_region_dtype(fn, dtype);
    if (rc == ND_AMD_OK) rc = check_connectivity(fn, connectivity);
    if (rc == ND_AMD_OK) rc = check_shape(fn, ny, nx, nplanes, empty);
    if (rc == ND_AMD_OK) rc = check_plane_pixels(fn, ny, nx);
    return rc;
}

int rg_blocks(const char *fn, int64_t per_plane, int64_t nplanes, unsigned *blocks)
{
    if (per_plane > RG_MAX_BLOCKS / nplanes) {
        set_error("%s: %lld x %lld blocks are more than one launch holds: label fewer planes per call", fn,
                  (long long)per_plane, (long long)nplanes);
        return ND_AMD_EUNSUPPORTED;
    }
    *blocks = (unsigned)(per_plane * nplanes);
    return ND_AMD_OK;
}

uint64_t rg_bits(const void *element, int dtype)
{
    uint64_t bits = 0;
    memcpy(&bits, element, (size_t)region_dtype_size(dtype));
    return bits;
}

// local, seam and flatten: the parent plane holds every pixel's root (and a.cnt the sizes) afterwards
int rg_label(const char *fn, RgArgs &a, int dtype, int connectivity, bool by_value, int32_t *blocksum,
             const RgPlan &plan, hipStream_t stream)
{
    const int64_t tx = ceil_div(a.nx, RG_TX), ty = ceil_div(a.ny, RG_TY);
    a.tiles_x = (uint32_t)tx;
    a.tiles_y = (uint32_t)ty;
    const int64_t row_items = (ty - 1) * a.nx, items = row_items + (tx - 1) * a.ny;
    unsigned local_blocks = 0, seam_blocks = 0, flat_blocks = 0;
    int rc = rg_blocks(fn, tx * ty, a.nplanes, &local_blocks);
    if (rc == ND_AMD_OK && items > 0) rc = rg_blocks(fn, ceil_div(items, RG_PX), a.nplanes, &seam_blocks);
    if (rc == ND_AMD_OK) rc = rg_blocks(fn, plan.scan_blocks, a.nplanes, &flat_blocks);
    if (rc != ND_AMD_OK) return rc;
    ND_HIP_CHECK(hipMemsetAsync(a.giveup, 0, sizeof(int32_t), stream));
    rg_pick(dtype, connectivity, by_value, [&](auto t, auto CONN, auto BYV) {
        using T = decltype(t);
        constexpr int C = decltype(CONN)::value;
        constexpr bool V = decltype(BYV)::value;
        using TS = std::conditional_t<V, T, uint8_t>;   // without by_value the seam pass never reads the map
        hipLaunchKernelGGL((regions_local_kernel<T, C, V>), dim3(local_blocks), dim3(RG_TX, RG_WAVES), 0, stream, a);
        if (seam_blocks)
            hipLaunchKernelGGL((regions_seam_kernel<TS, C, V>), dim3(seam_blocks), dim3(RG_PX), 0, stream, a,
                               row_items, items, (uint32_t)ceil_div(items, RG_PX));
    });
    ND_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(regions_flatten_kernel, dim3(flat_blocks), dim3(RG_SCAN), 0, stream, a, blocksum,
                       (uint32_t)plan.scan_blocks);
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

// the give-up word, read behind the call's launches: the one place where a region entry waits for the device
int rg_finish(const char *fn, const int32_t *giveup, hipStream_t stream)
{
    int32_t word = 0;
    ND_HIP_CHECK(hipMemcpyAsync(&word, giveup, sizeof(word), hipMemcpyDeviceToHost, stream));
    ND_HIP_CHECK(hipStreamSynchronize(stream));
    if (word == 0) return ND_AMD_OK;
    set_error("%s: a bounded loop of the union-find reached its bound; the outputs are not valid", fn);
    return ND_AMD_EINTERNAL;
}

int rg_workspace(const char *fn, const RgPlan &plan, const void *workspace, size_t workspace_bytes)
{
    if (workspace && workspace_bytes >= plan.bytes) return ND_AMD_OK;
    set_error("%s: needs a workspace of %zu bytes, got %zu", fn, plan.bytes, workspace ? workspace_bytes : (size_t)0);
    return ND_AMD_EWORKSPACE;
}

void rg_args(RgArgs &a, const void *src, const int64_t *ss, int64_t nplanes, int64_t ny, int64_t nx, void *workspace,
             const RgPlan &plan, bool sizes, uint64_t bg)
{
    unsigned char *w = reinterpret_cast<unsigned char *>(workspace);
    a.src = src;
    a.ssp = ss[0]; a.ssy = ss[1]; a.ssx = ss[2];
    a.giveup = reinterpret_cast<int32_t *>(w);
    a.parent = reinterpret_cast<int32_t *>(w + plan.parent_off);
    a.cnt = sizes ? reinterpret_cast<int32_t *>(w + plan.cnt_off) : nullptr;
    a.nplanes = nplanes; a.ny = ny; a.nx = nx; a.npix = ny * nx;
    a.tiles_x = a.tiles_y = 0;
    a.bg = bg;
}

}  // namespace

extern "C" size_t nd_amd_regions_workspace_bytes(int64_t nplanes, int64_t ny, int64_t nx, int with_sizes)
{
    if (nplanes <= 0 || ny <= 0 || nx <= 0 || check_plane_pixels("nd_amd_regions_workspace_bytes", ny, nx) != ND_AMD_OK)
        return 0;
    return rg_plan(nplanes, ny, nx, with_sizes != 0).bytes;
}

extern "C" int nd_amd_label_regions(const void *src, int dtype, int64_t nplanes, int64_t ny, int64_t nx,
                                    const int64_t *src_strides, int connectivity, int by_value,
                                    const void *background, int32_t *labels, const int64_t *label_strides,
                                    int32_t *area, const int64_t *area_strides, int64_t *counts, void *workspace,
                                    size_t workspace_bytes, void *hip_stream)
{
    const char *fn = "nd_amd_label_regions";
    bool empty = false;
    int rc = rg_check(fn, dtype, connectivity, nplanes, ny, nx, &empty);
    if (rc != ND_AMD_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    if (empty) {
        if (counts && nplanes > 0) ND_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)nplanes * sizeof(int64_t), stream));
        return ND_AMD_OK;
    }
    rc = check_strides(fn, "src_strides", src_strides);
    if (rc == ND_AMD_OK) rc = check_strides(fn, "label_strides", label_strides);
    if (rc == ND_AMD_OK && area) rc = check_strides(fn, "area_strides", area_strides);
    if (rc != ND_AMD_OK) return rc;
    if (!src || !labels || !counts || !background) {
        set_error("%s: src, labels, counts or background is null", fn);
        return ND_AMD_EINVAL;
    }
    const RgPlan plan = rg_plan(nplanes, ny, nx, area != nullptr);
    rc = rg_workspace(fn, plan, workspace, workspace_bytes);
    if (rc != ND_AMD_OK) return rc;
    RgArgs a;
    rg_args(a, src, src_strides, nplanes, ny, nx, workspace, plan, area != nullptr, rg_bits(background, dtype));
    int32_t *blocksum = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(workspace) + plan.sums_off);
    unsigned scan_blocks = 0, write_blocks = 0;
    rc = rg_blocks(fn, plan.scan_blocks, nplanes, &scan_blocks);
    if (rc == ND_AMD_OK) rc = rg_blocks(fn, ceil_div(a.npix, RG_PX), nplanes, &write_blocks);
    if (rc != ND_AMD_OK) return rc;

    KernelTimer timer(ND_AMD_KERNEL_REGIONS, stream);
    rc = rg_label(fn, a, dtype, connectivity, by_value != 0, blocksum, plan, stream);
    if (rc != ND_AMD_OK) return rc;
    hipLaunchKernelGGL(regions_scan_kernel, dim3((unsigned)nplanes), dim3(RG_SCAN), 0, stream, blocksum,
                       (uint32_t)plan.scan_blocks, counts);
    hipLaunchKernelGGL(regions_number_kernel, dim3(scan_blocks), dim3(RG_SCAN), 0, stream, a, blocksum,
                       (uint32_t)plan.scan_blocks);
    RgOut o;
    o.labels = labels;
    o.lsp = label_strides[0]; o.lsy = label_strides[1]; o.lsx = label_strides[2];
    o.area = area;
    o.asp = area ? area_strides[0] : 0; o.asy = area ? area_strides[1] : 0; o.asx = area ? area_strides[2] : 0;
    hipLaunchKernelGGL(regions_write_kernel, dim3(write_blocks), dim3(RG_PX), 0, stream, a, o,
                       (uint32_t)ceil_div(a.npix, RG_PX));
    ND_HIP_CHECK(hipGetLastError());
    return rg_finish(fn, a.giveup, stream);
}

extern "C" int nd_amd_region_sizes(const int32_t *labels, const int64_t *label_strides, int64_t nplanes, int64_t ny,
                                   int64_t nx, const int64_t *offsets, int32_t *sizes, int64_t nsizes,
                                   void *hip_stream)
{
    const char *fn = "nd_amd_region_sizes";
    bool empty = false;
    int rc = check_shape(fn, ny, nx, nplanes, &empty);
    if (rc == ND_AMD_OK) rc = check_plane_pixels(fn, ny, nx);
    if (rc != ND_AMD_OK) return rc;
    if (nsizes < 0) {
        set_error("%s: negative nsizes %lld", fn, (long long)nsizes);
        return ND_AMD_EINVAL;
    }
    if (nsizes == 0) return ND_AMD_OK;
    if (!sizes) {
        set_error("%s: sizes is null", fn);
        return ND_AMD_EINVAL;
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    if (empty) {
        ND_HIP_CHECK(hipMemsetAsync(sizes, 0, (size_t)nsizes * sizeof(int32_t), stream));
        return ND_AMD_OK;
    }
    rc = check_strides(fn, "label_strides", label_strides);
    if (rc != ND_AMD_OK) return rc;
    if (!labels || !offsets) {
        set_error("%s: labels or offsets is null", fn);
        return ND_AMD_EINVAL;
    }
    unsigned blocks = 0;
    const int64_t per_plane = ceil_div(ny * nx, RG_PX);
    rc = rg_blocks(fn, per_plane, nplanes, &blocks);
    if (rc != ND_AMD_OK) return rc;
    KernelTimer timer(ND_AMD_KERNEL_REGIONS, stream);
    ND_HIP_CHECK(hipMemsetAsync(sizes, 0, (size_t)nsizes * sizeof(int32_t), stream));
    hipLaunchKernelGGL(regions_sizes_kernel, dim3(blocks), dim3(RG_PX), 0, stream, labels, label_strides[0],
                       label_strides[1], label_strides[2], nx, ny * nx, offsets, sizes, nsizes, (uint32_t)per_plane);
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_sieve_regions(const void *src, void *dst, int dtype, int64_t nplanes, int64_t ny, int64_t nx,
                                    const int64_t *src_strides, const int64_t *dst_strides, int connectivity,
                                    int by_value, const void *background, const void *fill, int64_t min_size,
                                    void *workspace, size_t workspace_bytes, void *hip_stream)
{
    const char *fn = "nd_amd_sieve_regions";
    bool empty = false;
    int rc = rg_check(fn, dtype, connectivity, nplanes, ny, nx, &empty);
    if (rc != ND_AMD_OK || empty) return rc;
    rc = check_strides(fn, "src_strides", src_strides);
    if (rc == ND_AMD_OK) rc = check_strides(fn, "dst_strides", dst_strides);
    if (rc != ND_AMD_OK) return rc;
    if (!src || !dst || !background || !fill) {
        set_error("%s: src, dst, background or fill is null", fn);
        return ND_AMD_EINVAL;
    }
    const bool copy = min_size <= 1;
    const RgPlan plan = rg_plan(nplanes, ny, nx, true);
    if (!copy) {
        rc = rg_workspace(fn, plan, workspace, workspace_bytes);
        if (rc != ND_AMD_OK) return rc;
    }
    RgArgs a;
    if (copy) {
        a = RgArgs{};
        a.src = src;
        a.ssp = src_strides[0]; a.ssy = src_strides[1]; a.ssx = src_strides[2];
        a.nplanes = nplanes; a.ny = ny; a.nx = nx; a.npix = ny * nx;
    } else {
        rg_args(a, src, src_strides, nplanes, ny, nx, workspace, plan, true, rg_bits(background, dtype));
    }
    unsigned write_blocks = 0;
    const int64_t per_plane = ceil_div(a.npix, RG_PX);
    rc = rg_blocks(fn, per_plane, nplanes, &write_blocks);
    if (rc != ND_AMD_OK) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    KernelTimer timer(ND_AMD_KERNEL_REGIONS, stream);
    if (!copy) {
        rc = rg_label(fn, a, dtype, connectivity, by_value != 0, nullptr, plan, stream);
        if (rc != ND_AMD_OK) return rc;
    }
    const uint64_t fill_bits = rg_bits(fill, dtype);
    auto launch = [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL((regions_sieve_kernel<E>), dim3(write_blocks), dim3(RG_PX), 0, stream, a,
                           reinterpret_cast<E *>(dst), dst_strides[0], dst_strides[1], dst_strides[2], min_size,
                           fill_bits, (uint32_t)per_plane);
    };
    if (!pick_eq<1, 4, 8>(region_dtype_size(dtype), [&](auto S) {
            constexpr int B = decltype(S)::value;
            if constexpr (B == 1) launch(uint8_t{});
            else if constexpr (B == 4) launch(uint32_t{});
            else launch(uint64_t{});
        })) {
        set_error("%s: no kernel for elements of %d bytes", fn, region_dtype_size(dtype));
        return ND_AMD_EUNSUPPORTED;
    }
    ND_HIP_CHECK(hipGetLastError());
    return copy ? ND_AMD_OK : rg_finish(fn, a.giveup, stream);
}
