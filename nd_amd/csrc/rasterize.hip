// nd_amd/csrc/rasterize.hip -- polygons burned into a label raster (nd.vector.rasterize, nd/vector.py:48-187)
//
//   nd_amd_rasterize_polygons   out[l, i, j] = values[p] of the highest-index polygon p of layer l whose
//                               even-odd, half-open interior holds the centre of pixel (i, j), else fill
//                               (include/nd_amd.h has the rule, which is this project's).
//
// Three launches.  (a) the owner plane, uint32 (nlayers, ny, nx) in the workspace, is zeroed.  (b)
// rasterize_fill_kernel: one wave per (polygon, row) item, found by a wave-uniform binary search in the prefix
// sums `row_work`.  The lanes stride over the polygon's edges, apply the crossing test for the row's centre line
// and append the abscissae of the crossing edges to a wave-private LDS list; then they stride over the columns of
// the polygon's box and count the list entries <= u.  Odd pixels do atomicMax(owner, p + 1): an integer maximum
// does not depend on the arrival order, so the plane is reproducible, and a row's inside pixels are contiguous
// runs, so a wave's atomics are.  A row with more crossings than the list holds takes the fallback, in which
// every pixel lane walks all edges and counts on the fly with the same expression: the same bits.  The cost is
// the sum over rows of (edges + width x crossings), never box area x edges in the ordinary case.  (c)
// rasterize_resolve_kernel turns owners into values, 8-byte words copied bit for bit, with the caller's strides.
//
// The grid of (b) has a fixed upper size and its waves take items in turn, reading the item count from
// row_work[npolys] on the device: the host never needs that number, so the call does not synchronise.
#include "common.hpp"

#include <string.h>

using namespace nd_amd;

namespace {

constexpr int RAST_WAVE = 64;
constexpr int RAST_WAVES = 4;                       // waves (items in flight) per block
constexpr int RAST_THREADS = RAST_WAVE * RAST_WAVES;
constexpr int RAST_MAX = ND_AMD_RASTERIZE_MAX_CROSSINGS;
constexpr int64_t RAST_MAX_BLOCKS = 16384;          // 256 CUs x 8 blocks x 8: the tail of uneven items stays short

struct RastArgs {
    const double *verts;
    const int64_t *ring_offsets, *poly_offsets, *row_work;
    const int32_t *layer, *boxes;
    int64_t npolys, nlayers, ny, nx;
};

// (x1, y1) the endpoint with the smaller py; does the edge cross the centre line v, and where
__device__ __forceinline__ bool rast_cross(double px, double py, double qx, double qy, double v, double &xc)
{
    const bool swap = qy < py;
    const double x1 = swap ? qx : px, y1 = swap ? qy : py;
    const double x2 = swap ? px : qx, y2 = swap ? py : qy;
    if (!((y1 <= v) && !(y2 <= v))) return false;
    xc = x1 + ((v - y1) * (x2 - x1)) / (y2 - y1);
    return true;
}

__global__ __launch_bounds__(RAST_THREADS) void rasterize_fill_kernel(RastArgs a, uint32_t *owner)
{
    __shared__ double list[RAST_WAVES][RAST_MAX];
    const int lane = threadIdx.x & (RAST_WAVE - 1);
    const int wave = threadIdx.x / RAST_WAVE;
    double *mine = list[wave];
    const int64_t total = a.row_work[a.npolys];
    const int64_t step = (int64_t)gridDim.x * RAST_WAVES;

    for (int64_t item = (int64_t)blockIdx.x * RAST_WAVES + wave; item < total; item += step) {
        // the last p with row_work[p] <= item (wave-uniform)
        int64_t lo = 0, hi = a.npolys;
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.row_work[mid] <= item) lo = mid; else hi = mid;
        }
        const int64_t p = lo;
        const int32_t *box = a.boxes + 4 * p;
        const int64_t i = (int64_t)box[0] + (item - a.row_work[p]);
        int64_t c0 = box[2], c1 = box[3];
        const int64_t l = a.layer ? (int64_t)a.layer[p] : 0;
        // the tables are the caller's: nothing outside the owner plane is written whatever they hold
        if (i < 0 || i >= a.ny || i >= (int64_t)box[1] || l < 0 || l >= a.nlayers) continue;
        if (c0 < 0) c0 = 0;
        if (c1 > a.nx) c1 = a.nx;
        if (c0 >= c1) continue;
        const double v = (double)i + 0.5;
        const int64_t ring0 = a.poly_offsets[p], ring1 = a.poly_offsets[p + 1];
        uint32_t *orow = owner + (l * a.ny + i) * a.nx;
        const uint32_t mark = (uint32_t)(p + 1);

        int n = 0;                                  // crossings of this row, wave-uniform
        for (int64_t r = ring0; r < ring1; r++) {
            const int64_t v0 = a.ring_offsets[r], m = a.ring_offsets[r + 1] - v0;
            if (m < 3) continue;
            for (int64_t e0 = 0; e0 < m; e0 += RAST_WAVE) {
                const int64_t e = e0 + lane;
                bool cross = false;
                double xc = 0.0;
                if (e < m) {
                    const int64_t f = e + 1 < m ? e + 1 : 0;
                    const double2 P = reinterpret_cast<const double2 *>(a.verts)[v0 + e];
                    const double2 Q = reinterpret_cast<const double2 *>(a.verts)[v0 + f];
                    cross = rast_cross(P.x, P.y, Q.x, Q.y, v, xc);
                }
                const unsigned long long mask = __ballot(cross);
                const int at = n + __popcll(mask & ((1ull << lane) - 1ull));
                if (cross && at < RAST_MAX) mine[at] = xc;
                n += __popcll(mask);
            }
        }
        if (n == 0) continue;
        // the list is written and read by this wave only: order its LDS traffic, no block barrier
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        if (n <= RAST_MAX) {
            for (int64_t j = c0 + lane; j < c1; j += RAST_WAVE) {
                const double u = (double)j + 0.5;
                int cnt = 0;
                for (int q = 0; q < n; q++) cnt += mine[q] <= u ? 1 : 0;
                if (cnt & 1) atomicMax(&orow[j], mark);
            }
        } else {
            for (int64_t j = c0 + lane; j < c1; j += RAST_WAVE) {
                const double u = (double)j + 0.5;
                int cnt = 0;
                for (int64_t r = ring0; r < ring1; r++) {
                    const int64_t v0 = a.ring_offsets[r], m = a.ring_offsets[r + 1] - v0;
                    if (m < 3) continue;
                    const double2 first = reinterpret_cast<const double2 *>(a.verts)[v0];
                    double2 P = first;
                    for (int64_t e = 0; e < m; e++) {
                        const double2 Q = e + 1 < m ? reinterpret_cast<const double2 *>(a.verts)[v0 + e + 1] : first;
                        double xc;
                        if (rast_cross(P.x, P.y, Q.x, Q.y, v, xc)) cnt += xc <= u ? 1 : 0;
                        P = Q;
                    }
                }
                if (cnt & 1) atomicMax(&orow[j], mark);
            }
        }
        // the next item overwrites the list: every lane is done reading first
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// out[l, i, j] = owner ? values[owner - 1] : fill, as 8-byte words.  The thread index runs fastest along the
// output's fastest axis (`layer_fastest`: a (y, x, time) result), so the stores of a wave are contiguous there.
__global__ __launch_bounds__(256) void rasterize_resolve_kernel(const uint32_t *owner, const uint64_t *values,
                                                                uint64_t fill, int64_t npolys, int64_t nlayers,
                                                                int64_t ny, int64_t nx, uint64_t *out, int64_t sl,
                                                                int64_t sy, int64_t sx, int layer_fastest)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nlayers * ny * nx) return;
    int64_t l, i, j;
    if (layer_fastest) {
        l = t % nlayers;
        j = (t / nlayers) % nx;
        i = t / (nlayers * nx);
    } else {
        j = t % nx;
        i = (t / nx) % ny;
        l = t / (nx * ny);
    }
    const uint32_t o = owner[(l * ny + i) * nx + j];
    out[l * sl + i * sy + j * sx] = (o != 0 && (int64_t)o <= npolys) ? values[o - 1] : fill;
}

size_t rast_align(size_t v) { return (v + 255) & ~(size_t)255; }

const int64_t RAST_MAX_CELLS = (int64_t)1 << 32;

// ny * nx * nlayers, or -1 where it is negative somewhere or reaches 2^32
int64_t rast_cells(int64_t nlayers, int64_t ny, int64_t nx)
{
    if (nlayers < 0 || ny < 0 || nx < 0) return -1;
    if (nlayers == 0 || ny == 0 || nx == 0) return 0;
    if (ny >= RAST_MAX_CELLS || nx >= RAST_MAX_CELLS || nlayers >= RAST_MAX_CELLS) return -1;
    if (ny > (RAST_MAX_CELLS - 1) / nx) return -1;
    if (nlayers > (RAST_MAX_CELLS - 1) / (ny * nx)) return -1;
    return nlayers * ny * nx;
}

}  // namespace

extern "C" size_t nd_amd_rasterize_workspace_bytes(int64_t nlayers, int64_t ny, int64_t nx)
{
    const int64_t cells = rast_cells(nlayers, ny, nx);
    if (cells <= 0) return 0;
    return rast_align((size_t)cells * sizeof(uint32_t));
}

extern "C" int nd_amd_rasterize_polygons(const double *verts, const int64_t *ring_offsets, const int64_t *poly_offsets,
                                         const int32_t *layer, const int64_t *row_work, const int32_t *boxes,
                                         const void *values, int value_dtype, const void *fill, int64_t npolys,
                                         int64_t nlayers, int64_t ny, int64_t nx, void *out, int64_t stride_l,
                                         int64_t stride_y, int64_t stride_x, void *workspace, size_t workspace_bytes,
                                         void *hip_stream)
{
    const char *fn = "nd_amd_rasterize_polygons";
    if (value_dtype != ND_AMD_I64 && value_dtype != ND_AMD_F64) {
        set_error("%s: value_dtype must be ND_AMD_I64 or ND_AMD_F64, got %d", fn, value_dtype);
        return ND_AMD_EINVAL;
    }
    if (npolys < 0 || nlayers < 0 || ny < 0 || nx < 0) {
        set_error("%s: negative extent npolys=%lld nlayers=%lld ny=%lld nx=%lld", fn, (long long)npolys,
                  (long long)nlayers, (long long)ny, (long long)nx);
        return ND_AMD_EINVAL;
    }
    if (npolys >= (int64_t)0xffffffffll) {
        set_error("%s: %lld polygons, an owner is 32 bits wide (fewer than 2^32 - 1 are served)", fn,
                  (long long)npolys);
        return ND_AMD_EINVAL;
    }
    const int64_t cells = rast_cells(nlayers, ny, nx);
    if (cells < 0) {
        set_error("%s: ny * nx * nlayers = %lld * %lld * %lld reaches 2^32", fn, (long long)ny, (long long)nx,
                  (long long)nlayers);
        return ND_AMD_EINVAL;
    }
    if (stride_l < 0 || stride_y < 0 || stride_x < 0) {
        set_error("%s: negative stride (%lld, %lld, %lld)", fn, (long long)stride_l, (long long)stride_y,
                  (long long)stride_x);
        return ND_AMD_EINVAL;
    }
    if (!fill) {
        set_error("%s: fill is null", fn);
        return ND_AMD_EINVAL;
    }
    if (npolys > 0 && (!verts || !ring_offsets || !poly_offsets || !row_work || !boxes || !values)) {
        set_error("%s: null pointer among verts, ring_offsets, poly_offsets, row_work, boxes, values", fn);
        return ND_AMD_EINVAL;
    }
    if (((uintptr_t)verts & 15) || ((uintptr_t)values & 7) || ((uintptr_t)out & 7)) {
        set_error("%s: verts must be 16-byte aligned, values and out 8-byte aligned", fn);
        return ND_AMD_EINVAL;
    }
    if (cells == 0) return ND_AMD_OK;
    if (!out) {
        set_error("%s: out is null", fn);
        return ND_AMD_EINVAL;
    }
    const size_t need = nd_amd_rasterize_workspace_bytes(nlayers, ny, nx);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 255)) {
        set_error("%s: workspace missing, not 256-byte aligned or smaller than the %zu bytes "
                  "nd_amd_rasterize_workspace_bytes asks for", fn, need);
        return ND_AMD_EINVAL;
    }

    hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    uint32_t *owner = reinterpret_cast<uint32_t *>(workspace);
    uint64_t fill_bits;
    memcpy(&fill_bits, fill, sizeof(fill_bits));

    KernelTimer timer(ND_AMD_KERNEL_RASTERIZE, stream);
    ND_HIP_CHECK(hipMemsetAsync(owner, 0, need, stream));
    if (npolys > 0) {
        RastArgs a;
        a.verts = verts;
        a.ring_offsets = ring_offsets; a.poly_offsets = poly_offsets; a.row_work = row_work;
        a.layer = layer; a.boxes = boxes;
        a.npolys = npolys; a.nlayers = nlayers; a.ny = ny; a.nx = nx;
        // at most ny rows a polygon: no more blocks than items can exist, and no more than keep the device busy
        int64_t blocks = RAST_MAX_BLOCKS;
        if (npolys <= RAST_MAX_BLOCKS * RAST_WAVES / ny) blocks = ceil_div(npolys * ny, RAST_WAVES);
        if (blocks > RAST_MAX_BLOCKS) blocks = RAST_MAX_BLOCKS;
        hipLaunchKernelGGL(rasterize_fill_kernel, dim3((unsigned)blocks), dim3(RAST_THREADS), 0, stream, a, owner);
    }
    const int layer_fastest = (nlayers > 1 && stride_l < stride_x) ? 1 : 0;
    hipLaunchKernelGGL(rasterize_resolve_kernel, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, stream, owner,
                       reinterpret_cast<const uint64_t *>(values), fill_bits, npolys, nlayers, ny, nx,
                       reinterpret_cast<uint64_t *>(out), stride_l, stride_y, stride_x, layer_fastest);
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}
