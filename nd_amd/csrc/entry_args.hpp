// nd_amd/csrc/entry_args.hpp -- what the change-detection entries (nd_amd_omnibus_c2 / _c2_ml / _c2_pixel_major,
// _c3 / _c3_pixel_major, _diag, nd_amd_change_segments), the region and the zonal entries decide alike, written once: which arguments are
// acceptable, how a raster is walked in rows, and how many blocks walk a sharded candidate list; and align256, where
// every unit's workspace sections start.  Plain C++:
// no HIP header and no device symbol, so every unit may include it (common.hpp does) and a CPU checks it
// (tools/check_entry_args.cpp, tests/test_host_logic.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/nd_amd.h"

namespace nd_amd {

void set_error(const char *fmt, ...);

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// workspace sections start on 256-byte boundaries
static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- entry checks: ND_AMD_OK to go on, or the code to return with the message set.  `entry` is the entry
// point's name.  An entry keeps what only it checks between these calls.  Every refusal here is ND_AMD_EINVAL
// except the pixel index's ND_AMD_EUNSUPPORTED, so among the checks only their place relative to that one and
// to the empty raster's ND_AMD_OK can change a return code (tests/test_host_logic.py pins both).
static inline int check_dtype(const char *entry, int dtype)
{
    if (dtype == ND_AMD_F32 || dtype == ND_AMD_F64) return ND_AMD_OK;
    set_error("%s: dtype must be ND_AMD_F32 or ND_AMD_F64, got %d", entry, dtype);
    return ND_AMD_EINVAL;
}

// A negative dimension is refused; *empty says that there is nothing to write.  The entry returns ND_AMD_OK on
// it where it always did: behind the checks that it makes on an empty raster too, before the pointers are looked at.
static inline int check_shape(const char *entry, int64_t ny, int64_t nx, int64_t k, bool *empty)
{
    *empty = ny == 0 || nx == 0 || k == 0;
    if (ny >= 0 && nx >= 0 && k >= 0) return ND_AMD_OK;
    set_error("%s: negative shape (%lld, %lld, %lld)", entry, (long long)ny, (long long)nx, (long long)k);
    return ND_AMD_EINVAL;
}

static inline int check_planes(const char *entry, const void *const planes[], int n, const void *change)
{
    if (!planes || !change) {
        set_error("%s: null data pointer", entry);
        return ND_AMD_EINVAL;
    }
    for (int p = 0; p < n; ++p)
        if (!planes[p]) {
            set_error("%s: plane %d is null", entry, p);
            return ND_AMD_EINVAL;
        }
    return ND_AMD_OK;
}

static inline int check_looks(const char *entry, uint32_t n_looks)
{
    if (n_looks >= 1) return ND_AMD_OK;
    set_error("%s: n_looks must be >= 1", entry);
    return ND_AMD_EINVAL;
}

// pixels are listed by 32-bit index, 0xffffffff being the list's "none"
static inline int check_pixel_index(const char *entry, int64_t ny, int64_t nx)
{
    if (ny * nx < 0xffffffffLL) return ND_AMD_OK;
    set_error("%s: raster of %lld pixels exceeds the 32-bit pixel index", entry, (long long)(ny * nx));
    return ND_AMD_EUNSUPPORTED;
}

// the pixel-major entries: a variable's dates lie 1 (real) or 2 (one half of an interleaved complex array) apart
static inline int check_date_strides(const char *entry, const int64_t *date_stride, int n)
{
    if (!date_stride) {
        set_error("%s: date_stride is null", entry);
        return ND_AMD_EINVAL;
    }
    for (int v = 0; v < n; ++v)
        if (date_stride[v] != 1 && date_stride[v] != 2) {
            set_error("%s: date strides must be 1 or 2, got %lld for variable %d", entry, (long long)date_stride[v], v);
            return ND_AMD_EINVAL;
        }
    return ND_AMD_OK;
}

// ---- the region entries (nd_amd_label_regions, nd_amd_region_sizes, nd_amd_sieve_regions)
// the element size of a map's type, 0 for a type that is none
static inline int region_dtype_size(int dtype)
{
    switch (dtype) {
    case ND_AMD_U8: return 1;
    case ND_AMD_F32: case ND_AMD_I32: return 4;
    case ND_AMD_F64: case ND_AMD_I64: return 8;
    default: return 0;
    }
}

static inline int check_region_dtype(const char *entry, int dtype)
{
    if (region_dtype_size(dtype)) return ND_AMD_OK;
    set_error("%s: dtype must be ND_AMD_U8, ND_AMD_I32, ND_AMD_I64, ND_AMD_F32 or ND_AMD_F64, got %d", entry, dtype);
    return ND_AMD_EINVAL;
}

static inline int check_connectivity(const char *entry, int connectivity)
{
    if (connectivity == 4 || connectivity == 8) return ND_AMD_OK;
    set_error("%s: connectivity must be 4 or 8, got %d", entry, connectivity);
    return ND_AMD_EINVAL;
}

// pixels of a plane are linked by their in-plane index in an int32
static inline int check_plane_pixels(const char *entry, int64_t ny, int64_t nx)
{
    const int64_t limit = (int64_t)1 << 31;
    if (ny <= 0 || nx < limit / ny + (limit % ny != 0)) return ND_AMD_OK;
    set_error("%s: planes of 2^31 pixels or more are not served (%lld x %lld)", entry, (long long)ny, (long long)nx);
    return ND_AMD_EUNSUPPORTED;
}

// 3 host values in elements for (plane, y, x), none negative
static inline int check_strides(const char *entry, const char *what, const int64_t *s)
{
    if (!s) {
        set_error("%s: %s is null", entry, what);
        return ND_AMD_EINVAL;
    }
    if (s[0] >= 0 && s[1] >= 0 && s[2] >= 0) return ND_AMD_OK;
    set_error("%s: negative stride in %s (%lld, %lld, %lld)", entry, what, (long long)s[0], (long long)s[1],
              (long long)s[2]);
    return ND_AMD_EINVAL;
}

// ---- the zonal entries (nd_amd_zonal_keys, nd_amd_zonal_stats, nd_amd_zonal_paint)
// 2 host values in elements for (y, x) of one plane, none negative
static inline int check_strides2(const char *entry, const char *what, const int64_t *s)
{
    if (!s) {
        set_error("%s: %s is null", entry, what);
        return ND_AMD_EINVAL;
    }
    if (s[0] >= 0 && s[1] >= 0) return ND_AMD_OK;
    set_error("%s: negative stride in %s (%lld, %lld)", entry, what, (long long)s[0], (long long)s[1]);
    return ND_AMD_EINVAL;
}

// a pixel's key is its zone's rank in an int32, n itself being "no zone"
static inline int check_zone_count(const char *entry, int64_t n)
{
    if (n < 0) {
        set_error("%s: negative number of zones %lld", entry, (long long)n);
        return ND_AMD_EINVAL;
    }
    if (n < 0x7fffffffLL) return ND_AMD_OK;
    set_error("%s: 2^31 - 1 zones or more are not served (%lld)", entry, (long long)n);
    return ND_AMD_EUNSUPPORTED;
}

// ---- grids
// Blocks per shard that walk a candidate list of at most `listed` entries spread over `shards` shards, a block
// taking `per_block` entries at a time and striding through its shard's list: enough for one turn each, at most
// `cap` (what the chip holds; the blocks then take more turns), and never none -- zero blocks is a failed launch.
static inline int64_t shard_blocks(int64_t listed, int64_t shards, int64_t per_block, int64_t cap)
{
    const int64_t n = ceil_div(ceil_div(listed, shards), per_block);
    return n > cap ? cap : (n < 1 ? 1 : n);
}

// How a launch walks a raster: row by row, or -- rows back to back (stride_x == 1, stride_y == nx), and always
// for pixel-major input (force_flat) -- as ONE row of ny * nx pixels, so that no block is cut short at a row's
// end.  blocks_per_row blocks of px_per_block pixels cover a row; block b serves row b / blocks_per_row.
struct RowWalk {
    bool flat;
    int64_t nx, nrows, blocks_per_row;
    int64_t nblocks() const { return blocks_per_row * nrows; }
};

// the same rows in blocks of another width; ND_AMD_EUNSUPPORTED beyond the 2^31 - 1 blocks of one launch
// (only a strided raster of 2^31 rows and more gets there)
static inline int row_blocks(const char *entry, RowWalk *w, int64_t px_per_block)
{
    w->blocks_per_row = ceil_div(w->nx, px_per_block);
    if (w->nblocks() <= 0x7fffffffLL) return ND_AMD_OK;
    set_error("%s: raster too large for one launch (%lld blocks)", entry, (long long)w->nblocks());
    return ND_AMD_EUNSUPPORTED;
}

static inline int row_walk(const char *entry, int64_t ny, int64_t nx, int64_t sy, int64_t sx, bool force_flat,
                           int64_t px_per_block, RowWalk *w)
{
    w->flat = force_flat || (sx == 1 && sy == nx);
    w->nx = w->flat ? ny * nx : nx;
    w->nrows = w->flat ? 1 : ny;
    return row_blocks(entry, w, px_per_block);
}

}  // namespace nd_amd
