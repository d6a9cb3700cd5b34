// tools/check_entry_args.cpp -- the grid helpers of nd_amd/csrc/entry_args.hpp checked on a CPU against the
// forms they replaced, written out literally here.  Plain C++:
//
//   clang++ -std=c++17 -Wall tools/check_entry_args.cpp -o check_entry_args && ./check_entry_args
//
// Exit status 0 and one "ok" line per check, or a line per failure and status 1.  tests/test_dispatch_cpu.py
// builds it plainly and with -fsanitize=address,undefined.  (A GPU test cannot see a wrong upper clamp: any
// number of blocks walks a list correctly.)
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../nd_amd/csrc/entry_args.hpp"

static char last_error[256];
void nd_amd::set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}

using namespace nd_amd;

static int failures = 0;

static void expect(bool ok, const char *what, long long a, long long b, long long c, long long d)
{
    if (!ok) {
        printf("FAILED %s at (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
        ++failures;
    }
}

// ---- the clamp as the launch sites wrote it (the divisions written out too: the header's ceil_div is under test)
static int64_t literal_shard_blocks(int64_t listed, int64_t shards, int64_t per_block, int64_t cap)
{
    int64_t per_shard = ((listed + shards - 1) / shards + per_block - 1) / per_block;
    if (per_shard > cap) per_shard = cap;
    if (per_shard < 1) per_shard = 1;
    return per_shard;
}

static void check_shard_blocks()
{
    // every (shards, per_block, cap) of the library: the dual-pol searches (128 shards; 64 entries per block to
    // 16, 32 or 64 blocks, 32 or 16 per block to 256), the full-pol ones (the same, and the dump whose capacity is
    // a shard's share already), intensities only
    const int64_t uses[][3] = {{128, 64, 16}, {128, 64, 32}, {128, 64, 64}, {128, 32, 256}, {128, 16, 256}, {1, 64, 64}};
    for (const auto &u : uses) {
        const int64_t shards = u[0], per_block = u[1], cap = u[2];
        std::vector<int64_t> at = {0, 1, 2, 0xfffffffeLL, 0xfffffffdLL};
        // both sides of every multiple at which the result steps, up to and beyond where the upper clamp binds
        for (int64_t m = 1; m <= cap + 2; ++m)
            for (int64_t d = -1; d <= 1; ++d) at.push_back(shards * per_block * m + d);
        for (int64_t m = 1; m <= 4; ++m)
            for (int64_t d = -1; d <= 1; ++d) at.push_back(shards * m + d);
        for (const int64_t listed : at) {
            const int64_t got = shard_blocks(listed, shards, per_block, cap);
            expect(got == literal_shard_blocks(listed, shards, per_block, cap), "shard_blocks: the literal form", listed,
                   shards, per_block, cap);
            expect(got >= 1 && got <= cap, "shard_blocks: 1 <= blocks <= cap", listed, shards, per_block, cap);
            // below the cap the blocks cover a shard's share in one turn each, and none is idle
            const int64_t share = (listed + shards - 1) / shards;
            if (got < cap && listed > 0)
                expect(got * per_block >= share && (got - 1) * per_block < share, "shard_blocks: one turn each", listed,
                       shards, per_block, cap);
        }
        expect(shard_blocks(0, shards, per_block, cap) == 1, "shard_blocks: never zero blocks", 0, shards, per_block, cap);
        expect(shard_blocks(shards * per_block * cap, shards, per_block, cap) == cap, "shard_blocks: cap reached", 0, shards,
               per_block, cap);
        expect(shard_blocks(shards * per_block * (cap - 1), shards, per_block, cap) == cap - 1,
               "shard_blocks: one below the cap", 0, shards, per_block, cap);
    }
    printf("ok shard_blocks\n");
}

// ---- the row walk as the five functions wrote it
struct LiteralWalk {
    bool flat, refused;
    int64_t nx, nrows, blocks_per_row;
};
static LiteralWalk literal_row_walk(int64_t ny, int64_t nx, int64_t sy, int64_t sx, bool pixel_major, int64_t px_per_block)
{
    LiteralWalk w;
    const int64_t npix = ny * nx;
    w.flat = ((sx == 1) && (sy == nx)) || pixel_major;
    w.nx = w.flat ? npix : nx;
    w.nrows = w.flat ? 1 : ny;
    w.blocks_per_row = (w.nx + px_per_block - 1) / px_per_block;
    const int64_t nblocks = w.blocks_per_row * w.nrows;
    w.refused = nblocks > 0x7fffffffLL;
    return w;
}

static void check_row_walk()
{
    struct Case {
        int64_t ny, nx, sy, sx;
        bool pixel_major;
    };
    const int64_t two31 = 0x80000000LL;
    const Case cases[] = {
        {1, 1, 1, 1, false},          {1, 3, 3, 1, false},          {5, 7, 7, 1, false},           // flat
        {5, 7, 16, 1, false},         {5, 7, 1, 5, false},          {5, 7, 14, 2, false},          // strided
        {5, 7, 7 * 4, 4, true},       {3, 1000, 1000 * 8, 8, true},                                // pixel-major: forced flat
        {1024, 4096, 4096, 1, false}, {1024, 4096, 4100, 1, false}, {65535, 65536, 65536, 1, false},
        // a strided raster of 2^31 - 1, 2^31 and 2^31 + 1 one-block rows: the last launch that fits, the first two that do not
        {two31 - 1, 1, 2, 1, false},  {two31, 1, 2, 1, false},      {two31 + 1, 1, 2, 1, false},
        // the same rows back to back are one row of 2^31 pixels
        {two31, 1, 1, 1, false},      {two31 / 2 + 1, 300, 512, 1, false},
    };
    const int64_t widths[] = {64, 256, 512, 1024};     // a wave; kRetainThreads; kGlobalThreads x 2 and x 4 pixels per lane
    for (const Case &c : cases)
        for (const int64_t px : widths) {
            const LiteralWalk want = literal_row_walk(c.ny, c.nx, c.sy, c.sx, c.pixel_major, px);
            RowWalk w;
            last_error[0] = 0;
            const int rc = row_walk("entry", c.ny, c.nx, c.sy, c.sx, c.pixel_major, px, &w);
            expect(rc == (want.refused ? ND_AMD_EUNSUPPORTED : ND_AMD_OK), "row_walk: code", c.ny, c.nx, c.sy, px);
            expect(w.flat == want.flat && w.nx == want.nx && w.nrows == want.nrows && w.blocks_per_row == want.blocks_per_row,
                   "row_walk: the literal form", c.ny, c.nx, c.sy, px);
            expect((rc != ND_AMD_OK) == (strncmp(last_error, "entry: raster too large", 23) == 0), "row_walk: message", c.ny,
                   c.nx, c.sy, px);
            // the same rows in blocks of a wave, as the time-split forms ask for them behind the first walk
            const LiteralWalk want64 = literal_row_walk(c.ny, c.nx, c.sy, c.sx, c.pixel_major, 64);
            const int rc64 = row_blocks("entry", &w, 64);
            expect(rc64 == (want64.refused ? ND_AMD_EUNSUPPORTED : ND_AMD_OK), "row_blocks: code", c.ny, c.nx, c.sy, px);
            expect(w.nx == want64.nx && w.nrows == want64.nrows && w.blocks_per_row == want64.blocks_per_row,
                   "row_blocks: the literal form", c.ny, c.nx, c.sy, px);
        }
    printf("ok row_walk\n");
}

int main()
{
    check_shard_blocks();
    check_row_walk();
    return failures ? 1 : 0;
}
