// tools/check_memops.cpp -- the piece arithmetic of the LDS staging loops (nd_amd/csrc/memops.hpp, plain part) checked
// on a CPU.  Plain C++:
//
//   clang++ -std=c++17 -Wall tools/check_memops.cpp -o check_memops && ./check_memops
//
// For every run length from 0 to 64 pixels x 48 dates x 2 x 8 bytes -- the multiples of 16 in the plain form, the
// multiples of 4 in the form with the 4-byte tail -- it walks the steps the kernels walk (c0 = 0, kLdsStep, .. below
// lds_run_whole, one step further to see that nothing follows, then the tail) over 64 lanes and checks that the pieces
// cover [0, bytes) exactly once, that none reaches beyond it, that every piece lands in the image at the offset it came
// from (the instruction is given `base`, the hardware adds lane * width), and that the list of transfers is the one
// of the loop the kernels held before memops.hpp, restated below.  One "ok" line per form, or a line per failure and
// exit status 1.  tests/test_dispatch_cpu.py builds it plainly and with -fsanitize=address,undefined.
#include <stdio.h>

#include <vector>

#include "../nd_amd/csrc/memops.hpp"

using namespace nd_amd;

static int failures = 0;

static void expect(bool ok, const char *what, long long a, long long b, long long c)
{
    if (!ok && failures < 50) printf("FAILED %s at (%lld, %lld, %lld)\n", what, a, b, c);
    if (!ok) ++failures;
}

struct Transfer {
    int src, lds, width;          // source byte offset, LDS byte offset of the lane's piece, bytes
    bool operator==(const Transfer &o) const { return src == o.src && lds == o.lds && width == o.width; }
};

// The loop of omnibus_c2_pm_dma_kernel (with the tail) and of omnibus_c2_pm_long_kernel, omnibus_c2_stream_kernel and
// omnibus_c3_pm_kernel (without) as those kernels wrote it: global_load_lds(src + eb, dst + c0, 16) puts lane l's 16
// bytes at dst + c0 + 16 l.
static std::vector<Transfer> as_written(const int bytes, const bool tail)
{
    std::vector<Transfer> out;
    const int bytes16 = tail ? bytes & ~15 : bytes;
    for (int c0 = 0; c0 < bytes16; c0 += 1024)
        for (int lane = 0; lane < 64; ++lane) {
            const int eb = c0 + lane * 16;
            if (eb < bytes16) out.push_back({eb, c0 + lane * 16, 16});
        }
    if (tail)
        for (int lane = 0; lane < 64; ++lane)
            if (bytes16 < bytes && bytes16 + lane * 4 < bytes) out.push_back({bytes16 + lane * 4, bytes16 + lane * 4, 4});
    return out;
}

template <bool TAIL>
static void check_form(const int max_bytes, const int multiple)
{
    std::vector<unsigned char> words;
    for (int bytes = 0; bytes <= max_bytes; bytes += multiple) {
        std::vector<Transfer> got;
        words.assign((size_t)bytes / 4, 0);
        auto take = [&](const LdsPiece &p, const int lane, const int want_width, const int want_base) {
            if (!p.width) return;
            const int lds = p.base + lane * p.width;          // where the hardware puts the lane's piece
            expect(p.width == want_width && p.base == want_base, "width / base of a piece", bytes, p.base, lane);
            expect(p.src() >= 0 && p.src() + p.width <= bytes, "piece inside the run", bytes, p.src(), p.width);
            expect(lds == p.src(), "LDS offset == source offset", bytes, lds, p.src());
            if (p.src() >= 0 && p.src() + p.width <= bytes)
                for (int w = p.src() / 4; w < (p.src() + p.width) / 4; ++w) ++words[(size_t)w];
            got.push_back({p.src(), lds, p.width});
        };
        const int whole = lds_run_whole<TAIL>(bytes);
        expect(whole <= bytes && bytes - whole < kLdsLane && whole % kLdsLane == 0, "whole part", bytes, whole, 0);
        int c0 = 0;
        for (; c0 < whole; c0 += kLdsStep)
            for (int lane = 0; lane < 64; ++lane) take(lds_stage_piece<TAIL>(bytes, c0, lane), lane, kLdsLane, c0);
        for (int lane = 0; lane < 64; ++lane)                 // a step the loop does not take: nothing to move
            expect(lds_stage_piece<TAIL>(bytes, c0, lane).width == 0, "no piece behind the last step", bytes, c0, lane);
        if (TAIL) {
            for (int lane = 0; lane < 64; ++lane) {
                const LdsPiece p = lds_stage_tail(bytes, lane);
                expect(whole < bytes || p.width == 0, "no tail behind a whole run", bytes, lane, p.width);
                take(p, lane, kLdsTailLane, whole);
            }
        }
        for (size_t w = 0; w < words.size(); ++w) expect(words[w] == 1, "every word exactly once", bytes, 4 * (long long)w, words[w]);
        expect(got == as_written(bytes, TAIL), "the transfers of the loop as the kernels wrote it", bytes, (long long)got.size(), 0);
    }
    if (!failures) printf("ok %s form: run lengths 0 .. %d in steps of %d\n", TAIL ? "tail" : "plain", max_bytes, multiple);
}

int main()
{
    static_assert(kLdsStep == 1024 && kLdsLane == 16 && kLdsTailLane == 4, "64 lanes x 16 bytes; 4-byte tail pieces");
    const int max_bytes = 64 * 48 * 2 * 8;
    check_form<false>(max_bytes, 16);
    check_form<true>(max_bytes, 4);
    if (failures) printf("%d check(s) FAILED\n", failures);
    return failures ? 1 : 0;
}
