// tools/check_borders.cpp -- the border index maps of nd_amd/csrc/borders.hpp and align256 of entry_args.hpp checked
// on a CPU.  Plain C++:
//
//   clang++ -std=c++17 -Wall tools/check_borders.cpp -o check_borders && ./check_borders
//
// For every array length 1 .. 9 and every index from -4 len - 3 to 5 len + 2 it prints the two 64-bit maps, one line
// "index MODE len cc value" / "line MODE len cc value" each (tests/test_borders_cpu.py compares them with scipy), a
// line "differ MODE len cc index line" wherever the two rules disagree, then one "ok" line per check, or a line per
// failure and exit status 1.  The test builds it plainly and with -fsanitize=address,undefined: the 32-bit forms
// are run at the host-checked limit of their kernels, where only the sanitizer sees an overflow.
#include <stdio.h>

#include <vector>

#include "../nd_amd/csrc/borders.hpp"
#include "../nd_amd/csrc/entry_args.hpp"

void nd_amd::set_error(const char *, ...) {}

using namespace nd_amd;

static int failures = 0;

static void expect(bool ok, const char *what, long long a, long long b, long long c)
{
    if (!ok) {
        printf("FAILED %s at (%lld, %lld, %lld)\n", what, a, b, c);
        ++failures;
    }
}

static const int kModes[] = {ND_AMD_MODE_REFLECT, ND_AMD_MODE_CONSTANT, ND_AMD_MODE_NEAREST, ND_AMD_MODE_MIRROR,
                             ND_AMD_MODE_WRAP};
static const char *mode_name(int mode)
{
    switch (mode) {
    case ND_AMD_MODE_REFLECT: return "reflect";
    case ND_AMD_MODE_CONSTANT: return "constant";
    case ND_AMD_MODE_NEAREST: return "nearest";
    case ND_AMD_MODE_MIRROR: return "mirror";
    default: return "wrap";
    }
}

static int64_t clamp_into(int64_t m, int64_t len) { return m < 0 ? 0 : (m >= len ? len - 1 : m); }

// The source index of every position lo .. hi of the extended line, built without any index arithmetic of the kind
// under test: the array, then copies of the mode's pattern laid side by side to the left and to the right of it.
static std::vector<int64_t> tiled_line(int64_t len, int mode, int64_t lo, int64_t hi)
{
    std::vector<int64_t> ext(hi - lo + 1, -1);              // constant: -1 outside the array
    auto put = [&](int64_t cc, int64_t v) {
        if (cc >= lo && cc <= hi) ext[cc - lo] = v;
    };
    for (int64_t i = 0; i < len; ++i) put(i, i);
    std::vector<int64_t> pattern;                           // one period, starting at the array's first element
    for (int64_t i = 0; i < len; ++i) pattern.push_back(i);                                      // a b c d
    if (mode == ND_AMD_MODE_REFLECT)
        for (int64_t i = len - 1; i >= 0; --i) pattern.push_back(i);                             // a b c d | d c b a
    if (mode == ND_AMD_MODE_MIRROR)
        for (int64_t i = len - 2; i >= 1; --i) pattern.push_back(i);                             // a b c d | c b
    if (mode == ND_AMD_MODE_NEAREST) {
        for (int64_t cc = lo; cc < 0; ++cc) put(cc, 0);
        for (int64_t cc = len; cc <= hi; ++cc) put(cc, len - 1);
    }
    if (mode == ND_AMD_MODE_REFLECT || mode == ND_AMD_MODE_MIRROR || mode == ND_AMD_MODE_WRAP) {
        const int64_t period = (int64_t)pattern.size();
        int64_t start = 0;
        while (start > lo) start -= period;
        for (; start <= hi; start += period)
            for (int64_t j = 0; j < period; ++j) put(start + j, pattern[j]);
    }
    return ext;
}

static void check_rules()
{
    int differing = 0;
    for (const int mode : kModes)
        for (int64_t len = 1; len <= 9; ++len) {
            const int64_t lo = -4 * len - 3, hi = 5 * len + 2;
            const std::vector<int64_t> want = tiled_line(len, mode, lo, hi);
            for (int64_t cc = lo; cc <= hi; ++cc) {
                const int64_t line = extend_line<int64_t, false>(cc, len, mode);
                const int64_t index = extend_index<int64_t, false>(cc, len, mode);
                printf("line %s %lld %lld %lld\n", mode_name(mode), (long long)len, (long long)cc, (long long)line);
                printf("index %s %lld %lld %lld\n", mode_name(mode), (long long)len, (long long)cc, (long long)index);
                expect(line == want[cc - lo], "extend_line: the tiled pattern", mode, len, cc);
                if (mode == ND_AMD_MODE_REFLECT) {
                    expect(ml_reflect((int)cc, (int)len) == line, "ml_reflect: extend_line's reflect", mode, len, cc);
                    expect(reflect_line(cc, len) == line, "reflect_line: extend_line's reflect", mode, len, cc);
                }
                if (mode != ND_AMD_MODE_CONSTANT) {
                    expect(extend_line<int, true>((int)cc, (int)len, mode) == clamp_into(line, len),
                           "extend_line<int, true>: the clamped 64-bit result", mode, len, cc);
                    expect(extend_index<int, true>((int)cc, (int)len, mode) == clamp_into(index, len),
                           "extend_index<int, true>: the clamped 64-bit result", mode, len, cc);
                }
                if (cc >= -len && cc < 2 * len)
                    expect(index == line, "extend_index: extend_line within one length of the array", mode, len, cc);
                if (index != line) {
                    printf("differ %s %lld %lld %lld %lld\n", mode_name(mode), (long long)len, (long long)cc, (long long)index,
                           (long long)line);
                    ++differing;
                }
            }
        }
    printf("ok extend_line\nok extend_index (%d positions differ from extend_line)\n", differing);
}

// the 32-bit forms at the largest extent their kernels take (checked on the host: below 2^30)
static void check_limit()
{
    const int64_t len = ((int64_t)1 << 30) - 1, two30 = (int64_t)1 << 30;
    const int64_t around[] = {-two30, -len, -1, 0, len - 1, len, two30};
    for (const int mode : kModes) {
        if (mode == ND_AMD_MODE_CONSTANT) continue;
        for (const int64_t c0 : around)
            for (int64_t cc = c0 - 8; cc <= c0 + 8; ++cc) {
                expect(extend_line<int, true>((int)cc, (int)len, mode) == clamp_into(extend_line<int64_t, false>(cc, len, mode), len),
                       "extend_line<int, true> at len 2^30 - 1", mode, len, cc);
                expect(extend_index<int, true>((int)cc, (int)len, mode) == clamp_into(extend_index<int64_t, false>(cc, len, mode), len),
                       "extend_index<int, true> at len 2^30 - 1", mode, len, cc);
            }
    }
    printf("ok 32-bit limit\n");
}

// non-local means asks for p + offset with 0 <= p < n and |offset| < n
static void check_reflect_once()
{
    for (int64_t n = 1; n <= 9; ++n)
        for (int64_t i = -n + 1; i <= 2 * n - 2; ++i) {
            const int64_t want = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
            expect(reflect_once<int64_t>(i, n) == want, "reflect_once<int64_t>", n, i, want);
            expect(reflect_once<int>(i, n) == (int)want, "reflect_once<int>", n, i, want);
            expect(want >= 0 && want < n, "reflect_once: inside the array", n, i, want);
        }
    printf("ok reflect_once\n");
}

static void check_align256()
{
    auto check = [](size_t n) { expect(align256(n) == (n + 255) / 256 * 256, "align256", (long long)n, 0, 0); };
    for (size_t m = 0; m <= (size_t)1 << 16; m += 256)
        for (size_t d = 0; d < 5; ++d) {
            if (m + d >= 2) check(m + d - 2);
        }
    const size_t big = (size_t)1 << 40;
    for (size_t n = big - 300; n <= big + 300; ++n) check(n);
    printf("ok align256\n");
}

int main()
{
    check_rules();
    check_limit();
    check_reflect_once();
    check_align256();
    return failures ? 1 : 0;
}
