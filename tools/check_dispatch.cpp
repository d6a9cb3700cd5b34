// tools/check_dispatch.cpp -- the dispatch helpers (nd_amd/csrc/dispatch.hpp) checked on a CPU.  Plain C++:
//
//   clang++ -std=c++17 -Wall tools/check_dispatch.cpp -o check_dispatch && ./check_dispatch
//
// Exit status 0 and one "ok" line per check, or a line per failure and status 1.  tests/test_dispatch_cpu.py
// builds it plainly and with -fsanitize=address,undefined.
#include <stdio.h>

#include <vector>

#include "../nd_amd/csrc/dispatch.hpp"

using namespace nd_amd;

static int failures = 0;

static void expect(bool ok, const char *what, int v)
{
    if (!ok) {
        printf("FAILED %s at v = %d\n", what, v);
        ++failures;
    }
}

// every v from 0 to one past the last value: one call with the first V >= v, or none and `false` beyond the list
template <int... Vs>
static void check_le()
{
    const std::vector<int> list = {Vs...};
    for (int v = 0; v <= list.back() + 1; ++v) {
        int calls = 0, got = -1;
        const bool hit = pick_le<Vs...>(v, [&](auto V) {
            static_assert(std::is_same<decltype(V), int_c<decltype(V)::value>>::value, "an integral constant");
            ++calls;
            got = decltype(V)::value;
        });
        int want = -1;
        for (size_t i = list.size(); i-- > 0;)
            if (v <= list[i]) want = list[i];
        expect(hit == (want >= 0), "pick_le: result", v);
        expect(calls == (want >= 0 ? 1 : 0), "pick_le: number of calls", v);
        expect(got == want, "pick_le: value", v);
    }
}

// the same for exact matches, in whatever order the list is written
template <int... Vs>
static void check_eq()
{
    const std::vector<int> list = {Vs...};
    int top = 0;
    for (const int x : list) top = x > top ? x : top;
    for (int v = 0; v <= top + 1; ++v) {
        int calls = 0, got = -1;
        const bool hit = pick_eq<Vs...>(v, [&](auto V) {
            ++calls;
            got = decltype(V)::value;
        });
        int want = -1;
        for (const int x : list)
            if (x == v) want = x;
        expect(hit == (want >= 0), "pick_eq: result", v);
        expect(calls == (want >= 0 ? 1 : 0), "pick_eq: number of calls", v);
        expect(got == want, "pick_eq: value", v);
    }
}

int main()
{
    // the lists of the launch sites
    check_le<8, 16, 24, 32, 48>();
    check_le<8, 16, 24, 32>();
    check_le<8, 16, 24>();
    check_le<32, 64, 128>();
    check_le<16, 20, 24>();
    check_le<4, 8, 12, 16>();
    check_le<7>();
    printf("ok pick_le\n");
    check_eq<4, 8, 12, 16>();
    check_eq<64, 32, 16>();
    check_eq<3, 5>();
    check_eq<1, 2, 3>();
    check_eq<0>();
    printf("ok pick_eq\n");
    for (int b = 0; b < 2; ++b) {
        int calls = 0, got = -1;
        pick(b != 0, [&](auto B) {
            static_assert(std::is_same<decltype(B), bool_c<decltype(B)::value>>::value, "an integral constant");
            ++calls;
            got = decltype(B)::value ? 1 : 0;
        });
        expect(calls == 1, "pick: number of calls", b);
        expect(got == b, "pick: value", b);
    }
    printf("ok pick\n");
    // the value is a constant expression inside the callback, also in a nested one: it can size an array
    int total = 0;
    pick_le<2, 4>(3, [&](auto A) {
        pick(true, [&](auto B) {
            int cells[decltype(A)::value + (decltype(B)::value ? 1 : 0)] = {};
            total = (int)(sizeof(cells) / sizeof(cells[0]));
        });
    });
    expect(total == 5, "nested: constant expression", 3);
    printf("ok nested\n");
    return failures ? 1 : 0;
}
