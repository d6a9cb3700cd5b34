// tools/dump_omnibus_tables.cpp -- the raw bytes of the omnibus decision tables (nd_amd/csrc/omnibus_tables.hip)
// over a fixed grid, to stdout.  Plain C++, no GPU:
//
//   clang++ -x c++ -std=c++17 -O3 -ffp-contract=off -fno-fast-math \
//       tools/dump_omnibus_tables.cpp nd_amd/csrc/omnibus_tables.hip -o dump_omnibus_tables
//   ./dump_omnibus_tables | sha256sum
//
// Two builds of the tables on one machine are compared through that hash ("The decision tables in one
// host unit"); tests/test_omnibus_tables_cpu.py reads the records and checks what the bounds promise.
//
// Grid, in this order: family c2 {2,1}, c3 {3,1}, diag {1,1}, {1,2}, {1,3};  float32, float64;
// alpha 1e-4, 0.01, 0.5, 0.9, 0.99;  n 1, 4, 9 (diag: 1, 4, 4.4, 9).  One record per combination:
//   OmniTabEntry x 50      j = 1 .. 48 from get_table(48, ...), then j = 97 and 200 from make_entry
//   -- only where n is a whole number (the screens belong to the dual- and full-pol searches, whose look
//      count is an integer):
//   DenseScreen            make_dense_screen over the 48 entries
//   DenseScreenEntry x 2   make_dense_entry of j = 97 and 200
//   StreamScreen<128>      make_stream_screen over the 48 entries
//   -- only with --repeat:
//   OmniTabEntry x 48      j = 1 .. 48 from a second get_table call with the same key
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../nd_amd/csrc/omnibus_tables.hpp"

using namespace nd_amd;

static void put(const void *p, size_t n)
{
    if (fwrite(p, 1, n, stdout) != n) {
        perror("dump_omnibus_tables");
        exit(1);
    }
}

template <typename T>
static void put_screens(const std::vector<OmniTabEntry> &tab, const OmniTabEntry (&far)[2], int k, double n)
{
    const DenseScreen scr = make_dense_screen<T>(tab, k, n);
    put(&scr, sizeof(scr));
    const int jfar[2] = {97, 200};
    for (int i = 0; i < 2; ++i) {
        const DenseScreenEntry d = make_dense_entry<T>(far[i], jfar[i], n);
        put(&d, sizeof(d));
    }
    const StreamScreen<kDenseMax> ss = make_stream_screen<T, kDenseMax>(tab, scr, k, n);
    put(&ss, sizeof(ss));
}

int main(int argc, char **argv)
{
    const bool repeat = argc > 1 && strcmp(argv[1], "--repeat") == 0;
    const OmniFamily fams[5] = {{2, 1}, {3, 1}, {1, 1}, {1, 2}, {1, 3}};
    const int dtypes[2] = {ND_AMD_F32, ND_AMD_F64};
    const double alphas[5] = {1e-4, 0.01, 0.5, 0.9, 0.99};
    const double looks[4] = {1.0, 4.0, 4.4, 9.0};
    const int k = 48;
    for (const OmniFamily fam : fams)
        for (const int dtype : dtypes)
            for (const double alpha : alphas)
                for (const double n : looks) {
                    const bool whole = n == floor(n);
                    if (!whole && fam.p != 1) continue;
                    const std::vector<OmniTabEntry> tab = get_table(k, n, alpha, dtype, fam);
                    put(tab.data() + 1, (size_t)k * sizeof(OmniTabEntry));
                    const OmniTabEntry far[2] = {make_entry(97, n, alpha, dtype, fam),
                                                 make_entry(200, n, alpha, dtype, fam)};
                    put(far, sizeof(far));
                    if (whole) {
                        if (dtype == ND_AMD_F32)
                            put_screens<float>(tab, far, k, n);
                        else
                            put_screens<double>(tab, far, k, n);
                    }
                    if (repeat) {
                        const std::vector<OmniTabEntry> again = get_table(k, n, alpha, dtype, fam);
                        put(again.data() + 1, (size_t)k * sizeof(OmniTabEntry));
                    }
                }
    return 0;
}
