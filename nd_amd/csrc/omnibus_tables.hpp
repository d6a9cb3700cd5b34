// nd_amd/csrc/omnibus_tables.hpp -- the host-computed decision tables of the omnibus test, one unit for
// the three families (dual pol, full pol, intensity only): the per-series-length constants (rho, omega2,
// decision bounds) and the screens of the dense and streaming searches derived from them.  Plain C++: no
// HIP header, so the arithmetic compiles, runs and is checked on a CPU (tools/dump_omnibus_tables.cpp,
// tests/test_omnibus_tables_cpu.py).  The kernels read the types below as they are laid out here.
// p = 2 follows nd/_change.pyx:20-39, 133-151 to the letter; p = 3 is the same formulas with p = 3 (the
// reference hard-codes p = 2, nd/_change.pyx:51,99,135); q blocks: additivity of Box's expansion.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/nd_amd.h"

namespace nd_amd {

// q independent p x p blocks: dual pol {2, 1}, full pol {3, 1}, q intensity channels {1, q}
struct OmniFamily {
    int p, q;
};

// ---- constants of one omnibus test over j matrices (host-computed in double) ------------
struct OmniTabEntry {
    double m2rho;    // -2.0 * (double)(T)rho(p, j, n)        nd/_change.pyx:75-76
    double pklogk;   // (double)(p q * j) * log((double)j)    nd/_change.pyx:74
    double omega2;   // q omega2(p, j, n, rho) from double rho  nd/_change.pyx:139
    double lgam;     // lgamma(a + 1), a = f/2 = q (j - 1) p^2 / 2
    double zlo;      // fast-reject bound: z < zlo  =>  P <= alpha for certain (see omni_bounds)
    double zlo_a;    // the same bound for z_approx (hardware f32 log2), widened by its error
    double zhi;      // fast-accept bound: zhi < z < inf  =>  P > alpha for certain
    double zhi_a;    // the same for z_approx
};

constexpr int kTabArgs = 96;   // largest k whose table travels as a kernel argument
struct OmniTab {
    OmniTabEntry e[kTabArgs + 1];
};

// the kernels' data type T as the interface's ND_AMD_F32 / ND_AMD_F64
template <typename T>
constexpr int dtype_of() { return sizeof(T) == 4 ? ND_AMD_F32 : ND_AMD_F64; }

// a2 = 2a = f = q (j - 1) p^2
static inline int omni_a2(int j, OmniFamily fam) { return fam.q * (j - 1) * fam.p * fam.p; }

// Entry j of the table; dtype (ND_AMD_F32 / ND_AMD_F64) is the kernels' data type T, whose roundings the
// entry reproduces (rho, p q j) and whose precision the bounds allow for.
OmniTabEntry make_entry(int j, double n_looks, double alpha, int dtype, OmniFamily fam);

// Entries 0 (zeros) .. k, behind a small cache: they depend only on (k, dtype, family, n_looks, alpha).
std::vector<OmniTabEntry> get_table(int k, double n_looks, double alpha, int dtype, OmniFamily fam);

// ---- constants of the in-register search's screen (omnibus.hip: dense_search) ----------------
// The search decides a test from  L2 = log2(prod of determinants) - j * log2(det of sum),
// z = z0 + c * L2 with z0 = m2rho n pklogk and c = m2rho n ln 2 (< 0 for rho > 0), evaluated as
//   x = L2 - R  in float, relative to a reference point R = re + rf near the decision:
//   x < a  =>  the test fires for certain;   x > b  =>  it cannot fire;   otherwise: undecided,
// the pixel is handed to pass B (exact evaluation).  Error budget of the device's x (see
// dense_search): j * (6e-8 hardware log2 + 1.5e-8 fixed point) per determinant, j * 6e-8 for the
// determinant of the sum, < 6e-6 float32 arithmetic  =>  < 9e-6 at j = 24; `mg` below is more than
// twice that, plus the rounding of z to T that the exact bounds zlo / zhi refer to.
struct DenseScreenEntry {
    int re;
    float rf, a, b;
};
constexpr int kDenseMax = 128;
constexpr int kDenseMin = 16;     // listed pixels of a wave from which the wave is searched as a whole (65 = never)
struct DenseScreen {
    DenseScreenEntry e[kDenseMax + 1];
};

// (T: the kernels' data type; defined for float and double in omnibus_tables.hip)
template <typename T>
DenseScreenEntry make_dense_entry(const OmniTabEntry &t, int j, double n_looks);
template <typename T>
DenseScreen make_dense_screen(const std::vector<OmniTabEntry> &tab, int k, double n_looks);

typedef float f2_t __attribute__((ext_vector_type(2)));

// ---- constants of the streaming search (omnibus.hip: omnibus_c2_stream_kernel) -----------------
// The kernel walks the dates last to first, so the global test it meets at step jj = 1, 2, ... is
// the one over jj dates whatever k is: entry jj is read with one scalar load from the kernel's
// argument segment (a wave-uniform index into a by-value argument compiles to s_load_dwordx8), no
// vector instruction, no LDS.  jf / cj / mj are the wave-uniform factors of the rounding band of
// that test (see the kernel), precomputed so that they cost no conversions on the device.
struct StreamEntry {
    int re;
    float rf, a, b;     // as DenseScreenEntry
    float jf;           // (float) jj
    float cj;           // 1.46 * 5 u * jj:  rel = cj * s11 s22 / det
    float mj;           // 1.01 * jj:        band = mj * rel
    float pad;
};
// The 2- and 3-date marginal tests are decided without logarithms: with L2 = log2(prod det_t) -
// j log2 det(sum),  L2 < Lhi  <=>  prod det_t < 2^Lhi det(sum)^j.  The products of two or three
// determinants are formed in `floating` (each determinant inside [dlo, dhi], so the product is a
// normal number with j - 1 roundings), det(sum)^j with j - 1 roundings, the constant with one:
// <= 6 half-ulps, 4.3e-7 in log2 units at float32; the constants carry a margin of 4e-6.
//   prod < ca_j * det(sum)^j  =>  the test fires for certain;  prod > cb_j * det(sum)^j  =>  it cannot.
// A right-hand side that underflows is harmless (the product is a normal number, larger than
// anything that underflows: both verdicts are then true statements); overflow is excluded by
// det(sum) < dhi and ca, cb <= 64.
template <int NJ>
struct StreamScreen {
    StreamEntry e[NJ + 1];
    f2_t ca, cb;          // .x: the 2-date test, .y: the 3-date test (pairs: operands of packed multiplications)
    float dlo, dhi;       // a date's determinant and those of the 2- / 3-date sums: strictly inside (dlo, dhi)
    // the same constants in a longer table (entries beyond NJ: for the caller to fill)
    template <int NJ2>
    StreamScreen<NJ2> widen() const
    {
        static_assert(NJ2 >= NJ, "widen");
        StreamScreen<NJ2> w;
        memset(&w, 0, sizeof(w));
        for (int j = 0; j <= NJ; ++j) w.e[j] = e[j];
        w.ca = ca;
        w.cb = cb;
        w.dlo = dlo;
        w.dhi = dhi;
        return w;
    }
};

template <typename T>
void stream_marginal_bounds(const OmniTabEntry &t, int j, double n_looks, float *ca, float *cb);

template <typename T, int NJ>
static StreamScreen<NJ> make_stream_screen(const std::vector<OmniTabEntry> &tab, const DenseScreen &scr,
                                           int k, double n_looks)
{
    StreamScreen<NJ> s;
    memset(&s, 0, sizeof(s));
    const float cu = (sizeof(T) == 4 ? 5.9604645e-08f : 1.1102230e-16f) * 7.5f;   // 1.46 * 5 u, rounded up
    for (int j = 0; j <= NJ; ++j) {
        s.e[j].re = scr.e[j].re;
        s.e[j].rf = scr.e[j].rf;
        s.e[j].a = scr.e[j].a;
        s.e[j].b = scr.e[j].b;
        s.e[j].jf = (float)j;
        s.e[j].cj = cu * (float)j;
        s.e[j].mj = (float)j * 1.01f;
    }
    float ca2 = 0.f, ca3 = 0.f, cb2 = INFINITY, cb3 = INFINITY;
    if (k >= 2) stream_marginal_bounds<T>(tab[2], 2, n_looks, &ca2, &cb2);
    if (k >= 3) stream_marginal_bounds<T>(tab[3], 3, n_looks, &ca3, &cb3);
    s.ca.x = ca2;
    s.ca.y = ca3;
    s.cb.x = cb2;
    s.cb.y = cb3;
    // float32: the determinants of a date and of the 2- / 3-date sums inside 2^+-36 (a product of
    // three stays a normal number, 2^+-108; a cube times a constant <= 64 stays finite); float64:
    // 2^+-100.  Pixels outside go to the exact pass.  The running double product of the determinants
    // then moves by at most 36 (100) binary orders per date: see the kernel's range check.
    if (sizeof(T) == 4) {
        s.dlo = 1.4551915228366852e-11f;     // 2^-36
        s.dhi = 68719476736.f;               // 2^36
    } else {
        s.dlo = 7.888609052210118e-31f;      // 2^-100
        s.dhi = 1.2676506002282294e30f;      // 2^100
    }
    return s;
}

}  // namespace nd_amd
