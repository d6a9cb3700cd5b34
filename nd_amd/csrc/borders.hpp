// nd_amd/csrc/borders.hpp -- the border index maps of the filter families, written once: where position cc of an
// array of len elements, extended beyond its ends, is read from.  Plain C++: no HIP header, so the kernels
// inline them and a CPU checks them exhaustively (tools/check_borders.cpp, tests/test_borders_cpu.py).
//
// scipy.ndimage extends an array by two rules.  They agree within one array length of the array
// (-len <= cc < 2 len) and are different functions further out.
//
//   extend_line    NI_ExtendLine (ni_support.c), the rule of the 1-D filters (correlate1d, gaussian_filter):
//                  exactly periodic at any distance from the array.
//                      reflect  d c b a | a b c d | d c b a      (period 2 len)
//                      mirror     d c b | a b c d | c b a        (period 2 len - 2)
//                      wrap     a b c d | a b c d | a b c d      (period len)
//                      nearest  a a a a | a b c d | d d d d
//                      constant         | a b c d |              -1: the caller serves cval
//                  Callers: correlate1d_kernel, correlate1d_tiled_kernel, correlate1d_yx_kernel (correlate.hip).
//                  Its reflect case alone: reflect_line (speckle.hip) and, without a division, ml_reflect
//                  (omnibus_ml.hip).
//   extend_index   NI_InitFilterOffsets (ni_support.c), the offset table of the N-D filters (correlate, convolve):
//                  the same pictures by other arithmetic.  Callers: correlate_kernel, correlate_tiled_kernel,
//                  correlate_roll_kernel (correlate.hip).
//                  NOT PERIODIC in one place: reflect at cc = -2 m len (m >= 2, len >= 2; the first is -4 len) gives
//                  -1, which the callers serve as cval, where the picture has element 0.  scipy's table holds the
//                  same -1 there and uses it as an index: it reads the 8 bytes in front of the array.  A window
//                  reaches that far only with a radius of 4 len and more.  Recorded behaviour, pinned by the test
//                  as exactly this set; not corrected here.
//
// CLAMP = false returns -1 for "serve cval" (constant mode).  CLAMP = true is the form of the register-window
// kernels, which do not take the constant mode: the result always lies inside the array, so that a position
// nobody uses is still a valid address.  I is the integer type: int64_t, or int where the host has checked
// len < 2^30 (the row loops hold many inlined copies, and 64-bit divisions made most of their code).
//
//   reflect_once   the single whole-sample reflection of non-local means, nd/_filters.pyx:34-40 EDGE_MODE_REFLECT.
#pragma once

#include <stdint.h>

#include "../../include/nd_amd.h"

#ifdef __HIPCC__
#define ND_AMD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ND_AMD_HD static inline
#endif

namespace nd_amd {

template <typename I, bool CLAMP>
ND_AMD_HD I extend_index(I cc, const I len, const int mode)
{
    if (cc >= 0 && cc < len) return cc;
    I m = CLAMP ? 0 : -1;                   // constant
    if (!CLAMP || len > 1) switch (mode) {
    case ND_AMD_MODE_REFLECT: {
        if (!CLAMP && len <= 1) return 0;
        const I sz2 = 2 * len;
        if (cc < 0) {
            if (cc < -sz2) cc += sz2 * (-cc / sz2);
            m = cc < -len ? cc + sz2 : -cc - 1;
        } else {
            cc -= sz2 * (cc / sz2);
            m = cc >= len ? sz2 - cc - 1 : cc;
        }
        break;
    }
    case ND_AMD_MODE_NEAREST:
        m = cc < 0 ? 0 : len - 1;
        break;
    case ND_AMD_MODE_MIRROR: {
        if (!CLAMP && len <= 1) return 0;
        const I sz2 = 2 * len - 2;
        if (cc < 0) {
            cc = sz2 * (-cc / sz2) + cc;
            m = cc <= 1 - len ? cc + sz2 : -cc;
        } else {
            cc -= sz2 * (cc / sz2);
            m = cc >= len ? sz2 - cc : cc;
        }
        break;
    }
    case ND_AMD_MODE_WRAP: {
        if (!CLAMP && len <= 1) return 0;
        if (cc < 0) {
            cc += len * (-cc / len);
            if (cc < 0) cc += len;
            m = cc;
        } else {
            m = cc - len * (cc / len);
        }
        break;
    }
    }
    return !CLAMP ? m : (m < 0 ? 0 : (m >= len ? len - 1 : m));
}

// The two forms keep a switch of their own.  One switch for both was tried with and without the constant mode's
// empty case: with it the compiler lays out the blocks of correlate1d_yx_kernel in another order, without it
// those of correlate1d_tiled_kernel (profiles/borders_codeobj.txt).  The cases are the same statements.
template <typename I, bool CLAMP>
ND_AMD_HD I extend_line(const I cc, const I len, const int mode)
{
    if (cc >= 0 && cc < len) return cc;
    if constexpr (CLAMP) {
        I m = 0;
        if (len > 1) switch (mode) {
        case ND_AMD_MODE_REFLECT: {
            const I p = 2 * len;
            m = cc % p;
            if (m < 0) m += p;
            m = m < len ? m : p - 1 - m;
            break;
        }
        case ND_AMD_MODE_NEAREST:
            m = cc < 0 ? 0 : len - 1;
            break;
        case ND_AMD_MODE_MIRROR: {
            const I p = 2 * len - 2;
            m = cc % p;
            if (m < 0) m += p;
            m = m < len ? m : p - m;
            break;
        }
        case ND_AMD_MODE_WRAP: {
            m = cc % len;
            if (m < 0) m += len;
            break;
        }
        }
        return m < 0 ? 0 : (m >= len ? len - 1 : m);
    } else {
        switch (mode) {
        case ND_AMD_MODE_REFLECT: {
            const I p = 2 * len;
            I m = cc % p;
            if (m < 0) m += p;
            return m < len ? m : p - 1 - m;
        }
        case ND_AMD_MODE_CONSTANT:
            return -1;
        case ND_AMD_MODE_NEAREST:
            return cc < 0 ? 0 : len - 1;
        case ND_AMD_MODE_MIRROR: {
            if (len <= 1) return 0;
            const I p = 2 * len - 2;
            I m = cc % p;
            if (m < 0) m += p;
            return m < len ? m : p - m;
        }
        case ND_AMD_MODE_WRAP: {
            I m = cc % len;
            if (m < 0) m += len;
            return m;
        }
        }
        return -1;
    }
}

// extend_line's reflect case with the mode folded in (the windows of the speckle filters may be larger than the plane)
ND_AMD_HD int64_t reflect_line(int64_t i, int64_t n)
{
    if ((uint64_t)i < (uint64_t)n) return i;
    const int64_t m = 2 * n;
    int64_t p = i % m;
    if (p < 0) p += m;
    return p < n ? p : m - 1 - p;
}

// the same map without a division
ND_AMD_HD int ml_reflect(int cc, const int len)
{
    if (cc >= 0 && cc < len) return cc;
    const int sz2 = 2 * len;
    // (no division: the columns asked for lie within a tile of the raster, the loops run at most a
    //  few times, and only for rasters narrower than a tile)
    while (cc < -len) cc += sz2;
    while (cc >= sz2) cc -= sz2;
    if (cc < 0) return -cc - 1;
    if (cc >= len) return sz2 - cc - 1;
    return cc;
}

// d c b | a b c d | c b a, one reflection only: defined for -n < i < 2 n - 1.  R is the type the caller computes
// in (each branch is converted on its own, as the two functions this replaces did).
template <typename R>
ND_AMD_HD R reflect_once(const int64_t i, const int64_t n)
{
    if (i < 0) return (R)(-i);
    if (i >= n) return (R)(2 * n - 2 - i);
    return (R)i;
}

}  // namespace nd_amd
