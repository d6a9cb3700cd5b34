// nd_amd/csrc/omnibus_search.hpp -- the sequential segment search (nd/_change.pyx:235-257) as the kernels of
// every omnibus family run it, written once.  Device code only; included by omnibus_c2_device.hpp (dual pol),
// omnibus_c3.hip (full pol) and omnibus_diag.hip (intensities only).
//
// The search of one pixel is ONE SWEEP PER SEGMENT.  The reference first asks the global test over ts[l:], then the
// marginal ones over ts[l:l+j], j = 2, 3, ...; both are functions of the same running accumulation started at l (the
// global test is its state after the last date), so a lane folds the dates l .. k-1 once, remembers the first date
// whose marginal test fires and commits it only if the global test -- known behind the last date -- fires too.
// The pieces:
//   accumulator   Accum<T> (2 x 2), Accum3<T> (3 x 3), DiagAccum<T, Q> (Q intensities): the reference's sums in T and
//                 its double product of the determinants; step(), det_of_sum(), kDof = degrees of freedom per date
//   z_stat / z_approx   the statistic of the test over the j dates folded into an accumulator, exact / for the screen
//   table views   the per-j constants where a kernel keeps them: TabGlobal, TabOne, TabLds, ScreenLds
//   test_f64 / test_f32   one test: the screen, and the exact evaluation of what the screen cannot decide
//   Sweep         the per-lane state of the search: segment start, first firing date, the end-of-sweep commit
//   follow_starts_chain   the tail of the one-lane-per-segment-start forms
//   search_rounds the sweep in lockstep rounds on a blocked dump, for any accumulator and dump layout
#pragma once

#include "omnibus_common.hpp"

namespace nd_amd {

// ---- the reference's running state of one segment (nd/_change.pyx:53-69) ----------------------------
template <typename T>
struct Accum {
    typedef T value_type;
    static constexpr int kDof = 4;
    T s11, s12r, s12i, s22;
    double prod;
    __device__ __forceinline__ void reset()
    {
        s11 = 0;
        s12r = 0;
        s12i = 0;
        s22 = 0;
        prod = 1.0;
    }
    __device__ __forceinline__ void step(T a, T b, T c, T d)
    {
        const T det = (a * d) - ((b * b) + (c * c));
        prod = prod * (double)det;
        s11 = s11 + a;
        s12r = s12r + b;
        s12i = s12i + c;
        s22 = s22 + d;
    }
    __device__ __forceinline__ T det_of_sum() const { return (s11 * s22) - ((s12r * s12r) + (s12i * s12i)); }
};

// det C = abc - a|z|^2 - b|y|^2 - c|x|^2 + 2 Re(x z conj(y)), left to right in T; v = [C11, C22, C33, C12re, C12im,
// C13re, C13im, C23re, C23im]
template <typename T>
__device__ __forceinline__ T det3(const T (&v)[9])
{
    const T a = v[0], b = v[1], c = v[2];
    const T xr = v[3], xi = v[4], yr = v[5], yi = v[6], zr = v[7], zi = v[8];
    const T re = (((xr * zr) - (xi * zi)) * yr) + (((xr * zi) + (xi * zr)) * yi);
    return (((((a * b) * c) - (a * ((zr * zr) + (zi * zi)))) - (b * ((yr * yr) + (yi * yi)))) -
            (c * ((xr * xr) + (xi * xi)))) +
           ((T)2 * re);
}

template <typename T>
struct Accum3 {
    typedef T value_type;
    static constexpr int kDof = 9;
    T s[9];
    double prod;
    __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int c = 0; c < 9; ++c) s[c] = 0;
        prod = 1.0;
    }
    __device__ __forceinline__ void step(const T (&v)[9])
    {
        prod = prod * (double)det3<T>(v);
#pragma unroll
        for (int c = 0; c < 9; ++c) s[c] = s[c] + v[c];
    }
    __device__ __forceinline__ T det_of_sum() const { return det3<T>(s); }
};

// Q independent 1 x 1 blocks: the determinant of a date is the product of its intensities
template <typename T, int Q>
struct DiagAccum {
    typedef T value_type;
    static constexpr int kDof = Q;
    T s[Q];
    double prod;
    __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int c = 0; c < Q; ++c) s[c] = (T)0;
        prod = 1.0;
    }
    __device__ __forceinline__ void step(const T (&v)[Q])
    {
        T det = v[0];
#pragma unroll
        for (int c = 1; c < Q; ++c) det = det * v[c];
        prod = prod * (double)det;
#pragma unroll
        for (int c = 0; c < Q; ++c) s[c] = s[c] + v[c];
    }
    __device__ __forceinline__ T det_of_sum() const
    {
        T d = s[0];
#pragma unroll
        for (int c = 1; c < Q; ++c) d = d * s[c];
        return d;
    }
};

// ---- the statistic ----------------------------------------------------------------------------------
// z = -2 rho ln Q over the j dates folded into A (nd/_change.pyx:72-76), rounded to T as the reference does
template <typename Acc>
__device__ __forceinline__ typename Acc::value_type z_stat(const Acc &A, int j, double nlooks, double m2rho,
                                                           double pklogk)
{
    typedef typename Acc::value_type T;
    const T det_of_sum = A.det_of_sum();
    const double logQ = nlooks * ((pklogk + log(A.prod)) - ((double)j * log((double)det_of_sum)));
    return (T)(m2rho * logQ);
}

// Screen statistic: z from approx_ln.  |z_approx - z| <= |m2rho| n (k+1) 1e-7; the host widens zlo_a / zhi_a by ten
// times that, so z_approx < zlo_a implies z < zlo (make_entry, omnibus_tables.hip).
template <typename Acc>
__device__ __forceinline__ double z_approx(const Acc &A, int j, double nlooks, double m2rho, double pklogk)
{
    typedef typename Acc::value_type T;
    const T det_of_sum = A.det_of_sum();
    const double logQ = nlooks * ((pklogk + approx_ln(A.prod)) - ((double)j * approx_ln((double)det_of_sum)));
    return m2rho * logQ;
}

// ---- the per-j constants as a kernel reads them -------------------------------------------------------
// in global memory, as the host built them
struct TabGlobal {
    const OmniTabEntry *p;
    __device__ __forceinline__ double m2rho(int j) const { return p[j].m2rho; }
    __device__ __forceinline__ double pklogk(int j) const { return p[j].pklogk; }
    __device__ __forceinline__ double zlo_a(int j) const { return p[j].zlo_a; }
    __device__ __forceinline__ double zhi_a(int j) const { return p[j].zhi_a; }
    __device__ __forceinline__ OmniTabEntry entry(int j) const { return p[j]; }
};
// the one entry pass A needs, from the kernel's arguments
struct TabOne {
    const OmniTabEntry &e;
    __device__ __forceinline__ double m2rho(int) const { return e.m2rho; }
    __device__ __forceinline__ double pklogk(int) const { return e.pklogk; }
    __device__ __forceinline__ double zlo_a(int) const { return e.zlo_a; }
    __device__ __forceinline__ double zhi_a(int) const { return e.zhi_a; }
    __device__ __forceinline__ OmniTabEntry entry(int) const { return e; }
};
// in LDS, field by field (lanes at different j read different banks): field f of entry j at p[f * kp + j],
// f in the order of OmniTabEntry
struct TabLds {
    const double *p;
    int kp;
    __device__ __forceinline__ double m2rho(int j) const { return p[j]; }
    __device__ __forceinline__ double pklogk(int j) const { return p[kp + j]; }
    __device__ __forceinline__ double zlo_a(int j) const { return p[5 * kp + j]; }
    __device__ __forceinline__ double zhi_a(int j) const { return p[7 * kp + j]; }
    __device__ __forceinline__ OmniTabEntry entry(int j) const
    {
        OmniTabEntry e;
        e.m2rho = p[j];
        e.pklogk = p[kp + j];
        e.omega2 = p[2 * kp + j];
        e.lgam = p[3 * kp + j];
        e.zlo = p[4 * kp + j];
        e.zlo_a = p[5 * kp + j];
        e.zhi = p[6 * kp + j];
        e.zhi_a = p[7 * kp + j];
        return e;
    }
};
// The four constants of the double screen alone, in LDS: every lane looks up its own j at every date, so they sit
// as four arrays of doubles -- consecutive j in consecutive banks (as 64-byte records all j of one parity would
// share a bank).  The full records stay in global memory for the rare exact evaluation.
struct ScreenLds {
    const double *p;
    int kp;
    __device__ __forceinline__ double m2rho(int j) const { return p[j]; }
    __device__ __forceinline__ double pklogk(int j) const { return p[kp + j]; }
    __device__ __forceinline__ double zlo_a(int j) const { return p[2 * kp + j]; }
    __device__ __forceinline__ double zhi_a(int j) const { return p[3 * kp + j]; }
};
// entries 0 .. k of `tab` into the 4 (k + 1) doubles at scr, by the 64 lanes of a wave; the caller's barrier
// stands between this and the first look-up
__device__ __forceinline__ ScreenLds stage_screen(double *scr, const OmniTabEntry *tab, const int k, const int lane)
{
    const int kp = k + 1;
    for (int j = lane; j <= k; j += 64) {
        const OmniTabEntry e = tab[j];
        scr[j] = e.m2rho;
        scr[kp + j] = e.pklogk;
        scr[2 * kp + j] = e.zlo_a;
        scr[3 * kp + j] = e.zhi_a;
    }
    return ScreenLds{scr, kp};
}

// ---- one test ---------------------------------------------------------------------------------------------
// What a screen leaves undecided (`inband`) is evaluated exactly: the statistic with two double logarithms, zlo / zhi,
// and between those the chi-square pair.  It sits behind a wave-uniform branch so that the compiler cannot fold it
// into the body of the sweep: ~1e-5 of the tests need it, the body runs for all of them.
template <typename Acc>
__device__ __forceinline__ bool exact_tail(bool fires, const bool inband, const Acc &A, const int jj,
                                           const double nlooks, const double alpha, const OmniTabEntry *full_table)
{
    if (__any(inband)) {
        if (inband) {
            const OmniTabEntry e = full_table[jj];
            fires = exact_verdict<typename Acc::value_type>(z_stat(A, jj, nlooks, e.m2rho, e.pklogk),
                                                            Acc::kDof * (jj - 1), e, alpha);
        }
    }
    return fires;
}

// Does the test over the jj dates folded into A fire?  `need`: this lane asks it (the others answer false and only
// take part in the wave-uniform branch).  The double screen: z from the hardware log2 against the widened bounds of
// `view`: above zhi_a it fires for certain, below zlo_a (or NaN: both compares false) it cannot.
template <typename Acc, typename View>
__device__ __forceinline__ bool test_f64(const bool need, const Acc &A, const int jj, const double nlooks,
                                         const double alpha, const View &view, const OmniTabEntry *full_table)
{
    bool fires = false, inband = false;
    if (need) {
        const double za = z_approx(A, jj, nlooks, view.m2rho(jj), view.pklogk(jj));
        fires = (za > view.zhi_a(jj)) && (za < INFINITY);
        inband = (za >= view.zlo_a(jj)) && !fires;
    }
    return exact_tail(fires, inband, A, jj, nlooks, alpha, full_table);
}

// The float32 screen of dense_chain's second pass (omnibus_c2_device.hpp): x = log2(prod det) - j log2(det of sum)
// relative to the decision point, from the exponents and the hardware log2 of the mantissas of the reference's own
// running values, against the per-j band of make_dense_entry (scr[jj]; p-agnostic).  Undecided: the band, a
// non-positive or non-finite determinant of the sum, a product that is not a positive normal double (its logarithm
// would be meaningless here, and the reference's own log() of it is what the exact evaluation forms).
template <typename Acc>
__device__ __forceinline__ bool test_f32(const bool need, const Acc &A, const int jj, const double nlooks,
                                         const double alpha, const DenseScreenEntry *scr, const OmniTabEntry *full_table)
{
    typedef typename Acc::value_type T;
    bool fires = false, inband = false;
    if (need) {
        const T dets = A.det_of_sum();
        const bool ok = (dets > (T)0) & (dets < (T)INFINITY) & __builtin_amdgcn_class(A.prod, 0x100);
        const DenseScreenEntry c = scr[jj];
        int es, eP;
        float ms, mP;
        log2_parts(ok ? dets : (T)1, es, ms);
        log2_parts(ok ? A.prod : 1.0, eP, mP);
        const int E = (eP - c.re) - __mul24(jj, es);
        const float x = (float)E + __builtin_fmaf(-(float)jj, ms, mP - c.rf);
        fires = ok & (x < c.a);
        inband = !(fires | (ok & (x > c.b)));
    }
    return exact_tail(fires, inband, A, jj, nlooks, alpha, full_table);
}

// ---- the per-lane state of the search ---------------------------------------------------------------------
// A lane is in the segment that starts at l.  While it folds the dates of ts[l:] it asks the marginal test over
// j = 2, 3, ... dates until one fires (fire_at), and at the last date the global test of the segment, whose
// evaluation is the same one.  t: the next date to fold, for the forms in which a lane walks its own
// dates (the lockstep forms share one date per wave).
struct Sweep {
    int l, t, fire_at;
    bool done;
    __device__ __forceinline__ void begin(const bool active)
    {
        l = 0;
        t = 0;
        fire_at = -1;
        done = !active;
    }
    // is the test over jj dates asked?  A marginal test while none has fired yet (j >= 2); at the last date the
    // same evaluation is the global test, needed even if a marginal one fired earlier.
    __device__ __forceinline__ bool need(const int jj, const bool last) const
    {
        return (jj >= 2) && (fire_at < 0 || last);
    }
    // the answer of the test asked at date `at` (false where none was asked): the first firing date is kept
    __device__ __forceinline__ void note(const bool fires, const int at)
    {
        if (fires && fire_at < 0) fire_at = at;
    }
    // Behind the last date of the sweep; gfires: the answer of the test asked there, the global test of ts[l:]
    // (false for a segment of one date: need() asks none).  It fired: a change at the first date whose marginal test
    // fired -- fire(fire_at), :252, l + r with r = j - 1 -- and the next segment starts there (:255) unless that is
    // the last date (:256), with the accumulator A empty again.  It did not: the search is over (:241-242).
    template <typename Acc, typename Fire>
    __device__ __forceinline__ void commit(const bool gfires, const int k, Acc &A, Fire fire)
    {
        if (gfires) {
            fire(fire_at);                     // :252
            l = fire_at;                       // :255
            if (l >= k - 1) {
                done = true;                   // :256
            } else {
                A.reset();
                t = l;
                fire_at = -1;
            }
        } else {
            done = true;                       // :241-242
        }
    }
};

// ---- one lane per segment start: the chain behind the sweeps ----------------------------------------------------
// Lane l0 of a pixel's group of nsw lanes has swept ts[l:] for l = l0 + 64 u, u < NSWEEP: nxt[u] = the date of the
// first firing marginal test if the global test over ts[l:] fires, -1 (stop) otherwise.  The pixel's changes are the
// chain 0 -> nxt(0) -> nxt(nxt(0)) ..., followed here through wave shuffles by every lane of the group alike;
// `writer` (the group's first lane, of a listed pixel) stores them into the pixel's zero-filled row `res`.
// ns = k - 1 segment starts; grp: the group's number in the wave.
template <int NSWEEP>
__device__ __forceinline__ void follow_starts_chain(const int (&nxt)[NSWEEP], const int ns, const int nsw, const int grp,
                                                    const bool writer, uint8_t *res)
{
    int at = 0;
    for (int step = 0; step < ns; ++step) {
        // every chain of the wave has ended (a typical one after two or three steps): the steps left would move nothing
        if (!__any(at >= 0 && at < ns)) break;
        const int ats = (at >= 0 && at < ns) ? at : 0;
        const int src = grp * nsw + (ats & 63) % nsw;
        int nx[NSWEEP];
#pragma unroll
        for (int u = 0; u < NSWEEP; ++u) nx[u] = __shfl(nxt[u], src);
        int n1 = nx[0];
#pragma unroll
        for (int u = 1; u < NSWEEP; ++u) n1 = (ns > 64 && ats >= 64 * u) ? nx[u] : n1;
        if (at >= 0 && at < ns) {
            if (n1 < 0) {
                at = -1;                                   // :241-242
            } else {
                if (writer) res[n1] = 1;                   // :252
                at = n1;                                   // :255; n1 = k - 1 ends the search (:256)
            }
        }
    }
}

// ---- the sweep in lockstep rounds on a blocked dump -------------------------------------------------------------
// The 64 listed pixels of a wave are a BLOCK of the dump -- their series interleaved -- and the date index is
// wave-uniform: a round walks the dates from the earliest segment start among the wave's unfinished pixels to the
// end, whole contiguous kilobytes per date, every lane folding from its own segment start on; behind the last date a
// lane commits (Sweep::commit) and starts its next segment; rounds repeat while a lane has a segment left.  Screen:
// test_f32.  n: entries of the shard's list that lie in the dump; block(base) -> Loader of the 64 entries from `base`.
// A Loader hands out the dates four at a time:
//   kGrouped         the dump is read in aligned groups of four dates (a round then starts inside a group)
//   prime(t0, k)     before a round that starts at date t0
//   group(tb, k)     before the dates tb .. tb + 3
//   fold(A, u, t, k, on)   date t = tb + u: into A where `on`; may put a later date in flight in its place
template <typename Acc, typename MakeLoader>
__device__ __forceinline__ void search_rounds(const int k, const uint32_t n, const uint32_t *list,
                                              const unsigned lblock, const unsigned nlblock, uint8_t *change,
                                              const double nlooks, const double alpha, const DenseScreenEntry *scr,
                                              const OmniTabEntry *full_table, const int lane, MakeLoader block)
{
    for (uint32_t base = lblock * 64u; base < n; base += nlblock * 64u) {
        const uint32_t idx = base + lane;
        const bool active = idx < n;
        const int64_t pix = active ? (int64_t)list[idx] : 0;
        auto ld = block(base);
        typedef decltype(ld) Loader;
        uint8_t *res = change + pix * (int64_t)k;
        Acc A;
        A.reset();
        Sweep sw;
        sw.begin(active);
        while (__any(!sw.done)) {
            // the round starts at the earliest segment start among the unfinished lanes
            int t0 = sw.done ? k : sw.l;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int o = __shfl_xor(t0, off);
                t0 = o < t0 ? o : t0;
            }
            t0 = __builtin_amdgcn_readfirstlane(t0);
            bool gfires = false;                                 // of the test met at the last date: the global test
            ld.prime(t0, k);
            for (int tb = Loader::kGrouped ? (t0 & ~3) : t0; tb < k; tb += 4) {
                ld.group(tb, k);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int t = tb + u;                        // wave-uniform
                    if (t < k && (!Loader::kGrouped || t >= t0)) {
                        const bool on = !sw.done && t >= sw.l;
                        ld.fold(A, u, t, k, on);
                        const int jj = t - sw.l + 1;
                        const bool last = (t == k - 1);
                        const bool need = on && sw.need(jj, last);
                        const bool f = test_f32(need, A, jj, nlooks, alpha, scr, full_table);
                        if (need) {
                            sw.note(f, t);
                            if (last) gfires = f;
                        }
                    }
                }
            }
            if (!sw.done) sw.commit(gfires, k, A, [&](const int at) { res[at] = 1; });
        }
    }
}

}  // namespace nd_amd
