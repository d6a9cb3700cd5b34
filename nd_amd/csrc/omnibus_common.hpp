// nd_amd/csrc/omnibus_common.hpp -- device pieces shared by the omnibus kernels of every family (dual pol:
// omnibus.hip, full pol: omnibus_c3.hip, intensity only: omnibus_diag.hip): the chi-square pair, the
// approximate logarithm of the screen, the steps every kernel form repeats -- and the host prologue of the
// families' entry points.  The per-test constant table and the screens the kernels read are built on the
// host by omnibus_tables.hpp / .hip.
#pragma once

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "common.hpp"
#include "memops.hpp"
#include "omnibus_tables.hpp"

namespace nd_amd {

// 2/m, i.e. the reciprocal of the (half-)integer m/2, for the incomplete-gamma recurrences.
// For even m this is bit-for-bit 1/(m/2).
constexpr int kInvTab = 4096;
struct InvTab {
    double v[kInvTab];
    constexpr InvTab() : v()
    {
        v[0] = 0.0;
        for (int i = 1; i < kInvTab; ++i) v[i] = 2.0 / (double)i;
    }
};
static __constant__ InvTab c_inv2 = InvTab();

__device__ __forceinline__ double inv_half(int m2)   // 1 / (m2 / 2)
{
    return m2 < kInvTab ? c_inv2.v[m2] : 2.0 / (double)m2;
}

// P1 = P(a, z/2), P2 = P(a + 2, z/2) for a = a2/2 (integer or half-integer), N values in lockstep.
//   t_a = x^a e^-x / Gamma(a+1)
//   x <  a+1 :  P(a,x) = t_a * sum_{n>=0} x^n / ((a+1)...(a+n)),  P(a+2,x) = t_a * sum_{n>=2} ...
//   x >= a+1 :  Q(a,x) = t_{a-1} * sum_m (a-1)...(a-m) / x^m  over the factors >= 1
//               (+ erfc(sqrt x) when a is a half-integer),     Q(a+2,x) = Q(a,x) + t_a + t_{a+1}
// Both sums have decreasing positive terms; one loop serves both, four terms per trip, the
// reciprocals of the next trip fetched while this one computes.
// a2 = 4 (j-1) for dual pol (a integer: the gsl_cdf_chisq_P(z, f), (z, f+4) pair of
// nd/_change.pyx:147-148), 9 (j-1) for full pol.
template <int N>
__device__ __forceinline__ void chisq_pair(const double (&z)[N], int a2, double lgam_a1,
                                           double (&P1)[N], double (&P2)[N])
{
    double x[N], ta[N], rx[N], u1[N], term[N], sum[N];
    bool lower[N], ok[N];
    const double a = 0.5 * (double)a2;
    const double ap1 = a + 1.0;
    const double inv_ap1 = inv_half(a2 + 2);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        ok[i] = (z[i] > 0.0) && (z[i] < INFINITY);
        x[i] = ok[i] ? 0.5 * z[i] : 1.0;
        lower[i] = x[i] < ap1;
        ta[i] = exp(fma(a, log(x[i]), -x[i]) - lgam_a1);
        rx[i] = 1.0 / x[i];
        u1[i] = x[i] * inv_ap1;
        term[i] = lower[i] ? u1[i] : 1.0;
        sum[i] = lower[i] ? 0.0 : 1.0;
    }
    double inv_cur[4], inv_nxt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) inv_cur[u] = inv_half(a2 + 4 + 2 * u);
    for (int n = 1; n < 4000000; n += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) inv_nxt[u] = inv_half(a2 + 2 * (n + 4 + u) + 2);
        bool more = false;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d2 = a2 - 2 * (n + u);                 // 2 (a - m)
            const double up = d2 >= 2 ? 0.5 * (double)d2 : 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const double ratio = lower[i] ? x[i] * inv_cur[u] : up * rx[i];
                term[i] = term[i] * ratio;
                sum[i] = sum[i] + term[i];
                if (u == 3) more = more || (term[i] > 1e-17 * sum[i]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) inv_cur[u] = inv_nxt[u];
        if (!__any(more)) break;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double p1, p2;
        if (lower[i]) {
            p1 = ta[i] * ((1.0 + u1[i]) + sum[i]);
            p2 = ta[i] * sum[i];
        } else {
            double qa = (ta[i] * a * rx[i]) * sum[i];
            if (a2 & 1) qa = qa + erfc(sqrt(x[i]));
            p1 = 1.0 - qa;
            p2 = 1.0 - (qa + ta[i] + ta[i] * u1[i]);
        }
        if (!ok[i]) {
            // gsl_cdf_chisq_P (GSL cdf/gamma.c: gsl_cdf_gamma_P): x <= 0 -> 0 before anything is
            // evaluated; NaN stays NaN; +inf -> NaN (y > a -> 1 - gsl_sf_gamma_inc_Q, whose
            // large-x form evaluates exp(a ln x - x - ...) = exp(inf - inf); the branch list is
            // next to orc_cdf_chisq_P in oracle/nd_oracle.c)
            p1 = p2 = (z[i] <= 0.0) ? 0.0 : NAN;
        }
        P1[i] = p1;
        P2[i] = p2;
    }
}

// Cheap stand-in for ln used only to screen: ln x = (exponent + log2(mantissa)) ln 2 with the
// mantissa's log2 from the hardware v_log_f32 (1 ulp on [0.5, 1), i.e. <= 6e-8 absolute).  NaN,
// +-inf and zero arguments propagate exactly as in the double evaluation, so an approximate z is
// NaN or infinite precisely when the exact one is.
__device__ __forceinline__ double approx_ln(double x)
{
    int e;
    const double m = frexp(x, &e);
    return ((double)e + (double)__log2f((float)m)) * 0.6931471805599453;
}

// P = P1 + omega2 (P2 - P1) with the reference's rounding points (nd/_change.c:6087-6089)
template <typename T>
__device__ __forceinline__ T combine_P(double P1, double P2, double omega2)
{
    const T p1 = (T)P1, p2 = (T)P2;
    const T d = p2 - p1;
    return (T)((double)p1 + (omega2 * (double)d));
}

// ---- the steps every kernel form repeats (dual pol and full pol alike) -------------------------
// P of the test whose statistic is z (already rounded to T): the chi-square pair in double and the
// reference's combination.  a2 = p^2 (j - 1): 4 (j - 1) dual pol, 9 (j - 1) full pol; the statistic
// itself (z_stat / z_stat3) stays with the caller.
template <typename T>
__device__ __forceinline__ T global_P(const T z, const int a2, const OmniTabEntry &e)
{
    double zd[1] = {(double)z}, P1[1], P2[1];
    chisq_pair<1>(zd, a2, e.lgam, P1, P2);
    return combine_P<T>(P1[0], P2[0], e.omega2);
}

// The global test with statistics: P for every pixel, the z / P rasters stored where asked for, and
// the verdict (double)P > alpha of nd/_change.pyx:241-242.  `in`: the lane owns the pixel `pix`.
template <typename T>
__device__ __forceinline__ bool global_flag_stats(const T z, const int a2, const OmniTabEntry &e,
                                                  const double alpha, const bool in, T *z_out,
                                                  T *p_out, const int64_t pix)
{
    const T P = global_P<T>(z, a2, e);
    const bool flag = in && ((double)P > alpha);
    if (in) {
        if (z_out) z_out[pix] = z;
        if (p_out) p_out[pix] = P;
    }
    return flag;
}

// The exact verdict of one test from its statistic (nd/_change.pyx:235-257 asks it at :241-242 for
// the global test of a segment and at :252 for a marginal test, whose firing starts the next segment
// at :255): cannot fire (z < zlo, or NaN), fires for certain
// (zhi < z < inf), and only inside the band between the two the chi-square pair decides.
template <typename T>
__device__ __forceinline__ bool exact_verdict(const T z, const int a2, const OmniTabEntry &e,
                                              const double alpha)
{
    const double zd = (double)z;
    // 0 = cannot fire, 1 = fires for certain, 2 = inside the exact band: needs the chi-square pair
    int verdict = !(zd >= e.zlo) ? 0 : ((zd > e.zhi && zd < INFINITY) ? 1 : 2);
    if (verdict == 2) verdict = ((double)global_P<T>(z, a2, e) > alpha) ? 1 : 0;
    return verdict == 1;
}

// Slots of a shard's list for the flagged lanes of a wave: one ballot, one atomic on the shard's
// counter word by the wave's first lane, and each flagged lane's rank among them.  The returned
// slot is valid where `flag` is set.  Called under `if (__any(flag))`: a wave without a flagged
// lane has nothing to claim and leaves the counter alone.
__device__ __forceinline__ unsigned wave_claim(const bool flag, uint32_t *counter, const int lane)
{
    const unsigned long long m = __ballot(flag);
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(counter, (unsigned)__popcll(m));
    base = __shfl(base, 0);
    return base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

// The change map is written once: the zeros bypass the cache hierarchy's retention.
__device__ __forceinline__ void store_zero16_nt(uint4 *p)
{
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const u4 z = {0u, 0u, 0u, 0u};
    __builtin_nontemporal_store(z, reinterpret_cast<u4 *>(p));
}

// Zero-fill of nb bytes of the change map at ob (np.zeros at nd/_change.pyx:275) by STRIDE threads
// numbered t = 0 .. STRIDE - 1: head bytes up to the first 16-byte boundary, 16-byte pieces, tail
// bytes.  A wave calls it with its lane, a block with STRIDE = its thread count and t = tid.
// N: type of the byte count (int wherever a block's slice is below 2 GB).
template <int STRIDE = 64, typename N = int>
__device__ __forceinline__ void zero_fill_span(uint8_t *ob, const N nb, const int t)
{
    static_assert(STRIDE >= 16, "head and tail are one byte per thread");
    N head = (N)((16 - ((uintptr_t)ob & 15)) & 15);
    if (head > nb) head = nb;
    if (t < head) ob[t] = 0;
    const N nvec = (nb - head) >> 4;
    uint4 *vz = reinterpret_cast<uint4 *>(ob + head);
    for (N i = t; i < nvec; i += STRIDE) store_zero16_nt(vz + i);
    const N tail0 = head + (nvec << 4);
    if (tail0 + t < nb) ob[tail0 + t] = 0;
}

// ---- device side of the screen (shared by the dual-pol and the full-pol kernels) ---------------
// log2 of a positive finite x as (exponent, log2 of the mantissa in [0.5, 1)): the mantissa's
// log2 comes from the hardware v_log_f32 (<= 1 ulp of a value in [-1, 0], i.e. <= 6e-8 absolute).
__device__ __forceinline__ void log2_parts(float x, int &e, float &m)
{
    m = __log2f(__builtin_frexpf(x, &e));
}
__device__ __forceinline__ void log2_parts(double x, int &e, float &m)
{
    m = __log2f((float)__builtin_frexp(x, &e));
    // (float) of a mantissa just below 1 may round to 1: log2 = 0, error < 1e-7 as budgeted
}

constexpr float kLogFix = 33554432.f;          // 2^25: fixed-point scale of the mantissa logs

struct ScreenRegs {
    int re;
    float rf, a, b;
};
__device__ __forceinline__ ScreenRegs screen_regs_load(const DenseScreenEntry *scr_lds, const int lane)
{
    const DenseScreenEntry e = scr_lds[lane + 1];          // entries 1 .. 64 in lanes 0 .. 63
    ScreenRegs r;
    r.re = e.re;
    r.rf = e.rf;
    r.a = e.a;
    r.b = e.b;
    return r;
}
__device__ __forceinline__ DenseScreenEntry screen_entry(const ScreenRegs &r, const int j)
{
    DenseScreenEntry c;
    c.re = __builtin_amdgcn_readlane(r.re, j - 1);
    c.rf = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r.rf), j - 1));
    c.a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r.a), j - 1));
    c.b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r.b), j - 1));
    return c;
}

// Lm: sum of the dates' fixed-point mantissa logs (each in [-2^25, 0]): int up to 64 dates, long long
// beyond
template <typename T, typename LmT>
__device__ __forceinline__ float dense_x(const T dets, const bool ok, const int Le, const LmT Lm,
                                         const int jj, const DenseScreenEntry &c)
{
    int es;
    float ms;
    log2_parts(ok ? dets : (T)1, es, ms);
    const int E = (Le - __mul24(jj, es)) - c.re;
    const float F = (float)Lm * (1.0f / kLogFix);
    return (float)E + ((F - c.rf) - (float)jj * ms);
}

// ---- bit masks over the dates (position t = date t) ------------------------------------------
// 32 and 64 dates: plain integers.  Up to 128 dates: two 64-bit words.
struct Bits128 {
    unsigned long long lo, hi;
};
// Up to 192 dates (round 6: the two-pass chain search of series of 129 .. 192 dates): three words.
struct Bits192 {
    unsigned long long w0, w1, w2;
};
template <typename M>
__device__ __forceinline__ M mask_zero()
{
    return (M)0;
}
template <>
__device__ __forceinline__ Bits192 mask_zero<Bits192>()
{
    return Bits192{0ull, 0ull, 0ull};
}
template <>
__device__ __forceinline__ Bits128 mask_zero<Bits128>()
{
    return Bits128{0ull, 0ull};
}
// set bit i (any i, per lane) where `on`
template <typename M>
__device__ __forceinline__ void mask_set(M &m, const int i, const bool on)
{
    m |= on ? ((M)1 << i) : (M)0;
}
__device__ __forceinline__ void mask_set(Bits128 &m, const int i, const bool on)
{
    const unsigned long long b = on ? (1ull << (i & 63)) : 0ull;
    m.lo |= i < 64 ? b : 0ull;
    m.hi |= i < 64 ? 0ull : b;
}
template <typename M>
__device__ __forceinline__ bool mask_bit(const M &m, const int i)
{
    return ((m >> i) & (M)1) != 0;
}
__device__ __forceinline__ bool mask_bit(const Bits128 &m, const int i)
{
    return (((i < 64 ? m.lo : m.hi) >> (i & 63)) & 1ull) != 0ull;
}
// m = 2 m + bit: the streaming search meets the dates last to first, so after the last push the
// bit of date t sits at position t
template <typename M>
__device__ __forceinline__ void mask_push(M &m, const bool bit)
{
    m = (m + m) + (M)(bit ? 1 : 0);
}
// 32 bits: one add-with-carry whose carry-in is the condition's lane mask (the compiler's own
// selection is v_cndmask + v_lshl_or).  The carry-out lands in a scalar pair nobody reads.
__device__ __forceinline__ void mask_push(unsigned &m, const bool bit)
{
    const unsigned long long cin = __builtin_amdgcn_ballot_w64(bit);
    unsigned long long cout;
    unsigned r;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(cout) : "v"(m), "s"(cin));
    m = r;
}
// 64 bits: two of them, the carry of the low word (a lane mask in a scalar pair) feeding the high one
__device__ __forceinline__ void mask_push(unsigned long long &m, const bool bit)
{
    const unsigned long long cin = __builtin_amdgcn_ballot_w64(bit);
    unsigned long long c1, c2;
    const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
    unsigned rlo, rhi;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(rlo), "=s"(c1) : "v"(lo), "s"(cin));
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(rhi), "=s"(c2) : "v"(hi), "s"(c1));
    m = ((unsigned long long)rhi << 32) | rlo;
}
__device__ __forceinline__ void mask_push(Bits128 &m, const bool bit)
{
    m.hi = (m.hi + m.hi) + (m.lo >> 63);
    m.lo = (m.lo + m.lo) + (bit ? 1ull : 0ull);
}
// bits 0 .. n - 1 (0 <= n <= width)
template <typename M>
__device__ __forceinline__ M mask_low(const int n)
{
    return n >= (int)(8 * sizeof(M)) ? ~(M)0 : (((M)1 << n) - (M)1);
}
template <typename M>
__device__ __forceinline__ void mask_keep_low(M &m, const int n)
{
    m &= mask_low<M>(n);
}
__device__ __forceinline__ void mask_keep_low(Bits128 &m, const int n)
{
    m.lo &= mask_low<unsigned long long>(n < 64 ? n : 64);
    m.hi &= mask_low<unsigned long long>(n < 64 ? 0 : n - 64);
}
// bits where neither "fires" nor "cannot fire" is set
template <typename M>
__device__ __forceinline__ M mask_undecided(const M &f, const M &c)
{
    return (M) ~(f | c);
}
__device__ __forceinline__ Bits128 mask_undecided(const Bits128 &f, const Bits128 &c)
{
    return Bits128{~(f.lo | c.lo), ~(f.hi | c.hi)};
}
__device__ __forceinline__ int mask_ctz(const unsigned m) { return __builtin_ctz(m); }
__device__ __forceinline__ int mask_ctz(const unsigned long long m) { return __builtin_ctzll(m); }
// ---- three-word masks ----
__device__ __forceinline__ void mask_set(Bits192 &m, const int i, const bool on)
{
    const unsigned long long b = on ? (1ull << (i & 63)) : 0ull;
    m.w0 |= i < 64 ? b : 0ull;
    m.w1 |= (i >= 64 && i < 128) ? b : 0ull;
    m.w2 |= i >= 128 ? b : 0ull;
}
__device__ __forceinline__ bool mask_bit(const Bits192 &m, const int i)
{
    return (((i < 64 ? m.w0 : (i < 128 ? m.w1 : m.w2)) >> (i & 63)) & 1ull) != 0ull;
}
__device__ __forceinline__ void mask_push(Bits192 &m, const bool bit)
{
    m.w2 = (m.w2 + m.w2) + (m.w1 >> 63);
    m.w1 = (m.w1 + m.w1) + (m.w0 >> 63);
    m.w0 = (m.w0 + m.w0) + (bit ? 1ull : 0ull);
}
__device__ __forceinline__ void mask_keep_low(Bits192 &m, const int n)
{
    m.w0 &= mask_low<unsigned long long>(n < 64 ? (n < 0 ? 0 : n) : 64);
    m.w1 &= mask_low<unsigned long long>(n < 64 ? 0 : (n < 128 ? n - 64 : 64));
    m.w2 &= mask_low<unsigned long long>(n < 128 ? 0 : n - 128);
}
__device__ __forceinline__ Bits192 mask_undecided(const Bits192 &f, const Bits192 &c)
{
    return Bits192{~(f.w0 | c.w0), ~(f.w1 | c.w1), ~(f.w2 | c.w2)};
}
__device__ __forceinline__ unsigned mask_nibble(const Bits192 &m, const int q)
{
    return (unsigned)((q < 16 ? m.w0 : (q < 32 ? m.w1 : m.w2)) >> (4 * (q & 15))) & 0xFu;
}
// bits 4 q .. 4 q + 3
template <typename M>
__device__ __forceinline__ unsigned mask_nibble(const M &m, const int q)
{
    return (unsigned)(m >> (4 * q)) & 0xFu;
}
__device__ __forceinline__ unsigned mask_nibble(const Bits128 &m, const int q)
{
    return (unsigned)((q < 16 ? m.lo : m.hi) >> (4 * (q & 15))) & 0xFu;
}

// The rows of the change map of a wave's 64 pixels are 64 k contiguous bytes.  A lane storing its
// own row writes 4-byte pieces k bytes apart -- k / 4 store instructions that each touch every
// line of the span (measured on the streaming search: 0.24 ms of a 1.3 ms launch for 0.4 GB).
// Through a wave-private LDS image (16 k words) the same bytes leave as 16-byte pieces of
// consecutive lanes.  Needs all 64 pixels, k a multiple of 4 and a 16-byte aligned span.
template <typename MT>
__device__ __forceinline__ void store_change_rows_wave(uint8_t *wob, uint32_t *img, const int k,
                                                       const MT &mask, const int lane)
{
    const int kq = k >> 2;
    for (int q = 0; q < kq; ++q)
        img[lane * kq + q] = (mask_nibble(mask, q) * 0x00204081u) & 0x01010101u;     // bit i -> byte i
    wave_lds_fence();
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const u4 *src = reinterpret_cast<const u4 *>(img);
    u4 *dst = reinterpret_cast<u4 *>(wob);
    for (int c = lane; c < 4 * k; c += 64) __builtin_nontemporal_store(src[c], dst + c);
    wave_lds_fence();                                      // the image may be written again behind this
}
__device__ __forceinline__ bool change_rows_wave_ok(const uint8_t *wob, const int k, const int wnp)
{
    return wnp == 64 && (k & 3) == 0 && ((uintptr_t)wob & 15) == 0;
}

template <typename T, typename MT>
__device__ __forceinline__ void screen_decide(const float x, const float m2, const bool sane,
                                              const DenseScreenEntry &c, const int t,
                                              MT &fbits, MT &ibits)
{
    const bool fires = sane && (x + m2 < c.a);
    const bool cant = sane && (x - m2 > c.b);
    mask_set(fbits, t, fires);
    mask_set(ibits, t, !(fires || cant));
}


// ---- the prologue of the families' *_impl functions (host) -------------------------------------
// The workspace of entry point `name`: `need` bytes (`at_least`: a larger one is put to use), 256-byte aligned.
static inline int check_workspace(const char *name, const void *workspace, size_t given, size_t need,
                                  bool at_least = false)
{
    if (workspace == nullptr || given < need) {
        set_error("%s: workspace of %s%zu bytes needed, %zu given", name, at_least ? "at least " : "", need,
                  given);
        return ND_AMD_EWORKSPACE;
    }
    if (((uintptr_t)workspace & 255) != 0) {
        set_error("%s: workspace must be 256-byte aligned", name);
        return ND_AMD_EINVAL;
    }
    return ND_AMD_OK;
}

// The table where the kernels read it: in the kernel arguments (*tab) up to kTabArgs dates, otherwise at
// tab_dev through a pageable host copy (synchronises the stream once).  *tab_in_args says which.
static inline hipError_t stage_table(const std::vector<OmniTabEntry> &htab, int64_t k, OmniTab *tab,
                                     OmniTabEntry *tab_dev, hipStream_t stream, bool *tab_in_args)
{
    memset(tab, 0, sizeof(*tab));
    *tab_in_args = k <= kTabArgs;
    if (*tab_in_args) {
        memcpy(tab->e, htab.data(), htab.size() * sizeof(OmniTabEntry));
        return hipSuccess;
    }
    const hipError_t e = hipMemcpyAsync(tab_dev, htab.data(), htab.size() * sizeof(OmniTabEntry),
                                        hipMemcpyHostToDevice, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
}


}  // namespace nd_amd
