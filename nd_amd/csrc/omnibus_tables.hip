// nd_amd/csrc/omnibus_tables.hip -- the omnibus decision tables (omnibus_tables.hpp): host arithmetic in
// double, nothing of HIP.  Built into the library like every other unit; also compiles as plain C++
// (clang++ -x c++ -std=c++17) for the dump program and the CPU test.
#include "omnibus_tables.hpp"

#include <mutex>
#include <utility>

namespace nd_amd {

static inline double host_rho(double p, double k, double n)
{
    return (1.0 - ((((2.0 * (p * p)) - 1.0) / ((6.0 * (k - 1.0)) * p)) *
                   ((k / n) - (1.0 / (n * k)))));
}

static inline double host_omega2(double p, double k, double n, double rho)
{
    return (((((p * p) * ((p * p) - 1.0)) / (24.0 * (rho * rho))) *
             ((k / (n * n)) - (1.0 / ((n * k) * (n * k))))) -
            ((((p * p) * (k - 1.0)) / 4.0) * ((1.0 - (1.0 / rho)) * (1.0 - (1.0 / rho)))));
}

// half an ulp / one ulp of 1 in the kernels' data type
static inline double half_ulp(int dtype) { return dtype == ND_AMD_F32 ? 5.9604644775390625e-08 : 1.1102230246251565e-16; }
template <typename T>
static inline double eps_of() { return sizeof(T) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16; }

// host twin of the device's chisq_pair / diag_P (N = 1, no table), used only to place the decision bounds
static void host_chisq_pair(double z, int a2, double lgam_a1, double *P1, double *P2)
{
    if (!(z > 0.0)) {
        *P1 = *P2 = (z <= 0.0) ? 0.0 : NAN;
        return;
    }
    if (!(z < INFINITY)) {
        *P1 = *P2 = NAN;
        return;
    }
    const double a = 0.5 * (double)a2;
    const double x = 0.5 * z;
    const bool lower = x < a + 1.0;
    const double ta = exp((a * log(x) - x) - lgam_a1);
    const double u1 = x / (a + 1.0);
    double term = lower ? u1 : 1.0, sum = lower ? 0.0 : 1.0;
    for (int n = 1; n < 4000000; ++n) {
        const int d2 = a2 - 2 * n;
        const double ratio = lower ? x / (a + 1.0 + (double)n) : (d2 >= 2 ? 0.5 * (double)d2 : 0.0) / x;
        term *= ratio;
        sum += term;
        if (!(term > 1e-17 * sum)) break;
    }
    if (lower) {
        *P1 = ta * ((1.0 + u1) + sum);
        *P2 = ta * sum;
    } else {
        double qa = (ta * a / x) * sum;
        if (a2 & 1) qa += erfc(sqrt(x));
        // f = 1 (one intensity channel, two dates): the descending sum has no factor >= 1, Q(1/2, x) is the
        // complementary error function alone.  4 (j - 1) and 9 (j - 1) are never 1.
        if (a2 == 1) qa = erfc(sqrt(x));
        *P1 = 1.0 - qa;
        *P2 = 1.0 - (qa + ta + ta * u1);
    }
}

// Decision bounds of the test over j matrices: every z' < zlo has P(z') <= alpha for certain and
// every finite z' > zhi has P(z') > alpha for certain, so the chi-square pair is only needed for
// zlo <= z <= zhi (and for z = +inf, whose P is NaN).
//   The kernel's P differs from the exact P(z) = P1 + omega2 (P2 - P1) by the roundings to T of P1, P2,
//   their difference and the result, plus ~1e-13 from the series: bounded by `margin` below.
//   zlo = the z where the exact P equals alpha - margin, stepped down by 1e-9 relative;
//   zhi = the z where it equals alpha + margin, stepped up by 1e-9 relative.
// 0 <= omega2 <= 1:  P is non-decreasing in z (a mixture of two chi-square CDFs); the bisection's bracket
//   grows from 2 a2 + 64.  When a target leaves (0, 1), the bound is -inf / +inf: every non-NaN z is
//   evaluated exactly.
// omega2 < 0 (`negative_ok`: the intensity-only family, where it always is):  with w = -omega2 > 0, x = z / 2,
//   a = f / 2 and t_a = x^a e^-x / Gamma(a + 1):
//     P(a, x) - P(a + 2, x) = t_a + t_{a+1},  so  P = P(a, x) + w (t_a + t_{a+1});
//     d/dx P(a, x) = t_{a-1},  d/dx t_a = t_{a-1} - t_a,  t_{a+1} = t_{a-1} x^2 / (a (a + 1)),  hence
//     dP/dx = t_{a-1} (1 + w) - w t_{a+1} = t_{a-1} (1 + w - w x^2 / (a (a + 1))).
//   P rises from 0 up to x* = sqrt(a (a + 1) (1 + 1/w)) and falls beyond it towards its limit 1, so P >= 1 on
//   [x*, inf).  For a target tau < 1 the crossing P = tau is therefore unique, lies below x*, and P < tau before
//   it, P > tau behind it: the same bisection holds with the fixed bracket [0, 2 x*].  That needs
//   alpha + margin < 1; otherwise every test is evaluated exactly -- with omega2 < 0, P passes 1, so
//   "P <= 1 < alpha: nothing fires" does not hold here either.
// Anything else (omega2 < 0 in the dual- and full-pol families, e.g. n = 1 and small j; omega2 > 1; j < 2,
// where rho is NaN): -inf / +inf.
static void omni_bounds(int j, int a2, double omega2, double lgam, double alpha, int dtype, bool negative_ok,
                        double *zlo, double *zhi)
{
    *zlo = -INFINITY;    // evaluate everything exactly
    *zhi = INFINITY;     // never accept without evaluating
    if (j < 2 || a2 < 1) return;
    const bool mixture = omega2 >= 0.0 && omega2 <= 1.0;
    const bool negative = negative_ok && omega2 < 0.0 && omega2 > -INFINITY;
    if (!(mixture || negative) || !(alpha == alpha)) return;
    // the device's double evaluation: ~1e-13 from the series, plus the prefactor
    // exp(a ln x - x - lgamma(a + 1)), whose exponent carries ~a (1 + ln a) eps of absolute
    // rounding error -- negligible at a = 2 (k - 1) <= 100, 2e-10 for series of 10^4 dates
    const double a = 0.5 * (double)a2;
    const double margin = 16.0 * half_ulp(dtype) * (1.0 + 2.0 * fabs(omega2)) + 1e-11 +
                          8.0 * a * (1.0 + log(a + 2.0)) * 1.1102230246251565e-16;
    const double tlo = alpha - margin, thi = alpha + margin;
    double zcap = 0.0;
    if (negative) {
        if (!(thi < 1.0 - 1e-9)) return;
        zcap = 4.0 * sqrt(a * (a + 1.0) * (1.0 + 1.0 / -omega2));      // z = 2 x at x = 2 x*
        if (!(zcap > 0.0) || !(zcap < INFINITY)) return;
    }
    auto Pz = [&](double z) {
        double p1, p2;
        host_chisq_pair(z, a2, lgam, &p1, &p2);
        return p1 + omega2 * (p2 - p1);
    };
    // smallest z (to 1e-15 relative) with exact P(z) >= target, as a bracketing pair lo < hi
    auto quantile = [&](double target, double *lo_out, double *hi_out) -> bool {
        double lo = 0.0, hi;
        if (negative) {
            hi = zcap;
            if (!(Pz(hi) >= target)) return false;
        } else {
            hi = 2.0 * (double)a2 + 64.0;
            int guard = 0;
            while (Pz(hi) < target && guard++ < 64) hi *= 2.0;
            if (guard >= 64) return false;
        }
        for (int it = 0; it < 200; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (Pz(mid) < target)
                lo = mid;
            else
                hi = mid;
            if (hi - lo <= 1e-15 * hi) break;
        }
        *lo_out = lo;
        *hi_out = hi;
        return true;
    };
    double lo, hi;
    if (mixture && tlo >= 1.0) {
        *zlo = INFINITY;                      // P <= 1 < alpha: nothing can fire
    } else if (mixture ? tlo >= 0.0 : tlo > 0.0) {
        if (quantile(tlo, &lo, &hi))
            *zlo = lo * (1.0 - 1e-9);
        else if (mixture)
            *zlo = INFINITY;                  // target unreachable in double
    }
    if (thi > 0.0 && thi < 1.0 - 1e-9 && quantile(thi, &lo, &hi)) *zhi = hi * (1.0 + 1e-9);
}

OmniTabEntry make_entry(int j, double n, double alpha, int dtype, OmniFamily fam)
{
    OmniTabEntry e;
    const bool f32 = dtype == ND_AMD_F32;
    const bool blocks_1x1 = fam.p == 1;               // the intensity-only family
    const double p = (double)fam.p, k = (double)j;
    const double rho = host_rho(p, k, n);             // does not depend on q
    e.m2rho = -2.0 * (f32 ? (double)(float)rho : rho);
    // `p * k` in `floating`, nd/_change.c:3580
    const int pq = fam.p * fam.q;
    const double pk = f32 ? (double)((float)pq * (float)j) : (double)pq * (double)j;
    e.pklogk = pk * log(k);
    e.omega2 = (double)fam.q * host_omega2(p, k, n, rho);   // p = 1: -(q (j - 1) / 4) (1 - 1/rho)^2 < 0
    const int a2 = omni_a2(j, fam);
    e.lgam = lgamma(0.5 * (double)a2 + 1.0);
    omni_bounds(j, a2, e.omega2, e.lgam, alpha, dtype, blocks_1x1, &e.zlo, &e.zhi);
    // bounds for the f32-log2 screen: |z_approx - z| <= |m2rho| n (j + 1) 1e-7 (4.2e-8 with 1 x 1 blocks: two
    // hardware log2 of <= 6e-8 absolute, times ln 2, the second one j times); aerr is ten (twenty) times that
    // outside [zlo, zhi].  The intensity-only kernels compare z_approx before z is rounded to T, so there the
    // rounding of z to T (which zlo / zhi refer to) is added.
    const double aerr = 1e-6 * fabs(e.m2rho) * n * (k + 1.0);
    const double zr = blocks_1x1 ? 2.0 * (f32 ? eps_of<float>() : eps_of<double>()) + 1e-9 : 1e-9;
    e.zlo_a = (e.zlo > -INFINITY && e.zlo < INFINITY) ? e.zlo - (aerr + zr * fabs(e.zlo)) : e.zlo;
    e.zhi_a = (e.zhi < INFINITY) ? e.zhi + (aerr + zr * fabs(e.zhi)) : INFINITY;
    if (!(aerr == aerr) || !(aerr < INFINITY)) {   // rho is NaN/inf for j = 1: exact path only
        e.zlo = e.zlo_a = -INFINITY;
        e.zhi = e.zhi_a = INFINITY;
    }
    return e;
}

// small cache of per-call tables
struct TabKey {
    int k, dtype, p, q;
    double n, alpha;     // compared as bits
};

std::vector<OmniTabEntry> get_table(int k, double n_looks, double alpha, int dtype, OmniFamily fam)
{
    static std::mutex mu;
    static std::vector<std::pair<TabKey, std::vector<OmniTabEntry>>> cache;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const auto &c : cache)
            if (c.first.k == k && c.first.dtype == dtype && c.first.p == fam.p && c.first.q == fam.q &&
                memcmp(&c.first.n, &n_looks, sizeof(double)) == 0 &&
                memcmp(&c.first.alpha, &alpha, sizeof(double)) == 0)
                return c.second;
    }
    std::vector<OmniTabEntry> tab((size_t)k + 1);
    memset(tab.data(), 0, tab.size() * sizeof(OmniTabEntry));
    for (int j = 1; j <= k; ++j) tab[j] = make_entry(j, n_looks, alpha, dtype, fam);
    {
        std::lock_guard<std::mutex> lk(mu);
        if (cache.size() >= 32) cache.erase(cache.begin());
        cache.emplace_back(TabKey{k, dtype, fam.p, fam.q, n_looks, alpha}, tab);
    }
    return tab;
}

template <typename T>
DenseScreenEntry make_dense_entry(const OmniTabEntry &t, int j, double n_looks)
{
    DenseScreenEntry d;
    d.re = 0;
    d.rf = 0.f;
    d.a = -INFINITY;    // never "fires for certain"
    d.b = INFINITY;     // never "cannot fire"  => every test of this j is handed over
    const double c = t.m2rho * n_looks * 0.6931471805599453;
    const double z0 = t.m2rho * n_looks * t.pklogk;
    if (j < 2 || !(c < 0.0) || !(c > -INFINITY) || !(z0 == z0) || !(fabs(z0) < INFINITY)) return d;
    if (t.zlo == INFINITY) {          // P <= 1 < alpha: nothing can fire
        d.b = -INFINITY;
        return d;
    }
    const double eps = eps_of<T>();
    const bool hi_ok = t.zhi < INFINITY && t.zhi > -INFINITY;
    const bool lo_ok = t.zlo > -INFINITY && t.zlo < INFINITY;
    // beyond 32 dates the float32 arithmetic of x works on magnitudes up to j (ulp 7.6e-6 at 64) and
    // the fixed-point sum of the mantissa logs passes 2^24 before it is converted: the budget grows
    // to ~2.5e-5 at j = 64 and ~6e-5 at j = 128, the margin with it (4.6e-5 / 1.7e-4)
    const double mg0 = 2e-5 + 4e-7 * (double)j + (j > 32 ? 1e-6 * (double)(j - 32) : 0.0);
    double Lhi = 0, Llo = 0;
    if (hi_ok) {
        const double zr = 2.0 * eps * fabs(t.zhi);                 // (T) rounding of z
        Lhi = (t.zhi + zr - z0) / c;                               // z > zhi + zr  <=>  L2 < Lhi
        Lhi -= mg0 + 1e-12 * fabs(Lhi);
    }
    if (lo_ok) {
        const double zr = 2.0 * eps * fabs(t.zlo);
        Llo = (t.zlo - zr - z0) / c;                               // z < zlo - zr  <=>  L2 > Llo
        Llo += mg0 + 1e-12 * fabs(Llo);
    }
    if (!hi_ok && !lo_ok) return d;
    const double R = hi_ok ? Lhi : Llo;
    if (!(fabs(R) < 5e8)) return d;
    const double fl = floor(R);
    d.re = (int)fl;
    d.rf = (float)(R - fl);
    if (hi_ok) {
        d.a = 0.f;
        d.b = lo_ok ? (float)(Llo - R) + 1e-6f : INFINITY;
        if (lo_ok && !(Llo >= R)) {      // cannot happen (zlo <= zhi); be safe: exact only
            d.a = -INFINITY;
            d.b = INFINITY;
        }
    } else {
        d.a = -INFINITY;
        d.b = 0.f;
    }
    return d;
}

template <typename T>
DenseScreen make_dense_screen(const std::vector<OmniTabEntry> &tab, int k, double n_looks)
{
    DenseScreen s;
    memset(&s, 0, sizeof(s));
    for (int j = 0; j <= kDenseMax; ++j) {
        s.e[j].a = -INFINITY;
        s.e[j].b = INFINITY;
        if (j >= 1 && j <= k) s.e[j] = make_dense_entry<T>(tab[(size_t)j], j, n_looks);
    }
    return s;
}

template <typename T>
void stream_marginal_bounds(const OmniTabEntry &t, int j, double n_looks, float *ca, float *cb)
{
    *ca = 0.f;            // never "fires for certain"
    *cb = INFINITY;       // never "cannot fire"
    const double c = t.m2rho * n_looks * 0.6931471805599453;
    const double z0 = t.m2rho * n_looks * t.pklogk;
    if (j < 2 || !(c < 0.0) || !(c > -INFINITY) || !(z0 == z0) || !(fabs(z0) < INFINITY)) return;
    if (t.zlo == INFINITY) {          // P <= 1 < alpha: nothing can fire
        *cb = 0.f;
        return;
    }
    const double eps = eps_of<T>();
    const double mgp = 4e-6;
    if (t.zhi < INFINITY && t.zhi > -INFINITY) {
        const double zr = 2.0 * eps * fabs(t.zhi);
        double L = (t.zhi + zr - z0) / c;
        L -= mgp + 1e-12 * fabs(L);
        if (L == L && L > -100.0) {
            if (L > 6.0) L = 6.0;                                // a weaker claim, still true
            float v = (float)exp2(L);
            if ((double)v > exp2(L)) v = nextafterf(v, 0.f);     // rounded down
            *ca = v;
        }
    }
    if (t.zlo > -INFINITY && t.zlo < INFINITY) {
        const double zr = 2.0 * eps * fabs(t.zlo);
        double L = (t.zlo - zr - z0) / c;
        L += mgp + 1e-12 * fabs(L);
        if (L == L && L <= 6.0) {
            if (L < -100.0) L = -100.0;                          // a weaker claim, still true
            float v = (float)exp2(L);
            if ((double)v < exp2(L)) v = nextafterf(v, INFINITY);   // rounded up
            *cb = v;
        }
    }
    if (!(*ca <= *cb)) {              // cannot happen (zlo <= zhi); be safe: exact only
        *ca = 0.f;
        *cb = INFINITY;
    }
}

template DenseScreenEntry make_dense_entry<float>(const OmniTabEntry &, int, double);
template DenseScreenEntry make_dense_entry<double>(const OmniTabEntry &, int, double);
template DenseScreen make_dense_screen<float>(const std::vector<OmniTabEntry> &, int, double);
template DenseScreen make_dense_screen<double>(const std::vector<OmniTabEntry> &, int, double);
template void stream_marginal_bounds<float>(const OmniTabEntry &, int, double, float *, float *);
template void stream_marginal_bounds<double>(const OmniTabEntry &, int, double, float *, float *);

}  // namespace nd_amd
