// nd_amd/csrc/kmeans_fit.hip -- training k-means on every pixel of a stack, on the device:
//   nd_amd_kmeans_step      one Lloyd iteration: assignment, per-cluster sums and counts, inertia, changed labels
//   nd_amd_feature_moments  count, mean and population variance of every feature over the valid rows
//   nd_amd_gather_rows      the rows at given indices as a dense matrix (initial centres are drawn from it)
// Rows are addressed as in classify.hip: feature f of a row is read from feat[f] + row offset, and the
// scaler is applied by the same scaled<T>, so that fit and predict see the same values.
//
// Every sum here is formed in a FIXED order, so a call repeats its result bit for bit: the stopping rule
// of the Lloyd loop compares a centre shift with a threshold, and the number of iterations must not depend
// on scheduling.  No floating-point atomics.  The order:
//   a block is ONE wave; it walks batches of 64 consecutive rows, batch b, b + grid, b + 2 grid, ...;
//   inside a batch a sum over the lanes is the xor butterfly (32, 16, .., 1) with 0 from lanes that take no
//   part, which is one fixed tree; the batch's result is added to the block's accumulator (LDS, or a
//   register for the scalars) in batch order; the fold kernel adds the blocks' partials in block order.
// The grid is a function of (rows, k, nfeat) alone.
// The definitions are in include/nd_amd.h.
#include <math.h>

#include "classify_common.hpp"
#include "dispatch.hpp"
#include "lanes.hpp"

using namespace nd_amd;

namespace {

constexpr int WAVE = 64;                    // threads of a block of the reducing kernels
constexpr int FIT_MAX_GRID = 8192;
constexpr int64_t FIT_PARTIAL_DOUBLES = INT64_C(1) << 22;   // at most 32 MiB of float64 partials

// ---- one Lloyd iteration ----------------------------------------------------------------------
// NREG > 0: the row's nfeat <= NREG features live in registers.  NREG == 0: they are read again where
// they are needed (the second read hits the cache).
// LDS: acc[k * nfeat] float64 sums, then cnt[k] int64 counts.
// dpart[block][k * nfeat + 1]: sums, inertia.  ipart[block][k + 1]: counts, changed.
template <typename T, int NREG>
__global__ __launch_bounds__(WAVE) void kmeans_step_kernel(
    const void *const *tab, int nfeat, RowDims R, int64_t rows, const double *__restrict__ centers, int k,
    const double *__restrict__ mean, const double *__restrict__ scale, int32_t *__restrict__ labels,
    double *__restrict__ dpart, int64_t *__restrict__ ipart)
{
    extern __shared__ double fit_lds[];
    double *acc = fit_lds;
    long long *cnt = reinterpret_cast<long long *>(fit_lds + (int64_t)k * nfeat);
    const int lane = threadIdx.x;
    const int nacc = k * nfeat;
    for (int i = lane; i < nacc; i += WAVE) acc[i] = 0.0;
    for (int i = lane; i < k; i += WAVE) cnt[i] = 0;
    __syncthreads();
    double inertia = 0.0;
    long long changed = 0;
    const int64_t nbatch = (rows + WAVE - 1) / WAVE;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = b * WAVE + lane;
        const bool inside = row < rows;
        int64_t off = 0, loff;
        if (inside) row_offsets(R, row, off, loff);
        T x[NREG > 0 ? NREG : 1];
        bool valid = inside;
        if (NREG > 0) {
#pragma unroll
            for (int j = 0; j < NREG; j++) {
                x[j] = (T)0;
                if (j < nfeat && inside) {
                    const T v = static_cast<const T *>(tab[j])[off];
                    valid &= (v == v);
                    x[j] = scaled<T>(v, mean, scale, j);
                }
            }
        } else if (inside) {
            for (int f = 0; f < nfeat; f++) {
                const T v = static_cast<const T *>(tab[f])[off];
                valid &= (v == v);
            }
        }
        // the first nearest centre: the rule of classify_kmeans_kernel
        double best = INFINITY;
        int besti = 0;
        if (valid) {
            for (int j = 0; j < k; j++) {
                const double *c = centers + (int64_t)j * nfeat;
                double d = 0.0;
                if (NREG > 0) {
#pragma unroll
                    for (int f = 0; f < NREG; f++) {
                        if (f < nfeat) {
                            const double e = (double)x[f] - c[f];
                            d += e * e;
                        }
                    }
                } else {
                    for (int f = 0; f < nfeat; f++) {
                        const T v = scaled<T>(static_cast<const T *>(tab[f])[off], mean, scale, f);
                        const double e = (double)v - c[f];
                        d += e * e;
                    }
                }
                if (d < best) {
                    best = d;
                    besti = j;
                }
            }
        }
        const int label = valid ? besti : -1;
        if (inside) {
            changed += (valid && labels[row] != label) ? 1 : 0;
            labels[row] = label;
        }
        inertia += wave_sum(valid ? best : 0.0);
        // the labels present in this batch, in the order of their first row; every lane walks the same list
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            const int j = __shfl(label, src, WAVE);
            const unsigned long long members = __ballot(label == j);
            todo &= ~members;
            const bool mine = label == j;
            if (lane == 0) cnt[j] += __popcll(members);
            if (NREG > 0) {
#pragma unroll
                for (int f = 0; f < NREG; f++) {
                    if (f < nfeat) {
                        const double s = wave_sum(mine ? (double)x[f] : 0.0);
                        if (lane == 0) acc[j * nfeat + f] += s;
                    }
                }
            } else {
                for (int f = 0; f < nfeat; f++) {
                    double v = 0.0;
                    if (mine) v = (double)scaled<T>(static_cast<const T *>(tab[f])[off], mean, scale, f);
                    const double s = wave_sum(v);
                    if (lane == 0) acc[j * nfeat + f] += s;
                }
            }
        }
    }
    // changed: an integer sum, any order gives the same result
    for (int d = 32; d > 0; d >>= 1) changed += __shfl_xor(changed, d, WAVE);
    __syncthreads();
    double *dp = dpart + (int64_t)blockIdx.x * (nacc + 1);
    int64_t *ip = ipart + (int64_t)blockIdx.x * (k + 1);
    for (int i = lane; i < nacc; i += WAVE) dp[i] = acc[i];
    for (int i = lane; i < k; i += WAVE) ip[i] = cnt[i];
    if (lane == 0) {
        dp[nacc] = inertia;
        ip[k] = changed;
    }
}

// out[i] = sum over the blocks, in block order, of part[block][i]; one thread per entry
__global__ __launch_bounds__(BLOCK) void fit_fold_kernel(const double *__restrict__ dpart, int nd,
                                                         const int64_t *__restrict__ ipart, int ni, int nblocks,
                                                         double *__restrict__ dout, double *__restrict__ dlast,
                                                         int64_t *__restrict__ iout, int64_t *__restrict__ ilast)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < nd) {
        double s = 0.0;
        for (int b = 0; b < nblocks; b++) s += dpart[(int64_t)b * nd + i];
        if (i < nd - 1 || dlast == nullptr) dout[i] = s;
        else *dlast = s;
    } else if (i < nd + ni) {
        const int e = i - nd;
        int64_t s = 0;
        for (int b = 0; b < nblocks; b++) s += ipart[(int64_t)b * ni + e];
        if (e < ni - 1 || ilast == nullptr) iout[e] = s;
        else *ilast = s;
    }
}

// ---- feature moments --------------------------------------------------------------------------
// center == nullptr: per-feature sums of x.  Else: per-feature sums of (x - center[f])^2.
// LDS: acc[nfeat].  dpart[block][nfeat], ipart[block][1] (valid rows).
template <typename T>
__global__ __launch_bounds__(WAVE) void feature_moments_kernel(
    const void *const *tab, int nfeat, RowDims R, int64_t rows, const double *__restrict__ center,
    const double *__restrict__ mean, const double *__restrict__ scale, double *__restrict__ dpart,
    int64_t *__restrict__ ipart)
{
    extern __shared__ double fit_lds[];
    double *acc = fit_lds;
    const int lane = threadIdx.x;
    for (int i = lane; i < nfeat; i += WAVE) acc[i] = 0.0;
    __syncthreads();
    long long count = 0;
    const int64_t nbatch = (rows + WAVE - 1) / WAVE;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = b * WAVE + lane;
        const bool inside = row < rows;
        int64_t off = 0, loff;
        if (inside) row_offsets(R, row, off, loff);
        bool valid = inside;
        if (inside) {
            for (int f = 0; f < nfeat; f++) {
                const T v = static_cast<const T *>(tab[f])[off];
                valid &= (v == v);
            }
        }
        count += valid ? 1 : 0;
        if (__ballot(valid) == 0) continue;          // the same in every lane
        for (int f = 0; f < nfeat; f++) {
            double v = 0.0;
            if (valid) {
                v = (double)scaled<T>(static_cast<const T *>(tab[f])[off], mean, scale, f);
                if (center) {
                    const double e = v - center[f];
                    v = e * e;
                }
            }
            const double s = wave_sum(v);
            if (lane == 0) acc[f] += s;
        }
    }
    for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d, WAVE);
    __syncthreads();
    for (int i = lane; i < nfeat; i += WAVE) dpart[(int64_t)blockIdx.x * nfeat + i] = acc[i];
    if (lane == 0) ipart[blockIdx.x] = count;
}

// out[f] = sum[f] / count, in place (0 / 0 = NaN where no row is valid)
__global__ __launch_bounds__(BLOCK) void moments_divide_kernel(double *__restrict__ v, int nfeat,
                                                               const int64_t *__restrict__ count)
{
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f < nfeat) v[f] = v[f] / (double)*count;
}

// ---- gather rows ------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void gather_rows_kernel(
    const void *const *tab, int nfeat, RowDims R, int64_t rows, const int64_t *__restrict__ index, int64_t m,
    const double *__restrict__ mean, const double *__restrict__ scale, T *__restrict__ X,
    uint8_t *__restrict__ valid)
{
    const T nan = (T)__longlong_as_double(0x7ff8000000000000ll);
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * BLOCK) {
        const int64_t row = index[i];
        bool ok = row >= 0 && row < rows;           // an index outside the table is never followed
        if (ok) {
            int64_t off, loff;
            row_offsets(R, row, off, loff);
            for (int f = 0; f < nfeat; f++) {
                const T v = static_cast<const T *>(tab[f])[off];
                ok &= (v == v);
                X[i * nfeat + f] = scaled<T>(v, mean, scale, f);
            }
        } else {
            for (int f = 0; f < nfeat; f++) X[i * nfeat + f] = nan;
        }
        valid[i] = ok ? 1 : 0;
    }
}

// ---- host -------------------------------------------------------------------------------------
static bool fit_served(int nfeat, int k) { return k >= 1 && (int64_t)k * (nfeat + 1) <= ND_AMD_KMEANS_FIT_MAX_ACC; }

// blocks (of one wave) of the reducing kernels: a function of the problem's shape alone
static int fit_grid(int64_t rows, int nfeat, int k)
{
    int64_t cap = FIT_PARTIAL_DOUBLES / ((int64_t)k * (nfeat + 1));
    cap = cap > FIT_MAX_GRID ? FIT_MAX_GRID : (cap < 256 ? 256 : cap);
    const int64_t b = ceil_div(rows, WAVE);
    return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

struct FitWorkspace {
    const void *const *tab;
    double *dpart;
    int64_t *ipart;
};

static size_t fit_layout(int64_t rows, int nfeat, int k, void *workspace, FitWorkspace *w)
{
    const size_t grid = (size_t)fit_grid(rows, nfeat, k);
    const size_t t = nd_amd_classify_workspace_bytes(nfeat);
    const size_t d = align256(grid * ((size_t)k * nfeat + 1) * sizeof(double));
    const size_t i = align256(grid * ((size_t)k + 1) * sizeof(int64_t));
    if (w) {
        char *p = (char *)workspace;
        w->tab = (const void *const *)p;
        w->dpart = (double *)(p + t);
        w->ipart = (int64_t *)(p + t + d);
    }
    return t + d + i;
}

// the checks the three entries share; on success the table is on its way to the device
static int fit_common(const char *who, const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                      const int64_t *strides, const double *mean, const double *scale, int k, void *workspace,
                      size_t workspace_bytes, RowDims &R, int64_t &rows)
{
    int rc = check_table(who, feat, nfeat, dtype, workspace, nd_amd_classify_workspace_bytes(nfeat));
    if (rc != ND_AMD_OK) return rc;
    rc = make_dims(who, sizes, strides, nullptr, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if ((mean == nullptr) != (scale == nullptr)) {
        set_error("%s: scaler needs both mean and scale", who);
        return ND_AMD_EINVAL;
    }
    if (k < 1) {
        set_error("%s: needs k >= 1 centres (k = %d)", who, k);
        return ND_AMD_EINVAL;
    }
    if (!fit_served(nfeat, k)) {
        set_error("%s: serves k * (features + 1) <= %d (k = %d, %d features)", who, ND_AMD_KMEANS_FIT_MAX_ACC, k,
                  nfeat);
        return ND_AMD_EUNSUPPORTED;
    }
    if (workspace_bytes < nd_amd_kmeans_fit_workspace_bytes(nfeat, k, rows)) {
        set_error("%s: workspace smaller than nd_amd_kmeans_fit_workspace_bytes(%d, %d, %lld)", who, nfeat, k,
                  (long long)rows);
        return ND_AMD_EWORKSPACE;
    }
    return ND_AMD_OK;
}

}  // namespace

extern "C" size_t nd_amd_kmeans_fit_workspace_bytes(int nfeat, int k, int64_t rows)
{
    if (nfeat < 1 || nfeat > MAX_LDS_FEATURES || rows < 0 || !fit_served(nfeat, k)) return 0;
    return fit_layout(rows, nfeat, k, nullptr, nullptr);
}

extern "C" int nd_amd_kmeans_step(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                                  const int64_t *strides, const double *centers, int k, const double *mean,
                                  const double *scale, int32_t *labels, double *sums, int64_t *counts,
                                  double *inertia, int64_t *changed, void *workspace, size_t workspace_bytes,
                                  void *hip_stream)
{
    const char *who = "nd_amd_kmeans_step";
    RowDims R;
    int64_t rows;
    int rc = fit_common(who, feat, nfeat, dtype, sizes, strides, mean, scale, k, workspace, workspace_bytes, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (!centers || !sums || !counts || !inertia || !changed || (rows > 0 && !labels)) {
        set_error("%s: centers, labels, sums, counts, inertia and changed must be given", who);
        return ND_AMD_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (rows == 0) {
        ND_HIP_CHECK(hipMemsetAsync(sums, 0, sizeof(double) * k * nfeat, st));
        ND_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * k, st));
        ND_HIP_CHECK(hipMemsetAsync(inertia, 0, sizeof(double), st));
        ND_HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(int64_t), st));
        return ND_AMD_OK;
    }
    FitWorkspace w;
    fit_layout(rows, nfeat, k, workspace, &w);
    ND_HIP_CHECK(hipMemcpyAsync(workspace, feat, (size_t)nfeat * sizeof(void *), hipMemcpyHostToDevice, st));
    const int grid = fit_grid(rows, nfeat, k);
    const size_t lds = (size_t)k * (nfeat + 1) * sizeof(double);
    const int nd = k * nfeat + 1, ni = k + 1;
    {
        KernelTimer timer(ND_AMD_KERNEL_KMEANS_STEP, st);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            auto launch = [&](auto NREG) {
                hipLaunchKernelGGL((kmeans_step_kernel<T, decltype(NREG)::value>), dim3(grid), dim3(WAVE), lds, st, w.tab, nfeat, R,
                                   rows, centers, k, mean, scale, labels, w.dpart, w.ipart);
            };
            if (!pick_le<4, 8>(nfeat, launch)) launch(int_c<0>{});
        });
        hipLaunchKernelGGL(fit_fold_kernel, dim3((unsigned)ceil_div(nd + ni, BLOCK)), dim3(BLOCK), 0, st, w.dpart, nd,
                           w.ipart, ni, grid, sums, inertia, counts, changed);
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_feature_moments(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                                      const int64_t *strides, const double *mean, const double *scale,
                                      int64_t *count, double *fmean, double *fvar, void *workspace,
                                      size_t workspace_bytes, void *hip_stream)
{
    const char *who = "nd_amd_feature_moments";
    RowDims R;
    int64_t rows;
    int rc = fit_common(who, feat, nfeat, dtype, sizes, strides, mean, scale, 1, workspace, workspace_bytes, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (!count || !fmean || !fvar) {
        set_error("%s: count, mean and var outputs must be given", who);
        return ND_AMD_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    FitWorkspace w;
    fit_layout(rows, nfeat, 1, workspace, &w);
    if (rows > 0)
        ND_HIP_CHECK(hipMemcpyAsync(workspace, feat, (size_t)nfeat * sizeof(void *), hipMemcpyHostToDevice, st));
    const int grid = rows > 0 ? fit_grid(rows, nfeat, 1) : 0;
    const size_t lds = (size_t)nfeat * sizeof(double);
    const unsigned fblocks = (unsigned)ceil_div(nfeat + 1, BLOCK), dblocks = (unsigned)ceil_div(nfeat, BLOCK);
    {
        KernelTimer timer(ND_AMD_KERNEL_FEATURE_MOMENTS, st);
        for (int pass = 0; pass < 2; pass++) {
            double *out = pass == 0 ? fmean : fvar;
            if (grid > 0) {
                const double *center = pass == 0 ? nullptr : fmean;
                pick(dtype == ND_AMD_F64, [&](auto F64) {
                    using T = std::conditional_t<decltype(F64)::value, double, float>;
                    hipLaunchKernelGGL(feature_moments_kernel<T>, dim3(grid), dim3(WAVE), lds, st, w.tab, nfeat, R, rows, center,
                                       mean, scale, w.dpart, w.ipart);
                });
            }
            // with no block the fold writes zeros, and the division below NaN
            hipLaunchKernelGGL(fit_fold_kernel, dim3(fblocks), dim3(BLOCK), 0, st, w.dpart, nfeat, w.ipart, 1, grid, out,
                               (double *)nullptr, count, (int64_t *)nullptr);
            hipLaunchKernelGGL(moments_divide_kernel, dim3(dblocks), dim3(BLOCK), 0, st, out, nfeat, count);
        }
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_gather_rows(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                                  const int64_t *strides, const int64_t *index, int64_t m, const double *mean,
                                  const double *scale, void *X, uint8_t *valid, void *workspace,
                                  size_t workspace_bytes, void *hip_stream)
{
    const char *who = "nd_amd_gather_rows";
    int rc = check_table(who, feat, nfeat, dtype, workspace, workspace_bytes);
    if (rc != ND_AMD_OK) return rc;
    RowDims R;
    int64_t rows;
    rc = make_dims(who, sizes, strides, nullptr, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if ((mean == nullptr) != (scale == nullptr)) {
        set_error("%s: scaler needs both mean and scale", who);
        return ND_AMD_EINVAL;
    }
    if (m < 0 || m > (INT64_C(1) << 40) || (m > 0 && (!index || !X || !valid))) {
        set_error("%s: needs m >= 0 indices with the X and valid outputs (m = %lld)", who, (long long)m);
        return ND_AMD_EINVAL;
    }
    if (m == 0) return ND_AMD_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    ND_HIP_CHECK(hipMemcpyAsync(workspace, feat, (size_t)nfeat * sizeof(void *), hipMemcpyHostToDevice, st));
    const void *const *tab = (const void *const *)workspace;
    const int64_t b = ceil_div(m, BLOCK);
    const int grid = (int)(b < 8192 ? b : 8192);
    {
        KernelTimer timer(ND_AMD_KERNEL_GATHER_ROWS, st);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            hipLaunchKernelGGL(gather_rows_kernel<T>, dim3(grid), dim3(BLOCK), 0, st, tab, nfeat, R, rows, index, m, mean, scale,
                               (T *)X, valid);
        });
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}
