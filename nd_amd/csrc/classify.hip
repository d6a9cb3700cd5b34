// nd_amd/csrc/classify.hip -- pixel classification (nd/classify.py) on the device:
//   nd_amd_classify_forest   decision-forest predict / predict_proba, scikit-learn's arithmetic
//   nd_amd_classify_kmeans   nearest centre in float64
//   nd_amd_classify_knn      k nearest training samples in float64, votes and labels
//   nd_amd_classify_linear   decision values of a linear model, labels and probabilities
//   nd_amd_classify_select / _gather   the training rows, compacted in row order
//   nd_amd_class_stats / _fill         per-class statistics and the fill of class_mean
// No (rows, features) matrix is ever formed: a row's feature f is read from feat[f] + row offset.
// The definitions are in include/nd_amd.h.
#include <math.h>

#include "classify_common.hpp"
#include "dispatch.hpp"

using namespace nd_amd;

namespace {

constexpr int SELECT_ITEMS = ND_AMD_CLASSIFY_BLOCK_ROWS / BLOCK;   // rows per thread of select / gather
constexpr int STATS_REG_CLASSES = 8;
constexpr int STATS_LDS_CLASSES = 1024;

static_assert(ND_AMD_CLASSIFY_BLOCK_ROWS % BLOCK == 0, "block rows");

// ---- forest -----------------------------------------------------------------------------------
// node: {bits of t32, feature (-1: leaf), left | row of `values`, right}, absolute node indices.
// NREG > 0: the row's nfeat <= NREG features live in registers (as float32, what the trees see) and a
// node picks one by a select chain.  NREG == 0: the feature a node asks for is read from memory.
// NC class accumulators in registers; more classes than NC walk the forest once per NC classes, which
// keeps every class's sum in tree order.
template <typename T, int NREG, int NC>
__global__ __launch_bounds__(BLOCK) void classify_forest_kernel(
    const void *const *tab, int nfeat, RowDims R, int64_t rows, const int4 *__restrict__ nodes,
    const double *__restrict__ values, const int32_t *__restrict__ roots, int ntrees,
    const double *__restrict__ classes, int nclasses, const double *__restrict__ mean,
    const double *__restrict__ scale, double *__restrict__ labels, double *__restrict__ proba)
{
    __shared__ const void *sbase[NREG == 0 ? MAX_LDS_FEATURES : 1];
    stage_table<NREG>(sbase, tab, nfeat);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x; row < rows; row += (int64_t)gridDim.x * BLOCK) {
        int64_t off, loff;
        row_offsets(R, row, off, loff);
        float x[NREG > 0 ? NREG : 1];
        bool masked = false;
        if (NREG > 0) {
#pragma unroll
            for (int j = 0; j < NREG; j++) {
                x[j] = 0.f;
                if (j < nfeat) {
                    const T v = static_cast<const T *>(tab[j])[off];
                    masked |= (v != v);
                    x[j] = (float)scaled<T>(v, mean, scale, j);
                }
            }
        } else {
            for (int f = 0; f < nfeat; f++) {
                const T v = static_cast<const T *>(sbase[f])[off];
                masked |= (v != v);
            }
        }
        if (masked) {
            if (labels) labels[row] = nan;
            if (proba)
                for (int c = 0; c < nclasses; c++) proba[row * nclasses + c] = nan;
            continue;
        }
        double best = -1.0;
        int besti = 0;
        for (int c0 = 0; c0 < nclasses; c0 += NC) {
            double acc[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) acc[c] = 0.0;
            for (int t = 0; t < ntrees; t++) {
                int4 nd = nodes[roots[t]];
                while (nd.y >= 0) {
                    float xv;
                    if (NREG > 0) {
                        xv = x[0];
#pragma unroll
                        for (int j = 1; j < NREG; j++) xv = (nd.y == j) ? x[j] : xv;
                    } else {
                        const T v = static_cast<const T *>(sbase[nd.y])[off];
                        xv = (float)scaled<T>(v, mean, scale, nd.y);
                    }
                    nd = nodes[(xv <= __int_as_float(nd.x)) ? nd.z : nd.w];
                }
                const double *lv = values + (int64_t)nd.z * nclasses + c0;
#pragma unroll
                for (int c = 0; c < NC; c++)
                    if (c0 + c < nclasses) acc[c] += lv[c];
            }
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c0 + c < nclasses) {
                    const double p = acc[c] / (double)ntrees;
                    if (proba) proba[row * nclasses + c0 + c] = p;
                    if (p > best) {
                        best = p;
                        besti = c0 + c;
                    }
                }
            }
        }
        if (labels) labels[row] = classes[besti];
    }
}

// ---- k-means ----------------------------------------------------------------------------------
template <typename T, int NREG>
__global__ __launch_bounds__(BLOCK) void classify_kmeans_kernel(
    const void *const *tab, int nfeat, RowDims R, int64_t rows, const double *__restrict__ centers, int k,
    const double *__restrict__ mean, const double *__restrict__ scale, double *__restrict__ labels)
{
    __shared__ const void *sbase[NREG == 0 ? MAX_LDS_FEATURES : 1];
    stage_table<NREG>(sbase, tab, nfeat);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x; row < rows; row += (int64_t)gridDim.x * BLOCK) {
        int64_t off, loff;
        row_offsets(R, row, off, loff);
        T x[NREG > 0 ? NREG : 1];
        bool masked = false;
        if (NREG > 0) {
#pragma unroll
            for (int j = 0; j < NREG; j++) {
                x[j] = (T)0;
                if (j < nfeat) {
                    const T v = static_cast<const T *>(tab[j])[off];
                    masked |= (v != v);
                    x[j] = scaled<T>(v, mean, scale, j);
                }
            }
        } else {
            for (int f = 0; f < nfeat; f++) {
                const T v = static_cast<const T *>(sbase[f])[off];
                masked |= (v != v);
            }
        }
        if (masked) {
            labels[row] = nan;
            continue;
        }
        double best = INFINITY;
        int besti = 0;
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
                    const T v = scaled<T>(static_cast<const T *>(sbase[f])[off], mean, scale, f);
                    const double e = (double)v - c[f];
                    d += e * e;
                }
            }
            if (d < best) {
                best = d;
                besti = j;
            }
        }
        labels[row] = (double)besti;
    }
}

// ---- select / gather --------------------------------------------------------------------------
// One block per ND_AMD_CLASSIFY_BLOCK_ROWS rows; thread t takes rows base + i * BLOCK + t.
template <typename T>
__global__ __launch_bounds__(BLOCK) void classify_select_kernel(
    const void *const *tab, int nfeat, RowDims R, int64_t rows, const double *__restrict__ labels,
    uint8_t *__restrict__ mask, int64_t *__restrict__ block_counts)
{
    __shared__ int swave[BLOCK / 64];
    const int64_t base = (int64_t)blockIdx.x * ND_AMD_CLASSIFY_BLOCK_ROWS;
    int count = 0;
    for (int i = 0; i < SELECT_ITEMS; i++) {
        const int64_t row = base + i * BLOCK + threadIdx.x;
        if (row >= rows) break;
        int64_t off, loff;
        row_offsets(R, row, off, loff);
        bool m = true;
        if (labels) {
            const double l = labels[loff];
            m = (l == l) && l > 0.0;
        }
        if (m) {
            for (int f = 0; f < nfeat; f++) {
                const T v = static_cast<const T *>(tab[f])[off];
                m &= (v == v);
            }
        }
        mask[row] = m ? 1 : 0;
        count += m ? 1 : 0;
    }
    for (int d = 32; d > 0; d >>= 1) count += __shfl_down(count, d, 64);
    if ((threadIdx.x & 63) == 0) swave[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < BLOCK / 64; w++) s += swave[w];
        block_counts[blockIdx.x] = s;
    }
}

// exclusive scan of the block counts, in place; one block.  total -> *count
__global__ __launch_bounds__(BLOCK) void classify_scan_kernel(int64_t *__restrict__ v, int64_t n,
                                                              int64_t *__restrict__ count)
{
    __shared__ int64_t ssum[BLOCK];
    const int64_t chunk = (n + BLOCK - 1) / BLOCK;
    const int64_t lo = chunk * threadIdx.x < n ? chunk * threadIdx.x : n;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; i++) s += v[i];
    ssum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int i = 0; i < BLOCK; i++) {
            const int64_t c = ssum[i];
            ssum[i] = run;
            run += c;
        }
        *count = run;
    }
    __syncthreads();
    int64_t run = ssum[threadIdx.x];
    for (int64_t i = lo; i < hi; i++) {
        const int64_t c = v[i];
        v[i] = run;
        run += c;
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void classify_gather_kernel(
    const void *const *tab, int nfeat, RowDims R, int64_t rows, const double *__restrict__ labels,
    const uint8_t *__restrict__ mask, const int64_t *__restrict__ block_offsets, T *__restrict__ X,
    double *__restrict__ y)
{
    constexpr int WAVES = BLOCK / 64;
    __shared__ int sseg[SELECT_ITEMS * WAVES];
    const int64_t base = (int64_t)blockIdx.x * ND_AMD_CLASSIFY_BLOCK_ROWS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool m[SELECT_ITEMS];
    int before[SELECT_ITEMS];
#pragma unroll
    for (int i = 0; i < SELECT_ITEMS; i++) {
        const int64_t row = base + i * BLOCK + threadIdx.x;
        m[i] = row < rows && mask[row] != 0;
        const unsigned long long b = __ballot(m[i]);
        before[i] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) sseg[i * WAVES + wave] = __popcll(b);
    }
    __syncthreads();
    const int64_t out0 = block_offsets[blockIdx.x];
#pragma unroll
    for (int i = 0; i < SELECT_ITEMS; i++) {
        if (!m[i]) continue;
        int prefix = 0;
        for (int s = 0; s < i * WAVES + wave; s++) prefix += sseg[s];
        const int64_t dst = out0 + prefix + before[i];
        const int64_t row = base + i * BLOCK + threadIdx.x;
        int64_t off, loff;
        row_offsets(R, row, off, loff);
        for (int f = 0; f < nfeat; f++) X[dst * nfeat + f] = static_cast<const T *>(tab[f])[off];
        if (y) y[dst] = labels[loff];
    }
}

// ---- class statistics and fill ----------------------------------------------------------------
// class of a label: l in 0 .. n-1 where the label equals the integer l, else n ("other")
__device__ __forceinline__ int class_of(double l, int n)
{
    return (l >= 0.0 && l < (double)n && l == floor(l)) ? (int)l : n;
}

// MODE 0: n <= 8, per-lane registers, one LDS + global atomic round per block.  MODE 1: n <= 1024,
// LDS atomics per element.  MODE 2: global atomics per element.
template <typename T, int MODE>
__global__ __launch_bounds__(BLOCK) void class_stats_kernel(
    const T *__restrict__ var, RowDims R, int64_t rows, const double *__restrict__ labels, int n,
    double *__restrict__ sum, unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ nanc)
{
    constexpr int NL = MODE == 0 ? STATS_REG_CLASSES : (MODE == 1 ? STATS_LDS_CLASSES : 1);
    __shared__ double ssum[NL];
    __shared__ unsigned long long scnt[NL], snan[NL];
    if (MODE != 2) {
        for (int i = threadIdx.x; i < NL; i += BLOCK) {
            ssum[i] = 0.0;
            scnt[i] = 0;
            snan[i] = 0;
        }
        __syncthreads();
    }
    double rs[STATS_REG_CLASSES];
    unsigned int rc[STATS_REG_CLASSES], rn[STATS_REG_CLASSES];
#pragma unroll
    for (int c = 0; c < STATS_REG_CLASSES; c++) {
        rs[c] = 0.0;
        rc[c] = 0;
        rn[c] = 0;
    }
    // a lane sees at most rows / (gridDim * BLOCK) + 1 < 2^32 elements: the host sizes the grid for that
    for (int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x; row < rows; row += (int64_t)gridDim.x * BLOCK) {
        int64_t off, loff;
        row_offsets(R, row, off, loff);
        const int cls = class_of(labels[loff], n);
        if (cls >= n) continue;
        const T v = var[off];
        const bool isn = (v != v);
        if (MODE == 0) {
#pragma unroll
            for (int c = 0; c < STATS_REG_CLASSES; c++) {
                const bool hit = (cls == c);
                rs[c] += (hit && !isn) ? (double)v : 0.0;
                rc[c] += (hit && !isn) ? 1u : 0u;
                rn[c] += (hit && isn) ? 1u : 0u;
            }
        } else if (MODE == 1) {
            if (isn) {
                atomicAdd(&snan[cls], 1ull);
            } else {
                atomicAdd(&ssum[cls], (double)v);
                atomicAdd(&scnt[cls], 1ull);
            }
        } else {
            if (isn) {
                atomicAdd(&nanc[cls], 1ull);
            } else {
                atomicAdd(&sum[cls], (double)v);
                atomicAdd(&cnt[cls], 1ull);
            }
        }
    }
    if (MODE == 0) {
#pragma unroll
        for (int c = 0; c < STATS_REG_CLASSES; c++) {
            double s = rs[c];
            unsigned int a = rc[c], b = rn[c];
            for (int d = 32; d > 0; d >>= 1) {
                s += __shfl_down(s, d, 64);
                a += __shfl_down(a, d, 64);
                b += __shfl_down(b, d, 64);
            }
            if ((threadIdx.x & 63) == 0 && c < n) {
                atomicAdd(&ssum[c], s);
                atomicAdd(&scnt[c], (unsigned long long)a);
                atomicAdd(&snan[c], (unsigned long long)b);
            }
        }
    }
    if (MODE != 2) {
        __syncthreads();
        for (int i = threadIdx.x; i < n && i < NL; i += BLOCK) {
            if (scnt[i]) {
                atomicAdd(&sum[i], ssum[i]);
                atomicAdd(&cnt[i], scnt[i]);
            }
            if (snan[i]) atomicAdd(&nanc[i], snan[i]);
        }
    }
}

// out = fill[class] for labels in 0 .. n-1; elsewhere the value, or fill[n] where the value is NaN
template <typename T>
__global__ __launch_bounds__(BLOCK) void class_fill_kernel(
    const T *__restrict__ var, T *__restrict__ out, RowDims R, int64_t rows, const double *__restrict__ labels,
    int n, const T *__restrict__ fill)
{
    for (int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x; row < rows; row += (int64_t)gridDim.x * BLOCK) {
        int64_t off, loff;
        row_offsets(R, row, off, loff);
        const int cls = class_of(labels[loff], n);
        T v;
        if (cls < n) {
            v = fill[cls];
        } else {
            v = var[off];
            if (v != v) v = fill[n];
        }
        out[off] = v;
    }
}

// ---- k nearest neighbours ---------------------------------------------------------------------
// One lane per row.  Every lane of a wave meets training sample j at the same time, so a sample's
// features are wave-uniform loads (scalar registers feed the float64 subtraction directly) and the
// kernel needs no barrier.  The samples are walked in tiles of KNN_TILE: the tile's distances are formed
// first (their loads issue together), then each is offered to the row's best list.
// The k best (distance, index) pairs are CAP registers kept sorted by an unrolled compare-and-shift
// chain; no element is ever addressed by a run-time index.  `kth` is the distance at position k - 1,
// refreshed after every insertion, so a candidate costs one comparison unless it enters.  Samples
// arrive in index order: a candidate that ties with a held one is the farther of the two.
// NF > 0: the row's NF features are registers.  NF == 0: the block's rows lie in LDS, feature-major
// (xs[f * blockDim.x + lane]: a wave reads consecutive addresses, and a lane only its own column).
constexpr int KNN_TILE = ND_AMD_CLASSIFY_KNN_TILE;
constexpr int KNN_LDS_BYTES = 65536;

template <int CAP>
struct KnnBest {
    double d[CAP];
    int i[CAP];
    double kth;
};

template <int CAP>
__device__ __forceinline__ void knn_offer(KnnBest<CAP> &b, double d, int j, int k)
{
    if (d < b.kth) {
#pragma unroll
        for (int s = CAP - 1; s > 0; s--) {
            const bool up = d < b.d[s - 1];
            const bool here = !up && d < b.d[s];
            b.i[s] = up ? b.i[s - 1] : (here ? j : b.i[s]);
            b.d[s] = up ? b.d[s - 1] : (here ? d : b.d[s]);
        }
        if (d < b.d[0]) {
            b.d[0] = d;
            b.i[0] = j;
        }
        double kth = b.d[0];
#pragma unroll
        for (int s = 1; s < CAP; s++) kth = (s == k - 1) ? b.d[s] : kth;
        b.kth = kth;
    }
}

template <int NF, int TJ, typename T>
__device__ __forceinline__ void knn_distances(double (&d)[TJ], const double (&x)[NF > 0 ? NF : 1], const T *xs,
                                              int xstride, const double *__restrict__ train, int nfeat, int j)
{
#pragma unroll
    for (int t = 0; t < TJ; t++) d[t] = 0.0;
    if (NF > 0) {
#pragma unroll
        for (int t = 0; t < TJ; t++) {
            const double *s = train + (int64_t)(j + t) * NF;
#pragma unroll
            for (int f = 0; f < NF; f++) {
                const double e = x[f] - s[f];
                d[t] += e * e;
            }
        }
    } else {
        const double *s = train + (int64_t)j * nfeat;
        for (int f = 0; f < nfeat; f++) {
            const double xv = (double)xs[f * xstride];
#pragma unroll
            for (int t = 0; t < TJ; t++) {
                const double e = xv - s[(int64_t)t * nfeat + f];
                d[t] += e * e;
            }
        }
    }
}

template <typename T, int NF, int CAP>
__global__ __launch_bounds__(BLOCK) void classify_knn_kernel(
    const void *const *tab, int nfeat, RowDims R, int64_t rows, const double *__restrict__ train,
    const int32_t *__restrict__ target, int ntrain, int k, const double *__restrict__ classes, int nclasses,
    const double *__restrict__ mean, const double *__restrict__ scale, double *__restrict__ labels,
    double *__restrict__ proba)
{
    extern __shared__ double knn_lds[];
    const int bdim = blockDim.x;
    const T *xs = reinterpret_cast<const T *>(knn_lds) + threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int64_t row = (int64_t)blockIdx.x * bdim + threadIdx.x; row < rows; row += (int64_t)gridDim.x * bdim) {
        int64_t off, loff;
        row_offsets(R, row, off, loff);
        double x[NF > 0 ? NF : 1];
        bool masked = false;
        if (NF > 0) {
#pragma unroll
            for (int f = 0; f < NF; f++) {
                const T v = static_cast<const T *>(tab[f])[off];
                masked |= (v != v);
                x[f] = (double)scaled<T>(v, mean, scale, f);
            }
        } else {
            x[0] = 0.0;
            T *w = reinterpret_cast<T *>(knn_lds) + threadIdx.x;
            for (int f = 0; f < nfeat; f++) {
                const T v = static_cast<const T *>(tab[f])[off];
                masked |= (v != v);
                w[f * bdim] = scaled<T>(v, mean, scale, f);
            }
        }
        if (masked) {
            if (labels) labels[row] = nan;
            if (proba)
                for (int c = 0; c < nclasses; c++) proba[row * nclasses + c] = nan;
            continue;
        }
        KnnBest<CAP> b;
#pragma unroll
        for (int s = 0; s < CAP; s++) {
            b.d[s] = INFINITY;
            b.i[s] = 0;
        }
        b.kth = INFINITY;
        int j = 0;
        for (; j + KNN_TILE <= ntrain; j += KNN_TILE) {
            double d[KNN_TILE];
            knn_distances<NF, KNN_TILE, T>(d, x, xs, bdim, train, nfeat, j);
#pragma unroll
            for (int t = 0; t < KNN_TILE; t++) knn_offer<CAP>(b, d[t], j + t, k);
        }
        for (; j < ntrain; j++) {
            double d[1];
            knn_distances<NF, 1, T>(d, x, xs, bdim, train, nfeat, j);
            knn_offer<CAP>(b, d[0], j, k);
        }
        // the neighbours' classes; positions k .. CAP-1 of the list are no neighbours
        int tc[CAP];
#pragma unroll
        for (int s = 0; s < CAP; s++) tc[s] = (s < k) ? target[b.i[s]] : -1;
        int bestn = -1, besti = 0;
        for (int c = 0; c < nclasses; c++) {
            int n = 0;
#pragma unroll
            for (int s = 0; s < CAP; s++) n += (tc[s] == c) ? 1 : 0;
            if (proba) proba[row * nclasses + c] = (double)n / (double)k;
            if (n > bestn) {
                bestn = n;
                besti = c;
            }
        }
        if (labels) labels[row] = classes[besti];
    }
}

// ---- linear classifiers -----------------------------------------------------------------------
// One lane per row; a coefficient is the same for every lane: wave-uniform loads.  NC decision values
// in registers; a model with more rows of coefficients is served in passes of NC that re-read the
// features and keep a running maximum.  Probabilities are finished in the output itself: the decision
// values are written there, then every lane re-reads its own row, so the sums run in class order for
// any number of classes.
__device__ __forceinline__ double expit(double s)
{
    if (s < 0.0) {
        const double e = exp(s);
        return e / (1.0 + e);
    }
    return 1.0 / (1.0 + exp(-s));
}

template <typename T, int NC>
__global__ __launch_bounds__(BLOCK) void classify_linear_kernel(
    const void *const *tab, int nfeat, RowDims R, int64_t rows, const double *__restrict__ coef,
    const double *__restrict__ intercept, int ncoef, const double *__restrict__ classes, int link, int output,
    const double *__restrict__ mean, const double *__restrict__ scale, double *__restrict__ out)
{
    __shared__ const void *sbase[MAX_LDS_FEATURES];
    stage_table<0>(sbase, tab, nfeat);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int nclasses = ncoef == 1 ? 2 : ncoef;
    const int width = output == ND_AMD_LINEAR_LABELS ? 1 : (output == ND_AMD_LINEAR_DECISION ? ncoef : nclasses);
    for (int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x; row < rows; row += (int64_t)gridDim.x * BLOCK) {
        int64_t off, loff;
        row_offsets(R, row, off, loff);
        double *o = out + row * width;
        bool masked = false;
        double best = -INFINITY;
        int besti = 0;
        for (int c0 = 0; c0 < ncoef && !masked; c0 += NC) {
            double acc[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) acc[c] = (c0 + c < ncoef) ? intercept[c0 + c] : 0.0;
            for (int f = 0; f < nfeat; f++) {
                const T v = static_cast<const T *>(sbase[f])[off];
                masked |= (v != v);
                const double xv = (double)scaled<T>(v, mean, scale, f);
#pragma unroll
                for (int c = 0; c < NC; c++)
                    if (c0 + c < ncoef) acc[c] += xv * coef[(int64_t)(c0 + c) * nfeat + f];
            }
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c0 + c < ncoef) {
                    if (output != ND_AMD_LINEAR_LABELS && ncoef > 1 && !masked) o[c0 + c] = acc[c];
                    if (acc[c] > best) {
                        best = acc[c];
                        besti = c0 + c;
                    }
                }
            }
            if (ncoef == 1) best = acc[0];
        }
        if (masked) {
            for (int c = 0; c < width; c++) o[c] = nan;
            continue;
        }
        if (output == ND_AMD_LINEAR_LABELS) {
            o[0] = ncoef == 1 ? classes[best > 0.0 ? 1 : 0] : classes[besti];
        } else if (output == ND_AMD_LINEAR_DECISION) {
            if (ncoef == 1) o[0] = best;
        } else if (ncoef == 1) {
            if (link == ND_AMD_LINK_SOFTMAX) {
                const double m = fabs(best);
                const double e0 = exp(-best - m), e1 = exp(best - m);
                const double sum = e0 + e1;
                o[0] = e0 / sum;
                o[1] = e1 / sum;
            } else {
                const double p = expit(best);
                o[0] = 1.0 - p;
                o[1] = p;
            }
        } else {
            double sum = 0.0;
            for (int c = 0; c < ncoef; c++) {
                const double p = link == ND_AMD_LINK_SOFTMAX ? exp(o[c] - best) : expit(o[c]);
                o[c] = p;
                sum += p;
            }
            for (int c = 0; c < ncoef; c++) o[c] = o[c] / sum;
        }
    }
}

// ---- host -------------------------------------------------------------------------------------
static int grid_for(int64_t rows)
{
    const int64_t b = ceil_div(rows, BLOCK);
    return (int)(b < 8192 ? b : 8192);
}

}  // namespace

extern "C" size_t nd_amd_classify_workspace_bytes(int nfeat)
{
    if (nfeat < 1 || nfeat > MAX_LDS_FEATURES) return 0;
    return ((size_t)nfeat * sizeof(void *) + 255) / 256 * 256;
}

extern "C" int nd_amd_classify_forest(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                                      const int64_t *strides, const void *nodes, int64_t nnodes,
                                      const double *values, const int32_t *roots, int ntrees,
                                      const double *classes, int nclasses, const double *mean,
                                      const double *scale, double *labels, double *proba, void *workspace,
                                      size_t workspace_bytes, void *hip_stream)
{
    const char *who = "nd_amd_classify_forest";
    int rc = check_table(who, feat, nfeat, dtype, workspace, workspace_bytes);
    if (rc != ND_AMD_OK) return rc;
    RowDims R;
    int64_t rows;
    rc = make_dims(who, sizes, strides, nullptr, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (!nodes || !values || !roots || !classes || nnodes < 1 || nnodes > INT32_MAX || ntrees < 1 || nclasses < 1) {
        set_error("%s: bad forest (%lld nodes, %d trees, %d classes)", who, (long long)nnodes, ntrees, nclasses);
        return ND_AMD_EINVAL;
    }
    if ((mean == nullptr) != (scale == nullptr)) {
        set_error("%s: scaler needs both mean and scale", who);
        return ND_AMD_EINVAL;
    }
    if (!labels && !proba) {
        set_error("%s: no output: labels and proba are both NULL", who);
        return ND_AMD_EINVAL;
    }
    if (rows == 0) return ND_AMD_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    ND_HIP_CHECK(hipMemcpyAsync(workspace, feat, (size_t)nfeat * sizeof(void *), hipMemcpyHostToDevice, st));
    const void *const *tab = (const void *const *)workspace;
    const int grid = grid_for(rows);
    const int4 *nd = (const int4 *)nodes;
    {
        KernelTimer timer(ND_AMD_KERNEL_CLASSIFY_FOREST, st);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            auto features = [&](auto NREG) {
                auto launch = [&](auto NC) {
                    hipLaunchKernelGGL((classify_forest_kernel<T, decltype(NREG)::value, decltype(NC)::value>), dim3(grid),
                                       dim3(BLOCK), 0, st, tab, nfeat, R, rows, nd, values, roots, ntrees, classes, nclasses,
                                       mean, scale, labels, proba);
                };
                if (!pick_le<2, 4>(nclasses, launch)) launch(int_c<8>{});
            };
            if (!pick_le<4, 8>(nfeat, features)) features(int_c<0>{});
        });
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_classify_kmeans(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                                      const int64_t *strides, const double *centers, int k, const double *mean,
                                      const double *scale, double *labels, void *workspace,
                                      size_t workspace_bytes, void *hip_stream)
{
    const char *who = "nd_amd_classify_kmeans";
    int rc = check_table(who, feat, nfeat, dtype, workspace, workspace_bytes);
    if (rc != ND_AMD_OK) return rc;
    RowDims R;
    int64_t rows;
    rc = make_dims(who, sizes, strides, nullptr, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (!centers || k < 1 || !labels) {
        set_error("%s: needs k >= 1 centres and a labels output (k = %d)", who, k);
        return ND_AMD_EINVAL;
    }
    if ((mean == nullptr) != (scale == nullptr)) {
        set_error("%s: scaler needs both mean and scale", who);
        return ND_AMD_EINVAL;
    }
    if (rows == 0) return ND_AMD_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    ND_HIP_CHECK(hipMemcpyAsync(workspace, feat, (size_t)nfeat * sizeof(void *), hipMemcpyHostToDevice, st));
    const void *const *tab = (const void *const *)workspace;
    const int grid = grid_for(rows);
    {
        KernelTimer timer(ND_AMD_KERNEL_CLASSIFY_KMEANS, st);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            auto launch = [&](auto NREG) {
                hipLaunchKernelGGL((classify_kmeans_kernel<T, decltype(NREG)::value>), dim3(grid), dim3(BLOCK), 0, st, tab, nfeat,
                                   R, rows, centers, k, mean, scale, labels);
            };
            if (!pick_le<4, 8>(nfeat, launch)) launch(int_c<0>{});
        });
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_classify_select(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                                      const int64_t *strides, const double *labels, const int64_t *label_strides,
                                      uint8_t *mask, int64_t *block_offsets, int64_t *count, void *workspace,
                                      size_t workspace_bytes, void *hip_stream)
{
    const char *who = "nd_amd_classify_select";
    int rc = check_table(who, feat, nfeat, dtype, workspace, workspace_bytes);
    if (rc != ND_AMD_OK) return rc;
    RowDims R;
    int64_t rows;
    rc = make_dims(who, sizes, strides, labels ? label_strides : nullptr, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (!count || (rows > 0 && (!mask || !block_offsets)) || (labels && !label_strides)) {
        set_error("%s: mask, block_offsets, count (and label_strides with labels) must be given", who);
        return ND_AMD_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (rows == 0) {
        ND_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int64_t), st));
        return ND_AMD_OK;
    }
    ND_HIP_CHECK(hipMemcpyAsync(workspace, feat, (size_t)nfeat * sizeof(void *), hipMemcpyHostToDevice, st));
    const void *const *tab = (const void *const *)workspace;
    const int64_t nblocks = ceil_div(rows, ND_AMD_CLASSIFY_BLOCK_ROWS);
    {
        KernelTimer timer(ND_AMD_KERNEL_CLASSIFY_GATHER, st);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            hipLaunchKernelGGL(classify_select_kernel<T>, dim3((unsigned)nblocks), dim3(BLOCK), 0, st, tab, nfeat, R, rows,
                               labels, mask, block_offsets);
        });
        hipLaunchKernelGGL(classify_scan_kernel, dim3(1), dim3(BLOCK), 0, st, block_offsets, nblocks, count);
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_classify_gather(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                                      const int64_t *strides, const double *labels, const int64_t *label_strides,
                                      const uint8_t *mask, const int64_t *block_offsets, void *X, double *y,
                                      void *workspace, size_t workspace_bytes, void *hip_stream)
{
    const char *who = "nd_amd_classify_gather";
    int rc = check_table(who, feat, nfeat, dtype, workspace, workspace_bytes);
    if (rc != ND_AMD_OK) return rc;
    RowDims R;
    int64_t rows;
    rc = make_dims(who, sizes, strides, labels ? label_strides : nullptr, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (rows == 0) return ND_AMD_OK;
    if (!mask || !block_offsets || !X || (y && !labels) || (labels && !label_strides)) {
        set_error("%s: mask, block_offsets and X must be given, y needs labels and label_strides", who);
        return ND_AMD_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    ND_HIP_CHECK(hipMemcpyAsync(workspace, feat, (size_t)nfeat * sizeof(void *), hipMemcpyHostToDevice, st));
    const void *const *tab = (const void *const *)workspace;
    const int64_t nblocks = ceil_div(rows, ND_AMD_CLASSIFY_BLOCK_ROWS);
    {
        KernelTimer timer(ND_AMD_KERNEL_CLASSIFY_GATHER, st);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            hipLaunchKernelGGL(classify_gather_kernel<T>, dim3((unsigned)nblocks), dim3(BLOCK), 0, st, tab, nfeat, R, rows,
                               labels, mask, block_offsets, (T *)X, y);
        });
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

static int class_common(const char *who, const void *var, int dtype, const int64_t *sizes, const int64_t *strides,
                        const double *labels, const int64_t *label_strides, int nclasses, RowDims &R, int64_t &rows)
{
    if (dtype != ND_AMD_F32 && dtype != ND_AMD_F64) {
        set_error("%s: bad dtype %d", who, dtype);
        return ND_AMD_EINVAL;
    }
    if (!label_strides) {
        set_error("%s: label_strides is NULL", who);
        return ND_AMD_EINVAL;
    }
    int rc = make_dims(who, sizes, strides, label_strides, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (nclasses < 1 || nclasses > (1 << 24)) {
        set_error("%s: needs 1 to 2^24 classes, got %d", who, nclasses);
        return ND_AMD_EINVAL;
    }
    if (rows > 0 && (!var || !labels)) {
        set_error("%s: variable or labels pointer is NULL", who);
        return ND_AMD_EINVAL;
    }
    return ND_AMD_OK;
}

extern "C" int nd_amd_class_stats(const void *var, int dtype, const int64_t *sizes, const int64_t *strides,
                                  const double *labels, const int64_t *label_strides, int nclasses, double *sum,
                                  int64_t *count, int64_t *nan_count, void *hip_stream)
{
    const char *who = "nd_amd_class_stats";
    RowDims R;
    int64_t rows;
    int rc = class_common(who, var, dtype, sizes, strides, labels, label_strides, nclasses, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (!sum || !count || !nan_count) {
        set_error("%s: an output pointer is NULL", who);
        return ND_AMD_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    ND_HIP_CHECK(hipMemsetAsync(sum, 0, sizeof(double) * nclasses, st));
    ND_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int64_t) * nclasses, st));
    ND_HIP_CHECK(hipMemsetAsync(nan_count, 0, sizeof(int64_t) * nclasses, st));
    if (rows == 0) return ND_AMD_OK;
    // 2048 blocks: one atomic round per block and class, and far fewer than 2^32 elements per lane
    const int64_t b = ceil_div(rows, BLOCK);
    const int grid = (int)(b < 2048 ? b : 2048);
    unsigned long long *c = (unsigned long long *)count, *nn = (unsigned long long *)nan_count;
    {
        KernelTimer timer(ND_AMD_KERNEL_CLASS_MEAN, st);
        const int mode = nclasses <= STATS_REG_CLASSES ? 0 : (nclasses <= STATS_LDS_CLASSES ? 1 : 2);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            auto launch = [&](auto MODE) {
                hipLaunchKernelGGL((class_stats_kernel<T, decltype(MODE)::value>), dim3(grid), dim3(BLOCK), 0, st, (const T *)var,
                                   R, rows, labels, nclasses, sum, c, nn);
            };
            if (!pick_eq<0, 1>(mode, launch)) launch(int_c<2>{});
        });
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_class_fill(const void *var, void *out, int dtype, const int64_t *sizes,
                                 const int64_t *strides, const double *labels, const int64_t *label_strides,
                                 int nclasses, const void *fill, void *hip_stream)
{
    const char *who = "nd_amd_class_fill";
    RowDims R;
    int64_t rows;
    int rc = class_common(who, var, dtype, sizes, strides, labels, label_strides, nclasses, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (rows == 0) return ND_AMD_OK;
    if (!out || !fill) {
        set_error("%s: out or fill is NULL", who);
        return ND_AMD_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int grid = grid_for(rows);
    {
        KernelTimer timer(ND_AMD_KERNEL_CLASS_MEAN, st);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            hipLaunchKernelGGL(class_fill_kernel<T>, dim3(grid), dim3(BLOCK), 0, st, (const T *)var, (T *)out, R, rows, labels,
                               nclasses, (const T *)fill);
        });
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

// rows of a block of the LDS form: the most of 256, 128, 64 whose image fits in KNN_LDS_BYTES
static int knn_block_rows(int nfeat, size_t elem)
{
    int r = BLOCK;
    while (r > 64 && (size_t)r * nfeat * elem > (size_t)KNN_LDS_BYTES) r >>= 1;
    return r;
}

extern "C" int nd_amd_classify_knn(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                                   const int64_t *strides, const double *train, const int32_t *target, int ntrain,
                                   int k, const double *classes, int nclasses, const double *mean,
                                   const double *scale, double *labels, double *proba, void *workspace,
                                   size_t workspace_bytes, void *hip_stream)
{
    const char *who = "nd_amd_classify_knn";
    int rc = check_table(who, feat, nfeat, dtype, workspace, workspace_bytes);
    if (rc != ND_AMD_OK) return rc;
    RowDims R;
    int64_t rows;
    rc = make_dims(who, sizes, strides, nullptr, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (!train || !target || !classes || ntrain < 1 || nclasses < 1 || k < 1 || k > ntrain) {
        set_error("%s: bad model (%d training samples, %d classes, k = %d)", who, ntrain, nclasses, k);
        return ND_AMD_EINVAL;
    }
    if (k > ND_AMD_CLASSIFY_KNN_MAX_K || nfeat > ND_AMD_CLASSIFY_KNN_MAX_FEATURES) {
        set_error("%s: serves k <= %d and up to %d features (k = %d, %d features)", who, ND_AMD_CLASSIFY_KNN_MAX_K,
                  ND_AMD_CLASSIFY_KNN_MAX_FEATURES, k, nfeat);
        return ND_AMD_EUNSUPPORTED;
    }
    if ((mean == nullptr) != (scale == nullptr)) {
        set_error("%s: scaler needs both mean and scale", who);
        return ND_AMD_EINVAL;
    }
    if (!labels && !proba) {
        set_error("%s: no output: labels and proba are both NULL", who);
        return ND_AMD_EINVAL;
    }
    if (rows == 0) return ND_AMD_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    ND_HIP_CHECK(hipMemcpyAsync(workspace, feat, (size_t)nfeat * sizeof(void *), hipMemcpyHostToDevice, st));
    const void *const *tab = (const void *const *)workspace;
    {
        KernelTimer timer(ND_AMD_KERNEL_CLASSIFY_KNN, st);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            // up to eight features stay in registers; more are staged in LDS (NF = 0), in blocks of fewer rows
            auto features = [&](auto NF) {
                int grid = grid_for(rows), block = BLOCK;
                size_t lds = 0;
                if constexpr (decltype(NF)::value == 0) {
                    block = knn_block_rows(nfeat, sizeof(T));
                    const int64_t b = ceil_div(rows, block);
                    grid = (int)(b < 8192 ? b : 8192);
                    lds = (size_t)block * nfeat * sizeof(T);
                }
                auto launch = [&](auto CAP) {
                    hipLaunchKernelGGL((classify_knn_kernel<T, decltype(NF)::value, decltype(CAP)::value>), dim3(grid), dim3(block),
                                       lds, st, tab, nfeat, R, rows, train, target, ntrain, k, classes, nclasses, mean, scale,
                                       labels, proba);
                };
                if (!pick_le<1, 2, 4, 8, 16>(k, launch)) launch(int_c<32>{});
            };
            if (!pick_eq<1, 2, 3, 4, 5, 6, 7, 8>(nfeat, features)) features(int_c<0>{});
        });
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}

extern "C" int nd_amd_classify_linear(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                                      const int64_t *strides, const double *coef, const double *intercept, int ncoef,
                                      const double *classes, int link, int output, const double *mean,
                                      const double *scale, double *out, void *workspace, size_t workspace_bytes,
                                      void *hip_stream)
{
    const char *who = "nd_amd_classify_linear";
    int rc = check_table(who, feat, nfeat, dtype, workspace, workspace_bytes);
    if (rc != ND_AMD_OK) return rc;
    RowDims R;
    int64_t rows;
    rc = make_dims(who, sizes, strides, nullptr, R, rows);
    if (rc != ND_AMD_OK) return rc;
    if (!coef || !intercept || !classes || ncoef < 1) {
        set_error("%s: bad model (%d rows of coefficients)", who, ncoef);
        return ND_AMD_EINVAL;
    }
    if (link < ND_AMD_LINK_NONE || link > ND_AMD_LINK_OVR || output < ND_AMD_LINEAR_LABELS ||
        output > ND_AMD_LINEAR_PROBA || (output == ND_AMD_LINEAR_PROBA && link == ND_AMD_LINK_NONE)) {
        set_error("%s: bad link %d for output %d", who, link, output);
        return ND_AMD_EINVAL;
    }
    if ((mean == nullptr) != (scale == nullptr)) {
        set_error("%s: scaler needs both mean and scale", who);
        return ND_AMD_EINVAL;
    }
    if (!out) {
        set_error("%s: no output: out is NULL", who);
        return ND_AMD_EINVAL;
    }
    if (rows == 0) return ND_AMD_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    ND_HIP_CHECK(hipMemcpyAsync(workspace, feat, (size_t)nfeat * sizeof(void *), hipMemcpyHostToDevice, st));
    const void *const *tab = (const void *const *)workspace;
    const int grid = grid_for(rows);
    {
        KernelTimer timer(ND_AMD_KERNEL_CLASSIFY_LINEAR, st);
        pick(dtype == ND_AMD_F64, [&](auto F64) {
            using T = std::conditional_t<decltype(F64)::value, double, float>;
            auto launch = [&](auto NC) {
                hipLaunchKernelGGL((classify_linear_kernel<T, decltype(NC)::value>), dim3(grid), dim3(BLOCK), 0, st, tab, nfeat, R,
                                   rows, coef, intercept, ncoef, classes, link, output, mean, scale, out);
            };
            if (!pick_le<1, 2, 4>(ncoef, launch)) launch(int_c<8>{});
        });
    }
    ND_HIP_CHECK(hipGetLastError());
    return ND_AMD_OK;
}
