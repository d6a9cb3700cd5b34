// nd_amd/csrc/classify_common.hpp -- what the pixel-classification translation units share
// (classify.hip, kmeans_fit.hip): the row addressing of the feature table, the scaler's rounding,
// and the host-side validation of the table and its dimensions.
#pragma once

#include "common.hpp"

namespace {

using namespace nd_amd;

constexpr int BLOCK = 256;
constexpr int MAX_LDS_FEATURES = ND_AMD_CLASSIFY_MAX_FEATURES;             // pointer table staged in LDS: 8 KiB

// Up to four row dimensions, row-major, after the host merged what is contiguous: most stacks arrive
// here as ONE dimension and rows need no division.
struct RowDims {
    int64_t n1, n2, n3;       // sizes of dimensions 1..3 (dimension 0 is whatever remains)
    int64_t s[4];             // element strides of the features
    int64_t ls[4];            // element strides of the labels (0 where they are broadcast)
};

__device__ __forceinline__ void row_offsets(const RowDims &R, int64_t row, int64_t &off, int64_t &loff)
{
    if (R.n1 == 1 && R.n2 == 1 && R.n3 == 1) {
        off = row * R.s[0];
        loff = row * R.ls[0];
        return;
    }
    const int64_t i3 = row % R.n3;
    row /= R.n3;
    const int64_t i2 = row % R.n2;
    row /= R.n2;
    const int64_t i1 = row % R.n1;
    const int64_t i0 = row / R.n1;
    off = i0 * R.s[0] + i1 * R.s[1] + i2 * R.s[2] + i3 * R.s[3];
    loff = i0 * R.ls[0] + i1 * R.ls[1] + i2 * R.ls[2] + i3 * R.ls[3];
}

// StandardScaler.transform as numpy evaluates it in place on X of type T with float64 operands:
// X -= mean_ ; X /= scale_  -- each step computed in float64 and rounded to T.
template <typename T>
__device__ __forceinline__ T scaled(T v, const double *mean, const double *scale, int f)
{
    if (mean != nullptr) {
        v = (T)((double)v - mean[f]);
        v = (T)((double)v / scale[f]);
    }
    return v;
}

template <int NREG>
__device__ __forceinline__ void stage_table(const void **sbase, const void *const *tab, int nfeat)
{
    if (NREG == 0) {
        for (int i = threadIdx.x; i < nfeat; i += BLOCK) sbase[i] = tab[i];
        __syncthreads();
    }
}

// validate, drop dimensions of size 1, merge neighbours that are contiguous in both stride sets
static int make_dims(const char *who, const int64_t *sizes, const int64_t *strides, const int64_t *lstrides,
                     RowDims &R, int64_t &rows)
{
    if (!sizes || !strides) {
        set_error("%s: sizes / strides are NULL", who);
        return ND_AMD_EINVAL;
    }
    int64_t n[4], s[4], ls[4];
    int nd = 0;
    rows = 1;
    for (int d = 0; d < 4; d++) {
        if (sizes[d] < 0) {
            set_error("%s: bad shape (%lld, %lld, %lld, %lld)", who, (long long)sizes[0], (long long)sizes[1],
                      (long long)sizes[2], (long long)sizes[3]);
            return ND_AMD_EINVAL;
        }
        if (strides[d] < 0 || (lstrides && lstrides[d] < 0)) {
            set_error("%s: a stride is negative", who);
            return ND_AMD_EINVAL;
        }
        if (sizes[d] != 0 && rows > (INT64_C(1) << 40) / sizes[d]) {
            set_error("%s: bad shape: more than 2^40 rows", who);
            return ND_AMD_EINVAL;
        }
        rows *= sizes[d];
    }
    for (int d = 0; d < 4; d++) {
        if (sizes[d] == 1) continue;
        const int64_t l = lstrides ? lstrides[d] : 0;
        if (nd > 0 && s[nd - 1] == strides[d] * sizes[d] && ls[nd - 1] == l * sizes[d]) {
            n[nd - 1] *= sizes[d];
            s[nd - 1] = strides[d];
            ls[nd - 1] = l;
        } else {
            n[nd] = sizes[d];
            s[nd] = strides[d];
            ls[nd] = l;
            nd++;
        }
    }
    for (; nd < 4; nd++) {
        n[nd] = 1;
        s[nd] = 0;
        ls[nd] = 0;
    }
    R.n1 = n[1];
    R.n2 = n[2];
    R.n3 = n[3];
    for (int d = 0; d < 4; d++) {
        R.s[d] = s[d];
        R.ls[d] = ls[d];
    }
    return ND_AMD_OK;
}

static int check_table(const char *who, const void *const *feat, int nfeat, int dtype, void *workspace,
                       size_t workspace_bytes)
{
    if (dtype != ND_AMD_F32 && dtype != ND_AMD_F64) {
        set_error("%s: bad dtype %d", who, dtype);
        return ND_AMD_EINVAL;
    }
    if (nfeat < 1 || nfeat > MAX_LDS_FEATURES || !feat) {
        set_error("%s: needs 1 to %d features, got %d", who, MAX_LDS_FEATURES, nfeat);
        return ND_AMD_EINVAL;
    }
    for (int f = 0; f < nfeat; f++) {
        if (!feat[f]) {
            set_error("%s: feature pointer %d is NULL", who, f);
            return ND_AMD_EINVAL;
        }
    }
    if (!workspace || workspace_bytes < nd_amd_classify_workspace_bytes(nfeat)) {
        set_error("%s: workspace missing or smaller than nd_amd_classify_workspace_bytes(%d)", who, nfeat);
        return ND_AMD_EWORKSPACE;
    }
    return ND_AMD_OK;
}

}  // namespace
