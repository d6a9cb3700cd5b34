// nd_amd/csrc/common.hpp -- shared host-side plumbing of libnd_amd.so
// (error strings, HIP call checking, per-kernel event timing).
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "entry_args.hpp"   // set_error, ceil_div, the entry checks and grid helpers (host only, no HIP)

namespace nd_amd {

#define ND_HIP_CHECK(expr)                                                        \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess) {                                                   \
            ::nd_amd::set_error("%s failed: %s (%s:%d)", #expr,                   \
                                hipGetErrorString(_e), __FILE__, __LINE__);       \
            return ND_AMD_EHIP;                                                   \
        }                                                                         \
    } while (0)

// Records a start/stop event pair around one kernel launch when timing is on.
struct KernelTimer {
    KernelTimer(int kernel_id, hipStream_t stream);
    ~KernelTimer();
    int slot;
    hipStream_t stream;
};

// Lets `kernel` be launched with `bytes` of dynamic LDS (a launch beyond 64 KB needs the attribute raised first).
// It belongs to the CURRENT device's function object, so callers set it on every launch that needs it.
template <class Kernel>
static inline hipError_t allow_dynamic_lds(Kernel *kernel, size_t bytes)
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes);
}

// A library switch from the environment (README.md lists them all); `def` where it is unset.  Callers keep the
// value in a `static const`: one look per process.
static inline int env_int(const char *name, int def)
{
    const char *e = getenv(name);
    return e ? atoi(e) : def;
}
static inline double env_double(const char *name, double def)
{
    const char *e = getenv(name);
    return e ? atof(e) : def;
}

}  // namespace nd_amd
