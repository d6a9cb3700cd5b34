// nd_amd/csrc/memops.hpp -- how a kernel addresses memory through a buffer descriptor, how a wave streams a contiguous
// run into its LDS image, and how it waits for that, written once.  The only file under nd_amd/csrc that names
// make_buffer_rsrc, raw_buffer_load_* / raw_buffer_store_*, global_load_lds and the two bare waits
// `s_waitcnt vmcnt(0)` / `s_waitcnt lgkmcnt(0)`.  Includes nothing of the omnibus headers: the filters use it too.
//
//   plain part (no HIP, no builtin: tools/check_memops.cpp runs it on a CPU)
//     lds_stage_piece / lds_stage_tail   which bytes of a run lane l moves at step s, and where they land
//   device part
//     buffer_of                  the one buffer descriptor of the library
//     kAuxDefault / kAuxNt       the cache policy of a buffer or LDS-DMA access
//     buffer_load, buffer_load16, buffer_store, buffer_store16   typed accesses through a descriptor
//     PlaneBuffers, plane_buffers                the descriptors of the four dual-pol planes at one element offset
//     lds_dma16 / lds_dma4       one LDS-DMA instruction: 16 / 4 bytes per lane from global memory into the wave's image
//     lds_dma_wait, wave_lds_fence               the two waits
//     Pack<T, N>                 N elements as one aligned register pack (a 16-byte LDS or global access)
//
// What is NOT here, because a helper moved kernels (profiles/memops_codeobj.txt): the staging loop itself -- the four
// pixel-major kernels keep `for (c0 ..) { piece; if (p.width) lds_dma16(..); }` -- and the filters' "four elements
// as one vector access if the wave may, else four scalar ones", which stays at its sites over the typed accesses.
//
// The exception is omnibus_ml.hip.  Its transfers are `buffer_load_dword(x4) ... lds` from inline assembly, because
// they write M0 themselves, reach the rows of an image through the instruction's immediate offset and are waited
// for by COUNT (ml_wait_vm: vmcnt(16 | 4 | 0)) with the workgroup barrier in the same statement (ml_barrier), so
// that transfers of two steps stay in flight behind the wait.  None of that can be said through the builtins here,
// which leave M0 and the wait to the compiler; those helpers and ml_make_rsrc (the descriptor as the four integers
// an assembly operand takes) stay in that file.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define ND_AMD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ND_AMD_HD static inline
#endif

namespace nd_amd {

// ---- the pieces of a staged run ------------------------------------------------------------------------------------
// One LDS-DMA instruction moves kLdsLane bytes per lane: kLdsStep = 1 KiB of consecutive memory to 1 KiB of consecutive
// LDS.  A run of `bytes` bytes is moved in steps s = 0, 1, ..: step s, named by its first byte c0 = s * kLdsStep,
// covers the bytes [c0, c0 + kLdsStep) of the run's whole part (all of it, or with TAIL its multiple of 16), lane l
// its kLdsLane bytes at src().  With TAIL the rest (4, 8 or 12 bytes: the run is a multiple of 4) follows as one
// instruction of 4 bytes per lane.  The
// instruction takes the LDS address of lane 0's piece (`base`, wave-uniform); the hardware adds lane * width, so
// a piece lands at the offset it came from: base + off.
constexpr int kLdsLane = 16, kLdsStep = 64 * kLdsLane, kLdsTailLane = 4;
struct LdsPiece {
    int base;       // byte offset of lane 0's piece, in the run and in the image: what the instruction is given
    int off;        // the lane's piece behind it: lane * width
    int width;      // kLdsLane | kLdsTailLane; 0: the lane moves nothing
    constexpr int src() const { return base + off; }      // byte offset of the lane's piece in the run
};
template <bool TAIL>
ND_AMD_HD int lds_run_whole(const int bytes)
{
    return TAIL ? bytes & ~(kLdsLane - 1) : bytes;
}
// the piece of lane `lane` at the step that begins at byte c0; steps: c0 = 0, kLdsStep, .. < lds_run_whole(bytes)
template <bool TAIL>
ND_AMD_HD LdsPiece lds_stage_piece(const int bytes, const int c0, const int lane)
{
    const int eb = c0 + lane * kLdsLane;
    return {c0, lane * kLdsLane, eb < lds_run_whole<TAIL>(bytes) ? kLdsLane : 0};
}
// (TAIL) the last span of a variable whose series length is not a multiple of the vector: up to three words more,
// behind the whole part and only if lds_run_whole<true>(bytes) < bytes
ND_AMD_HD LdsPiece lds_stage_tail(const int bytes, const int lane)
{
    const int bytes16 = lds_run_whole<true>(bytes);
    return {bytes16, lane * kLdsTailLane, bytes16 + lane * kLdsTailLane < bytes ? kLdsTailLane : 0};
}

}  // namespace nd_amd

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace nd_amd {

// ---- buffer descriptor ---------------------------------------------------------------------------------------------
// The four words of a gfx950 buffer resource: the 48-bit base address with stride 0 in its upper bits (a raw buffer:
// an access is addressed by its byte offset alone), 0x7fffffff = the record count, which for stride 0 is the number
// of BYTES the range check lets through (offsets at and beyond it are dropped: a load returns 0), and 0x00020000 =
// the fourth word: DATA_FORMAT 32 in bits 15 .. 18, which the untyped accesses ignore but which must not be 0, and
// zero elsewhere -- no swizzle, no index stride, no thread-id addressing.  So the descriptor checks nothing the host
// has not checked: every offset a kernel forms (lane offset + scalar offset, unsigned 32-bit) stays below 2^31
// because the host says so before it chooses such a kernel -- series_fits_buffer for the omnibus planes, the
// filters' plane-size checks ((ny * stride + nx) * sizeof(T) < 2^31, next to where they set vec_in / vec_out).
// Built from wave-uniform values only.
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_of(const T *p)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(p), 0, 0x7fffffff, 0x00020000);
}

// ---- cache policy: the aux argument of a buffer or LDS-DMA access ------------------------------------------------------
// kAuxNt = aux bit 1, "nt" on gfx950 (__builtin_nontemporal_* on plain accesses): data that is read once or written
// once bypasses the cache hierarchy's retention.  The omnibus plane reads and LDS-DMA runs (pass A: 1.30 -> 1.14 ms,
// profiles/r01_probe_bandwidth.txt) and the 16-byte output stores of the window filters (boxcar 3 x 3 / 5 x 5 on
// 24 x 4096^2: 0.632 / 0.640 -> 0.612 / 0.620 ms, the fused Gaussian unchanged).  Non-temporal LOADS of the filters'
// rows measured slower (0.611 -> 0.623 ms): those and the scalar tail stores stay kAuxDefault.
constexpr int kAuxDefault = 0, kAuxNt = 2;

// ---- typed access: descriptor (SGPRs) + lane byte offset + scalar byte offset ----------------------------------------
template <typename T, int AUX>
__device__ __forceinline__ T buffer_load(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
    if constexpr (sizeof(T) == 4)
        return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, soff, AUX));
    else
        return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, soff, AUX));
}

// 16 bytes of a lane as one access.  V: a 16-byte vector type (four floats, two doubles)
typedef unsigned memops_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned memops_u32x2 __attribute__((ext_vector_type(2)));
template <typename V, int AUX>
__device__ __forceinline__ V buffer_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff)
{
    static_assert(sizeof(V) == 16, "a 16-byte vector");
    return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, AUX));
}
template <int AUX, typename V>
__device__ __forceinline__ void buffer_store16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, const V v)
{
    static_assert(sizeof(V) == 16, "a 16-byte vector");
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(memops_u32x4, v), rsrc, voff, soff, AUX);
}
template <int AUX, typename T>
__device__ __forceinline__ void buffer_store(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, const T v)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float or double");
    if constexpr (sizeof(T) == 4)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc, voff, soff, AUX);
    else
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(memops_u32x2, v), rsrc, voff, soff, AUX);
}

// ---- the four planes of a dual-pol stack at one element offset ---------------------------------------------------------
// One descriptor per plane (base = element `ub` of the plane, wave-uniform), the lane's byte offset for element lx
// behind it and the byte step between dates: a date's four values are four loads with one scalar offset t * sstep.
// (host: k * st * sizeof(T) < 2^31)
struct PlaneBuffers {
    __amdgpu_buffer_rsrc_t r11, r12r, r12i, r22;
    unsigned voff, sstep;
    // the four values at lane offset vo and scalar offset soff (read once: non-temporal)
    template <typename T>
    __device__ __forceinline__ void load(const unsigned vo, const unsigned soff, T &a, T &b, T &c, T &d) const
    {
        a = buffer_load<T, kAuxNt>(r11, vo, soff);
        b = buffer_load<T, kAuxNt>(r12r, vo, soff);
        c = buffer_load<T, kAuxNt>(r12i, vo, soff);
        d = buffer_load<T, kAuxNt>(r22, vo, soff);
    }
};
template <typename T>
__device__ __forceinline__ PlaneBuffers plane_buffers(const T *c11, const T *c12r, const T *c12i, const T *c22,
                                                      const int64_t ub, const unsigned lx, const int64_t st)
{
    PlaneBuffers pb;
    pb.voff = lx * (unsigned)sizeof(T);
    pb.r11 = buffer_of(c11 + ub);
    pb.r12r = buffer_of(c12r + ub);
    pb.r12i = buffer_of(c12i + ub);
    pb.r22 = buffer_of(c22 + ub);
    pb.sstep = (unsigned)st * (unsigned)sizeof(T);
    return pb;
}

// ---- LDS-DMA -----------------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) unsigned char lds_u8_t;
typedef __attribute__((address_space(1))) const unsigned char glb_u8_t;

// One transfer: 16 (4) bytes per lane from src, the LANE's address in global memory, to dst + 16 (4) * lane, dst being
// the wave-uniform address of lane 0's piece in the wave's LDS image.  No register staging and no wait: a wave issues
// every piece of its runs (lds_stage_piece / lds_stage_tail say which) and calls lds_dma_wait() before the first read.
template <int AUX>
__device__ __forceinline__ void lds_dma16(const unsigned char *src, unsigned char *dst)
{
    __builtin_amdgcn_global_load_lds((glb_u8_t *)src, (lds_u8_t *)dst, 16, 0, AUX);
}
template <int AUX>
__device__ __forceinline__ void lds_dma4(const unsigned char *src, unsigned char *dst)
{
    __builtin_amdgcn_global_load_lds((glb_u8_t *)src, (lds_u8_t *)dst, 4, 0, AUX);
}

// ---- the two waits -----------------------------------------------------------------------------------------------------
// LDS-DMA arrivals are invisible to the compiler (it tracks no dependence from a transfer to an LDS read): the wave
// waits for all its outstanding memory operations by hand before it reads what it staged.
__device__ __forceinline__ void lds_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// LDS operations of one wave complete in order: once the counter is 0, what this wave's lanes wrote is there for
// its other lanes to read, and what they read has been read -- a wave-private image needs no workgroup barrier.
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- N elements as one register pack -----------------------------------------------------------------------------------
template <typename T, int N>
struct alignas(sizeof(T) * N) Pack {
    T v[N];
};

}  // namespace nd_amd
#endif  // __HIPCC__
