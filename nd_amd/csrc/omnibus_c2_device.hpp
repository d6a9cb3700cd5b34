// nd_amd/csrc/omnibus_c2_device.hpp -- device-side pieces of the dual-pol omnibus test shared by
// omnibus.hip and omnibus_ml.hip: pass A's argument block, the dump of a register-held series and
// the two-pass search on a series held in registers (dense_chain); the running state and the search
// shared with the other families come with omnibus_search.hpp.  Moved here verbatim from omnibus.hip (round 4) so that the
// multilooking front end can live in a translation unit of its own.
#pragma once
#include <type_traits>

#include "omnibus_common.hpp"
#include "omnibus_search.hpp"

namespace nd_amd {

// The running state Accum<T> and the statistic over it: omnibus_search.hpp.  The entry forms, as pass A asks them:
template <typename T>
__device__ __forceinline__ T z_stat(const Accum<T> &A, int j, double nlooks, const OmniTabEntry &e)
{
    return z_stat(A, j, nlooks, e.m2rho, e.pklogk);
}
template <typename T>
__device__ __forceinline__ double z_approx(const Accum<T> &A, int j, double nlooks, const OmniTabEntry &e)
{
    return z_approx(A, j, nlooks, e.m2rho, e.pklogk);
}

// A series held in registers goes to its slot d of the dump ([date][4]): one 16-byte store per date.
// EXACT: k == KMAX.
template <typename T, int KMAX, bool EXACT>
__device__ __forceinline__ void dump_series(T *d, const T (&v)[KMAX][4], const int k)
{
#pragma unroll
    for (int t = 0; t < KMAX; ++t) {
        if (EXACT || t < k) {
            Pack<T, 4> q;
            q.v[0] = v[t][0];
            q.v[1] = v[t][1];
            q.v[2] = v[t][2];
            q.v[3] = v[t][3];
            *reinterpret_cast<Pack<T, 4> *>(d + 4 * t) = q;
        }
    }
}

// =========================================================================================
// pass A
// =========================================================================================
template <typename T>
struct OmniGlobalArgs {
    const T *c11, *c12r, *c12i, *c22;
    int64_t nx, nrows;        // pixels per row, rows (flattened to one row when planes are contiguous)
    int64_t sy, sx, st;       // element strides
    int64_t blocks_per_row;
    int k;
    int write_tab;            // block 0 copies `tab` into tab_dev
    double nlooks, alpha;
    OmniTabEntry e;           // constants of the test over all k matrices
    uint8_t *change;
    T *z_out, *p_out;
    // The list of pixels whose global test can fire is kept in kShards independent segments
    // (shard = block index mod kShards), each with its own counter on its own 128-byte line:
    // one counter would serialise ~2e5 wave-level atomics per launch at ~88 per microsecond.
    uint32_t *flag_count;     // [kShards] counters, kCounterStride words apart
    uint32_t *flag_idx;       // [kShards][seg] pixel indices
    uint32_t seg;             // list entries per shard
    OmniTabEntry *tab_dev;
    T *dump;                  // [kShards][dump_cap][date][4] series of the first dump_cap pixels of a shard
    uint32_t dump_cap;
    // Waves in which at least `dense_min` pixels are listed are not listed pixel by pixel: one
    // entry (the pixel index of lane 0) goes to the dense list and omnibus_c2_dense_kernel searches
    // all 64 pixels from registers.  Counter: word 1 of the shard's counter line.
    uint32_t *dense_idx;      // [kShards][segd]
    uint32_t segd;
    int dense_min;            // 65 = never
    // Data-driven choice between the sparse design (this pass + pass B) and the fused search, made
    // on the device: omnibus_c2_sample_kernel counts the candidates among `gate_n` sampled pixels
    // into *gate; both variants are launched and the one the count does not favour returns at
    // once.  gate_mode 0: no gate; 1: run only if the sample is dense; 2: only if it is sparse.
    const uint32_t *gate;
    uint32_t gate_n;
    int gate_mode;
};

// dense <=> at least 1/8 of the sampled pixels pass the global screen (measured break-even of
// pass A + pass B against the fused kernel: ~10 % candidates)
template <typename T>
__device__ __forceinline__ bool omni_gate_skip(const OmniGlobalArgs<T> &g)
{
    if (g.gate_mode == 0) return false;
    const uint32_t hits = __builtin_nontemporal_load(g.gate);
    const bool dense = hits * 8u >= g.gate_n;
    return (g.gate_mode == 1) != dense;
}

constexpr int kGlobalThreads = 256;
constexpr int kRetainThreads = 256;   // block size of the register-retaining pass A
constexpr int kShards = 128;
constexpr int kCounterStride = 32;   // uint32 words between shard counters (128 B)
constexpr int kTimeChunk = 4;

// The loads of the register-retaining pass A: one thread per pixel issues all k x 4 loads at once.
// EXACT (k == KMAX, stride_x == 1): buffer loads through one descriptor per plane (base = first pixel of
// this block, uniform), a per-date scalar byte offset and a 32-bit lane offset -- no 64-bit per-lane
// address arithmetic, which keeps the kernel at 4 waves per SIMD.  Otherwise: plain loads of the dates
// t < k; v[t] of the others stays unset.
template <typename T, int KMAX, bool EXACT>
__device__ __forceinline__ void retain_load_series(const OmniGlobalArgs<T> &g, const int64_t row, const int64_t bpx0,
                                                   const int tid, const bool in, const int k, T (&v)[KMAX][4])
{
    if (EXACT) {
        const int64_t ub = row * g.sy + bpx0;
        const unsigned lx = in ? (unsigned)tid : (unsigned)(g.nx - 1 - bpx0);   // idle lanes re-read the last pixel
        const PlaneBuffers pb = plane_buffers(g.c11, g.c12r, g.c12i, g.c22, ub, lx, g.st);
#pragma unroll
        for (int t = 0; t < KMAX; ++t) {
            const unsigned soff = (unsigned)t * pb.sstep;
            pb.load(pb.voff, soff, v[t][0], v[t][1], v[t][2], v[t][3]);
        }
    } else {
        const int64_t xc = in ? bpx0 + tid : g.nx - 1;
        const int64_t off0 = row * g.sy + xc * g.sx;
#pragma unroll
        for (int t = 0; t < KMAX; ++t) {
            if (t < k) {
                const int64_t off = off0 + (int64_t)t * g.st;
                v[t][0] = __builtin_nontemporal_load(g.c11 + off);
                v[t][1] = __builtin_nontemporal_load(g.c12r + off);
                v[t][2] = __builtin_nontemporal_load(g.c12i + off);
                v[t][3] = __builtin_nontemporal_load(g.c22 + off);
            }
        }
    }
}

// A lane's row of the change map from its mask, where the wave cannot store its rows as one span
// (change_rows_wave_ok): 4-byte pieces if the row allows them, bytes otherwise.
template <int KMAX, typename MT>
__device__ __forceinline__ void store_change_row_lane(uint8_t *res, const int k, const MT mask)
{
    if ((k & 3) == 0 && ((uintptr_t)res & 3) == 0) {
        uint32_t *w = reinterpret_cast<uint32_t *>(res);
#pragma unroll
        for (int q = 0; q < KMAX / 4; ++q)
            if (q < (k >> 2)) w[q] = (mask_nibble(mask, q) * 0x00204081u) & 0x01010101u;
    } else {
        for (int t = 0; t < k; ++t) res[t] = (uint8_t)((mask >> t) & (MT)1);
    }
}

// -----------------------------------------------------------------------------------------
// The search of a sparse wave's own candidates (the wave-search form of pass A): one lane per SEGMENT
// START, the algorithm of omnibus_c2_search_starts_kernel on series the wave has staged in LDS.
//   img   the wave's image [candidate][KMAX dates][4], nc candidates (1 <= nc <= kWaveSearchMax)
//   rows  [candidate][KMAX] bytes, zeroed: the candidate's row of the change map, written here
// Lane l of a group of k - 1 lanes sweeps ts[l:] of the group's candidate once -- one 16-byte LDS read per
// date, the next one in flight -- 64 / (k - 1) candidates per trip.  At step i every lane tests over
// j = i + 1 dates: the constants of the float32 screen (scr, a kernel argument) are one scalar load.
// What the screen cannot decide is evaluated exactly on the spot (exact_tail; full_table: the kernel's
// own copy of the table), so the wave finishes its pixels: nothing is handed on.
// -----------------------------------------------------------------------------------------
constexpr int kWaveSearchMax = kDenseMin - 1;    // candidates of a wave below which it is not searched as a whole
template <typename T, int KMAX>
__device__ __forceinline__ void wave_search_starts(const T *img, uint8_t *rows, const int nc, const int k,
                                                   const double nlooks, const double alpha,
                                                   const DenseScreenEntry *scr, const OmniTabEntry *full_table,
                                                   const int lane)
{
    const int ns = k - 1;                       // segment starts per pixel: 0 .. k - 2
    const int ppw = 64 / ns;                    // candidates per trip
    const int grp = lane / ns;
    const int l0 = lane - grp * ns;
    for (int c0 = 0; c0 < nc; c0 += ppw) {
        const int cand = c0 + grp;
        const bool lact = grp < ppw && cand < nc;
        const int slot = lact ? cand : 0;       // idle lanes read along in candidate 0
        const Pack<T, 4> *src = reinterpret_cast<const Pack<T, 4> *>(img) + slot * KMAX;
        Accum<T> A;
        A.reset();
        Sweep sw;                               // (of the one segment this lane sweeps: l stays)
        sw.begin(true);
        int nx = -1;                            // stop
        Pack<T, 4> qn = src[l0];
        for (int i = 0; i < k; ++i) {           // the lane's date is l0 + i
            const Pack<T, 4> q = qn;
            const int t = l0 + i;
            qn = src[t + 1 < k ? t + 1 : k - 1];
            const bool on = lact && t < k;
            if (on) A.step(q.v[0], q.v[1], q.v[2], q.v[3]);
            const int jj = i + 1;               // wave-uniform
            const bool last = (t == k - 1);
            const bool need = on && sw.need(jj, last);
            const bool fires = test_f32(need, A, jj, nlooks, alpha, scr, full_table);
            sw.note(fires, t);
            if (last && fires) nx = sw.fire_at;              // the global test of ts[l0:] fired (jj >= 2 here)
        }
        const int nxt[1] = {nx};
        follow_starts_chain<1>(nxt, ns, ns, grp, lact && l0 == 0, rows + slot * KMAX);
    }
}


// (series of up to 96 registers: three waves per SIMD; beyond -- 32 float32 / 16 float64 dates and
// more -- two: under the cap of three the search spilled 150 - 230 bytes per lane)
constexpr int chain_waves(const int kmax, const size_t elem) { return kmax * (int)elem <= 96 ? 3 : 2; }
constexpr int chain_nj(const int kmax) { return kmax > 32 ? 64 : 32; }

// -----------------------------------------------------------------------------------------
// The same search in two passes over the registers, linear in k (round 3).
//
// dense_search above walks a triangle: one row per segment start, each row re-adding its dates.
// But single_pixel_change_detection consumes every date ONCE: within a segment the marginal tests
// j = 2, 3, ... extend one running sum date by date, and where one fires the next segment starts at
// that very date (nd/_change.pyx:247-256).  The only thing that looks ahead is the global test of
// ts[l:], asked at each segment start.  So:
//   pass 1 (dates last to first, as in omnibus_c2_stream_kernel): the global test of EVERY start
//           from suffix sums in double, with the rounding band of the reference's forward float
//           sums; two bits per date (fires / cannot fire).
//   pass 2 (dates first to last, date index wave-uniform, every lane busy at every date): each lane
//           carries the reference's own running state of its CURRENT segment -- the four sums in
//           `floating`, started as 0 + a_l, and the double product of the determinants -- adds date
//           t, and decides the marginal test over its j = t - l + 1 dates (bit-identical
//           determinants, tight band; the constants of the lane's own j come from an LDS table).
//           Where it fires: change at t, and if the global test of ts[t:] (pass 1) fires too the
//           state restarts as date t alone; if that test cannot fire the lane is finished; an
//           undecided test of either kind hands the pixel to the exact pass.  At the last date the
//           marginal test IS the global test of the segment, which fired.
// ~105 vector instructions per date in all, whatever the threshold: no rows, no deep searches,
// no divergence.
// -----------------------------------------------------------------------------------------
// MT: unsigned for KMAX <= 32, unsigned long long up to 64 dates
template <typename T, int KMAX, int NJ, typename MT>
__device__ __forceinline__ void dense_chain(const T (&v)[KMAX][4], const int k, const bool active,
                                            const StreamScreen<NJ> &ss, const StreamEntry *tab_lds,
                                            MT &mask_out, bool &handoff_out, bool &cand_out)
{
    static_assert(KMAX <= (int)(8 * sizeof(MT)) && KMAX <= NJ, "mask width");
    // the instantiation serves kmin <= k <= KMAX (8, 16, 24, 32 dates; 48 takes 33 .. 48)
    constexpr int kmin = KMAX == 8 ? 2 : (KMAX == 48 ? 33 : KMAX - 7);
    const T dlo = (T)ss.dlo, dhi = (T)ss.dhi;
    MT gF = 0, gC = 0;
    bool bad = false, dead = false;
    {
        double S11 = 0.0, S12r = 0.0, S12i = 0.0, S22 = 0.0, PP = 1.0;
        int emin = 1, emax = 1;
#pragma unroll
        for (int t = KMAX - 1; t >= 0; --t) {
            // branch-free: elements beyond k hold a copy of a valid date and are masked out
            const bool live = (t < kmin) || (t < k);
            const T a = v[t][0], b = v[t][1], c = v[t][2], d = v[t][3];
            const T det = (a * d) - ((b * b) + (c * c));
            bad = bad | (live & !((a > (T)0) & (det > dlo) & (det < dhi)));
            dead = dead | (live & !((det > (T)0) | (det < (T)0)));
            PP = PP * (live ? (double)det : 1.0);
            S11 += live ? (double)a : 0.0;
            S12r += live ? (double)b : 0.0;
            S12i += live ? (double)c : 0.0;
            S22 += live ? (double)d : 0.0;
            const int jr = k - t;
            const int jj = jr > 0 ? jr : 0;
            const StreamEntry e = ss.e[jj];                  // wave-uniform: one scalar load
            const double pp = S11 * S22;
            const double dets = pp - ((S12r * S12r) + (S12i * S12i));
            const float df = (float)dets;
            bool okd;
            int es, eP;
            float ms, mP;
            if (sizeof(T) == 4) {
                okd = df > 7.888609052210118e-31f;
                log2_parts(df, es, ms);
            } else {
                okd = (dets > 0.0) & (dets < (double)INFINITY);
                log2_parts(dets, es, ms);
            }
            log2_parts(PP, eP, mP);
            emin = eP < emin ? eP : emin;
            emax = eP > emax ? eP : emax;
            const int E = (eP - e.re) - __mul24(jj, es);
            const float x = (float)E + __builtin_fmaf(-e.jf, ms, mP - e.rf);
            const float qq = (float)pp * __builtin_amdgcn_rcpf(df);
            const float rel = e.cj * qq;                     // 1.46 * 5 n u * s11 s22 / det
            const float m2 = e.mj * rel;
            bad = bad | (live & !(okd & (rel < 0.01f)));
            mask_push(gF, x + m2 < e.a);
            mask_push(gC, x - m2 > e.b);
            __builtin_amdgcn_sched_barrier(0);               // one date at a time (registers)
        }
        bad = bad | (emax - emin > 900);
    }
    // KMAX pushes: the bit of date t sits at position t
    MT gI = (MT) ~(gF | gC);
    mask_keep_low(gF, k - 1);
    mask_keep_low(gI, k - 1);
    if (dead) {                                 // a NaN or zero determinant: no change anywhere, no exact pass
        bad = false;
        gF = 0;
        gI = 0;
    }
    cand_out = active && (bad || ((gF | gI) & (MT)1));
    bool handoff = active && (bad || (gI & (MT)1));
    bool done = !active || bad || !(gF & (MT)1) || (gI & (MT)1);
    MT mask = 0;
    // the running state of the segment that starts at date 0 (0 + a_0 = a_0)
    T s11 = v[0][0], s12r = v[0][1], s12i = v[0][2], s22 = v[0][3];
    double PP = (double)((v[0][0] * v[0][3]) - ((v[0][1] * v[0][1]) + (v[0][2] * v[0][2])));
    int j = 1;
#pragma unroll
    for (int t = 1; t < KMAX; ++t) {
        const bool live = (t < kmin) || (t < k);
        const bool last = (t == k - 1);
        T a = v[t][0], b = v[t][1];
        const T c = v[t][2], d = v[t][3];
        // (opaque to the optimiser: it would otherwise keep the 24 determinants of pass 1, and their
        // conversions to double, alive in 72 registers instead of recomputing them here; for the long
        // series also b^2 + c^2, one register per date)
        asm volatile("" : "+v"(a));
        if (KMAX * sizeof(T) > 96) asm volatile("" : "+v"(b));
        const T det = (a * d) - ((b * b) + (c * c));
        s11 = s11 + a;
        s12r = s12r + b;
        s12i = s12i + c;
        s22 = s22 + d;
        PP = PP * (double)det;
        j = j + 1;
        const T dets = (s11 * s22) - ((s12r * s12r) + (s12i * s12i));
        const bool oks = (dets > (T)0) & (dets < (T)INFINITY);
        const StreamEntry *ep = tab_lds + j;                 // the lane's own j
        const int re = ep->re;
        const float rf = ep->rf, ca = ep->a, cb = ep->b;
        int es, eP;
        float ms, mP;
        log2_parts(dets, es, ms);
        log2_parts(PP, eP, mP);
        const int E = (eP - re) - __mul24(j, es);
        const float x = (float)E + __builtin_fmaf(-(float)j, ms, mP - rf);
        const bool fires = last | (oks & (x < ca));
        const bool cant = !last & oks & (x > cb);
        const bool act = !done & live;
        const bool und = act & !(fires | cant);
        const bool f = act & fires;
        handoff = handoff | und;
        mask |= f ? ((MT)1 << t) : (MT)0;                    // :252
        // the segment that starts at t (:255): its global test was decided in pass 1
        const bool gi = (gI >> t) & (MT)1, gf = (gF >> t) & (MT)1;
        handoff = handoff | (f & !last & gi);
        done = done | und | (f & (last | gi | !gf));         // :256, :241-242
        s11 = f ? a : s11;
        s12r = f ? b : s12r;
        s12i = f ? c : s12i;
        s22 = f ? d : s22;
        PP = f ? (double)det : PP;
        j = f ? 1 : j;
        __builtin_amdgcn_sched_barrier(0);
    }
    mask_out = mask;
    handoff_out = handoff;
}

// ---- OmnibusTest(ml=w): multilooking fused into pass A (omnibus_ml.hip) -------------------------
constexpr int kMlTileRows = 12;          // rows of a strip = waves of a block
struct OmniMlPlan {
    int ml;
    int64_t ny, nx;
    int strips, xsegs, segw;             // row strips, segments per strip, output columns per segment
    int64_t nblocks;
    uint32_t seg;                        // list (and dump) entries per shard
};
// false: this (shape, strides, window, dtype) is not covered -- the caller multilooks separately
bool omni_ml_plan(int64_t ny, int64_t nx, int64_t k, int64_t sy, int64_t sx, int64_t st, int ml, int dtype,
                  OmniMlPlan *p);
// ss != null: the search fused in (dense_chain); else the sparse design's pass A (stats: with the z / P
// rasters; list = false: rasters only, no candidate list and no zero-fill)
// -> ND_AMD_OK or ND_AMD_EHIP (the dynamic-LDS opt-in of the current device failed)
int launch_ml_pass_a(const OmniGlobalArgs<float> &g, const OmniTab &tab, const OmniMlPlan &p,
                     const StreamScreen<32> *ss, bool stats, bool list, hipStream_t stream);

}  // namespace nd_amd
