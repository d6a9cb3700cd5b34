/*
 * nd_amd.h -- C ABI of libnd_amd.so, the MI355X (gfx950) implementation of the
 * per-pixel compute path of jnhansen/nd.
 *
 * Every entry point replaces one native (or third-party native) call that the
 * reference's Python layer makes; the reference-side binding a maintainer
 * would add is shown in INTEGRATION.md.  All pointers named `*_dev` / data
 * pointers are DEVICE pointers (HIP), all sizes/strides are in ELEMENTS unless
 * they say bytes.  Calls enqueue work on `hip_stream` and return without
 * synchronising (exceptions are noted per function).  Return value: 0 on
 * success, a negative ND_AMD_E* code otherwise; nd_amd_last_error() returns a
 * thread-local description.  The library never throws and never aborts.
 *
 * Streams and threads.  Every launch, memset and copy of an entry goes to
 * `hip_stream`, nothing to the null stream.  These entries WAIT for the stream
 * before they return, and therefore cannot be captured in a graph:
 *   nd_amd_correlate                     with more than 128 taps (the tap list
 *                                        goes through a host copy);
 *   nd_amd_omnibus_c2, _c2_pixel_major,
 *   nd_amd_omnibus_c3, _c3_pixel_major,
 *   nd_amd_omnibus_diag                  with more than 96 dates (the decision
 *                                        table likewise);
 *   nd_amd_resample_check_table          always (it reads its verdict back);
 *   nd_amd_label_regions,
 *   nd_amd_sieve_regions                 always (they read a word back).
 * No other entry waits for its stream or for the device.  Entries may be
 * called from several host threads at once on different streams: the state
 * the library keeps between calls (hipFFT plans, per stream; decision tables;
 * the error text, per thread) is guarded.  Calls on ONE stream from several
 * threads are the caller's to order: the library takes no lock around the
 * work it enqueues.  The nd_amd_timing_* ring is one per process and is not
 * meant for concurrent callers.
 *
 * No host twins.  SURVEY.md 8(b) sketched a `*_cpu` entry next to every device
 * entry (same arguments on host pointers).  The ABI deliberately has none: the
 * reference interface itself has no such pair (its native calls ARE the host
 * path), the product path has no CPU fallback by rule -- every entry fails with
 * ND_AMD_EINVAL / ND_AMD_EHIP rather than compute on the host -- and the only
 * CPU arithmetic of this repository, oracle/, is test infrastructure that
 * nothing under nd_amd/ may link or call.  A caller that wants the host path
 * keeps calling the reference's own nd._change / nd._filters / scipy.
 *
 * Paths are relative to the reference checkout (/root/reference).
 */
#ifndef ND_AMD_H
#define ND_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ND_AMD_ABI_VERSION 1

/* dtype of the `floating` fused type (nd/_change.pyx:8, nd/_filters.pyx:3) */
#define ND_AMD_F32 0
#define ND_AMD_F64 1

#define ND_AMD_OK            0
#define ND_AMD_EINVAL       -1   /* bad argument */
#define ND_AMD_EWORKSPACE   -2   /* workspace missing or too small */
#define ND_AMD_EHIP         -3   /* a HIP runtime call failed */
#define ND_AMD_ENOSOLUTION  -4   /* nlmeans: find_weight has no solution (ValueError in the reference) */
#define ND_AMD_EUNSUPPORTED -5   /* valid request this build does not cover */
#define ND_AMD_EINTERNAL    -6   /* a bounded loop of the region kernels reached its bound: a bug, never the input */

/* scipy.ndimage border modes accepted by nd_amd_correlate (nd/filters.py:226
 * forwards **kwargs to scipy.ndimage.convolve; default 'reflect') */
#define ND_AMD_MODE_REFLECT  0
#define ND_AMD_MODE_CONSTANT 1
#define ND_AMD_MODE_NEAREST  2
#define ND_AMD_MODE_MIRROR   3
#define ND_AMD_MODE_WRAP     4

/* ids reported by nd_amd_timing_collect */
#define ND_AMD_KERNEL_OMNIBUS_GLOBAL 1
#define ND_AMD_KERNEL_OMNIBUS_SEARCH 2
#define ND_AMD_KERNEL_CORRELATE      3
#define ND_AMD_KERNEL_NLMEANS        4
#define ND_AMD_KERNEL_BOXCAR_TILED   5
#define ND_AMD_KERNEL_NLMEANS_TILED  6
#define ND_AMD_KERNEL_CORRELATE1D    7
#define ND_AMD_KERNEL_RELAYOUT       8
#define ND_AMD_KERNEL_OMNIBUS_DENSE  9
#define ND_AMD_KERNEL_OMNIBUS_FUSED  10   /* pass A with the change-point search fused in */
#define ND_AMD_KERNEL_OMNIBUS_SAMPLE 11   /* density sample that gates the fused form */
#define ND_AMD_KERNEL_OMNIBUS_EXACT  12   /* pass B, exact form behind the register form (marked pixels only) */
#define ND_AMD_KERNEL_COREG_SHIFTS   13   /* nd_amd_coregister_shifts, the whole call (FFTs included) */
#define ND_AMD_KERNEL_COREG_WARP     14   /* nd_amd_warp_translate, the whole call */
#define ND_AMD_KERNEL_RGB_LIMITS     15   /* nd_amd_rgb_limits, the whole call (every selection pass) */
#define ND_AMD_KERNEL_RGB_COMPOSE    16   /* nd_amd_rgb_compose */
#define ND_AMD_KERNEL_CLASSIFY_FOREST 17  /* nd_amd_classify_forest */
#define ND_AMD_KERNEL_CLASSIFY_KMEANS 18  /* nd_amd_classify_kmeans */
#define ND_AMD_KERNEL_CLASSIFY_GATHER 19  /* nd_amd_classify_select (mask + scan) and nd_amd_classify_gather */
#define ND_AMD_KERNEL_CLASS_MEAN      20  /* nd_amd_class_stats and nd_amd_class_fill */
#define ND_AMD_KERNEL_CLASSIFY_KNN    21  /* nd_amd_classify_knn */
#define ND_AMD_KERNEL_CLASSIFY_LINEAR 22  /* nd_amd_classify_linear */
#define ND_AMD_KERNEL_KMEANS_STEP     23  /* nd_amd_kmeans_step: the pass over the rows and the fold of its partials */
#define ND_AMD_KERNEL_FEATURE_MOMENTS 24  /* nd_amd_feature_moments, the whole call (both passes) */
#define ND_AMD_KERNEL_GATHER_ROWS     25  /* nd_amd_gather_rows */
#define ND_AMD_KERNEL_CHANGE_SEGMENTS 26  /* nd_amd_change_segments */
#define ND_AMD_KERNEL_RASTERIZE       27  /* nd_amd_rasterize_polygons, the whole call (clear, fill, resolve) */
#define ND_AMD_KERNEL_RESAMPLE        28  /* nd_amd_resample and nd_amd_resample_nearest */
#define ND_AMD_KERNEL_SPECKLE         29  /* nd_amd_speckle_lee and nd_amd_speckle_multitemporal, the whole call */
#define ND_AMD_KERNEL_REGIONS         30  /* nd_amd_label_regions, nd_amd_region_sizes, nd_amd_sieve_regions, the whole call */
#define ND_AMD_KERNEL_ZONAL           31  /* nd_amd_zonal_keys, nd_amd_zonal_stats, nd_amd_zonal_paint, the whole call */
#define ND_AMD_KERNEL_TEMPORAL        32  /* nd_amd_temporal_stats, the whole call */

/* layouts of nd_amd_warp_translate */
#define ND_AMD_LAYOUT_PLANAR       0   /* (time, row, col), col fastest */
#define ND_AMD_LAYOUT_PIXEL_MAJOR  1   /* (row, col, time), time fastest: the reference's (y, x, time) */

/* rows per block of nd_amd_classify_select / _gather: block_offsets has one entry per that many rows */
#define ND_AMD_CLASSIFY_BLOCK_ROWS 1024
#define ND_AMD_CLASSIFY_MAX_FEATURES 1024
/* nd_amd_classify_knn: neighbours and features it serves, and the training samples of one tile */
#define ND_AMD_CLASSIFY_KNN_MAX_K 32
#define ND_AMD_CLASSIFY_KNN_MAX_FEATURES 128
#define ND_AMD_CLASSIFY_KNN_TILE 8
/* nd_amd_kmeans_step: k * (nfeat + 1) float64 / int64 accumulators per block, 32 KiB of LDS */
#define ND_AMD_KMEANS_FIT_MAX_ACC 4096
/* nd_amd_classify_linear: link (what predict_proba applies to the decision values) and output */
#define ND_AMD_LINK_NONE    0
#define ND_AMD_LINK_SOFTMAX 1   /* exp(s_c - max s) / sum, in class order */
#define ND_AMD_LINK_OVR     2   /* expit(s_c), divided by their sum when there are more than two classes */
#define ND_AMD_LINEAR_LABELS   0
#define ND_AMD_LINEAR_DECISION 1
#define ND_AMD_LINEAR_PROBA    2

/* nd_amd_rasterize_polygons: type of `values`, `fill` and `out` (8-byte elements, copied bit for bit) */
#define ND_AMD_I64 2
/* the region entries: maps of 1-byte (uint8, and bool as 0 / 1) and int32 elements besides the three above */
#define ND_AMD_U8  3
#define ND_AMD_I32 4
/* crossings of one (polygon, row) a wave keeps in its LDS list; rows with more take the per-pixel walk */
#define ND_AMD_RASTERIZE_MAX_CROSSINGS 256
/* nd_amd_resample: the longest run of taps an axis table may hold */
#define ND_AMD_RESAMPLE_MAX_TAPS 256

#define ND_AMD_COREG_MAX_UPSAMPLING 128
#define ND_AMD_COREG_MAX_VARS       16

int nd_amd_abi_version(void);
const char *nd_amd_last_error(void);

/* ------------------------------------------------------------------------
 * OmnibusTest, dual-pol C2.
 * Replaces  nd._change.change_detection(values, alpha, n, njobs)
 *           nd/_change.pyx:263-287, sole caller nd/change.py:69.
 *
 * The reference passes one (y, x, time, 4) strided view whose last axis is
 * [C11, C12__re, C12__im, C22] (nd/change.py:66-67); here the four variables
 * are four plane pointers that share one set of element strides, which is
 * what that view is in memory.  Fast path: stride_x == 1 and 16-byte aligned
 * rows (planar [time][y][x]); any other strides run the generic kernel.
 *
 *   change   : uint8 (y, x, time) C-order, caller-allocated, fully overwritten
 *              (the reference returns a fresh np.zeros array, :275).
 *   z_out,
 *   p_out    : optional (y, x) rasters of dtype `dtype`: the test statistic
 *              -2 rho ln Q and the probability P of the global test over the
 *              whole series (nd/_change.pyx:46-77, 133-151) -- values the
 *              reference only exposes per pixel via its cpdef functions.
 *   workspace: device scratch, 256-byte aligned.  It holds the list of pixels
 *              whose global test can fire and a compact copy of their series
 *              (so the change-point search never re-reads the planes).
 *              nd_amd_omnibus_c2_workspace_bytes() returns the recommended
 *              size (room for the series of 1/8 of the pixels) and, through
 *              *min_bytes, the smallest size the call accepts; anything in
 *              between trades speed on change-rich rasters for memory.
 * njobs has no equivalent: the whole raster is one launch.
 * Series length: any k >= 1; parity-tested up to k = 5200 (tests/
 * test_long_series_gpu.py; fuzzed over 193 .. 4096).  Beyond 192 dates pass B
 * sweeps each listed pixel from memory; its per-j screen constants, 32 (k + 1)
 * bytes, sit in LDS up to the device's limit per block (160 KB on gfx950,
 * k <= 5119) and are read from global memory beyond it.  The first call
 * with a new (k, n_looks, alpha, dtype) tabulates one pair of decision bounds
 * per sub-series length on the host (O(k^2) work, cached); their safety
 * margin grows with k (see omni_bounds) so that very long series stay exact.
 * Fast forms of the regimes in which most pixels change (alpha below ~0.9;
 * chosen by threshold, series length and a device-side sample of the data)
 * cover k <= 192 (as do those of the sparse regime); longer series are still
 * exact but search pixel by pixel.  Where no screen can decide the test over
 * the whole series (omega2 outside [0, 1]: the reference's default n_looks = 1
 * on more than a few dates) that one test is evaluated exactly for every pixel
 * in the first pass, and only the pixels it fires for are searched.
 * ---------------------------------------------------------------------- */
size_t nd_amd_omnibus_c2_workspace_bytes(int dtype, int64_t ny, int64_t nx, int64_t k,
                                         size_t *min_bytes);

/* 1 if nd_amd_omnibus_c2 serves a call with these arguments in the wave-search form of its first pass (a wave
 * searches the few candidates it finds itself; float32, 2 <= k <= 24, no z / P rasters, alpha >= 0.99), 0 if
 * in another form.  Host only; every form gives the same map.  ND_AMD_WAVE_SEARCH=0 (read once per process)
 * turns the form off. */
int nd_amd_omnibus_c2_uses_wave_search(int dtype, int64_t k, int64_t stride_x, double alpha,
                                       uint32_t n_looks, int stats);

int nd_amd_omnibus_c2(const void *c11, const void *c12re, const void *c12im,
                      const void *c22, int dtype,
                      int64_t ny, int64_t nx, int64_t k,
                      int64_t stride_y, int64_t stride_x, int64_t stride_t,
                      uint32_t n_looks, double alpha,
                      uint8_t *change, void *z_out, void *p_out,
                      void *workspace, size_t workspace_bytes,
                      void *hip_stream);

/* ------------------------------------------------------------------------
 * OmnibusTest(ml=w): spatial multilooking fused into the test.
 * Replaces  ds_m = BoxcarFilter(w=ml).apply(ds_m); n = ml ** 2
 *           followed by nd._change.change_detection(values, alpha, n)
 *           nd/change.py:61-69 (BoxcarFilter = scipy.ndimage.convolve with
 *           ones((ml, ml)) / ml**2, mode 'reflect': nd/filters.py:256-267, 294-298).
 *
 * The four planes are read once: every (date, variable) value is the boxcar
 * mean of its ml x ml window in scipy's arithmetic (double products and sums
 * in footprint order, rounded to float32) and exists only in registers; the
 * number of looks is ml * ml.  Results equal nd_amd_correlate on every plane
 * followed by nd_amd_omnibus_c2 bit for bit.
 * Covered: float32, stride_x == 1, ml = 3 or 5, 2 <= k <= 24, ny, nx >= ml;
 * anything else returns ND_AMD_EUNSUPPORTED (and the workspace query 0): the
 * caller then multilooks with nd_amd_correlate and calls nd_amd_omnibus_c2.
 * The workspace must hold the multilooked series of every pixel the test can
 * list (they exist nowhere else): nd_amd_omnibus_c2_ml_workspace_bytes() is
 * the minimum the call accepts; only the listed part is ever touched.
 * ---------------------------------------------------------------------- */
size_t nd_amd_omnibus_c2_ml_workspace_bytes(int dtype, int64_t ny, int64_t nx, int64_t k, int ml);

int nd_amd_omnibus_c2_ml(const void *c11, const void *c12re, const void *c12im,
                         const void *c22, int dtype,
                         int64_t ny, int64_t nx, int64_t k,
                         int64_t stride_y, int64_t stride_x, int64_t stride_t,
                         int ml, double alpha,
                         uint8_t *change, void *z_out, void *p_out,
                         void *workspace, size_t workspace_bytes,
                         void *hip_stream);

/* ------------------------------------------------------------------------
 * OmnibusTest, full-pol C3 (3 x 3 complex Hermitian) -- EXTENSION.
 * The reference has no full-pol implementation (p = 2 is hard-coded,
 * nd/_change.pyx:51, 99, 135); this is the same algorithm with p = 3 and the
 * generic `_f`, `_rho`, `_omega2` of nd/_change.pyx:20-39 (BASELINE.json
 * config "OmnibusTest full-pol C3").  planes[9], all with the same element
 * strides: C11, C22, C33, C12re, C12im, C13re, C13im, C23re, C23im.
 * Everything else as nd_amd_omnibus_c2; k <= 96.
 * Workspace: candidate lists plus, for series of up to 64 dates, room for
 * the series of one pixel in 16 (float32: the sparse regime's pass A hands
 * the candidates' series to the search from its registers; what does not
 * fit is gathered from the planes, slower, never wrong): ~ 6.5 % of the
 * size of a float32 stack.
 * ---------------------------------------------------------------------- */
size_t nd_amd_omnibus_c3_workspace_bytes(int64_t ny, int64_t nx, int64_t k);

int nd_amd_omnibus_c3(const void *const planes[9], int dtype,
                      int64_t ny, int64_t nx, int64_t k,
                      int64_t stride_y, int64_t stride_x, int64_t stride_t,
                      uint32_t n_looks, double alpha,
                      uint8_t *change, void *z_out, void *p_out,
                      void *workspace, size_t workspace_bytes,
                      void *hip_stream);

/* ------------------------------------------------------------------------
 * nd_amd_omnibus_c3 for data in the reference's own layout, without a
 * transpose (the full-pol counterpart of nd_amd_omnibus_c2_pixel_major;
 * nd/change.py:66-67 stacks (y, x, time) variables): plane c holds element
 * (y, x, t) at  planes[c][((y * nx + x) * k + t) * date_stride[c]].
 * date_stride = 1 for a real (y, x, time) array; 2, with
 * planes[c + 1] == planes[c] + 1, for the two halves of an interleaved
 * complex C12 / C13 / C23.  Accepted: nine real arrays, or three real and
 * three interleaved complex ones; 16-byte aligned; k a multiple of 4
 * (float64: of 2) with 9 k elements of 16 pixels within 56 KB; the sparse
 * regime, alpha >= 0.75.  Everything else returns ND_AMD_EUNSUPPORTED --
 * transpose and call nd_amd_omnibus_c3.  The series is folded out of LDS
 * images of the contiguous per-pixel runs, and the search reads a listed
 * pixel's series where it lies (9 runs of k values instead of 9 k values
 * gathered from planes).  Workspace as for nd_amd_omnibus_c3.
 * ---------------------------------------------------------------------- */
int nd_amd_omnibus_c3_pixel_major(const void *const planes[9], int dtype,
                                  int64_t ny, int64_t nx, int64_t k,
                                  const int64_t date_stride[9],
                                  uint32_t n_looks, double alpha, uint8_t *change,
                                  void *z_out, void *p_out,
                                  void *workspace, size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------
 * OmnibusTest for intensity-only stacks (pol = 'diag') -- EXTENSION.
 * The block-diagonal case of the omnibus test: nch = q independent 1 x 1
 * blocks (1 <= q <= 3 real intensity channels, e.g. VV and VH of detected
 * products, which have no C12).  The reference's algorithm
 * (nd/_change.pyx:46-77, 133-151, 224-257) with p replaced by q and a date's
 * determinant by the product of its intensities; f = q (j - 1),
 * rho = 1 - (j/n - 1/(n j)) / (6 (j - 1)), omega2 = -(q (j - 1) / 4) (1 - 1/rho)^2.
 * planes[nch] share one set of element strides; n_looks is a double (> 0,
 * finite: equivalent numbers of looks are not integers).  Every k >= 1 and
 * every alpha is served; rasters of 2^32 - 1 pixels and more return
 * ND_AMD_EUNSUPPORTED.  change (ny, nx, k) uint8 is written whole; z_out /
 * p_out (ny, nx), optional, receive the whole-series statistic and its P.
 * Workspace: 256-byte aligned, nd_amd_omnibus_diag_workspace_bytes() bytes
 * (counters, the per-j table, one u32 per pixel; 0 for invalid arguments).
 * ---------------------------------------------------------------------- */
size_t nd_amd_omnibus_diag_workspace_bytes(int dtype, int nch, int64_t ny, int64_t nx, int64_t k);

int nd_amd_omnibus_diag(const void *const planes[], int nch, int dtype,
                        int64_t ny, int64_t nx, int64_t k,
                        int64_t stride_y, int64_t stride_x, int64_t stride_t,
                        double n_looks, double alpha,
                        uint8_t *change, void *z_out, void *p_out,
                        void *workspace, size_t workspace_bytes,
                        void *hip_stream);

/* ------------------------------------------------------------------------
 * Direction of each detected change and the segment means -- EXTENSION.
 * planes: the real planes an omnibus entry reads, in its order
 *   ND_AMD_STRUCT_DIAG  1..3 intensities
 *   ND_AMD_STRUCT_C2    [C11, C12re, C12im, C22]
 *   ND_AMD_STRUCT_C3    [C11, C22, C33, C12re, C12im, C13re, C13im, C23re, C23im]
 * change (ny, nx, k) bytes as the omnibus entries write them: non-zero at
 * date t >= 1 opens a new segment at t (nd/_change.pyx:253); byte 0 of a
 * pixel is ignored.  Per pixel, in double and in date order: the running
 * sums s_p and the count m of the open segment; at a change
 * mean_p = s_p / m, d_p = x_p[t] - mean_p and
 *   direction[t] = 1  d positive definite   (all d_p > 0 / leading minors > 0)
 *                  2  d negative definite   (all d_p < 0 / minors -, +, -)
 *                  3  anything else (indefinite, singular, any NaN)
 * direction is 0 where no change is declared.  means_p[t] = (T)(s_p / m) of
 * the segment date t lies in, rounded to nearest: the piecewise-constant
 * series the sequential search implies.  No value is special-cased.
 * direction (ny, nx, k) int8 and means (nplanes planes with the strides of
 * `planes`, not overlapping them) are optional, one of them is required.
 * Every k >= 1, every stride combination (fast: stride_x == 1), no
 * workspace.  ND_AMD_EINVAL before any HIP call for a bad dtype, structure,
 * plane count, negative extent, null pointers or no output; ND_AMD_OK for
 * an empty raster.
 * ---------------------------------------------------------------------- */
#define ND_AMD_STRUCT_DIAG 0   /* nplanes 1..3 */
#define ND_AMD_STRUCT_C2   1   /* nplanes 4    */
#define ND_AMD_STRUCT_C3   2   /* nplanes 9    */

int nd_amd_change_segments(const void *const planes[], int nplanes, int structure, int dtype,
                           int64_t ny, int64_t nx, int64_t k,
                           int64_t stride_y, int64_t stride_x, int64_t stride_t,
                           const uint8_t *change,      /* (ny, nx, k) contiguous            */
                           int8_t *direction,          /* (ny, nx, k) contiguous, optional  */
                           void *const means[],        /* nplanes planes, optional, strides */
                           void *hip_stream);          /* of `planes`; must not overlap them */

/* ------------------------------------------------------------------------
 * Kernel convolution / boxcar.
 * Replaces  scipy.ndimage.convolve(arr, nd_kernel, output=output, **kwargs)
 *           as called at nd/filters.py:256-267 (scipy is the reference's
 *           third-party arithmetic for ConvolutionFilter / BoxcarFilter).
 *
 * The host (nd_amd/filters.py) turns the kernel into scipy's footprint: the
 * non-zero taps (|w| > DBL_EPSILON) of the flipped kernel in C order, with
 * per-axis input offsets.  The array is viewed as 4-D (dims[4], missing
 * leading axes = 1) with element strides.  Per output element:
 *   double tmp = 0; for each tap: tmp += w * (double)in[extend(i + off)];
 *   out = (T)tmp          -- same order, double accumulation, no FMA.
 *   offsets : host pointer, ntaps x 4 int64
 *   weights : host pointer, ntaps double
 * Up to 128 taps travel to the kernel as a launch argument (fully asynchronous).
 * Larger footprints are copied into `taps_dev`
 * (>= 24 * ntaps bytes of device memory, may be NULL otherwise); that path
 * synchronises the stream once.
 * ---------------------------------------------------------------------- */
int nd_amd_correlate(const void *in, void *out, int dtype,
                     const int64_t dims[4],
                     const int64_t in_strides[4], const int64_t out_strides[4],
                     int64_t ntaps, const int64_t *offsets, const double *weights,
                     int mode, double cval,
                     void *taps_dev, size_t taps_dev_bytes,
                     void *hip_stream);

/* ------------------------------------------------------------------------
 * 1-D correlation along one axis -- the building block of GaussianFilter.
 * Replaces  scipy.ndimage.correlate1d(input, weights, axis, output, mode, cval, 0)
 *           which scipy.ndimage.gaussian_filter1d calls once per filtered axis
 *           (reference call site nd/filters.py:365-378).
 *
 * scipy's NI_Correlate1D arithmetic, restated: with the weights centred at
 * size1 = n/2, an odd-length kernel that is symmetric to DBL_EPSILON gives
 *   out = x[0] w[0];  for j = -size1..-1:  out += (x[j] + x[-j]) * w[j]
 * (anti-symmetric: x[j] - x[-j]); any other kernel
 *   out = x[size2] w[size2];  for j = -size1..size2-1:  out += x[j] * w[j]
 * all in double, cast to the array dtype on store.  `in` and `out` must not
 * overlap.  weights: host pointer, n <= 255 doubles.
 * ---------------------------------------------------------------------- */
int nd_amd_correlate1d(const void *in, void *out, int dtype,
                       const int64_t dims[4],
                       const int64_t in_strides[4], const int64_t out_strides[4],
                       int axis, int nweights, const double *weights,
                       int mode, double cval, void *hip_stream);

/* ------------------------------------------------------------------------
 * Two 1-D correlations in one pass over memory: along axis 2 (y), then along
 * axis 3 (x), the intermediate array rounded to the array dtype exactly as
 * scipy.ndimage.gaussian_filter does between its per-axis passes (it filters
 * `output` in place from the second axis on) -- GaussianFilter(dims=('y','x'))
 * at nd/filters.py:365-378 on x-contiguous planes.
 * Fused form only: float32, x stride 1, both kernels symmetric (to
 * DBL_EPSILON, as NI_Correlate1D tests) and of the same odd length
 * 3, 5, ..., 13 or 17, any border mode except `constant`.  Everything else
 * returns ND_AMD_EUNSUPPORTED and the caller runs two nd_amd_correlate1d
 * passes (nd_amd/kernels.py does).  `in` and `out` must not overlap.
 * ---------------------------------------------------------------------- */
int nd_amd_correlate1d_yx(const void *in, void *out, int dtype,
                          const int64_t dims[4],
                          const int64_t in_strides[4], const int64_t out_strides[4],
                          int nweights, const double *weights_y, const double *weights_x,
                          int mode, void *hip_stream);

/* ------------------------------------------------------------------------
 * Non-local means.
 * Replaces  nd._filters._pixelwise_nlmeans_3d(arr, output, r, f, sigma, h, n_eff)
 *           nd/_filters.pyx:320-420, sole caller nd/filters.py:462.
 *
 *   arr, out      : (N0, N1, N2, nvars) views, element strides given.
 *   patch_mode    : 0 = what the compiled reference does on LP64 platforms:
 *                   `range(-f[i], f[i]+1)` with an unsigned f starts at
 *                   2^32 - f[i], so the patch loops are empty whenever any
 *                   f[i] > 0 and every neighbour gets weight exp(0) = 1
 *                   (nd/_filters.c:3539-3553); 1 = the signed range the
 *                   source text intends (true patch distances).
 *   neff_policy   : find_weight failure (nd/_filters.pyx:310-311):
 *                   0 = self weight 0, as the shipped Cython-0.29 C does;
 *                   1 = report ND_AMD_ENOSOLUTION, as a Cython>=3 build does.
 *   status_dev    : device int32 the kernel sets to 1 on a find_weight
 *                   failure (policy 1); zeroed by the call.  May be NULL for
 *                   n_eff < 0.  The caller reads it after synchronising.
 *   global_N,
 *   tile_off      : for tiled (multi-GPU) use: `arr` is the tile
 *                   [tile_off, tile_off + N) of an array of shape global_N
 *                   that carries its halo rows, `out` likewise; only
 *                   [core_lo, core_hi) of axis `N` is written and reflection
 *                   happens at the GLOBAL edges.  NULL for any of the four means
 *                   the plain call's value: global_N = N, tile_off = 0,
 *                   core = [0, N).
 * ---------------------------------------------------------------------- */
int nd_amd_nlmeans3d(const void *arr, void *out, int dtype,
                     const int64_t N[3], int64_t nvars,
                     const int64_t in_strides[4], const int64_t out_strides[4],
                     const uint32_t r[3], const uint32_t f[3],
                     double sigma, double h, double n_eff,
                     int patch_mode, int neff_policy, int32_t *status_dev,
                     const int64_t global_N[3], const int64_t tile_off[3],
                     const int64_t core_lo[3], const int64_t core_hi[3],
                     void *hip_stream);

/* ------------------------------------------------------------------------
 * nd_amd_omnibus_c2 for data in the reference's own layout, without a
 * transpose: variable v holds element (y, x, t) at
 *     ptr_v[((y * nx + x) * k + t) * date_stride[v]]
 * (order C11, C12re, C12im, C22).  date_stride = 1 for a real (y, x, time)
 * array; 2, with c12im == c12re + 1, for the two halves of an interleaved
 * complex C12 (read once).  Every threshold up to k = 24 dates (float32;
 * float64: 12), whatever the length (lengths that are not a multiple of the
 * 16-byte vector read the staged spans element by element).  Longer series (up to 192 dates, a multiple of 4 -- float64:
 * of 2 --, 16-byte aligned variables) in the sparse regime, alpha >= 0.75:
 * the series is folded out of LDS images instead of being retained, and the
 * search reads a listed pixel's series where it lies.  Everything else
 * returns ND_AMD_EUNSUPPORTED -- transpose with nd_amd_relayout_planar and
 * call nd_amd_omnibus_c2.  Workspace as for nd_amd_omnibus_c2.
 * ---------------------------------------------------------------------- */
int nd_amd_omnibus_c2_pixel_major(const void *c11, const void *c12re, const void *c12im,
                                  const void *c22, int dtype,
                                  int64_t ny, int64_t nx, int64_t k,
                                  const int64_t date_stride[4],
                                  uint32_t n_looks, double alpha, uint8_t *change,
                                  void *z_out, void *p_out,
                                  void *workspace, size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------
 * Layout change in front of the hot path.  The reference hands its native
 * code a (y, x, time, variable) view with time (and variable) fastest
 * (nd/change.py:66-67: to_array().transpose('y','x','time','variable'));
 * the kernels above read planar (time, y, x) stacks.  For one variable that
 * is already on the device:
 *     out[t * out_date_stride + p] = in[p * k * in_date_stride + t * in_date_stride]
 * p = flattened (y, x) pixel.  in_date_stride = 1 for a real (y, x, time)
 * array, 2 for the real (in = base) or imaginary (in = base + 1) half of an
 * interleaved complex array (C12).  out_date_stride >= npix.
 * ---------------------------------------------------------------------- */
int nd_amd_relayout_planar(const void *in, void *out, int dtype,
                           int64_t npix, int64_t k, int64_t in_date_stride,
                           int64_t out_date_stride, void *hip_stream);

/* Both halves of an interleaved complex (y, x, time) array in one pass (the C12 term):
 *     out_re[t * s + p] = in[(p * k + t) * 2],  out_im[t * s + p] = in[(p * k + t) * 2 + 1]
 * dtype is that of the real components. */
int nd_amd_relayout_planar_complex(const void *in, void *out_re, void *out_im,
                                   int dtype, int64_t npix, int64_t k,
                                   int64_t out_date_stride, void *hip_stream);

/* The way back (filter outputs handed to a caller that keeps the reference's
 * layout, nd/filters.py:139-176):
 *     out[p * k * out_date_stride + t * out_date_stride] = in[t * in_date_stride + p]
 * out_date_stride = 1 or 2 (one half of an interleaved complex array),
 * in_date_stride >= npix. */
int nd_amd_relayout_pixel_major(const void *in, void *out, int dtype,
                                int64_t npix, int64_t k, int64_t in_date_stride,
                                int64_t out_date_stride, void *hip_stream);

/* ------------------------------------------------------------------------
 * Per-kernel timing with HIP events recorded on the caller's stream
 * (bench.py's roofline figures).  enable(capacity) pre-creates the events;
 * collect() synchronises on them and returns (kernel id, milliseconds) pairs
 * in launch order, then resets.  enable(0) turns timing off.  Launches beyond
 * the capacity are not timed; timing_dropped() says how many that were since
 * the last collect().
 * ---------------------------------------------------------------------- */
int nd_amd_timing_enable(int capacity);
int nd_amd_timing_collect(int32_t *kernel_ids, float *ms, int max_n, int *n_out);
int nd_amd_timing_dropped(void);
/* Restrict the timing to the kernel ids whose bit is set in `id_mask` (bit i = id i; 0 = all, the
 * default after every enable).  An event pair costs a few microseconds of stream time: a benchmark
 * that wants the duration of its dominant kernel inside the timed region times only that one. */
int nd_amd_timing_select(uint64_t id_mask);

/* ------------------------------------------------------------------------
 * Interleaved complex -> real and imaginary arrays of the same contiguous
 * shape: the device side of nd.io.disassemble_complex (nd/io.py:26-69,
 * called at nd/change.py:59 and nd/filters.py:132-134) for a variable that
 * is already in (time, y, x) order.  `in`: n complex values of the real type
 * `dtype` (2 n reals), 16-byte aligned like the outputs.
 * ---------------------------------------------------------------------- */
int nd_amd_split_complex(const void *in, void *out_re, void *out_im, int dtype, int64_t n,
                         void *hip_stream);

/* The inverse (nd.io.assemble_complex, nd/io.py:72-123): two real arrays of n
 * elements -> n interleaved complex values.  16-byte aligned pointers. */
int nd_amd_merge_complex(const void *in_re, const void *in_im, void *out, int dtype, int64_t n,
                         void *hip_stream);

/* ------------------------------------------------------------------------
 * Coregistration, step 1: the shift of every date against a reference date.
 * Replaces  skimage.registration.phase_cross_correlation(C11[t], C11[reference],
 *           upsample_factor=upsampling)[0]   (scikit-image 0.18; nd/warp.py:1150-1151)
 * for every date t of one stack at once.
 *
 * c11 holds element (t, y, x) at c11[t * stride_t + y * stride_y + x * stride_x]
 * (element strides; planar and (y, x, time) inputs are copied with the copy
 * engine / nd_amd_relayout_planar, anything else gathered).  Output, device
 * memory: shifts[2 t], shifts[2 t + 1] = (row, col) shift of date t, 0 for the
 * reference date; status[t] = 1 where skimage raises ValueError("NaN values
 * found ...") -- a NaN reached the correlation (a NaN in C11 of date t or of the
 * reference) -- else 0.  Nothing is synchronised.
 * Arithmetic: hipFFT in the input precision (R2C / C2R, plans cached per device,
 * shape, batch and dtype; the first call of a shape builds them), whole-pixel
 * peak = first maximum of |cc| in C order, then for upsampling > 1 the upsampled
 * DFT of R = ceil(1.5 u) x R points around it in complex128.  Sums are ordered
 * differently from numpy's, so a near-tie of two peak values may pick the other:
 * one 1 / u step on such a date.
 * Limits: 1 <= upsampling <= ND_AMD_COREG_MAX_UPSAMPLING, ny * nx < 2^31,
 * k <= 65535.  workspace: >= nd_amd_coregister_shifts_workspace_bytes() bytes,
 * 256-byte aligned (about 3 x the C11 stack plus 96 R (ny + nx) bytes per date);
 * the query returns 0 for arguments the call refuses.
 * ---------------------------------------------------------------------- */
size_t nd_amd_coregister_shifts_workspace_bytes(int dtype, int64_t k, int64_t ny, int64_t nx,
                                                int upsampling);

int nd_amd_coregister_shifts(const void *c11, int dtype, int64_t k, int64_t ny, int64_t nx,
                             int64_t stride_t, int64_t stride_y, int64_t stride_x,
                             int64_t reference, int upsampling,
                             double *shifts, int32_t *status,
                             void *workspace, size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------
 * Coregistration, step 2: translate every plane of `nvars` variables by its
 * date's shift.  Replaces, for every date t != reference and variable v,
 *   skimage.transform.warp(v[t], AffineTransform(translation=(shifts[2 t + 1],
 *                          shifts[2 t])), order=3)            (nd/warp.py:1152-1159)
 * out[r, c] = the Catmull-Rom bicubic of the plane at (r + s_row, c + s_col),
 * taps outside the plane 0 (mode 'constant', cval 0), the sample coordinates
 * formed in the data type (as skimage forms them), then clipped to the plane's
 * own [min, max]; when 0 lies outside that range, outputs exactly 0 stay 0.  A
 * NaN in a plane makes its min / max NaN and so every output of that plane NaN
 * except those exact zeros (reference behaviour).  The reference date (-1:
 * none) is copied unchanged.  in[v], out[v]: device pointers, each variable
 * contiguous in `layout` (ND_AMD_LAYOUT_PLANAR: (k, nr, nc); _PIXEL_MAJOR:
 * (nr, nc, k)), all of dtype `dtype`; outputs are new memory (the call refuses
 * out[v] == in[v] and never writes an input).  shifts: device, k x 2 doubles
 * (nd_amd_coregister_shifts' output).  nvars <= ND_AMD_COREG_MAX_VARS,
 * nvars * k <= 65535.  workspace: >= nd_amd_warp_translate_workspace_bytes(),
 * 256-byte aligned (per-date coordinate tables and per-plane min / max).
 * ---------------------------------------------------------------------- */
size_t nd_amd_warp_translate_workspace_bytes(int dtype, int nvars, int64_t k, int64_t nr, int64_t nc,
                                             int layout);

int nd_amd_warp_translate(const void *const *in, void *const *out, int nvars, int dtype,
                          int64_t k, int64_t nr, int64_t nc, int layout,
                          const double *shifts, int64_t reference,
                          void *workspace, size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------
 * RGB composites, step 1: the stretch limits of every channel plane.
 * Replaces  np.nanpercentile(channel, pmin), np.nanpercentile(channel, pmax)
 * (nd/visualize.py:184, 188) for nframes x nchan planes at once, as numpy 2.2.6
 * computes them for data of type T = dtype.
 *
 * A batch is nframes frames of nchan (1 or 3) channels.  num[c] / den[c]: host
 * arrays of nchan device pointers; channel c of frame f holds element (y, x) at
 *   num[c][f * stride_frame + y * stride_y + x * stride_x]
 * divided (IEEE division in T, never stored) by the same element of den[c] where
 * den is not NULL and den[c] is not NULL.  The strides are in elements, shared by
 * every plane and not negative: (time, y, x) variables have stride_x = 1,
 * (y, x, time) variables stride_frame = 1.  Contiguous planes whose pointers and
 * frame stride are multiples of 16 bytes are read with 16-byte loads.
 *
 * Output, device memory: limits[2 p], limits[2 p + 1] (type T) for plane
 * p = f * nchan + c, counts[p] = its number of non-NaN values n.  Definition:
 * NaNs are dropped and n == 0 gives NaN; infinities are ordinary values;
 * q = T(p) / T(100), vi = T(n - 1) * q, lo = floor(vi), hi = min(lo + 1, n - 1)
 * (both n - 1 where vi >= T(n - 1)), g = vi - lo; with A, B the values of rank
 * lo, hi and d = B - A the result is A + d * g, or B - d * (1 - g) where
 * g >= 0.5: every operation rounded to T, none fused.  For float32 planes of more
 * than 2^24 values the index is therefore as coarse as numpy's.
 * The selection is exact (digit histograms of order-preserving keys: 3 reads of
 * the planes for float32, 6 for float64).  Nothing is synchronised.
 * Limits: 0 <= pmin, pmax <= 100, ny * nx <= 2^31, nframes * nchan <= 65535.
 * workspace: >= nd_amd_rgb_limits_workspace_bytes(dtype, nframes * nchan) bytes,
 * 256-byte aligned (96 KiB per float32 plane, 192 KiB per float64 plane); the
 * query returns 0 for arguments the call refuses.
 * ---------------------------------------------------------------------- */
size_t nd_amd_rgb_limits_workspace_bytes(int dtype, int64_t nplanes);

int nd_amd_rgb_limits(const void *const *num, const void *const *den, int nchan, int dtype,
                      int64_t nframes, int64_t ny, int64_t nx,
                      int64_t stride_frame, int64_t stride_y, int64_t stride_x,
                      double pmin, double pmax, void *limits, int64_t *counts,
                      void *workspace, size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------
 * RGB composites, step 2: the 8-bit image.  Replaces, per channel c of frame f
 * (nd/visualize.py:189-193, 206 without the cv2 calls),
 *   if maxval > minval: channel = (channel - minval) / (maxval - minval) * 255
 *   np.clip(channel as float64, 0, 255).astype(np.uint8);  pixels outside mask = 0
 * Planes as for nd_amd_rgb_limits.  minval / maxval of plane p = f * nchan + c:
 * vmin[c] / vmax[c] (host arrays of nchan doubles, the Python numbers a caller
 * passed) where the array is not NULL, else limits[2 p] / limits[2 p + 1] (device,
 * type T, as nd_amd_rgb_limits wrote them; may be NULL when both arrays are
 * given).  Arithmetic in T as numpy does it: two given numbers are compared and
 * subtracted in double and the span rounded to T; a given number beside a
 * percentile is rounded to T first.  NaN limits, or maxval <= minval, leave the
 * channel unscaled.  NaN and values below 0 give 0, values above 255 give 255,
 * the rest is truncated.  mask: NULL or ny * nx bytes (device), 0 = black.
 * out: device, (nframes, ny, nx, 3) uint8, 4-byte aligned; one channel is
 * replicated into the three bytes.  Nothing is synchronised.
 * ---------------------------------------------------------------------- */
int nd_amd_rgb_compose(const void *const *num, const void *const *den, int nchan, int dtype,
                       int64_t nframes, int64_t ny, int64_t nx,
                       int64_t stride_frame, int64_t stride_y, int64_t stride_x,
                       const void *limits, const double *vmin, const double *vmax,
                       const uint8_t *mask, uint8_t *out, void *hip_stream);

/* ------------------------------------------------------------------------
 * Pixel classification (nd/classify.py).  Common to the nd_amd_classify_*
 * entries: the FEATURE TABLE.  The reference stacks every variable into a host
 * matrix X of (rows, nfeat) (_build_X, nd/classify.py:47-59); here X is never
 * formed.  feat: host array of nfeat (1 .. ND_AMD_CLASSIFY_MAX_FEATURES) device
 * pointers of type T = dtype; sizes[4] / strides[4]: host arrays, the row
 * dimensions (pad with size 1) and their element strides, shared by every
 * feature and not negative.  Row r, counted row-major over sizes, has
 *   X[r, f] = feat[f][i0 * strides[0] + i1 * strides[1] + i2 * strides[2] + i3 * strides[3]].
 * A variable with a feature dimension contributes one pointer per position along
 * it.  Neighbouring dimensions that are contiguous are merged inside the call, so
 * the usual stacks cost no index arithmetic; lanes run along the row index.
 * workspace: >= nd_amd_classify_workspace_bytes(nfeat) device bytes, 256-byte
 * aligned (the pointer table; the query returns 0 for an nfeat the calls refuse).
 * The table is copied with hipMemcpyAsync from `feat`, which may be reused when
 * the call returns.  At most 2^40 rows.  Nothing is synchronised.
 *
 * Optional scaler, mean / scale: device, nfeat doubles each, both or neither.
 * Replaces StandardScaler.transform (nd/classify.py:230) as numpy evaluates it in
 * place on X of type T:  x = T(double(x) - mean[f]);  x = T(double(x) / scale[f]).
 * ---------------------------------------------------------------------- */
size_t nd_amd_classify_workspace_bytes(int nfeat);

/* ------------------------------------------------------------------------
 * Decision forest.  Replaces  clf.predict(X) / clf.predict_proba(X)  and the mask
 * and scatter around it (nd/classify.py:222-241) for scikit-learn's
 * DecisionTreeClassifier, ExtraTreeClassifier, RandomForestClassifier and
 * ExtraTreesClassifier with one output, bit for bit with scikit-learn 1.7.2 at
 * n_jobs = 1.
 *
 * nodes: device, nnodes x 16 bytes {float t32, int32 feature, int32 left, int32 right},
 * 16-byte aligned, node indices absolute.  feature < 0 marks a leaf, whose `left`
 * is its row in values.  values: device, (.., nclasses) doubles, the leaf
 * distributions (tree_.value[node, 0, :]).  roots: device, ntrees int32, in
 * estimator order.  classes: device, nclasses doubles (classes_).
 * scikit-learn casts X to float32 and goes left where float32 x <= float64
 * threshold; for a float32 x that is x <= t32 with t32 the largest float32 not
 * above the threshold, which is what a node stores.  Per row: x_f = float32 of the
 * (scaled) feature, rounded to nearest; for every tree in order walk to a leaf and
 * add its distribution, one float64 add per class; p_c = sum_c / ntrees;
 * labels[r] = classes[first c with the largest p_c].  A row with a NaN feature
 * gives NaN in labels and in every p_c.
 * labels: device, rows doubles, or NULL.  proba: device, (rows, nclasses)
 * doubles, or NULL.  Not both NULL.  The caller guarantees that child and value
 * indices lie inside the arrays and node features below nfeat.
 * ---------------------------------------------------------------------- */
int nd_amd_classify_forest(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                           const int64_t *strides, const void *nodes, int64_t nnodes,
                           const double *values, const int32_t *roots, int ntrees,
                           const double *classes, int nclasses, const double *mean, const double *scale,
                           double *labels, double *proba, void *workspace, size_t workspace_bytes,
                           void *hip_stream);

/* ------------------------------------------------------------------------
 * K-means.  Replaces  KMeans / MiniBatchKMeans .predict(X)  (nd/classify.py:232):
 * centers: device, (k, nfeat) doubles.  d_j = sum over f, in feature order and in
 * float64, of (double(x_f) - centers[j, f])^2 with x_f the (scaled) feature in
 * type T; labels[r] = the first j with the smallest d_j, NaN for a row with a NaN
 * feature.  labels: device, rows doubles.
 * ---------------------------------------------------------------------- */
int nd_amd_classify_kmeans(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                           const int64_t *strides, const double *centers, int k, const double *mean,
                           const double *scale, double *labels, void *workspace, size_t workspace_bytes,
                           void *hip_stream);

/* ------------------------------------------------------------------------
 * k nearest neighbours.  Replaces  KNeighborsClassifier.predict(X) / .predict_proba(X)
 * (nd/classify.py:232) for uniform weights and the Euclidean metric.
 * train: device, (ntrain, nfeat) doubles, the fitted samples (_fit_X).  target:
 * device, ntrain int32, each sample's index into classes (_y).  classes: device,
 * nclasses doubles.  1 <= k <= min(ND_AMD_CLASSIFY_KNN_MAX_K, ntrain) and
 * nfeat <= ND_AMD_CLASSIFY_KNN_MAX_FEATURES, else ND_AMD_EUNSUPPORTED.
 * Per row, with x_f the (scaled) feature in type T:
 *   d_j = sum over f, in feature order and in float64, of (double(x_f) - train[j, f])^2
 * (the product and the sum are two roundings).  The neighbours are the k samples
 * smallest by (d_j, j): of two samples at the same distance the one with the
 * lower index is nearer.  proba[r, c] = (neighbours of class c) / k in float64;
 * labels[r] = classes[first c with the largest count].  A row with a NaN feature
 * gives NaN in labels and in every proba.  labels: device, rows doubles, or NULL.
 * proba: device, (rows, nclasses) doubles, or NULL.  Not both NULL.  The caller
 * guarantees 0 <= target[j] < nclasses and finite train.
 * ---------------------------------------------------------------------- */
int nd_amd_classify_knn(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                        const int64_t *strides, const double *train, const int32_t *target, int ntrain,
                        int k, const double *classes, int nclasses, const double *mean, const double *scale,
                        double *labels, double *proba, void *workspace, size_t workspace_bytes,
                        void *hip_stream);

/* ------------------------------------------------------------------------
 * Linear classifiers.  Replaces  decision_function / predict / predict_proba of
 * scikit-learn's linear models (LinearClassifierMixin, LogisticRegression).
 * coef: device, (ncoef, nfeat) doubles; intercept: device, ncoef doubles.  A
 * binary model has ncoef = 1 and two classes, any other ncoef classes.  classes:
 * device doubles.  Per row, with x_f the (scaled) feature in type T:
 *   s_c = intercept[c] + sum over f, in feature order and in float64, of double(x_f) * coef[c, f]
 * (the product and the sum are two roundings).  out: device doubles,
 *   ND_AMD_LINEAR_LABELS    (rows): classes[s > 0] for a binary model, else classes[first c with the largest s_c]
 *   ND_AMD_LINEAR_DECISION  (rows, ncoef): s
 *   ND_AMD_LINEAR_PROBA     (rows, classes): by `link`.  ND_AMD_LINK_SOFTMAX: e_c = exp(s_c - max s),
 *       p_c = e_c / sum e in class order; a binary model takes the softmax of (-s, s).
 *       ND_AMD_LINK_OVR: p_c = expit(s_c), divided by their sum in class order; a binary model gives
 *       (1 - p, p).  ND_AMD_LINK_NONE with this output is refused.
 * A row with a NaN feature gives NaN in every output.
 * ---------------------------------------------------------------------- */
int nd_amd_classify_linear(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                           const int64_t *strides, const double *coef, const double *intercept, int ncoef,
                           const double *classes, int link, int output, const double *mean,
                           const double *scale, double *out, void *workspace, size_t workspace_bytes,
                           void *hip_stream);

/* ------------------------------------------------------------------------
 * Training rows.  Replaces the masks and boolean indexing of make_Xy
 * (nd/classify.py:164-178):  ymask = ~isnan(labels) & (labels > 0),
 * Xmask = ~isnan(X).any(axis=1),  X = X[ymask][Xmask],  y = labels[ymask][Xmask].
 * labels: device doubles read at the row's offset under label_strides[4] (0 along
 * a dimension the labels are broadcast over), or NULL for an unsupervised fit
 * (then only Xmask applies).
 * nd_amd_classify_select writes mask[r] (rows bytes, 1 = kept), block_offsets[b] =
 * the number of kept rows before row b * ND_AMD_CLASSIFY_BLOCK_ROWS (one int64 per
 * block of rows, rounded up) and *count = the number of kept rows (device).
 * nd_amd_classify_gather, given the same arguments and those two arrays, writes
 * the kept rows in row order -- the order scikit-learn's fit depends on -- into
 * X (device, (count, nfeat) of type T, unscaled) and, where y is not NULL, their
 * labels into y (device, count doubles).  Both are deterministic.
 * ---------------------------------------------------------------------- */
int nd_amd_classify_select(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                           const int64_t *strides, const double *labels, const int64_t *label_strides,
                           uint8_t *mask, int64_t *block_offsets, int64_t *count, void *workspace,
                           size_t workspace_bytes, void *hip_stream);

int nd_amd_classify_gather(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                           const int64_t *strides, const double *labels, const int64_t *label_strides,
                           const uint8_t *mask, const int64_t *block_offsets, void *X, double *y,
                           void *workspace, size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------
 * class_mean (nd/classify.py:36-44), the two device passes around a closed form
 * the caller evaluates on the host.  var: device, one variable of type T over
 * sizes[4] / strides[4] (any order of its dimensions; pass them by decreasing
 * stride for coalesced reads); labels as above.  The class of an element is l
 * where its label equals an integer l in 0 .. nclasses-1, else none.
 * nd_amd_class_stats: sum[l] (float64 sum of the non-NaN values of class l),
 * count[l] (how many) and nan_count[l] (NaN values of class l); device arrays of
 * nclasses entries, zeroed by the call.  Sums are combined with float64 atomics:
 * the last bits may differ from run to run.
 * nd_amd_class_fill: out[e] = fill[l] for an element of class l; for an element
 * of no class its own value, or fill[nclasses] where that is NaN.  fill: device,
 * nclasses + 1 values of type T.  out has var's strides and must not overlap it.
 * ---------------------------------------------------------------------- */
int nd_amd_class_stats(const void *var, int dtype, const int64_t *sizes, const int64_t *strides,
                       const double *labels, const int64_t *label_strides, int nclasses, double *sum,
                       int64_t *count, int64_t *nan_count, void *hip_stream);

int nd_amd_class_fill(const void *var, void *out, int dtype, const int64_t *sizes, const int64_t *strides,
                      const double *labels, const int64_t *label_strides, int nclasses, const void *fill,
                      void *hip_stream);

/* ------------------------------------------------------------------------
 * Training k-means on every row (scikit-learn's lloyd loop; the caller drives the
 * iterations).  The feature table, the scaler and the pointer-table part of the
 * workspace are those of the nd_amd_classify_* entries; a row with a NaN feature
 * is not VALID and takes no part in any sum, as make_Xy drops it
 * (nd/classify.py:164-178).  x_f below is the (scaled) feature in type T.
 *
 * All three reducing passes are DETERMINISTIC: every floating-point sum is formed
 * in an order fixed by (rows, k, nfeat) -- a fixed tree over the 64 rows of a
 * batch, batches in order inside a block, blocks in order -- with no
 * floating-point atomics, so a call repeats its results bit for bit.
 *
 * workspace: >= nd_amd_kmeans_fit_workspace_bytes(nfeat, k, rows) device bytes,
 * 256-byte aligned (the pointer table and the per-block partial sums; k = 1 for
 * nd_amd_feature_moments).  The query returns 0 for a request the calls refuse.
 * Served: k * (nfeat + 1) <= ND_AMD_KMEANS_FIT_MAX_ACC, else ND_AMD_EUNSUPPORTED.
 *
 * nd_amd_kmeans_step: one Lloyd iteration in one pass.  centers: device, (k, nfeat)
 * doubles.  Every valid row is assigned to the first j with the smallest
 *   d_j = sum over f, in feature order and in float64, of (double(x_f) - centers[j, f])^2
 * (the rule of nd_amd_classify_kmeans).  labels: device, rows int32, read and
 * written: labels[r] = j, or -1 for a row that is not valid; *changed = the number
 * of valid rows whose label differs from the value found there (fill with -1
 * before the first iteration: every valid row then counts).  sums: device, (k,
 * nfeat) doubles, sums[j, f] = sum of double(x_f) over the rows of cluster j;
 * counts: device, k int64; *inertia = sum of the smallest d_j over the valid rows
 * (device double); *changed: device int64.  Every output is overwritten.
 *
 * nd_amd_feature_moments: *count = the valid rows (device int64), fmean[f] = sum of
 * double(x_f) / count, fvar[f] = sum of (double(x_f) - fmean[f])^2 / count in a second
 * pass (the population variance); device, nfeat doubles each, NaN where no row is
 * valid.  Serves StandardScaler (mean_, var_) and the tol * mean(var) threshold.
 *
 * nd_amd_gather_rows: X[i, f] = x_f of row index[i] (device, (m, nfeat) of type T),
 * valid[i] = 1 where that row has no NaN feature (device, m bytes).  index: device,
 * m int64 row numbers, counted row-major over sizes, in any order, repeats
 * allowed; an index outside 0 .. rows-1 is not followed: its row of X is NaN and
 * valid[i] = 0.  workspace as for the nd_amd_classify_* entries.
 * ---------------------------------------------------------------------- */
size_t nd_amd_kmeans_fit_workspace_bytes(int nfeat, int k, int64_t rows);

int nd_amd_kmeans_step(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                       const int64_t *strides, const double *centers, int k, const double *mean,
                       const double *scale, int32_t *labels, double *sums, int64_t *counts,
                       double *inertia, int64_t *changed, void *workspace, size_t workspace_bytes,
                       void *hip_stream);

int nd_amd_feature_moments(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                           const int64_t *strides, const double *mean, const double *scale,
                           int64_t *count, double *fmean, double *fvar, void *workspace,
                           size_t workspace_bytes, void *hip_stream);

int nd_amd_gather_rows(const void *const *feat, int nfeat, int dtype, const int64_t *sizes,
                       const int64_t *strides, const int64_t *index, int64_t m, const double *mean,
                       const double *scale, void *X, uint8_t *valid, void *workspace,
                       size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------
 * Polygons burned into a label raster -- the native step under
 * nd.vector.rasterize (nd/vector.py:48-187, rasterio.features.rasterize).
 * The reference's test compares eroded interiors only and pins no boundary
 * rule; THE RULE BELOW IS THIS PROJECT'S.
 *
 * The definition, as the README ("Labels from polygons") states it:
 *
 * A polygon is a set of rings: exterior, holes, and the parts of a
 * MultiPolygon, all together. A ring is m ≥ 3 vertices (X, Y) in float64. A
 * repeated closing vertex is allowed and harmless.
 *
 * The grid is a rotation-free transform (a, 0, c, 0, e, f) with a ≠ 0 and
 * e ≠ 0, either sign. It is the 6-tuple of nd.warp.get_transform
 * (nd/warp.py:189-196):
 *
 * - a = (x[-1] − x[0]) / (len(x) − 1), c = x[0], and likewise e, f from y.
 * - x[0] / y[0] is the corner of pixel (0, 0), as the reference passes it to
 *   rasterio.
 *
 * Vertices go to pixel coordinates on the host, in float64, bracketed as
 * written:
 *
 * - px = (X − c) / a
 * - py = (Y − f) / e
 *
 * The centre of pixel (i, j) is u = j + 0.5, v = i + 0.5. Both are exact in
 * float64.
 *
 * For an edge with endpoints P, Q, let (x1, y1) be the endpoint with the
 * smaller py and (x2, y2) the other. The rule is:
 *
 *     the edge crosses row i        iff  (y1 ≤ v) and not (y2 ≤ v)                    (half-open; y1 == y2 never crosses)
 *     its abscissa                   xc = x1 + ((v − y1) * (x2 − x1)) / (y2 − y1)      (float64, this bracketing, no fma)
 *     pixel (i, j) is inside polygon iff the number of crossing edges of ALL its rings with xc ≤ u is odd
 *
 * What the rule implies:
 *
 * - It is even-odd.
 * - It is half-open on both axes. A square from 0.5 to 2.5 covers pixels 0
 *   and 1, not 2.
 * - Ordering the endpoints by py makes xc identical for the two polygons that
 *   share an edge. Polygons that tile the plane therefore tile the raster: no
 *   pixel is claimed twice or dropped.
 * - The count is independent of the order of edges and rings, so any kernel
 *   structure gives the same bits.
 *
 * Burning follows rasterio.features.rasterize's replace rule. The value of
 * pixel (i, j) in layer l is values[p] of the highest-index polygon p with
 * layer[p] == l that contains the centre. It is fill (default 0) where there
 * is none.
 *
 * Non-finite vertices raise ValueError on the host. Rings with fewer than 3
 * vertices contribute nothing.
 *
 * `verts` holds (px, py).  The Python layer accepts |px|, |py| up to 2^40:
 * below that xc lies within 2^-10 pixel of the edge's extent, which is what
 * lets a box of the extent and one pixel beyond stand for the whole row.
 *
 * row_work / boxes: per polygon a row range r0 <= i < r1 and a column range
 * c0 <= j < c1, clipped to the raster, and the prefix sums of r1 - r0.  They
 * may be any superset of the rows and columns whose centres lie in the
 * polygon's extent: the rule decides, not the box (the kernel clips them to
 * the raster again before it writes).  One wave serves one (polygon, row):
 * its lanes stride over the edges and append xc of the crossing ones to a
 * wave-private LDS list, then stride over the columns and count the entries
 * <= u; odd pixels do atomicMax(owner, p + 1) on a uint32 owner plane in the
 * workspace, which the resolve pass turns into values.  Rows with more than
 * ND_AMD_RASTERIZE_MAX_CROSSINGS crossings count per pixel over all edges
 * with the same expression.  The waves of a fixed-size grid take the items
 * in turn and read the item count from row_work[npolys] on the device, so
 * the call does not synchronise.  Values are 8-byte words copied bit for bit
 * (int64 never passes through a double, NaN payloads and -0.0 survive).
 * All pointers but `fill` are device pointers; `fill` is one host value.
 * ND_AMD_EINVAL before any HIP call for null pointers, a bad dtype, negative
 * extents or strides, npolys >= 2^32 - 1, ny * nx * nlayers >= 2^32 or a
 * workspace that is missing, misaligned (256 bytes) or too small;
 * ND_AMD_OK for an empty raster and for zero polygons (fill everywhere).
 * ---------------------------------------------------------------------- */
size_t nd_amd_rasterize_workspace_bytes(int64_t nlayers, int64_t ny, int64_t nx);

int nd_amd_rasterize_polygons(const double *verts,          /* (nverts, 2) pixel coordinates, device        */
                              const int64_t *ring_offsets,  /* nrings + 1                                   */
                              const int64_t *poly_offsets,  /* npolys + 1, into rings                       */
                              const int32_t *layer,         /* npolys, in [0, nlayers); NULL = all 0        */
                              const int64_t *row_work,      /* npolys + 1: prefix sums of the rows each polygon's clipped box spans */
                              const int32_t *boxes,         /* (npolys, 4) r0, r1, c0, c1 clipped to the raster */
                              const void *values, int value_dtype,      /* npolys, ND_AMD_I64 or ND_AMD_F64 */
                              const void *fill,                         /* one host value of that type      */
                              int64_t npolys, int64_t nlayers, int64_t ny, int64_t nx,
                              void *out, int64_t stride_l, int64_t stride_y, int64_t stride_x,  /* elements */
                              void *workspace, size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------
 * Resampling onto another rotation-free grid -- the native step under
 * nd.warp.Resample, Reprojection (within one coordinate system) and
 * Alignment (nd/warp.py:872-1097, rasterio.warp.reproject).  GDAL is not
 * reproduced bit for bit; THE DEFINITION BELOW IS THIS PROJECT'S.  It is the
 * convention of Pillow's resize and of torch's interpolate(antialias=True):
 * the kernel is stretched by the down-sampling ratio, clipped at the raster's
 * edge and renormalised.
 *
 * A grid is a rotation-free transform (a, 0, c, 0, e, f), a ≠ 0 and e ≠ 0 of
 * either sign, and a size.  Everything on the host is float64, bracketed as
 * written.  Per axis (x shown; y alike with e, f, rows), for a source of n
 * samples with (a_s, c_s) and an output of m samples with (a_d, c_d):
 *
 *     ρ   = |a_d / a_s|
 *     u_j = ((c_d + a_d * (j + 0.5)) − c_s) / a_s     centre of output sample j in source pixel units
 *     output sample j is inside  iff  0 ≤ u_j < n     (false for NaN)
 *
 * The taps of an inside sample are a contiguous run of source indices:
 *
 * - nearest: the one tap floor(u_j), weight 1.
 * - bilinear (R = 1) and cubic (R = 2): s = max(ρ, 1); the taps are
 *   x = max(0, floor(u − R s + 0.5)) … min(n, floor(u + R s + 0.5)) − 1 with
 *   the raw weight φ((x + 0.5 − u) / s).  Bilinear: φ(d) = 1 − |d| for
 *   |d| < 1, else 0.  Cubic is Keys's kernel with a = −0.5:
 *   ((a + 2)|d| − (a + 3))|d|² + 1 for |d| < 1,
 *   (((|d| − 5)|d| + 8)|d| − 4) a for 1 ≤ |d| < 2, else 0.
 * - average: lo = u − ρ/2, hi = u + ρ/2; the taps are
 *   x = max(0, floor(lo)) … min(n, ceil(hi)) − 1 with the raw weight
 *   min(x + 1, hi) − max(x, lo).
 *
 * Taps of weight exactly 0 are trimmed from both ends of the run (zeros inside
 * stay), the weights are divided by their sum, added in tap order, and a run
 * left empty makes the sample outside.
 *
 * Per output pixel (i, j), T the data's type:
 *
 *     if row i and column j are both inside:
 *         acc = 0.0
 *         for r over the row taps, ascending:
 *             h = 0.0
 *             for q over the column taps, ascending:  h = h + wx_q * double(src[r, q])
 *             acc = acc + wy_r * h
 *         out[i, j] = T(acc)                           (one rounding, no fma)
 *     else:
 *         out[i, j] = fill
 *
 * No value is special-cased: a NaN or inf under a tap enters the sum as it is,
 * under an interior zero weight too.  nd_amd_resample_nearest copies the
 * element's bits, out[i, j] = src[floor(v_i), floor(u_j)], for elements of 1,
 * 2, 4 and 8 bytes: NaN payloads and -0.0 survive, integers keep their type.
 *
 * The tables of an axis of m output samples, device memory: start[m] and
 * count[m] int32 (count 0 = outside), weights[taps][m] float64, tap-major,
 * `taps` the longest run.  The kernels do no coordinate arithmetic.  An entry
 * whose run does not lie inside the source extent, or is longer than `taps`,
 * gives fill: nothing outside the stated extent is read whatever the tables
 * hold.  nd_amd_resample_check_table says whether a table has such entries
 * (ND_AMD_EINVAL, "count / start out of range"); it synchronises, the other
 * two entries do not.
 *
 * The data are a batch of nplanes images with an inner axis of length `inner`;
 * src_strides / dst_strides are 4 host values in elements for (plane, y, x,
 * inner).  inner = 1 is a planar stack; inner = k with stride 1 is the
 * reference's (y, x, time) layout.  Lanes run along whichever of x and the
 * inner axis has the smaller stride in the destination; the result is written
 * in the layout the strides state, without a transpose pass.
 * ND_AMD_EINVAL before any HIP call for null pointers, a bad dtype or element
 * size, negative sizes, strides or tap counts; ND_AMD_EUNSUPPORTED for more
 * than ND_AMD_RESAMPLE_MAX_TAPS taps on an axis, for rasters of 2^31 pixels
 * or more per plane on either side and for nplanes * inner of 2^31 or more;
 * ND_AMD_OK for an empty destination.
 * ---------------------------------------------------------------------- */
int nd_amd_resample(const void *src, void *dst, int dtype,             /* ND_AMD_F32 or ND_AMD_F64          */
                    int64_t nplanes, int64_t inner,
                    int64_t src_ny, int64_t src_nx, const int64_t *src_strides,
                    int64_t dst_ny, int64_t dst_nx, const int64_t *dst_strides,
                    const int32_t *start_y, const int32_t *count_y,     /* dst_ny each                       */
                    const double *weights_y, int taps_y,               /* (taps_y, dst_ny)                  */
                    const int32_t *start_x, const int32_t *count_x,     /* dst_nx each                       */
                    const double *weights_x, int taps_x,               /* (taps_x, dst_nx)                  */
                    double fill, void *hip_stream);

int nd_amd_resample_nearest(const void *src, void *dst, int elem_size, /* 1, 2, 4 or 8 bytes                */
                            int64_t nplanes, int64_t inner,
                            int64_t src_ny, int64_t src_nx, const int64_t *src_strides,
                            int64_t dst_ny, int64_t dst_nx, const int64_t *dst_strides,
                            const int32_t *start_y, const int32_t *count_y,
                            const int32_t *start_x, const int32_t *count_x,
                            const void *fill,                          /* one host element                  */
                            void *hip_stream);

int nd_amd_resample_check_table(const int32_t *start, const int32_t *count, int64_t m, /* output samples    */
                                int64_t n, int taps,                   /* source samples, rows of weights   */
                                void *hip_stream);

/* ----------------------------------------------------------------------
 * Speckle filters on detected (intensity) images: the local-statistics
 * filter of Lee 1980 / Kuan et al. 1985 and the temporal filter of Quegan &
 * Yu 2001.  The reference has no counterpart; the definition is this
 * project's, and tests/speckle_ref.py restates it in numpy.
 *
 * Everything is float64, bracketed as written, no fma.  T is the data's type.
 *
 * Window sums.  A plane has ny x nx samples, w is odd, R = w / 2 (integer),
 * N = double(w * w).  The border rule is scipy's 'reflect' (half-sample
 * symmetric), extended periodically so that windows larger than the plane
 * are defined:
 *
 *     refl(i, n):  p = i mod 2n (non-negative);  p if p < n else 2n - 1 - p
 *
 * The sums are separable; each window's sum is formed fresh, taps ascending,
 * rows after columns:
 *
 *     h1[r, j] = 0;  for d = -R .. R:  h1[r, j] = h1[r, j] + double(x[r, refl(j + d, nx)])
 *     h2[r, j] likewise over  double(x) * double(x)
 *     S1[i, j] = 0;  for d = -R .. R:  S1[i, j] = S1[i, j] + h1[refl(i + d, ny), j]      (S2 from h2)
 *
 * No running sums, and no value is special-cased: a NaN, inf, zero or
 * negative sample enters the sums as it is.
 *
 * nd_amd_speckle_lee, per plane, cu2 = 1 / looks computed by the caller:
 *
 *     m = S1 / N
 *     v = S2 / N - m * m
 *     q = ((m * m) * cu2) / v
 *     b = 1 - q                        ND_AMD_SPECKLE_LEE   (Lee 1980 in the form of Lopes et al. 1990)
 *     b = (1 - q) / (1 + cu2)          ND_AMD_SPECKLE_KUAN  (Kuan et al. 1985)
 *     b = b  if (v > 0 and b > 0)  else 0              (a comparison with NaN is false)
 *     out = T(m + b * (double(x) - m))                 (one rounding)
 *
 * nd_amd_speckle_multitemporal, per pixel over the k dates in order and the
 * nvar variables (1 .. ND_AMD_SPECKLE_MAX_VARIABLES) in the order given:
 *
 *     r = 0
 *     for t = 0 .. k-1:  for c = 0 .. nvar-1:  m[c,t] = S1[c,t] / N;  r = r + double(x[c,t]) / m[c,t]
 *     out[c,t] = T((m[c,t] * r) / double(k * nvar))
 *
 * A zero local mean divides as it does.  With k * nvar <=
 * ND_AMD_SPECKLE_HOT_MAX_PLANES the call is one launch that keeps every m in
 * registers (one read, one write of the stack); beyond, pass 1 leaves r in the
 * workspace (ny * nx float64; nd_amd_speckle_multitemporal_workspace_bytes,
 * 0 where none is needed) and pass 2 forms m again.  Both give the same bits;
 * k * nvar alone decides.
 *
 * Strides are 3 host values in elements for (plane or date, y, x), any
 * non-negative values: crops and (y, x, time) data are read where they lie
 * (the latter uncoalesced: not served natively, transpose with
 * nd_amd_relayout_planar for speed).  The variables of a joint call share
 * sizes and strides.  src and dst must not overlap.  A block owns a tile of
 * ND_AMD_SPECKLE_TILE_Y x ND_AMD_SPECKLE_TILE_X outputs
 * (ND_AMD_SPECKLE_HOT_TILE_Y rows in the one-launch multitemporal form).
 * ND_AMD_EINVAL before any HIP call for null pointers, a bad dtype or method,
 * negative sizes or strides, w < 1, cu2 not positive and finite, nvar < 1;
 * ND_AMD_EUNSUPPORTED for an even w or w > ND_AMD_SPECKLE_MAX_W, more than
 * ND_AMD_SPECKLE_MAX_VARIABLES variables and planes of 2^31 pixels or more;
 * ND_AMD_EWORKSPACE for a missing or short workspace; ND_AMD_OK for an empty
 * stack.
 * ---------------------------------------------------------------------- */
#define ND_AMD_SPECKLE_LEE  0
#define ND_AMD_SPECKLE_KUAN 1
#define ND_AMD_SPECKLE_MAX_W 31
#define ND_AMD_SPECKLE_MAX_VARIABLES 4
#define ND_AMD_SPECKLE_HOT_MAX_PLANES 32
#define ND_AMD_SPECKLE_TILE_Y 32
#define ND_AMD_SPECKLE_TILE_X 64
#define ND_AMD_SPECKLE_HOT_TILE_Y 8

int nd_amd_speckle_lee(const void *src, void *dst, int dtype,          /* ND_AMD_F32 or ND_AMD_F64          */
                       int64_t nplanes, int64_t ny, int64_t nx,
                       const int64_t *src_strides, const int64_t *dst_strides,
                       int w, double cu2, int method, void *hip_stream);

size_t nd_amd_speckle_multitemporal_workspace_bytes(int64_t ny, int64_t nx, int64_t k, int nvar);

int nd_amd_speckle_multitemporal(const void *const *src, void *const *dst, int nvar,   /* nvar host pointers */
                                 int dtype, int64_t k, int64_t ny, int64_t nx,
                                 const int64_t *src_strides, const int64_t *dst_strides,
                                 int w, void *workspace, size_t workspace_bytes, void *hip_stream);

/* ----------------------------------------------------------------------
 * Regions of a map: connected-component labelling, region sizes and the
 * sieve (minimum mapping unit) of boolean, class and label maps.  The
 * reference has no counterpart.  The result is pinned by scipy itself:
 * scipy.ndimage.label numbers regions in raster order of their first pixel,
 * which makes the labels a pure function of the input, so the device result
 * equals scipy's everywhere.  tests/regions_ref.py restates the by_value form.
 *
 * A plane v has ny x nx elements of type T: ND_AMD_U8 (bool as 0 / 1),
 * ND_AMD_I32, ND_AMD_I64, ND_AMD_F32 or ND_AMD_F64.
 *
 *   Foreground.  A pixel is foreground iff v != background and v == v: NaN is
 *       always background.  `background` is one host element of type T.
 *   Joined.  Two foreground pixels are joined iff they are neighbours and
 *       (by_value is 0 or their values compare ==).  connectivity 4:
 *       neighbours share an edge; 8: an edge or a corner.  -0.0 == 0.0 holds;
 *       int64 values are compared as int64, never through a double.
 *   Region.  A class of the transitive closure of "joined".
 *   labels[i, j] (int32) is 0 on background, else 1 + the rank of the pixel's
 *       region, regions ranked by the raster index i * nx + j of their first
 *       pixel.  counts[plane] (int64) is the number of regions of the plane.
 *       With by_value 0 this is scipy.ndimage.label(v != background,
 *       structure), structure = generate_binary_structure(2, 1) for 4 and
 *       ones((3, 3)) for 8.
 *   area[i, j] (int32) is the pixel count of the pixel's region, 0 on
 *       background; sizes[l - 1] is the pixel count of region l.
 *   sieve: out = v where the pixel is background (NaN bits kept) or
 *       area >= min_size, elsewhere out = fill (one host element of type T).
 *       min_size <= 1 is a copy.
 *   Batches.  Every plane is labelled on its own and labels restart at 1 per
 *       plane; no link is ever made between planes.
 *
 * nd_amd_label_regions writes labels, area (may be NULL) and counts (device,
 * nplanes) from one labelling.  nd_amd_region_sizes writes sizes[offsets[p] +
 * l - 1] = pixels of label l of plane p from a labelling (integer counts; it
 * does not label again): offsets is a device array of nplanes int64, the
 * exclusive prefix sums of counts; sizes has nsizes elements and is zeroed
 * first; a label outside its plane's range is counted nowhere.
 * nd_amd_sieve_regions writes the sieved planes without materialising labels.
 *
 * Strides are 3 host values in elements for (plane, y, x), none negative:
 * (time, y, x) and (y, x, time) maps, crops and strided outputs are read and
 * written where they lie.  Outputs must not overlap the input or each other.
 *
 * The workspace (nd_amd_regions_workspace_bytes; with_sizes for a labelling
 * with area, and for the sieve) holds an int32 parent per pixel and plane, with
 * sizes another int32, and one int32 per 1024 pixels: 4 or 8 bytes per pixel
 * and plane.  A caller caps it by passing fewer planes per call.
 *
 * The labelling is a union-find whose loops are all bounded by what a correct
 * run cannot reach; a loop that reaches its bound sets a word that
 * nd_amd_label_regions and nd_amd_sieve_regions read back before they return:
 * these two entries WAIT for the stream (they cannot be captured in a graph)
 * and return ND_AMD_EINTERNAL then.  nd_amd_region_sizes does not wait.
 * ND_AMD_EINVAL before any HIP call for a bad dtype or connectivity, negative
 * sizes or strides and null pointers; ND_AMD_EUNSUPPORTED for planes of 2^31
 * pixels or more (checked before the pointers) and more blocks than a launch
 * holds; ND_AMD_EWORKSPACE for a missing or short workspace; ND_AMD_OK for an
 * empty batch or plane.
 * ---------------------------------------------------------------------- */
size_t nd_amd_regions_workspace_bytes(int64_t nplanes, int64_t ny, int64_t nx, int with_sizes);

int nd_amd_label_regions(const void *src, int dtype, int64_t nplanes, int64_t ny, int64_t nx,
                         const int64_t *src_strides, int connectivity, int by_value,
                         const void *background,                       /* one host element                  */
                         int32_t *labels, const int64_t *label_strides,
                         int32_t *area, const int64_t *area_strides,   /* NULL: no area plane               */
                         int64_t *counts,                              /* device, nplanes                   */
                         void *workspace, size_t workspace_bytes, void *hip_stream);

int nd_amd_region_sizes(const int32_t *labels, const int64_t *label_strides,
                        int64_t nplanes, int64_t ny, int64_t nx,
                        const int64_t *offsets,                        /* device, nplanes                   */
                        int32_t *sizes, int64_t nsizes, void *hip_stream);

int nd_amd_sieve_regions(const void *src, void *dst, int dtype, int64_t nplanes, int64_t ny, int64_t nx,
                         const int64_t *src_strides, const int64_t *dst_strides,
                         int connectivity, int by_value,
                         const void *background, const void *fill,     /* one host element each             */
                         int64_t min_size, void *workspace, size_t workspace_bytes, void *hip_stream);

/* ----------------------------------------------------------------------
 * Statistics of zones: count, sum, mean, variance, minimum and maximum of
 * every plane of a stack inside every zone of a label map (a rasterized
 * parcel layer, a labelling of regions, a class map), and a zone's statistic
 * painted back onto its pixels.  The reference has no counterpart; the
 * definition is this project's, tests/zonal_ref.py restates it bit for bit and
 * scipy.ndimage.sum_labels / mean / variance / minimum / maximum hold it.
 *
 *   Zones.  A label plane has ny x nx elements of ND_AMD_U8 (bool as 0 / 1),
 *       ND_AMD_I32, ND_AMD_I64, ND_AMD_F32 or ND_AMD_F64.  ids is a strictly
 *       increasing list of n int64 zone ids; NULL stands for 1 .. n.  A pixel
 *       belongs to zone z (rank 0 .. n - 1) iff its label compares equal to
 *       ids[z]; NaN and every other value belong to no zone.  Integer labels
 *       are compared as int64, never through a double; a floating label is
 *       compared as the int64 it equals, if it is whole and in range.
 *   Sequence.  A zone's pixels in raster order of i * nx + j are its
 *       positions p = 0 .. m - 1.  For a data plane of type T (ND_AMD_F32,
 *       ND_AMD_F64) c_p = (double)x_p; a position takes part iff x_p == x_p.
 *       NaN is skipped and counted; nothing else is special: inf, zeros and
 *       negative values enter as they are.
 *   Statistics per (plane, zone):
 *       count (int64)      positions that take part
 *       nan_count (int64)  positions that are NaN
 *       sum                the sum of c_p over the participants, 0.0 with none
 *       min, max           of the participants, NaN with none (the sign of a
 *                          zero is not pinned)
 *       m2                 the sum of (c_p - mean) * (c_p - mean), mean = sum /
 *                          count in one IEEE division, one rounding for the
 *                          difference and one for the product
 *                          (-ffp-contract=off); 0.0 with none
 *       mean = sum / count, var = m2 / (count - ddof) and std = sqrt(var) are
 *       the caller's (nd_amd/kernels.py, nd_amd/zonal.py).
 *   The order of the sums.  Every floating-point sum is formed in one fixed
 *       tree, a function of the zone's own sequence alone -- not of other
 *       zones, the number of planes, the layout, the grid or scheduling -- and
 *       there is no floating-point atomic anywhere:
 *         chunk    64 consecutive positions, summed by the aligned pairwise
 *                  tree: position l with l ^ 1, the pairs with ^ 2, ... ^ 32.
 *                  An operand that is absent (behind the zone's end) or
 *                  skipped (NaN) does not take part: a (+) absent = a.
 *         segment  64 chunks (4096 positions): the chunk sums added
 *                  sequentially in order, chunks without a participant left out
 *         zone     its segment sums added sequentially in order, segments
 *                  without a participant left out
 *       Two calls give the same bytes, and a zone's bytes do not change when
 *       other zones are relabelled or merged.
 *   Paint.  out[i, j] = (T)table[plane, z] for a pixel of zone z; a pixel of
 *       no zone keeps src's value where src is given, else it is (T)fill.
 *
 * nd_amd_zonal_keys writes the dense int32 keys[ny * nx]: the zone's rank, or
 * n for no zone (a binary search in ids where given; ids is a device array).
 * BETWEEN the two entries the CALLER sorts: perm (int32, ny * nx) is the
 * stable argsort of keys, and offsets (int64, n + 1) has offsets[z] = the
 * number of keys < z, so zone z's pixels are perm[offsets[z] .. offsets[z +
 * 1]) in raster order.  nd_amd.kernels.zonal_index does this with torch's
 * stable sort and searchsorted on the device; the library contains no sort.
 * Entries of perm outside the plane and offsets outside 0 .. ny * nx are
 * read as nothing, never followed.
 * nd_amd_zonal_stats takes nplanes data planes (strides: 3 host values in
 * elements for (plane, y, x), none negative: (time, y, x) and (y, x, time)
 * stacks and crops are read where they lie) and writes the outputs, each
 * (nplanes, n) contiguous on the device and each NULL to skip it.  The
 * workspace (nd_amd_zonal_workspace_bytes) holds the partial sums of the
 * segments of zones of more than 4096 pixels: 40 bytes per plane and 2048
 * pixels, and 16 bytes per (plane, zone).  nd_amd_zonal_paint takes keys, a
 * (nplanes, n) float64 table, src (NULL: fill) and dst of type dtype with
 * their strides.  No entry waits for the device.
 * ND_AMD_EINVAL before any HIP call for a bad dtype, negative sizes, n or
 * strides and null pointers; ND_AMD_EUNSUPPORTED for planes of 2^31 pixels or
 * more, for n >= 2^31 - 1 (both checked before the pointers) and for more
 * blocks than a launch holds; ND_AMD_EWORKSPACE for a missing or short
 * workspace; ND_AMD_OK with nothing done for an empty plane or batch, and in
 * nd_amd_zonal_stats for n = 0.
 * ---------------------------------------------------------------------- */
int nd_amd_zonal_keys(const void *labels, int dtype, int64_t ny, int64_t nx,
                      const int64_t *label_strides,                    /* 2 host values: y, x               */
                      const int64_t *ids, int64_t n,                   /* device, n; NULL: 1 .. n           */
                      int32_t *keys, void *hip_stream);

size_t nd_amd_zonal_workspace_bytes(int64_t nplanes, int64_t ny, int64_t nx, int64_t n);

int nd_amd_zonal_stats(const void *values, int dtype, int64_t nplanes, int64_t ny, int64_t nx,
                       const int64_t *strides,
                       const int32_t *perm, const int64_t *offsets, int64_t n,
                       int64_t *count, int64_t *nan_count,             /* (nplanes, n) each, NULL to skip   */
                       double *sum, double *min, double *max, double *m2,
                       void *workspace, size_t workspace_bytes, void *hip_stream);

int nd_amd_zonal_paint(const int32_t *keys, const double *table, int64_t nplanes, int64_t ny, int64_t nx,
                       int64_t n, const void *src, const int64_t *src_strides,   /* NULL: fill               */
                       void *dst, const int64_t *dst_strides, int dtype, double fill, void *hip_stream);

/* ----------------------------------------------------------------------
 * Statistics along time: per-pixel reductions over the dates of a stack --
 * count, sum, mean, second moment, variance, standard deviation, coefficient
 * of variation, minimum and maximum with their dates, the median and any
 * percentiles.  The reference has no counterpart; the moments are this
 * project's definition, the order statistics numpy 2.2.6's
 * (np.nanmedian, np.nanpercentile; np.median, np.percentile with skipna = 0),
 * and tests/temporal_ref.py restates all of it bit for bit.
 *
 *   Per pixel, x[0 .. k - 1] is the series in date order, of type T
 *   (ND_AMD_F32, ND_AMD_F64).  "double" below is float64, bracketed as
 *   written, nothing fused (-ffp-contract=off).  With skipna != 0 the valid
 *   dates are those with x[t] not NaN; with skipna == 0 every date is valid
 *   and NaN enters the arithmetic as it is.
 *       n = the number of valid dates (count); nan_count = the NaN dates
 *           (in both modes)
 *       sum = 0.0;  for valid t ascending:  sum = sum + double(x[t])
 *       mean = sum / double(n)                        (0 / 0 = NaN for n = 0)
 *       m2 = 0.0;   for valid t ascending:  d = double(x[t]) - mean;
 *                                           m2 = m2 + d * d
 *       var = m2 / double(n - ddof) if n - ddof > 0 else NaN
 *       std = sqrt(var), correctly rounded;  cv = std / mean
 *       min, max     the smallest / largest valid value; NaN for n = 0, and
 *                    with skipna == 0 NaN if any date is NaN
 *       argmin, argmax   the first date whose value == min / max; -1 for
 *                    n = 0; with skipna == 0 the first NaN date if there is one
 *       order statistics   the valid values sorted ascending, A_0 <= ... <=
 *                    A_{n-1}; NaN for n = 0, and with skipna == 0 NaN if any
 *                    date is NaN
 *         percentile p   exactly the arithmetic of nd_amd_rgb_limits in T:
 *                    q = T(p) / T(100), vi = T(n - 1) * q, lo = floor(vi),
 *                    hi = min(lo + 1, n - 1) (both n - 1 where vi >= T(n - 1)),
 *                    g = vi - lo, d = A_hi - A_lo; A_lo + d * g, or
 *                    A_hi - d * (1 - g) where g >= 0.5; every operation
 *                    rounded to T
 *         median     A_{(n-1)/2} for odd n, (A_{n/2-1} + A_{n/2}) / T(2) in T
 *                    for even n (np.nanmedian's arithmetic, not percentile 50's)
 *   Infinities are ordinary values and nothing is special-cased.  The sign of
 *   a zero result of min, max, the median or a percentile is not pinned, and
 *   neither are the payload and sign of a NaN result.
 *
 * x holds element (t, y, x) at x[t * strides[0] + y * strides[1] + x *
 * strides[2]]: 3 host values in elements for (series, y, x), none negative;
 * (time, y, x) and (y, x, time) stacks, crops and steps are read where they
 * lie, and a (time, x) variable is ny = 1.  percentiles: a host array of
 * npercentiles values in [0, 100].  Outputs, device memory, each (ny, nx)
 * contiguous and each NULL to skip it: count, nan_count, argmin, argmax int32;
 * sum, mean, m2, var, std, cv float64; min, max, median of type T;
 * percentile_out (npercentiles, ny, nx) of type T.
 *
 * Forms (nd_amd/csrc/temporal.hip), chosen by k, the type, the strides and
 * whether an order statistic is asked for, all giving the same bits: series of at most
 * ND_AMD_TEMPORAL_REG_MAX_* dates are held in registers; order statistics of
 * at most ND_AMD_TEMPORAL_LDS_MAX_* dates are sorted in LDS; the moments alone
 * are served for every k by two walks over memory (through the LDS tile where
 * a series of stride 1 fits it).  No workspace, nothing is synchronised,
 * every launch goes to hip_stream.
 * ND_AMD_EINVAL before any HIP call for a bad dtype, negative sizes or
 * strides, k < 1, ddof < 0, a percentile outside [0, 100] (NaN included) and
 * a null data pointer; ND_AMD_EUNSUPPORTED for planes of 2^31 pixels or more,
 * for order statistics of more than ND_AMD_TEMPORAL_LDS_MAX_* dates and for
 * more than 2^26 - 1 blocks of 64 pixels (only a strided view of that many
 * short rows gets there); ND_AMD_OK with nothing done for an empty plane or
 * when no output is asked for.
 * ---------------------------------------------------------------------- */
#define ND_AMD_TEMPORAL_REG_MAX_F32 64     /* the longest series of the register form                         */
#define ND_AMD_TEMPORAL_REG_MAX_F64 64
#define ND_AMD_TEMPORAL_LDS_MAX_F32 256    /* the longest series whose order statistics are served: a tile of */
#define ND_AMD_TEMPORAL_LDS_MAX_F64 128    /* 64 pixels x k in 64 KiB of LDS                                  */

int nd_amd_temporal_stats(const void *x, int dtype, int64_t k, int64_t ny, int64_t nx,
                          const int64_t *strides,                      /* 3 host values: series, y, x       */
                          int skipna, int ddof,
                          const double *percentiles, int npercentiles, /* host                              */
                          int32_t *count, int32_t *nan_count,          /* (ny, nx) each, NULL to skip       */
                          double *sum, double *mean, void *min, void *max,
                          int32_t *argmin, int32_t *argmax,
                          double *m2, double *var, double *std, double *cv,
                          void *median, void *percentile_out,          /* (npercentiles, ny, nx)            */
                          void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* ND_AMD_H */
