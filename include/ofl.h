/*
 * ofl.h -- C ABI of the MI355X-native optical-flow-field engine (libofl_hip.so).
 *
 * The reference (oflibnumpy 1.1.1, pure Python) has no FFI; its hot path funnels through ONE
 * Python seam, `apply_flow(flow, target, ref, mask)` (src/oflibnumpy/utils.py:199-261), plus the
 * expressions built on it in src/oflibnumpy/flow_class.py.  Every entry point below names the
 * reference lines it replaces.  A maintainer binds these with ctypes.
 *
 * Conventions
 *   - plain C types only: pointers, sizes, ints.  No torch / numpy types.
 *   - every function returns OFL_OK (0) or a negative OFL_E* code; ofl_last_error() gives the text.
 *   - *_dev entry points take DEVICE pointers (from ofl_malloc) and a stream handle (NULL = the
 *     library's default stream); they enqueue work and return without synchronising.
 *   - host entry points (no suffix) take caller-owned, C-contiguous HOST buffers, do
 *     H2D -> kernel -> D2H on the default stream and return when the result is in host memory.
 *     Each call stages its arrays in ONE device allocation (every array on a 16-byte boundary, so the
 *     _dev entry behind it takes its aligned kernel route) and frees it before it returns, after a
 *     failure too: nothing is retained and nothing is left queued.
 *   - layouts: flow vecs float32 [H][W][2] (channel 0 = x / horizontal, 1 = y / vertical),
 *     masks uint8 [H][W] with values 0/1, images [H][W][C] C-contiguous.
 *   - one process drives one GPU (ofl_init(device) once per process); the library is re-entrant
 *     across streams of that device.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry fails with
 *     OFL_E_NODEVICE.
 */
#ifndef OFL_H
#define OFL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFL_ABI_VERSION 4

/* status codes */
enum {
    OFL_OK          = 0,
    OFL_E_INVALID   = -1,   /* bad argument (shape, dtype, NULL pointer, unsupported combination) */
    OFL_E_NODEVICE  = -2,   /* no HIP device / ofl_init not called */
    OFL_E_HIP       = -3,   /* a HIP runtime call failed (text in ofl_last_error) */
    OFL_E_NOMEM     = -4,
    OFL_E_NOPOINTS  = -5,   /* scatter: no valid source points (qhull "No points given" in the reference) */
    OFL_E_RCCL      = -6
};

/* element types of warp targets (what cv2.remap accepts for INTER_LINEAR) */
enum { OFL_U8 = 0, OFL_I16 = 1, OFL_U16 = 2, OFL_F32 = 3, OFL_F64 = 4 };

/* element types of flow fields that cross to or from another framework (K11) */
enum { OFL_EL_F16 = 0, OFL_EL_BF16 = 1, OFL_EL_F32 = 2, OFL_EL_F64 = 3 };

/* sample-position quantisation of the bilinear gather */
enum {
    OFL_QUANT_OPENCV = 0,   /* cv2.remap semantics: coordinates snapped to 1/32 px (INTER_BITS = 5) */
    OFL_QUANT_EXACT  = 1    /* floor / fractional part in float32, no snapping (extension) */
};

/* arithmetic of the blend for 8-bit sources */
enum {
    OFL_ARITH_NATIVE    = 0,  /* u8: 15-bit fixed point, (acc + 2^14) >> 15; others float/double */
    OFL_ARITH_FLOAT_RNE = 1   /* u8 riding in an int16 concat (flow_class.py:615,644): float sum, round-half-even */
};

/* how "warped_mask == 1" (flow_class.py:668) evaluates for the dtype the reference's concat had */
enum {
    OFL_RULE_EQ1     = 0,   /* float concat: interpolated mask == 1 exactly */
    OFL_RULE_GE_HALF = 1,   /* uint8 concat (fixed point): interpolated >= 0.5 */
    OFL_RULE_GT_HALF = 2    /* int16 concat (round-half-even): interpolated > 0.5 */
};

/* flags OR-ed into the `valid_rule` argument of the scatter entries */
enum {
    OFL_SCATTER_ROUND  = 0x100,  /* out = rint(result): np.round of integer-typed targets, utils.py:256-257 */
    OFL_SCATTER_NEGATE = 0x200,  /* out = -result: the values are -vals (Flow.invert s->s = self.apply(-self), flow_class.py:746,
                                    without materialising -self; negation commutes exactly with the interpolation) */
    OFL_SCATTER_UNCERTIFIED = 0x400  /* the caller KNOWS the mesh cannot be certified (a certificate from ofl_scatter_certify_dev
                                    that says so, or a point mask with zeros): the entry skips its own certificate pass and
                                    read-back and takes the Delaunay path at once.  Never changes a result -- that path is the
                                    general one -- only saves the pass */
};

/* bits written by the zero-flow statistics (ofl_flow_stats_dev, and the fused compose kernel) */
enum {
    OFL_STAT_NONZERO_MASKED     = 1,  /* some vector component != 0 where mask   (Flow.is_zero(thresholded=False), flow_class.py:1244) */
    OFL_STAT_NONZERO_TH_MASKED  = 2,  /* some |component| >= 1e-3 where mask     (Flow.is_zero(thresholded=True)) */
    OFL_STAT_NONZERO            = 4,  /* some component != 0 anywhere            (is_zero_flow(thresholded=False), utils.py:527) */
    OFL_STAT_NONZERO_TH         = 8,  /* some |component| >= 1e-3 anywhere       (is_zero_flow(thresholded=True), utils.py:215) */
    OFL_STAT_NONFINITE          = 16, /* NaN / Inf present                       (validate_flow_array, utils.py:86) */
    OFL_STAT_MASK_HAS_ZERO      = 32  /* some mask byte is 0 (ofl_flow_stats only; lets callers pass NULL instead of an all-ones point mask) */
};

/* ------------------------------------------------------------------ runtime / device memory */
int         ofl_abi_version(void);
const char *ofl_last_error(void);
int         ofl_device_count(int *count);
int         ofl_init(int device);                 /* select device, create default stream */
int         ofl_device_name(char *buf, size_t buflen);
int         ofl_malloc(void **dptr, size_t bytes);
int         ofl_free(void *dptr);
int         ofl_memset(void *dptr, int value, size_t bytes, void *stream);
int         ofl_upload(void *dptr, const void *host, size_t bytes, void *stream);     /* async on stream; pinned staging not required */
int         ofl_download(void *host, const void *dptr, size_t bytes, void *stream);
int         ofl_download_async(void *host, const void *dptr, size_t bytes, void *stream);  /* no synchronisation: host must be pinned (ofl_host_alloc) for a true DMA */
int         ofl_copy_dev(void *dst, const void *src, size_t bytes, void *stream);
/* page-locked host memory: uploads / downloads from it are asynchronous DMA transfers that overlap with kernels
 * (on-disk formats are read straight into it: oflibnumpy_amd.device.load_sintel_device; utils.py:447-470) */
int         ofl_host_alloc(void **hptr, size_t bytes);
int         ofl_host_free(void *hptr);
int         ofl_stream_create(void **stream);
int         ofl_stream_destroy(void *stream);
int         ofl_stream_sync(void *stream);        /* NULL = default stream */
/* `stream` (NULL = the library's) waits, on the device, for everything queued so far on `producer_stream`, a stream of
 * another framework in this process (NULL = the legacy default stream, (void *)2 = the per-thread default stream): an
 * event without timing is recorded there, hipStreamWaitEvent enqueued here, the event destroyed.  Never blocks the host.
 * Needed because the library's streams are non-blocking: they do not order themselves after anyone else's work. */
int         ofl_stream_wait_external(void *producer_stream, void *stream);
/* hipPointerGetAttributes: *is_device = 1 and *device = its ordinal for device memory, 0 and -1 for anything else --
 * NULL, registered host memory, managed memory, and plain host memory the runtime has never seen (HIP's error for that is
 * cleared: it is an answer, not a failure).  Callers check every foreign pointer with it before a kernel is launched. */
int         ofl_pointer_info(const void *p, int *is_device, int *device);
int         ofl_device_sync(void);
int         ofl_event_create(void **event);
int         ofl_event_destroy(void *event);
int         ofl_event_record(void *event, void *stream);
int         ofl_event_sync(void *event);
int         ofl_event_elapsed_ms(void *start, void *stop, float *ms);
int         ofl_mem_info(size_t *free_bytes, size_t *total_bytes);
/* host helper of the dataset loaders (load_kitti, load_sintel_mask; utils.py:426-490): PNG row un-filtering, types 0-4;
 * raw = inflated IDAT stream (height rows of 1 filter byte + stride bytes), out [height][stride]; no device needed */
int         ofl_png_unfilter(const uint8_t *raw, size_t raw_bytes, int height, int stride, int bpp, uint8_t *out);

/* ------------------------------------------------------------------ non-finite flow vectors in K1, K2, K12 and K13
 * These four turn a flow vector into an address.  A vector with a non-finite component samples nothing: value 0, invalid --
 * every tap is outside the source, as for a vector that points beyond int32 (cvtss2si gives INT_MIN for all of them, which
 * is what cv2.remap and oracle/ofl_oracle.c see), and no address depends on it.  "Invalid" is mout / valid / covered /
 * consistent = 0.  "Value 0" is the sampled term: K2 and K13 go on to add it to the vector itself, which is not finite.  Under
 * OFL_QUANT_EXACT a NaN or Inf coordinate has no fraction either: the four weights are NaN and the sampled term, four zero taps
 * times NaN, is NaN as in the oracle.  NaN / Inf in the SAMPLED data travel through the blend unchanged, a tap of weight 0
 * included (0 * NaN); the host Flow refuses such fields, device-resident chains may carry them.
 * tests/test_gpu_nonfinite.py.
 */

/* ------------------------------------------------------------------ K2: fused mode-3 composition
 * Replaces Flow.combine_with(mode=3) numerics, flow_class.py:1412-1422 (+ Flow.apply :632-684,
 * apply_flow 't' utils.py:231-236, Flow.__add__ :332-334):
 *     out  = fb + B(fa; x + sign*fb)                 B = cv2.remap bilinear, 0 outside
 *     mout = mb & [B(ma; x + sign*fb) == 1]
 *   ref 't': fa/ma = self (f1), fb/mb = flow (f2), sign = -1
 *   ref 's': fa/ma = flow (f2), fb/mb = self (f1), sign = +1
 * batch fields are stored back to back ([batch][H][W][..]).  `stats` (device, uint32[batch][8] or
 * NULL) receives zero-flow flag WORDS computed from data the launch reads anyway (no extra traffic):
 * a word is set to 1 when its condition holds and is never cleared, so the caller zeroes the words
 * beforehand (plain idempotent stores -- no atomics on the hot path).
 *     stats[b][4 + k], k = 0..3 (the OFL_STAT_* bit index): EXACT predicates of fb/mb.
 *     stats[b][0], stats[b][1]: CERTIFICATES for fa/ma -- set when a gathered, masked vector of fa is
 *         non-zero / at or above the 1e-3 threshold, i.e. fa is certainly not (thresholded-)zero.  A clear
 *         word means "not observed": the caller confirms with ofl_flow_stats_dev before taking one of the
 *         reference's early exits (flow_class.py:1339-1354).  stats[b][2..3] are not written.
 *     In every word a NaN component counts as non-zero AND as at or above the threshold, as the reference's comparisons
 *     have it (`v != 0`, `!(v < th && v > -th)`, utils.py:310-315, 527-544); +-Inf does too, -0.0 is zero, a subnormal is
 *     non-zero.  The words equal the OFL_STAT_* bits of ofl_flow_stats_dev on every input, finite or not.
 * The host entry returns exact OFL_STAT_* bit masks: stats_host[2*b] for fa, stats_host[2*b+1] for fb.
 * out / mout must not alias the inputs.
 */
int ofl_compose3_dev(const float *fa, const uint8_t *ma, const float *fb, const uint8_t *mb,
                     int sign, int H, int W, int batch, float *out, uint8_t *mout,
                     uint32_t *stats, int quant, void *stream);
int ofl_compose3(const float *fa, const uint8_t *ma, const float *fb, const uint8_t *mb,
                 int sign, int H, int W, int batch, float *out, uint8_t *mout,
                 uint32_t *stats_host, int quant);

/* K2 with PACKED masks, for chains that stay on the device (SURVEY hard part H5: "masks as bytes, or bit-packed internally").
 * The three mask planes are one BIT per pixel -- bit (x & 31) of the uint32 word (x >> 5) of a row, rows padded to whole
 * words: [batch][H][(W + 31) / 32] words, allocated with ofl_mask_bits_bytes (16 bytes of slack after the last row) -- which
 * takes the masks from 3 of the 27 B/px of the contract to 0.4 (and from up to five times that, on a rotated sampling grid, in
 * partially used cache lines).  Same arithmetic, same flag words as ofl_compose3_dev (OFL_QUANT_OPENCV); the result equals
 * ofl_compose3_dev's bit for bit once unpacked.  W must be even.  ofl_mask_pack_dev / ofl_mask_unpack_dev convert between the
 * uint8 masks of every other entry (and of the host API) and the planes.
 */
int ofl_mask_bits_bytes(int H, int W, int batch, size_t *bytes);
int ofl_mask_pack_dev(const uint8_t *mask, int H, int W, int batch, uint32_t *bits, void *stream);
int ofl_mask_unpack_dev(const uint32_t *bits, int H, int W, int batch, uint8_t *mask, void *stream);
int ofl_compose3_bits_dev(const float *fa, const uint32_t *ma_bits, const float *fb, const uint32_t *mb_bits,
                          int sign, int H, int W, int batch, float *out, uint32_t *mout_bits,
                          uint32_t *stats, void *stream);

/* ------------------------------------------------------------------ K1: general bilinear gather
 * Replaces apply_flow(flow, target, 't') utils.py:231-236 and the mask handling around it in
 * Flow.apply flow_class.py:632-695, valid_target :1148-1150, valid_source :1179-1183:
 *     dst[y][x][c] = B(src[..][c]; (x, y) + sign * flow[y - pad_top][x - pad_left])
 *     valid[y][x]  = rule(B(smask; ...)) [& fmask[y - pad_top][x - pad_left], 0 outside the flow area]
 *   src/dst [H][W][C] of `dtype`; flow [fH][fW][2] located at (pad_top, pad_left) inside the
 *   H x W target with ZERO flow elsewhere (Flow.pad mode 'constant', flow_class.py:652-659);
 *   smask [H][W] or NULL (all ones); valid [H][W] or NULL; fmask [fH][fW] or NULL.
 *   C == 0 with src = dst = NULL computes `valid` only (warp of an all-ones / smask image).
 */
int ofl_gather_bilinear_dev(const void *src, int dtype, int C, int H, int W,
                            const float *flow, int fH, int fW, int pad_top, int pad_left, int sign,
                            const uint8_t *smask, const uint8_t *fmask,
                            void *dst, uint8_t *valid,
                            int quant, int arith, int rule, void *stream);
/* K1 over a BATCH of fields in one launch (Flow.apply for a stack of independent warps: BASELINE config 2-sized jobs are one
 * generation of waves per launch when launched alone, utils.py:231-236 / flow_class.py:632-695 per field).  Field b of the
 * batch reads flow [b][fH][fW][2], fmask [b][fH][fW] (or NULL), writes dst [b][H][W][C] and valid [b][H][W] (or NULL);
 * src is [b][H][W][C] -- or ONE image [H][W][C] warped by every flow when src_shared != 0 -- and smask likewise
 * ([b][H][W], one shared [H][W] when smask_shared != 0, or NULL).  Everything else as ofl_gather_bilinear_dev, whose results
 * the fields equal bit for bit.  batch in [1, 65535].
 */
int ofl_gather_bilinear_batch_dev(const void *src, int src_shared, int dtype, int C, int H, int W, int batch,
                                  const float *flow, int fH, int fW, int pad_top, int pad_left, int sign,
                                  const uint8_t *smask, int smask_shared, const uint8_t *fmask,
                                  void *dst, uint8_t *valid, int quant, int arith, int rule, void *stream);

/* One row band of the same result, for a field split over several GPUs: the source
 * image (and smask) are replicated, each rank holds rows [row0, row0 + rows) of the flow / its mask and
 * produces the same rows of dst / valid:
 *     dst_rows[y][x][c] = B(src[..][c]; (x, row0 + y) + sign * flow_rows[y][x]),  0 <= y < rows
 * flow_rows [rows][W][2], fmask_rows [rows][W] or NULL, dst_rows [rows][W][C], valid_rows [rows][W] or NULL.
 * Bands are disjoint, so there is no exchange step after the launch.
 */
int ofl_gather_rows_dev(const void *src, int dtype, int C, int H, int W, int row0, int rows,
                        const float *flow_rows, int sign, const uint8_t *smask, const uint8_t *fmask_rows,
                        void *dst_rows, uint8_t *valid_rows, int quant, int arith, int rule, void *stream);
int ofl_gather_bilinear(const void *src, int dtype, int C, int H, int W,
                        const float *flow, int fH, int fW, int pad_top, int pad_left, int sign,
                        const uint8_t *smask, const uint8_t *fmask,
                        void *dst, uint8_t *valid,
                        int quant, int arith, int rule);

/* ------------------------------------------------------------------ K4: zero-flow / finite statistics
 * Replaces is_zero_flow utils.py:527-544, threshold_vectors :298-316, Flow.is_zero
 * flow_class.py:1230-1245 and the finite check of validate_flow_array utils.py:86.
 * stats: one uint32 (device for _dev, host otherwise), OR of OFL_STAT_* bits; zeroed by the callee.
 */
int ofl_flow_stats_dev(const float *flow, const uint8_t *mask, size_t n_px, float threshold,
                       uint32_t *stats, void *stream);
int ofl_flow_stats(const float *flow, const uint8_t *mask, size_t n_px, float threshold,
                   uint32_t *stats_host);

/* ------------------------------------------------------------------ K5: element-wise epilogues
 * Flow.__add__/__sub__/__neg__ flow_class.py:310-375, 479-489:  out = a + alpha*b, mout = ma & mb.
 * b/mb may be NULL (then out = alpha * a, mout = ma: negation / scaling).
 */
int ofl_axpy_dev(const float *a, const uint8_t *ma, const float *b, const uint8_t *mb, float alpha,
                 size_t n_px, float *out, uint8_t *mout, void *stream);

/* ------------------------------------------------------------------ K3: scattered -> regular grid
 * Replaces apply_flow(flow, target, 's', mask) utils.py:237-258 (scipy.interpolate.griddata 'linear',
 * NaN -> 0) and the inline griddata of mode 2 / ref 't' flow_class.py:1398-1410.
 * Source point i sits at (x, y) + sign*flow[i] -- evaluated in float64 (point_precision 0, utils.py:242)
 * or rounded to float32 first (point_precision 1, flow_class.py:1398-1400) -- and carries
 * vals[i][0..C) (float32) plus, optionally, a mask value vmask[i]; points with pmask[i] == 0 are
 * dropped (pmask NULL = keep all, utils.py:249-251), and so are points whose position is not finite (the reference's Flow
 * refuses NaN / Inf vectors before it gets here).  The result is linear on the Delaunay triangulation of the kept
 * points (what griddata builds with Qhull):
 *     out[H][W][C]  piecewise-linear interpolation (float64 barycentric, stored as float32),
 *                   0 where no triangle covers the node;
 *     valid[H][W]   valid_rule 0: float32(interpolated vmask) == 1   (flow_class.py:668)
 *                   valid_rule 1: interpolated vmask > 0.99           (flow_class.py:1410)
 *                   valid_rule 2: rint(interpolated vmask) == 1 -- integer-typed targets, whose concatenated mask channel
 *                                 the reference rounds before the comparison (utils.py:256-257, flow_class.py:668)
 *                   valid_rule | OFL_SCATTER_ROUND: additionally out = float32(rint(float64 result)), the
 *                   np.round the reference applies to integer-typed targets (utils.py:256-257)
 *                   (vmask NULL = all ones, i.e. valid == "covered by a triangle").
 * query == NULL evaluates at the regular grid nodes; otherwise query [H][W][2] holds absolute (x, y)
 * positions (mode 2 't').  C may be 0 (validity only).  `workspace` (device) must hold
 * ofl_scatter_workspace_bytes() bytes.  info_host (host uint64[3] or NULL): [0] kept points (exact duplicates of a
 * site included, although only the smallest index of a location is a site of the triangulation); on the Delaunay path
 * [1] points whose star neither the mesh-fan pass nor the per-thread ring search could finish and [2] those of them left
 * for the workgroup pass (hull points, fan apexes of border pockets); 0 / 0 on the certified path.
 * OFL_E_NOPOINTS when no point is kept (qhull's "No points given") -- on the Delaunay path this and the capacity errors are
 * known only after the fact and reported to callers that pass info_host (one read-back at the end of the call); with
 * info_host == NULL that path only enqueues work and a field without kept points gives an all-invalid result.
 * Grid nodes take one of two paths: a field whose cell-wise mesh is certified to BE the Delaunay triangulation
 * (ofl_scatter_certify_dev) is resolved by one kernel; every other field -- folds, dropped points, curved borders,
 * sheared cells -- gets a real Delaunay triangulation of the kept points on the GPU.
 * valid_rule | OFL_SCATTER_UNCERTIFIED skips the entry's own certificate pass (and its read-back) for callers that know
 * the answer is "not certified"; the result is the same either way.
 * A certificate says that the mesh is the triangulation, not that the one-kernel path finds every node's triangle in it
 * (a certified field may squeeze a third of the image into a sliver): that kernel counts the nodes it could not locate,
 * the entry -- which has synchronised for the certificate anyway -- reads the count back and, if it is not zero, computes
 * the call on the Delaunay path instead.  The results are SciPy's either way.
 * Degenerate point sets: exact duplicates are ONE site (Qhull's Qc; a flow may collapse a whole image block onto one pixel:
 * buckets of thousands of coincident points are reduced through a hash table of positions).  What remains degenerate is
 * refused like Qhull refuses a flat initial simplex (the reference raises QhullError): all points on one spot or one
 * axis-parallel line, more than 65 536 distinct sites crowded into buckets of more than 4 096, more than 2^20 unfinished
 * or 2^18 unbounded cells (bulk collinearity) -- OFL_E_INVALID for callers that pass info_host, an all-zero / all-invalid
 * result for everybody (also after any capacity error: never a partial warp).
 */
int ofl_scatter_linear_dev(const float *flow, int sign, int point_precision, const uint8_t *pmask,
                           const float *vals, int C, const uint8_t *vmask, int H, int W,
                           const float *query, float *out, uint8_t *valid, int valid_rule,
                           void *workspace, size_t workspace_bytes, uint64_t *info_host, void *stream);
/* The same for float64 values at the grid nodes (no query positions): griddata interpolates in float64 and
 * apply_flow returns result.astype(target.dtype) (utils.py:253-258), so a float64 image keeps its precision.
 */
int ofl_scatter_linear_f64_dev(const float *flow, int sign, int point_precision, const uint8_t *pmask,
                               const double *vals, int C, const uint8_t *vmask, int H, int W,
                               double *out, uint8_t *valid, int valid_rule,
                               void *workspace, size_t workspace_bytes, uint64_t *info_host, void *stream);

/* One row band of the grid result (SURVEY 8e, config 5 as loaded, ref 's'): every rank holds the full inputs
 * (flow, masks, values are replicated), rasterises only the triangles that reach rows
 * [row0 - 16, row0 + rows + 16) and resolves rows [row0, row0 + rows): out_rows [rows][W][C],
 * valid_rows [rows][W].  The concatenation of the bands equals ofl_scatter_linear_dev bit for bit; bands are
 * disjoint, nothing is exchanged afterwards.  Same workspace size as the full call.
 */
int ofl_scatter_rows_dev(const float *flow, int sign, int point_precision, const uint8_t *pmask,
                         const float *vals, int C, const uint8_t *vmask, int H, int W, int row0, int rows,
                         float *out_rows, uint8_t *valid_rows, int valid_rule,
                         void *workspace, size_t workspace_bytes, uint64_t *info_host, void *stream);
int ofl_scatter_workspace_bytes(int H, int W, int C, size_t *bytes);

/* The same band with the STAR passes sharded too (SURVEY 8e, config 5 'ref s' -- a field the certificate refuses, whose
 * Delaunay stars are most of the time): two calls per rank around ONE exchange.
 *   1. ofl_scatter_slab_stars_dev: bins all sites (replicated inputs, as above), builds the stars of the sites within a
 *      margin of the band's rows only, and writes the sites it could not finish -- rims of holes, hull sites: those of
 *      the rank's own rows, the first / last band open-ended -- to `list` (device memory, list_bytes a multiple of 16):
 *      uint32 { entries, error bits, 0, 0 } followed by one 64-byte record per site.  64 bytes per expected site; a
 *      list that overflows is reported by step 2 on every rank (OFL_E_INVALID, err flag 32) -- retry with a larger one
 *      or fall back to ofl_scatter_rows_dev.
 *   2. all-gather the lists (ofl_comm_allgather: `list_bytes` per rank, in rank order or any other).
 *   3. ofl_scatter_slab_finish_dev with the gathered buffer (`n_lists` lists of `list_bytes` each, this rank's among
 *      them) and THE SAME workspace, untouched since step 1 (checked: step 1 stamps its band into the workspace, a
 *      workspace without that stamp -- no step 1, another band's, any other scatter call in between, a second step 2 --
 *      is refused with OFL_E_INVALID before any kernel runs): every rank finishes all unfinished stars (they can reach
 *      any band), rasterises and resolves its rows.  out_rows / valid_rows / valid_rule / info_host as above; the call
 *      synchronises (it reads the error bits back: an error on one rank blanks every band).
 * The concatenation of the bands equals ofl_scatter_linear_dev with OFL_SCATTER_UNCERTIFIED bit for bit.  A field whose
 * mesh certifies needs none of this: ofl_scatter_certified_dev shards by rows without any exchange.
 */
int ofl_scatter_slab_stars_dev(const float *flow, int sign, int point_precision, const uint8_t *pmask, int H, int W,
                               int row0, int rows, uint32_t *list, size_t list_bytes,
                               void *workspace, size_t workspace_bytes, void *stream);
int ofl_scatter_slab_finish_dev(const float *flow, int sign, int point_precision, const float *vals, int C,
                                const uint8_t *vmask, int H, int W, int row0, int rows,
                                const uint32_t *lists, size_t list_bytes, int n_lists,
                                float *out_rows, uint8_t *valid_rows, int valid_rule,
                                void *workspace, size_t workspace_bytes, uint64_t *info_host, void *stream);

/* Certificate of the warped grid as a triangulation (one pass over the flow, one 144-byte read-back; synchronises).
 * SciPy's griddata (utils.py:253) triangulates the points with Qhull; the cell-wise mesh of the warped grid IS that
 * Delaunay triangulation when no triangle is folded, every interior edge passes the local Delaunay test, no point is
 * dropped and the mesh border is straight between the warped image corners (then the convex hull is the border's).
 * `certified` = 1 states exactly that; such a field takes ofl_scatter_certified_dev -- one kernel, no owner map, no
 * atomics, no synchronisation.  The scatter entries above certify internally on every call; callers that warp with
 * the same field repeatedly certify once and keep the record (it depends on flow, sign, point_precision, pmask only).
 */
typedef struct ofl_mesh_cert {
    uint32_t certified;        /* 1: cell-wise mesh == Delaunay triangulation of the warped points (up to co-circular cells) */
    uint32_t folded_cells;     /* cells whose two triangles are not both positively oriented (counted exactly up to ~65 000, a lower bound beyond) */
    uint32_t bad_edges;        /* interior mesh edges failing the local Delaunay (in-circle) test beyond rounding (likewise) */
    uint32_t dropped;          /* 1: pmask drops points */
    double   border_dev;       /* px: largest distance of a border point from the straight side between its corners */
    double   corner[4][2];     /* warped image corners (x, y): (0,0), (W-1,0), (W-1,H-1), (0,H-1) */
    const uint32_t *diag_bits; /* the diag_bits buffer given to ofl_scatter_certify_dev (device memory the CALLER owns and keeps
                                  alive as long as the certificate is used), or NULL */
} ofl_mesh_cert;
/* diag_bits (device, ofl_scatter_diag_bytes(H, W) bytes, or NULL): receives the Delaunay diagonal of every grid cell, one bit
 * per cell, rows padded to 32-bit words.  ofl_scatter_certified_dev then reads a bit where it would otherwise evaluate the
 * cell's float64 in-circle determinant for every node -- same predicate, same numbers, same results, fewer instructions. */
int ofl_scatter_diag_bytes(int H, int W, size_t *bytes);
int ofl_scatter_certify_dev(const float *flow, int sign, int point_precision, const uint8_t *pmask, int H, int W,
                            void *workspace, size_t workspace_bytes, ofl_mesh_cert *cert_host, uint32_t *diag_bits, void *stream);
/* Rows [row0, row0 + rows) of the grid result for a CERTIFIED field (cert->certified must be 1, no point mask):
 * out_rows [rows][W][C], valid_rows [rows][W] as in ofl_scatter_linear_dev; asynchronous.  fail_count_dev (device
 * uint32, may be NULL; the caller zeroes it) counts nodes well inside the hull for which the kernel found no triangle
 * (written as 0 / invalid).  It is 0 for every affine field; a caller that keeps a certificate should check it once per
 * (field, sign) -- which nodes are found depends on nothing else -- and send a field that loses nodes through
 * ofl_scatter_linear_dev with OFL_SCATTER_UNCERTIFIED (the Python layer does exactly that). */
int ofl_scatter_certified_dev(const float *flow, int sign, int point_precision, const float *vals, int C,
                              const uint8_t *vmask, int H, int W, int row0, int rows, float *out_rows,
                              uint8_t *valid_rows, int valid_rule, const ofl_mesh_cert *cert,
                              uint32_t *fail_count_dev, void *stream);
int ofl_scatter_linear(const float *flow, int sign, int point_precision, const uint8_t *pmask,
                       const float *vals, int C, const uint8_t *vmask, int H, int W,
                       const float *query, float *out, uint8_t *valid, int valid_rule);

/* ------------------------------------------------------------------ sparse point tracking (next tier)
 * track_pts, utils.py:547-622:
 *   ofl_sample_points_dev   'ref s' default: bilinear_interpolation(flow[..., ::-1], pts) utils.py:161-196, float64,
 *                           pts_rc / out_rc are [n][2] in (row, col) order; points must lie inside the field
 *   ofl_scatter_query_dev   'ref t' (utils.py:610-615) and s_exact_mode (:599-603): griddata(points, values, pts):
 *                           same triangulation as ofl_scatter_linear_dev, evaluated at n_query float64 points
 *                           query_xy [n][2] = (x, y); out float64 [n][C]; found[i] = 0 where griddata gives NaN.
 *                           Synchronises: the point counts and error flags of the triangulation are read back inside, so
 *                           "no point kept" (OFL_E_NOPOINTS) and a refused / overflowing point set (OFL_E_INVALID) are
 *                           ERRORS here, never a list of found = 0 that looks like "outside the hull".
 */
int ofl_sample_points_dev(const float *flow, int H, int W, const double *pts_rc, size_t n, double *out_rc, void *stream);
int ofl_scatter_query_dev(const float *flow, int sign, int point_precision, const uint8_t *pmask,
                          const float *vals, int C, int H, int W,
                          const double *query_xy, size_t n_query, double *out, uint8_t *found,
                          void *workspace, size_t workspace_bytes, void *stream);

/* Tracking with RESIDENT points (K10, csrc/ofl_track.hip): the NumPy halves of track_pts (utils.py:547-622) and Flow.track
 * (flow_class.py:755-795) on the device, so that points, like fields, stay in HBM between steps.  All four entries are
 * asynchronous on `stream` (ofl_scatter_query_dev, which the query paths call in between, synchronises as before).
 * Common conventions:
 *   points    [n][2] in (row, col) order, 16-byte aligned: float64, or int32 / int64 where a dtype code is taken;
 *   stats     device uint32 per field, the OFL_STAT_* word ofl_flow_stats_dev writes, or NULL: a field whose
 *             OFL_STAT_NONZERO_TH bit is clear leaves the points where they are (is_zero_flow(flow, thresholded=True),
 *             utils.py:588) -- read on the device, no host round trip;
 *   valid     uint8 [H][W] per field (Flow.valid_source()) or NULL; with it, status [..] = valid[rint(row)][rint(col)] at the
 *             position BEFORE the step, rint = round-half-even like np.round (flow_class.py:791-793).  A rounded position
 *             that is no pixel of the field gives 0 (NumPy wraps negative indices and raises beyond the end).  status and
 *             valid are given together or not at all;
 *   int_out   != 0: the result is int32 after rint (np.round(warped).astype('i'), utils.py:619-620), else float64;
 *   n == 0    is no error: nothing is launched.
 *
 * ofl_track_bilinear_dev   ref 's', bilinear sampling (utils.py:593-606): p + sample(p), sample being exactly what
 *     ofl_sample_points_dev computes, then one float64 add.  flows: B fields back to back, [B][H][W][2]; stats [B];
 *     valid [B][H][W].
 *       chain == 0: every field is applied to the same n points: out [B][n][2], status [B][n].  A point outside
 *           0 <= row <= H-1, 0 <= col <= W-1 (NaN included) -- where the reference raises IndexError -- is left unchanged and
 *           counted in *outside_count (device uint32, zeroed by the caller, required).
 *       chain != 0: field k maps frame k to frame k+1 and each point runs through all B fields in one launch: out [n][2];
 *           a point whose position before step k is outside is frozen there, lost_at[i] = k (int32 [n], required; -1 = never
 *           lost); status [n] is the AND over the steps taken and 0 for a lost point; path (or NULL) float64 [B+1][n][2]
 *           receives every intermediate position, path[0] being the input.
 * ofl_track_pixels_dev     ref 's', integer points (utils.py:590-591): (double)p + (double)flow[row, col, ::-1].  pts_dtype
 *     OFL_TRACK_I32 or OFL_TRACK_I64.  An index outside [0, H) x [0, W) is counted in *outside_count and left unchanged
 *     (NumPy's wrap-around of negative indices is not reproduced).
 * ofl_track_query_points_dev   points of dtype pts_dtype (OFL_TRACK_*) -> query_xy float64 [n][2] = (x, y), the layout
 *     ofl_scatter_query_dev takes (pts[:, ::-1].astype(float64), utils.py:603 / :614).
 * ofl_track_query_epilogue_dev the tail of ref 't' and s_exact_mode (utils.py:603-620): query_xy / vals_uv (float64 [n][2], C = 2)
 *     / found are the input and the results of ofl_scatter_query_dev; the values are swapped back to (row, col) and added.
 *     One field: stats one word, valid [H][W].  Outputs, each optional (at least one is required): out_rc float64
 *     [n][2], out_int int32 [n][2] after rint, next_query_xy float64 [n][2] -- the result in (x, y) order, the next step's query.
 *       step < 0: one call of track_pts -- a point that was not found becomes (0, 0) (utils.py:616-618).
 *       step >= 0: step `step` of a sequence -- such a point is LOST: frozen where it is, lost_at[i] = step (int32 [n],
 *           required; read when step > 0, so step 0 initialises it); a point lost earlier stays frozen; status is ANDed with
 *           the previous steps' (read when step > 0) and 0 for lost points.
 */
enum {
    OFL_TRACK_F64 = 0,
    OFL_TRACK_I32 = 1,
    OFL_TRACK_I64 = 2
};
int ofl_track_bilinear_dev(const float *flows, int B, int H, int W, int chain, const double *pts_rc, size_t n,
                           const uint32_t *stats, const uint8_t *valid, int int_out, void *out, uint8_t *status,
                           uint32_t *outside_count, int32_t *lost_at, double *path, void *stream);
int ofl_track_pixels_dev(const float *flow, int H, int W, const void *pts_rc, int pts_dtype, size_t n,
                         const uint32_t *stats, const uint8_t *valid, int int_out, void *out, uint8_t *status,
                         uint32_t *outside_count, void *stream);
int ofl_track_query_points_dev(const void *pts_rc, int pts_dtype, size_t n, double *query_xy, void *stream);
int ofl_track_query_epilogue_dev(const double *query_xy, const double *vals_uv, const uint8_t *found, size_t n, int H, int W,
                                 const uint32_t *stats, const uint8_t *valid, int step, double *out_rc, int32_t *out_int,
                                 double *next_query_xy, uint8_t *status, int32_t *lost_at, void *stream);

/* small device helpers of the flow algebra:
 *   ofl_mask_and_dev     out = a & b                      (flow_class.py:643)
 *   ofl_grid_offset_dev  out[y][x] = float32((x, y) + sign * vecs[y][x])   (flow_class.py:1398-1406)
 */
int ofl_mask_and_dev(const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n, void *stream);
/*   ofl_convert_dev      element-wise dtype conversion on the device, n elements: any OFL_* dtype -> OFL_F32 (the
 *                        values the scatter kernel interpolates, utils.py:253) and OFL_F32 -> any dtype with a plain
 *                        C cast (result.astype(target.dtype), utils.py:258; integer destinations expect integral,
 *                        in-range values -- the scatter entries with OFL_SCATTER_ROUND produce them)
 */
int ofl_convert_dev(const void *src, int src_dtype, void *dst, int dst_dtype, size_t n, void *stream);
/*   ofl_flow_extent_dev  extent (device float32[4]) = { min y, max y, min x, max x } of the positions
 *                        float32((x, y) + sign * threshold_vectors(vecs)[y][x]) over the masked pixels
 *                        (Flow.get_padding, flow_class.py:1214-1226: sign -1 for ref 't', +1 for 's');
 *                        { +inf, -inf, +inf, -inf } when no pixel is masked
 */
int ofl_flow_extent_dev(const float *vecs, const uint8_t *mask, int H, int W, int sign, float threshold,
                        float *extent, void *stream);
int ofl_grid_offset_dev(const float *vecs, int sign, int H, int W, float *out, void *stream);

/* ------------------------------------------------------------------ K4: bilinear resize of a flow field
 * Replaces resize_flow (src/oflibnumpy/utils.py:493-525: cv2.resize(flow, None, fx, fy), INTER_LINEAR, then
 * vecs[..., 0] *= fx, vecs[..., 1] *= fy) and the mask half of Flow.resize (flow_class.py:501-506:
 * np.round(cv2.resize(mask.astype('f'), ..))).  The caller supplies the output size Ho = cvRound(H * fy),
 * Wo = cvRound(W * fx), the inverse scales scale_y = 1 / fy, scale_x = 1 / fx (doubles, as OpenCV derives
 * them) and the float32 channel factors mul_u = float32(fx), mul_v = float32(fy).
 * vecs float32[H][W][2] -> out float32[Ho][Wo][2];  mask uint8[H][W] -> mout uint8[Ho][Wo] (both or neither).
 */
int ofl_resize_flow(const float *vecs, const uint8_t *mask, int H, int W, int Ho, int Wo,
                    double scale_y, double scale_x, float mul_u, float mul_v, float *out, uint8_t *mout);
int ofl_resize_flow_dev(const float *vecs, const uint8_t *mask, int H, int W, int Ho, int Wo,
                        double scale_y, double scale_x, float mul_u, float mul_v,
                        float *out, uint8_t *mout, void *stream);

/* ------------------------------------------------------------------ K7: flow visualisation
 * Replaces Flow.visualise (flow_class.py:869-951) and visualise_flow (flow_operations.py:274-284): the field as an
 * HSV / RGB / BGR image, optionally with invalid areas dimmed (V = 180) and the mask border drawn black.  Per pixel:
 * components with -threshold < c < threshold become 0 (threshold_vectors); magnitude sqrt(u*u + v*v) and angle
 * (OpenCV 4.x fastAtan2, degrees) in float32; H = mod(angle, 360) / 2, S = clip(float32(mag * 255) / range, 0, 255),
 * V = 255; a border pixel (mask true, on the image frame or with a mask-false 4-neighbour) gets H = S = V = 0.
 * hsv bytes are rint(H, S, V); rgb / bgr bytes come from the reference's float64 colour-wheel arithmetic.
 * Layouts: flow float32 [batch][H][W][2], mask uint8 [batch][H][W] (0/1), out uint8 [batch][H][W][3].
 *
 *   ofl_visualise_range_dev  the default scale of every field of the batch, range_out float32[batch] (device):
 *                            np.percentile(mag, 99) if it is > 0, else max(mag) if that is > 0, else 1
 *                            (flow_class.py:910-916).  The caller passes the ranks lo <= hi < H * W of the two
 *                            order statistics NumPy interpolates between and its float32 weight gamma (they depend on
 *                            H * W only: numpy/lib/_function_base_impl.py, _quantile / _lerp); the kernels find both
 *                            values exactly (a radix select over the magnitude bits) and apply _lerp in float32.
 *                            workspace: ofl_visualise_workspace_bytes(H, W, batch) bytes of device memory, no
 *                            initialisation needed.  flow 8-byte aligned.  Nothing is synchronised.
 *   ofl_visualise_dev        the image.  range_dev: float32[batch] on the device (from ofl_visualise_range_dev), or
 *                            NULL -- then range_const (> 0, +inf allowed) serves every field.  mask may be NULL (all
 *                            valid).  flow 8-byte, out 4-byte aligned, mask at any address: vectors on the 16-byte and a
 *                            mask on the 4-byte grid are read four pixels a load pair, anything else pixel by pixel --
 *                            the same pixels per thread, the same bytes out.
 * A field holding NaN / Inf gives an unspecified image but never reads or writes out of bounds.
 */
enum { OFL_VIS_HSV = 0, OFL_VIS_RGB = 1, OFL_VIS_BGR = 2 };
enum {
    OFL_VIS_SHOW_MASK    = 1,   /* show_mask: V = 180 where the mask is false */
    OFL_VIS_MASK_BORDERS = 2    /* show_mask_borders: the border of the mask in black */
};
int ofl_visualise_workspace_bytes(int H, int W, int batch, size_t *bytes);
int ofl_visualise_range_dev(const float *flow, int H, int W, int batch, float threshold, size_t lo, size_t hi,
                            float gamma, void *workspace, size_t workspace_bytes, float *range_out, void *stream);
int ofl_visualise_dev(const float *flow, const uint8_t *mask, int H, int W, int batch, float threshold,
                      const float *range_dev, float range_const, int mode, int flags, uint8_t *out, void *stream);

/* ------------------------------------------------------------------ K8: fitting a matrix to a flow field
 * The O(H * W) passes of Flow.matrix (flow_class.py:797-867) and get_flow_matrix (flow_operations.py:251-271): affine
 * (dof 4 / 6) and homography (dof 8) fitting by least squares, RANSAC or least median.  The tiny linear algebra stays with
 * the caller (oflibnumpy_amd/matrix_fit.py); parity with OpenCV's estimators is not pinned.
 *
 * Correspondences are rebuilt per pixel (col, row) with vector v, in float64 from the float32 vector (exact):
 *     sign +1 (ref 's'): src = (col, row), dst = src + v        sign -1 (ref 't'): dst = (col, row), src = dst - v
 * A pixel whose mask byte is 0 is skipped (mask NULL: none is); a non-finite vector is skipped and counted.
 *
 * RESIDUAL of a model M (9 doubles, row-major 3x3) at a correspondence (x, y) -> (X, Y), every operation a float64
 * operation rounded once, in exactly this order, nothing contracted:
 *     w  = (M[6]*x + M[7]*y) + M[8]
 *     px = ((M[0]*x + M[1]*y) + M[2]) / w          py = ((M[3]*x + M[4]*y) + M[5]) / w
 *     dx = px - X                                   dy = py - Y
 *     r  = float32(dx*dx + dy*dy)                   NaN or Inf (w == 0, overflow) -> +Inf
 * The float32 r is the quantity that is thresholded (r <= thr), counted and ranked; r >= 0, so its bits sort as uint32.
 * GATE: the sum entries take gate_model (host, 9 doubles, or NULL = no gate) and gate_thr; only correspondences with
 * residual(gate_model) <= gate_thr contribute -- "refit on the inliers" is the same kernel as "fit on everything".
 * Models, origins and normalisations are HOST pointers (they travel as kernel arguments); flow, mask, workspace and
 * every output are DEVICE pointers.  flow 8-byte aligned, mask at any address; H * W < 2^31.  Nothing is synchronised.
 * Vectors on the 16-byte and a mask on the 4-byte grid are read 16 and 4 bytes a load, anything else 8 bytes and 1 byte a
 * load: the pixels of a thread and the order of every addition are the same, so the results do not depend on alignment.
 *
 * SUMS (device float64): one workgroup per 4096 px writes its partial sums to the workspace -- per thread its <= 19 terms in
 * pixel order, per wave a six-level butterfly, then ((w0 + w1) + w2) + w3 -- and one thread per sum adds the
 * ceil(H*W / 4096) partials in order.  No floating-point atomics, a grid that depends on H * W only: two calls on the
 * same input return the same bits.
 *   ofl_fit_moments_dev  sums[16]: with v = (x - ox, y - oy, X - ox, Y - oy, 1), origin = (ox, oy): the 15 products
 *                        v[i]*v[j], i <= j, row by row ((0,0), (0,1), .. (0,4), (1,1), .. (4,4) -- the last is the number
 *                        of correspondences), then [15] the number of non-finite vectors skipped.
 *   ofl_fit_dlt_dev      sums[47]: with norm = (cx, cy, s, cX, cY, S) and the normalised x~ = (x - cx)*s, y~ = (y - cy)*s,
 *                        X~ = (X - cX)*S, Y~ = (Y - cY)*S, the rows a1 = (x~, y~, 1, 0, 0, 0, -(X~*x~), -(X~*y~), -X~),
 *                        a2 = (0, 0, 0, x~, y~, 1, -(Y~*x~), -(Y~*y~), -Y~): the 45 terms a1[i]*a1[j] + a2[i]*a2[j],
 *                        i <= j, row by row (L^T L of the direct linear transform), [45] n, [46] non-finite.
 *   ofl_fit_gn_dev       sums[47] at the homography h = model (normalised coordinates, h[8] held fixed): with
 *                        w = (h[6]*x~ + h[7]*y~) + h[8], px = ((h[0]*x~ + h[1]*y~) + h[2]) / w, py likewise, rx = px - X~,
 *                        ry = py - Y~, j1 = (x~/w, y~/w, 1/w, 0, 0, 0, -(x~*px)/w, -(y~*px)/w),
 *                        j2 = (0, 0, 0, x~/w, y~/w, 1/w, -(x~*py)/w, -(y~*py)/w): [0..36) j1[i]*j1[j] + j2[i]*j2[j], i <= j
 *                        (J^T J), [36..44) j1[i]*rx + j2[i]*ry (J^T r), [44] rx*rx + ry*ry, [45] n, [46] non-finite.
 * COUNTS AND RANKS (device uint32, exact):
 *   ofl_fit_score_dev    counts[K]: correspondences with residual(models[k]) <= thr, K in [1, 32], one read of the field.
 *   ofl_fit_median_dev   out[2*k], out[2*k + 1]: the bits of the residuals of models[k] at ranks rank_lo <= rank_hi (0-based,
 *                        ascending) among the valid correspondences -- the two values a median interpolates between
 *                        ((n - 1) / 2 and n / 2 for n correspondences).  Any K >= 1; three models share one pass.
 * SAMPLING (a pixel is valid when its mask byte is not 0 and its vector is finite):
 *   ofl_fit_index_dev    builds the rank index of the valid pixels in the workspace (kept until the next call on it; the
 *                        other entries leave it alone).
 *   ofl_fit_pick_dev     idx[i] = pixel index (row * W + col) of the ranks[i]-th valid pixel in row-major order,
 *                        0xffffffff when there are fewer.  ranks, idx: device uint32[count].
 *   ofl_fit_gather_dev   out[i] = { idx[i], bits of u, bits of v, mask byte (1 without a mask) } as uint32[count][4], 16-byte
 *                        aligned; { idx[i], 0, 0, 0 } for an index outside the field.
 * workspace: ofl_fit_workspace_bytes(H, W) bytes of device memory, no initialisation needed.
 * A field holding NaN / Inf gives an unspecified matrix but never reads or writes out of bounds.
 */
int ofl_fit_workspace_bytes(int H, int W, size_t *bytes);
int ofl_fit_moments_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *origin,
                        const double *gate_model, float gate_thr, void *workspace, size_t workspace_bytes,
                        double *sums, void *stream);
int ofl_fit_dlt_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *norm,
                    const double *gate_model, float gate_thr, void *workspace, size_t workspace_bytes,
                    double *sums, void *stream);
int ofl_fit_gn_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *norm, const double *model,
                   const double *gate_model, float gate_thr, void *workspace, size_t workspace_bytes,
                   double *sums, void *stream);
int ofl_fit_score_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *models, int K,
                      float thr, uint32_t *counts, void *stream);
int ofl_fit_median_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *models, int K,
                       size_t rank_lo, size_t rank_hi, void *workspace, size_t workspace_bytes, uint32_t *out, void *stream);
int ofl_fit_index_dev(const float *flow, const uint8_t *mask, int H, int W, void *workspace, size_t workspace_bytes, void *stream);
int ofl_fit_pick_dev(const float *flow, const uint8_t *mask, int H, int W, const void *workspace, size_t workspace_bytes,
                     const uint32_t *ranks, size_t count, uint32_t *idx, void *stream);
int ofl_fit_gather_dev(const float *flow, const uint8_t *mask, int H, int W, const uint32_t *idx, size_t count,
                       uint32_t *out, void *stream);

/* ------------------------------------------------------------------ K9: building, scaling, padding, cropping fields
 * The constructors and element-wise / shape operations of Flow that had no device form: Flow.from_matrix /
 * from_transforms (flow_class.py:173-234 over utils.flow_from_matrix, utils.py:91-111, and from_matrix :319-344),
 * Flow.__mul__ / __truediv__ (flow_class.py:377-443), Flow.pad (:508-526) and Flow.__getitem__ (:297-308).  Streaming
 * kernels; every entry only enqueues work.  Vector buffers that are written are 16-byte aligned, written masks 2-byte
 * aligned -- except ofl_scale_dev, whose source and result need 8 bytes only (below 16 it moves 8 bytes a load); outputs
 * must not alias inputs.
 *
 *   ofl_flow_from_matrix_dev  n fields out_vecs [n][H][W][2] from n row-major 3x3 float64 matrices in DEVICE memory
 *                             (mats_dev [n][9]), one launch; n in [1, 65535].  Per pixel (x, y), every operation a float64
 *                             operation rounded once, in exactly this order, nothing contracted:
 *                                 X = (m[0]*x + m[1]*y) + m[2]    Y = (m[3]*x + m[4]*y) + m[5]    Z = (m[6]*x + m[7]*y) + m[8]
 *                                 u = float32(X / Z - x)          v = float32(Y / Z - y)
 *                             and for sign -1 (u, v) = (-u, -v) after the cast (a zero becomes -0.0f).  This is
 *                             utils.flow_from_matrix bit for bit (np.matmul of the float64 matrix with the float32 column
 *                             (x, y, 1)); reference 't' passes pinv(matrix) and sign -1 (utils.py:343-344).  A matrix whose
 *                             last row is exactly (0, 0, 1) skips Z and the quotients: Z is exactly 1.
 *   ofl_scale_dev             out = vecs * (k0, k1) per channel, or vecs / (k0, k1) with divide != 0; n_px pixels.
 *                             wide == 0: float32 arithmetic with float32(k) -- NumPy's result for a Python scalar or a float32
 *                             operand; wide != 0: float32(float64(v) op k) -- a float64 or integer array operand.
 *                             Correctly rounded, never contracted.  The mask is not involved.
 *   ofl_pad_flow_dev          out [H + top + bottom][W + left + right]; mode 0 'constant' (zero vectors), 1 'edge' (source
 *                             index clamped), 2 'symmetric' (source index reflected with period 2n: i mod 2n, mirrored when
 *                             >= n -- np.pad for any pad width, pads larger than the field included).  out_mask is the mask
 *                             inside the original frame and 0 outside in every mode.
 *   ofl_crop_flow_dev         out [rows][cols]: out[r][c] = field[row0 + r * row_step][col0 + c * col_step], vectors and
 *                             mask; steps may be negative or larger than 1; every source index must lie inside the field
 *                             (the caller normalises a slice with slice.indices).
 */
int ofl_flow_from_matrix_dev(const double *mats_dev, int n, int sign, int H, int W, float *out_vecs, void *stream);
int ofl_scale_dev(const float *vecs, double k0, double k1, int divide, int wide, size_t n_px, float *out, void *stream);
int ofl_pad_flow_dev(const float *vecs, const uint8_t *mask, int H, int W, int top, int bottom, int left, int right,
                     int mode, float *out_vecs, uint8_t *out_mask, void *stream);
int ofl_crop_flow_dev(const float *vecs, const uint8_t *mask, int H, int W, int row0, int row_step, int rows,
                      int col0, int col_step, int cols, float *out_vecs, uint8_t *out_mask, void *stream);

/* ------------------------------------------------------------------ K11: fields and images of another framework
 * Conversions between the layouts and element types other frameworks keep in device memory and the library's own
 * ([H][W][2] float32 + uint8 mask, images [H][W][C]).  Strides are in ELEMENTS, >= 0 (0 = a broadcast dimension), 64-bit;
 * the caller guarantees that every address they reach is device memory of this device (ofl_pointer_info).  Streaming
 * kernels, every entry only enqueues work.  A lane owns 4 horizontally adjacent pixels of a row and accesses each
 * address as widely as its alignment allows -- decided per address, so any element-aligned view is correct.
 *
 *   ofl_import_flow_dev    n fields from `src` (OFL_EL_*) with strides (field, channel, row, column) into out_vecs
 *                          [n][H][W][2] float32 and out_mask [n][H][W] uint8.  f16 / bf16 -> float32 exactly, f64 ->
 *                          float32 to nearest even.  mask_src: 1-byte elements with strides (field, row, column), out =
 *                          (m != 0); NULL: all valid.  counters (device uint32[2], zeroed by the caller) or NULL:
 *                          [0] += vector components whose float32 value is not finite, [1] += mask bytes that are neither
 *                          0 nor 1.  out_vecs and out_mask may both be NULL: count only.  out_vecs 8-byte aligned.
 *   ofl_export_flow_dev    vecs [n][H][W][2] float32 into a contiguous dst of OFL_EL_F16 / BF16 / F32, [n][H][W][2] or, with
 *                          planar != 0, [n][2][H][W].  To nearest even, overflow to +-inf; bf16 on the bit pattern, every
 *                          NaN becomes 0x7fc0.
 *   ofl_permute_image_dev  to_hwc != 0: src [C][H][W] with strides (channel, row, column) -> dst contiguous [H][W][C];
 *                          to_hwc == 0: src contiguous [H][W][C] -> dst [C][H][W] with those strides.  Elements of 1, 2, 4
 *                          or 8 bytes move unchanged; C in [1, 6].
 */
int ofl_import_flow_dev(const void *src, int elem, int64_t s_field, int64_t s_chan, int64_t s_row, int64_t s_col,
                        int n, int H, int W, const uint8_t *mask_src, int64_t m_field, int64_t m_row, int64_t m_col,
                        float *out_vecs, uint8_t *out_mask, uint32_t *counters, void *stream);
int ofl_export_flow_dev(const float *vecs, int n, int H, int W, int elem, int planar, void *dst, void *stream);
int ofl_permute_image_dev(const void *src, void *dst, int elem_bytes, int C, int H, int W,
                          int64_t s_chan, int64_t s_row, int64_t s_col, int to_hwc, void *stream);

/* ------------------------------------------------------------------ K12: warping many-channel float tensors
 * Flow.apply with reference 't' (utils.py:231-236, flow_class.py:604-695, without padding) for the feature maps of a
 * network: N items of C channels, contiguous (N, C, H, W) or (N, H, W, C), of OFL_EL_F32, OFL_EL_F16 or OFL_EL_BF16
 * (OFL_EL_F64 and anything else: OFL_E_INVALID).  src and dst share one layout; N and C in [1, 65535], H and W as K1
 * allows; every element offset is 64-bit (N * C * H * W may exceed 2^31).  Asynchronous; a bad argument returns
 * OFL_E_INVALID before any launch.
 *
 *   ofl_gather_tensor_dev   dst[n, c, y, x] = B(src[n, c]; (x, y) + sign * flow[y, x]) for every channel from ONE set of
 *                           taps per pixel -- K1's coordinates, taps and blend, operation for operation; taps outside the
 *                           frame read 0.  16-bit elements are widened to float32 (exact), blended in float32 and rounded
 *                           once to the storage type, to nearest even with overflow to +-inf (ofl_export_flow_dev's
 *                           rounding); a float32 tensor equals ofl_gather_bilinear_dev channel for channel, bit for bit.
 *                           flow [H][W][2] and fmask [H][W] warp all N items when flow_shared != 0, else N fields and masks
 *                           lie back to back.  valid (NULL: skipped) [N][H][W] = fmask & [interpolated smask == 1]
 *                           (OFL_RULE_EQ1), one mask per item; smask [H][W] when smask_shared != 0, else [N][H][W], NULL: all
 *                           ones.  With a shared field and a shared (or no) smask every item's mask is the same: valid is
 *                           then ONE [H][W] mask.  valid needs fmask.
 *   ofl_tensor_import_dev   a strided view -- element strides (item, channel, row, column) >= 0, elements of 2 or 4 bytes
 *                           that move unchanged -- into a contiguous dst of `layout`.
 *   ofl_tensor_permute_dev  contiguous (N, C, H, W) -> (N, H, W, C) with to_nhwc != 0, else the way back; any C.
 *   ofl_tensor_halve_dev    the 2 x 2 mean of a tensor of either layout and of OFL_EL_F32 / F16 / BF16 -> dst of the same
 *                           layout and element with H >> 1 rows and W >> 1 columns: ((tl + tr) + (bl + br)) * 0.25f in
 *                           float32, rounded once to the element (K18's ofl_avgpool2_dev arithmetic); an odd last row or
 *                           column is dropped; H or W < 2 is refused; dst must not overlap src.  One level of the image
 *                           pyramid of estimate_flow (K24).
 */
enum { OFL_TENSOR_NCHW = 0, OFL_TENSOR_NHWC = 1 };
int ofl_gather_tensor_dev(const void *src, int elem, int layout, int N, int C, int H, int W,
                          const float *flow, int flow_shared, int sign,
                          const uint8_t *smask, int smask_shared, const uint8_t *fmask,
                          void *dst, uint8_t *valid, int quant, void *stream);
int ofl_tensor_import_dev(const void *src, int elem_bytes, int64_t s_item, int64_t s_chan, int64_t s_row, int64_t s_col,
                          int layout, int N, int C, int H, int W, void *dst, void *stream);
int ofl_tensor_permute_dev(const void *src, void *dst, int elem_bytes, int N, int C, int H, int W, int to_nhwc, void *stream);
int ofl_tensor_halve_dev(const void *src, int elem, int layout, int N, int C, int H, int W, void *dst, void *stream);

/* ------------------------------------------------------------------ K13: forward-backward consistency of two fields
 * The check between "two fields come out of a network" and "warp with them": sample the backward field b where the
 * forward field f points, add the two vectors, and call the pixel inconsistent (occluded) when the sum is larger than a
 * bound that grows with the two magnitudes.  f and b have one shape and ONE reference; sign = +1 for 's', -1 for 't' --
 * the pairing of ofl_compose3_dev with fb = f, fa = b.  Per pixel (x, y), every operation float32 and rounded once:
 *     tap        = the bilinear tap of (x, y) + sign * f[y][x]          (map_coord / make_tap, `quant` as in K1 / K2)
 *     bu, bv     = b's four taps blended (0 outside the frame);  am = bm's four taps blended as 0.0f / 1.0f
 *     covered    = fm & (am == 1.0f)                                    == ofl_compose3_dev's mout, bit for bit
 *     ru, rv     = f.u + bu, f.v + bv                                   == ofl_compose3_dev's out, bit for bit
 *     r2         = ru*ru + rv*rv
 *     s2         = (f.u*f.u + f.v*f.v) + (bu*bu + bv*bv)
 *     lim        = alpha*s2 + beta
 *     consistent = covered & (r2 <= lim)
 *     residual   = covered ? sqrtf(r2) : 0.0f                           (the correctly rounded square root)
 * This is not a function of the reference and the formula is its definition: there is NO zero-flow short cut in either
 * `quant` mode (under OFL_QUANT_EXACT a sub-threshold f therefore differs from f + f.apply(b); it equals K2 always).
 * batch pairs are stored back to back ([batch][H][W][..]), batch in [1, 65535], H and W in [1, 32766].  consistent is
 * required; covered and residual may be NULL (not written).  counts (device, uint32[batch][2] = {covered, consistent}
 * pixels per pair, or NULL) is ADDED to: the caller zeroes it; each workgroup reduces its pixels and issues at most one
 * atomic add per counter (integer adds: the result does not depend on their order), and with counts == NULL the launch
 * issues no atomics at all.  Outputs must not alias inputs.  f and b must be 8-byte aligned.
 * Bytes per pixel: reads 8 (f, streamed) + 8 (b, gathered) + 2 (masks); writes 1 (consistent) + 1 (covered) + 4 (residual)
 * -- 2 where ofl_compose3_dev writes 9, or 6 with the residual.
 * A bad argument -- a NULL f / fm / b / bm / consistent, sizes or batch out of range, sign not +-1, alpha or beta negative
 * or not finite, an unknown quant -- returns OFL_E_INVALID with a message before any launch.  The _dev entry is
 * asynchronous; the host entry uploads, launches once, downloads (counts_host: host uint32[batch][2] or NULL) and
 * synchronises.
 */
int ofl_consistency_dev(const float *f, const uint8_t *fm, const float *b, const uint8_t *bm, int sign,
                        int H, int W, int batch, float alpha, float beta,
                        uint8_t *consistent, uint8_t *covered, float *residual, uint32_t *counts,
                        int quant, void *stream);
int ofl_consistency(const float *f, const uint8_t *fm, const float *b, const uint8_t *bm, int sign,
                    int H, int W, int batch, float alpha, float beta,
                    uint8_t *consistent, uint8_t *covered, float *residual, uint32_t *counts_host, int quant);

/* ------------------------------------------------------------------ K14: an estimated field against a ground truth
 * How far `est` is from `gt`: end-point error, threshold and outlier counts, and the error by speed of the ground truth --
 * Sintel's EPE by speed bins (edges 10, 40) and KITTI's "Fl" rule (3 px and 5 %) with its validity mask are two settings
 * of it.  est and gt have one shape and one reference; the reference does not enter the arithmetic.  Per pixel, every
 * operation float32 and rounded once (sqrtf is the correctly rounded square root):
 *     du = est.u - gt.u;  dv = est.v - gt.v
 *     epe  = sqrtf(du*du + dv*dv)
 *     g    = sqrtf(gt.u*gt.u + gt.v*gt.v)
 *     eval = gt.mask & (est_mask given ? est.mask : 1)
 *     bad  = eval & !isfinite(epe)            NaN / Inf in either field, or an overflow of du*du + dv*dv: one rule
 *     ok   = eval &  isfinite(epe)
 *     over[k] = ok & (epe > thr[k])           k < 4, strict; an unused slot is +inf
 *     outlier = ok & (epe > out_abs) & (epe > out_rel * g)        a product: no division by 0 where gt = 0
 *     bin     = the number of edges[j] (j < 3, ascending, unused = +inf) with g >= edges[j]
 * (g = +inf, a ground truth whose square overflows, is >= every edge, the unused ones included: such a pixel is in bin 3.)
 * Per pair one record; the uint32 part comes first so that the doubles are 8-byte aligned; 96 bytes:
 */
struct ofl_flow_error {
    uint32_t n;               /* ok pixels: every count and sum below runs over these */
    uint32_t n_nonfinite;     /* bad pixels */
    uint32_t n_over[4];       /* epe > thr[k] */
    uint32_t n_outlier;
    uint32_t n_bin[4];
    uint32_t max_epe_bits;    /* the float32 bit pattern of the largest ok epe (non-negative floats sort as uint32), 0 if n = 0 */
    double   sum_epe;
    double   sum_epe2;        /* terms double(epe) * double(epe): exact */
    double   sum_bin_epe[4];
};
/* Optional per-pixel outputs, written when the pointer is not NULL: epe_map float32 [batch][H][W] = epe where ok, else 0;
 * outlier_map uint8 [batch][H][W] = the outlier bit.
 * A pure stream: 18 B/px read (two 8-byte vectors, two mask bytes; 17 without est_mask), nothing written per pixel without
 * a map, no LDS staging of data and no atomics.  A workgroup takes one chunk of 4096 consecutive pixels of one pair;
 * thread t of chunk c owns pixels c*4096 + s*1024 + 4*t + j (s, j < 4) on every load path, so the order of additions is a
 * function of H * W alone: the doubles of a record do not depend on alignment, on the load path or on batch.  A thread
 * adds its terms in pixel order, a wave reduces by a six-level xor butterfly, the four wave values are added in order, and a
 * finishing kernel (one workgroup of 256 threads per pair) gives thread t the chunk partials t, t + 256, ... in order, then
 * butterfly, then waves in order.  The longest chain of additions a term passes through is
 *     depth(H*W) = 16 + 6 + 3 + ceil(chunks / 256) + 6 + 3,        chunks = ceil(H*W / 4096)
 * so every float64 sum (its terms are >= 0) is within depth * 2^-53 * sum of the exact sum.  Counts and the maximum are
 * integer operations and exact.
 * Out of scope: the angular error (it needs atan2, which cannot be pinned bit for bit against NumPy here), and the median or
 * a percentile of the EPE (it would need a third copy of the radix select of K7 / K8).
 * thr, edges: HOST pointers, passed on as kernel arguments.  workspace: device memory of at least
 * ofl_flow_error_workspace_bytes(H, W, batch) bytes, 8-byte aligned; it needs no initialisation (the kernels write every
 * word they read).  est, gt 8-byte, epe_map 4-byte, records 8-byte aligned.  Outputs must not alias inputs.
 * A bad argument -- a NULL est / gt / gt_mask / thr / edges / workspace / records, H or W < 1, H*W >= 2^31, batch outside
 * [1, 65535], a NaN or negative threshold, bound or edge, edges not ascending, a short workspace -- returns OFL_E_INVALID
 * with a message before any launch.  The _dev entry is asynchronous; the host entry takes host pointers (est_mask,
 * epe_map, outlier_map optional), uploads, launches, downloads and synchronises.
 */
int ofl_flow_error_workspace_bytes(int H, int W, int batch, size_t *bytes);
int ofl_flow_error_dev(const float *est, const uint8_t *est_mask, const float *gt, const uint8_t *gt_mask,
                       int H, int W, int batch, const float thr[4], float out_abs, float out_rel, const float edges[3],
                       void *workspace, size_t workspace_bytes, struct ofl_flow_error *records,
                       float *epe_map, uint8_t *outlier_map, void *stream);
int ofl_flow_error(const float *est, const uint8_t *est_mask, const float *gt, const uint8_t *gt_mask,
                   int H, int W, int batch, const float thr[4], float out_abs, float out_rel, const float edges[3],
                   struct ofl_flow_error *records_host, float *epe_map, uint8_t *outlier_map);

/* ------------------------------------------------------------------ K15: masked-out vectors from the nearest valid pixel
 * The step after a consistency check, a sparse ground truth or a scatter with holes: every pixel takes the vector of the
 * nearest valid pixel.  Exact integer arithmetic; the reference of the field does not enter.  Per field:
 *     vecs   float32 [H][W][2]        mask  uint8 [H][W]        valid  uint8 [H][W] or NULL        max_d2  int, -1 = no limit
 *     source(q)  = (mask[q] & (valid ? valid[q] : 0xFF)) != 0
 *     d2(p, q)   = (x - qx)^2 + (y - qy)^2                      p = (x, y), q = (qx, qy); an exact integer, < 2^31
 *     near(p)    = the source that minimises d2(p, .); among equals the smaller qy, then the smaller qx -- the smallest
 *                  linear index qy * W + qx among the nearest.  A source is its own nearest.
 *     filled(p)  = a source exists and (max_d2 < 0 or d2(p, near(p)) <= max_d2)
 *     out_vecs[p] = the 8 bytes of vecs[near(p)] where filled, the 8 bytes of vecs[p] where not: copied, never recomputed
 *                   (NaN payloads and -0.0 survive)
 *     out_mask[p] = filled ? 1 : 0
 *     index[p]    = filled ? qy * W + qx of near(p) : -1              int32, optional
 *     d2[p]       = filled ? d2(p, near(p)) : 0xFFFFFFFF              uint32, optional
 * vecs and out_vecs may both be NULL -- the distance transform of a mask alone --, and then index or d2 is required; with
 * vectors, out_mask, index and d2 are each optional.  `batch` fields lie back to back, offsets are size_t.
 * Two launches.  The row pass (one workgroup per row; a ballot of 64 source bits per wave and step, the nearest set bit on
 * either side by clz / ffs, the carry across 64-pixel words by a scan in LDS) writes for every pixel the signed column offset
 * to the nearest source of its own row -- a tie goes to the smaller column -- as int16 into the workspace; offsets reach
 * +-32765, -32768 says "no source in this row, or none within max_d2".  The column pass (lanes along x) minimises
 * (y - y')^2 + off(x, y')^2 over the rows y' by scanning outward, y -+ 1, y -+ 2, ...: a row above wins a tie against
 * everything found so far, a row below wins only when strictly nearer, and the scan stops at the first k with
 * k^2 > min(best, max_d2).  Its cost grows with the distance to the nearest source; max_d2 bounds it.  No atomics.
 *     ofl_fill_workspace_bytes = batch * H * W * 2
 * workspace: device memory, 2-byte aligned, needs no initialisation.  vecs / out_vecs 8-byte, index / d2 4-byte aligned;
 * the masks may sit at any address.  Outputs must not alias inputs.
 * A bad argument -- a NULL mask, only one of vecs / out_vecs, nothing to write (without vectors neither index nor d2),
 * H or W outside [1, 32766], batch outside [1, 65535], max_d2 < -1, an output that is an input, a missing, short or
 * misaligned workspace -- returns OFL_E_INVALID with a message before any launch.  The _dev entry is asynchronous; the host
 * entry takes host pointers, uploads, launches, downloads and synchronises.
 */
int ofl_fill_workspace_bytes(int H, int W, int batch, size_t *bytes);
int ofl_fill_dev(const float *vecs, const uint8_t *mask, const uint8_t *valid, int H, int W, int batch, int max_d2,
                 void *workspace, size_t workspace_bytes, float *out_vecs, uint8_t *out_mask, int32_t *index, uint32_t *d2,
                 void *stream);
int ofl_fill(const float *vecs, const uint8_t *mask, const uint8_t *valid, int H, int W, int batch, int max_d2,
             float *out_vecs, uint8_t *out_mask, int32_t *index, uint32_t *d2);

/* ------------------------------------------------------------------ K16: mask-aware median filter of the vectors
 * The step after fill (its output is piecewise constant with Voronoi seams), after a consistency check (outliers take the
 * median of their consistent neighbours) or on a raw network output (despeckle).  No float operation touches a vector; the
 * reference of the field does not enter.  Per field:
 *     vecs  float32 [H][W][2]     mask  uint8 [H][W]     valid, only  uint8 [H][W] or NULL     ksize in {3, 5, 7}, r = ksize / 2
 *     1 <= min_count <= ksize^2
 *     member(q)  = q inside the frame and (mask[q] & (valid ? valid[q] : 0xFF)) != 0
 *     N(p)       = { q : |qx - x| <= r, |qy - y| <= r, member(q) }      n(p) = |N(p)|   (the frame edge shrinks the window;
 *                                                                                        no padding)
 *     key(f)     = bits(f) ^ (bits(f) >> 31 ? 0xFFFFFFFF : 0x80000000)   uint32; a total order, equal to < on everything
 *                  but NaN; -0.0 < +0.0; NaNs sort beyond +-Inf by sign and payload
 *     med_c(p)   = the element of 0-based rank (n - 1) >> 1 in ascending key order among { vecs[q].c : q in N(p) }
 *                  c = u, v separately
 *     target(p)  = only ? only[p] != 0 : true
 *     ok(p)      = target(p) and n(p) >= min_count
 *     out_vecs[p].c = ok(p) ? the 4 bytes of med_c(p) : the 4 bytes of vecs[p].c
 *     out_mask[p]   = target(p) ? (ok(p) ? 1 : 0) : (mask[p] != 0 ? 1 : 0)
 * The median is the LOWER median: for an even count nothing is averaged, so every output word is a word of the input field
 * (NaN payloads, +-Inf, -0.0 and denormals survive).  The centre pixel is a member like any other; a pixel that `valid`
 * excludes is replaced by the median of its neighbours and becomes valid.  A valid pixel with fewer than min_count members
 * around it keeps its vector and gets mask 0.  `batch` fields lie back to back and a window never crosses from one field
 * into the next; offsets are size_t.  out_mask is optional.
 * One launch: a workgroup stages a tile of 64 x 16 pixels plus its halo in LDS as keys, every pixel sorts the keys of its
 * window in registers (non-members as 0xFFFFFFFF; the chosen rank is below n, so a real key equal to it yields the same
 * bytes) and picks the rank.  No atomics, no workspace.
 * vecs / out_vecs 8-byte aligned; the masks may sit at any address.  Outputs must not overlap inputs.
 * A bad argument -- a NULL vecs, mask or out_vecs, H or W < 1, batch outside [1, 65535], a ksize other than 3, 5, 7, a
 * min_count outside [1, ksize^2], an output range that overlaps an input range, a misaligned vector pointer -- returns
 * OFL_E_INVALID with a message before any launch.  The _dev entry is asynchronous; the host entry takes host pointers,
 * uploads, launches, downloads and synchronises.
 * Not built: a vector (L1) median, weighted and bilateral medians, ksize > 7, an iteration count (call it twice).
 */
int ofl_median_dev(const float *vecs, const uint8_t *mask, const uint8_t *valid, const uint8_t *only,
                   int H, int W, int batch, int ksize, int min_count,
                   float *out_vecs, uint8_t *out_mask, void *stream);
int ofl_median(const float *vecs, const uint8_t *mask, const uint8_t *valid, const uint8_t *only,
               int H, int W, int batch, int ksize, int min_count,
               float *out_vecs, uint8_t *out_mask);

/* ------------------------------------------------------------------ K17: convex upsampling of a network's coarse flow
 * The step between a flow network (RAFT, GMA, GMFlow / UniMatch, SEA-RAFT, FlowFormer) and the chain above: the network
 * emits the flow at 1/f resolution with 9 f^2 mask logits per coarse pixel, and every fine pixel is the softmax-weighted
 * combination of the 3 x 3 coarse neighbours, scaled by f.  Per item:
 *     vecs    float32 [h][w][2]     mask  uint8 [h][w]     factor f in {2, 4, 8}
 *     logits  9 f^2 channels of OFL_EL_F32, OFL_EL_F16 or OFL_EL_BF16, [9 f^2][h][w] (OFL_TENSOR_NCHW) or [h][w][9 f^2]
 *             (OFL_TENSOR_NHWC); channel c = k f^2 + i f + j  (RAFT's order): tap k = (dy + 1) 3 + (dx + 1) with dy, dx in
 *             {-1, 0, 1} as unfold orders them, sub-row i and sub-column j in [0, f)
 *     out_vecs  float32 [f h][f w][2]     out_mask  uint8 [f h][f w] or NULL
 * For the fine pixel (f y + i, f x + j), every operation float32 and rounded once (no FMA), taps in the order k = 0 .. 8:
 *     x_k   = the logit as float32 (exact)               M = max_k x_k               t_k = x_k - M
 *     e_k   = t_k < -87 ? 0 : exp32(t_k)
 *     u_k   = f * vecs[y + dy][x + dx] (exact), 0 where the tap lies outside the coarse frame -- the zero padding of
 *             unfold(padding=1); such a tap still takes part in the softmax
 *     s     = e_0 + e_1 + ... + e_8          a_c = e_0 u_0c + e_1 u_1c + ... + e_8 u_8c          out_c = a_c / s  (IEEE)
 *     out_mask = 1 where every tap INSIDE the frame has mask != 0, else 0; the vector is computed regardless
 *     exp32(t), t in [-87, 0]:  n = rint(t * 1.44269504f);  r = (t - n * 0.693359375f) - n * -2.12194440e-4f;
 *             p = 1/5040;  p = p r + c  for c = 1/720, 1/120, 1/24, 1/6, 1/2, 1, 1  (multiply and add rounded apart);
 *             result = the float whose bit pattern is bits(p) + (n << 23).   exp32(0) = 1 exactly; within 2 * 2^-24
 *             relative error of exp (tests/test_upsample_host.py measures it).
 * float32 subnormals are kept, as NumPy keeps them.  Logits that are NaN or +-Inf give unspecified values in their pixel
 * and never an access outside the buffers: no address depends on a logit's value.
 * `batch` items lie back to back; offsets are 64-bit.  One launch: a workgroup stages the 3 x (T + 2) coarse neighbourhood
 * of a tile of one coarse row in LDS, computes a band of fine rows into LDS and writes it out as whole rows.  No atomics,
 * no workspace.
 * vecs / out_vecs 8-byte aligned, logits aligned to their element, masks at any address.  Outputs must not overlap inputs.
 * A bad argument -- a NULL vecs, mask, logits or out_vecs, a factor other than 2, 4, 8, another elem or layout, h or w < 1,
 * f h or f w > 32766 (what the field kernels accept), batch outside [1, 65535], an overlap, a misaligned pointer -- returns
 * OFL_E_INVALID with a message before any launch.  The _dev entry is asynchronous; the host entry takes host pointers,
 * uploads, launches, downloads and synchronises.
 * Not built: a batched bilinear resize, mask-aware renormalisation of the softmax, windows other than 3 x 3, other factors,
 * a backward pass.
 */
int ofl_upsample_convex_dev(const float *vecs, const uint8_t *mask, const void *logits, int elem, int layout,
                            int h, int w, int batch, int factor,
                            float *out_vecs, uint8_t *out_mask, void *stream);
int ofl_upsample_convex(const float *vecs, const uint8_t *mask, const void *logits, int elem, int layout,
                        int h, int w, int batch, int factor,
                        float *out_vecs, uint8_t *out_mask);

/* ------------------------------------------------------------------ K18: on-demand correlation lookup of two feature tensors
 * The correlation step of a flow network -- RAFT's multi-level lookup (levels = 4, r = 4, scale = 1 / sqrt(C)), the local
 * cost volume of PWC-Net (levels = 1 after a warp by K12) -- without the all-pairs volume of (H W)^2 floats: the dot
 * products a pixel needs are formed when it asks for them.  Per item:
 *     f1   C channels on an H x W grid, channels last [H][W][C], of OFL_EL_F32, OFL_EL_F16 or OFL_EL_BF16
 *     f2_l level l of the pyramid of f2, channels last [H_l][W_l][C]: level 0 is f2 as stored (any of the three types, not
 *          necessarily f1's), level l >= 1 is the 2 x 2 mean of level l - 1 (ofl_avgpool2_dev), always float32:
 *              ((a + b) + (c + d)) * 0.25f      a, b, c, d = top-left, top-right, bottom-left, bottom-right
 *          H_l = H >> l, W_l = W >> l: a trailing odd row or column is dropped, as avg_pool2d(2, stride=2) drops it; an
 *          empty level is refused.  16-bit values are widened to float32, which is exact.
 *     flow float32 [H][W][2] in pixels of the H x W grid, or NULL (u = v = 0, nothing is read); one field per item, or one
 *          for all (flow_shared).  No mask is read and none is written.
 * For pixel (x, y), every operation float32 and rounded once (no FMA):
 *     px = map_coord(x, u, sign) * 2^-l,  py = map_coord(y, v, sign) * 2^-l      map_coord: the float64 sum x +- u rounded
 *          once to float32, as in K1 / K12; the product with a power of two is exact.  sign +1 is the 's' rule, -1 the 't' rule
 *     t  = make_tap<quant>(px, py)        K1's taps: OFL_QUANT_EXACT floor and fraction (what grid_sample does),
 *          OFL_QUANT_OPENCV the 1/32-px snap; t.ix, t.iy saturated to [-32768, 32767]
 *     D(ix, iy) = sum_c f1[x, y, c] * f2_l[ix, iy, c]  for the (2r + 2)^2 integer taps ix in [t.ix - r, t.ix + r + 1], iy in
 *          [t.iy - r, t.iy + r + 1]; exactly 0 where the tap lies outside the H_l x W_l frame.  The order of the sum:
 *          the channels go in groups of V = OFL_CORR_V = 4 consecutive channels, group g to partial sum g mod L,
 *          L = OFL_CORR_L = 16; partial sum p starts with its first product and adds the others in ascending channel order
 *          (p_0 = c0 + c1 + c2 + c3 + c64 + c65 + ..., left to right); the partial sums are added in the pairwise tree
 *          ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))  +  the same of p8 .. p15.  A partial sum without a channel
 *          (C <= 4 p) is left out of the tree -- nothing is added for it, not even + 0.0f, so a sum of -0.0 stays -0.0 --
 *          and the tree keeps its shape: with C = 20, D = ((p0 + p1) + (p2 + p3)) + p4.  V and L do not depend on C, N,
 *          the element types or the position in a batch: 16 lanes x 4 channels is one 128- or 256-byte load of a row.
 *     value(ox, oy) = blend4(D(t.ix + ox, t.iy + oy), D(t.ix + ox + 1, t.iy + oy), D(t.ix + ox, t.iy + oy + 1),
 *          D(t.ix + ox + 1, t.iy + oy + 1), t) * scale          ox, oy in [-r, r]; K1's blend, left to right; all
 *          (2r + 1)^2 samples of a pixel share the centre's fraction, as alt_cuda_corr does
 *     out  float32, planar [total_channels][H][W] per item; this level writes the (2r + 1)^2 channels from first_channel:
 *          channel first_channel + k with k = (ox + r)(2r + 1) + (oy + r) for OFL_CORR_XY -- the order of RAFT's
 *          CorrBlock, whose first window axis moves x -- and k = (oy + r)(2r + 1) + (ox + r) for OFL_CORR_YX, the row-major
 *          order of PWC-style cost volumes.  A multi-level lookup is one call per level with first_channel = l (2r + 1)^2.
 * A NaN or huge coordinate leads only to taps that are inside the frame or skipped (the clamps of make_tap; the window
 * arithmetic is int); the values of a pixel with a NaN coordinate are unspecified.  No address depends on a feature value.
 * `N` items lie back to back; offsets are 64-bit.  One launch per level: a wave reads whole rows of f2_l, 16 lanes a row;
 * no atomics, no workspace.  Both entries take channels-last tensors only (ofl_tensor_permute_dev makes one of a planar
 * tensor, at the cost of one read and one write of it).
 * f1 / f2_l aligned to their element (a base aligned to four elements, with C % 4 == 0, is read four elements a load),
 * out 4-byte, flow 8-byte aligned.  A bad argument -- a NULL f1, f2_l or out, an element other than the three (OFL_EL_F64
 * included), an unknown order or quant, a sign other than +-1, r outside [1, 4], level outside [0, 7], N or C outside
 * [1, 65535], H or W outside [1, 32766], H_l, W_l other than H >> level, W >> level or < 1, channels
 * [first_channel, first_channel + (2r + 1)^2) that do not lie in [0, total_channels), an output that overlaps an input, a
 * misaligned pointer -- returns OFL_E_INVALID with a message before any launch.  ofl_avgpool2_dev refuses H or W < 2 likewise.
 * The _dev entries are asynchronous.  The host entry ofl_corr_lookup takes host pointers -- f1 and f2 (level 0) channels last,
 * the optional flow, out [N][levels (2r + 1)^2][H][W] with levels in [1, 8] --, uploads, builds the pyramid, launches the
 * `levels` lookups, downloads and synchronises.
 * Not built: a backward pass, radii above 4, strides and dilations, an MFMA or FMA path (neither can be restated in NumPy
 * float32), 16-bit output, the all-pairs volume itself.
 */
enum { OFL_CORR_XY = 0, OFL_CORR_YX = 1 };
#define OFL_CORR_V 4
#define OFL_CORR_L 16
int ofl_avgpool2_dev(const void *src, int elem, int N, int C, int H, int W, float *dst, void *stream);
int ofl_corr_lookup_dev(const void *f1, int elem1, const void *f2_l, int elem2, int N, int C, int H, int W, int H_l, int W_l,
                        int level, const float *flow, int flow_shared, int sign, int r, float scale, int order, int quant,
                        float *out, int total_channels, int first_channel, void *stream);
int ofl_corr_lookup(const void *f1, int elem1, const void *f2, int elem2, int N, int C, int H, int W, int levels,
                    const float *flow, int flow_shared, int sign, int r, float scale, int order, int quant, float *out);

/* ------------------------------------------------------------------ K19: global matching of two feature tensors
 * The first flow of a GMFlow / UniMatch- or FlowFormer-style matcher, and of a classical forward / backward pair that K13,
 * K15 and K16 then clean up: every pixel of f1 is dotted with every pixel of f2, a softmax runs over all H W candidates and
 * the flow is the expected coordinate minus the pixel's own.  The (H W)^2 volume of the textbook formulation
 * (f1 @ f2^T, softmax(dim=-1), @ grid) is never stored.  Per item:
 *     f1, f2   C channels on an H x W grid, channels last [H][W][C], both of ONE element type: OFL_EL_F16, OFL_EL_BF16 or
 *              OFL_EL_F32.  The keys are the pixels of f2, numbered k = ky W + kx.
 * For the query pixel q = (x, y) of f1:
 *     D_k  = sum_c f1[q, c] * f2[k, c]     on the matrix core, float32 accumulation from 0, channels ascending through the K
 *            steps (C is padded to the step with zeros).  16-bit: mfma_f32_32x32x16_{f16,bf16}, 16 channels a step; the order
 *            inside one instruction is the hardware's and is not stated.  float32: mfma_f32_32x32x2f32, 2 channels a step.
 *     s_k  = D_k * scale                   float32, rounded once
 *     m    = max_k s_k                     exact, no order
 *     idx  = the smallest k with s_k == m  (ties: the first in row-major order); always in [0, H W)
 *     t_k  = s_k - m
 *     e_k  = t_k < -87 ? 0 : exp32(t_k)    K17's exp32 above, the stated float32 sequence; exp32(0) = 1
 *     l = sum_k e_k,  ax = sum_k e_k * (float)kx,  ay = sum_k e_k * (float)ky      products rounded once, no FMA; the ORDER:
 *            the keys go in tiles of T = OFL_MATCH_TILE = 32 consecutive keys; tile j belongs to group w = j mod G,
 *            G = OFL_MATCH_WAVES = 4; inside a tile, key offset o belongs to half h = (o >> 2) & 1 (o = 0 .. 3, 8 .. 11,
 *            16 .. 19, 24 .. 27: h = 0; the others: h = 1).  Each of the 2 G partial sums P[w][h] starts at +0 and adds its
 *            keys in ascending k.  Then S_w = P[w][0] + P[w][1] and the sum is ((S_0 + S_1) + S_2) + S_3.  A partial sum without
 *            a key is +0, and since no term is negative no sum is ever -0.0, so adding it -- like adding any e_k = 0 --
 *            changes no bit.  T and G do not depend on N, C, the element type, alignment, the position in a batch or the
 *            number of CUs: the 32 x 32 accumulator tile holds a query on a lane and 16 keys in each lane half's registers,
 *            and four waves share the keys of a query.
 *     mx = ax / l,  my = ay / l            IEEE division
 *     u  = mx - (float)x,  v = my - (float)y
 *     out_vecs = sign * (u, v)             sign +1: 's' (q + flow is the match); -1: 't'
 *     out_conf = 1.0f / l                  the softmax probability of the best candidate
 *     out_mask = conf >= min_conf          min_conf = 0 sets every pixel
 *     out_index = idx                      int32
 * Two sweeps over the keys: the first forms every D_k and keeps m and idx, the second forms every D_k again by the same
 * instruction sequence -- so t_k <= 0 everywhere and = 0 at idx -- and accumulates l, ax, ay; a tile whose every t_k < -87
 * is skipped after its dots, which changes no bit (above).  Keys beyond H W in the last tile take part in nothing; queries
 * beyond H W write nothing.  No address depends on a feature value: NaN / Inf features give unspecified values, an index in
 * range and no fault.  `N` items lie back to back; offsets are 64-bit.  One launch; no atomics, no workspace.
 *     out_vecs float32 [H][W][2], out_mask uint8 [H][W], out_conf float32 [H][W] or NULL, out_index int32 [H][W] or NULL
 * f1 / f2 aligned to their element: 16-byte-aligned bases with C % 8 == 0 (16-bit) or C % 4 == 0 (float32) are read 16 bytes
 * a load, anything else element by element.  out_vecs 8-byte, out_conf and out_index 4-byte aligned.  A bad argument -- a
 * NULL f1, f2, out_vecs or out_mask, an element other than the three (OFL_EL_F64 included), a sign other than +-1, a negative
 * or NaN min_conf, N outside [1, 65535], C outside [1, 512], H or W outside [1, 32766], an output that overlaps an input or
 * another output, a misaligned pointer -- returns OFL_E_INVALID with a message before any launch.  The _dev entry is
 * asynchronous; the host entry takes host pointers, uploads, launches, downloads and synchronises.
 * Not built: a mask over the keys (padded frames), a local-window softmax (K18's output plus a softmax), returning the
 * probabilities themselves, a key split across workgroups with a merge pass for very small frames, a backward pass, fp8,
 * mixed element types.
 */
#define OFL_MATCH_TILE 32
#define OFL_MATCH_WAVES 4
int ofl_global_match_dev(const void *f1, const void *f2, int elem, int N, int C, int H, int W, float scale, int sign,
                         float min_conf, float *out_vecs, uint8_t *out_mask, float *out_conf, int32_t *out_index, void *stream);
int ofl_global_match(const void *f1, const void *f2, int elem, int N, int C, int H, int W, float scale, int sign,
                     float min_conf, float *out_vecs, uint8_t *out_mask, float *out_conf, int32_t *out_index);

/* ------------------------------------------------------------------ K20: forward warp by splatting
 * The forward warp of a network pipeline (Niklaus & Liu, Softmax Splatting, CVPR 2020): every source pixel adds its value to
 * the four pixels around where an 's'-reference field sends it, with bilinear weights times an importance factor.  Summation,
 * average and softmax splatting; the weight plane alone (C = 0) is the range map "how many source pixels land here".  This is
 * NOT the reference's 's' apply (griddata on the Delaunay path, K3) and does not replace it.
 *     src    N items of C channels of OFL_EL_F32, OFL_EL_F16 or OFL_EL_BF16, (N, C, H, W) or (N, H, W, C) (K12's layouts)
 *     flow   [H][W][2] float32 with fmask [H][W]: ONE field and mask for all items when flow_shared != 0, else N back to back
 *     z      float32 [H][W] per field, the importance (OFL_SPLAT_SOFTMAX only; otherwise ignored, may be NULL);  alpha float
 *     N in [1, 65535], C in [0, 65535], H and W as K12 allows; element offsets are 64-bit
 * The sums are INTEGERS: int64 accumulators filled by 64-bit integer atomic adds (ordinary vector memory instructions), and
 * the softmax shift is an integer atomic max.  Both commute, so the result is a function of the inputs alone and
 * tests/splat_ref.py restates it with np.add.at / np.maximum.at byte for byte.
 * Per source pixel (x, y); every float operation is float32 and rounded once (no FMA):
 *   1. skipped if fmask == 0, or u or v is not finite, or px = float(x) + u or py = float(y) + v has magnitude >= 2^30, or --
 *      softmax -- zs = alpha * z is not finite.  A skipped pixel contributes nothing and adds 1 to counters[0] (once per
 *      pixel of a FIELD: a shared field counts once, not once per item).
 *   2. x0 = floorf(px), fx = px - x0, likewise y; the four taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) have the
 *      weights w = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy.  A tap whose weight is exactly 0 or whose pixel
 *      lies outside the frame does not exist: an integer landing touches one pixel.
 *   3. e = 1 for OFL_SPLAT_SUM and OFL_SPLAT_AVERAGE.  OFL_SPLAT_SOFTMAX: a first launch records PER TARGET PIXEL the maximum
 *      zs over all taps that exist there -- an integer atomic max on the order-preserving int32 key of the float
 *      (b ^ ((b >> 31) & 0x7fffffff) of the bit pattern b), the plane initialised to the smallest key -- and the accumulate
 *      launch forms t = zs - zmax[target] (<= 0) and e = t < -87 ? 0 : exp32(t), K17's exp32.  The shift cancels in the
 *      ratio: this is softmax splatting exactly.  Because the shift is per target pixel and not per field, the largest
 *      weight at every covered pixel has e = 1: no region whose importances are all low can be wiped out by the fixed point.
 *   4. we = w * e; the tap pixel's weight accumulator gains the integer nearest to we * 2^32 (ties to even).
 *   5. per channel val = we * float(I_c); the accumulator gains the integer nearest to val * 2^frac_bits (ties to even),
 *      frac_bits in [0, 40], 24 by default.  A val that is NaN or has |val| * 2^frac_bits >= 2^62 contributes 0 and adds 1 to
 *      counters[1].  The caller's precondition, not checked: landings per pixel * max |val| < 2^(63 - frac_bits).
 * Per target pixel, with D the weight accumulator and A_c the channel accumulators, each converted to float64 to nearest:
 *     weight = float32(D * 2^-32)                        valid = D >= the integer nearest to min_weight * 2^32
 *     SUM:               out_c = float32(A_c * 2^-frac_bits)                          (valid is informational)
 *     AVERAGE, SOFTMAX:  out_c = valid ? float32((A_c / D) * 2^(32 - frac_bits)) : 0
 * 16-bit outputs are then rounded to storage with ofl_export_flow_dev's rounding: a SECOND rounding.  min_weight in
 * [2^-20, 1], 2^-10 by default.  Consequence: every finite float16 is a multiple of 2^-24, so with frac_bits = 24 a float16
 * tensor under an integer translation comes back byte for byte in AVERAGE and SUM; so does integer-valued float32 / bfloat16.
 *     dst     as src (NULL allowed when C = 0)
 *     valid   uint8, weight float32 (each may be NULL): [H][W] when flow_shared != 0, else [N][H][W]
 *     counters  device uint32[2] or NULL, ADDED to by integer atomics: the caller zeroes it
 *     workspace ofl_splat_workspace_bytes = 8 (C + 1) H W per item, plus 4 H W per field for softmax; 8-byte aligned; the
 *               entry zeroes it on the stream.  Accumulators are channels-last [N][H][W][C + 1], the weight last.
 * Launches: [the max pass,] accumulate, finish.  No loop depends on the data: a field that contracts everything into one
 * pixel costs contention, not iterations.  flow 8-byte aligned, src / dst aligned to their element, z / weight / counters
 * 4-byte, masks at any address; src may be the field's own vector buffer (C = 2, channels-last: the projection of a field).
 * Outputs must not overlap inputs.  A bad argument -- a NULL flow or fmask, a NULL src or dst with C > 0, C = 0 without valid
 * or weight, another elem, layout or mode, softmax without z or with a non-finite alpha, frac_bits or min_weight out of
 * range, sizes out of range, an overlap, a misaligned pointer, a short workspace -- returns OFL_E_INVALID with a message
 * before any launch.  The _dev entry is asynchronous; the host entry takes host pointers (counters_host: host uint32[2] or
 * NULL, written, not added to), uploads, launches, downloads and synchronises.
 * Not built: linear splatting, a backward pass, kernels other than bilinear, float accumulators, channel chunking to cap
 * the workspace, combining the taps of neighbouring lanes before the atomic.
 */
enum { OFL_SPLAT_SUM = 0, OFL_SPLAT_AVERAGE = 1, OFL_SPLAT_SOFTMAX = 2 };
int ofl_splat_workspace_bytes(int N, int C, int H, int W, int flow_shared, int mode, size_t *bytes);
int ofl_splat_dev(const void *src, int elem, int layout, int N, int C, int H, int W,
                  const float *flow, const uint8_t *fmask, int flow_shared, const float *z, float alpha,
                  int mode, int frac_bits, float min_weight, void *workspace, size_t workspace_bytes,
                  void *dst, uint8_t *valid, float *weight, uint32_t *counters, void *stream);
int ofl_splat(const void *src, int elem, int layout, int N, int C, int H, int W,
              const float *flow, const uint8_t *fmask, int flow_shared, const float *z, float alpha,
              int mode, int frac_bits, float min_weight, void *dst, uint8_t *valid, float *weight, uint32_t *counters_host);

/* ------------------------------------------------------------------ K21: photometric error of a warp
 * The third check of a field, after a ground truth (K14) and a backward twin (K13): take a pixel of the field's own frame,
 * find where the field sends it in the other frame, and ask whether it looks the same there -- the brightness- or
 * feature-constancy error that unsupervised flow, candidate selection and occlusion reasoning are built on, and, negated
 * and scaled, the importance metric of softmax splatting (K20; Niklaus & Liu: -alpha |I0 - backwarp(I1, F0->1)|).  The
 * tensor analogue of K13: K12's taps and blend, but the C warped channels are reduced to ONE float per pixel and never stored.
 *     near   the tensor of the field's own frame, far the tensor of the other frame: N items of C channels, both of ONE
 *            element type (OFL_EL_F32, OFL_EL_F16, OFL_EL_BF16) and ONE layout ((N, C, H, W) or (N, H, W, C), K12's)
 *     flow   [H][W][2] float32 with fmask [H][W]; near_mask, far_mask [H][W] or NULL (all valid).  flow_shared != 0: ONE
 *            field and one of each mask serve all N items; otherwise N of each lie back to back
 *     sign   +1 for an 's' field, -1 for a 't' field, as in K13;  N and C in [1, 65535], H and W in [1, 32766]
 * Per item n and pixel (x, y), every operation float32 and rounded once (no FMA); 16-bit elements are widened exactly:
 *     tap      = the bilinear tap of (x, y) + sign * flow[y][x]     (map_coord / make_tap, `quant` as in K1 / K12 / K13;
 *                                                                    a non-finite vector samples what it samples there)
 *     w_c      = far[n, c]'s four taps blended (0 outside the frame)                == K12's value BEFORE its rounding to storage
 *     am       = far_mask's four taps blended as 0.0f / 1.0f (NULL: 1 inside the frame, 0 outside)
 *     covered  = fmask & near_mask (NULL: 1) & (am == 1.0f)                         == K12's valid, ANDed with near_mask
 *     d_c      = near[n, c] - w_c
 *     t_c      = |d_c| (OFL_PHOTO_L1)  |  d_c * d_c (OFL_PHOTO_L2)  |  sqrtf(d_c * d_c + eps * eps) (OFL_PHOTO_CHARBONNIER)
 *     S        = the sum of the t_c in the fixed order below
 *     e        = S * inv_c,  inv_c = (float)(1.0 / (double)C);  OFL_PHOTO_L2: e = sqrtf(e), the root mean square
 *     err      = covered ? e : 0.0f                                                 (sqrtf: the correctly rounded one, as in K13)
 *     within   = covered & (e <= tau)                                               (a NaN error is never within)
 * The order of the sum depends on C alone -- not on layout or element type, so a planar and a channels-last tensor of the
 * same values give the same bytes.  It is K18's scheme: the groups of 4 consecutive channels g = c / 4 are dealt to 16
 * partial sums, p_j = the t_c with (c / 4) % 16 == j, added in ascending c to +0.0f; then p_j += p_(j + 8) for j < 8,
 * p_j += p_(j + 4) for j < 4, p_j += p_(j + 2) for j < 2, and S = p_0 + p_1.  Every t_c is >= +0 or NaN, so a partial sum
 * without channels is +0.0f and adding it changes nothing.  tests/photometric_ref.py restates all of this in NumPy.
 * This is not a function of the reference and the formula is its definition: there is NO zero-flow short cut in either
 * `quant` mode, as in K13.
 *     err float32, covered and within uint8: [N][H][W].  One of err / within is required, covered is optional; within is
 *     computed when it is given, and tau must then be finite and >= 0.  eps (finite, >= 0) is used by CHARBONNIER only.
 *     counts  device uint32[N][2] = {covered, within} pixels per item, or NULL: ADDED to, the caller zeroes it; each
 *             workgroup issues at most one integer atomic add per counter.  No other atomics, no workspace.
 * near / far aligned to their element, flow 8-byte, err and counts 4-byte, masks at any address; element offsets are
 * 64-bit.  Outputs must not alias inputs.  A bad argument -- a NULL near / far / flow / fmask, another elem, layout, metric
 * or quant, sizes out of range, sign not +-1, eps or tau negative or not finite, neither err nor within, a misaligned
 * pointer -- returns OFL_E_INVALID with a message before any launch.  The _dev entry is asynchronous, one launch; the host
 * entry takes host pointers (counts_host: host uint32[N][2] or NULL), uploads, launches, downloads and synchronises.
 * Bytes per pixel: reads 2 C elements (near streamed, far gathered) + 8 (flow) + 1 to 3 (masks); writes 4 + 1 + 1, where
 * K12 plus an elementwise pass writes and re-reads C elements more.
 * Not built: the window metric gradient constancy (the census distance is K22, below, SSIM is K26), a reduction
 * of the map to a mean or percentiles, a backward pass, mixed element types or layouts, integer tensors on the device,
 * padding offsets.
 */
enum { OFL_PHOTO_L1 = 0, OFL_PHOTO_L2 = 1, OFL_PHOTO_CHARBONNIER = 2 };
int ofl_photometric_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                        const float *flow, const uint8_t *fmask, int flow_shared, int sign,
                        const uint8_t *near_mask, const uint8_t *far_mask,
                        int metric, float eps, float tau,
                        float *err, uint8_t *covered, uint8_t *within, uint32_t *counts, int quant, void *stream);
int ofl_photometric(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                    const float *flow, const uint8_t *fmask, int flow_shared, int sign,
                    const uint8_t *near_mask, const uint8_t *far_mask,
                    int metric, float eps, float tau,
                    float *err, uint8_t *covered, uint8_t *within, uint32_t *counts_host, int quant);

/* ------------------------------------------------------------------ K22: census distance of a warp over a window
 * K21 compares raw values, so a change of exposure or gain between the two frames reads as error everywhere.  The census
 * distance compares the ORDER of the intensities in a K x K window around the pixel, in `near` and in the warped `far`
 * (Zabih & Woodfill; the ternary census unsupervised flow trains and selects candidates on): a brightness change that
 * keeps the order costs nothing.  One fused launch: the warped image is never written.
 *     near, far, elem, layout, N, C, H, W, flow, fmask, flow_shared, sign, near_mask, far_mask, quant: K21's, but C in [1, 4]
 *     window    K in {3, 5, 7}, r = K / 2;    mode  OFL_CENSUS_HARD or OFL_CENSUS_SOFT
 *     p0, p1    HARD: p0 = delta >= 0 (p1 is not read);  SOFT: p0 = noise > 0, p1 = knee > 0 (0.81 and 0.1 in the literature,
 *               both meant for intensities 0 ... 255)
 *     min_count in [1, K * K - 1]: the members a window needs;  tau as in K21
 * Per item n and pixel q, every operation float32 and rounded once (no FMA), exactly as K21 computes them:
 *     tap(q), w_c(q), am(q);   cov1(q) = fmask & near_mask (NULL: 1) & (am(q) == 1.0f)          == K21's covered
 *     A(q) = (near_0 + ... + near_(C-1)) * inv_c,  B(q) = (w_0 + ... + w_(C-1)) * inv_c,  inv_c = (float)(1.0 / (double)C),
 *            each sum started at +0.0f and added in ascending c                                   (K21's order for one group)
 *     member(q) = q inside the frame & cov1(q)
 * For the pixel p and every offset d = (dx, dy) with |dx|, |dy| <= r and d != 0:
 *     a = A(p + d) - A(p);   b = B(p + d) - B(p)
 *     HARD:  s(v) = v > delta ? 1 : (v < -delta ? -1 : 0)   (a NaN compares false twice: 0);   t_d = s(a) != s(b) ? 1.0f : 0.0f
 *     SOFT:  rho(v) = v / sqrtf(noise + v * v)   (product, sum, the correctly rounded sqrtf, a correctly rounded division)
 *            g = rho(a) - rho(b);   q = g * g;   t_d = q / (knee + q)
 *     t_d is REPLACED by +0.0f where !member(p + d)                 (a select, not a product: a NaN there does not leak)
 *     R_dy = t_(-r,dy) + ... + t_(r,dy), added in ascending dx to +0.0f;   S = R_(-r) + ... + R_r, in ascending dy to +0.0f
 *     n = the number of member offsets;   covered(p) = cov1(p) & (n >= min_count)
 *     e = S / (float)n (correctly rounded);   err = covered ? e : 0.0f;   within = covered & (e <= tau)
 * min_count = K * K - 1 asks for the full window, the border mask the literature uses.  There is NO zero-flow short cut.
 * tests/census_ref.py restates all of this in NumPy.
 *     err, covered, within, counts: K21's ([N][H][W]; one of err / within required; counts uint32[N][2] ADDED to, at most one
 *     integer atomic add per workgroup and counter; no other atomics, no workspace).
 * Alignment, 64-bit offsets, aliasing and the two entries (asynchronous _dev, host-staged) as in K21.  A bad argument -- those
 * of K21, C > 4, another window or mode, min_count outside [1, K * K - 1], delta negative, noise or knee not positive, any
 * of them or tau (when within is given) not finite -- returns OFL_E_INVALID with a message before any launch.
 * Not built: C > 4 and a per-channel census, luma weights (pass a reduced plane), gradient constancy (SSIM is K26), windows above
 * 7 or not square, a reduction of the map, a backward pass, mixed element types or layouts, integer tensors on the device.
 */
enum { OFL_CENSUS_HARD = 0, OFL_CENSUS_SOFT = 1 };
enum { OFL_CENSUS_MAX_C = 4 };
int ofl_census_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                   const float *flow, const uint8_t *fmask, int flow_shared, int sign,
                   const uint8_t *near_mask, const uint8_t *far_mask,
                   int window, int mode, float p0, float p1, int min_count, float tau,
                   float *err, uint8_t *covered, uint8_t *within, uint32_t *counts, int quant, void *stream);
int ofl_census(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
               const float *flow, const uint8_t *fmask, int flow_shared, int sign,
               const uint8_t *near_mask, const uint8_t *far_mask,
               int window, int mode, float p0, float p1, int min_count, float tau,
               float *err, uint8_t *covered, uint8_t *within, uint32_t *counts_host, int quant);

/* ------------------------------------------------------------------ K23: variational refinement of a field on two images
 * K13, K21 and K22 score a field, K15 and K16 move existing vectors around; K23 moves a vector a fraction of a pixel towards
 * where the images say it belongs: the variational refinement of Brox et al. (ECCV 2004) without the gradient-constancy
 * term, the step EpicFlow, DeepFlow, RICFlow and DIS end with.  out = f + d, where d = (du, dv) approximately minimises
 *     E(d) = sum_q data(q) (delta / n(q)) psi(r(q)^2 / n(q) ...) + alpha sum_q psi(|grad(u + du)|^2 + |grad(v + dv)|^2),
 *     psi(s^2) = sqrt(s^2 + eps^2)
 * by ONE linearisation (one warp), `fixed_point` lagged-weight updates and `sor` red-black SOR sweeps per update.  Calling
 * it again re-warps; there is no loop over warps inside.  There is NO zero-flow short cut.
 *     near, far, elem, layout, C, H, W, sign, near_mask, far_mask, quant: K22's (C in [1, 4]); N fields, fmasks and masks lie
 *     back to back, one per item;  valid: uint8 [N][H][W] or NULL (all set), as in K15 / K16
 * Every operation is float32 and rounded once (no FMA); sqrtf and every division are the correctly rounded ones; a sum
 * written a + b + c is (a + b) + c.  (u, v) = flow[q], ex = (1, 0), ey = (0, 1), zeta2 = zeta * zeta, eps2 = eps * eps.
 * Setup, per item and pixel q:
 *     A(q), B(q), cov1(q)   K22's: the channel means of `near` and of the warped `far`, and K21's covered
 *     dom(q)  = fmask(q) & valid(q) & isfinite(u) & isfinite(v)               a pixel outside the domain keeps its vector bit
 *               for bit, has d = 0 and is nobody's neighbour
 *     Bx = 0.5f * (B(q + ex) - B(q - ex)),  By = 0.5f * (B(q + ey) - B(q - ey));  a neighbour outside the frame is replaced
 *               by q itself;   gx = sign > 0 ? Bx : -Bx,  gy likewise;   Iz = B(q) - A(q)
 *     n       = gx * gx + gy * gy + zeta2
 *     data(q) = dom(q) & cov1(q) & cov1 at every 4-neighbour inside the frame & isfinite(gx) & isfinite(gy) & isfinite(Iz)
 *     d(q)    = (+0.0f, +0.0f)
 * Each of the fixed_point iterations, from the current d:
 *     r  = Iz + gx * du + gy * dv;    wD = data ? delta / (n * sqrtf((r * r) / n + eps2)) : +0.0f              (a select)
 *     p  = wD * gx,  q = wD * gy;   A11 = p * gx,  A12 = p * gy,  A22 = q * gy,  b1 = -(p * Iz),  b2 = -(q * Iz)
 *     U  = u + du,  V = v + dv;   Ux = 0.5f * (U(q + ex) - U(q - ex)),  Uy, Vx, Vy likewise; a neighbour outside the frame
 *          OR the domain is replaced by q itself
 *     s  = alpha / sqrtf(Ux * Ux + Uy * Uy + Vx * Vx + Vy * Vy + eps2)
 *     w(q, q') = q' inside the frame and the domain ? 0.5f * (s(q) + s(q')) : +0.0f
 *     sigma = +0.0f + w_up + w_left + w_right + w_down                        (q - ey, q - ex, q + ex, q + ey: the order of
 *                                                                             every sum over the neighbours)
 *   and each of the `sor` sweeps, colour 0 then colour 1 with colour = (x + y) & 1, for the domain pixels of that colour:
 *     t_k  = neighbour k ? w_k * ((u' + du') - u) : +0.0f                      (a select; v likewise)
 *     du*  = (b1 - A12 * dv + t_up + t_left + t_right + t_down) / (A11 + sigma);    du_new = du + omega * (du* - du)
 *     ok_u = (A11 + sigma != 0) & isfinite(du_new)
 *     dv*  = (b2 - A12 * (ok_u ? du* : du) + ...) / (A22 + sigma);    dv_new and ok_v likewise
 *     du <- ok_u ? du_new : du;    dv <- ok_v ? dv_new : dv
 *   A component whose denominator is 0 or whose new value is not finite stays as it is, so a NaN or Inf in an image or a
 *   vector never spreads.  A pixel reads only its own values and the other colour's, so the result does not depend on how a
 *   sweep is scheduled: the bits are reproducible.
 * Finally out(q) = dom(q) ? (du != 0 ? u + du : u, dv != 0 ? v + dv : v) : flow(q): d = 0 keeps the bits of the input, the
 * sign of a zero included.  The mask of the result is fmask.  tests/refine_ref.py restates all of this in NumPy.
 *     alpha, delta finite and >= 0;  zeta, eps finite and > 0 with zeta2, eps2 finite and > 0;  fixed_point, sor in [1, 32];
 *     omega in (0, 2).
 *     Defaults of the Python layer: 20, 5, 0.1, 0.1, 5, 5, 1.6 -- eps is deliberately not Brox's 0.001, which makes a flat
 *     field so stiff that 25 sweeps move it 1 % of the way.
 *     out     float32 [N][H][W][2];   data  uint8 [N][H][W] or NULL: the data map
 *     workspace  ofl_refine_workspace_bytes = 29 N H W (d, gx, gy, Iz, wD, s, flags), 8-byte aligned, caller-provided
 * Launches: setup, then per iteration one for the weights and two per sweep, then one that writes out; no atomics, 64-bit
 * offsets across items.  near / far aligned to their element, flow, out and workspace 8-byte, masks at any address.  out
 * and the workspace must not overlap another argument.  A bad argument -- a NULL near / far / flow / fmask / out, another
 * elem, layout or quant, C > 4, sizes out of range, sign not +-1, a parameter out of its range or not finite, an overlap, a
 * misaligned pointer, a short workspace -- returns OFL_E_INVALID with a message before any launch.  The _dev entry is
 * asynchronous; the host entry takes host pointers, uploads, launches, downloads and synchronises.
 * Not built: the gradient-constancy term, per-channel data terms and C > 4, a loop over warps or a pyramid inside the call,
 * image-driven (edge-aware) smoothness weights, a choice of omega, an energy read-back, a backward pass, mixed element types
 * or layouts, several sweeps on one LDS tile.
 */
enum { OFL_REFINE_MAX_C = 4, OFL_REFINE_MAX_ITER = 32 };
int ofl_refine_workspace_bytes(int N, int H, int W, size_t *bytes);
int ofl_refine_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                   const float *flow, const uint8_t *fmask, int sign,
                   const uint8_t *near_mask, const uint8_t *far_mask, const uint8_t *valid,
                   float alpha, float delta, float zeta, float eps, int fixed_point, int sor, float omega,
                   void *workspace, size_t workspace_bytes, float *out, uint8_t *data, int quant, void *stream);
int ofl_refine(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
               const float *flow, const uint8_t *fmask, int sign,
               const uint8_t *near_mask, const uint8_t *far_mask, const uint8_t *valid,
               float alpha, float delta, float zeta, float eps, int fixed_point, int sor, float omega,
               float *out, uint8_t *data, int quant);

/* ------------------------------------------------------------------ K24: dense inverse search of a field on two images
 * K23 moves a vector a fraction of a pixel; K24 finds it: the patch inverse search and the densification of Dense Inverse
 * Search (Kroeger et al., ECCV 2016; OpenCV's DISOpticalFlow).  Every patch of P x P pixels on a grid of stride S takes
 * `iterations` inverse-compositional Lucas-Kanade translation steps from the vector of `flow` at its centre, then every
 * pixel takes the weighted average of the patches that cover it.  There is NO zero-flow short cut.
 *     near, far, elem, layout, C in [1, 4], H, W, sign, quant: K22's;  N items, fields and fmasks lie back to back
 *     flow  float32 [N][H][W][2] or NULL: the zero field (fmask is then not read);  fmask uint8 [N][H][W] or NULL: all set
 * Every operation is float32 and rounded once (no FMA); every division is the correctly rounded one; a sum written
 * a + b + c is (a + b) + c.  ex = (1, 0), ey = (0, 1), PP = P * P.
 * Setup, per item and pixel q:
 *     A(q), Bm(q)  K22's channel means of `near` and of the UNWARPED `far` (ascending c from +0.0f, times (float)(1.0 / C)),
 *                  two float32 planes in the workspace: the mean first, the blend later, so a tap costs the same for any C
 *     Ax = 0.5f * (A(q + ex) - A(q - ex)),  Ay = 0.5f * (A(q + ey) - A(q - ey));  a neighbour outside the frame is replaced
 *                  by q itself (K23's rule);   gx = sign > 0 ? Ax : -Ax,  gy likewise
 * Patch grid: along an axis of length n the origins are 0, S, 2 S, ... <= n - P, and one more at n - P where the last of
 *     them is not n - P, so every pixel lies in a patch;  origin(i) = min(i S, n - P);  ny x nx patches in row-major order.
 * Sample: S(q, u) = the bilinear blend of Bm at the position (K12's map_coord of q and u under `sign`) clamped
 *     componentwise to [0, W - 1] x [0, H - 1]; taps and weights are K21's for that position under `quant`, the blend is
 *     K12's v00 w0 + v01 w1 + v10 w2 + v11 w3.  After the clamp only a tap at column W or row H can lie outside the frame:
 *     it counts as +0.0f, K21's rule, and its weight is 0.
 * Tree sum over a patch: the PP values in row-major patch order, added pairwise x[2i] + x[2i + 1], level by level,
 *     log2(PP) levels.  Float addition is commutative, so an xor butterfly across lanes gives these bits in every lane.
 * Per patch with origin (ox, oy), pixels q of the patch:
 *     u0   = the vector of `flow` at (ox + P / 2, oy + P / 2) if fmask is set there and both components are finite, else
 *            (+0.0f, +0.0f)
 *     T    = normalise ? A - (sum A) * (1 / PP) : A
 *     H11  = sum gx * gx,  H12 = sum gx * gy,  H22 = sum gy * gy,  det = H11 * H22 - H12 * H12
 *     r(u) = (normalise ? S(q, u) - (sum S) * (1 / PP) : S(q, u)) - T,   ssd(u) = sum r * r
 *     best = ssd(u0), +Inf if that is not finite;  ubest = u = u0
 *     if det is finite and > 0, `iterations` times:
 *         b1 = sum r * gx,  b2 = sum r * gy;   du = (H22 * b1 - H12 * b2) / det,  dv = (H11 * b2 - H12 * b1) / det
 *         u' = (u.x - du, u.y - dv);  e = u' - u0
 *         stop if a component of u' is not finite or e.x * e.x + e.y * e.y > PP
 *         u <- u';  r and ssd at u;  if ssd < best (a NaN never wins): best <- ssd, ubest <- u
 *     patch_vecs = ubest,  patch_ssd = best
 *   A flat or NaN-ridden patch therefore returns u0 bit for bit, and ubest never lies farther than P from u0.
 * Densify, per pixel q, the patches p that contain q in row-major grid order, u_p = patch_vecs(p):
 *     d   = |S(q, u_p) - A(q)|   (raw intensities, as OpenCV takes them);   w_p = 1 / (d < floor ? floor : d): a NaN
 *           difference is a NaN weight
 *     out = ((+0 + w_1 u_1.x + ...) / (+0 + w_1 + ...),  likewise y);  out_mask = both components finite; else the vector
 *           is (+0.0f, +0.0f) and the mask 0.  A NaN poisons only the pixels of the patches it touches.
 *     patch P in {4, 8};  stride S in [1, P];  iterations in [1, 32];  floor finite and > 0 (the Python layer's default 1.0
 *     is meant for intensities 0 ... 255);  H >= P and W >= P
 *     out float32 [N][H][W][2], out_mask uint8 [N][H][W];  patch_vecs float32 [N][ny][nx][2], patch_ssd float32 [N][ny][nx],
 *     each or NULL;  workspace: 8 N H W bytes, plus 12 bytes per patch unless both patch buffers are given;
 *     ofl_inverse_search_workspace_bytes returns the larger figure.  8-byte aligned, caller-provided.
 * Three launches: setup (one thread per pixel), search (one wave per 8 x 8 patch, four 4 x 4 patches a wave; the sums cross
 * lanes, no LDS, 12 bytes written per patch), densify (one thread per pixel); no atomics, 64-bit offsets across items.
 * near / far aligned to their element, flow, out, patch_vecs and the workspace 8-byte, patch_ssd 4-byte.  The outputs and
 * the workspace must not overlap each other or an input.  A bad argument -- a NULL near / far / out / out_mask, another
 * elem, layout or quant, C > 4, sizes out of range, sign not +-1, a parameter out of its range or not finite, an overlap,
 * a misaligned pointer, a short workspace -- returns OFL_E_INVALID with a message before any launch.  The _dev entry is
 * asynchronous; the host entry takes host pointers, uploads, launches, downloads and synchronises.
 * Not built: OpenCV's spatial propagation between neighbouring patches and its early exits, patches of 12 / 16 px,
 * per-channel residuals and C > 4, near_mask / far_mask, affine patch models, a pyramid or a fused multi-level launch (the
 * Python layer's estimate_flow loops over halved levels), a backward pass.
 */
enum { OFL_ISEARCH_MAX_C = 4, OFL_ISEARCH_MAX_ITER = 32 };
int ofl_inverse_search_workspace_bytes(int N, int H, int W, int patch, int stride, size_t *bytes);
int ofl_inverse_search_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                           const float *flow, const uint8_t *fmask, int sign, int patch, int stride, int iterations,
                           int normalise, float floor, void *workspace, size_t workspace_bytes,
                           float *out, uint8_t *out_mask, float *patch_vecs, float *patch_ssd, int quant, void *stream);
int ofl_inverse_search(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                       const float *flow, const uint8_t *fmask, int sign, int patch, int stride, int iterations,
                       int normalise, float floor, float *out, uint8_t *out_mask, float *patch_vecs, float *patch_ssd, int quant);

/* ------------------------------------------------------------------ K25: a sequence of fields accumulated into one
 * Chains the consecutive flows of a video into one long-range field: what a host loop of L - 1 Flow.combine_with(mode=3)
 * calls (flow_class.py:1412-1422) computes, in ONE launch, with the accumulated vector in registers, no intermediate
 * field and no read-back.  A sequence is L fields of one shape and ONE reference, field k mapping frame k to frame k + 1;
 * sign = +1 for 's', which walks k = 0, 1, ..., L - 1, and -1 for 't', which walks k = L - 1, ..., 0.  Per pixel (x, y), with
 * k0 the first field of the walk, every operation float32 and rounded once:
 *     acc = f_k0[y][x];  m = mask_k0[y][x]
 *     for every later k of the walk:
 *         tap = the bilinear tap of (x, y) + sign * acc                 (map_coord / make_tap, `quant` as in K1 / K2)
 *         s   = f_k's four taps blended (0 outside the frame);  am = mask_k's four taps blended as 0.0f / 1.0f
 *         m   = m & (am == 1.0f)
 *         acc = (acc.u + s.u, acc.v + s.v)
 * This is ofl_compose3_dev with fb = acc and fa = f_k, folded over the sequence, bit for bit, vectors and masks:
 *     's':  F <- F.combine_with(f_k, 3)  for k = 1 ... L - 1
 *     't':  G <- f_k.combine_with(G, 3)  for k = L - 2 ... 0
 * For 't' this right fold is the only association that is a per-pixel walk.  The left fold, ((f_0 (+) f_1) (+) f_2) ...,
 * interpolates the accumulated field and is NOT what this entry computes.  There is NO zero-flow short cut in either `quant`
 * mode (as in K13: the reference's early exits are a host decision) and no early exit that changes a value.  The non-finite
 * rules above (K1 / K2 / K12 / K13) hold: a non-finite accumulated vector samples nothing, the pixel is invalid from that
 * step on.  L = 1 copies the field.
 *     flows   float32 [S][L][H][W][2], masks uint8 [S][L][H][W]: S sequences of L fields each, back to back
 *     out     float32 [S][H][W][2],    mout  uint8 [S][H][W]: required
 *     part_vecs float32 [S][L][H][W][2] and part_masks uint8 [S][L][H][W], both or neither (NULL): the accumulated field
 *             after each step, stored at the batch index of the field taken last -- for 's' entry k is the composition of
 *             fields 0 ... k and entry L - 1 the result, for 't' entry k is the composition of fields k ... L - 1 and entry
 *             0 the result; the entry at k0 is that field itself
 *     lost_at int32 [S][H][W] or NULL: the batch index k of the field at which the pixel's mask first became 0 -- k0 for a
 *             pixel whose own mask in the first-walked field is unset --, -1 for a pixel still valid at the end
 * An output that is NULL is not written.  H and W in [1, 32766], L >= 1, S in [1, 65535] (the grid's z).  flows, out and
 * part_vecs must be 8-byte, lost_at 4-byte aligned; the outputs must not overlap the inputs or each other.
 * One launch: one lane per pixel, L - 1 dependent gathers, every tap its own guarded 8-byte and 1-byte load; no LDS, no
 * atomics, no workspace, 64-bit offsets across fields.  Bytes per pixel: reads 9 L; writes 9, + 9 L with the partial
 * results, + 4 with lost_at -- where the chain of L - 1 ofl_compose3_dev launches reads 18 (L - 1) and writes 9 (L - 1).
 * A bad argument -- a NULL flows / masks / out / mout, sizes, L or S out of range, sign not +-1, an unknown quant, one
 * partial buffer without the other, an overlap, a misaligned pointer -- returns OFL_E_INVALID with a message before any
 * launch.  The _dev entry is asynchronous; the host entry takes host pointers, uploads, launches once, downloads and
 * synchronises.
 * Not built: a tiled / LDS path for the first, most coherent steps, modes 1 and 2, sequences of mixed reference, the left
 * fold for 't', re-anchoring or filling lost pixels inside the call (ofl_fill_dev does that afterwards), packed masks, a
 * backward pass.
 */
int ofl_compose_sequence_dev(const float *flows, const uint8_t *masks, int sign, int H, int W, int L, int S,
                             float *out, uint8_t *mout, float *part_vecs, uint8_t *part_masks, int32_t *lost_at,
                             int quant, void *stream);
int ofl_compose_sequence(const float *flows, const uint8_t *masks, int sign, int H, int W, int L, int S,
                         float *out, uint8_t *mout, float *part_vecs, uint8_t *part_masks, int32_t *lost_at, int quant);

/* ------------------------------------------------------------------ K26: structural similarity of a warp over a window
 * K21 compares raw values and K22 their order.  The third standard term compares the local mean, variance and covariance of
 * the intensities in a weighted K x K window around the pixel, in `near` and in the warped `far`: Wang et al.'s SSIM -- with
 * an 11 x 11 Gaussian window the number quoted for the quality of a warp where there is no ground truth -- and, with a
 * uniform window, the avg_pool2d form in the photometric loss of UnFlow / DDFlow / ARFlow / UFlow / SMURF.  The output is the
 * DISSIMILARITY (1 - SSIM) / 2 in [0, 1]; SSIM itself is 1 - 2 err.  One fused launch: the warped image is never written.
 *     near, far, elem, layout, N, C, H, W, flow, fmask, flow_shared, sign, near_mask, far_mask, quant: K22's (C in [1, 4])
 *     window    K in {3, 5, 7, 11}, r = K / 2
 *     taps      a HOST pointer to K float32 values, in both entries: the 1-D window g[0 ... K-1], read during the call and
 *               passed to the kernel by value; every tap finite and > 0.  The 2-D window is g[dx + r] * g[dy + r]
 *     c1, c2    float32, finite and > 0: Wang's (k1 L)^2 and (k2 L)^2
 *     min_count in [1, K * K]: the members a window needs -- the centre IS a member of its own window, unlike K22
 *     tau       as in K21
 * Per item n and pixel q, every operation float32 and rounded once (no FMA; the divisions correctly rounded):
 *     tap(q), w_c(q), am(q), cov1(q), A(q), B(q)        K22's, unchanged
 *     member(q) = q inside the frame & cov1(q)
 *     for every row dy = -r ... r and dx = -r ... r of the window of p (the centre included), q = p + (dx, dy):
 *         ga = g[dx+r] * A(q);   gb = g[dx+r] * B(q)
 *         the six terms  g[dx+r],  ga,  gb,  ga * A(q),  gb * B(q),  ga * B(q)
 *         each term is REPLACED by +0.0f where !member(q)            (a select, not a product: a NaN there does not leak)
 *         R^k_dy = the row sum of term k, ascending dx, from +0.0f                          k = 0 ... 5
 *     S^k = g[-r+r] * R^k_(-r) + ... + g[r+r] * R^k_r, one product and one addition a row, ascending dy, from +0.0f
 *     (Wt, Sa, Sb, Saa, Sbb, Sab) = S^0 ... S^5;   n = the number of members (an integer)
 *     mu_a = Sa / Wt;  mu_b = Sb / Wt
 *     va  = Saa / Wt - mu_a * mu_a;   vb = Sbb / Wt - mu_b * mu_b;   vab = Sab / Wt - mu_a * mu_b
 *     num = (2 * (mu_a * mu_b) + c1) * (2 * vab + c2)
 *     den = ((mu_a * mu_a + mu_b * mu_b) + c1) * ((va + vb) + c2)
 *     s = num / den;   e = (1 - s) * 0.5;   e = e < 0 ? 0 : (e > 1 ? 1 : e)          (a NaN stays a NaN)
 *     covered(p) = cov1(p) & (n >= min_count);  err = covered ? e : 0.0f;  within = covered & (e <= tau)
 * These are population moments -- Wang et al. with a Gaussian window, the avg_pool2d form with a uniform one --, and the
 * intensity is the channel mean, as in K22 ... K24.  The definition is separable on purpose: the six row sums of a tile row
 * do not depend on the centre, so the centres a thread owns share them, and a window of ones gives Wt == n exactly.  The raw
 * second moments are on purpose too: centring on the centre pixel would cut the cancellation in Saa / Wt - mu_a^2 but end
 * the sharing; in float32 they cost 1e-5 to 1e-4 of e against float64 at intensities 0 ... 255 (tests/ssim_ref.py derives the
 * bound and restates all of this in NumPy).  There is NO zero-flow short cut.
 *     err, covered, within, counts: K21's ([N][H][W]; one of err / within required; counts uint32[N][2] ADDED to, at most one
 *     integer atomic add per workgroup and counter; no other atomics, no workspace).
 * Alignment, 64-bit offsets, aliasing and the two entries (asynchronous _dev, host-staged) as in K21.  A bad argument -- those
 * of K21, C > 4, another window, a NULL taps, a tap, c1 or c2 not finite or not positive, min_count outside [1, K * K], tau
 * (when within is given) negative or not finite -- returns OFL_E_INVALID with a message before any launch.
 * Not built: C > 4 and a per-channel SSIM, luma weights (pass a reduced plane), sample (N - 1) moments, other or non-square
 * windows, MS-SSIM, the three components as outputs, gradient constancy, a reduction of the map, PSNR, a backward pass,
 * mixed element types or layouts, integer tensors on the device.
 */
enum { OFL_SSIM_MAX_C = 4 };
int ofl_ssim_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                 const float *flow, const uint8_t *fmask, int flow_shared, int sign,
                 const uint8_t *near_mask, const uint8_t *far_mask,
                 int window, const float *taps, float c1, float c2, int min_count, float tau,
                 float *err, uint8_t *covered, uint8_t *within, uint32_t *counts, int quant, void *stream);
int ofl_ssim(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
             const float *flow, const uint8_t *fmask, int flow_shared, int sign,
             const uint8_t *near_mask, const uint8_t *far_mask,
             int window, const float *taps, float c1, float c2, int min_count, float tau,
             float *err, uint8_t *covered, uint8_t *within, uint32_t *counts_host, int quant);

/* ------------------------------------------------------------------ C1: the exchange steps (RCCL)
 * Two exchange steps exist in the sharded workload: one broadcast of a shared source image / flow from rank `root`
 * to all ranks over xGMI, and -- for one huge field warped with ref 's' in slab mode (above) -- one all-gather of the
 * ranks' lists of unfinished sites (`bytes` from every rank into recv[rank * bytes ...], send may alias its own slot).
 * The 128-byte unique id is created on rank 0 with ofl_comm_unique_id and distributed by the launcher
 * (torch.distributed store / gloo).
 */
int ofl_comm_unique_id(void *id128);
int ofl_comm_init(const void *id128, int rank, int world);
int ofl_comm_broadcast(void *dptr, size_t bytes, int root, void *stream);
int ofl_comm_allgather(const void *send, void *recv, size_t bytes, void *stream);
int ofl_comm_size(int *world);              /* ranks of the live communicator (ncclCommCount), 0 without one */
int ofl_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* OFL_H */
