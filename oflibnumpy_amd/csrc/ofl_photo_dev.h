// ofl_photo_dev.h -- what the image-pair families K21 (ofl_photometric.hip), K22 (ofl_census.hip), K23 (ofl_refine.hip), K24
// (ofl_inverse_search.hip) and K26 (ofl_ssim.hip) share.  Host: PairArgs, the kernel arguments that describe the two tensors and
// the field, with their checks (check_pair_args, check_pair_alignment) and pair_fill, which sets them; for the error-map entries
// K21, K22 and K26 -- err, covered, within, counts and a tau -- the two halves of their checks, error_map_fill (the `_dev` form)
// and error_map_host (the host form).  Device: the frame test of a tap, the `covered` rule of a pixel, finite32, the channel
// mean of a pixel (K24), the warp of a tile plus halo into LDS (K22, K23, K26) with its tile and window_grid, the counts of a
// workgroup, error_store (the stores of one pixel) and window_finish (the epilogue of K22 and K26).  A family keeps the checks
// of its settings and workspace and its launches (DESIGN "Image-pair families").
#pragma once
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_host_stage.h"

namespace ofl {

// ----------------------------------------------------------------------------- host side
// the arguments every kernel of the four families takes: the Args of stage_warped_tile.  K23's and K24's structs derive from
// it.  K21's and K22's declare the same members by name in an order of their own, their outputs between the pointers and the
// sizes: where a member lies in the kernel-argument segment changes the code of their kernels -- derived, with the outputs
// behind, census_kernel<..., 7, hard> ran 7 - 10 % and photo_nchw_kernel<..., 0> at C = 128 42 % longer (profiles/r24_pair_fold_ab.txt).
struct PairArgs {
    const void    *near, *far;
    const float   *flow;
    const uint8_t *fmask, *near_mask, *far_mask;
    int            N, C, H, W, sign;
    float          inv_c;
    size_t         step;            // pixels from one item's field and masks to the next (0: shared)
    size_t         s_px, s_ch;      // elements from a pixel to the next and from a channel to the next
};

// the checks of the arguments the four families share, C against the family's limit `max_c`
inline int check_pair_args(const char *who, int elem, int layout, int N, int C, int max_c, int H, int W, int sign, int quant)
{
    if (elem != OFL_EL_F16 && elem != OFL_EL_BF16 && elem != OFL_EL_F32)
        return fail(OFL_E_INVALID, "%s: elem must be OFL_EL_F16, OFL_EL_BF16 or OFL_EL_F32, got %d", who, elem);
    if (layout != OFL_TENSOR_NCHW && layout != OFL_TENSOR_NHWC) return fail(OFL_E_INVALID, "%s: bad layout %d", who, layout);
    if (N < 1 || N > 65535) return fail(OFL_E_INVALID, "%s: N must be in [1, 65535], got %d", who, N);
    if (C < 1 || C > max_c) return fail(OFL_E_INVALID, "%s: C must be in [1, %d], got %d", who, max_c, C);
    OFL_TRY(check_field_dims(who, H, W));
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "%s: sign must be +1 or -1", who);
    if (quant != OFL_QUANT_OPENCV && quant != OFL_QUANT_EXACT) return fail(OFL_E_INVALID, "%s: bad quant", who);
    return OFL_OK;
}

// the device pointers `near` and `far` on a boundary of their element
inline int check_pair_alignment(const char *who, const void *near, const void *far, int elem)
{
    const unsigned eb = elem == OFL_EL_F32 ? 4 : 2;
    if (!host_aligned(near, eb) || !host_aligned(far, eb)) return fail(OFL_E_INVALID, "%s: near and far must be aligned to the element size", who);
    return OFL_OK;
}

// checked arguments -> the members of PairArgs (Args: PairArgs, a struct derived from it or one with the same members); both
// layouts become a pixel stride and a channel stride
template <class Args>
inline void pair_fill(Args &a, const void *near, const void *far, int layout, int N, int C, int H, int W,
                      const float *flow, const uint8_t *fmask, bool flow_shared, int sign,
                      const uint8_t *near_mask, const uint8_t *far_mask)
{
    a.near = near; a.far = far; a.flow = flow; a.fmask = fmask; a.near_mask = near_mask; a.far_mask = far_mask;
    a.N = N; a.C = C; a.H = H; a.W = W; a.sign = sign;
    a.inv_c = (float)(1.0 / (double)C);
    a.step = flow_shared ? 0 : (size_t)H * W;
    a.s_px = layout == OFL_TENSOR_NCHW ? 1 : (size_t)C;
    a.s_ch = layout == OFL_TENSOR_NCHW ? (size_t)H * W : 1;
}

// ----------------------------------------------------------------------------- host side: the error-map entries K21, K22, K26
// their checks come in one order: check_error_map_inputs -- the required pointers, then the shared arguments --, the family's
// own settings, check_error_map_outputs -- err / within, then tau
inline int check_error_map_inputs(const char *who, const void *near, const void *far, const void *flow, const void *fmask,
                                  int elem, int layout, int N, int C, int max_c, int H, int W, int sign, int quant)
{
    if (!near || !far || !flow || !fmask) return fail(OFL_E_INVALID, "%s: NULL pointer (near, far, flow and fmask are required)", who);
    return check_pair_args(who, elem, layout, N, C, max_c, H, W, sign, quant);
}

inline int check_error_map_outputs(const char *who, const void *err, const void *within, float tau)
{
    if (!err && !within) return fail(OFL_E_INVALID, "%s: one of err and within is required", who);
    if (within && !finite_not_negative(tau)) return fail(OFL_E_INVALID, "%s: tau must be finite and not negative (got %g)", who, (double)tau);
    return OFL_OK;
}

// the `_dev` form, arguments checked: the device pointers on their boundaries -- near and far by element, the float2 field,
// the 4-byte outputs --, then pair_fill and, next to it, the outputs and tau of PArgs, CArgs and SArgs
template <class Args>
inline int error_map_fill(const char *who, Args &a, const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                          const float *flow, const uint8_t *fmask, bool flow_shared, int sign, const uint8_t *near_mask,
                          const uint8_t *far_mask, float *err, uint8_t *covered, uint8_t *within, uint32_t *counts, float tau)
{
    OFL_TRY(check_pair_alignment(who, near, far, elem));
    if (!host_aligned(flow, 8)) return fail(OFL_E_INVALID, "%s: flow must be 8-byte aligned", who);
    if (!host_aligned(err, 4) || !host_aligned(counts, 4)) return fail(OFL_E_INVALID, "%s: err and counts must be 4-byte aligned", who);
    pair_fill(a, near, far, layout, N, C, H, W, flow, fmask, flow_shared, sign, near_mask, far_mask);
    a.err = err; a.covered = covered; a.within = within; a.counts = counts; a.tau = tau;
    return OFL_OK;
}

// the host form of an error-map entry, arguments checked: upload, `dev`, the family's `_dev` entry, on the copies (NULL where
// the host pointer was) with the family's `settings` in their place, tau last among them, download
template <class Dev, class... Settings>
inline int error_map_host(const char *who, Dev dev, const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                          const float *flow, const uint8_t *fmask, int flow_shared, int sign, const uint8_t *near_mask,
                          const uint8_t *far_mask, float *err, uint8_t *covered, uint8_t *within, uint32_t *counts_host, int quant,
                          Settings... settings)
{
    const size_t hw = (size_t)H * W, n = (size_t)N * hw, nf = flow_shared ? hw : n;
    const size_t bytes = n * C * (elem == OFL_EL_F32 ? 4 : 2);
    HostStage st(who);
    auto dn = st.in(near, bytes), df = st.in(far, bytes);
    auto dfl = st.in(flow, nf * 2);
    auto dfm = st.in(fmask, nf), dnm = st.in(near_mask, nf), dam = st.in(far_mask, nf);
    auto de = st.out(err, n);
    auto dc = st.out(covered, n), dw = st.out(within, n);
    auto cnt = st.out(counts_host, (size_t)N * 2, true);          // the launch adds to the counts
    OFL_TRY(st.upload());
    OFL_TRY(dev(dn, df, elem, layout, N, C, H, W, dfl, dfm, flow_shared, sign, dnm, dam, settings..., de, dc, dw, cnt, quant, st.stream()));
    return st.download();
}

// ----------------------------------------------------------------------------- device side
__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the four in-frame flags and in-plane offsets of a tap (inside one plane: H * W < 2^31)
__device__ __forceinline__ void tap_frame(const Tap &tp, int H, int W, bool (&in)[4], int (&off)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = tp.iy + (k >> 1), xx = tp.ix + (k & 1);
        in[k]  = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        off[k] = in[k] ? yy * W + xx : 0;
    }
}

// K12's `valid` ANDed with near_mask; the masks are those of this pixel's field (near_mask, far_mask may be NULL)
__device__ __forceinline__ bool photo_covered(const uint8_t *fmask, const uint8_t *near_mask, const uint8_t *far_mask,
                                              size_t field, size_t pix, const Tap &tp, const bool (&in)[4], const int (&off)[4])
{
    const uint8_t *fm = far_mask ? far_mask + field : nullptr;
    float m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = in[k] ? ((fm ? fm[off[k]] != 0 : true) ? 1.0f : 0.0f) : 0.0f;
    bool cov = (blend4(m[0], m[1], m[2], m[3], tp) == 1.0f) & (fmask[field + pix] != 0);
    if (near_mask) cov &= near_mask[field + pix] != 0;
    return cov;
}

// K22's channel mean of ONE unwarped pixel, for K24's planes: the C values (1 ... 4) of pixel `pix` of the item whose element 0
// is `base`, added in ascending c from +0.0f, times inv_c -- the A of stage_warped_tile below
template <int E>
__device__ __forceinline__ float channel_mean(const void *tensor, size_t base, size_t pix, size_t s_px, size_t s_ch, int C, float inv_c)
{
    typedef typename Elem<E>::T T;
    const T *p = static_cast<const T *>(tensor) + base + pix * s_px;
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c >= C) break;                                              // uniform
        m = __fadd_rn(m, Elem<E>::to_f32(p[(size_t)c * s_ch]));
    }
    return __fmul_rn(m, inv_c);
}

// K22's and K23's staging: one workgroup of 256 threads warps the TX x TY tile at (x0, y0) of item n and its halo of R pixels
// into LDS -- entry i = ty * (TX + 2 R) + tx holds the pixel (x0 - R + tx, y0 - R + ty): A, the channel mean of `near`, B, that
// of the warped `far` (sums from +0.0f in ascending c, times inv_c), and member = inside the frame & K21's covered; outside
// the frame 0, 0 and 0.  The entries are dealt to the threads; a thread first loads the flow vectors of all its pixels, then
// per pixel makes the tap and issues the C `near`, 4 C `far` and the mask loads together (unconditional, as in K21: a tap
// outside the frame reads element 0 and is replaced by 0.0f).  Both layouts go through ONE code path, as a pixel stride and
// a channel stride; the element type and `quant` are template arguments and end here.  The caller synchronises.
// Args: PairArgs, a struct derived from it or one with the same members, with C in 1 ... 4.  K22 and K23 instantiate it on the tile below.
constexpr int kTX = 64, kTY = 16;       // the tile
constexpr int kRows = 4;                // rows of a column one thread owns after the staging: 4 waves x 4 rows

// the grid of a kernel instantiated on that tile: one workgroup a tile, the items along z
inline dim3 window_grid(int N, int H, int W) { return dim3((unsigned)((W + kTX - 1) / kTX), (unsigned)((H + kTY - 1) / kTY), (unsigned)N); }

template <int E, int QUANT, int R, int TX, int TY, class Args>
__device__ __forceinline__ void stage_warped_tile(const Args &a, int n, int x0, int y0, float *s_a, float *s_b, uint8_t *s_m)
{
    typedef typename Elem<E>::T T;
    constexpr int TW = TX + 2 * R, TH = TY + 2 * R, NE = TW * TH, NIT = (NE + 255) / 256;
    const int H = a.H, W = a.W, C = a.C;
    const size_t hw = (size_t)H * W, field = a.step * n;
    const float *flow = a.flow + 2 * field;
    float2 f[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {                  // entry i of the tile; the flow of pixel 0 where there is no pixel
        const int i = threadIdx.x + 256 * it, ty = i / TW, tx = i - ty * TW, x = x0 - R + tx, y = y0 - R + ty;
        const bool inside = i < NE && (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
        f[it] = *reinterpret_cast<const float2 *>(flow + 2 * (inside ? (size_t)y * W + x : (size_t)0));
    }
    const T *fp = static_cast<const T *>(a.far) + (size_t)n * C * hw;        // element 0 of item n
    const T *np = static_cast<const T *>(a.near) + (size_t)n * C * hw;
    const size_t s_px = a.s_px, s_ch = a.s_ch;
    const float inv_c = a.inv_c;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int i = threadIdx.x + 256 * it, ty = i / TW, tx = i - ty * TW, x = x0 - R + tx, y = y0 - R + ty;
        if (i >= NE) break;
        float A = 0.0f, B = 0.0f;
        bool member = false;
        if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) {
            const size_t pix = (size_t)y * W + x;
            const Tap tp = make_tap<QUANT>(map_coord(x, f[it].x, a.sign), map_coord(y, f[it].y, a.sign));
            bool in[4];
            int  off[4];
            tap_frame(tp, H, W, in, off);
            member = photo_covered(a.fmask, a.near_mask, a.far_mask, field, pix, tp, in, off);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c >= C) break;                                      // uniform
                const T *s = fp + (size_t)c * s_ch;
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float t = Elem<E>::to_f32(s[(size_t)off[k] * s_px]);
                    v[k] = in[k] ? t : 0.0f;
                }
                A = __fadd_rn(A, Elem<E>::to_f32(np[pix * s_px + (size_t)c * s_ch]));
                B = __fadd_rn(B, blend4(v[0], v[1], v[2], v[3], tp));
            }
            A = __fmul_rn(A, inv_c);
            B = __fmul_rn(B, inv_c);
        }
        s_a[i] = A;
        s_b[i] = B;
        s_m[i] = member ? 1 : 0;
    }
}

// the covered and within pixels of this wave (n_cov, n_wi: wave-uniform) -> the block's two counts -> at most one atomicAdd
// per counter; every thread of a block of 4 waves calls this
__device__ __forceinline__ void photo_count(uint32_t *counts, int n, uint32_t n_cov, uint32_t n_wi)
{
    __shared__ uint32_t s_n[4][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { s_n[wave][0] = n_cov; s_n[wave][1] = n_wi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t c0 = s_n[0][0] + s_n[1][0] + s_n[2][0] + s_n[3][0], c1 = s_n[0][1] + s_n[1][1] + s_n[2][1] + s_n[3][1];
        if (c0) atomicAdd(counts + 2 * (size_t)n, c0);
        if (c1) atomicAdd(counts + 2 * (size_t)n + 1, c1);
    }
}

// the three optional stores of ONE pixel of an error map (Args: PArgs, CArgs, SArgs) at element `at`: err = covered ? e : 0.0f,
// covered, within = covered & (e <= tau) -- false for a NaN -- -> within, for the counts
template <class Args>
__device__ __forceinline__ bool error_store(const Args &a, size_t at, float e, bool cov)
{
    const bool wi = a.within != nullptr && cov && e <= a.tau;
    if (a.err) a.err[at] = cov ? e : 0.0f;
    if (a.covered) a.covered[at] = cov ? 1 : 0;
    if (a.within) a.within[at] = wi ? 1 : 0;
    return wi;
}

// the epilogue of a window kernel (K22, K26), called by every thread: it owns the kRows rows from y0 + kRows * wave of column
// x0 + lane of item n; per row cm, the centre's member flag, cnt, the members of its window, and e, computed covered or not.
// covered = inside the frame & cm & (cnt >= min_count); error_store; the wave's two ballots a row; photo_count.
template <class Args>
__device__ __forceinline__ void window_finish(const Args &a, int n, int x0, int y0, const bool (&cm)[kRows], const int (&cnt)[kRows],
                                              const float (&e)[kRows])
{
    const int top = kRows * (threadIdx.x >> 6), x = x0 + (threadIdx.x & 63);
    const size_t hw = (size_t)a.H * a.W;
    uint32_t n_cov = 0, n_wi = 0;
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int y = y0 + top + j;
        const bool act = x < a.W && y < a.H;
        const bool cov = act && cm[j] && cnt[j] >= a.min_count;
        const bool wi = act && error_store(a, (size_t)n * hw + (size_t)y * a.W + x, e[j], cov);      // no store outside the frame
        n_cov += (uint32_t)__popcll(__ballot(cov));
        n_wi += (uint32_t)__popcll(__ballot(wi));
    }
    if (a.counts) photo_count(a.counts, n, n_cov, n_wi);
}

}  // namespace ofl
