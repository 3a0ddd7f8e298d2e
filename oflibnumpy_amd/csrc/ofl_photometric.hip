// ofl_photometric.hip -- K21: brightness- / feature-constancy error of a warp (gfx950).
//
// The tensor analogue of K13: `far`, the tensor of the other frame, is sampled where the field points (K12's / K13's taps
// and blend) and compared, channel by channel, with `near`, the tensor of the field's own frame; the C differences are
// reduced to ONE float per pixel.  Per item n and pixel (x, y), every operation float32 and rounded once:
//     tap      = make_tap<quant>(map_coord(x, f.u, sign), map_coord(y, f.v, sign))
//     w_c      = blend4 of far[n, c]'s four taps (0 outside the frame)            -- K12's value before its rounding to storage
//     am       = blend4 of far_mask's four taps as 0.0f / 1.0f (NULL: 1 inside the frame, 0 outside)
//     covered  = f.mask & near_mask (NULL: 1) & (am == 1.0f)
//     d_c      = near[n, c] - w_c
//     t_c      = |d_c| (L1)  |  d_c * d_c (L2)  |  sqrtf(d_c * d_c + eps * eps) (CHARBONNIER)
//     S        = sum of t_c in the order below;  e = S * inv_c;  L2: e = sqrtf(e)
//     err      = covered ? e : 0.0f;  within = covered & (e <= tau)
// There is no zero-flow short cut.  16-bit elements are widened exactly.
//
// The order of the sum depends on C alone (K18's scheme): the groups of 4 consecutive channels g = c / 4 are dealt to 16
// partial sums, p_j = the t_c with (c / 4) % 16 == j added in ascending c to +0.0f, and the partial sums are folded by
// p_j += p_(j + 8) for j < 8, then p_j += p_(j + 4), p_j += p_(j + 2), p_0 += p_1.  Every t_c is >= +0 or NaN, so a partial
// sum without channels stays +0.0f and adding it is exact: the fold may start at any width that holds all groups.
//
// Two mappings, as K12 has, because no single one keeps both layouts contiguous per wave-instruction:
//   NCHW  lanes run along x; a block of 4 waves covers 4 rows x 64 columns of one item and owns ALL C channels of its
//         pixels (the reduction never crosses a block).  Taps and the 16 partial sums live in registers over the channel
//         loop, which is unrolled over the 64 channels of one round of the deal so that every partial sum has a constant index.
//         Tap loads are unconditional (a tap outside the frame reads element 0 of its plane and is replaced by 0.0f), so
//         the loads of a round are issued together: 0.37 ms against 1.12 ms at C = 128 float16, 270 x 480 x 8.  C = 1 ... 4
//         takes a variant with the count as a template constant: one partial sum, all 5 C loads of a pixel in flight, 25 to
//         32 VGPRs -- 0.55 ms against 0.99 ms in the general kernel at C = 3 float32, 2160 x 3840 x 8.
//   NHWC  lanes run along the channels of a pixel: G = min(16, the power of two >= ceil(C / 4)) lanes own a pixel, lane j the
//         groups j, j + 16, ... as ONE partial sum, and the fold is __shfl_xor over G / 2 ... 1.  C <= 4 (grey, RGB, RGBA)
//         is G = 1: 64 pixels per wave, no lane idle.  With C % 4 == 0 and aligned tensors a group is one 16-byte (float32)
//         or 8-byte (16-bit) load per lane; otherwise its channels are loaded one by one.  The G lanes of a pixel compute the
//         same tap: a few dozen ALU operations, against an LDS round trip and a barrier.
// Reads what K12 reads plus `near`; writes 4 (err) + 1 (covered) + 1 (within) bytes per pixel, each optional.  With counts
// the block reduces its two counts through ballot + popcount and four LDS words per counter and one lane issues at most one
// atomicAdd per counter (integer adds: their order cannot change the result); these are the only atomics.  Every element
// offset is 64-bit.  No workspace.  A variant with two pixels per lane was not built: no figure, no variant.
//
// Shared (ofl_photo_dev.h): PairArgs with its checks, tap_frame, photo_covered, photo_count; with K22 and K26 the entries' frame and error_store.
//
// OUT OF SCOPE: window metrics (SSIM, gradient constancy; the census distance is K22, ofl_census.hip), a reduction of the
// map, a backward pass, mixed element types or layouts, integer tensors, padding offsets.
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_photo_dev.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

constexpr int kV = 4;       // consecutive channels per group
constexpr int kL = 16;      // partial sums

struct PArgs {                      // PairArgs' members by name, in the order the kernels were measured with (ofl_photo_dev.h)
    const void    *near, *far;
    const float   *flow;
    const uint8_t *fmask, *near_mask, *far_mask;
    float         *err;
    uint8_t       *covered, *within;
    uint32_t      *counts;
    int            N, C, H, W, sign, metric;
    float          eps2, tau, inv_c;
    size_t         step;
    size_t         s_px, s_ch;      // pair_fill's; K21's two mappings index their layout themselves
};

// one channel's term from the difference d
__device__ __forceinline__ float photo_term(float d, int metric, float eps2)
{
    if (metric == OFL_PHOTO_L1) return fabsf(d);
    const float q = __fmul_rn(d, d);
    return metric == OFL_PHOTO_L2 ? q : sqrtf(__fadd_rn(q, eps2));
}

// the sum S -> the stores of one pixel; -> (covered, within) for the counts
__device__ __forceinline__ void photo_finish(const PArgs &a, size_t at, float S, bool cov, bool &wi)
{
    float e = __fmul_rn(S, a.inv_c);
    if (a.metric == OFL_PHOTO_L2) e = sqrtf(e);
    wi = error_store(a, at, e, cov);                     // ofl_photo_dev.h
}

// ---------------------------------------------------------------------------------------------- planar
// CN: the channel count where it is 1 to 4 -- grey, flow-like, RGB, RGBA: ONE group, so one partial sum, every load of a pixel
// issued at once and few registers -- or 0 for any count
template <int E, int QUANT, int CN>
__global__ __launch_bounds__(256)
void photo_nchw_kernel(const PArgs a)
{
    typedef typename Elem<E>::T T;
    const int H = a.H, W = a.W, C = CN ? CN : a.C;
    const int n = blockIdx.z;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6), x = blockIdx.x * 64 + (threadIdx.x & 63);
    const bool act = y < H && x < W;
    const size_t hw = (size_t)H * W, field = a.step * n;
    bool cov = false, wi = false;

    if (act) {
        const size_t pix = (size_t)y * W + x;
        const float2 f = *reinterpret_cast<const float2 *>(a.flow + 2 * (field + pix));
        const Tap tp = make_tap<QUANT>(map_coord(x, f.x, a.sign), map_coord(y, f.y, a.sign));
        bool in[4];
        int  off[4];
        tap_frame(tp, H, W, in, off);
        cov = photo_covered(a.fmask, a.near_mask, a.far_mask, field, pix, tp, in, off);

        const T *fp = static_cast<const T *>(a.far) + (size_t)n * C * hw;       // plane 0 of item n
        const T *np = static_cast<const T *>(a.near) + (size_t)n * C * hw + pix;
        const int metric = a.metric;
        const float eps2 = a.eps2;
        // every load is unconditional -- a tap outside the frame reads element 0 of the plane and is then replaced by 0.0f --
        // so that the loads of a group of channels are issued together, with no branch between them
        auto term = [&](int c) {
            const T *s = fp + (size_t)c * hw;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float t = Elem<E>::to_f32(s[off[k]]);
                v[k] = in[k] ? t : 0.0f;
            }
            const float d = __fsub_rn(Elem<E>::to_f32(np[(size_t)c * hw]), blend4(v[0], v[1], v[2], v[3], tp));
            return photo_term(d, metric, eps2);
        };

        float S = 0.0f;
        if constexpr (CN > 0) {                                       // p_0 alone: the other partial sums are +0.0f, the fold adds nothing
            float t[CN];
#pragma unroll
            for (int v = 0; v < CN; ++v) t[v] = term(v);
#pragma unroll
            for (int v = 0; v < CN; ++v) S = __fadd_rn(S, t[v]);
        } else {
            float p[kL];
#pragma unroll
            for (int j = 0; j < kL; ++j) p[j] = 0.0f;
            int c0 = 0;
            for (; c0 + kV * kL <= C; c0 += kV * kL) {                    // whole rounds of the deal
#pragma unroll
                for (int j = 0; j < kL; ++j)
#pragma unroll
                    for (int v = 0; v < kV; ++v) p[j] = __fadd_rn(p[j], term(c0 + kV * j + v));
            }
#pragma unroll
            for (int j = 0; j < kL; ++j) {                                // the last, partial round: one uniform branch per group
                if (c0 + kV * j >= C) break;
                float t[kV];
#pragma unroll
                for (int v = 0; v < kV; ++v) t[v] = term(min(c0 + kV * j + v, C - 1));         // a missing channel re-reads the last one
#pragma unroll
                for (int v = 0; v < kV; ++v) p[j] = __fadd_rn(p[j], c0 + kV * j + v < C ? t[v] : 0.0f);       // and contributes +0.0f
            }
#pragma unroll
            for (int s = kL / 2; s; s >>= 1)
#pragma unroll
                for (int j = 0; j < s; ++j) p[j] = __fadd_rn(p[j], p[j + s]);
            S = p[0];
        }
        photo_finish(a, (size_t)n * hw + pix, S, cov, wi);
    }
    if (a.counts) photo_count(a.counts, n, (uint32_t)__popcll(__ballot(cov)), (uint32_t)__popcll(__ballot(wi)));
}

// ---------------------------------------------------------------------------------------------- channels-last
// the kV channels from c of one pixel as float32.  WIDE: one load, unconditional -- px is always a pixel of the item, pixel 0
// for a tap outside the frame -- and !ok replaces what it read by 0.0f, so no branch stands between the loads of a group.
// Otherwise channel by channel, 0.0f beyond C: there the guarded load was measured faster (RGB float32 at 4K x 8: 0.70 ms
// against 0.87 ms with a clamped fourth channel).
template <int E, bool WIDE>
__device__ __forceinline__ void load_group(const typename Elem<E>::T *px, int c, int C, bool ok, float (&v)[kV])
{
    typedef typename Elem<E>::T T;
    if constexpr (WIDE && sizeof(T) == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(px + c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if constexpr (WIDE) {
        const uint2 q = *reinterpret_cast<const uint2 *>(px + c);
        v[0] = Elem<E>::to_f32((T)(q.x & 0xffffu)); v[1] = Elem<E>::to_f32((T)(q.x >> 16));
        v[2] = Elem<E>::to_f32((T)(q.y & 0xffffu)); v[3] = Elem<E>::to_f32((T)(q.y >> 16));
    } else {
#pragma unroll
        for (int i = 0; i < kV; ++i) v[i] = ok && c + i < C ? Elem<E>::to_f32(px[c + i]) : 0.0f;
    }
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < kV; ++i) v[i] = ok ? v[i] : 0.0f;
    }
}

// lg: log2 of G, the lanes per pixel
template <int E, int QUANT, bool WIDE>
__global__ __launch_bounds__(256)
void photo_nhwc_kernel(const PArgs a, int lg)
{
    typedef typename Elem<E>::T T;
    const int H = a.H, W = a.W, C = a.C;
    const int n = blockIdx.y, j = threadIdx.x & ((1 << lg) - 1);
    const size_t hw = (size_t)H * W, field = a.step * n;
    const size_t pix = (size_t)blockIdx.x * (256u >> lg) + (threadIdx.x >> lg);
    const bool act = pix < hw;            // the G lanes of a pixel are active together
    bool cov = false;
    float p = 0.0f;

    if (act) {
        const int y = (int)((uint32_t)pix / (uint32_t)W), x = (int)((uint32_t)pix - (uint32_t)y * (uint32_t)W);      // H * W < 2^31
        const float2 f = *reinterpret_cast<const float2 *>(a.flow + 2 * (field + pix));
        const Tap tp = make_tap<QUANT>(map_coord(x, f.x, a.sign), map_coord(y, f.y, a.sign));
        bool in[4];
        int  off[4];
        tap_frame(tp, H, W, in, off);
        cov = photo_covered(a.fmask, a.near_mask, a.far_mask, field, pix, tp, in, off);

        const T *item = static_cast<const T *>(a.far) + (size_t)n * hw * C;
        const T *np = static_cast<const T *>(a.near) + ((size_t)n * hw + pix) * C;
        const T *t0 = item + (size_t)off[0] * C, *t1 = item + (size_t)off[1] * C, *t2 = item + (size_t)off[2] * C, *t3 = item + (size_t)off[3] * C;
        const int metric = a.metric;
        const float eps2 = a.eps2;
        for (int c = kV * j; c < C; c += kV * kL) {                   // this lane's groups, ascending
            float v0[kV], v1[kV], v2[kV], v3[kV], nr[kV];
            load_group<E, WIDE>(np, c, C, true, nr);
            load_group<E, WIDE>(t0, c, C, in[0], v0);
            load_group<E, WIDE>(t1, c, C, in[1], v1);
            load_group<E, WIDE>(t2, c, C, in[2], v2);
            load_group<E, WIDE>(t3, c, C, in[3], v3);
#pragma unroll
            for (int i = 0; i < kV; ++i) {
                const float t = photo_term(__fsub_rn(nr[i], blend4(v0[i], v1[i], v2[i], v3[i], tp)), metric, eps2);
                if (WIDE || c + i < C) p = __fadd_rn(p, t);
            }
        }
    }
    for (int s = (1 << lg) >> 1; s; s >>= 1) p = __fadd_rn(p, __shfl_xor(p, s));      // lanes j < s hold p_j + p_(j + s)
    const bool owner = act && j == 0;
    bool wi = false;
    if (owner) photo_finish(a, (size_t)n * hw + pix, p, cov, wi);
    if (a.counts) photo_count(a.counts, n, (uint32_t)__popcll(__ballot(owner && cov)), (uint32_t)__popcll(__ballot(wi)));
}

int check_photometric_args(const char *who, const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                           const void *flow, const void *fmask, int sign, int metric, float eps, float tau,
                           const void *err, const void *within, int quant)
{
    OFL_TRY(check_error_map_inputs(who, near, far, flow, fmask, elem, layout, N, C, 65535, H, W, sign, quant));
    if (metric != OFL_PHOTO_L1 && metric != OFL_PHOTO_L2 && metric != OFL_PHOTO_CHARBONNIER) return fail(OFL_E_INVALID, "%s: bad metric %d", who, metric);
    if (!finite_not_negative(eps)) return fail(OFL_E_INVALID, "%s: eps must be finite and not negative (got %g)", who, (double)eps);
    return check_error_map_outputs(who, err, within, tau);
}

template <int E, int QUANT>
void launch_photometric(const PArgs &a, int layout, hipStream_t s)
{
    if (layout == OFL_TENSOR_NCHW) {
        const dim3 grid((unsigned)((a.W + 63) / 64), (unsigned)((a.H + 3) / 4), (unsigned)a.N);
        switch (a.C) {
        case 1:  hipLaunchKernelGGL((photo_nchw_kernel<E, QUANT, 1>), grid, dim3(256), 0, s, a); break;
        case 2:  hipLaunchKernelGGL((photo_nchw_kernel<E, QUANT, 2>), grid, dim3(256), 0, s, a); break;
        case 3:  hipLaunchKernelGGL((photo_nchw_kernel<E, QUANT, 3>), grid, dim3(256), 0, s, a); break;
        case 4:  hipLaunchKernelGGL((photo_nchw_kernel<E, QUANT, 4>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((photo_nchw_kernel<E, QUANT, 0>), grid, dim3(256), 0, s, a); break;
        }
        return;
    }
    const int groups = (a.C + kV - 1) / kV;
    int lg = 0;
    while (lg < 4 && (1 << lg) < groups) ++lg;
    const size_t ppb = 256u >> lg;
    const dim3 grid((unsigned)(((size_t)a.H * a.W + ppb - 1) / ppb), (unsigned)a.N);
    const unsigned wide = kV * sizeof(typename Elem<E>::T);
    if (a.C % kV == 0 && host_aligned(a.near, wide) && host_aligned(a.far, wide))
        hipLaunchKernelGGL((photo_nhwc_kernel<E, QUANT, true>), grid, dim3(256), 0, s, a, lg);
    else
        hipLaunchKernelGGL((photo_nhwc_kernel<E, QUANT, false>), grid, dim3(256), 0, s, a, lg);
}

}  // namespace

extern "C" {

int ofl_photometric_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                        const float *flow, const uint8_t *fmask, int flow_shared, int sign,
                        const uint8_t *near_mask, const uint8_t *far_mask,
                        int metric, float eps, float tau,
                        float *err, uint8_t *covered, uint8_t *within, uint32_t *counts, int quant, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_photometric_args("ofl_photometric", near, far, elem, layout, N, C, H, W, flow, fmask, sign, metric, eps, tau, err, within, quant));
    PArgs a;
    OFL_TRY(error_map_fill("ofl_photometric", a, near, far, elem, layout, N, C, H, W, flow, fmask, flow_shared != 0, sign, near_mask, far_mask,
                           err, covered, within, counts, tau));
    a.metric = metric;
    a.eps2 = eps * eps;                                  // float32, rounded once (-ffp-contract=off)
    hipStream_t s = stream_of(stream);
    with_elem(elem, [&](auto E) { with_quant(quant, [&](auto Q) { launch_photometric<E.value, Q.value>(a, layout, s); }); });
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_photometric(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                    const float *flow, const uint8_t *fmask, int flow_shared, int sign,
                    const uint8_t *near_mask, const uint8_t *far_mask,
                    int metric, float eps, float tau,
                    float *err, uint8_t *covered, uint8_t *within, uint32_t *counts_host, int quant)
{
    OFL_TRY(need_device());
    OFL_TRY(check_photometric_args("ofl_photometric", near, far, elem, layout, N, C, H, W, flow, fmask, sign, metric, eps, tau, err, within, quant));
    return error_map_host("ofl_photometric", ofl_photometric_dev, near, far, elem, layout, N, C, H, W, flow, fmask, flow_shared, sign, near_mask, far_mask,
                          err, covered, within, counts_host, quant, metric, eps, tau);
}

}  // extern "C"
