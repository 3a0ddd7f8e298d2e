// ofl_upsample.hip -- K17: convex upsampling of a network's coarse flow (gfx950); the definition is in include/ofl.h.
// Every fine pixel (F * y + i, F * x + j) is the softmax-weighted combination of the 3 x 3 coarse neighbours of (y, x),
// scaled by F, with the 9 logits x[k * F * F + i * F + j] of that coarse pixel.  Every operation is float32 and rounded
// once, in the order tests/upsample_ref.py restates; exp32 below is a stated sequence of such operations, not a library or
// hardware exp.  The kernel relies on hipcc's default mode, which keeps float32 subnormals, as NumPy does.
//
// upsample_kernel<F, E, LAYOUT>, one workgroup per tile of T coarse pixels of one coarse row (and, planar with F = 8, per
// half of the sub-rows); 3 factors x 3 element types x 2 layouts = 18 instantiations.
//   stage      the 3 x (T + 2) coarse neighbourhood goes to LDS once: vectors already multiplied by F (exact), zero outside
//              the frame, and a byte "inside the frame implies mask set".  A coarse pixel's nine vectors and mask bytes are
//              loaded from memory here and nowhere else.
//   compute    NCHW  T = 64: lanes run along x, wave r of the block takes sub-row i = g * R + r and walks j = 0 .. F - 1, so
//                    a wave reads 64 consecutive coarse columns of one (k, i, j) plane per load; the sub-rows are split over
//                    the R = min(F, 4) waves of a block and, for F = 8, over two blocks: 136 x 240 coarse pixels give 4352
//                    waves.
//              NHWC  T = 128 / F: lanes run along the F * F sub-positions of a coarse pixel (F = 8: the 64 lanes of a wave
//                    are the 64 sub-positions of one pixel, a load reads 64 consecutive elements), 256 / (F * F) pixels per
//                    pass, F / 2 passes; the nine taps come from LDS as broadcasts.
//              Each result goes into a band of R fine rows x T * F fine pixels in LDS.
//   write-out  the band leaves as whole fine rows: consecutive lanes store consecutive 16-byte pairs of pixels (two 8-byte
//              stores where out_vecs is only 8-byte aligned), the mask four pixels per lane.  Nothing is stored with a
//              stride of F pixels.
// Logits are read element by element at their own alignment (a tensor may start at any element), offsets are 64-bit.  No
// index depends on a logit's value: NaN or Inf logits give unspecified values and nothing else.
// No atomics, no workspace, no scratch.
#include <stddef.h>
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_exp32.h"
#include "ofl_host_stage.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

// waves per SIMD the register allocator leaves room for (tests/test_upsample_resources.py): with 8 (64 registers) the
// channels-last F = 8 kernels, which hold the next pass's nine loads in flight, spill; they take 72, the others 61 at most
constexpr int kWaves = 6;
constexpr int kMaxFine = 32766;    // the largest height or width the field kernels take

template <int F, int LAYOUT> struct Tile {
    static constexpr bool kPlanar  = LAYOUT == OFL_TENSOR_NCHW;
    static constexpr int  kT       = kPlanar ? 64 : 128 / F;           // coarse pixels per tile
    static constexpr int  kRows    = kPlanar ? (F < 4 ? F : 4) : F;    // fine rows in the band of one block
    static constexpr int  kThreads = kPlanar ? 64 * kRows : 256;
    static constexpr int  kGroups  = F / kRows;                        // blocks that share one tile
    static constexpr int  kBand    = kT * F;                           // fine pixels per band row
};

struct UArgs {
    const float2  *vecs;
    const uint8_t *mask;
    const void    *logits;
    float2        *out_vecs;
    uint8_t       *out_mask;
    int            h, w;
};

// one fine pixel: the logits of tap k at p[k * step], the taps' scaled vectors in u, v.  The nine loads are unconditional, so
// that they are issued together and waited for once (a lane outside the frame is given the address of column 0).
template <int E>
__device__ __forceinline__ float2 convex(const typename Elem<E>::T *p, size_t step, const float (&u)[9], const float (&v)[9])
{
    float x[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = Elem<E>::to_f32(p[k * step]);
    float m = x[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) m = fmaxf(m, x[k]);
    float s = 0.0f, au = 0.0f, av = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float t = __fsub_rn(x[k], m);
        const float e = t < -87.0f ? 0.0f : exp32(t);
        const float eu = __fmul_rn(e, u[k]), ev = __fmul_rn(e, v[k]);
        s  = k ? __fadd_rn(s, e) : e;
        au = k ? __fadd_rn(au, eu) : eu;
        av = k ? __fadd_rn(av, ev) : ev;
    }
    return make_float2(__fdiv_rn(au, s), __fdiv_rn(av, s));
}

template <int F, int E, int LAYOUT>
__global__ __launch_bounds__((Tile<F, LAYOUT>::kThreads), kWaves)
void upsample_kernel(const UArgs a)
{
    typedef Tile<F, LAYOUT> C;
    typedef typename Elem<E>::T T;
    constexpr int TC = C::kT, SW = TC + 2, FF = F * F, NC = 9 * FF, BW = C::kBand, kThreads = C::kThreads;
    __shared__ float   su[3 * SW], sv[3 * SW];
    __shared__ uint8_t sok[3 * SW], scm[TC];
    __shared__ float4  band[C::kRows * BW / 2];
    float2 *band2 = reinterpret_cast<float2 *>(band);

    const int t = threadIdx.x, h = a.h, w = a.w;
    const int g = blockIdx.x % C::kGroups, x0 = (int)(blockIdx.x / C::kGroups) * TC, y = blockIdx.y;
    const size_t n = blockIdx.z, cpx = (size_t)h * w;

    for (int i = t; i < 3 * SW; i += kThreads) {
        const int dy = i / SW, yy = y + dy - 1, xx = x0 + (i - dy * SW) - 1;
        float2  f  = make_float2(0.0f, 0.0f);
        uint8_t ok = 1;
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
            const size_t q = n * cpx + (size_t)yy * w + xx;
            f  = a.vecs[q];
            ok = a.mask[q] != 0 ? 1 : 0;
        }
        su[i] = __fmul_rn(f.x, (float)F);
        sv[i] = __fmul_rn(f.y, (float)F);
        sok[i] = ok;
    }
    __syncthreads();
    if (t < TC) {
        uint8_t ok = 1;
#pragma unroll
        for (int k = 0; k < 9; ++k) ok &= sok[(k / 3) * SW + t + k % 3];
        scm[t] = ok;
    }

    const T *logits = static_cast<const T *>(a.logits);
    if (C::kPlanar) {
        const int lx = t & 63, i = g * C::kRows + (t >> 6), x = x0 + lx;
        float u[9], v[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { u[k] = su[(k / 3) * SW + lx + k % 3]; v[k] = sv[(k / 3) * SW + lx + k % 3]; }
        const T *p = logits + (n * NC + (size_t)i * F) * cpx + (size_t)y * w + (x < w ? x : 0);
#pragma unroll
        for (int j = 0; j < F; ++j)
            band2[(t >> 6) * BW + lx * F + j] = convex<E>(p + j * cpx, FF * cpx, u, v);
    } else {
        constexpr int kPass = 256 / FF;                    // coarse pixels per pass of the block
#pragma unroll 1
        for (int q = 0; q < TC / kPass; ++q) {
            const int lx = q * kPass + t / FF, s = t % FF, x = x0 + lx;
            float u[9], v[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) { u[k] = su[(k / 3) * SW + lx + k % 3]; v[k] = sv[(k / 3) * SW + lx + k % 3]; }
            const T *p = logits + (n * cpx + (size_t)y * w + (x < w ? x : 0)) * NC + s;
            band2[(s / F) * BW + lx * F + s % F] = convex<E>(p, FF, u, v);
        }
    }
    __syncthreads();

    // the band leaves as whole fine rows; `valid` fine pixels of a band row lie inside the frame (a multiple of F: even)
    const int valid = F * min(TC, w - x0), fw = F * w;
    const size_t row0 = (n * F * h + (size_t)F * y + g * C::kRows) * fw + (size_t)F * x0;
    const bool wide = (reinterpret_cast<uintptr_t>(a.out_vecs) & 15u) == 0;          // row0 is even: pairs are 16-byte aligned
    for (int c = t; c < C::kRows * BW / 2; c += kThreads) {
        const int r = c / (BW / 2), px = 2 * (c - r * (BW / 2));
        if (px < valid) {
            const float4 o = band[c];
            float2 *d = a.out_vecs + row0 + (size_t)r * fw + px;
            if (wide) *reinterpret_cast<float4 *>(d) = o;
            else { d[0] = make_float2(o.x, o.y); d[1] = make_float2(o.z, o.w); }
        }
    }
    if (a.out_mask) {
        for (int c = t; c < C::kRows * BW / 4; c += kThreads) {
            const int r = c / (BW / 4), px = 4 * (c - r * (BW / 4));
            if (px < valid) {
                uint8_t *d = a.out_mask + row0 + (size_t)r * fw + px;
                const uint32_t b0 = scm[px / F], b1 = scm[(px + 1) / F], b2 = scm[(px + 2) / F], b3 = scm[(px + 3) / F];
                if (px + 4 <= valid && (reinterpret_cast<uintptr_t>(d) & 3u) == 0) {
                    *reinterpret_cast<uint32_t *>(d) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
                } else {                                                              // valid is even: px + 1 is inside
                    d[0] = (uint8_t)b0; d[1] = (uint8_t)b1;
                    if (px + 2 < valid) { d[2] = (uint8_t)b2; d[3] = (uint8_t)b3; }
                }
            }
        }
    }
}

template <int F, int E, int LAYOUT>
void launch(const UArgs &a, int batch, hipStream_t s)
{
    typedef Tile<F, LAYOUT> C;
    const dim3 grid((unsigned)((a.w + C::kT - 1) / C::kT) * C::kGroups, (unsigned)a.h, (unsigned)batch);
    hipLaunchKernelGGL((upsample_kernel<F, E, LAYOUT>), grid, dim3(C::kThreads), 0, s, a);
}

template <int F, int E>
void launch_layout(int layout, const UArgs &a, int batch, hipStream_t s)
{
    if (layout == OFL_TENSOR_NCHW) launch<F, E, OFL_TENSOR_NCHW>(a, batch, s);
    else                           launch<F, E, OFL_TENSOR_NHWC>(a, batch, s);
}

template <int F>
void launch_elem(int elem, int layout, const UArgs &a, int batch, hipStream_t s)
{
    if (elem == OFL_EL_F16)       launch_layout<F, OFL_EL_F16>(layout, a, batch, s);
    else if (elem == OFL_EL_BF16) launch_layout<F, OFL_EL_BF16>(layout, a, batch, s);
    else                          launch_layout<F, OFL_EL_F32>(layout, a, batch, s);
}

size_t elem_bytes(int elem) { return elem == OFL_EL_F32 ? 4 : 2; }

int check_upsample_args(const char *who, const void *vecs, const void *mask, const void *logits, int elem, int layout, int h, int w,
                        int batch, int factor, const void *out_vecs, const void *out_mask)
{
    if (!vecs || !mask || !logits || !out_vecs)
        return fail(OFL_E_INVALID, "%s: NULL pointer (vecs, mask, logits and out_vecs are required)", who);
    if (factor != 2 && factor != 4 && factor != 8) return fail(OFL_E_INVALID, "%s: factor must be 2, 4 or 8 (got %d)", who, factor);
    if (elem != OFL_EL_F16 && elem != OFL_EL_BF16 && elem != OFL_EL_F32)
        return fail(OFL_E_INVALID, "%s: elem must be OFL_EL_F16, OFL_EL_BF16 or OFL_EL_F32 (got %d)", who, elem);
    if (layout != OFL_TENSOR_NCHW && layout != OFL_TENSOR_NHWC) return fail(OFL_E_INVALID, "%s: bad layout %d", who, layout);
    if (h < 1 || w < 1 || batch < 1 || batch > 65535)
        return fail(OFL_E_INVALID, "%s: h, w must be positive and batch in [1, 65535] (got %d x %d, %d)", who, h, w, batch);
    if (h > kMaxFine / factor || w > kMaxFine / factor)
        return fail(OFL_E_INVALID, "%s: %d x %d times %d is beyond the %d x %d a field may have", who, h, w, factor, kMaxFine, kMaxFine);
    const size_t c = (size_t)batch * h * w, f = c * factor * factor, lb = c * 9 * factor * factor * elem_bytes(elem);
    const void *ins[3] = { vecs, mask, logits };
    const size_t in_bytes[3] = { c * 8, c, lb };
    for (int i = 0; i < 3; ++i)
        if (overlap(out_vecs, f * 8, ins[i], in_bytes[i]) || overlap(out_mask, f, ins[i], in_bytes[i]))
            return fail(OFL_E_INVALID, "%s: outputs must not overlap inputs", who);
    if (overlap(out_vecs, f * 8, out_mask, f)) return fail(OFL_E_INVALID, "%s: out_vecs and out_mask overlap", who);
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_upsample_convex_dev(const float *vecs, const uint8_t *mask, const void *logits, int elem, int layout, int h, int w,
                            int batch, int factor, float *out_vecs, uint8_t *out_mask, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_upsample_args("ofl_upsample_convex", vecs, mask, logits, elem, layout, h, w, batch, factor, out_vecs, out_mask));
    if (!host_aligned(vecs, 8) || !host_aligned(out_vecs, 8))
        return fail(OFL_E_INVALID, "ofl_upsample_convex: vecs and out_vecs must be 8-byte aligned");
    if (!host_aligned(logits, (unsigned)elem_bytes(elem)))
        return fail(OFL_E_INVALID, "ofl_upsample_convex: logits must be aligned to the element size");
    UArgs a;
    a.vecs = reinterpret_cast<const float2 *>(vecs); a.mask = mask; a.logits = logits;
    a.out_vecs = reinterpret_cast<float2 *>(out_vecs); a.out_mask = out_mask; a.h = h; a.w = w;
    hipStream_t s = stream_of(stream);
    if (factor == 2)      launch_elem<2>(elem, layout, a, batch, s);
    else if (factor == 4) launch_elem<4>(elem, layout, a, batch, s);
    else                  launch_elem<8>(elem, layout, a, batch, s);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_upsample_convex(const float *vecs, const uint8_t *mask, const void *logits, int elem, int layout, int h, int w,
                        int batch, int factor, float *out_vecs, uint8_t *out_mask)
{
    OFL_TRY(need_device());
    OFL_TRY(check_upsample_args("ofl_upsample_convex", vecs, mask, logits, elem, layout, h, w, batch, factor, out_vecs, out_mask));
    const size_t c = (size_t)batch * h * w, f = c * factor * factor;
    HostStage st("ofl_upsample_convex");
    auto dv = st.in(vecs, c * 2);
    auto dm = st.in(mask, c);
    auto dl = st.in(logits, c * 9 * factor * factor * elem_bytes(elem));
    auto ov = st.out(out_vecs, f * 2);
    auto om = st.out(out_mask, f);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_upsample_convex_dev(dv, dm, dl, elem, layout, h, w, batch, factor, ov, om, st.stream()));
    return st.download();
}

}  // extern "C"
