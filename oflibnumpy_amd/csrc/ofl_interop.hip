// ofl_interop.hip -- K11: fields and images of another framework in, results out, without leaving HBM (gfx950).
// Three pure streaming kernels: no LDS, no scratch, 64-bit index arithmetic.  A lane owns 4 horizontally adjacent pixels
// of one row; every access is as wide as the ADDRESS it meets allows (decided per address, not per call: a view whose base
// is one element off still takes the scalar path and is correct), the row tail W % 4 goes element by element.
#include "ofl_common.h"
#include "ofl_elem.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

int stream_grid(uint64_t n_items)
{
    const uint64_t nb = (n_items + 255) / 256;
    return (int)(nb < 1 ? 1 : (nb < 0x7fffffff ? nb : 0x7fffffff));
}

__device__ __forceinline__ bool aligned_to(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

// item -> (row of the stack of fields, group of 4 pixels in it); 32-bit division whenever the item index allows it
__device__ __forceinline__ uint64_t div_u64(uint64_t a, uint32_t b)
{
    return (a >> 32) == 0 ? (uint64_t)((uint32_t)a / b) : a / b;
}

// ---------------------------------------------------------------------------------------------- 4 elements at a time
template <typename W, int BYTES>
__device__ __forceinline__ void load_words(const void *p, void *regs)
{
#pragma unroll
    for (int i = 0; i < BYTES / (int)sizeof(W); ++i) {
        const W w = reinterpret_cast<const W *>(p)[i];
        __builtin_memcpy(static_cast<char *>(regs) + i * sizeof(W), &w, sizeof(W));
    }
}

template <typename W, int BYTES>
__device__ __forceinline__ void store_words(void *p, const void *regs)
{
#pragma unroll
    for (int i = 0; i < BYTES / (int)sizeof(W); ++i) {
        W w;
        __builtin_memcpy(&w, static_cast<const char *>(regs) + i * sizeof(W), sizeof(W));
        reinterpret_cast<W *>(p)[i] = w;
    }
}

// N contiguous elements (N * sizeof(T) a multiple of 4): 16-, 8- or 4-byte words where the address allows, else elements
template <typename T, int N>
__device__ __forceinline__ void load_run(const T *p, T *v)
{
    constexpr int B = N * (int)sizeof(T);
    if (B % 16 == 0 && aligned_to(p, 16)) load_words<uint4, B>(p, v);
    else if (B % 8 == 0 && aligned_to(p, 8)) load_words<uint2, B>(p, v);
    else if (aligned_to(p, 4)) load_words<uint32_t, B>(p, v);
    else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = p[k];
    }
}

template <typename T, int N>
__device__ __forceinline__ void store_run(T *p, const T *v)
{
    constexpr int B = N * (int)sizeof(T);
    if (B % 16 == 0 && aligned_to(p, 16)) store_words<uint4, B>(p, v);
    else if (B % 8 == 0 && aligned_to(p, 8)) store_words<uint2, B>(p, v);
    else if (aligned_to(p, 4)) store_words<uint32_t, B>(p, v);
    else {
#pragma unroll
        for (int k = 0; k < N; ++k) p[k] = v[k];
    }
}

// the first `cnt` of 4 elements `stride` apart; the rest of v is zero and is never read from or written to memory
template <typename T>
__device__ __forceinline__ void load4(const T *p, int64_t stride, int cnt, T *v)
{
    if (cnt == 4 && stride == 1) {
        load_run<T, 4>(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < cnt ? p[k * stride] : T(0);
    }
}

template <typename T>
__device__ __forceinline__ void store4(T *p, int64_t stride, int cnt, const T *v)
{
    if (cnt == 4 && stride == 1) {
        store_run<T, 4>(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) p[k * stride] = v[k];
    }
}

__device__ __forceinline__ bool not_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) == 0x7f800000u; }

// ---------------------------------------------------------------------------------------------- import
// n fields of element type E with element strides (field, channel, row, column) -> [n][H][W][2] float32 + [n][H][W] uint8.
// out / mout may be NULL (count only).  counters[0] += components whose float32 value is not finite, counters[1] += mask
// bytes that are neither 0 nor 1: a ballot decides whether a wave has anything to count, popcounts of further ballots count
// it, and the first lane of a wave with a count adds it with one atomic each.
template <int E>
__global__ __launch_bounds__(256)
void import_flow_kernel(const typename Elem<E>::T *__restrict__ src, int64_t sf, int64_t sc, int64_t sr, int64_t sx,
                        int n, int H, int W, const uint8_t *__restrict__ msrc, int64_t mf, int64_t mr, int64_t mx,
                        float *__restrict__ out, uint8_t *__restrict__ mout, uint32_t *__restrict__ counters)
{
    typedef typename Elem<E>::T T;
    const uint32_t G = ((uint32_t)W + 3u) / 4u;
    const uint64_t items = (uint64_t)n * (uint64_t)H * G, step = (uint64_t)gridDim.x * blockDim.x;
    uint32_t bad_v = 0, bad_m = 0;                      // wave-uniform sums
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += step) {
        const uint64_t row = div_u64(i, G), f = div_u64(row, (uint32_t)H);
        const int64_t y = (int64_t)(row - f * (uint32_t)H), x = 4 * (int64_t)(i - row * G);
        const int cnt = (int)(W - x < 4 ? W - x : 4);
        const T *p = src + (int64_t)f * sf + y * sr + x * sx;
        T a[4], b[4];
        if (sc == 1 && sx == 2 && cnt == 4) {
            T w[8];                                     // interleaved and contiguous: 8 elements in a row (f32: two 16-byte loads)
            load_run<T, 8>(p, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) { a[k] = w[2 * k]; b[k] = w[2 * k + 1]; }
        } else {
            load4(p, sx, cnt, a);
            load4(p + sc, sx, cnt, b);
        }
        float u[4], v[4];
        uint32_t nf[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u[k] = Elem<E>::to_f32(a[k]);
            v[k] = Elem<E>::to_f32(b[k]);
            nf[k] = (not_finite(u[k]) ? 1u : 0u) | (not_finite(v[k]) ? 2u : 0u);
        }
        uint8_t m[4] = { 1, 1, 1, 1 };
        uint32_t odd = 0;                               // bit k: mask byte k is neither 0 nor 1
        if (msrc) {
            load4(msrc + (int64_t)f * mf + y * mr + x * mx, mx, cnt, m);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                odd |= (m[k] > 1 ? 1u : 0u) << k;
                m[k] = m[k] != 0 ? 1 : 0;
            }
        }
        if (counters && __ballot((nf[0] | nf[1] | nf[2] | nf[3] | odd) != 0)) {       // rare, and the same in every lane
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bad_v += __popcll(__ballot(nf[k] & 1u)) + __popcll(__ballot(nf[k] & 2u));
                bad_m += __popcll(__ballot((odd >> k) & 1u));
            }
        }
        if (out) {
            const uint64_t px = row * (uint32_t)W + (uint64_t)x;
            float2 *o = reinterpret_cast<float2 *>(out) + px;
            if (cnt == 4 && aligned_to(o, 16)) {
                reinterpret_cast<float4 *>(o)[0] = make_float4(u[0], v[0], u[1], v[1]);
                reinterpret_cast<float4 *>(o)[1] = make_float4(u[2], v[2], u[3], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) o[k] = make_float2(u[k], v[k]);
            }
            store4(mout + px, 1, cnt, m);
        }
    }
    // the lowest lane of a wave has the lowest item index: it is active in every round of the loop any lane of its wave takes
    if (counters && (threadIdx.x & 63u) == 0) {
        if (bad_v) atomicAdd(&counters[0], bad_v);
        if (bad_m) atomicAdd(&counters[1], bad_m);
    }
}

// ---------------------------------------------------------------------------------------------- export
// [n][H][W][2] float32 -> contiguous [n][H][W][2] or (PLANAR) [n][2][H][W] of element type E.
template <int E, bool PLANAR>
__global__ __launch_bounds__(256)
void export_flow_kernel(const float *__restrict__ vecs, int n, int H, int W, typename Elem<E>::T *__restrict__ dst)
{
    typedef typename Elem<E>::T T;
    const uint32_t G = ((uint32_t)W + 3u) / 4u;
    const uint64_t items = (uint64_t)n * (uint64_t)H * G, step = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t plane = (uint64_t)H * (uint32_t)W;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += step) {
        const uint64_t row = div_u64(i, G), f = div_u64(row, (uint32_t)H);
        const uint64_t y = row - f * (uint32_t)H, x = 4 * (i - row * G);
        const int cnt = (int)((uint64_t)W - x < 4 ? (uint64_t)W - x : 4);
        const uint64_t px = row * (uint32_t)W + x;
        float w[8];
        if (cnt == 4) {
            load_run<float, 8>(vecs + 2 * px, w);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] = k < 2 * cnt ? vecs[2 * px + k] : 0.0f;
        }
        if (PLANAR) {
            T a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { a[k] = Elem<E>::from_f32(w[2 * k]); b[k] = Elem<E>::from_f32(w[2 * k + 1]); }
            T *d = dst + 2 * f * plane + y * (uint32_t)W + x;
            store4(d, 1, cnt, a);
            store4(d + plane, 1, cnt, b);
        } else {
            T o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = Elem<E>::from_f32(w[k]);
            T *d = dst + 2 * px;
            if (cnt == 4) {
                store_run<T, 8>(d, o);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < 2 * cnt) d[k] = o[k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- image layouts
// TO_HWC: src [C][H][W] with element strides (s_c, s_h, s_w) -> dst contiguous [H][W][C]; else the other way round, the
// strides then describe dst.  T stands for the element SIZE only: nothing is converted.  Eight waves per SIMD are asked for
// (left alone the register allocator takes 116 VGPRs for 4-byte elements at C = 6) except for 8-byte elements at C = 5
// and 6, whose 40 and 48 data registers per lane would spill under that bound: those run at 5 to 7 waves, without scratch.
template <typename T, int C, bool TO_HWC>
__global__ __launch_bounds__(256, (sizeof(T) == 8 && C > 4) ? 1 : 8)
void permute_image_kernel(const T *__restrict__ src, T *__restrict__ dst, int H, int W, int64_t s_c, int64_t s_h, int64_t s_w)
{
    const uint32_t G = ((uint32_t)W + 3u) / 4u;
    const uint64_t items = (uint64_t)H * G, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += step) {
        const uint64_t y = div_u64(i, G), x = 4 * (i - y * G);
        const int cnt = (int)((uint64_t)W - x < 4 ? (uint64_t)W - x : 4);
        const int64_t planar = (int64_t)y * s_h + (int64_t)x * s_w;
        const uint64_t packed = (y * (uint32_t)W + x) * C;
        T v[4 * C], t[4];                               // v in [pixel][channel] order
        if (TO_HWC) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                load4(src + planar + c * s_c, s_w, cnt, t);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k * C + c] = t[k];
            }
            if (cnt == 4) {
                store_run<T, 4 * C>(dst + packed, v);
            } else {
#pragma unroll
                for (int k = 0; k < 4 * C; ++k)
                    if (k < cnt * C) dst[packed + k] = v[k];
            }
        } else {
            if (cnt == 4) {
                load_run<T, 4 * C>(src + packed, v);
            } else {
#pragma unroll
                for (int k = 0; k < 4 * C; ++k) v[k] = k < cnt * C ? src[packed + k] : T(0);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int k = 0; k < 4; ++k) t[k] = v[k * C + c];
                store4(dst + planar + c * s_c, s_w, cnt, t);
            }
        }
    }
}

template <typename T, bool TO_HWC>
int launch_permute(const void *src, void *dst, int C, int H, int W, int64_t s_c, int64_t s_h, int64_t s_w, hipStream_t s)
{
    const dim3 grid(stream_grid((uint64_t)H * (((uint64_t)W + 3) / 4))), block(256);
    const T *a = static_cast<const T *>(src);
    T *b = static_cast<T *>(dst);
    switch (C) {
    case 1: hipLaunchKernelGGL((permute_image_kernel<T, 1, TO_HWC>), grid, block, 0, s, a, b, H, W, s_c, s_h, s_w); break;
    case 2: hipLaunchKernelGGL((permute_image_kernel<T, 2, TO_HWC>), grid, block, 0, s, a, b, H, W, s_c, s_h, s_w); break;
    case 3: hipLaunchKernelGGL((permute_image_kernel<T, 3, TO_HWC>), grid, block, 0, s, a, b, H, W, s_c, s_h, s_w); break;
    case 4: hipLaunchKernelGGL((permute_image_kernel<T, 4, TO_HWC>), grid, block, 0, s, a, b, H, W, s_c, s_h, s_w); break;
    case 5: hipLaunchKernelGGL((permute_image_kernel<T, 5, TO_HWC>), grid, block, 0, s, a, b, H, W, s_c, s_h, s_w); break;
    default: hipLaunchKernelGGL((permute_image_kernel<T, 6, TO_HWC>), grid, block, 0, s, a, b, H, W, s_c, s_h, s_w); break;
    }
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

template <typename T>
int launch_permute_dir(const void *src, void *dst, int C, int H, int W, int64_t s_c, int64_t s_h, int64_t s_w, int to_hwc, hipStream_t s)
{
    return to_hwc ? launch_permute<T, true>(src, dst, C, H, W, s_c, s_h, s_w, s)
                  : launch_permute<T, false>(src, dst, C, H, W, s_c, s_h, s_w, s);
}

const unsigned kElemBytes[4] = { 2, 2, 4, 8 };          // OFL_EL_F16, OFL_EL_BF16, OFL_EL_F32, OFL_EL_F64

}  // namespace

extern "C" {

int ofl_import_flow_dev(const void *src, int elem, int64_t s_field, int64_t s_chan, int64_t s_row, int64_t s_col,
                        int n, int H, int W, const uint8_t *mask_src, int64_t m_field, int64_t m_row, int64_t m_col,
                        float *out_vecs, uint8_t *out_mask, uint32_t *counters, void *stream)
{
    OFL_TRY(need_device());
    if (!src || n <= 0 || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_import_flow: bad arguments");
    if (elem < OFL_EL_F16 || elem > OFL_EL_F64) return fail(OFL_E_INVALID, "ofl_import_flow: unknown element type %d", elem);
    if (s_field < 0 || s_chan < 0 || s_row < 0 || s_col < 0 || m_field < 0 || m_row < 0 || m_col < 0)
        return fail(OFL_E_INVALID, "ofl_import_flow: negative stride");
    if ((out_vecs == nullptr) != (out_mask == nullptr)) return fail(OFL_E_INVALID, "ofl_import_flow: out_vecs and out_mask go together");
    if (!out_vecs && !counters) return fail(OFL_E_INVALID, "ofl_import_flow: nothing to write and nothing to count");
    if (!host_aligned(src, kElemBytes[elem])) return fail(OFL_E_INVALID, "ofl_import_flow: src is not aligned to its element size");
    if (!host_aligned(out_vecs, 8) || !host_aligned(counters, 4)) return fail(OFL_E_INVALID, "ofl_import_flow: out_vecs must be 8-byte, counters 4-byte aligned");
    const dim3 grid(stream_grid((uint64_t)n * H * (((uint64_t)W + 3) / 4))), block(256);
    hipStream_t s = stream_of(stream);
#define OFL_IMPORT(E)                                                                                                         \
    hipLaunchKernelGGL((import_flow_kernel<E>), grid, block, 0, s, static_cast<const Elem<E>::T *>(src), s_field, s_chan,     \
                       s_row, s_col, n, H, W, mask_src, m_field, m_row, m_col, out_vecs, out_mask, counters)
    switch (elem) {
    case OFL_EL_F16:  OFL_IMPORT(OFL_EL_F16); break;
    case OFL_EL_BF16: OFL_IMPORT(OFL_EL_BF16); break;
    case OFL_EL_F32:  OFL_IMPORT(OFL_EL_F32); break;
    default:          OFL_IMPORT(OFL_EL_F64); break;
    }
#undef OFL_IMPORT
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_export_flow_dev(const float *vecs, int n, int H, int W, int elem, int planar, void *dst, void *stream)
{
    OFL_TRY(need_device());
    if (!vecs || !dst || n <= 0 || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_export_flow: bad arguments");
    if (elem < OFL_EL_F16 || elem > OFL_EL_F32) return fail(OFL_E_INVALID, "ofl_export_flow: element type must be f16, bf16 or f32, got %d", elem);
    if (!host_aligned(vecs, 8) || !host_aligned(dst, kElemBytes[elem])) return fail(OFL_E_INVALID, "ofl_export_flow: vecs must be 8-byte aligned, dst to its element size");
    const dim3 grid(stream_grid((uint64_t)n * H * (((uint64_t)W + 3) / 4))), block(256);
    hipStream_t s = stream_of(stream);
#define OFL_EXPORT(E)                                                                                                         \
    do {                                                                                                                      \
        if (planar) hipLaunchKernelGGL((export_flow_kernel<E, true>), grid, block, 0, s, vecs, n, H, W, static_cast<Elem<E>::T *>(dst)); \
        else        hipLaunchKernelGGL((export_flow_kernel<E, false>), grid, block, 0, s, vecs, n, H, W, static_cast<Elem<E>::T *>(dst)); \
    } while (0)
    switch (elem) {
    case OFL_EL_F16:  OFL_EXPORT(OFL_EL_F16); break;
    case OFL_EL_BF16: OFL_EXPORT(OFL_EL_BF16); break;
    default:          OFL_EXPORT(OFL_EL_F32); break;
    }
#undef OFL_EXPORT
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_permute_image_dev(const void *src, void *dst, int elem_bytes, int C, int H, int W,
                          int64_t s_chan, int64_t s_row, int64_t s_col, int to_hwc, void *stream)
{
    OFL_TRY(need_device());
    if (!src || !dst || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_permute_image: bad arguments");
    if (C < 1 || C > 6) return fail(OFL_E_INVALID, "ofl_permute_image: C must be in [1, 6], got %d", C);
    if (s_chan < 0 || s_row < 0 || s_col < 0) return fail(OFL_E_INVALID, "ofl_permute_image: negative stride");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
        return fail(OFL_E_INVALID, "ofl_permute_image: elements of 1, 2, 4 or 8 bytes, got %d", elem_bytes);
    if (!host_aligned(src, (unsigned)elem_bytes) || !host_aligned(dst, (unsigned)elem_bytes))
        return fail(OFL_E_INVALID, "ofl_permute_image: src and dst must be aligned to the element size");
    hipStream_t s = stream_of(stream);
    switch (elem_bytes) {
    case 1:  return launch_permute_dir<uint8_t>(src, dst, C, H, W, s_chan, s_row, s_col, to_hwc, s);
    case 2:  return launch_permute_dir<uint16_t>(src, dst, C, H, W, s_chan, s_row, s_col, to_hwc, s);
    case 4:  return launch_permute_dir<uint32_t>(src, dst, C, H, W, s_chan, s_row, s_col, to_hwc, s);
    default: return launch_permute_dir<uint64_t>(src, dst, C, H, W, s_chan, s_row, s_col, to_hwc, s);
    }
}

}  // extern "C"
