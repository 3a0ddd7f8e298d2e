// ofl_build.hip -- K9: building, scaling, padding and cropping flow fields in HBM (gfx950).
// Pure streaming kernels: no LDS, no atomics, size_t indices, one workgroup per 256 work items with a grid-stride loop
// behind it; every lane stores one float4 (two pixels) and, where there is a mask, one 16-bit word; an odd pixel is left
// to one scalar store.
#include "ofl_common.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

int stream_grid(size_t n_items)
{
    const size_t nb = (n_items + 255) / 256;
    return (int)(nb < 1 ? 1 : (nb < 0x7fffffff ? nb : 0x7fffffff));
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// ---------------------------------------------------------------------------------------------- fields from matrices
// utils.flow_from_matrix (reference utils.py:91-111) per pixel: np.matmul of the float64 matrix with the float32 column
// (x, y, 1) accumulates left to right in float64, the quotient and the difference with the float32 grid are float64
// operations and the result is rounded to float32 once.
struct Mat { double m[9]; bool affine; };

__device__ __forceinline__ float2 matrix_vector(const Mat &M, int x, int y, int sign)
{
    const double xd = (double)x, yd = (double)y;
    double X = __dadd_rn(__dadd_rn(__dmul_rn(M.m[0], xd), __dmul_rn(M.m[1], yd)), M.m[2]);
    double Y = __dadd_rn(__dadd_rn(__dmul_rn(M.m[3], xd), __dmul_rn(M.m[4], yd)), M.m[5]);
    if (!M.affine) {        // last row (0, 0, 1): Z is exactly 1 and X / 1 == X
        const double Z = __dadd_rn(__dadd_rn(__dmul_rn(M.m[6], xd), __dmul_rn(M.m[7], yd)), M.m[8]);
        X = __ddiv_rn(X, Z);
        Y = __ddiv_rn(Y, Z);
    }
    float u = (float)__dsub_rn(X, xd), v = (float)__dsub_rn(Y, yd);
    if (sign < 0) { u = -u; v = -v; }       // after the cast: 0 becomes -0.0f like NumPy's -array
    return make_float2(u, v);
}

// blockIdx.y = field.  A field of an odd number of pixels leaves every second field 8 bytes off the 16-byte grid of the
// float4 stores: such a field stores its first pixel alone (`lead`) and pairs up the rest.
__global__ __launch_bounds__(256)
void flow_from_matrix_kernel(const double *__restrict__ mats, int sign, int H, int W, float *__restrict__ out)
{
    const size_t n_px = (size_t)H * W, field = blockIdx.y;
    Mat M;
#pragma unroll
    for (int k = 0; k < 9; ++k) M.m[k] = mats[field * 9 + k];
    M.affine = M.m[6] == 0.0 && M.m[7] == 0.0 && M.m[8] == 1.0;
    float2 *o2 = reinterpret_cast<float2 *>(out) + field * n_px;
    const size_t lead = (field * n_px) & 1, n2 = (n_px - lead) / 2, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n2; p += stride) {
        const size_t i = lead + 2 * p;                       // i + 1 < n_px
        const int y0 = (int)(i / W), x0 = (int)(i - (size_t)y0 * W);
        const bool wrap = x0 + 1 == W;
        const float2 a = matrix_vector(M, x0, y0, sign), b = matrix_vector(M, wrap ? 0 : x0 + 1, wrap ? y0 + 1 : y0, sign);
        *reinterpret_cast<float4 *>(o2 + i) = make_float4(a.x, a.y, b.x, b.y);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (lead) o2[0] = matrix_vector(M, 0, 0, sign);
        if (lead + 2 * n2 < n_px) o2[n_px - 1] = matrix_vector(M, W - 1, H - 1, sign);
    }
}

// ---------------------------------------------------------------------------------------------- scaling
// Flow.__mul__ / __truediv__ (flow_class.py:377-443) with a per-channel factor.  WIDE 0: float32 arithmetic with the
// factor rounded to float32 (NumPy with a Python scalar or a float32 operand); WIDE 1: the float64 operation rounded to
// float32 once (a float64 or integer array operand).
template <int WIDE, int DIVIDE>
__device__ __forceinline__ float scale1(float v, double k)
{
    if (WIDE) return (float)(DIVIDE ? __ddiv_rn((double)v, k) : __dmul_rn((double)v, k));
    return DIVIDE ? __fdiv_rn(v, (float)k) : __fmul_rn(v, (float)k);
}

// PAIR 1: one float4 per lane, vectors and result on the 16-byte grid.  PAIR 0: a field 8 bytes off it (every second field
// of a batch of odd fields, a view) -- the same pixel pair per lane as two float2, so the bytes do not depend on the route.
template <int WIDE, int DIVIDE, int PAIR>
__global__ __launch_bounds__(256)
void scale_kernel(const float *__restrict__ vecs, double k0, double k1, size_t n_px, float *__restrict__ out)
{
    const size_t n2 = n_px / 2, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n2; p += stride) {
        float4 v;
        if (PAIR) {
            v = reinterpret_cast<const float4 *>(vecs)[p];
        } else {
            const float2 a = reinterpret_cast<const float2 *>(vecs)[2 * p], b = reinterpret_cast<const float2 *>(vecs)[2 * p + 1];
            v = make_float4(a.x, a.y, b.x, b.y);
        }
        const float4 r = make_float4(scale1<WIDE, DIVIDE>(v.x, k0), scale1<WIDE, DIVIDE>(v.y, k1),
                                     scale1<WIDE, DIVIDE>(v.z, k0), scale1<WIDE, DIVIDE>(v.w, k1));
        if (PAIR) {
            reinterpret_cast<float4 *>(out)[p] = r;
        } else {
            reinterpret_cast<float2 *>(out)[2 * p] = make_float2(r.x, r.y);
            reinterpret_cast<float2 *>(out)[2 * p + 1] = make_float2(r.z, r.w);
        }
    }
    if ((n_px & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const size_t i = n_px - 1;
        out[2 * i] = scale1<WIDE, DIVIDE>(vecs[2 * i], k0);
        out[2 * i + 1] = scale1<WIDE, DIVIDE>(vecs[2 * i + 1], k1);
    }
}

template <int PAIR>
void launch_scale(const float *vecs, double k0, double k1, int divide, int wide, size_t n_px, float *out, hipStream_t s)
{
    const dim3 grid(stream_grid(n_px / 2)), block(256);
    if (wide && divide)  hipLaunchKernelGGL((scale_kernel<1, 1, PAIR>), grid, block, 0, s, vecs, k0, k1, n_px, out);
    else if (wide)       hipLaunchKernelGGL((scale_kernel<1, 0, PAIR>), grid, block, 0, s, vecs, k0, k1, n_px, out);
    else if (divide)     hipLaunchKernelGGL((scale_kernel<0, 1, PAIR>), grid, block, 0, s, vecs, k0, k1, n_px, out);
    else                 hipLaunchKernelGGL((scale_kernel<0, 0, PAIR>), grid, block, 0, s, vecs, k0, k1, n_px, out);
}

// ---------------------------------------------------------------------------------------------- padding and cropping
// Both are "output pixel (oy, ox) <- source pixel map(oy, ox)" with a source that is always inside the field.
struct Px { float2 v; uint32_t m; };

struct PadMap {     // Flow.pad, flow_class.py:508-526
    int H, W, top, left, mode;

    static __device__ __forceinline__ int reflect(int s, int n)      // np.pad 'symmetric': period 2n, mirrored in its second half
    {
        int m = s % (2 * n);
        if (m < 0) m += 2 * n;
        return m < n ? m : 2 * n - 1 - m;
    }

    __device__ __forceinline__ Px operator()(const float2 *__restrict__ vecs, const uint8_t *__restrict__ mask, int oy, int ox) const
    {
        int sy = oy - top, sx = ox - left;
        const bool inside = sy >= 0 && sy < H && sx >= 0 && sx < W;
        Px r = { make_float2(0.0f, 0.0f), 0u };
        if (inside) r.m = mask[(size_t)sy * W + sx];                 // the mask is 0 outside the frame in every mode
        if (!inside && mode == 0) return r;
        if (mode == 1) { sy = min(max(sy, 0), H - 1); sx = min(max(sx, 0), W - 1); }
        if (mode == 2) { sy = reflect(sy, H); sx = reflect(sx, W); }
        r.v = vecs[(size_t)sy * W + sx];
        return r;
    }
};

struct CropMap {    // Flow.__getitem__ with slices, flow_class.py:297-308
    int W, row0, row_step, col0, col_step;

    __device__ __forceinline__ Px operator()(const float2 *__restrict__ vecs, const uint8_t *__restrict__ mask, int oy, int ox) const
    {
        const size_t s = (size_t)(row0 + oy * row_step) * W + (size_t)(col0 + ox * col_step);
        Px r = { vecs[s], mask[s] };
        return r;
    }
};

template <typename Map>
__global__ __launch_bounds__(256)
void remap_kernel(Map map, const float2 *__restrict__ vecs, const uint8_t *__restrict__ mask, int Ho, int Wo,
                  float *__restrict__ out, uint8_t *__restrict__ mout)
{
    const size_t n_px = (size_t)Ho * Wo, n2 = n_px / 2, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n2; p += stride) {
        const size_t i = 2 * p;                              // i + 1 < n_px
        const int y0 = (int)(i / Wo), x0 = (int)(i - (size_t)y0 * Wo);
        const bool wrap = x0 + 1 == Wo;
        const Px a = map(vecs, mask, y0, x0), b = map(vecs, mask, wrap ? y0 + 1 : y0, wrap ? 0 : x0 + 1);
        reinterpret_cast<float4 *>(out)[p] = make_float4(a.v.x, a.v.y, b.v.x, b.v.y);
        reinterpret_cast<uint16_t *>(mout)[p] = (uint16_t)(a.m | (b.m << 8));
    }
    if ((n_px & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const Px a = map(vecs, mask, Ho - 1, Wo - 1);
        reinterpret_cast<float2 *>(out)[n_px - 1] = a.v;
        mout[n_px - 1] = (uint8_t)a.m;
    }
}

template <typename Map>
int launch_remap(const Map &map, const float *vecs, const uint8_t *mask, int Ho, int Wo, float *out, uint8_t *mout, void *stream)
{
    hipLaunchKernelGGL((remap_kernel<Map>), dim3(stream_grid((size_t)Ho * Wo / 2)), dim3(256), 0, stream_of(stream),
                       map, reinterpret_cast<const float2 *>(vecs), mask, Ho, Wo, out, mout);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_flow_from_matrix_dev(const double *mats_dev, int n, int sign, int H, int W, float *out_vecs, void *stream)
{
    OFL_TRY(need_device());
    if (!mats_dev || !out_vecs || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_flow_from_matrix: bad arguments");
    if (n < 1 || n > 65535) return fail(OFL_E_INVALID, "ofl_flow_from_matrix: n must be in [1, 65535], got %d", n);
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "ofl_flow_from_matrix: sign must be +1 or -1");
    if (!aligned16(out_vecs)) return fail(OFL_E_INVALID, "ofl_flow_from_matrix: out_vecs must be 16-byte aligned");
    hipLaunchKernelGGL(flow_from_matrix_kernel, dim3(stream_grid((size_t)H * W / 2), n), dim3(256), 0, stream_of(stream),
                       mats_dev, sign, H, W, out_vecs);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_scale_dev(const float *vecs, double k0, double k1, int divide, int wide, size_t n_px, float *out, void *stream)
{
    OFL_TRY(need_device());
    if (!vecs || !out) return fail(OFL_E_INVALID, "ofl_scale: NULL pointer");
    if (!aligned8(vecs) || !aligned8(out)) return fail(OFL_E_INVALID, "ofl_scale: vecs and out must be 8-byte aligned");
    if (n_px == 0) return OFL_OK;
    if (aligned16(vecs) && aligned16(out)) launch_scale<1>(vecs, k0, k1, divide, wide, n_px, out, stream_of(stream));
    else                                   launch_scale<0>(vecs, k0, k1, divide, wide, n_px, out, stream_of(stream));
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_pad_flow_dev(const float *vecs, const uint8_t *mask, int H, int W, int top, int bottom, int left, int right,
                     int mode, float *out_vecs, uint8_t *out_mask, void *stream)
{
    OFL_TRY(need_device());
    if (!vecs || !mask || !out_vecs || !out_mask || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_pad_flow: bad arguments");
    if (top < 0 || bottom < 0 || left < 0 || right < 0) return fail(OFL_E_INVALID, "ofl_pad_flow: negative padding");
    if (mode < 0 || mode > 2) return fail(OFL_E_INVALID, "ofl_pad_flow: mode must be 0 (constant), 1 (edge) or 2 (symmetric)");
    const int64_t Ho = (int64_t)H + top + bottom, Wo = (int64_t)W + left + right;
    if (Ho > 0x3fffffff || Wo > 0x3fffffff) return fail(OFL_E_INVALID, "ofl_pad_flow: padded field too large");
    if (!aligned16(out_vecs) || (reinterpret_cast<uintptr_t>(out_mask) & 1u))
        return fail(OFL_E_INVALID, "ofl_pad_flow: out_vecs must be 16-byte, out_mask 2-byte aligned");
    const PadMap map = { H, W, top, left, mode };
    return launch_remap(map, vecs, mask, (int)Ho, (int)Wo, out_vecs, out_mask, stream);
}

int ofl_crop_flow_dev(const float *vecs, const uint8_t *mask, int H, int W, int row0, int row_step, int rows,
                      int col0, int col_step, int cols, float *out_vecs, uint8_t *out_mask, void *stream)
{
    OFL_TRY(need_device());
    if (!vecs || !mask || !out_vecs || !out_mask || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_crop_flow: bad arguments");
    if (rows <= 0 || cols <= 0) return fail(OFL_E_INVALID, "ofl_crop_flow: empty result");
    const int64_t row1 = (int64_t)row0 + (int64_t)(rows - 1) * row_step, col1 = (int64_t)col0 + (int64_t)(cols - 1) * col_step;
    if (row0 < 0 || row0 >= H || row1 < 0 || row1 >= H || col0 < 0 || col0 >= W || col1 < 0 || col1 >= W)
        return fail(OFL_E_INVALID, "ofl_crop_flow: the slice leaves the %d x %d field", H, W);
    if (!aligned16(out_vecs) || (reinterpret_cast<uintptr_t>(out_mask) & 1u))
        return fail(OFL_E_INVALID, "ofl_crop_flow: out_vecs must be 16-byte, out_mask 2-byte aligned");
    const CropMap map = { W, row0, row_step, col0, col_step };
    return launch_remap(map, vecs, mask, rows, cols, out_vecs, out_mask, stream);
}

}  // extern "C"
