// ofl_tensor.hip -- K12: warp many-channel float tensors, (N, C, H, W) planar or (N, H, W, C) channels-last (gfx950).
//
// A C-channel float warp under cv2.remap is C one-channel warps that share one set of taps (utils.py:231-236,
// flow_class.py:604-695): per pixel the taps, the four weights and the four in-frame flags are computed ONCE
// (map_coord / make_tap of ofl_common.h, as K1 computes them) and every channel is blended from them with blend4.
// Elements are float32, float16 or bfloat16; 16-bit taps are widened to float32 (exact), blended in float32 and rounded
// once to the storage type (to nearest even, overflow to +-inf: Elem<E>::from_f32, the rounding of the K11 export).  A
// float32 tensor therefore equals K1's float32 result channel for channel, bit for bit.  Validity is K1's rule for a float
// concat (OFL_RULE_EQ1), one mask per item.
//
// Two memory mappings, because no single one keeps both layouts contiguous per wave-instruction:
//   NCHW  lanes run along x.  A block of 4 waves covers a tile of 4 rows x 64 (float32) or 128 (16-bit: two pixels per
//         lane) columns -- 256 contiguous bytes per wave store -- times a chunk of kChunk channels (blockIdx.y), so a small
//         image with many channels still gives chunks x tiles x N blocks.  Taps live in registers over the channel loop.
//   NHWC  lanes run along the channels.  A block covers kPix consecutive pixels of an item; its first wave computes their
//         taps into LDS (one coalesced flow load, one coalesced validity store), then all 256 threads walk the block's
//         kPix * C output elements in memory order: every store is contiguous over the block, every tap load contiguous over
//         the lanes of one pixel.  The same code takes C = 1 (64 lanes = 64 pixels) and C = 512 (8 wave-instructions a pixel).
// Every element offset is 64-bit and comes from the one helper tensor_index.
//
// OUT OF SCOPE: 's'-reference (scatter) warps of tensors, padding offsets (the field has the tensor's height and width),
// row bands, integer and float64 tensors, strided sources (ofl_tensor_import_dev makes a foreign view contiguous first).
#include "ofl_common.h"
#include "ofl_elem.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

constexpr int kChunk = 32;      // NCHW: channels per block
constexpr int kPix   = 64;      // NHWC: pixels per block

// element offset of (n, c, y, x) in a contiguous tensor of either layout; y and x may lie outside the frame (the offset of
// such a tap is formed but never dereferenced)
__device__ __forceinline__ int64_t tensor_index(int layout, int C, int H, int W, int n, int c, int y, int x)
{
    if (layout == OFL_TENSOR_NCHW) return (((int64_t)n * C + c) * H + y) * W + x;
    return (((int64_t)n * H + y) * W + x) * C + c;
}

// validity of one pixel, K1's OFL_RULE_EQ1: the bilinearly interpolated target mask is exactly 1, and the flow mask is set
__device__ __forceinline__ bool tap_valid(const uint8_t *__restrict__ smask, int W, const Tap &tp, const bool (&in)[4], uint8_t fm)
{
    float m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = tp.iy + (k >> 1), xx = tp.ix + (k & 1);
        m[k] = in[k] ? ((smask ? smask[(size_t)yy * W + xx] != 0 : true) ? 1.0f : 0.0f) : 0.0f;
    }
    return (blend4(m[0], m[1], m[2], m[3], tp) == 1.0f) & (fm != 0);
}

struct TArgs {
    const void    *src;
    void          *dst;
    const float   *flow;
    const uint8_t *smask, *fmask;
    uint8_t       *valid;
    int            N, C, H, W, sign;
    size_t         flow_step, smask_step, valid_step;      // pixels from one item's field / target mask / valid mask to the next (0: shared)
};

// ---------------------------------------------------------------------------------------------- planar
template <int E, int QUANT>
__global__ __launch_bounds__(256)
void gather_nchw_kernel(const TArgs a, int tiles_x)
{
    typedef typename Elem<E>::T T;
    constexpr int PX = sizeof(T) == 2 ? 2 : 1;            // pixels per lane: 256 bytes per wave store
    const int H = a.H, W = a.W, C = a.C;
    const int n = blockIdx.z, c0 = blockIdx.y * kChunk, c1 = min(c0 + kChunk, C);
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y = ty * 4 + (threadIdx.x >> 6);
    const int x0 = (tx * 64 + (threadIdx.x & 63)) * PX;
    if (y >= H || x0 >= W) return;
    const size_t px_n = (size_t)H * W, row = (size_t)y * W;
    const float   *flow  = a.flow + 2 * a.flow_step * n;
    const uint8_t *fmask = a.fmask ? a.fmask + a.flow_step * n : nullptr;
    const uint8_t *smask = a.smask ? a.smask + a.smask_step * n : nullptr;
    const bool want_valid = a.valid != nullptr && blockIdx.y == 0 && (a.valid_step != 0 || n == 0);

    Tap  tp[PX];
    bool in[PX][4], act[PX];
    int  off[PX][4];                                      // inside one plane: H * W < 2^31
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int x = x0 + j;
        act[j] = x < W;
        const float2 f = act[j] ? *reinterpret_cast<const float2 *>(flow + 2 * (row + x)) : make_float2(0.0f, 0.0f);
        tp[j] = make_tap<QUANT>(map_coord(x, f.x, a.sign), map_coord(y, f.y, a.sign));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int yy = tp[j].iy + (k >> 1), xx = tp[j].ix + (k & 1);
            in[j][k]  = act[j] && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            off[j][k] = in[j][k] ? yy * W + xx : 0;
        }
        if (want_valid && act[j])
            a.valid[a.valid_step * n + row + x] = tap_valid(smask, W, tp[j], in[j], fmask[row + x]) ? 1 : 0;
    }

    const T *sp = static_cast<const T *>(a.src) + tensor_index(OFL_TENSOR_NCHW, C, H, W, n, c0, 0, 0);
    T       *dp = static_cast<T *>(a.dst) + tensor_index(OFL_TENSOR_NCHW, C, H, W, n, c0, y, x0);
#pragma unroll 4
    for (int c = c0; c < c1; ++c, sp += px_n, dp += px_n) {
        T r[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = in[j][k] ? Elem<E>::to_f32(sp[off[j][k]]) : 0.0f;
            r[j] = Elem<E>::from_f32(blend4(v[0], v[1], v[2], v[3], tp[j]));
        }
        if constexpr (PX == 2) {
            if (act[1] && (reinterpret_cast<uintptr_t>(dp) & 3u) == 0) {
                *reinterpret_cast<uint32_t *>(dp) = (uint32_t)r[0] | ((uint32_t)r[1] << 16);
            } else {
                dp[0] = r[0];
                if (act[1]) dp[1] = r[1];
            }
        } else {
            dp[0] = r[0];
        }
    }
}

// ---------------------------------------------------------------------------------------------- channels-last
template <int E, int QUANT>
__global__ __launch_bounds__(256)
void gather_nhwc_kernel(const TArgs a)
{
    typedef typename Elem<E>::T T;
    __shared__ int4   s_pos[kPix];        // ix, iy, in-frame flags (bit k: tap k), unused
    __shared__ float4 s_w[kPix];
    const int H = a.H, W = a.W, C = a.C;
    const int n = blockIdx.y;
    const size_t px_n = (size_t)H * W, pix0 = (size_t)blockIdx.x * kPix;
    const uint32_t npx = (uint32_t)min((size_t)kPix, px_n - pix0);

    if (threadIdx.x < npx) {
        const size_t pix = pix0 + threadIdx.x;
        const int y = (int)((uint32_t)pix / (uint32_t)W), x = (int)((uint32_t)pix - (uint32_t)y * (uint32_t)W);      // H * W < 2^31
        const float2 f = *reinterpret_cast<const float2 *>(a.flow + 2 * (a.flow_step * n + pix));
        const Tap tp = make_tap<QUANT>(map_coord(x, f.x, a.sign), map_coord(y, f.y, a.sign));
        bool in[4];
        int flags = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int yy = tp.iy + (k >> 1), xx = tp.ix + (k & 1);
            in[k] = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            flags |= in[k] ? 1 << k : 0;
        }
        s_pos[threadIdx.x] = make_int4(tp.ix, tp.iy, flags, 0);
        s_w[threadIdx.x]   = make_float4(tp.w0, tp.w1, tp.w2, tp.w3);
        if (a.valid && (a.valid_step != 0 || n == 0)) {
            const uint8_t *smask = a.smask ? a.smask + a.smask_step * n : nullptr;
            a.valid[a.valid_step * n + pix] = tap_valid(smask, W, tp, in, a.fmask[a.flow_step * n + pix]) ? 1 : 0;
        }
    }
    __syncthreads();

    // the block's npx * C output elements in memory order: element e is channel c of pixel p
    const uint32_t total = npx * (uint32_t)C, q = 256u / (uint32_t)C, r = 256u - q * (uint32_t)C;
    uint32_t p = threadIdx.x / (uint32_t)C, c = threadIdx.x - p * (uint32_t)C;
    const T *src = static_cast<const T *>(a.src);
    T *dp = static_cast<T *>(a.dst) + tensor_index(OFL_TENSOR_NHWC, C, H, W, n, 0, 0, 0) + (int64_t)pix0 * C;
    const int64_t right = C, down = (int64_t)W * C;
    for (uint32_t e = threadIdx.x; e < total; e += 256u) {
        const int4   ps = s_pos[p];
        const float4 w  = s_w[p];
        Tap tp;
        tp.w0 = w.x; tp.w1 = w.y; tp.w2 = w.z; tp.w3 = w.w;
        const T *t00 = src + tensor_index(OFL_TENSOR_NHWC, C, H, W, n, (int)c, ps.y, ps.x);
        const float v00 = (ps.z & 1) ? Elem<E>::to_f32(t00[0]) : 0.0f;
        const float v01 = (ps.z & 2) ? Elem<E>::to_f32(t00[right]) : 0.0f;
        const float v10 = (ps.z & 4) ? Elem<E>::to_f32(t00[down]) : 0.0f;
        const float v11 = (ps.z & 8) ? Elem<E>::to_f32(t00[down + right]) : 0.0f;
        dp[e] = Elem<E>::from_f32(blend4(v00, v01, v10, v11, tp));
        c += r; p += q;
        if (c >= (uint32_t)C) { c -= (uint32_t)C; ++p; }
    }
}

// ---------------------------------------------------------------------------------------------- import, permute
__device__ __forceinline__ uint64_t div_u64(uint64_t a, uint32_t b)
{
    return (a >> 32) == 0 ? (uint64_t)((uint32_t)a / b) : a / b;
}

// a strided (N, C, H, W) view -> a contiguous tensor of `layout`; one element per thread and round, stores in memory order
template <typename T>
__global__ __launch_bounds__(256)
void tensor_import_kernel(const T *__restrict__ src, int64_t s_n, int64_t s_c, int64_t s_h, int64_t s_w,
                          int layout, int N, int C, int H, int W, T *__restrict__ dst)
{
    const uint64_t total = (uint64_t)N * C * H * W, step = (uint64_t)gridDim.x * blockDim.x;
    // the three inner extents of the destination, outermost first
    const uint32_t d1 = layout == OFL_TENSOR_NCHW ? C : H, d2 = layout == OFL_TENSOR_NCHW ? H : W, d3 = layout == OFL_TENSOR_NCHW ? W : C;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const uint64_t i2 = div_u64(i, d3), i1 = div_u64(i2, d2), n = div_u64(i1, d1);
        const int64_t k3 = (int64_t)(i - i2 * d3), k2 = (int64_t)(i2 - i1 * d2), k1 = (int64_t)(i1 - n * d1);
        const int64_t at = layout == OFL_TENSOR_NCHW ? k1 * s_c + k2 * s_h + k3 * s_w : k3 * s_c + k1 * s_h + k2 * s_w;
        dst[i] = src[(int64_t)n * s_n + at];
    }
}

// [N][R][K] -> [N][K][R] through a 32 x 32 tile in LDS (33 columns: no bank conflicts): both sides move 32 contiguous elements a row
template <typename T>
__global__ __launch_bounds__(256)
void tensor_transpose_kernel(const T *__restrict__ src, T *__restrict__ dst, uint32_t R, uint32_t K, uint32_t tiles_k)
{
    __shared__ T tile[32][33];
    const uint32_t tr = blockIdx.x / tiles_k, tk = blockIdx.x - tr * tiles_k;
    const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;
    const uint64_t item = (uint64_t)blockIdx.y * R * K;
#pragma unroll
    for (uint32_t j = ly; j < 32u; j += 8u) {
        const uint32_t rr = tr * 32u + j, kk = tk * 32u + lx;
        if (rr < R && kk < K) tile[j][lx] = src[item + (uint64_t)rr * K + kk];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = ly; j < 32u; j += 8u) {
        const uint32_t kk = tk * 32u + j, rr = tr * 32u + lx;
        if (rr < R && kk < K) dst[item + (uint64_t)kk * R + rr] = tile[lx][j];
    }
}

// the 2 x 2 mean ((tl + tr) + (bl + br)) * 0.25f of a tensor seen as [M][H][W][K] -- planar: M = N C, K = 1; channels last:
// M = N, K = C -- in float32, rounded once to the element type; one output element per thread and round, in memory order.
// An odd last row or column is never read.
template <int E>
__global__ __launch_bounds__(256)
void tensor_halve_kernel(const typename Elem<E>::T *__restrict__ src, typename Elem<E>::T *__restrict__ dst,
                         uint32_t K, uint32_t H, uint32_t W, uint32_t Ho, uint32_t Wo, uint64_t total)
{
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const size_t right = K, down = (size_t)W * K;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const uint64_t p = div_u64(i, K), q = div_u64(p, Wo), m = div_u64(q, Ho);
        const uint64_t k = i - p * K, xo = p - q * Wo, yo = q - m * Ho;
        const typename Elem<E>::T *s = src + ((m * H + 2 * yo) * W + 2 * xo) * K + k;
        const float tl = Elem<E>::to_f32(s[0]), tr = Elem<E>::to_f32(s[right]);
        const float bl = Elem<E>::to_f32(s[down]), br = Elem<E>::to_f32(s[down + right]);
        dst[i] = Elem<E>::from_f32(__fmul_rn(__fadd_rn(__fadd_rn(tl, tr), __fadd_rn(bl, br)), 0.25f));
    }
}

int check_tensor_dims(const char *who, int N, int C, int H, int W)
{
    if (N < 1 || N > 65535) return fail(OFL_E_INVALID, "%s: N must be in [1, 65535], got %d", who, N);
    if (C < 1 || C > 65535) return fail(OFL_E_INVALID, "%s: C must be in [1, 65535], got %d", who, C);
    // cv2.remap asserts src/dst dims < SHRT_MAX, as K1 does
    return check_field_dims(who, H, W);
}

template <int E>
int launch_gather_tensor(const TArgs &a, int layout, int quant, hipStream_t s)
{
    if (layout == OFL_TENSOR_NCHW) {
        const int cols = 64 * (sizeof(typename Elem<E>::T) == 2 ? 2 : 1);
        const int tiles_x = (a.W + cols - 1) / cols, tiles_y = (a.H + 3) / 4;
        const dim3 grid(tiles_x * tiles_y, (a.C + kChunk - 1) / kChunk, a.N);
        if (quant == OFL_QUANT_OPENCV) hipLaunchKernelGGL((gather_nchw_kernel<E, OFL_QUANT_OPENCV>), grid, dim3(256), 0, s, a, tiles_x);
        else                           hipLaunchKernelGGL((gather_nchw_kernel<E, OFL_QUANT_EXACT>), grid, dim3(256), 0, s, a, tiles_x);
    } else {
        const dim3 grid((unsigned)(((size_t)a.H * a.W + kPix - 1) / kPix), a.N);
        if (quant == OFL_QUANT_OPENCV) hipLaunchKernelGGL((gather_nhwc_kernel<E, OFL_QUANT_OPENCV>), grid, dim3(256), 0, s, a);
        else                           hipLaunchKernelGGL((gather_nhwc_kernel<E, OFL_QUANT_EXACT>), grid, dim3(256), 0, s, a);
    }
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_gather_tensor_dev(const void *src, int elem, int layout, int N, int C, int H, int W,
                          const float *flow, int flow_shared, int sign,
                          const uint8_t *smask, int smask_shared, const uint8_t *fmask,
                          void *dst, uint8_t *valid, int quant, void *stream)
{
    OFL_TRY(need_device());
    if (!src) return fail(OFL_E_INVALID, "ofl_gather_tensor: NULL src");
    if (!dst) return fail(OFL_E_INVALID, "ofl_gather_tensor: NULL dst");
    if (!flow) return fail(OFL_E_INVALID, "ofl_gather_tensor: NULL flow");
    if (elem != OFL_EL_F16 && elem != OFL_EL_BF16 && elem != OFL_EL_F32)
        return fail(OFL_E_INVALID, "ofl_gather_tensor: elem must be OFL_EL_F16, OFL_EL_BF16 or OFL_EL_F32, got %d", elem);
    if (layout != OFL_TENSOR_NCHW && layout != OFL_TENSOR_NHWC) return fail(OFL_E_INVALID, "ofl_gather_tensor: bad layout %d", layout);
    OFL_TRY(check_tensor_dims("ofl_gather_tensor", N, C, H, W));
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "ofl_gather_tensor: sign must be +1 or -1");
    if (quant != OFL_QUANT_OPENCV && quant != OFL_QUANT_EXACT) return fail(OFL_E_INVALID, "ofl_gather_tensor: bad quant");
    if (valid && !fmask) return fail(OFL_E_INVALID, "ofl_gather_tensor: valid needs fmask");
    const unsigned eb = elem == OFL_EL_F32 ? 4 : 2;
    if (!host_aligned(src, eb) || !host_aligned(dst, eb)) return fail(OFL_E_INVALID, "ofl_gather_tensor: src and dst must be aligned to the element size");
    if (!host_aligned(flow, 8)) return fail(OFL_E_INVALID, "ofl_gather_tensor: flow must be 8-byte aligned");
    TArgs a;
    a.src = src; a.dst = dst; a.flow = flow; a.smask = smask; a.fmask = fmask; a.valid = valid;
    a.N = N; a.C = C; a.H = H; a.W = W; a.sign = sign;
    a.flow_step  = flow_shared ? 0 : (size_t)H * W;
    a.smask_step = smask_shared ? 0 : (size_t)H * W;
    a.valid_step = (flow_shared && (!smask || smask_shared)) ? 0 : (size_t)H * W;      // every item's mask is the same one
    hipStream_t s = stream_of(stream);
    switch (elem) {
    case OFL_EL_F16:  return launch_gather_tensor<OFL_EL_F16>(a, layout, quant, s);
    case OFL_EL_BF16: return launch_gather_tensor<OFL_EL_BF16>(a, layout, quant, s);
    default:          return launch_gather_tensor<OFL_EL_F32>(a, layout, quant, s);
    }
}

int ofl_tensor_import_dev(const void *src, int elem_bytes, int64_t s_n, int64_t s_c, int64_t s_h, int64_t s_w,
                          int layout, int N, int C, int H, int W, void *dst, void *stream)
{
    OFL_TRY(need_device());
    if (!src || !dst) return fail(OFL_E_INVALID, "ofl_tensor_import: NULL pointer");
    if (elem_bytes != 2 && elem_bytes != 4) return fail(OFL_E_INVALID, "ofl_tensor_import: elements of 2 or 4 bytes, got %d", elem_bytes);
    if (layout != OFL_TENSOR_NCHW && layout != OFL_TENSOR_NHWC) return fail(OFL_E_INVALID, "ofl_tensor_import: bad layout %d", layout);
    OFL_TRY(check_tensor_dims("ofl_tensor_import", N, C, H, W));
    if (s_n < 0 || s_c < 0 || s_h < 0 || s_w < 0) return fail(OFL_E_INVALID, "ofl_tensor_import: negative stride");
    if (!host_aligned(src, (unsigned)elem_bytes) || !host_aligned(dst, (unsigned)elem_bytes))
        return fail(OFL_E_INVALID, "ofl_tensor_import: src and dst must be aligned to the element size");
    const uint64_t nb = ((uint64_t)N * C * H * W + 255) / 256;
    const dim3 grid((unsigned)(nb < 0x7fffffffull ? nb : 0x7fffffffull)), block(256);
    hipStream_t s = stream_of(stream);
    if (elem_bytes == 2)
        hipLaunchKernelGGL((tensor_import_kernel<uint16_t>), grid, block, 0, s, static_cast<const uint16_t *>(src), s_n, s_c, s_h, s_w,
                           layout, N, C, H, W, static_cast<uint16_t *>(dst));
    else
        hipLaunchKernelGGL((tensor_import_kernel<uint32_t>), grid, block, 0, s, static_cast<const uint32_t *>(src), s_n, s_c, s_h, s_w,
                           layout, N, C, H, W, static_cast<uint32_t *>(dst));
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_tensor_permute_dev(const void *src, void *dst, int elem_bytes, int N, int C, int H, int W, int to_nhwc, void *stream)
{
    OFL_TRY(need_device());
    if (!src || !dst) return fail(OFL_E_INVALID, "ofl_tensor_permute: NULL pointer");
    if (elem_bytes != 2 && elem_bytes != 4) return fail(OFL_E_INVALID, "ofl_tensor_permute: elements of 2 or 4 bytes, got %d", elem_bytes);
    OFL_TRY(check_tensor_dims("ofl_tensor_permute", N, C, H, W));
    if (!host_aligned(src, (unsigned)elem_bytes) || !host_aligned(dst, (unsigned)elem_bytes))
        return fail(OFL_E_INVALID, "ofl_tensor_permute: src and dst must be aligned to the element size");
    // NCHW -> NHWC transposes each item's [C][H * W] matrix, the way back its [H * W][C] matrix
    const uint32_t px = (uint32_t)H * (uint32_t)W, R = to_nhwc ? (uint32_t)C : px, K = to_nhwc ? px : (uint32_t)C;
    const uint64_t tiles_r = (R + 31u) / 32u, tiles_k = (K + 31u) / 32u;
    if (tiles_r * tiles_k > 0x7fffffffull) return fail(OFL_E_INVALID, "ofl_tensor_permute: %d x %d x %d is too large for one launch", C, H, W);
    const dim3 grid((unsigned)(tiles_r * tiles_k), N), block(256);
    hipStream_t s = stream_of(stream);
    if (elem_bytes == 2)
        hipLaunchKernelGGL((tensor_transpose_kernel<uint16_t>), grid, block, 0, s, static_cast<const uint16_t *>(src), static_cast<uint16_t *>(dst), R, K, (uint32_t)tiles_k);
    else
        hipLaunchKernelGGL((tensor_transpose_kernel<uint32_t>), grid, block, 0, s, static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst), R, K, (uint32_t)tiles_k);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_tensor_halve_dev(const void *src, int elem, int layout, int N, int C, int H, int W, void *dst, void *stream)
{
    OFL_TRY(need_device());
    if (!src || !dst) return fail(OFL_E_INVALID, "ofl_tensor_halve: NULL pointer");
    if (elem != OFL_EL_F16 && elem != OFL_EL_BF16 && elem != OFL_EL_F32)
        return fail(OFL_E_INVALID, "ofl_tensor_halve: elem must be OFL_EL_F16, OFL_EL_BF16 or OFL_EL_F32, got %d", elem);
    if (layout != OFL_TENSOR_NCHW && layout != OFL_TENSOR_NHWC) return fail(OFL_E_INVALID, "ofl_tensor_halve: bad layout %d", layout);
    OFL_TRY(check_tensor_dims("ofl_tensor_halve", N, C, H, W));
    if (H < 2 || W < 2) return fail(OFL_E_INVALID, "ofl_tensor_halve: a %d x %d tensor has no 2 x 2 mean", H, W);
    const unsigned eb = elem == OFL_EL_F32 ? 4 : 2;
    if (!host_aligned(src, eb) || !host_aligned(dst, eb)) return fail(OFL_E_INVALID, "ofl_tensor_halve: src and dst must be aligned to the element size");
    const uint32_t Ho = (uint32_t)H >> 1, Wo = (uint32_t)W >> 1, K = layout == OFL_TENSOR_NCHW ? 1u : (uint32_t)C;
    const uint64_t total = (uint64_t)N * C * Ho * Wo;
    if (overlap(dst, total * eb, src, (size_t)N * C * H * W * eb)) return fail(OFL_E_INVALID, "ofl_tensor_halve: dst must not overlap src");
    const uint64_t nb = (total + 255) / 256;
    const dim3 grid((unsigned)(nb < 0x7fffffffull ? nb : 0x7fffffffull)), block(256);
    hipStream_t s = stream_of(stream);
    if (elem == OFL_EL_F16)
        hipLaunchKernelGGL((tensor_halve_kernel<OFL_EL_F16>), grid, block, 0, s, static_cast<const uint16_t *>(src), static_cast<uint16_t *>(dst), K, (uint32_t)H, (uint32_t)W, Ho, Wo, total);
    else if (elem == OFL_EL_BF16)
        hipLaunchKernelGGL((tensor_halve_kernel<OFL_EL_BF16>), grid, block, 0, s, static_cast<const uint16_t *>(src), static_cast<uint16_t *>(dst), K, (uint32_t)H, (uint32_t)W, Ho, Wo, total);
    else
        hipLaunchKernelGGL((tensor_halve_kernel<OFL_EL_F32>), grid, block, 0, s, static_cast<const float *>(src), static_cast<float *>(dst), K, (uint32_t)H, (uint32_t)W, Ho, Wo, total);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

}  // extern "C"
