// ofl_correlation.hip -- K18: on-demand correlation lookup of two feature tensors (gfx950); the definition is in include/ofl.h.
// For every pixel of f1 the (2r + 2)^2 dot products with the rows of one pyramid level of f2 around the sample position are
// formed once, in float32 with every product and every sum rounded (no FMA) in the order tests/correlation_ref.py restates,
// and the (2r + 1)^2 window values are blended from them with the taps and weights of make_tap / blend4.  The all-pairs
// volume is never formed.
//
// corr_kernel<E1, E2, K>, one workgroup of four waves per tile of kTile = 32 consecutive pixels of one row of one item.
//   dots       a wave takes the pixels wave, wave + 4, ... of the tile, one at a time.  Its 64 lanes are 4 tap slots x kL = 16
//              channel lanes: a 16-lane group reads ONE row of f2 (the C channels of one integer tap), lane j the kV = 4
//              consecutive channels of the groups j, j + 16, j + 32, ... -- 16 B (float32) or 8 B (16-bit) per lane and load,
//              256 or 128 contiguous bytes per group -- so a wave-instruction touches four rows, never 64.  All loads of a
//              row are issued before the first product: they are unconditional, a tap outside the frame or a group beyond C
//              re-reads a valid address and its result is discarded.  The pixel's f1 channels stay in registers over the
//              (r + 1)^2 steps of the window (K = 2: C <= 128, K = 4: C <= 256); K = 0 takes any C and re-reads them, 128
//              channels at a time, from the cache; K = -1 reads element by element, 64 channels at a time (below).  The 16
//              partial sums of a group are added by four DPP stages inside the 16-lane row (quad_perm, quad_perm,
//              row_shr:4, row_shr:8): the pairwise tree of the definition, which is what makes kV = 4 and kL = 16.  Each
//              dot goes to LDS once.
//   window     after one barrier the 256 threads walk the tile's (2r + 1)^2 x 32 outputs with x fastest: four LDS reads
//              (101 floats per pixel: no bank conflicts), blend4, one multiply by scale, and a store that is contiguous
//              along x for 32 lanes -- a whole 128-byte line per channel.
// Where a tensor's base is not aligned to four elements, or C is no multiple of 4, both are read element by element by
// the K = -1 kernel, which also leaves the channels beyond C out of the last group.  Offsets are 64-bit.  No address
// depends on a feature value; the window arithmetic is int on taps saturated to +-32768.
// avgpool_kernel<E>: the 2 x 2 mean ((a + b) + (c + d)) * 0.25f of a channels-last tensor, one thread per output element.
// No atomics, no workspace, no scratch, no environment knob.
#include <stddef.h>
#include <vector>
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_host_stage.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

// waves per SIMD the register allocator is asked to leave room for (tests/test_correlation_resources.py).  Every
// instantiation takes 60 vector registers at most and would fit 8, but asked for 8 -- 96 scalar registers a wave -- the
// loop-invariant lane masks no longer fit and spill; asked for 6 nothing spills, and the hardware still holds 8.
constexpr int kWaves  = 6;
constexpr int kV      = OFL_CORR_V;     // consecutive channels per group
constexpr int kL      = OFL_CORR_L;     // partial sums: the channel lanes of one row
constexpr int kTile   = 32;             // pixels per workgroup
constexpr int kStride = 101;            // floats of LDS per pixel: (2 * 4 + 2)^2 dots, odd against the banks
static_assert(kV == 4 && kL == 16, "the loads and the DPP tree below are written for 4 channels x 16 lanes");

struct CArgs {
    const void  *f1, *f2;
    const float *flow;
    float       *out;
    int          C, H, W, Hl, Wl, sign, r, order, quant, total_ch, first_ch;
    float        inv, scale;            // 2^-level
    size_t       flow_step;             // pixels from one item's field to the next (0: shared)
};

template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// one stage of the tree: the blocks of S lanes [base, base + S) and [base + S, base + 2 S) of a 16-lane row become one.  The
// sum of a block is held by its HIGHEST lane; `o` is what lane j - S holds, for the highest lane of the upper block the sum
// of the lower block.  A block whose first lane has no channel (4 * lane >= C) is absent and adds nothing -- not even
// + 0.0f.  Channels fill the lanes from 0 up, so only the upper block can be absent: its highest lane then passes the lower
// block's sum on.  The other lanes compute values nobody reads.
template <int S>
__device__ __forceinline__ float tree_stage(float v, float o, int j, int C)
{
    const bool upper = 4 * ((j & ~(2 * S - 1)) | S) < C;
    return upper ? __fadd_rn(o, v) : o;
}

// -> the dot product, in lane 15 of the row
__device__ __forceinline__ float reduce16(float v, int j, int C)
{
    v = tree_stage<1>(v, dpp<0xB1>(v), j, C);        // quad_perm [1, 0, 3, 2]: lane ^ 1, for the odd lanes lane - 1
    v = tree_stage<2>(v, dpp<0x4E>(v), j, C);        // quad_perm [2, 3, 0, 1]: lane ^ 2, for lanes 3, 7, 11, 15 lane - 2
    v = tree_stage<4>(v, dpp<0x114>(v), j, C);       // row_shr:4: lane - 4
    v = tree_stage<8>(v, dpp<0x118>(v), j, C);       // row_shr:8: lane - 8
    return v;
}

// the groups c0 / 4 + j + 16 k (k < KK) of one row as float32; WIDE: one unconditional load per group
template <int E, int KK, bool WIDE>
__device__ __forceinline__ void load_groups(const typename Elem<E>::T *row, int c0, int C, int j, float (&v)[KK][4])
{
    typedef typename Elem<E>::T T;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        const int ch = c0 + kV * (j + kL * k), n = min(max(C - ch, 0), kV);
        if constexpr (WIDE) {                         // C % 4 == 0: n is 0 or 4, and an absent group re-reads group 0
            const T *p = row + (n ? ch : 0);
            if constexpr (sizeof(T) == 4) {
                const float4 q = *reinterpret_cast<const float4 *>(p);
                v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
            } else {
                const uint2 q = *reinterpret_cast<const uint2 *>(p);
                v[k][0] = Elem<E>::to_f32((T)(q.x & 0xffffu)); v[k][1] = Elem<E>::to_f32((T)(q.x >> 16));
                v[k][2] = Elem<E>::to_f32((T)(q.y & 0xffffu)); v[k][3] = Elem<E>::to_f32((T)(q.y >> 16));
            }
        } else {
#pragma unroll
            for (int i = 0; i < kV; ++i) v[k][i] = i < n ? Elem<E>::to_f32(row[ch + i]) : 0.0f;
        }
    }
}

// this lane's partial sum continued over the same groups, in ascending channel order; FIRST or first: the chain starts here
template <int KK, bool FIRST, bool WIDE>
__device__ __forceinline__ float dot_groups(float acc, const float (&x)[KK][4], const float (&y)[KK][4], int c0, int C, int j, bool first = false)
{
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        const int n = min(max(C - (c0 + kV * (j + kL * k)), 0), kV);
        if constexpr (WIDE) {
            float g = __fmul_rn(x[k][0], y[k][0]);
            if (!(FIRST && k == 0)) g = __fadd_rn(acc, g);
            g = __fadd_rn(g, __fmul_rn(x[k][1], y[k][1]));
            g = __fadd_rn(g, __fmul_rn(x[k][2], y[k][2]));
            g = __fadd_rn(g, __fmul_rn(x[k][3], y[k][3]));
            acc = n ? g : acc;
        } else {
#pragma unroll
            for (int i = 0; i < kV; ++i) {
                const float p = __fmul_rn(x[k][i], y[k][i]);
                const float g = ((FIRST || first) && k == 0 && i == 0) ? p : __fadd_rn(acc, p);
                acc = i < n ? g : acc;
            }
        }
    }
    return acc;
}

template <int E1, int E2, int K>
__global__ __launch_bounds__(256, kWaves)
void corr_kernel(const CArgs a)
{
    typedef typename Elem<E1>::T T1;
    typedef typename Elem<E2>::T T2;
    constexpr bool WIDE = K >= 0;
    constexpr int KK = K > 0 ? K : (K == 0 ? 2 : 1), kChunk = kV * kL * KK;      // channels per pass of the K <= 0 kernels
    __shared__ float  sD[kTile * kStride];
    __shared__ float4 sW[kTile];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slot = lane >> 4, j = lane & 15;
    const int C = a.C, H = a.H, W = a.W, Hl = a.Hl, Wl = a.Wl, r = a.r, S = 2 * r + 2;
    const int x0 = blockIdx.x * kTile, y = blockIdx.y, npx = min(kTile, W - x0);
    const size_t n = blockIdx.z;
    const T2 *item2 = static_cast<const T2 *>(a.f2) + n * Hl * Wl * (size_t)C;

    for (int xx = wave; xx < npx; xx += 4) {
        const int x = x0 + xx;
        const size_t pix = (size_t)y * W + x;
        float2 f = make_float2(0.0f, 0.0f);
        if (a.flow) f = *reinterpret_cast<const float2 *>(a.flow + 2 * (a.flow_step * n + pix));
        const float px = __fmul_rn(map_coord(x, f.x, a.sign), a.inv), py = __fmul_rn(map_coord(y, f.y, a.sign), a.inv);
        const Tap t = a.quant == OFL_QUANT_OPENCV ? make_tap<OFL_QUANT_OPENCV>(px, py) : make_tap<OFL_QUANT_EXACT>(px, py);
        if (lane == 0) sW[xx] = make_float4(t.w0, t.w1, t.w2, t.w3);

        const T1 *p1 = static_cast<const T1 *>(a.f1) + (n * H * W + pix) * (size_t)C;
        float a1[KK][4], a2[KK][4];
        if (K > 0) load_groups<E1, KK, WIDE>(p1, 0, C, j, a1);

        int tx = slot, ty = 0;                                           // S >= 4: a step of four taps wraps at most once
        for (int q = slot; q < S * S; q += 4) {
            const int ix = t.ix - r + tx, iy = t.iy - r + ty;
            const bool in = (unsigned)ix < (unsigned)Wl && (unsigned)iy < (unsigned)Hl;
            const T2 *row = item2 + (in ? ((size_t)iy * Wl + ix) * (size_t)C : (size_t)0);
            float acc = 0.0f;
            if (K > 0) {
                load_groups<E2, KK, WIDE>(row, 0, C, j, a2);
                acc = dot_groups<KK, true, WIDE>(acc, a1, a2, 0, C, j);
            } else if (K < 0) {
#pragma unroll 1
                for (int c0 = 0; c0 < C; c0 += kChunk) {
                    load_groups<E1, KK, WIDE>(p1, c0, C, j, a1);
                    load_groups<E2, KK, WIDE>(row, c0, C, j, a2);
                    acc = dot_groups<KK, false, WIDE>(acc, a1, a2, c0, C, j, c0 == 0);
                }
            } else {
                load_groups<E1, KK, WIDE>(p1, 0, C, j, a1);
                load_groups<E2, KK, WIDE>(row, 0, C, j, a2);
                acc = dot_groups<KK, true, WIDE>(acc, a1, a2, 0, C, j);
#pragma unroll 1
                for (int c0 = kChunk; c0 < C; c0 += kChunk) {
                    load_groups<E1, KK, WIDE>(p1, c0, C, j, a1);
                    load_groups<E2, KK, WIDE>(row, c0, C, j, a2);
                    acc = dot_groups<KK, false, WIDE>(acc, a1, a2, c0, C, j);
                }
            }
            acc = reduce16(acc, j, C);
            if (j == kL - 1) sD[xx * kStride + q] = in ? acc : 0.0f;
            tx += 4;
            if (tx >= S) { tx -= S; ++ty; }
        }
    }
    __syncthreads();

    const int win = 2 * r + 1, nch = win * win;
    const size_t plane = (size_t)H * W;
    float *out = a.out + (n * a.total_ch + a.first_ch) * plane + (size_t)y * W + x0;
    for (int e = threadIdx.x; e < nch * kTile; e += 256) {
        const int c = e / kTile, xx = e - c * kTile;
        if (xx < npx) {
            const int hi = c / win, lo = c - hi * win;
            const int tx = a.order == OFL_CORR_XY ? hi : lo, ty = a.order == OFL_CORR_XY ? lo : hi;
            const float *d = sD + xx * kStride + ty * S + tx;
            const float4 w = sW[xx];
            Tap t;
            t.w0 = w.x; t.w1 = w.y; t.w2 = w.z; t.w3 = w.w;
            out[(size_t)c * plane + xx] = __fmul_rn(blend4(d[0], d[1], d[S], d[S + 1], t), a.scale);
        }
    }
}

__device__ __forceinline__ uint64_t div_u64(uint64_t a, uint32_t b)
{
    return (a >> 32) == 0 ? (uint64_t)((uint32_t)a / b) : a / b;
}

template <int E>
__global__ __launch_bounds__(256)
void avgpool_kernel(const typename Elem<E>::T *__restrict__ src, float *__restrict__ dst, uint32_t C, uint32_t H, uint32_t W,
                    uint32_t Ho, uint32_t Wo, uint64_t total)
{
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const size_t right = C, down = (size_t)W * C;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const uint64_t p = div_u64(i, C), q = div_u64(p, Wo), n = div_u64(q, Ho);
        const uint64_t c = i - p * C, xo = p - q * Wo, yo = q - n * Ho;
        const typename Elem<E>::T *s = src + ((n * H + 2 * yo) * W + 2 * xo) * C + c;
        const float tl = Elem<E>::to_f32(s[0]), tr = Elem<E>::to_f32(s[right]);
        const float bl = Elem<E>::to_f32(s[down]), br = Elem<E>::to_f32(s[down + right]);
        dst[i] = __fmul_rn(__fadd_rn(__fadd_rn(tl, tr), __fadd_rn(bl, br)), 0.25f);
    }
}

template <int E1, int E2>
void launch_pair(const CArgs &a, int N, bool wide, hipStream_t s)
{
    const dim3 grid((unsigned)((a.W + kTile - 1) / kTile), (unsigned)a.H, (unsigned)N), block(256);
    if (!wide)                   hipLaunchKernelGGL((corr_kernel<E1, E2, -1>), grid, block, 0, s, a);
    else if (a.C <= kV * kL * 2) hipLaunchKernelGGL((corr_kernel<E1, E2, 2>), grid, block, 0, s, a);
    else if (a.C <= kV * kL * 4) hipLaunchKernelGGL((corr_kernel<E1, E2, 4>), grid, block, 0, s, a);
    else                         hipLaunchKernelGGL((corr_kernel<E1, E2, 0>), grid, block, 0, s, a);
}

template <int E1>
void launch_elem2(int elem2, const CArgs &a, int N, bool wide, hipStream_t s)
{
    if (elem2 == OFL_EL_F16)       launch_pair<E1, OFL_EL_F16>(a, N, wide, s);
    else if (elem2 == OFL_EL_BF16) launch_pair<E1, OFL_EL_BF16>(a, N, wide, s);
    else                           launch_pair<E1, OFL_EL_F32>(a, N, wide, s);
}

size_t elem_bytes(int elem) { return elem == OFL_EL_F32 ? 4 : 2; }

bool float_elem(int elem) { return elem == OFL_EL_F16 || elem == OFL_EL_BF16 || elem == OFL_EL_F32; }

int check_dims(const char *who, int N, int C, int H, int W)
{
    if (N < 1 || N > 65535 || C < 1 || C > 65535)
        return fail(OFL_E_INVALID, "%s: N and C must be in [1, 65535] (got %d and %d)", who, N, C);
    return check_field_dims(who, H, W);
}

// everything of a lookup but the pointers
int check_lookup_settings(const char *who, int elem1, int elem2, int N, int C, int H, int W, int sign, int r, int order, int quant)
{
    if (!float_elem(elem1) || !float_elem(elem2))
        return fail(OFL_E_INVALID, "%s: elements must be OFL_EL_F16, OFL_EL_BF16 or OFL_EL_F32 (got %d and %d)", who, elem1, elem2);
    OFL_TRY(check_dims(who, N, C, H, W));
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "%s: sign must be +1 or -1", who);
    if (r < 1 || r > 4) return fail(OFL_E_INVALID, "%s: the radius must be in [1, 4] (got %d)", who, r);
    if (order != OFL_CORR_XY && order != OFL_CORR_YX) return fail(OFL_E_INVALID, "%s: bad order %d", who, order);
    if (quant != OFL_QUANT_OPENCV && quant != OFL_QUANT_EXACT) return fail(OFL_E_INVALID, "%s: bad quant %d", who, quant);
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_avgpool2_dev(const void *src, int elem, int N, int C, int H, int W, float *dst, void *stream)
{
    OFL_TRY(need_device());
    if (!src || !dst) return fail(OFL_E_INVALID, "ofl_avgpool2: NULL pointer");
    if (!float_elem(elem)) return fail(OFL_E_INVALID, "ofl_avgpool2: elem must be OFL_EL_F16, OFL_EL_BF16 or OFL_EL_F32 (got %d)", elem);
    OFL_TRY(check_dims("ofl_avgpool2", N, C, H, W));
    if (H < 2 || W < 2) return fail(OFL_E_INVALID, "ofl_avgpool2: a %d x %d level has no 2 x 2 mean", H, W);
    if (!host_aligned(src, (unsigned)elem_bytes(elem)) || !host_aligned(dst, 4))
        return fail(OFL_E_INVALID, "ofl_avgpool2: src and dst must be aligned to their elements");
    const int Ho = H >> 1, Wo = W >> 1;
    const uint64_t total = (uint64_t)N * Ho * Wo * C;
    if (overlap(dst, total * 4, src, (size_t)N * H * W * C * elem_bytes(elem)))
        return fail(OFL_E_INVALID, "ofl_avgpool2: dst must not overlap src");
    const uint64_t nb = (total + 255) / 256;
    const dim3 grid((unsigned)(nb < 0x7fffffffull ? nb : 0x7fffffffull)), block(256);
    hipStream_t s = stream_of(stream);
    if (elem == OFL_EL_F16)
        hipLaunchKernelGGL((avgpool_kernel<OFL_EL_F16>), grid, block, 0, s, static_cast<const uint16_t *>(src), dst, C, H, W, Ho, Wo, total);
    else if (elem == OFL_EL_BF16)
        hipLaunchKernelGGL((avgpool_kernel<OFL_EL_BF16>), grid, block, 0, s, static_cast<const uint16_t *>(src), dst, C, H, W, Ho, Wo, total);
    else
        hipLaunchKernelGGL((avgpool_kernel<OFL_EL_F32>), grid, block, 0, s, static_cast<const float *>(src), dst, C, H, W, Ho, Wo, total);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_corr_lookup_dev(const void *f1, int elem1, const void *f2_l, int elem2, int N, int C, int H, int W, int H_l, int W_l,
                        int level, const float *flow, int flow_shared, int sign, int r, float scale, int order, int quant,
                        float *out, int total_channels, int first_channel, void *stream)
{
    const char *who = "ofl_corr_lookup";
    OFL_TRY(need_device());
    if (!f1 || !f2_l || !out) return fail(OFL_E_INVALID, "%s: NULL pointer (f1, f2_l and out are required)", who);
    OFL_TRY(check_lookup_settings(who, elem1, elem2, N, C, H, W, sign, r, order, quant));
    if (level < 0 || level > 7) return fail(OFL_E_INVALID, "%s: the level must be in [0, 7] (got %d)", who, level);
    if (H_l < 1 || W_l < 1 || H_l != H >> level || W_l != W >> level)
        return fail(OFL_E_INVALID, "%s: level %d of a %d x %d grid is %d x %d and must not be empty (got %d x %d)", who, level, H, W,
                    H >> level, W >> level, H_l, W_l);
    const int nch = (2 * r + 1) * (2 * r + 1);
    if (first_channel < 0 || total_channels < 1 || first_channel > total_channels - nch)
        return fail(OFL_E_INVALID, "%s: channels [%d, %d) do not lie in the %d of the output", who, first_channel, first_channel + nch,
                    total_channels);
    if (!host_aligned(f1, (unsigned)elem_bytes(elem1)) || !host_aligned(f2_l, (unsigned)elem_bytes(elem2)))
        return fail(OFL_E_INVALID, "%s: f1 and f2_l must be aligned to their elements", who);
    if (!host_aligned(out, 4) || !host_aligned(flow, 8)) return fail(OFL_E_INVALID, "%s: out must be 4-byte, flow 8-byte aligned", who);
    const size_t px = (size_t)H * W, ob = (size_t)N * total_channels * px * 4;
    const size_t b1 = (size_t)N * px * C * elem_bytes(elem1), b2 = (size_t)N * H_l * W_l * C * elem_bytes(elem2);
    if (overlap(out, ob, f1, b1) || overlap(out, ob, f2_l, b2) || overlap(out, ob, flow, (flow_shared ? 1 : (size_t)N) * px * 8))
        return fail(OFL_E_INVALID, "%s: the output must not overlap an input", who);
    CArgs a;
    a.f1 = f1; a.f2 = f2_l; a.flow = flow; a.out = out;
    a.C = C; a.H = H; a.W = W; a.Hl = H_l; a.Wl = W_l; a.sign = sign; a.r = r; a.order = order; a.quant = quant;
    a.total_ch = total_channels; a.first_ch = first_channel;
    // four elements per load where every row of both tensors starts on such a boundary; element by element otherwise
    const bool wide = C % kV == 0 && host_aligned(f1, (unsigned)(kV * elem_bytes(elem1))) && host_aligned(f2_l, (unsigned)(kV * elem_bytes(elem2)));
    a.inv = 1.0f / (float)(1 << level); a.scale = scale;
    a.flow_step = flow_shared ? 0 : px;
    hipStream_t s = stream_of(stream);
    if (elem1 == OFL_EL_F16)       launch_elem2<OFL_EL_F16>(elem2, a, N, wide, s);
    else if (elem1 == OFL_EL_BF16) launch_elem2<OFL_EL_BF16>(elem2, a, N, wide, s);
    else                           launch_elem2<OFL_EL_F32>(elem2, a, N, wide, s);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_corr_lookup(const void *f1, int elem1, const void *f2, int elem2, int N, int C, int H, int W, int levels,
                    const float *flow, int flow_shared, int sign, int r, float scale, int order, int quant, float *out)
{
    const char *who = "ofl_corr_lookup";
    OFL_TRY(need_device());
    if (!f1 || !f2 || !out) return fail(OFL_E_INVALID, "%s: NULL pointer (f1, f2 and out are required)", who);
    OFL_TRY(check_lookup_settings(who, elem1, elem2, N, C, H, W, sign, r, order, quant));
    if (levels < 1 || levels > 8) return fail(OFL_E_INVALID, "%s: levels must be in [1, 8] (got %d)", who, levels);
    if (H >> (levels - 1) < 1 || W >> (levels - 1) < 1)
        return fail(OFL_E_INVALID, "%s: level %d of a %d x %d grid is empty", who, levels - 1, H, W);
    const int nch = (2 * r + 1) * (2 * r + 1), total = levels * nch;
    const size_t px = (size_t)H * W;
    HostStage st(who);
    auto d1 = st.in(f1, (size_t)N * px * C * elem_bytes(elem1));
    auto d2 = st.in(f2, (size_t)N * px * C * elem_bytes(elem2));
    auto df = st.in(flow, (flow_shared ? 1 : (size_t)N) * px * 2);
    std::vector<HostStage::Part<float>> pyr;
    for (int l = 1; l < levels; ++l) pyr.push_back(st.scratch<float>((size_t)N * (H >> l) * (W >> l) * C));
    auto dout = st.out(out, (size_t)N * total * px);
    OFL_TRY(st.upload());
    const void *level = d2;
    int elem = elem2;
    for (int l = 0; l < levels; ++l) {
        if (l) {
            float *next = pyr[l - 1];
            OFL_TRY(ofl_avgpool2_dev(level, elem, N, C, H >> (l - 1), W >> (l - 1), next, st.stream()));
            level = next; elem = OFL_EL_F32;
        }
        OFL_TRY(ofl_corr_lookup_dev(d1, elem1, level, elem, N, C, H, W, H >> l, W >> l, l, df, flow_shared, sign, r, scale, order,
                                    quant, dout, total, l * nch, st.stream()));
    }
    return st.download();
}

}  // extern "C"
