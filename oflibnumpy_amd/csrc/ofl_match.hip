// ofl_match.hip -- K19: global matching of two feature tensors on the matrix cores (gfx950); the definition is in include/ofl.h.
// Every pixel of f1 (a query) is dotted with every pixel of f2 (a key), a softmax runs over all H W keys and the flow is the
// expected key coordinate minus the query's own.  The (H W)^2 volume is never stored: a 32 x 32 tile of it lives in the 16
// accumulator registers of one MFMA chain, is consumed, and is formed again in the second sweep.
//
// match_kernel<E, MODE, B>, one workgroup of kW = 4 waves per B blocks of kT = 32 consecutive queries of one item: every wave
// holds all B blocks, so a key operand it loads feeds B MFMAs (B = 2 where that leaves a workgroup per CU, else B = 1).
//   tile       D = A B with A = 32 keys x channels (f2) and B = channels x 32 queries (f1).  Both tensors are channels-last, so
//              lane l reads the 8 consecutive channels 8 (l >> 5) ... of pixel l & 31 for either operand of
//              mfma_f32_32x32x16_{f16,bf16}: one 16-byte load.  For mfma_f32_32x32x2f32 lane l holds channel 2 s + (l >> 5) of
//              step s; it loads four channels (both lane halves the same 16 bytes) and picks.  Channels ascend through the steps; a step's tail beyond C is zero.
//              The result has the QUERY on the lane (l & 31) and 16 KEYS in the registers: register r of lane half
//              h = l >> 5 is key 32 T + (r & 3) + 8 (r >> 2) + 4 h of tile T, ascending in r.  So a lane walks keys of ONE query,
//              and max, index and the three sums run down the registers without a lane crossing.
//   keys       tile T goes to wave T mod 4; a wave walks its tiles upwards.  Keys beyond H W load key 0 and are left out.
//   sweep 1    per lane the maximum of s = D * scale and its first key (strict >, keys ascend); the two lane halves, then
//              the four waves (LDS), are merged by (larger s, then smaller key).
//   sweep 2    the same tiles by the same function; e = exp32(s - m), l += e, ax += e kx, ay += e ky per lane from +0.  A tile
//              in which every lane's largest s is below m - 87 adds only zeros and is skipped after its MFMAs (wave-uniform
//              branch).  (kx, ky) of a lane's first key comes from one division per tile, the 15 others from constant steps
//              and a wrap (W >= 28: one wrap at most) or a small division (W < 28).
//   merge      l_w = half 0 + half 1 per wave, then ((l_0 + l_1) + l_2) + l_3; likewise ax, ay.  The first 32 B threads write, a query each.
// MODE 0: aligned tensors with C <= 128 (16-bit) or 64 (float32), the queries' operands stay in registers over all tiles; MODE 1: aligned, any C, both
// operands are read per tile; MODE 2: any alignment and any C, element by element.  Offsets are 64-bit.  No address depends
// on a feature value.  No atomics, no workspace, no scratch.  The order of the sums (OFL_MATCH_TILE, OFL_MATCH_WAVES) does not
// depend on B or MODE: every route gives the same bytes.
#include <stddef.h>
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_exp32.h"
#include "ofl_host_stage.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

constexpr int kWavesOf[3] = { 0, 3, 2 };     // waves per SIMD the register allocator leaves room for, by B (tests/test_match_resources.py)
constexpr int kT     = OFL_MATCH_TILE;       // keys per tile = queries per workgroup
constexpr int kW     = OFL_MATCH_WAVES;      // waves that share the keys of one workgroup's queries
constexpr int kMaxC  = 512;
static_assert(kT == 32 && kW == 4, "the operand maps and the merge below are written for 32 x 32 tiles and four waves");

typedef float    acc_t  __attribute__((ext_vector_type(16)));
typedef _Float16 half8  __attribute__((ext_vector_type(8)));
typedef __bf16   bhalf8 __attribute__((ext_vector_type(8)));

struct MArgs {
    const void *f1, *f2;
    float2     *out_vecs;
    uint8_t    *out_mask;
    float      *out_conf;
    int32_t    *out_index;
    int         C, W, HW, sign;
    float       scale, min_conf;
};

// what one lane feeds into the MFMAs of `kChunk` channels
template <int E> struct Frag {                                  // 16-bit: one step of 16 channels, 8 of them in this lane
    static constexpr int kChunk = 16, kHeld = 8;                // channels per operand; operands MODE 0 holds in registers
    uint4 v;
};
template <> struct Frag<OFL_EL_F32> {                           // float32: two steps of 2 channels, one a lane and step
    static constexpr int kChunk = 4, kHeld = 16;
    float a, b;
};

// the operand of chunk c0 of the pixel whose channels start at `row`; channels >= C read as zero.  WIDE: `row` is 16-byte
// aligned and C a multiple of the 16 bytes, so a lane's vector is inside the row or wholly beyond it (then channel 0 is re-read).
template <int E, bool WIDE>
__device__ __forceinline__ Frag<E> load_frag(const typename Elem<E>::T *row, int c0, int C, int h)
{
    Frag<E> f;
    if constexpr (E == OFL_EL_F32) {
        float q[4];
        if constexpr (WIDE) {
            const bool in = c0 < C;
            const float4 t = *reinterpret_cast<const float4 *>(row + (in ? c0 : 0));
            q[0] = in ? t.x : 0.0f; q[1] = in ? t.y : 0.0f; q[2] = in ? t.z : 0.0f; q[3] = in ? t.w : 0.0f;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) { const bool in = c0 + i < C; const float t = row[in ? c0 + i : 0]; q[i] = in ? t : 0.0f; }
        }
        f.a = h ? q[1] : q[0];
        f.b = h ? q[3] : q[2];
    } else {
        const int c = c0 + 8 * h;
        if constexpr (WIDE) {
            const bool in = c < C;
            const uint4 t = *reinterpret_cast<const uint4 *>(row + (in ? c : 0));
            f.v = in ? t : make_uint4(0u, 0u, 0u, 0u);
        } else {
            uint32_t e[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { const bool in = c + i < C; const uint32_t t = row[in ? c + i : 0]; e[i] = in ? t : 0u; }
            f.v = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
        }
    }
    return f;
}

template <int E>
__device__ __forceinline__ acc_t mfma(const Frag<E> &key, const Frag<E> &query, acc_t acc)
{
    if constexpr (E == OFL_EL_F16) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, key.v), __builtin_bit_cast(half8, query.v), acc, 0, 0, 0);
    } else if constexpr (E == OFL_EL_BF16) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bhalf8, key.v), __builtin_bit_cast(bhalf8, query.v), acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(key.a, query.a, acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x2f32(key.b, query.b, acc, 0, 0, 0);
    }
}

// the kB 32 x 32 tiles of dots of one key tile with the workgroup's kB query blocks: the one instruction sequence both sweeps
// use.  A key operand is loaded once and feeds kB MFMAs.  krow: this lane's key pixel, qrow[b]: its query pixel of block b;
// held[b]: that query's operands (MODE 0).
template <int E, int MODE, int kB>
__device__ __forceinline__ void tile_dots(acc_t (&acc)[kB], const typename Elem<E>::T *krow, const typename Elem<E>::T *const (&qrow)[kB],
                                          const Frag<E> (&held)[kB][Frag<E>::kHeld], int C, int h)
{
    constexpr int kChunk = Frag<E>::kChunk;
#pragma unroll
    for (int b = 0; b < kB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
    if constexpr (MODE == 0) {
#pragma unroll
        for (int s = 0; s < Frag<E>::kHeld; ++s)
            if (s * kChunk < C) {
                const Frag<E> key = load_frag<E, true>(krow, s * kChunk, C, h);
#pragma unroll
                for (int b = 0; b < kB; ++b) acc[b] = mfma<E>(key, held[b][s], acc[b]);
            }
    } else {
        for (int c0 = 0; c0 < C; c0 += kChunk) {
            const Frag<E> key = load_frag<E, MODE == 1>(krow, c0, C, h);
#pragma unroll
            for (int b = 0; b < kB; ++b) acc[b] = mfma<E>(key, load_frag<E, MODE == 1>(qrow[b], c0, C, h), acc[b]);
        }
    }
}

// (m, i) <- the better of (m, i) and (m2, i2): the larger logit, of two equal ones the smaller key
__device__ __forceinline__ void better(float &m, int &i, float m2, int i2)
{
    const bool take = m2 > m || (m2 == m && i2 < i);
    m = take ? m2 : m;
    i = take ? i2 : i;
}

template <int E, int MODE, int kB>
__global__ __launch_bounds__(64 * kW, kWavesOf[kB])
void match_kernel(const MArgs a)
{
    typedef typename Elem<E>::T T;
    constexpr int kHeld = Frag<E>::kHeld, kQ = kB * kT;                   // kQ queries per workgroup
    __shared__ float sM[kW][kQ], sL[kW][kQ], sX[kW][kQ], sY[kW][kQ];
    __shared__ int   sI[kW][kQ];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, h = lane >> 5;
    const int C = a.C, W = a.W, HW = a.HW;
    const size_t n = blockIdx.y;
    const T *item1 = static_cast<const T *>(a.f1) + n * HW * (size_t)C, *item2 = static_cast<const T *>(a.f2) + n * HW * (size_t)C;
    const int tiles = (HW + kT - 1) / kT;
    int q[kB];                                                            // this lane's queries; beyond H W it computes on query 0
    const T *qrow[kB];
#pragma unroll
    for (int b = 0; b < kB; ++b) {
        q[b] = blockIdx.x * kQ + b * kT + col;
        qrow[b] = item1 + (size_t)(q[b] < HW ? q[b] : 0) * C;
    }

    Frag<E> held[kB][kHeld];
    if constexpr (MODE == 0) {
#pragma unroll
        for (int b = 0; b < kB; ++b)
#pragma unroll
            for (int s = 0; s < kHeld; ++s) held[b][s] = load_frag<E, true>(qrow[b], s * Frag<E>::kChunk, C, h);
    }

    // ---- sweep 1: the maximum and its first key
    float m[kB];
    int idx[kB];
#pragma unroll
    for (int b = 0; b < kB; ++b) { m[b] = -INFINITY; idx[b] = 0; }
    for (int t = wave; t < tiles; t += kW) {
        const int key = t * kT + col;                                     // as the A operand this lane reads key t kT + col
        acc_t d[kB];
        tile_dots<E, MODE, kB>(d, item2 + (size_t)(key < HW ? key : 0) * C, qrow, held, C, h);
        const int k0 = t * kT + 4 * h;
#pragma unroll
        for (int b = 0; b < kB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = k0 + (r & 3) + 8 * (r >> 2);
                const float s = __fmul_rn(d[b][r], a.scale);
                const bool take = k < HW && s > m[b];
                m[b] = take ? s : m[b];
                idx[b] = take ? k : idx[b];
            }
    }
#pragma unroll
    for (int b = 0; b < kB; ++b) {
        better(m[b], idx[b], __shfl_xor(m[b], 32), __shfl_xor(idx[b], 32));
        if (h == 0) { sM[wave][b * kT + col] = m[b]; sI[wave][b * kT + col] = idx[b]; }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < kB; ++b) {
        m[b] = sM[0][b * kT + col]; idx[b] = sI[0][b * kT + col];
#pragma unroll
        for (int w = 1; w < kW; ++w) better(m[b], idx[b], sM[w][b * kT + col], sI[w][b * kT + col]);
    }

    // ---- sweep 2: the three sums
    float l[kB], ax[kB], ay[kB];
#pragma unroll
    for (int b = 0; b < kB; ++b) l[b] = ax[b] = ay[b] = 0.0f;
    const bool one_wrap = W >= 28;                                        // the 28 keys a lane spans in a tile cross one row end at most
    for (int t = wave; t < tiles; t += kW) {
        const int key = t * kT + col;
        acc_t d[kB];
        tile_dots<E, MODE, kB>(d, item2 + (size_t)(key < HW ? key : 0) * C, qrow, held, C, h);
        const int k0 = t * kT + 4 * h;
        int x0 = 0, y0 = -1;                                              // of key k0, once a block needs it
#pragma unroll
        for (int b = 0; b < kB; ++b) {
            float s[16], top = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = __fmul_rn(d[b][r], a.scale); top = fmaxf(top, s[r]); }
            if (!__any(!(__fsub_rn(top, m[b]) < -87.0f))) continue;       // every e of the tile is 0: adding them changes no bit
            if (y0 < 0) { y0 = (int)((unsigned)k0 / (unsigned)W); x0 = k0 - y0 * W; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = (r & 3) + 8 * (r >> 2);
                int kx = x0 + o, ky = y0;
                if (one_wrap) {
                    if (kx >= W) { kx -= W; ky += 1; }
                } else {
                    const int up = (int)((unsigned)kx / (unsigned)W);
                    kx -= up * W; ky += up;
                }
                const float tt = __fsub_rn(s[r], m[b]);
                const float e = (tt < -87.0f || k0 + o >= HW) ? 0.0f : exp32(tt);
                l[b]  = __fadd_rn(l[b], e);
                ax[b] = __fadd_rn(ax[b], __fmul_rn(e, (float)kx));
                ay[b] = __fadd_rn(ay[b], __fmul_rn(e, (float)ky));
            }
        }
    }
#pragma unroll
    for (int b = 0; b < kB; ++b) {
        l[b]  = __fadd_rn(l[b], __shfl_xor(l[b], 32));
        ax[b] = __fadd_rn(ax[b], __shfl_xor(ax[b], 32));
        ay[b] = __fadd_rn(ay[b], __shfl_xor(ay[b], 32));
        if (h == 0) { sL[wave][b * kT + col] = l[b]; sX[wave][b * kT + col] = ax[b]; sY[wave][b * kT + col] = ay[b]; }
    }
    __syncthreads();
    // the workgroup's kQ queries: one lane each
    const int t = threadIdx.x, qq = blockIdx.x * kQ + t;
    if (t >= kQ || qq >= HW) return;
    float L = sL[0][t], X = sX[0][t], Y = sY[0][t];
#pragma unroll
    for (int w = 1; w < kW; ++w) { L = __fadd_rn(L, sL[w][t]); X = __fadd_rn(X, sX[w][t]); Y = __fadd_rn(Y, sY[w][t]); }
    float M = sM[0][t];
    int I = sI[0][t];
#pragma unroll
    for (int w = 1; w < kW; ++w) better(M, I, sM[w][t], sI[w][t]);

    const int y = (int)((unsigned)qq / (unsigned)W), x = qq - y * W;
    const float u = __fsub_rn(__fdiv_rn(X, L), (float)x), v = __fsub_rn(__fdiv_rn(Y, L), (float)y);
    const float conf = __fdiv_rn(1.0f, L), sg = (float)a.sign;
    const size_t o = n * HW + qq;
    a.out_vecs[o] = make_float2(__fmul_rn(sg, u), __fmul_rn(sg, v));
    a.out_mask[o] = conf >= a.min_conf ? 1 : 0;
    if (a.out_conf)  a.out_conf[o]  = conf;
    if (a.out_index) a.out_index[o] = I;                                   // 0, or a k < H W that sweep 1 took
}

template <int E, int B>
void launch_blocks(const MArgs &a, int N, int mode, hipStream_t s)
{
    const dim3 grid((unsigned)((a.HW + B * kT - 1) / (B * kT)), (unsigned)N), block(64 * kW);
    if (mode == 0)      hipLaunchKernelGGL((match_kernel<E, 0, B>), grid, block, 0, s, a);
    else if (mode == 1) hipLaunchKernelGGL((match_kernel<E, 1, B>), grid, block, 0, s, a);
    else                hipLaunchKernelGGL((match_kernel<E, 2, B>), grid, block, 0, s, a);
}

// two query blocks a wave where that still leaves a workgroup for every CU, one otherwise; the bytes are the same either way
template <int E>
void launch(const MArgs &a, int N, int mode, hipStream_t s)
{
    if ((long long)N * ((a.HW + 2 * kT - 1) / (2 * kT)) >= rt().n_cu) launch_blocks<E, 2>(a, N, mode, s);
    else                                                               launch_blocks<E, 1>(a, N, mode, s);
}

size_t elem_bytes(int elem) { return elem == OFL_EL_F32 ? 4 : 2; }

// everything but the pointers' presence and alignment
int check_match_settings(const char *who, int elem, int N, int C, int H, int W, int sign, float min_conf)
{
    if (elem != OFL_EL_F16 && elem != OFL_EL_BF16 && elem != OFL_EL_F32)
        return fail(OFL_E_INVALID, "%s: elem must be OFL_EL_F16, OFL_EL_BF16 or OFL_EL_F32 (got %d)", who, elem);
    if (N < 1 || N > 65535) return fail(OFL_E_INVALID, "%s: N must be in [1, 65535] (got %d)", who, N);
    if (C < 1 || C > kMaxC) return fail(OFL_E_INVALID, "%s: C must be in [1, %d] (got %d)", who, kMaxC, C);
    OFL_TRY(check_field_dims(who, H, W));
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "%s: sign must be +1 or -1", who);
    if (!(min_conf >= 0.0f)) return fail(OFL_E_INVALID, "%s: min_conf must be >= 0 and not NaN", who);
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_global_match_dev(const void *f1, const void *f2, int elem, int N, int C, int H, int W, float scale, int sign,
                         float min_conf, float *out_vecs, uint8_t *out_mask, float *out_conf, int32_t *out_index, void *stream)
{
    const char *who = "ofl_global_match";
    OFL_TRY(need_device());
    if (!f1 || !f2 || !out_vecs || !out_mask) return fail(OFL_E_INVALID, "%s: NULL pointer (f1, f2, out_vecs and out_mask are required)", who);
    OFL_TRY(check_match_settings(who, elem, N, C, H, W, sign, min_conf));
    const unsigned eb = (unsigned)elem_bytes(elem);
    if (!host_aligned(f1, eb) || !host_aligned(f2, eb)) return fail(OFL_E_INVALID, "%s: f1 and f2 must be aligned to their element", who);
    if (!host_aligned(out_vecs, 8) || !host_aligned(out_conf, 4) || !host_aligned(out_index, 4))
        return fail(OFL_E_INVALID, "%s: out_vecs must be 8-byte, out_conf and out_index 4-byte aligned", who);
    const size_t px = (size_t)N * H * W, fb = px * C * eb;
    const void *outs[4] = { out_vecs, out_mask, out_conf, out_index };
    const size_t out_bytes[4] = { px * 8, px, px * 4, px * 4 };
    for (int i = 0; i < 4; ++i) {
        if (overlap(outs[i], out_bytes[i], f1, fb) || overlap(outs[i], out_bytes[i], f2, fb))
            return fail(OFL_E_INVALID, "%s: an output must not overlap an input", who);
        for (int j = 0; j < i; ++j)
            if (overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return fail(OFL_E_INVALID, "%s: the outputs overlap each other", who);
    }
    MArgs a;
    a.f1 = f1; a.f2 = f2; a.out_vecs = reinterpret_cast<float2 *>(out_vecs); a.out_mask = out_mask; a.out_conf = out_conf;
    a.out_index = out_index; a.C = C; a.W = W; a.HW = H * W; a.sign = sign; a.scale = scale; a.min_conf = min_conf;
    // 16 bytes per load where every pixel's channels of both tensors start on such a boundary; element by element otherwise
    const bool wide = C % (16 / (int)eb) == 0 && host_aligned(f1, 16) && host_aligned(f2, 16);
    const int mode = !wide ? 2 : (C <= (elem == OFL_EL_F32 ? Frag<OFL_EL_F32>::kChunk * Frag<OFL_EL_F32>::kHeld : Frag<OFL_EL_F16>::kChunk * Frag<OFL_EL_F16>::kHeld) ? 0 : 1);
    hipStream_t s = stream_of(stream);
    if (elem == OFL_EL_F16)       launch<OFL_EL_F16>(a, N, mode, s);
    else if (elem == OFL_EL_BF16) launch<OFL_EL_BF16>(a, N, mode, s);
    else                          launch<OFL_EL_F32>(a, N, mode, s);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_global_match(const void *f1, const void *f2, int elem, int N, int C, int H, int W, float scale, int sign,
                     float min_conf, float *out_vecs, uint8_t *out_mask, float *out_conf, int32_t *out_index)
{
    const char *who = "ofl_global_match";
    OFL_TRY(need_device());
    if (!f1 || !f2 || !out_vecs || !out_mask) return fail(OFL_E_INVALID, "%s: NULL pointer (f1, f2, out_vecs and out_mask are required)", who);
    OFL_TRY(check_match_settings(who, elem, N, C, H, W, sign, min_conf));
    const size_t px = (size_t)N * H * W;
    HostStage st(who);
    auto d1 = st.in(f1, px * C * elem_bytes(elem));
    auto d2 = st.in(f2, px * C * elem_bytes(elem));
    auto ov = st.out(out_vecs, px * 2);
    auto om = st.out(out_mask, px);
    auto oc = st.out(out_conf, px);
    auto oi = st.out(out_index, px);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_global_match_dev(d1, d2, elem, N, C, H, W, scale, sign, min_conf, ov, om, oc, oi, st.stream()));
    return st.download();
}

}  // extern "C"
