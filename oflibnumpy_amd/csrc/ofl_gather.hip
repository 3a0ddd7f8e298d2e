// ofl_gather.hip -- K1, the general bilinear gather of an image along a flow field, for gfx950.
//
// An HBM-bound byte mover (no MFMA): every output pixel streams its flow vector (coalesced, 16 B per lane), derives the
// cv2.remap sample position, and gathers the 2x2 source neighbourhood of every channel.  Reuse between neighbouring pixels is
// served by the per-CU L1 and the per-XCD L2, which is why workgroups own 2-D tiles.  Numerics follow oracle/ofl_oracle.c
// operation for operation (contraction disabled): results and validity masks are bit-identical to the CPU restatement.
#include "ofl_common.h"
#include "ofl_host_stage.h"
#include "ofl_pairs.h"
#include <type_traits>

#pragma clang fp contract(off)

using namespace ofl;

namespace {

// MI355X deals consecutive workgroups round-robin over its 8 XCDs.  Give every XCD a contiguous
// run of tiles so that neighbouring tiles (which share gather halos) meet in the same L2.
__device__ __forceinline__ int xcd_swizzle(int bid, int nblocks)
{
    constexpr int kXcd = 8;
    int per = nblocks / kXcd;
    int main = per * kXcd;
    if (bid >= main) return bid;            // ragged tail keeps its natural position
    return (bid % kXcd) * per + bid / kXcd;
}

template <typename T> struct Acc { typedef float type; };
template <> struct Acc<double> { typedef double type; };

template <typename T> __device__ __forceinline__ T finish(float s, int arith);
template <> __device__ __forceinline__ float    finish<float>(float s, int) { return s; }
template <> __device__ __forceinline__ int16_t  finish<int16_t>(float s, int) { return (int16_t)sat_s16(cv_round(s)); }
template <> __device__ __forceinline__ uint16_t finish<uint16_t>(float s, int) { return (uint16_t)min(max(cv_round(s), 0), 65535); }
template <> __device__ __forceinline__ uint8_t  finish<uint8_t>(float s, int) { return (uint8_t)sat_s16(cv_round(s)); }

// Batched launches of K1 (ofl_gather_bilinear_batch_dev): blockIdx.y = the field of the batch; element strides from one field's
// arrays to the next (0: the array is shared by the whole batch -- one source image warped by B flows; or absent).
struct GBatch { size_t src, smask, flow, fmask, dst, valid; };

template <typename T, int CT>
__global__ __launch_bounds__(256)
void gather_kernel(const T *__restrict__ src0, int Crt, int H, int W,
                   const float *__restrict__ flow0, int fH, int fW, int pad_top, int pad_left, int sign,
                   const uint8_t *__restrict__ smask0, const uint8_t *__restrict__ fmask0,
                   T *__restrict__ dst0, uint8_t *__restrict__ valid0,
                   int quant, int arith, int rule, int tiles_x, int nblocks, int row0, int rows, GBatch bs)
{
    const size_t bi = blockIdx.y;
    const T *__restrict__ src = src0 + bi * bs.src;
    const float *__restrict__ flow = flow0 + bi * bs.flow;
    const uint8_t *__restrict__ smask = smask0 ? smask0 + bi * bs.smask : nullptr;
    const uint8_t *__restrict__ fmask = fmask0 ? fmask0 + bi * bs.fmask : nullptr;
    T *__restrict__ dst = dst0 + bi * bs.dst;
    uint8_t *__restrict__ valid = valid0 ? valid0 + bi * bs.valid : nullptr;
    const int C    = CT > 0 ? CT : Crt;
    const int tile = xcd_swizzle(blockIdx.x, nblocks);
    const int ty   = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x    = tx * 32 + (threadIdx.x & 31);
    const int yl   = ty * 8 + (threadIdx.x >> 5);           // row inside the output band [row0, row0 + rows)
    const int y    = row0 + yl;
    if (x >= W || yl >= rows) return;

    float fu = 0.0f, fv = 0.0f;
    const int  fy = y - pad_top, fx = x - pad_left;
    const bool in_flow = (unsigned)fy < (unsigned)fH && (unsigned)fx < (unsigned)fW;
    if (in_flow) {
        const float2 f = *reinterpret_cast<const float2 *>(flow + ((size_t)fy * fW + fx) * 2);
        fu = f.x; fv = f.y;
    }
    const float px = map_coord(x, fu, sign), py = map_coord(y, fv, sign);
    const Tap tp = (quant == OFL_QUANT_OPENCV) ? make_tap<OFL_QUANT_OPENCV>(px, py) : make_tap<OFL_QUANT_EXACT>(px, py);

    int wi[4];
    if (quant == OFL_QUANT_OPENCV) {
        wi[0] = (32 - tp.ay) * (32 - tp.ax) * 32; wi[1] = (32 - tp.ay) * tp.ax * 32;
        wi[2] = tp.ay * (32 - tp.ax) * 32;        wi[3] = tp.ay * tp.ax * 32;
    } else {
        wi[0] = __float2int_rn(tp.w0 * 32768.0f); wi[1] = __float2int_rn(tp.w1 * 32768.0f);
        wi[2] = __float2int_rn(tp.w2 * 32768.0f); wi[3] = __float2int_rn(tp.w3 * 32768.0f);
    }

    bool   in[4];
    size_t off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = tp.iy + (k >> 1), xx = tp.ix + (k & 1);
        in[k]  = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        off[k] = in[k] ? (size_t)yy * W + xx : 0;
    }
    const size_t o = (size_t)yl * W + x;
    const bool fixed_u8 = (sizeof(T) == 1) && arith == OFL_ARITH_NATIVE;

    auto do_channel = [&](int cc) {
        typedef typename Acc<T>::type A;
        A v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = in[k] ? (A)src[off[k] * C + cc] : (A)0;
        if constexpr (sizeof(T) == 8) {
            dst[o * C + cc] = (T)blend4d(v[0], v[1], v[2], v[3], tp);
        } else {
            if (fixed_u8) {
                const int acc = (int)v[0] * wi[0] + (int)v[1] * wi[1] + (int)v[2] * wi[2] + (int)v[3] * wi[3];
                dst[o * C + cc] = (T)min(max((acc + (1 << 14)) >> 15, 0), 255);
            } else {
                dst[o * C + cc] = finish<T>(blend4((float)v[0], (float)v[1], (float)v[2], (float)v[3], tp), arith);
            }
        }
    };
    if constexpr (CT > 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) do_channel(c);
    } else {
        for (int c = 0; c < C; ++c) do_channel(c);
    }

    if (valid) {
        int m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = in[k] ? (smask ? (smask[off[k]] != 0) : 1) : 0;
        bool ok;
        if (rule == OFL_RULE_GE_HALF) {
            const int acc = m[0] * wi[0] + m[1] * wi[1] + m[2] * wi[2] + m[3] * wi[3];
            ok = ((acc + (1 << 14)) >> 15) == 1;
        } else {
            const float s = blend4((float)m[0], (float)m[1], (float)m[2], (float)m[3], tp);
            ok = (rule == OFL_RULE_EQ1) ? (s == 1.0f) : (cv_round(s) == 1);
        }
        if (fmask) ok = ok & in_flow & (in_flow ? fmask[(size_t)fy * fW + fx] != 0 : false);
        valid[o] = ok ? 1 : 0;
    }
}

// K1, paired form (W even, C = 1..4): same lane mapping as K2 -- 128 x 8 tiles, each lane owns the pixel
// pairs at x = 2*lx and x = 64 + 2*lx, so flow loads (16 B), image stores (2*C elements) and validity stores
// (2 B) of a wave are contiguous -- and the same three wave-uniform paths (all samples outside / all
// inside / border).  Numerics are those of gather_kernel (and of the oracle), element for element.
// BYTES (2 .. 16) consecutive bytes from a possibly unaligned address into 32-bit words
template <int BYTES>
__device__ __forceinline__ void load_run(const uint8_t *p, uint32_t (&w)[4])
{
    if constexpr (BYTES == 2) {
        w[0] = *reinterpret_cast<const uint16_t *>(p);
    } else if constexpr (BYTES == 4) {
        w[0] = *reinterpret_cast<const uint32_t *>(p);
    } else if constexpr (BYTES == 6) {
        w[0] = *reinterpret_cast<const uint32_t *>(p);
        w[1] = *reinterpret_cast<const uint16_t *>(p + 4);
    } else if constexpr (BYTES == 8) {
        const uint2 t = *reinterpret_cast<const uint2 *>(p);
        w[0] = t.x; w[1] = t.y;
    } else if constexpr (BYTES == 12) {
        const uint2 t = *reinterpret_cast<const uint2 *>(p);
        w[0] = t.x; w[1] = t.y;
        w[2] = *reinterpret_cast<const uint32_t *>(p + 8);
    } else {
        static_assert(BYTES == 16, "load_run: unsupported run length");
        const uint4 t = *reinterpret_cast<const uint4 *>(p);
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
    }
}

template <typename T>
__device__ __forceinline__ T run_elem(const uint32_t (&w)[4], int i)      // i is a compile-time constant after unrolling
{
    if constexpr (sizeof(T) == 1)      return (T)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
    else if constexpr (sizeof(T) == 2) return (T)((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
    else                               return (T)__uint_as_float(w[i]);
}

// Are the two taps of a row fetched as ONE run of 2 * CT adjacent elements (2 .. 16 bytes; float: 1 or 2 channels), where they
// lie inside the source, or tap by tap?
template <typename T, int CT> struct PxRun { static constexpr bool value = sizeof(T) <= 2 || (sizeof(T) == 4 && CT <= 2); };

// A pixel's taps as blend_taps takes them: the two rows' runs, or a callable (tap k, channel c) -> value for taps fetched one by one
struct RunTaps { const uint32_t (&run)[2][4]; };

// K1's arithmetic, stated once: the four taps of a pixel's channels (taps) and of its source mask (m) in, the result and the
// validity out.  gather_px and px_blend differ only in how the taps were fetched.
template <typename T, int CT, typename Taps>
__device__ __forceinline__ void blend_taps(const Taps &taps, const int (&m)[4], const Tap &tp, const int (&wi)[4], bool fixed_u8, bool sep,
                                           int arith, int rule, bool want_valid, T (&res)[CT], bool &ok)
{
    typedef typename Acc<T>::type A;
    // uint8 images with cv2's 15-bit fixed-point weights: w_k = 32 (32 - ay | ay) (32 - ax | ax), so
    //   (sum v_k w_k + 2^14) >> 15  ==  ((32 - ay) h0 + ay h1 + 512) >> 10   with   h_r = (32 - ax) v_r0 + ax v_r1
    // exactly (32 S + 16384 = 32 (S + 512)); the weights sum to 1024, so the result needs no clamp.  Per channel: one
    // v_perm_b32 per row puts the two taps side by side, one v_dot4_u32_u8 blends them horizontally, one multiply-add
    // vertically -- about half the integer work of the four-tap form (which stays for the un-snapped weights).
    bool done_sep = false;
    if constexpr (std::is_same<Taps, RunTaps>::value && sizeof(T) == 1) {
        if (fixed_u8 && sep) {
            const uint32_t wx = (uint32_t)(32 - tp.ax) | ((uint32_t)tp.ax << 8);
            const int wy0 = 32 - tp.ay, wy1 = tp.ay;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                constexpr uint32_t kZero = 0x0C0C0000u;                       // selector bytes 2, 3: constant 0
                const uint32_t sel = kZero | (uint32_t)c | ((uint32_t)(CT + c) << 8);
                const uint32_t t0 = __builtin_amdgcn_perm(taps.run[0][1], taps.run[0][0], sel), t1 = __builtin_amdgcn_perm(taps.run[1][1], taps.run[1][0], sel);
                const uint32_t h0 = __builtin_amdgcn_udot4(t0, wx, 0u, false), h1 = __builtin_amdgcn_udot4(t1, wx, 0u, false);
                res[c] = (T)((__umul24(h0, (uint32_t)wy0) + __umul24(h1, (uint32_t)wy1) + 512u) >> 10);
            }
            done_sep = true;
        }
    }
    if (!done_sep) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            A v[4];
            if constexpr (std::is_same<Taps, RunTaps>::value) {
                v[0] = (A)run_elem<T>(taps.run[0], c); v[1] = (A)run_elem<T>(taps.run[0], CT + c);
                v[2] = (A)run_elem<T>(taps.run[1], c); v[3] = (A)run_elem<T>(taps.run[1], CT + c);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = taps(k, c);
            }
            if constexpr (sizeof(T) == 8) {
                res[c] = (T)blend4d(v[0], v[1], v[2], v[3], tp);
            } else {
                if (fixed_u8) {
                    const int acc = __mul24((int)v[0], wi[0]) + __mul24((int)v[1], wi[1]) + __mul24((int)v[2], wi[2]) + __mul24((int)v[3], wi[3]);
                    res[c] = (T)min(max((acc + (1 << 14)) >> 15, 0), 255);
                } else {
                    res[c] = finish<T>(blend4((float)v[0], (float)v[1], (float)v[2], (float)v[3], tp), arith);
                }
            }
        }
    }
    ok = false;
    if (want_valid) {
        if (rule == OFL_RULE_GE_HALF) {
            const int acc = __mul24(m[0], wi[0]) + __mul24(m[1], wi[1]) + __mul24(m[2], wi[2]) + __mul24(m[3], wi[3]);
            ok = ((acc + (1 << 14)) >> 15) == 1;
        } else {
            const float sm = blend4((float)m[0], (float)m[1], (float)m[2], (float)m[3], tp);
            ok = (rule == OFL_RULE_EQ1) ? (sm == 1.0f) : (cv_round(sm) == 1);
        }
    }
}

// One pixel at a time: the taps are asked for (predicated, or unpredicated when the wave is INSIDE the source) and blended at once.
template <typename T, int CT, bool INSIDE>
__device__ __forceinline__ void gather_px(const T *__restrict__ src, const uint8_t *__restrict__ smask, int H, int W,
                                          const Tap &tp, const int (&wi)[4], bool fixed_u8, bool sep, int arith, int rule,
                                          bool want_valid, T (&res)[CT], bool &ok)
{
    bool     in[4];
    uint32_t off[4];          // 32-bit offsets (the paired kernel takes images below 4 GiB): scalar base + 32-bit lane offset, no 64-bit address math
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = tp.iy + (k >> 1), xx = tp.ix + (k & 1);
        in[k]  = INSIDE ? true : ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W);
        off[k] = in[k] ? __umul24((uint32_t)yy, (uint32_t)W) + (uint32_t)xx : 0u;
    }
    // the mask taps are requested BEFORE the image taps (their latency hides behind the image loads); inside the
    // image the two taps of a row are one 2-byte load (unaligned addresses are fine for global loads on gfx950)
    int m[4] = { 0, 0, 0, 0 };
    if (want_valid) {
        if (!smask) {
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = in[k] ? 1 : 0;
        } else if (INSIDE) {
            const uint32_t r0 = *reinterpret_cast<const uint16_t *>(smask + off[0]), r1 = *reinterpret_cast<const uint16_t *>(smask + off[2]);
            m[0] = (r0 & 0xffu) != 0; m[1] = (r0 & 0xff00u) != 0; m[2] = (r1 & 0xffu) != 0; m[3] = (r1 & 0xff00u) != 0;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = in[k] ? (smask[off[k]] != 0) : 0;
        }
    }
    typedef typename Acc<T>::type A;
    // 8- and 16-bit images inside the source: the two taps of a row are 2 * CT adjacent elements = 2 .. 16 bytes,
    // fetched as one or two wide loads per row instead of 2 * CT element loads (unaligned global loads are fine)
    constexpr bool kRun = INSIDE && PxRun<T, CT>::value;
    if constexpr (kRun) {
        uint32_t run[2][4] = { { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u } };
        constexpr int kRB = 2 * CT * (int)sizeof(T);
        // 6- and 12-byte runs are read as ONE 8- / 16-byte load (two or four bytes too many) wherever that stays inside the
        // image -- everywhere but the last pixels of the last row
        const uint32_t total = (uint32_t)H * (uint32_t)W * (uint32_t)(CT * sizeof(T));
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t at = off[2 * r] * (uint32_t)(CT * sizeof(T));
            const uint8_t *pr = reinterpret_cast<const uint8_t *>(src) + at;
            if constexpr (kRB == 6 || kRB == 12) {
                if (at + kRB + kRB / 3 <= total) load_run<kRB + kRB / 3>(pr, run[r]);
                else                             load_run<kRB>(pr, run[r]);
            } else load_run<kRB>(pr, run[r]);
        }
        blend_taps<T, CT>(RunTaps{ run }, m, tp, wi, fixed_u8, sep, arith, rule, want_valid, res, ok);
    } else {
        // (one zero-extended base per tap: the channel loads still merge)
        blend_taps<T, CT>([&](int k, int c) { return in[k] ? (A)(src + off[k] * (uint32_t)CT)[c] : (A)0; },
                          m, tp, wi, fixed_u8, sep, arith, rule, want_valid, res, ok);
    }
}

// ---- the all-inside path in two phases: every pixel's loads are issued before the first pixel is blended ----
// gather_px asks for a pixel's taps and blends them at once; four pixels of a lane one after the other are four dependent
// rounds of loads behind the round of the flow itself (PMC: a wave of the 8-bit kernel lives 11.9 us for 2 000 cycles of
// instructions, 70 % of it waiting; six waves per SIMD cannot hide five rounds of 2.3 us).  For a wave whose taps are all inside
// the source -- nearly every wave -- the loads need no predication: px_load asks for all of them, px_blend hands
// what they return to blend_taps.  Same values, same operations, same order per pixel: the same bits.
template <typename T, int CT>
struct PxLoad {
    uint32_t run[2][4];                              // PxRun: the two taps of a row as one run of 2 * CT elements
    typename Acc<T>::type v[PxRun<T, CT>::value ? 1 : 4][PxRun<T, CT>::value ? 1 : CT];      // otherwise: tap by tap
    uint32_t m01, m23;                               // the source mask's two bytes per row
};

template <typename T, int CT, bool WIDE>        // WIDE: 6- and 12-byte runs may be read as 8 / 16 bytes (the caller checked the image's end)
__device__ __forceinline__ void px_load(const T *__restrict__ src, const uint8_t *__restrict__ smask, int W, int ix, int iy,
                                        bool want_valid, PxLoad<T, CT> &L)
{
    const uint32_t off0 = __umul24((uint32_t)iy, (uint32_t)W) + (uint32_t)ix, off2 = off0 + (uint32_t)W;
    L.m01 = L.m23 = 0x0101u;
    if (want_valid && smask) {
        L.m01 = *reinterpret_cast<const uint16_t *>(smask + off0);
        L.m23 = *reinterpret_cast<const uint16_t *>(smask + off2);
    }
    if constexpr (PxRun<T, CT>::value) {
        constexpr int kRB = 2 * CT * (int)sizeof(T);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            L.run[r][0] = L.run[r][1] = L.run[r][2] = L.run[r][3] = 0u;
            const uint8_t *pr = reinterpret_cast<const uint8_t *>(src) + (r ? off2 : off0) * (uint32_t)(CT * sizeof(T));
            if constexpr ((kRB == 6 || kRB == 12) && WIDE) load_run<kRB + kRB / 3>(pr, L.run[r]);
            else load_run<kRB>(pr, L.run[r]);
        }
    } else {
        typedef typename Acc<T>::type A;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const T *t = src + ((k >> 1) ? off2 : off0) * (uint32_t)CT + (uint32_t)((k & 1) * CT);
#pragma unroll
            for (int c = 0; c < CT; ++c) L.v[k][c] = (A)t[c];
        }
    }
}

template <typename T, int CT>
__device__ __forceinline__ void px_blend(const PxLoad<T, CT> &L, const Tap &tp, const int (&wi)[4], bool fixed_u8, bool sep, int arith, int rule,
                                         bool want_valid, T (&res)[CT], bool &ok)
{
    const int m[4] = { (L.m01 & 0xffu) != 0, (L.m01 & 0xff00u) != 0, (L.m23 & 0xffu) != 0, (L.m23 & 0xff00u) != 0 };
    if constexpr (PxRun<T, CT>::value) {
        blend_taps<T, CT>(RunTaps{ L.run }, m, tp, wi, fixed_u8, sep, arith, rule, want_valid, res, ok);
    } else {
        blend_taps<T, CT>([&](int k, int c) { return L.v[k][c]; }, m, tp, wi, fixed_u8, sep, arith, rule, want_valid, res, ok);
    }
}

// taps, gather and blend of four pixels (gx[j], y) of one lane; wave-uniform all-outside / all-inside / border paths
template <typename T, int CT>
__device__ __forceinline__ void gather2_core(const T *__restrict__ src, const uint8_t *__restrict__ smask, int H, int W,
                                             const int (&gx)[4], int y, const bool (&act4)[4],
                                             const float (&fu)[4], const float (&fv)[4], int sign,
                                             int quant, int arith, int rule, bool want_valid,
                                             T (&res)[4][CT], bool (&ok)[4])
{
    Tap  tp[4];
    int  wi[4][4];
    bool inside = true, outside = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // float32(float64(grid) +- float64(flow)) of utils.py:231-235 as ONE float32 operation: exact for integer grid
        // coordinates below 2^15 (proof at c3_pos; the float64 form costs a dozen half-rate instructions per pixel)
        const float px = sign >= 0 ? __fadd_rn((float)gx[j], fu[j]) : __fsub_rn((float)gx[j], fu[j]);
        const float py = sign >= 0 ? __fadd_rn((float)y, fv[j]) : __fsub_rn((float)y, fv[j]);
        tp[j] = (quant == OFL_QUANT_OPENCV) ? make_tap<OFL_QUANT_OPENCV>(px, py) : make_tap<OFL_QUANT_EXACT>(px, py);
        if (quant == OFL_QUANT_OPENCV) {
            wi[j][0] = __mul24(32 - tp[j].ay, 32 - tp[j].ax) * 32; wi[j][1] = __mul24(32 - tp[j].ay, tp[j].ax) * 32;
            wi[j][2] = __mul24(tp[j].ay, 32 - tp[j].ax) * 32;      wi[j][3] = __mul24(tp[j].ay, tp[j].ax) * 32;
        } else {
            wi[j][0] = __float2int_rn(tp[j].w0 * 32768.0f); wi[j][1] = __float2int_rn(tp[j].w1 * 32768.0f);
            wi[j][2] = __float2int_rn(tp[j].w2 * 32768.0f); wi[j][3] = __float2int_rn(tp[j].w3 * 32768.0f);
        }
        const bool in_j  = (unsigned)tp[j].ix <= (unsigned)(W - 2) && (unsigned)tp[j].iy <= (unsigned)(H - 2);
        bool out_j = tp[j].ix < -1 || tp[j].ix >= W || tp[j].iy < -1 || tp[j].iy >= H;
        // un-snapped weights of a NaN or Inf coordinate are NaN, and so is their blend of four zeros (the oracle's 0 * NaN): such a
        // pixel takes the border path, which multiplies, and never the shortcut that writes 0 for a whole wave
        if (quant != OFL_QUANT_OPENCV) out_j = out_j && (tp[j].w0 == tp[j].w0) && (tp[j].w3 == tp[j].w3);
        inside  = inside && (in_j || !act4[j]);
        outside = outside && (out_j || !act4[j]);
    }
    if (H < 2) inside = false;
    const bool fixed_u8 = (sizeof(T) == 1) && arith == OFL_ARITH_NATIVE;

#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ok[j] = false;
#pragma unroll
        for (int c = 0; c < CT; ++c) res[j][c] = (T)0;
    }
    const bool all_outside = __all(outside), all_inside = !all_outside && __all(inside);
    if (all_outside) {
        // nothing to fetch: every tap of every pixel of this wave is outside the source
    } else if (all_inside && sizeof(T) < 8) {
        // (float64 images keep the one-pixel-at-a-time form: their taps alone are 4 * CT * 2 registers per pixel)
        constexpr int kRB = 2 * CT * (int)sizeof(T);
        constexpr bool kPadded = PxRun<T, CT>::value && (kRB == 6 || kRB == 12);
        bool wide = true;                            // may every 6- / 12-byte run of this lane be read as 8 / 16 bytes?
        if constexpr (kPadded) {
            const uint32_t total = (uint32_t)H * (uint32_t)W * (uint32_t)(CT * sizeof(T));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (act4[j]) wide = wide && (__umul24((uint32_t)(tp[j].iy + 1), (uint32_t)W) + (uint32_t)tp[j].ix) * (uint32_t)(CT * sizeof(T)) + kRB + kRB / 3 <= total;
        }
        // pixels in flight together: all four when a pixel's taps are runs (<= 8 registers), two otherwise (float images of 3 / 4
        // channels: 12 / 16 registers per pixel)
        constexpr int kGroup = PxRun<T, CT>::value ? 4 : 2;
        const bool all_wide = __all(wide);
        int lix[4], liy[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { lix[j] = act4[j] ? tp[j].ix : 0; liy[j] = act4[j] ? tp[j].iy : 0; }      // (a pixel off the frame reads the image's first taps)
#pragma unroll
        for (int j0 = 0; j0 < 4; j0 += kGroup) {
            PxLoad<T, CT> L[kGroup];
            if (all_wide) {                          // (the branch around the whole group, not inside it: each load phase is straight-line code)
#pragma unroll
                for (int j = 0; j < kGroup; ++j) px_load<T, CT, true>(src, smask, W, lix[j0 + j], liy[j0 + j], want_valid, L[j]);
            } else {
#pragma unroll
                for (int j = 0; j < kGroup; ++j) px_load<T, CT, false>(src, smask, W, lix[j0 + j], liy[j0 + j], want_valid, L[j]);
            }
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
                if (act4[j0 + j]) px_blend<T, CT>(L[j], tp[j0 + j], wi[j0 + j], fixed_u8, quant == OFL_QUANT_OPENCV, arith, rule, want_valid, res[j0 + j], ok[j0 + j]);
        }
    } else if (all_inside) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (act4[j]) gather_px<T, CT, true>(src, smask, H, W, tp[j], wi[j], fixed_u8, quant == OFL_QUANT_OPENCV, arith, rule, want_valid, res[j], ok[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (act4[j]) gather_px<T, CT, false>(src, smask, H, W, tp[j], wi[j], fixed_u8, quant == OFL_QUANT_OPENCV, arith, rule, want_valid, res[j], ok[j]);
    }

}

// SPEC: the (quant, arith, rule) triple as compile-time constants for the combinations the Flow algebra actually asks for --
// 1 = cv2's 1/32-px snap + uint8 fixed point + `>= 1/2` (a uint8 image with a boolean mask, flow_class.py:644), 2 = the snap +
// float accumulate + `== 1` (float images and Flow targets), 3 = the snap + float sum rounded half to even + `> 1/2` (a uint8 image
// with the default mask: an int16 concat, flow_class.py:615); 0 = whatever the arguments say.  Same code, the branches folded.
// (4 = 2 held to five waves per SIMD: the folded float kernel needs 74 VGPRs instead of 90, and the sixth wave that buys is worth 5 % on
// config 2 and COSTS 5 % on config 5 't', whose scattered taps of a 400 MB image thrash the caches -- the launcher picks by the source's size)
template <typename T, int CT, int SPEC = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, SPEC == 4 ? 5 : 8)))
void gather2_kernel(const T *__restrict__ src0, int H, int W,
                    const float *__restrict__ flow0, int fH, int fW, int pad_top, int pad_left, int sign,
                    const uint8_t *__restrict__ smask0, const uint8_t *__restrict__ fmask0,
                    T *__restrict__ dst0, uint8_t *__restrict__ valid0,
                    int quant, int arith, int rule, int tiles_x, int row0, int rows, GBatch bs)
{
    if (SPEC == 1) { quant = OFL_QUANT_OPENCV; arith = OFL_ARITH_NATIVE; rule = OFL_RULE_GE_HALF; }
    if (SPEC == 2 || SPEC == 4) { quant = OFL_QUANT_OPENCV; arith = OFL_ARITH_NATIVE; rule = OFL_RULE_EQ1; }
    if (SPEC == 3) { quant = OFL_QUANT_OPENCV; arith = OFL_ARITH_FLOAT_RNE; rule = OFL_RULE_GT_HALF; }
    // (batched launches: one field per blockIdx.y; the offsets below stay 32-bit relative to the FIELD's base pointers)
    const size_t bi = blockIdx.y;
    const T *__restrict__ src = src0 + bi * bs.src;
    const float *__restrict__ flow = flow0 + bi * bs.flow;
    const uint8_t *__restrict__ smask = smask0 ? smask0 + bi * bs.smask : nullptr;
    const uint8_t *__restrict__ fmask = fmask0 ? fmask0 + bi * bs.fmask : nullptr;
    T *__restrict__ dst = dst0 + bi * bs.dst;
    uint8_t *__restrict__ valid = valid0 ? valid0 + bi * bs.valid : nullptr;
    const int tile = blockIdx.x;
    const int ty   = tile / tiles_x, tx = tile - ty * tiles_x;
    const int lx   = threadIdx.x & 31, yl = ty * 8 + (threadIdx.x >> 5), y = row0 + yl;     // output band [row0, row0 + rows)
    const int xg[2] = { tx * 128 + 2 * lx, tx * 128 + 64 + 2 * lx };
    const bool act[2] = { yl < rows && xg[0] < W, yl < rows && xg[1] < W };
    const int  fy = y - pad_top;
    const bool row_in_flow = (unsigned)fy < (unsigned)fH;
    const bool aligned = ((pad_left | fW) & 1) == 0;          // 16-byte aligned flow pairs

    float fu[4], fv[4];
    bool  inf[4];
    uint32_t fmw[2] = { 0u, 0u };          // flow-mask bytes of the pixel pairs, fetched with the flow (not at the store)
    // The common wave -- both pixel pairs of every lane inside the flow area, pairs 16-byte aligned -- asks for its two vector
    // pairs and its two mask words in one go; the general form below predicates every load and waits for each (its loads sit in
    // divergent branches: four dependent rounds of loads before the first tap is asked for).
    const bool whole = aligned && act[0] && act[1] && row_in_flow && (unsigned)(xg[0] - pad_left) < (unsigned)fW && (unsigned)(xg[0] - pad_left + 1) < (unsigned)fW &&
                       (unsigned)(xg[1] - pad_left) < (unsigned)fW && (unsigned)(xg[1] - pad_left + 1) < (unsigned)fW;
    if (__all(whole)) {
        const uint32_t o0 = __umul24((uint32_t)fy, (uint32_t)fW) + (uint32_t)(xg[0] - pad_left), o1 = __umul24((uint32_t)fy, (uint32_t)fW) + (uint32_t)(xg[1] - pad_left);
        const float4 f0 = *reinterpret_cast<const float4 *>(flow + o0 * 2), f1 = *reinterpret_cast<const float4 *>(flow + o1 * 2);
        if (fmask && valid) {
            fmw[0] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(fmask + o0));
            fmw[1] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(fmask + o1));
        }
        fu[0] = f0.x; fv[0] = f0.y; fu[1] = f0.z; fv[1] = f0.w; fu[2] = f1.x; fv[2] = f1.y; fu[3] = f1.z; fv[3] = f1.w;
        inf[0] = inf[1] = inf[2] = inf[3] = true;
    } else
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int fx = xg[g] - pad_left;
        inf[2 * g]     = act[g] && row_in_flow && (unsigned)fx < (unsigned)fW;
        inf[2 * g + 1] = act[g] && row_in_flow && (unsigned)(fx + 1) < (unsigned)fW;
        fu[2 * g] = fv[2 * g] = fu[2 * g + 1] = fv[2 * g + 1] = 0.0f;
        if (fmask && valid) {
            if (aligned && inf[2 * g] && inf[2 * g + 1]) {
                fmw[g] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(fmask + __umul24((uint32_t)fy, (uint32_t)fW) + (uint32_t)fx));
            } else {
                if (inf[2 * g]) fmw[g] |= fmask[__umul24((uint32_t)fy, (uint32_t)fW) + (uint32_t)fx];
                if (inf[2 * g + 1]) fmw[g] |= (uint32_t)fmask[__umul24((uint32_t)fy, (uint32_t)fW) + (uint32_t)fx + 1] << 8;
            }
        }
        if (aligned && inf[2 * g] && inf[2 * g + 1]) {
            const float4 f = *reinterpret_cast<const float4 *>(flow + (__umul24((uint32_t)fy, (uint32_t)fW) + (uint32_t)fx) * 2);
            fu[2 * g] = f.x; fv[2 * g] = f.y; fu[2 * g + 1] = f.z; fv[2 * g + 1] = f.w;
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (inf[2 * g + e]) {
                    const float2 f = *reinterpret_cast<const float2 *>(flow + (__umul24((uint32_t)fy, (uint32_t)fW) + (uint32_t)fx + e) * 2);
                    fu[2 * g + e] = f.x; fv[2 * g + e] = f.y;
                }
        }
    }

    const bool want_valid = valid != nullptr;
    T    res[4][CT];
    bool ok[4];
    // transposed gather for rotated sampling grids (see K2's transposed-gather form) -- float images with 3 or 4 channels only:
    // measured +10 % on a 30-degree grid.  For 1 / 2 channels and for 8- / 16-bit images the extra registers cost a wave
    // of occupancy (and the byte-wise LDS hand-over is slow), which loses more than the fewer tag look-ups save.
    constexpr bool kXp = sizeof(T) == 4 && CT >= 3;
    __shared__ __attribute__((aligned(16))) float2  xp_f[kXp ? 8 * kXpRowF2 : 1];
    __shared__ __attribute__((aligned(16))) T       xp_r[kXp ? 8 * 128 * CT : 1];
    __shared__ __attribute__((aligned(16))) uint8_t xp_k[kXp ? 8 * 128 : 1];
    bool rotated = false;
    if constexpr (kXp) {
        // uniform decision from the vertical flow at the two ends of the tile's first row (zero outside the flow area)
        const int x0 = tx * 128, x1 = min(x0 + 127, W - 1), y0 = row0 + min(ty * 8, rows - 1);
        const int fy0 = y0 - pad_top, fxa = x0 - pad_left, fxb = x1 - pad_left;
        const bool rin = (unsigned)fy0 < (unsigned)fH;
        const float va = (rin && (unsigned)fxa < (unsigned)fW) ? flow[((size_t)fy0 * fW + fxa) * 2 + 1] : 0.0f;
        const float vb = (rin && (unsigned)fxb < (unsigned)fW) ? flow[((size_t)fy0 * fW + fxb) * 2 + 1] : 0.0f;
        rotated = fabsf(vb - va) * 128.0f > (float)(kXposeRows * (x1 - x0 + 1));
    }
    if (!rotated) {
        const int  gx[4]   = { xg[0], xg[0] + 1, xg[1], xg[1] + 1 };
        const bool act4[4] = { act[0], act[0], act[1], act[1] };
        gather2_core<T, CT>(src, smask, H, W, gx, y, act4, fu, fv, sign, quant, arith, rule, want_valid, res, ok);
    } else if constexpr (kXp) {
        const int ly = threadIdx.x >> 5;
        *reinterpret_cast<float4 *>(&xp_f[ly * kXpRowF2 + 2 * lx])      = make_float4(fu[0], fv[0], fu[1], fv[1]);
        *reinterpret_cast<float4 *>(&xp_f[ly * kXpRowF2 + 64 + 2 * lx]) = make_float4(fu[2], fv[2], fu[3], fv[3]);
        __syncthreads();
        // block layout: wave w owns columns [32 w, 32 w + 32) of the 8 rows; gather instruction j covers the 8 x 8 block
        // of columns 8 j .. 8 j + 7
        const int w4 = threadIdx.x >> 6, l = threadIdx.x & 63, r = l >> 3, c0 = 32 * w4 + (l & 7);
        {
            const int ylb = ty * 8 + r;
            int   gxb[4];
            bool  actb[4];
            float fub[4], fvb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 f = xp_f[r * kXpRowF2 + c0 + 8 * j];
                fub[j] = f.x; fvb[j] = f.y;
                gxb[j] = tx * 128 + c0 + 8 * j;
                actb[j] = ylb < rows && gxb[j] < W;
            }
            T    resb[4][CT];
            bool okb[4];
            gather2_core<T, CT>(src, smask, H, W, gxb, row0 + ylb, actb, fub, fvb, sign, quant, arith, rule, want_valid, resb, okb);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int c = 0; c < CT; ++c) xp_r[(r * 128 + c0 + 8 * j) * CT + c] = resb[j][c];
                xp_k[r * 128 + c0 + 8 * j] = okb[j] ? 1 : 0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = (j >> 1) * 64 + 2 * lx + (j & 1);
#pragma unroll
            for (int c = 0; c < CT; ++c) res[j][c] = xp_r[(ly * 128 + col) * CT + c];
            ok[j] = xp_k[ly * 128 + col] != 0;
        }
    }

    uint32_t vword[2] = { 0u, 0u };
    // 8- and 16-bit results leave as DWORDS as well: the two pixels of a lane are 2 .. 16 bytes; 2- and 6-byte pairs are
    // joined with the neighbouring lane's (four consecutive pixels = 4 / 12 bytes, dword-aligned when W is a multiple of 4).
    // Element-wise byte stores made this kernel instruction-bound: RGB uint8 cost 12 stores per lane, now 3 per lane PAIR.
    constexpr int kPB = 2 * CT * (int)sizeof(T);          // bytes of a pixel pair
    constexpr bool kPack = sizeof(T) <= 2;
    const bool quad4 = (W & 3) == 0;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const uint32_t o = __umul24((uint32_t)yl, (uint32_t)W) + (uint32_t)xg[g];
        if constexpr (kPack) {
            uint32_t pw[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
            for (int i = 0; i < 2 * CT; ++i) {
                const uint32_t v = (uint32_t)(typename std::make_unsigned<T>::type)res[2 * g + i / CT][i % CT];
                if constexpr (sizeof(T) == 1) pw[i >> 2] |= v << (8 * (i & 3));
                else                          pw[i >> 1] |= v << (16 * (i & 1));
            }
            uint8_t *d8 = reinterpret_cast<uint8_t *>(dst) + o * (uint32_t)(CT * sizeof(T));
            if constexpr (kPB == 2 || kPB == 6) {
                const uint32_t q0 = (uint32_t)__shfl_xor((int)pw[0], 1), q1 = (uint32_t)__shfl_xor((int)pw[1], 1);
                if (quad4) {
                    if (act[g] && (lx & 1) == 0) {
                        if constexpr (kPB == 2) {
                            *reinterpret_cast<uint32_t *>(d8) = pw[0] | (q0 << 16);
                        } else {
                            uint32_t *d32 = reinterpret_cast<uint32_t *>(d8);
                            d32[0] = pw[0]; d32[1] = pw[1] | (q0 << 16); d32[2] = (q0 >> 16) | (q1 << 16);
                        }
                    }
                } else if (act[g]) {
                    if constexpr (kPB == 2) *reinterpret_cast<uint16_t *>(d8) = (uint16_t)pw[0];
                    else { *reinterpret_cast<uint16_t *>(d8) = (uint16_t)pw[0]; *reinterpret_cast<uint16_t *>(d8 + 2) = (uint16_t)(pw[0] >> 16);
                           *reinterpret_cast<uint16_t *>(d8 + 4) = (uint16_t)pw[1]; }
                }
            } else if (act[g]) {
                if constexpr (kPB == 4)       *reinterpret_cast<uint32_t *>(d8) = pw[0];
                else if constexpr (kPB == 8)  *reinterpret_cast<uint2 *>(d8) = make_uint2(pw[0], pw[1]);
                else if constexpr (kPB == 12) { uint32_t *d32 = reinterpret_cast<uint32_t *>(d8); d32[0] = pw[0]; d32[1] = pw[1]; d32[2] = pw[2]; }
                else                          *reinterpret_cast<uint4 *>(d8) = make_uint4(pw[0], pw[1], pw[2], pw[3]);
            }
        } else if (act[g]) {
            T *d = dst + o * (uint32_t)CT;
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int c = 0; c < CT; ++c) d[e * CT + c] = res[2 * g + e][c];
        }
        if (act[g] && want_valid) {
            uint32_t m = (ok[2 * g] ? 1u : 0u) | (ok[2 * g + 1] ? 0x100u : 0u);
            if (fmask) m &= ((fmw[g] & 0xffu) ? 1u : 0u) | ((fmw[g] & 0xff00u) ? 0x100u : 0u);
            vword[g] = m;
        }
    }
    if (want_valid) {
        // Validity bytes leave as DWORDS: the lane pairs (2k, 2k + 1) own four consecutive pixels, the even lane
        // stores both lanes' bytes -- sub-dword stores cost as much per instruction as 16-byte ones.
        const bool quad = (W & 3) == 0;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint32_t other = (uint32_t)__shfl_xor((int)vword[g], 1);
            if (!act[g]) continue;
            const uint32_t o = __umul24((uint32_t)yl, (uint32_t)W) + (uint32_t)xg[g];
            if (quad) {
                if ((lx & 1) == 0) __builtin_nontemporal_store(vword[g] | (other << 16), reinterpret_cast<uint32_t *>(valid + o));
            } else {
                __builtin_nontemporal_store((uint16_t)vword[g], reinterpret_cast<uint16_t *>(valid + o));
            }
        }
    }
}

// One K1 launch as gather_rows_impl checked it: the kernels' arguments, the batch, and which source arrays the batch shares.
struct GArgs {
    const void *src; int C, H, W;
    const float *flow; int fH, fW, pad_top, pad_left, sign;
    const uint8_t *smask, *fmask;
    void *dst; uint8_t *valid;
    int quant, arith, rule, row0, rows, batch;
    bool shared_src, shared_smask;
};

template <typename T>
int launch_gather_t(const GArgs &g, hipStream_t s)
{
    const int C = g.C, H = g.H, W = g.W;
    GBatch bs;
    bs.src = g.shared_src ? 0 : (size_t)H * W * C; bs.smask = g.shared_smask ? 0 : (size_t)H * W;
    bs.flow = (size_t)g.fH * g.fW * 2; bs.fmask = (size_t)g.fH * g.fW; bs.dst = (size_t)g.rows * W * C; bs.valid = (size_t)g.rows * W;
    // (the paired kernel addresses with 32-bit offsets: images, flows and results below 4 GiB)
    if (W % 2 == 0 && C >= 1 && C <= 4 && (unsigned long long)H * W * C * sizeof(T) < (1ull << 32) && (unsigned long long)g.fH * g.fW * 8 < (1ull << 32)) {
        const int tiles_x = (W + 127) / 128, tiles_y = (g.rows + 7) / 8;
        const int nblocks = tiles_x * tiles_y;
#define OFL_GATHER2_LAUNCH(CT, SPEC)                                                                     \
        hipLaunchKernelGGL((gather2_kernel<T, CT, SPEC>), dim3(nblocks, g.batch), dim3(256), 0, s, (const T *)g.src, H, W, \
                           g.flow, g.fH, g.fW, g.pad_top, g.pad_left, g.sign, g.smask, g.fmask, (T *)g.dst, g.valid, g.quant,   \
                           g.arith, g.rule, tiles_x, g.row0, g.rows, bs)
#define OFL_GATHER2_LAUNCH_C(SPEC)      /* (C is 1 .. 4 here) */                                          \
        do { if (C == 1) OFL_GATHER2_LAUNCH(1, SPEC); else if (C == 2) OFL_GATHER2_LAUNCH(2, SPEC);       \
             else if (C == 3) OFL_GATHER2_LAUNCH(3, SPEC); else OFL_GATHER2_LAUNCH(4, SPEC); } while (0)
        // the combinations the Flow algebra asks for run as specialised instantiations (same code, branches folded: 7 - 10 % faster)
        int spec = 0;
        if (g.quant == OFL_QUANT_OPENCV) {
            if (std::is_same<T, uint8_t>::value && g.arith == OFL_ARITH_NATIVE && g.rule == OFL_RULE_GE_HALF) spec = 1;
            else if (std::is_same<T, float>::value && g.arith == OFL_ARITH_NATIVE && g.rule == OFL_RULE_EQ1)
                spec = (unsigned long long)H * W * C * sizeof(T) > (128ull << 20) ? 4 : 2;      // a source beyond half the Infinity Cache: five waves
            else if (std::is_same<T, uint8_t>::value && g.arith == OFL_ARITH_FLOAT_RNE && g.rule == OFL_RULE_GT_HALF) spec = 3;
        }
        if constexpr (std::is_same<T, uint8_t>::value || std::is_same<T, float>::value) {
            constexpr int kA = std::is_same<T, float>::value ? 2 : 1, kB = std::is_same<T, float>::value ? 4 : 3;      // the specialisations of this type
            if (spec == kA) OFL_GATHER2_LAUNCH_C(kA); else if (spec == kB) OFL_GATHER2_LAUNCH_C(kB);
        }
        if (spec == 0) OFL_GATHER2_LAUNCH_C(0);
#undef OFL_GATHER2_LAUNCH_C
#undef OFL_GATHER2_LAUNCH
        OFL_HIP(hipGetLastError());
        return OFL_OK;
    }
    const int tiles_x = (W + 31) / 32, tiles_y = (g.rows + 7) / 8;
    const int nblocks = tiles_x * tiles_y;
#define OFL_GATHER_LAUNCH(CT)                                                                          \
    hipLaunchKernelGGL((gather_kernel<T, CT>), dim3(nblocks, g.batch), dim3(256), 0, s, (const T *)g.src, C, H, W, \
                       g.flow, g.fH, g.fW, g.pad_top, g.pad_left, g.sign, g.smask, g.fmask, (T *)g.dst, g.valid, g.quant,     \
                       g.arith, g.rule, tiles_x, nblocks, g.row0, g.rows, bs)
    switch (C) {
    case 1: OFL_GATHER_LAUNCH(1); break;
    case 2: OFL_GATHER_LAUNCH(2); break;
    case 3: OFL_GATHER_LAUNCH(3); break;
    case 4: OFL_GATHER_LAUNCH(4); break;
    default: OFL_GATHER_LAUNCH(0); break;
    }
#undef OFL_GATHER_LAUNCH
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

size_t dtype_size(int dtype)
{
    switch (dtype) {
    case OFL_U8: return 1;
    case OFL_I16: case OFL_U16: return 2;
    case OFL_F32: return 4;
    case OFL_F64: return 8;
    default: return 0;
    }
}

}  // namespace

extern "C" {

static int gather_rows_impl(const void *src, int dtype, int C, int H, int W,
                            const float *flow, int fH, int fW, int pad_top, int pad_left, int sign,
                            const uint8_t *smask, const uint8_t *fmask,
                            void *dst, uint8_t *valid,
                            int quant, int arith, int rule, int row0, int rows, void *stream,
                            int batch = 1, bool shared_src = false, bool shared_smask = false)
{
    OFL_TRY(need_device());
    OFL_TRY(check_field_dims("ofl_gather_bilinear", H, W));
    if (!flow) return fail(OFL_E_INVALID, "ofl_gather_bilinear: NULL flow");
    if (C == 0) {   // validity-only launch: no image channels are read or written
        if (src || dst || !valid) return fail(OFL_E_INVALID, "ofl_gather_bilinear: C == 0 needs src = dst = NULL and valid != NULL");
        dtype = OFL_U8;
    } else if (!src || !dst) {
        return fail(OFL_E_INVALID, "ofl_gather_bilinear: NULL pointer");
    }
    if (C < 0) return fail(OFL_E_INVALID, "ofl_gather_bilinear: C must be >= 0");
    if (dtype_size(dtype) == 0) return fail(OFL_E_INVALID, "ofl_gather_bilinear: unsupported dtype %d", dtype);
    if (fH <= 0 || fW <= 0 || pad_top < 0 || pad_left < 0 || pad_top + fH > H || pad_left + fW > W)
        return fail(OFL_E_INVALID, "ofl_gather_bilinear: flow %dx%d at (%d,%d) does not fit target %dx%d",
                    fH, fW, pad_top, pad_left, H, W);
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "ofl_gather_bilinear: sign must be +1 or -1");
    if (quant != OFL_QUANT_OPENCV && quant != OFL_QUANT_EXACT) return fail(OFL_E_INVALID, "ofl_gather_bilinear: bad quant");
    if (rule < OFL_RULE_EQ1 || rule > OFL_RULE_GT_HALF) return fail(OFL_E_INVALID, "ofl_gather_bilinear: bad rule");
    if (arith != OFL_ARITH_NATIVE && arith != OFL_ARITH_FLOAT_RNE) return fail(OFL_E_INVALID, "ofl_gather_bilinear: bad arith");
    if (row0 < 0 || rows <= 0 || row0 + rows > H)
        return fail(OFL_E_INVALID, "ofl_gather_bilinear: rows [%d, %d) outside the %d-row result", row0, row0 + rows, H);
    hipStream_t s = stream_of(stream);
    const GArgs g = { src, C, H, W, flow, fH, fW, pad_top, pad_left, sign, smask, fmask, dst, valid,
                      quant, arith, rule, row0, rows, batch, shared_src, shared_smask };
    switch (dtype) {
    case OFL_U8:  return launch_gather_t<uint8_t>(g, s);
    case OFL_I16: return launch_gather_t<int16_t>(g, s);
    case OFL_U16: return launch_gather_t<uint16_t>(g, s);
    case OFL_F32: return launch_gather_t<float>(g, s);
    default:      return launch_gather_t<double>(g, s);
    }
}

int ofl_gather_bilinear_dev(const void *src, int dtype, int C, int H, int W,
                            const float *flow, int fH, int fW, int pad_top, int pad_left, int sign,
                            const uint8_t *smask, const uint8_t *fmask,
                            void *dst, uint8_t *valid,
                            int quant, int arith, int rule, void *stream)
{
    return gather_rows_impl(src, dtype, C, H, W, flow, fH, fW, pad_top, pad_left, sign, smask, fmask, dst, valid,
                            quant, arith, rule, 0, H, stream);
}

int ofl_gather_bilinear_batch_dev(const void *src, int src_shared, int dtype, int C, int H, int W, int batch,
                                  const float *flow, int fH, int fW, int pad_top, int pad_left, int sign,
                                  const uint8_t *smask, int smask_shared, const uint8_t *fmask,
                                  void *dst, uint8_t *valid, int quant, int arith, int rule, void *stream)
{
    if (batch < 1 || batch > 65535) return fail(OFL_E_INVALID, "ofl_gather_bilinear_batch: batch must be in [1, 65535]");
    return gather_rows_impl(src, dtype, C, H, W, flow, fH, fW, pad_top, pad_left, sign, smask, fmask, dst, valid,
                            quant, arith, rule, 0, H, stream, batch, src_shared != 0, smask_shared != 0);
}

int ofl_gather_rows_dev(const void *src, int dtype, int C, int H, int W, int row0, int rows,
                        const float *flow_rows, int sign, const uint8_t *smask, const uint8_t *fmask_rows,
                        void *dst_rows, uint8_t *valid_rows, int quant, int arith, int rule, void *stream)
{
    if (rows <= 0 || row0 < 0) return fail(OFL_E_INVALID, "ofl_gather_rows: bad row band");
    return gather_rows_impl(src, dtype, C, H, W, flow_rows, rows, W, row0, 0, sign, smask, fmask_rows, dst_rows, valid_rows,
                            quant, arith, rule, row0, rows, stream);
}

int ofl_gather_bilinear(const void *src, int dtype, int C, int H, int W,
                        const float *flow, int fH, int fW, int pad_top, int pad_left, int sign,
                        const uint8_t *smask, const uint8_t *fmask,
                        void *dst, uint8_t *valid,
                        int quant, int arith, int rule)
{
    OFL_TRY(need_device());
    OFL_TRY(check_field_dims("ofl_gather_bilinear", H, W));
    const size_t es = dtype_size(dtype);
    if (es == 0 || C <= 0) return fail(OFL_E_INVALID, "ofl_gather_bilinear: unsupported dtype/C");
    if (!src || !flow || !dst) return fail(OFL_E_INVALID, "ofl_gather_bilinear: NULL pointer");
    if (fH <= 0 || fW <= 0) return fail(OFL_E_INVALID, "ofl_gather_bilinear: bad flow shape");
    const size_t n = (size_t)H * W, nf = (size_t)fH * fW;
    HostStage st("ofl_gather_bilinear");
    auto dsrc = st.in(src, n * C * es);
    auto dflow = st.in(flow, nf * 2);
    auto dsm = st.in(smask, n), dfm = st.in(fmask, nf);
    auto ddst = st.out(dst, n * C * es);
    auto dval = st.out(valid, n);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_gather_bilinear_dev(dsrc, dtype, C, H, W, dflow, fH, fW, pad_top, pad_left, sign, dsm, dfm, ddst, dval,
                                    quant, arith, rule, st.stream()));
    return st.download();
}

}  // extern "C"
