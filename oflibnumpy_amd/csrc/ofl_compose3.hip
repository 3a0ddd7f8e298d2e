// ofl_compose3.hip -- K2, the fused mode-3 composition of two flow fields, and the packed mask planes it can read, for gfx950.
//
// An HBM-bound byte mover (no MFMA): every output pixel streams its vector of fb (coalesced, 16 B per lane), derives the
// cv2.remap sample position, and gathers the 2x2 neighbourhood of fa and of its mask.  The two horizontally adjacent taps of
// one source row are fetched with ONE 8-byte-aligned 16-byte load; reuse between neighbouring pixels is served by the per-CU
// L1 and the per-XCD L2, which is why workgroups own 2-D tiles.  Numerics follow oracle/ofl_oracle.c operation for operation
// (contraction disabled): the float results and the validity masks are bit-identical to the CPU restatement.
#include "ofl_common.h"
#include "ofl_host_stage.h"
#include "ofl_compose3_route.h"
#include "ofl_pairs.h"
#include <type_traits>

#pragma clang fp contract(off)

using namespace ofl;

namespace {

// Tap selection for a row pair loaded at the clamped column ixc: d = ix - ixc is 0 in the interior,
// -1 when the left tap hangs over the left edge, +1 when the right tap hangs over the right edge;
// anything else means both taps are outside.
__device__ __forceinline__ void select_pair(const Pair2 &p, int d, bool row_ok,
                                            float &u0, float &v0, float &u1, float &v1)
{
    bool lo0 = row_ok & (d == 0), hi0 = row_ok & (d == 1);
    bool hi1 = row_ok & (d == 0), lo1 = row_ok & (d == -1);
    u0 = lo0 ? p.lo_u : (hi0 ? p.hi_u : 0.0f);
    v0 = lo0 ? p.lo_v : (hi0 ? p.hi_v : 0.0f);
    u1 = hi1 ? p.hi_u : (lo1 ? p.lo_u : 0.0f);
    v1 = hi1 ? p.hi_v : (lo1 ? p.lo_v : 0.0f);
}

__device__ __forceinline__ void select_mask(uint32_t lo, uint32_t hi, int d, bool row_ok, float &m0, float &m1)
{
    bool lo0 = row_ok & (d == 0), hi0 = row_ok & (d == 1);
    bool hi1 = row_ok & (d == 0), lo1 = row_ok & (d == -1);
    m0 = (lo0 ? (lo != 0) : (hi0 ? (hi != 0) : false)) ? 1.0f : 0.0f;
    m1 = (hi1 ? (hi != 0) : (lo1 ? (lo != 0) : false)) ? 1.0f : 0.0f;
}

// Packed mask planes (device-resident chains, ofl_compose3_bits_dev): one BIT per pixel, bit x & 31 of the 32-bit word x >> 5,
// rows padded to whole words.  The three 1-byte mask streams of the fused compose are 3 of its 27 B/px by the contract but up
// to five times that in partially used 128-byte lines on a rotated sampling grid; as bit planes they are 0.4 B/px.
// taps (x, x + 1) of a plane row as bits 0 and 1 -- one 4-byte load from the byte that holds bit x (x & 7 <= 7: both bits lie
// within the 32; planes are allocated with 16 bytes of slack, ofl_mask_bits_bytes)
__device__ __forceinline__ uint32_t c3_bits_at(const uint8_t *plane_row, int x)
{
    return reinterpret_cast<const U32u *>(plane_row + (x >> 3))->v >> (x & 7);
}
__device__ __forceinline__ uint32_t c3_bit(const uint8_t *plane_row, int x) { return ((uint32_t)plane_row[x >> 3] >> (x & 7)) & 1u; }
// 16 bits -> the even bit positions of 32
__device__ __forceinline__ uint32_t c3_spread16(uint32_t x)
{
    x &= 0xFFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu; x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u; x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// Workgroup tile: 128 px x 8 rows, 256 threads.  Lane (lx, ly) owns the two pixel PAIRS at
// x = 2*lx and x = 64 + 2*lx of its tile row, so that every stream instruction of a wave covers
// contiguous memory (32 lanes x 16 B = 512 B of vectors, 32 lanes x 2 B = 64 B of mask per row):
// no half-filled 64-byte requests on either the read or the write side.
//
// Register budget (tests/test_k2_resources.py): kC3Waves per SIMD with no spills and <= 80 SGPRs, so that scalar registers
// never limit residency.  Only the interior gather is unrolled over a lane's four pixels; the border paths take one pixel
// (c3_border_px) or one pixel pair (c3_border_pair) per loop trip through the lane's LDS slots, sample positions stay in their compact form while the loads are in flight,
// and every address is a wave-uniform field base plus a 32-bit offset (ofl_compose3_route.h sends fields whose vector
// plane reaches 4 GiB to the generic kernel).
constexpr int kC3LanesX = 32;      // lanes along x per tile row: tile = 4*LX px x 256/LX rows
constexpr int kC3TileW = 4 * kC3LanesX, kC3TileH = 256 / kC3LanesX, kC3Px = 4;

// Sample position of one pixel in two registers: QUANT_OPENCV keeps cv2's 1/32-px fixed point (sx, sy), QUANT_EXACT the
// float32 coordinate itself (as bits).  The top-left tap and the fraction are derived where they are used.
struct C3Pos { int x, y; };

struct C3Tap {
    int   ax, ay;         // "fraction is non-zero" indicators for the validity test
    float w0, w1, w2, w3;
};

// Sample position: utils.py:231-235 evaluates float32(float64(grid) -/+ float64(flow)).  For an integer
// grid coordinate below 2^15 and any float32 flow value this equals the single float32 operation
// (the float64 sum is exact unless |flow| < 2^-14, and then it cannot land on a float32 rounding
// midpoint, whose distance from the integer is at least 2^-24 * 2^floor(log2 grid)), so one v_add_f32
// / v_sub_f32 reproduces NumPy bit for bit; tests compare against the float64 oracle.
template <int QUANT>
__device__ __forceinline__ C3Pos c3_pos(int gx, int gy, float fu, float fv, int sign)
{
    const float px = sign >= 0 ? __fadd_rn((float)gx, fu) : __fsub_rn((float)gx, fu);
    const float py = sign >= 0 ? __fadd_rn((float)gy, fv) : __fsub_rn((float)gy, fv);
    if (QUANT == OFL_QUANT_OPENCV) return { cv_round_coord(__fmul_rn(px, 32.0f)), cv_round_coord(__fmul_rn(py, 32.0f)) };
    return { __float_as_int(px), __float_as_int(py) };
}

// top-left tap along one axis
template <int QUANT>
__device__ __forceinline__ int c3_tap(int s)
{
    if (QUANT == OFL_QUANT_OPENCV) return s >> 5;      // unsaturated: beyond +-32767 every tap is outside anyway
    return (int)fminf(fmaxf(floorf(__int_as_float(s)), -32768.0f), 32767.0f);
}

// fractional position along one axis (multiples of 1/32 with cv2's snapping)
template <int QUANT>
__device__ __forceinline__ float c3_frac(int s)
{
    if (QUANT == OFL_QUANT_OPENCV) return (float)(s & 31) * (1.0f / 32.0f);
    const float p = __int_as_float(s);
    return __fsub_rn(p, floorf(p));
}

// Once a pixel's taps are addressed, QUANT_OPENCV weights need only the two 1/32-px fractions: one register instead of two.
__device__ __forceinline__ int   c3_pack_frac(const C3Pos &p) { return (p.x & 31) | ((p.y & 31) << 8); }
__device__ __forceinline__ C3Pos c3_unpack_frac(int f) { return { f & 0xff, f >> 8 }; }

// Bilinear weights from the fractional position; evaluated AFTER the gather has been issued so that
// they do not occupy registers while the loads are in flight.
template <int QUANT>
__device__ __forceinline__ C3Tap c3_weights(const C3Pos &p)
{
    C3Tap t;
    const float fx = c3_frac<QUANT>(p.x), fy = c3_frac<QUANT>(p.y);
    t.ax = (QUANT == OFL_QUANT_OPENCV) ? (fx != 0.0f) : 1;
    t.ay = (QUANT == OFL_QUANT_OPENCV) ? (fy != 0.0f) : 1;
    const float x0 = __fsub_rn(1.0f, fx), y0 = __fsub_rn(1.0f, fy);
    t.w0 = __fmul_rn(y0, x0); t.w1 = __fmul_rn(y0, fx);
    t.w2 = __fmul_rn(fy, x0); t.w3 = __fmul_rn(fy, fx);
    return t;
}

__device__ __forceinline__ float c3_blend(float v00, float v01, float v10, float v11, const C3Tap &t)
{
    float s = __fmul_rn(v00, t.w0);
    s = __fadd_rn(s, __fmul_rn(v01, t.w1));
    s = __fadd_rn(s, __fmul_rn(v10, t.w2));
    s = __fadd_rn(s, __fmul_rn(v11, t.w3));
    return s;
}

// "interpolated mask == 1" (flow_class.py:668).  With cv2's 1/32-px weights (multiples of 1/1024
// that sum to exactly 1) the float sum equals 1 iff every tap with a non-zero weight carries mask 1,
// which is pure integer logic; the un-snapped extension mode keeps the float comparison.
template <int QUANT>
__device__ __forceinline__ bool c3_valid(bool m00, bool m01, bool m10, bool m11, const C3Tap &t)
{
    if (QUANT == OFL_QUANT_OPENCV) {
        const bool zx = t.ax == 0, zy = t.ay == 0;
        return m00 & (m01 | zx) & (m10 | zy) & (m11 | zx | zy);
    }
    return c3_blend(m00 ? 1.0f : 0.0f, m01 ? 1.0f : 0.0f, m10 ? 1.0f : 0.0f, m11 ? 1.0f : 0.0f, t) == 1.0f;
}

struct C3Args {
    const float *fa; const uint8_t *ma; const float *fb; const uint8_t *mb;
    float *out; uint8_t *mout; uint32_t *stats;
    int sign, H, W, tiles_x, tiles_per_field, ntiles;
    float th;
    int mwpr;              // BITS kernels: 32-bit words per row of the packed mask planes ma / mb / mout (bit x & 31 of word x >> 5); else 0
};

// The planes of field pair b: wave-uniform bases (scalar registers); everything below adds an offset of type C3Ix to them.
struct C3Field {
    const float *fa, *fb; const uint8_t *ma, *mb;
    float *out; uint8_t *mout;
};

// Offsets within a field: 32 bits for the byte-mask kernels (the launcher keeps their fields below 4 GiB of vectors, so
// every address is one scalar base plus one 32-bit VGPR), size_t for the packed-mask ones, which have no generic fallback.
template <bool BITS> using C3Ix = typename std::conditional<BITS, size_t, uint32_t>::type;

template <typename T, typename Ix>
__device__ __forceinline__ T *c3_elem(T *base, Ix i)
{
    // the byte offset is formed in Ix so that a 32-bit one reaches the address unit as one VGPR next to the scalar base
    typedef typename std::conditional<std::is_const<T>::value, const char, char>::type C;
    return reinterpret_cast<T *>(reinterpret_cast<C *>(base) + (Ix)(i * (Ix)sizeof(T)));
}

// taps (s, s + 1) of a row of a float2 field
template <typename Ix>
__device__ __forceinline__ Pair2 c3_pair(const float *fa, Ix s) { return *reinterpret_cast<const Pair2 *>(c3_elem(fa, (Ix)(2 * s))); }

template <bool BITS>
__device__ __forceinline__ C3Field c3_field(const C3Args &a, int b)
{
    const size_t field = (size_t)b * a.H * a.W;
    const size_t mfield = BITS ? (size_t)b * a.H * a.mwpr * 4 : field;      // BITS: the field's bit planes, rows of mwpr words
    return { a.fa + 2 * field, a.fb + 2 * field, a.ma + mfield, a.mb + mfield, a.out + 2 * field, a.mout + mfield };
}

struct C3Stream {          // one lane's share of a tile row of the streamed field fb/mb
    float4   v[2];
    uint32_t m[2];
};

// Running maxima for the zero-flow predicates of one field pair, kept as the BIT PATTERNS of |u|, |v|: non-negative floats
// order like their bits, and every NaN pattern orders above Inf, so that a NaN component counts as non-zero and as >= th
// exactly as stat_bits' `v != 0` and `!(v < th && v > -th)` have it (a float maximum would drop it: fmaxf(x, NaN) == x).
struct C3Stat {
    uint32_t amax_m, bmax, bmax_m;
};

__device__ __forceinline__ uint32_t c3_abs_bits(float u, float v)
{
    return max(__float_as_uint(u) & 0x7fffffffu, __float_as_uint(v) & 0x7fffffffu);
}

// the six predicates of a lane's maxima: fa masked, fb masked, fb anywhere; each non-zero / >= th (th > 0, as bits)
__device__ __forceinline__ void c3_stat_predicates(const C3Stat &st, float th, bool (&c)[6])
{
    const uint32_t tb = __float_as_uint(th);
    c[0] = st.amax_m != 0u; c[1] = st.amax_m >= tb;
    c[2] = st.bmax_m != 0u; c[3] = st.bmax_m >= tb;
    c[4] = st.bmax != 0u;   c[5] = st.bmax >= tb;
}

template <bool BITS = false>
__device__ __forceinline__ C3Stream c3_load_stream(const C3Args &a, const C3Field &F, int y, const int (&xg)[2])
{
    typedef C3Ix<BITS> Ix;
    C3Stream s;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        s.v[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        s.m[g] = 0;
        if (y < a.H && xg[g] < a.W) {
            const Ix o = (Ix)y * (Ix)a.W + (Ix)xg[g];
            const v4f t = __builtin_nontemporal_load(c3_elem(reinterpret_cast<const v4f *>(F.fb), o >> 1));
            s.v[g] = make_float4(t.x, t.y, t.z, t.w);
            if (BITS) {
                // the pair's two bits (xg is even: both in one word; the 16 lanes of a word read the same address)
                const uint32_t w = reinterpret_cast<const uint32_t *>(F.mb)[(size_t)y * a.mwpr + (xg[g] >> 5)] >> (xg[g] & 31);
                s.m[g] = (w & 1u) | ((w & 2u) << 7);
            } else {
                s.m[g] = __builtin_nontemporal_load(c3_elem(reinterpret_cast<const uint16_t *>(F.mb), o >> 1));
            }
        }
    }
    return s;
}

// Flag words of field pair b (set-only, plain idempotent stores; thousands of waves issuing atomics on one address would
// serialise at the memory side).  fb: all four predicates, exact.  fa: words 0/1 are set when a GATHERED masked vector is
// non-zero / above threshold -- a certificate that fa is not zero; a clear word means "not observed" and is confirmed by
// ofl_flow_stats_dev.  Words 2/3 are never touched here.
//
// A wave reads the row ONCE, at its top: lane k loads word k & 7 (one instruction on one 32-byte segment), ahead of the stream loads,
// so that the wait for the stream data covers it, and keeps "which words were clear" as a wave-uniform bit mask (one scalar
// register) while it makes the stream and gather round trips it makes anyway.  At its end the wave only stores, and only the
// words it needs that its early copy showed clear: nothing is loaded or waited for after the output stores.  The words
// never go back to 0 within a launch (the caller zeroes them beforehand), so a stale copy can only show 0 where memory
// already holds 1, which costs a redundant store of the same value and never a wrong word.
//
// The load is a plain, L1-cacheable VECTOR load (measured faster than an agent-scope one, HISTORY round 6): L1 is invalidated
// at kernel start and a stale line of zeros lives only until the streaming traffic evicts it.  It must not become a scalar
// load -- the scalar cache would hold the hot line for the whole kernel and every wave would store -- which the per-lane
// address (lane & 7) rules out.
__device__ __forceinline__ uint32_t c3_load_flags(const C3Args &a, int b)
{
    // every lane asks for word (lane & 7): no branch around the load, so nothing ties the wait for it to this place
    return a.stats[(size_t)b * 8 + (threadIdx.x & 7)];
}

// bit k = word k of the row was clear when the wave read it
__device__ __forceinline__ uint32_t c3_clear_flags(uint32_t seen) { return (uint32_t)__ballot(seen == 0u) & 0xffu; }

__device__ __forceinline__ void c3_flush_stats(const C3Args &a, int b, const C3Stat &st, uint32_t clear)
{
    bool c[6];
    c3_stat_predicates(st, a.th, c);
    uint32_t need = 0;                        // wave-uniform: bit k = some lane saw predicate k
#pragma unroll
    for (int k = 0; k < 6; ++k) need |= (__ballot(c[k]) != 0ull) ? 1u << k : 0u;
    const uint32_t words = ((need & 3u) | ((need >> 2) << 4)) & clear;      // predicates 0 .. 5 live in words 0, 1, 4, 5, 6, 7
    const uint32_t lane = __lane_id();        // (not threadIdx.x: no vector register has to live to the end of the wave for it)
    if (lane < 8u && ((words >> lane) & 1u))
        a.stats[(size_t)b * 8 + lane] = 1u;
}

// The read-at-the-end form of the same flush (one round trip for the six words, then the stores), kept for the QUANT_EXACT
// byte-mask instantiation: that kernel sits at exactly the 80 VGPRs of kC3Waves, and with the store-only tail above the
// register allocator spills two of them in the interior gather, with or without the early read (HISTORY round 6).
__device__ __forceinline__ void c3_flush_stats_late(const C3Args &a, int b, const C3Stat &st)
{
    bool c[6];
    c3_stat_predicates(st, a.th, c);
    const int  slot[6] = { 0, 1, 4, 5, 6, 7 };
    uint32_t need = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) need |= (__ballot(c[k]) != 0ull) ? 1u << k : 0u;
    if (need != 0u && (threadIdx.x & 63) == 0) {
        uint32_t *s = a.stats + (size_t)b * 8;
        uint32_t seen[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) seen[k] = __hip_atomic_load(s + slot[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (((need >> k) & 1u) && seen[k] == 0u) s[slot[k]] = 1u;
    }
}

// stream out: out = fb + B(fa), mout = mb & valid   (flow_class.py:332-334, 668, 680)
template <bool STATS, bool BITS = false>
__device__ __forceinline__ void c3_finish(const C3Args &a, const C3Field &F, int y, const int (&xg)[2], const bool (&act)[2],
                                          const float (&bu)[kC3Px], const float (&bv)[kC3Px], const bool (&bm)[kC3Px],
                                          const float (&su)[kC3Px], const float (&sv)[kC3Px], const bool (&ok)[kC3Px],
                                          C3Stat &st)
{
    typedef C3Ix<BITS> Ix;
    const Ix row = (Ix)y * (Ix)a.W;
    if constexpr (BITS) {
        // vectors as in the byte form; the mask leaves as whole words: a wave is two tile rows (lanes 0 .. 31 / 32 .. 63), the
        // ballots of the pairs' even and odd pixels are interleaved by the lanes that store (lane 0 / 16 of a row: the words of
        // pixels 0 .. 31 / 32 .. 63 of the 64-px stretch)
        const int lx = threadIdx.x & 31;
        const size_t wrow = (size_t)y * a.mwpr;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int j = 2 * g;
            const bool be = act[g] && ok[j] && bm[j], bo = act[g] && ok[j + 1] && bm[j + 1];
            const unsigned long long me = __ballot(be), mo = __ballot(bo);
            if (act[g]) {
                const float4 o4 = make_float4(__fadd_rn(bu[j], su[j]), __fadd_rn(bv[j], sv[j]),
                                              __fadd_rn(bu[j + 1], su[j + 1]), __fadd_rn(bv[j + 1], sv[j + 1]));
                const v4f t = { o4.x, o4.y, o4.z, o4.w };
                __builtin_nontemporal_store(t, c3_elem(reinterpret_cast<v4f *>(F.out), (row + xg[g]) >> 1));
                if (STATS) {
                    const uint32_t a0 = c3_abs_bits(bu[j], bv[j]), a1 = c3_abs_bits(bu[j + 1], bv[j + 1]);
                    st.bmax   = max(st.bmax, max(a0, a1));
                    st.bmax_m = max(st.bmax_m, max(bm[j] ? a0 : 0u, bm[j + 1] ? a1 : 0u));
                }
            }
            // (lane 0 / 16 of a row: its pair starts the word, so its own `act` says whether the word exists -- x < W, y < H)
            if ((lx & 15) == 0 && act[g]) {
                const uint32_t e32 = (uint32_t)(me >> (threadIdx.x & 32)), o32 = (uint32_t)(mo >> (threadIdx.x & 32));
                const uint32_t word = c3_spread16(e32 >> lx) | (c3_spread16(o32 >> lx) << 1);
                __builtin_nontemporal_store(word, reinterpret_cast<uint32_t *>(F.mout) + wrow + (xg[g] >> 5));
            }
        }
        return;
    }
    // Mask bytes leave as DWORDS when the row length allows aligned ones: the lane pairs (2k, 2k + 1) own four consecutive
    // pixels, the even lane stores both lanes' bytes (sub-dword stores cost as much per instruction as 16-byte ones)
    const bool quad = (a.W & 3) == 0;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int jj = 2 * g;
        const uint32_t mine = ((ok[jj] && bm[jj]) ? 1u : 0u) | ((ok[jj + 1] && bm[jj + 1]) ? 0x100u : 0u);
        const uint32_t other = (uint32_t)__shfl_xor((int)mine, 1);
        if (act[g]) {
            const int j = 2 * g;
            const Ix o = row + (Ix)xg[g];
            const v4f t = { __fadd_rn(bu[j], su[j]), __fadd_rn(bv[j], sv[j]), __fadd_rn(bu[j + 1], su[j + 1]), __fadd_rn(bv[j + 1], sv[j + 1]) };
            __builtin_nontemporal_store(t, c3_elem(reinterpret_cast<v4f *>(F.out), o >> 1));
            if (quad) {
                if ((threadIdx.x & 1) == 0) __builtin_nontemporal_store(mine | (other << 16), c3_elem(reinterpret_cast<uint32_t *>(F.mout), o >> 2));
            } else {
                __builtin_nontemporal_store((uint16_t)mine, c3_elem(reinterpret_cast<uint16_t *>(F.mout), o >> 1));
            }
            if (STATS) {
                const uint32_t a0 = c3_abs_bits(bu[j], bv[j]), a1 = c3_abs_bits(bu[j + 1], bv[j + 1]);
                st.bmax   = max(st.bmax, max(a0, a1));
                st.bmax_m = max(st.bmax_m, max(bm[j] ? a0 : 0u, bm[j + 1] ? a1 : 0u));
            }
        }
    }
}

// One pixel whose taps may lie partly outside the source: clamp the addresses, zero the taps that fall outside (cv2
// BORDER_CONSTANT 0).  `v` holds the pixel's sampling vector on entry and B(fa) on return, `k` its validity: the border
// paths run one pixel per loop trip through LDS slots so that this rare path does not set the kernel's register budget.
template <int QUANT, bool STATS, bool BITS>
__device__ __forceinline__ void c3_border_px(const C3Args &a, const C3Field &F, int gx, int gy, bool act,
                                             float2 &v, uint8_t &k, C3Stat &st)
{
    typedef C3Ix<BITS> Ix;
    const int H = a.H, W = a.W;
    const int mrow = a.mwpr * 4;              // BITS: row pitch of the bit planes in bytes
    const C3Pos p = c3_pos<QUANT>(gx, gy, v.x, v.y, a.sign);
    const int  ix  = c3_tap<QUANT>(p.x), iy = c3_tap<QUANT>(p.y);
    const int  ixc = min(max(ix, 0), max(W - 2, 0));
    const int  d   = ix - ixc;
    const bool r0  = (unsigned)iy < (unsigned)H;
    const bool r1  = (unsigned)(iy + 1) < (unsigned)H;
    const int  y0c = min(max(iy, 0), H - 1);
    const int  y1c = min(max(iy + 1, 0), H - 1);
    const Ix s0 = (Ix)y0c * (Ix)W + (Ix)ixc, s1 = (Ix)y1c * (Ix)W + (Ix)ixc;
    const Pair2 p0 = c3_pair(F.fa, s0);
    const Pair2 p1 = c3_pair(F.fa, s1);
    uint32_t q00, q01, q10, q11;
    if (BITS) {
        const uint8_t *r0p = F.ma + (size_t)y0c * mrow, *r1p = F.ma + (size_t)y1c * mrow;
        q00 = c3_bit(r0p, ixc); q01 = c3_bit(r0p, min(ixc + 1, W - 1)); q10 = c3_bit(r1p, ixc); q11 = c3_bit(r1p, min(ixc + 1, W - 1));
    } else {
        q00 = *c3_elem(F.ma, s0); q01 = *c3_elem(F.ma, s0 + 1); q10 = *c3_elem(F.ma, s1); q11 = *c3_elem(F.ma, s1 + 1);
    }
    float u00, v00, u01, v01, u10, v10, u11, v11, a00, a01, a10, a11;
    select_pair(p0, d, r0, u00, v00, u01, v01);
    select_pair(p1, d, r1, u10, v10, u11, v11);
    select_mask(q00, q01, d, r0, a00, a01);
    select_mask(q10, q11, d, r1, a10, a11);
    const C3Tap w = c3_weights<QUANT>(p);
    v = make_float2(c3_blend(u00, u01, u10, u11, w), c3_blend(v00, v01, v10, v11, w));
    k = c3_valid<QUANT>(a00 != 0.0f, a01 != 0.0f, a10 != 0.0f, a11 != 0.0f, w) ? 1 : 0;
    if (STATS) st.amax_m = max(st.amax_m, (a00 != 0.0f && act) ? c3_abs_bits(u00, v00) : 0u);
}

// interior and outside tests of one pixel's taps, accumulated over a lane's pixels
template <int QUANT>
__device__ __forceinline__ void c3_classify(const C3Pos &p, int H, int W, bool act, bool &inside, bool &outside)
{
    const int ix = c3_tap<QUANT>(p.x), iy = c3_tap<QUANT>(p.y);
    const bool in_j  = (unsigned)ix <= (unsigned)(W - 2) && (unsigned)iy <= (unsigned)(H - 2);
    bool out_j = ix < -1 || ix >= W || iy < -1 || iy >= H;
    // QUANT_EXACT: a NaN or Inf coordinate has no fraction, its weights are NaN and so is its blend of four zeros (the oracle's
    // 0 * NaN); such a pixel takes the border path, which multiplies, and never the shortcut that writes 0 for a whole wave
    if (QUANT == OFL_QUANT_EXACT) out_j = out_j && __builtin_isfinite(__int_as_float(p.x)) && __builtin_isfinite(__int_as_float(p.y));
    inside  = inside && (in_j || !act);
    outside = outside && (out_j || !act);
}

// The two pixels of one lane pair (gx, gx + 1 of row gy; slots v[0..1], k[0..1]) in ONE gather round trip instead of
// c3_border_px's two: both pixels' mask taps (one unaligned 2-byte load per row and pixel at the clamped column, bytes
// ixc and ixc + 1 <= W - 1) and then both pixels' vector taps are requested before anything is selected or blended.  Per
// pixel the calls and their order are c3_border_px's, so the values are too: a tap outside the source becomes 0.0f by
// selecting the VALUE (a zeroed weight would change the sign of zero sums and let a clamped Inf / NaN through).  A pair
// group whose pixels are outside (or inactive) in every lane of the wave loads nothing: (0, 0) and validity 0 are what the
// selects give such pixels.  Byte masks with QUANT_OPENCV only: QUANT_EXACT has no register left for it (HISTORY round 7).
template <int QUANT, bool STATS>
__device__ __forceinline__ void c3_border_pair(const C3Args &a, const C3Field &F, int gx, int gy, bool act,
                                               float2 *v, uint8_t *k, C3Stat &st)
{
    const int H = a.H, W = a.W;
    const float4 f = *reinterpret_cast<const float4 *>(v);
    C3Pos p[2] = { c3_pos<QUANT>(gx, gy, f.x, f.y, a.sign), c3_pos<QUANT>(gx + 1, gy, f.z, f.w, a.sign) };
    bool inside = true, outside = true;       // (`inside` is not used: the wave is a border wave)
#pragma unroll
    for (int i = 0; i < 2; ++i) c3_classify<QUANT>(p[i], H, W, act, inside, outside);
    if (__all(outside)) {
        *reinterpret_cast<float4 *>(v) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        *reinterpret_cast<uint16_t *>(k) = 0;
        return;
    }
    uint32_t s0[2], s1[2];                    // the clamped tap rows' offsets (the rows clamp independently)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ix  = c3_tap<QUANT>(p[i].x), iy = c3_tap<QUANT>(p[i].y);
        const int ixc = min(max(ix, 0), max(W - 2, 0));
        s0[i] = (uint32_t)min(max(iy, 0), H - 1) * (uint32_t)W + (uint32_t)ixc;
        s1[i] = (uint32_t)min(max(iy + 1, 0), H - 1) * (uint32_t)W + (uint32_t)ixc;
    }
    uint32_t q0[2], q1[2];
    Pair2    p0[2], p1[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {             // mask taps first, as in the interior gather
        q0[i] = reinterpret_cast<const U16u *>(c3_elem(F.ma, s0[i]))->v;
        q1[i] = reinterpret_cast<const U16u *>(c3_elem(F.ma, s1[i]))->v;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        p0[i] = c3_pair(F.fa, s0[i]);
        p1[i] = c3_pair(F.fa, s1[i]);
    }
    float   su[2], sv[2];
    uint32_t ok = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        // Which taps exist is worked out only here, behind the loads and behind the first pixel's blend: as compare results
        // the select conditions and the mask taps are wave masks, two scalar registers each, and with those of both pixels
        // alive across the round trip the kernel goes past its 80 SGPRs.  The empty statements emit nothing; they only keep
        // the compiler from moving what follows them to the front.
        if (i == 0) asm volatile("" : "+v"(p[0].x), "+v"(p[0].y));
        else        asm volatile("" : "+v"(p[1].x), "+v"(p[1].y), "+v"(su[0]), "+v"(sv[0]), "+v"(ok));
        const int  ix = c3_tap<QUANT>(p[i].x), iy = c3_tap<QUANT>(p[i].y);
        const int  d  = ix - min(max(ix, 0), max(W - 2, 0));
        const bool r0 = (unsigned)iy < (unsigned)H;
        const bool r1 = (unsigned)(iy + 1) < (unsigned)H;
        float u00, v00, u01, v01, u10, v10, u11, v11, a00, a01, a10, a11;
        select_pair(p0[i], d, r0, u00, v00, u01, v01);
        select_pair(p1[i], d, r1, u10, v10, u11, v11);
        select_mask(q0[i] & 0xffu, q0[i] & 0xff00u, d, r0, a00, a01);
        select_mask(q1[i] & 0xffu, q1[i] & 0xff00u, d, r1, a10, a11);
        const C3Tap w = c3_weights<QUANT>(p[i]);
        su[i] = c3_blend(u00, u01, u10, u11, w);
        sv[i] = c3_blend(v00, v01, v10, v11, w);
        ok |= c3_valid<QUANT>(a00 != 0.0f, a01 != 0.0f, a10 != 0.0f, a11 != 0.0f, w) ? 1u << (8 * i) : 0u;
        if (STATS) st.amax_m = max(st.amax_m, (a00 != 0.0f && act) ? c3_abs_bits(u00, v00) : 0u);
    }
    *reinterpret_cast<float4 *>(v) = make_float4(su[0], sv[0], su[1], sv[1]);
    *reinterpret_cast<uint16_t *>(k) = (uint16_t)ok;
}

// One tile in the streaming layout: taps from the already loaded stream data, gather, blend, store.
template <int QUANT, bool STATS, bool BITS = false>
__device__ __forceinline__ void c3_tile(const C3Args &a, const C3Field &F, int y, const int (&xg)[2], const bool (&act)[2],
                                        const C3Stream &in, float2 *xp_v, uint8_t *xp_ok, C3Stat &st)
{
    typedef C3Ix<BITS> Ix;
    const int H = a.H, W = a.W, sign = a.sign;
    const int mrow = a.mwpr * 4;              // BITS: row pitch of the bit planes in bytes

    float       bu[kC3Px] = { in.v[0].x, in.v[0].z, in.v[1].x, in.v[1].z };
    float       bv[kC3Px] = { in.v[0].y, in.v[0].w, in.v[1].y, in.v[1].w };
    const bool  bm[kC3Px] = { (in.m[0] & 0xffu) != 0, (in.m[0] & 0xff00u) != 0,
                              (in.m[1] & 0xffu) != 0, (in.m[1] & 0xff00u) != 0 };
    // this lane's own LDS slots (the tile's transposition buffer, unused in the streaming layout; no other lane touches
    // them, so no barrier)
    float2  *v = xp_v + (threadIdx.x >> 5) * kXpRowF2 + 2 * (threadIdx.x & 31);
    uint8_t *k = xp_ok + (threadIdx.x >> 5) * 128 + 2 * (threadIdx.x & 31);

    C3Pos tp[kC3Px];
    bool inside = true, outside = true;
#pragma unroll
    for (int j = 0; j < kC3Px; ++j) {
        tp[j] = c3_pos<QUANT>(xg[j >> 1] + (j & 1), y, bu[j], bv[j], sign);
        c3_classify<QUANT>(tp[j], H, W, act[j >> 1], inside, outside);
    }
    if (H < 2) inside = false;

    float su[kC3Px], sv[kC3Px];
    bool  ok[kC3Px];
#pragma unroll
    for (int j = 0; j < kC3Px; ++j) { su[j] = 0.0f; sv[j] = 0.0f; ok[j] = false; }

    if (__all(outside)) {
        // every tap of every pixel of this wave lies outside the source: B(.) = 0, nothing to fetch
    } else if (__all(inside)) {
        // interior fast path: all four taps in bounds, no clamping and no selects.  The streamed vectors wait in LDS
        // while the gather is in flight (8 VGPRs of the 64).
        *reinterpret_cast<float4 *>(v)      = in.v[0];
        *reinterpret_cast<float4 *>(v + 64) = in.v[1];
        Pair2    p0[kC3Px], p1[kC3Px];
        uint32_t m0[kC3Px], m1[kC3Px];
        // The two pixels of a pair usually sample the same two source rows at columns at most two apart (axis-aligned
        // sampling: scalings, translations): their eight mask taps are then four bytes of each row -- ONE unaligned
        // 4-byte load per row and pair instead of one 2-byte load per row and pixel (4 instead of 8 mask gathers per lane).
        bool share = true;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int ix0 = c3_tap<QUANT>(tp[2 * g].x), ix1 = c3_tap<QUANT>(tp[2 * g + 1].x);
            share = share && (!act[g] || (c3_tap<QUANT>(tp[2 * g].y) == c3_tap<QUANT>(tp[2 * g + 1].y) &&
                                          (unsigned)(ix1 - ix0) <= 2u && ix0 + 3 < W));
        }
        share = __all(share);
        Ix  s[kC3Px];                         // top-left taps as offsets in the field
        int fr[kC3Px];                        // QUANT_OPENCV: all the weights need once the taps are addressed (c3_pack_frac)
        // the second tap row through second scalar bases: all four loads of a pixel take the same 32-bit offset register
        const float   *fa1 = F.fa + 2 * (size_t)W;
        const uint8_t *ma1 = F.ma + (BITS ? (size_t)mrow : (size_t)W);
#pragma unroll
        for (int j = 0; j < kC3Px; ++j) {
            const int ix = act[j >> 1] ? c3_tap<QUANT>(tp[j].x) : 0, iy = act[j >> 1] ? c3_tap<QUANT>(tp[j].y) : 0;
            s[j] = (Ix)iy * (Ix)W + (Ix)ix;
            fr[j] = c3_pack_frac(tp[j]);
            if (BITS) {
                // bits 0 / 1 = taps ix / ix + 1 (bits 2, 3 serve the pair's other pixel when it shares the load)
                if (share && (j & 1)) {
                    const int sh = act[j >> 1] ? c3_tap<QUANT>(tp[j].x) - c3_tap<QUANT>(tp[j - 1].x) : 0;
                    m0[j] = m0[j - 1] >> sh;
                    m1[j] = m1[j - 1] >> sh;
                } else {
                    const size_t r0 = (size_t)iy * mrow;
                    m0[j] = c3_bits_at(F.ma + r0, ix);
                    m1[j] = c3_bits_at(ma1 + r0, ix);
                }
            }
        }
        // mask taps first, so that their addresses are spent before the vector taps occupy their registers
        if constexpr (!BITS) {
            if (share) {
#pragma unroll
                for (int j = 0; j < kC3Px; j += 2) {
                    m0[j] = reinterpret_cast<const U32u *>(c3_elem(F.ma, s[j]))->v;
                    m1[j] = reinterpret_cast<const U32u *>(c3_elem(ma1, s[j]))->v;
                }
#pragma unroll
                for (int j = 1; j < kC3Px; j += 2) {
                    const int sh = 8 * (int)(s[j] - s[j - 1]);      // same row: the column step (0 for a pair outside the field)
                    m0[j] = m0[j - 1] >> sh;
                    m1[j] = m1[j - 1] >> sh;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kC3Px; ++j) {
                    m0[j] = reinterpret_cast<const U16u *>(c3_elem(F.ma, s[j]))->v;
                    m1[j] = reinterpret_cast<const U16u *>(c3_elem(ma1, s[j]))->v;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kC3Px; ++j) {
            p0[j] = c3_pair(F.fa, s[j]);
            p1[j] = c3_pair(fa1, s[j]);
        }
#pragma unroll
        for (int j = 0; j < kC3Px; ++j) {
            const C3Tap w = c3_weights<QUANT>(QUANT == OFL_QUANT_OPENCV ? c3_unpack_frac(fr[j]) : tp[j]);
            su[j] = c3_blend(p0[j].lo_u, p0[j].hi_u, p1[j].lo_u, p1[j].hi_u, w);
            sv[j] = c3_blend(p0[j].lo_v, p0[j].hi_v, p1[j].lo_v, p1[j].hi_v, w);
            const bool m00 = (m0[j] & (BITS ? 1u : 0xffu)) != 0, m01 = (m0[j] & (BITS ? 2u : 0xff00u)) != 0;
            const bool m10 = (m1[j] & (BITS ? 1u : 0xffu)) != 0, m11 = (m1[j] & (BITS ? 2u : 0xff00u)) != 0;
            ok[j] = c3_valid<QUANT>(m00, m01, m10, m11, w);
            if (STATS) st.amax_m = max(st.amax_m, (m00 && act[j >> 1]) ? c3_abs_bits(p0[j].lo_u, p0[j].lo_v) : 0u);
        }
        const float4 b01 = *reinterpret_cast<const float4 *>(v), b23 = *reinterpret_cast<const float4 *>(v + 64);
        bu[0] = b01.x; bu[1] = b01.z; bu[2] = b23.x; bu[3] = b23.z;
        bv[0] = b01.y; bv[1] = b01.w; bv[2] = b23.y; bv[3] = b23.w;
    } else {
        // border path through the lane's LDS slots: a pixel PAIR per trip, or one pixel where the pair form does not fit
        constexpr bool pairs = !BITS && QUANT == OFL_QUANT_OPENCV;      // (c3_border_pair: QUANT_EXACT is at 80 of 80 VGPRs without it)
        *reinterpret_cast<float4 *>(v)      = in.v[0];
        *reinterpret_cast<float4 *>(v + 64) = in.v[1];
        if constexpr (pairs) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int g = 0; g < 2; ++g)
                c3_border_pair<QUANT, STATS>(a, F, xg[0] + 64 * g, y, g ? act[1] : act[0], v + 64 * g, k + 64 * g, st);
        } else {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int j = 0; j < kC3Px; ++j) {
                const int o = (j & 1) + 64 * (j >> 1);
                c3_border_px<QUANT, STATS, BITS>(a, F, xg[0] + o, y, y < H && xg[0] + o < W, v[o], k[o], st);
            }
        }
        const float4 s01 = *reinterpret_cast<const float4 *>(v), s23 = *reinterpret_cast<const float4 *>(v + 64);
        const uint32_t k01 = *reinterpret_cast<const uint16_t *>(k), k23 = *reinterpret_cast<const uint16_t *>(k + 64);
        su[0] = s01.x; su[1] = s01.z; su[2] = s23.x; su[3] = s23.z;
        sv[0] = s01.y; sv[1] = s01.w; sv[2] = s23.y; sv[3] = s23.w;
        ok[0] = (k01 & 0xffu) != 0; ok[1] = (k01 & 0xff00u) != 0; ok[2] = (k23 & 0xffu) != 0; ok[3] = (k23 & 0xff00u) != 0;
    }

    c3_finish<STATS, BITS>(a, F, y, xg, act, bu, bv, bm, su, sv, ok, st);
}

// ---------------------------------------------------------------------------------------------------------
// K2, transposed-gather form.  The streaming layout (a wave = 2 rows x 128 px) is what the stream loads
// and stores want, but when the sampling grid is ROTATED each gather instruction of such a wave touches 60+ cache
// lines (one per source row its 128-px segment crosses): the texture cache's tag look-ups, not HBM, bound the
// kernel (rocprofv3: 2.75 x the cache accesses of the axis-aligned case).  Workgroups that see such a field hand
// their sampling vectors through LDS to a BLOCK layout (a wave = 32 px x 8 rows, every gather instruction one 8 x 8
// block of it), gather and blend there (~15 lines per instruction), and hand the results back for the streaming stores.  Same arithmetic
// per pixel, bit-identical results; axis-aligned fields keep the direct path.
//
// Block layout, lane (r, c) of wave w: pixel j at row r, column 32 w + c + 8 j, whose LDS slot holds its sampling vector on
// entry and B(fa) / validity on return.
template <int QUANT, bool STATS, bool BITS = false>
__device__ __forceinline__ void c3_sample_block(const C3Args &a, const C3Field &F, int gx0, int gy,
                                                float2 *v, uint8_t *k, C3Stat &st)
{
    typedef C3Ix<BITS> Ix;
    const int H = a.H, W = a.W;
    const int mrow = a.mwpr * 4;              // BITS: row pitch of the bit planes in bytes
    C3Pos tp[4];
    bool inside = true, outside = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float2 f = v[8 * j];
        tp[j] = c3_pos<QUANT>(gx0 + 8 * j, gy, f.x, f.y, a.sign);
        c3_classify<QUANT>(tp[j], H, W, gy < H && gx0 + 8 * j < W, inside, outside);
    }
    if (H < 2) inside = false;
    if (__all(outside)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[8 * j] = make_float2(0.0f, 0.0f); k[8 * j] = 0; }
        return;
    }
    if (__all(inside)) {
        Pair2    p0[4], p1[4];
        uint32_t m0[4], m1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool act = gy < H && gx0 + 8 * j < W;
            const int ix = act ? c3_tap<QUANT>(tp[j].x) : 0, iy = act ? c3_tap<QUANT>(tp[j].y) : 0;
            const Ix s0 = (Ix)iy * (Ix)W + (Ix)ix;
            p0[j] = c3_pair(F.fa, s0);
            p1[j] = c3_pair(F.fa, (Ix)(s0 + (Ix)W));
            if (BITS) {
                const uint8_t *r0 = F.ma + (size_t)iy * mrow;
                m0[j] = c3_bits_at(r0, ix);
                m1[j] = c3_bits_at(r0 + mrow, ix);
            } else {
                m0[j] = reinterpret_cast<const U16u *>(c3_elem(F.ma, s0))->v;
                m1[j] = reinterpret_cast<const U16u *>(c3_elem(F.ma, s0 + (Ix)W))->v;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const C3Tap w = c3_weights<QUANT>(tp[j]);
            v[8 * j] = make_float2(c3_blend(p0[j].lo_u, p0[j].hi_u, p1[j].lo_u, p1[j].hi_u, w),
                                   c3_blend(p0[j].lo_v, p0[j].hi_v, p1[j].lo_v, p1[j].hi_v, w));
            const bool m00 = (m0[j] & (BITS ? 1u : 0xffu)) != 0, m01 = (m0[j] & (BITS ? 2u : 0xff00u)) != 0;
            const bool m10 = (m1[j] & (BITS ? 1u : 0xffu)) != 0, m11 = (m1[j] & (BITS ? 2u : 0xff00u)) != 0;
            k[8 * j] = c3_valid<QUANT>(m00, m01, m10, m11, w) ? 1 : 0;
            const bool act = gy < H && gx0 + 8 * j < W;
            if (STATS) st.amax_m = max(st.amax_m, (m00 && act) ? c3_abs_bits(p0[j].lo_u, p0[j].lo_v) : 0u);
        }
        return;
    }
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int j = 0; j < 4; ++j)               // border path, as in c3_tile
        c3_border_px<QUANT, STATS, BITS>(a, F, gx0 + 8 * j, gy, gy < H && gx0 + 8 * j < W, v[8 * j], k[8 * j], st);
}

constexpr int kC3Waves = 6;                   // waves per SIMD the register allocator is asked to leave room for (7 and 8 spill and are slower: HISTORY, round 5)
constexpr int kC3BitsWaves = 5;               // the packed-mask form needs a few registers more than the 6-wave budget leaves
template <int QUANT, bool STATS, bool BITS = false>      // BITS: the three masks are packed bit planes (ofl_compose3_bits_dev)
__global__ __launch_bounds__(256, BITS ? kC3BitsWaves : kC3Waves)
void compose3_xpose_kernel(const C3Args a)
{
    static_assert(kC3LanesX == 32, "the transposed form assumes 128 x 8 tiles");
    __shared__ __attribute__((aligned(16))) float2 xp_v[8 * kXpRowF2];
    __shared__ __attribute__((aligned(16))) uint8_t xp_ok[8 * 128];
    const int tile = blockIdx.x;          // natural tile order (XCD-aware orders were measured slower)
    if (tile >= a.ntiles) return;
    const int H = a.H, W = a.W;
    // lane (lx, ly) owns the pixel pairs at x = 2*lx and x = 2*kC3LanesX + 2*lx of tile row ly
    const int b   = tile / a.tiles_per_field;
    const int t   = tile - b * a.tiles_per_field;
    const int ty  = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int ly  = threadIdx.x >> 5, lx = threadIdx.x & 31;
    const int y   = ty * kC3TileH + ly;
    const int xg[2] = { tx * kC3TileW + 2 * lx, tx * kC3TileW + 2 * lx + 2 * kC3LanesX };
    const bool act[2] = { y < H && xg[0] < W, y < H && xg[1] < W };
    const C3Field F = c3_field<BITS>(a, b);
    C3Stat st = { 0u, 0u, 0u };
    const C3Stream in = c3_load_stream<BITS>(a, F, y, xg);
    constexpr bool early = STATS && (BITS || QUANT != OFL_QUANT_EXACT);      // (c3_flush_stats_late: the one instantiation without)
    const uint32_t seen = early ? c3_load_flags(a, b) : 1u;      // the field's flag row, in flight with the stream (c3_flush_stats)
    const uint32_t clear = early ? c3_clear_flags(seen) : 0u;
    // Does a streamed row segment of this tile cross many source rows (sample row = y -/+ v)?  Every wave answers from
    // the SAME two values -- the vertical flow at the two ends of the tile's first row (uniform loads, L2 hits) -- so
    // the workgroup agrees without a barrier and the direct path costs nothing extra.
    bool rotated;
    {
        const int x0 = tx * 128, x1 = min(x0 + 127, W - 1), yy = min(ty * 8, H - 1);
        const float *frow = F.fb + 2 * (size_t)yy * W;
        rotated = fabsf(frow[2 * x1 + 1] - frow[2 * x0 + 1]) * 128.0f > (float)(kXposeRows * (x1 - x0 + 1));
    }
    if (!rotated) {
        c3_tile<QUANT, STATS, BITS>(a, F, y, xg, act, in, xp_v, xp_ok, st);
        if (early) c3_flush_stats(a, b, st, clear); else if (STATS) c3_flush_stats_late(a, b, st);
        return;
    }
    // streaming layout -> LDS: the sampling vectors of this lane's two pixel pairs
    *reinterpret_cast<float4 *>(&xp_v[ly * kXpRowF2 + 2 * lx])      = in.v[0];
    *reinterpret_cast<float4 *>(&xp_v[ly * kXpRowF2 + 64 + 2 * lx]) = in.v[1];
    __syncthreads();
    // block layout: wave w owns columns [32 w, 32 w + 32) of all 8 rows, a lane four adjacent pixels
    // every gather INSTRUCTION (fixed j) then covers a compact 8 x 8 block: pixel j of lane (r, c) is column 8 j + c
    {
        const int w4 = threadIdx.x >> 6, l = threadIdx.x & 63, r = l >> 3, c0 = 32 * w4 + (l & 7);
        c3_sample_block<QUANT, STATS, BITS>(a, F, tx * 128 + c0, ty * 8 + r, &xp_v[r * kXpRowF2 + c0], &xp_ok[r * 128 + c0], st);
    }
    __syncthreads();
    // back in the streaming layout: add, combine the masks, store
    {
        const float4 s01 = *reinterpret_cast<const float4 *>(&xp_v[ly * kXpRowF2 + 2 * lx]);
        const float4 s23 = *reinterpret_cast<const float4 *>(&xp_v[ly * kXpRowF2 + 64 + 2 * lx]);
        const uint32_t k01 = *reinterpret_cast<const uint16_t *>(&xp_ok[ly * 128 + 2 * lx]);
        const uint32_t k23 = *reinterpret_cast<const uint16_t *>(&xp_ok[ly * 128 + 64 + 2 * lx]);
        const float su[kC3Px] = { s01.x, s01.z, s23.x, s23.z }, sv[kC3Px] = { s01.y, s01.w, s23.y, s23.w };
        const bool  ok[kC3Px] = { (k01 & 0xffu) != 0, (k01 & 0xff00u) != 0, (k23 & 0xffu) != 0, (k23 & 0xff00u) != 0 };
        const float bu[kC3Px] = { in.v[0].x, in.v[0].z, in.v[1].x, in.v[1].z };
        const float bv[kC3Px] = { in.v[0].y, in.v[0].w, in.v[1].y, in.v[1].w };
        const bool  bm[kC3Px] = { (in.m[0] & 0xffu) != 0, (in.m[0] & 0xff00u) != 0, (in.m[1] & 0xffu) != 0, (in.m[1] & 0xff00u) != 0 };
        c3_finish<STATS, BITS>(a, F, y, xg, act, bu, bv, bm, su, sv, ok, st);
    }
    if (early) c3_flush_stats(a, b, st, clear); else if (STATS) c3_flush_stats_late(a, b, st);
}

// Generic-shape fallback (any W >= 1, one pixel per thread, no vector accesses).
template <int QUANT>
__global__ __launch_bounds__(256)
void compose3_generic_kernel(const float *__restrict__ fa, const uint8_t *__restrict__ ma,
                             const float *__restrict__ fb, const uint8_t *__restrict__ mb,
                             int sign, int H, int W, size_t n_total,
                             float *__restrict__ out, uint8_t *__restrict__ mout,
                             uint32_t *__restrict__ stats, float th)
{
    const size_t hw = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_total;
         i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / hw, o = i - b * hw;
        const int y = (int)(o / W), x = (int)(o - (size_t)y * W);
        const float *fab = fa + b * hw * 2;
        const uint8_t *mab = ma + b * hw;
        const float bu = fb[2 * i], bv = fb[2 * i + 1];
        const Tap tp = make_tap<QUANT>(map_coord(x, bu, sign), map_coord(y, bv, sign));
        float u[4], v[4], a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int yy = tp.iy + (k >> 1), xx = tp.ix + (k & 1);
            const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            const size_t s = in ? (size_t)yy * W + xx : 0;
            u[k] = in ? fab[2 * s] : 0.0f;
            v[k] = in ? fab[2 * s + 1] : 0.0f;
            a[k] = (in && mab[s] != 0) ? 1.0f : 0.0f;
        }
        out[2 * i]     = __fadd_rn(bu, blend4(u[0], u[1], u[2], u[3], tp));
        out[2 * i + 1] = __fadd_rn(bv, blend4(v[0], v[1], v[2], v[3], tp));
        const bool mbit = mb[i] != 0;
        mout[i] = (uint8_t)((blend4(a[0], a[1], a[2], a[3], tp) == 1.0f) & mbit);
        if (stats) {
            uint32_t sb = stat_bits(bu, bv, mbit, th);
            uint32_t sa = stat_bits(fa[2 * i], fa[2 * i + 1], ma[i] != 0, th);
            uint32_t *s = stats + b * 8;
            for (int k = 0; k < 4; ++k) {
                if ((sa >> k) & 1u) s[k] = 1u;
                if ((sb >> k) & 1u) s[4 + k] = 1u;
            }
        }
    }
}

// uint8 masks <-> packed bit planes (rows padded to whole words): one thread per word
__global__ __launch_bounds__(256)
void mask_pack_kernel(const uint8_t *__restrict__ mask, size_t rows, int W, int wpr, uint32_t *__restrict__ bits)
{
    const size_t words = rows * (size_t)wpr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) {
        const size_t r = i / (size_t)wpr;
        const int x0 = (int)(i - r * (size_t)wpr) * 32;
        const uint8_t *m = mask + r * (size_t)W + x0;
        uint32_t w = 0;
        if (x0 + 32 <= W && (((size_t)m) & 15) == 0) {
            const uint4 a = reinterpret_cast<const uint4 *>(m)[0], b = reinterpret_cast<const uint4 *>(m)[1];
            const uint32_t d[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) w |= ((d[k] >> (8 * e)) & 0xffu) ? 1u << (4 * k + e) : 0u;
        } else {
            for (int k = 0; k < 32 && x0 + k < W; ++k) w |= m[k] ? 1u << k : 0u;
        }
        bits[i] = w;
    }
}

__global__ __launch_bounds__(256)
void mask_unpack_kernel(const uint32_t *__restrict__ bits, size_t rows, int W, int wpr, uint8_t *__restrict__ mask)
{
    const size_t words = rows * (size_t)wpr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) {
        const size_t r = i / (size_t)wpr;
        const int x0 = (int)(i - r * (size_t)wpr) * 32;
        const uint32_t w = bits[i];
        uint8_t *m = mask + r * (size_t)W + x0;
        for (int k = 0; k < 32 && x0 + k < W; ++k) m[k] = (w >> k) & 1u;
    }
}

}  // namespace

extern "C" {

int ofl_compose3_dev(const float *fa, const uint8_t *ma, const float *fb, const uint8_t *mb,
                     int sign, int H, int W, int batch, float *out, uint8_t *mout,
                     uint32_t *stats, int quant, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_field_dims("ofl_compose3", H, W));
    if (!fa || !ma || !fb || !mb || !out || !mout) return fail(OFL_E_INVALID, "ofl_compose3: NULL pointer");
    if (batch <= 0) return fail(OFL_E_INVALID, "ofl_compose3: batch must be >= 1");
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "ofl_compose3: sign must be +1 or -1");
    if (quant != OFL_QUANT_OPENCV && quant != OFL_QUANT_EXACT) return fail(OFL_E_INVALID, "ofl_compose3: bad quant");
    hipStream_t s = stream_of(stream);
    const float th = 1e-3f;   // DEFAULT_THRESHOLD, utils.py:22 (compared in float32)

    if (c3_tiled_fits(H, W)) {
        // One workgroup per 128 x 8 tile in natural order -- the dispatcher keeps every wave slot filled and all XCDs sweep
        // one window of memory (measured +2..7 % over a persistent grid at 1..8 4K pairs per launch) -- with the gather
        // transposed through LDS in workgroups whose sampling grid is rotated.
        const int tiles_x = (W + kC3TileW - 1) / kC3TileW, tiles_y = (H + kC3TileH - 1) / kC3TileH;
        const long long nt = (long long)tiles_x * tiles_y * batch;
        if (nt > 0x7fffffffLL) return fail(OFL_E_INVALID, "ofl_compose3: too many tiles");
        C3Args a = { fa, ma, fb, mb, out, mout, stats, sign, H, W, tiles_x, tiles_x * tiles_y, (int)nt, th, 0 };
#define OFL_C3(Q, S) hipLaunchKernelGGL((compose3_xpose_kernel<Q, S>), dim3((int)nt), dim3(256), 0, s, a)
        if (quant == OFL_QUANT_OPENCV) { if (stats) OFL_C3(OFL_QUANT_OPENCV, true); else OFL_C3(OFL_QUANT_OPENCV, false); }
        else                           { if (stats) OFL_C3(OFL_QUANT_EXACT, true);  else OFL_C3(OFL_QUANT_EXACT, false); }
#undef OFL_C3
    } else {
        const size_t n = (size_t)batch * H * W;
        const int nblocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        if (quant == OFL_QUANT_OPENCV)
            hipLaunchKernelGGL((compose3_generic_kernel<OFL_QUANT_OPENCV>), dim3(nblocks), dim3(256), 0, s,
                               fa, ma, fb, mb, sign, H, W, n, out, mout, stats, th);
        else
            hipLaunchKernelGGL((compose3_generic_kernel<OFL_QUANT_EXACT>), dim3(nblocks), dim3(256), 0, s,
                               fa, ma, fb, mb, sign, H, W, n, out, mout, stats, th);
    }
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_mask_bits_bytes(int H, int W, int batch, size_t *bytes)
{
    if (!bytes || H <= 0 || W <= 0 || batch <= 0) return fail(OFL_E_INVALID, "ofl_mask_bits_bytes: bad arguments");
    *bytes = (size_t)batch * H * ((W + 31) / 32) * 4 + 16;      // 16 bytes of slack: the gather reads 4 bytes from the byte of a tap's bit
    return OFL_OK;
}

int ofl_mask_pack_dev(const uint8_t *mask, int H, int W, int batch, uint32_t *bits, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_field_dims("ofl_mask_pack", H, W));
    if (!mask || !bits || batch <= 0) return fail(OFL_E_INVALID, "ofl_mask_pack: NULL pointer / batch < 1");
    const size_t words = (size_t)batch * H * ((W + 31) / 32);
    hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)std::min<size_t>((words + 255) / 256, 65535)), dim3(256), 0, stream_of(stream),
                       mask, (size_t)batch * H, W, (W + 31) / 32, bits);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_mask_unpack_dev(const uint32_t *bits, int H, int W, int batch, uint8_t *mask, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_field_dims("ofl_mask_unpack", H, W));
    if (!mask || !bits || batch <= 0) return fail(OFL_E_INVALID, "ofl_mask_unpack: NULL pointer / batch < 1");
    const size_t words = (size_t)batch * H * ((W + 31) / 32);
    hipLaunchKernelGGL(mask_unpack_kernel, dim3((unsigned)std::min<size_t>((words + 255) / 256, 65535)), dim3(256), 0, stream_of(stream),
                       bits, (size_t)batch * H, W, (W + 31) / 32, mask);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_compose3_bits_dev(const float *fa, const uint32_t *ma_bits, const float *fb, const uint32_t *mb_bits,
                          int sign, int H, int W, int batch, float *out, uint32_t *mout_bits,
                          uint32_t *stats, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_field_dims("ofl_compose3_bits", H, W));
    if (!fa || !ma_bits || !fb || !mb_bits || !out || !mout_bits) return fail(OFL_E_INVALID, "ofl_compose3_bits: NULL pointer");
    if (batch <= 0) return fail(OFL_E_INVALID, "ofl_compose3_bits: batch must be >= 1");
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "ofl_compose3_bits: sign must be +1 or -1");
    if (W % 2) return fail(OFL_E_INVALID, "ofl_compose3_bits: the packed-mask kernel takes even widths (odd ones: ofl_compose3_dev)");
    hipStream_t s = stream_of(stream);
    const int tiles_x = (W + kC3TileW - 1) / kC3TileW, tiles_y = (H + kC3TileH - 1) / kC3TileH;
    const long long nt = (long long)tiles_x * tiles_y * batch;
    if (nt > 0x7fffffffLL) return fail(OFL_E_INVALID, "ofl_compose3_bits: too many tiles");
    C3Args a = { fa, reinterpret_cast<const uint8_t *>(ma_bits), fb, reinterpret_cast<const uint8_t *>(mb_bits), out,
                 reinterpret_cast<uint8_t *>(mout_bits), stats, sign, H, W, tiles_x, tiles_x * tiles_y, (int)nt, 1e-3f, (W + 31) / 32 };
    if (stats) hipLaunchKernelGGL((compose3_xpose_kernel<OFL_QUANT_OPENCV, true, true>), dim3((int)nt), dim3(256), 0, s, a);
    else       hipLaunchKernelGGL((compose3_xpose_kernel<OFL_QUANT_OPENCV, false, true>), dim3((int)nt), dim3(256), 0, s, a);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_compose3(const float *fa, const uint8_t *ma, const float *fb, const uint8_t *mb,
                 int sign, int H, int W, int batch, float *out, uint8_t *mout,
                 uint32_t *stats_host, int quant)
{
    OFL_TRY(need_device());
    OFL_TRY(check_field_dims("ofl_compose3", H, W));
    if (batch <= 0) return fail(OFL_E_INVALID, "ofl_compose3: batch must be >= 1");
    if (!fa || !ma || !fb || !mb || !out || !mout) return fail(OFL_E_INVALID, "ofl_compose3: NULL pointer");
    const size_t n = (size_t)batch * H * W, hw = (size_t)H * W;
    HostStage st("ofl_compose3");
    auto dfa = st.in(fa, n * 2), dfb = st.in(fb, n * 2);
    auto dma = st.in(ma, n), dmb = st.in(mb, n);
    auto dout = st.out(out, n * 2);
    auto dmout = st.out(mout, n);
    auto dst = st.out(stats_host, (size_t)batch * 2);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_compose3_dev(dfa, dma, dfb, dmb, sign, H, W, batch, dout, dmout, nullptr, quant, st.stream()));
    // exact predicates for the host caller: one pass of the statistics kernel per field and operand (the fused
    // launch above only certifies "fa is not zero" from the vectors it happened to gather)
    for (int b = 0; stats_host && b < batch; ++b) {
        OFL_TRY(ofl_flow_stats_dev(dfa + (size_t)b * hw * 2, dma + (size_t)b * hw, hw, 1e-3f, dst + 2 * b, st.stream()));
        OFL_TRY(ofl_flow_stats_dev(dfb + (size_t)b * hw * 2, dmb + (size_t)b * hw, hw, 1e-3f, dst + 2 * b + 1, st.stream()));
    }
    OFL_TRY(st.download());
    for (int k = 0; stats_host && k < 2 * batch; ++k) stats_host[k] &= 15u;
    return OFL_OK;
}

}  // extern "C"
