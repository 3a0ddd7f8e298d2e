// ofl_consistency.hip -- K13: forward-backward consistency of two fields of one reference (gfx950).
//
// Per pixel (x, y) of the forward field f, with the backward field b sampled where f points (sign +1 for 's', -1 for 't':
// the pairing of ofl_compose3_dev with fb = f, fa = b):
//     tap        = make_tap<quant>(map_coord(x, f.u, sign), map_coord(y, f.v, sign))
//     bu, bv     = blend4 of b's four taps (0 outside the frame);  am = blend4 of b's mask taps as 0.0f / 1.0f
//     covered    = f.mask & (am == 1.0f)                                   -- ofl_compose3_dev's mout, bit for bit
//     ru, rv     = f.u + bu, f.v + bv                                      -- ofl_compose3_dev's out, bit for bit
//     r2         = ru*ru + rv*rv;  s2 = (f.u*f.u + f.v*f.v) + (bu*bu + bv*bv);  lim = alpha*s2 + beta
//     consistent = covered & (r2 <= lim);  residual = covered ? sqrtf(r2) : 0
// Every operation is float32 and rounded once (__fmul_rn / __fadd_rn; sqrtf is the correctly rounded one, see vis_mag in
// ofl_visualise.hip).  This is a definition of its own, not a reference function: there is no zero-flow short cut.
//
// Mapping: lanes run along x, so the streamed loads of f / f.mask and every store are contiguous per wave-instruction.  A
// block of 4 waves covers a tile of 4 rows x 64 * PX columns, blockIdx = (tile column, tile row, field): no index division.
//   PX = 1  any W >= 1, any alignment: 8-byte f loads, 1-byte mask loads and stores.
//   PX = 2  even W with suitably aligned pointers: two pixels per lane -- one 16-byte f load, 2-byte mask loads and stores,
//           one 8-byte residual store.  x0 is even and W is even, so a lane's two pixels are inside the row together.
//           Kept because it was measured: 8 to 10 % less time than PX = 1 on the same fields at 4K x 8.
// Every tap is its own guarded 8-byte load and 1-byte mask load, as in compose3_generic_kernel.  Fetching the two taps of a
// source row as one 16-byte load at a clamped column, with two rows per lane, was measured slower and is not here.
// Reads 8 B/px of f, 8 B/px of gathered b and 2 B/px of masks; writes 1 B/px (consistent) + 1 B/px (covered, optional) +
// 4 B/px (residual, optional).  With COUNTS the block reduces its two counts through ballot + popcount and four LDS words
// per counter, then one lane issues at most one atomicAdd per counter (integer adds: the order cannot change the result);
// without COUNTS the kernel has neither LDS nor atomics.
#include "ofl_common.h"
#include "ofl_host_stage.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

struct CArgs {
    const float   *f, *b;
    const uint8_t *fm, *bm;
    uint8_t       *consistent, *covered;
    float         *residual;
    uint32_t      *counts;
    int            H, W, sign;
    float          alpha, beta;
};

// one pixel: (f.u, f.v, f.mask) against field b / bm of H x W; -> covered, consistent, residual
template <int QUANT>
__device__ __forceinline__ void consistency_pixel(const float *__restrict__ b, const uint8_t *__restrict__ bm, int H, int W, int sign,
                                                  float alpha, float beta, int x, int y, float fu, float fv, bool fmask,
                                                  bool &cov, bool &con, float &res)
{
    const Tap tp = make_tap<QUANT>(map_coord(x, fu, sign), map_coord(y, fv, sign));
    float u[4], v[4], a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = tp.iy + (k >> 1), xx = tp.ix + (k & 1);
        const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        const int s = in ? yy * W + xx : 0;                           // inside one field: H * W < 2^31
        const float2 t = in ? *reinterpret_cast<const float2 *>(b + 2 * (size_t)s) : make_float2(0.0f, 0.0f);
        u[k] = t.x;
        v[k] = t.y;
        a[k] = (in && bm[s] != 0) ? 1.0f : 0.0f;
    }
    const float bu = blend4(u[0], u[1], u[2], u[3], tp), bv = blend4(v[0], v[1], v[2], v[3], tp);
    cov = fmask & (blend4(a[0], a[1], a[2], a[3], tp) == 1.0f);
    const float ru = __fadd_rn(fu, bu), rv = __fadd_rn(fv, bv);
    const float r2 = __fadd_rn(__fmul_rn(ru, ru), __fmul_rn(rv, rv));
    const float s2 = __fadd_rn(__fadd_rn(__fmul_rn(fu, fu), __fmul_rn(fv, fv)), __fadd_rn(__fmul_rn(bu, bu), __fmul_rn(bv, bv)));
    const float lim = __fadd_rn(__fmul_rn(alpha, s2), beta);
    con = cov & (r2 <= lim);
    res = cov ? sqrtf(r2) : 0.0f;
}

template <int QUANT, int PX, bool COUNTS>
__global__ __launch_bounds__(256)
void consistency_kernel(const CArgs a)
{
    const int H = a.H, W = a.W;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = blockIdx.y * 4 + wave;
    const int x0 = (blockIdx.x * 64 + lane) * PX;
    const bool act = y < H && x0 < W;                                  // PX = 2: W is even, so x0 + 1 < W as well
    if (!COUNTS && !act) return;
    const size_t hw = (size_t)H * W, item = (size_t)blockIdx.z * hw, at = item + (size_t)y * W + x0;

    bool  cov[PX], con[PX];
    float res[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) { cov[j] = con[j] = false; res[j] = 0.0f; }
    if (act) {
        float   fu[PX], fv[PX];
        uint8_t fm[PX];
        if constexpr (PX == 2) {
            const float4 q = *reinterpret_cast<const float4 *>(a.f + 2 * at);
            const uint16_t m = *reinterpret_cast<const uint16_t *>(a.fm + at);
            fu[0] = q.x; fv[0] = q.y; fu[1] = q.z; fv[1] = q.w;
            fm[0] = (uint8_t)(m & 0xffu); fm[1] = (uint8_t)(m >> 8);
        } else {
            const float2 q = *reinterpret_cast<const float2 *>(a.f + 2 * at);
            fu[0] = q.x; fv[0] = q.y;
            fm[0] = a.fm[at];
        }
#pragma unroll
        for (int j = 0; j < PX; ++j)
            consistency_pixel<QUANT>(a.b + 2 * item, a.bm + item, H, W, a.sign, a.alpha, a.beta, x0 + j, y, fu[j], fv[j], fm[j] != 0,
                                     cov[j], con[j], res[j]);
        if constexpr (PX == 2) {
            *reinterpret_cast<uint16_t *>(a.consistent + at) = (uint16_t)((con[0] ? 1u : 0u) | (con[1] ? 0x100u : 0u));
            if (a.covered) *reinterpret_cast<uint16_t *>(a.covered + at) = (uint16_t)((cov[0] ? 1u : 0u) | (cov[1] ? 0x100u : 0u));
            if (a.residual) *reinterpret_cast<float2 *>(a.residual + at) = make_float2(res[0], res[1]);
        } else {
            a.consistent[at] = con[0] ? 1 : 0;
            if (a.covered) a.covered[at] = cov[0] ? 1 : 0;
            if (a.residual) a.residual[at] = res[0];
        }
    }

    if constexpr (COUNTS) {
        __shared__ uint32_t s_n[4][2];
        uint32_t n_cov = 0, n_con = 0;
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            n_cov += (uint32_t)__popcll(__ballot(cov[j]));
            n_con += (uint32_t)__popcll(__ballot(con[j]));
        }
        if (lane == 0) { s_n[wave][0] = n_cov; s_n[wave][1] = n_con; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t c0 = s_n[0][0] + s_n[1][0] + s_n[2][0] + s_n[3][0], c1 = s_n[0][1] + s_n[1][1] + s_n[2][1] + s_n[3][1];
            if (c0) atomicAdd(a.counts + 2 * (size_t)blockIdx.z, c0);
            if (c1) atomicAdd(a.counts + 2 * (size_t)blockIdx.z + 1, c1);
        }
    }
}

int check_consistency_args(const char *who, const void *f, const void *fm, const void *b, const void *bm, int sign, int H, int W,
                           int batch, float alpha, float beta, const void *consistent, int quant)
{
    if (!f || !fm || !b || !bm || !consistent) return fail(OFL_E_INVALID, "%s: NULL pointer (f, fm, b, bm and consistent are required)", who);
    // the taps are int16 inside cv2.remap, as for ofl_compose3
    OFL_TRY(check_field_dims(who, H, W));
    if (batch < 1 || batch > 65535) return fail(OFL_E_INVALID, "%s: batch must be in [1, 65535], got %d", who, batch);
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "%s: sign must be +1 or -1", who);
    if (!(alpha >= 0.0f) || !(beta >= 0.0f) || !__builtin_isfinite(alpha) || !__builtin_isfinite(beta))
        return fail(OFL_E_INVALID, "%s: alpha and beta must be finite and not negative (got %g, %g)", who, (double)alpha, (double)beta);
    if (quant != OFL_QUANT_OPENCV && quant != OFL_QUANT_EXACT) return fail(OFL_E_INVALID, "%s: bad quant", who);
    return OFL_OK;
}

template <int QUANT, int PX>
void launch_consistency(const CArgs &a, dim3 grid, hipStream_t s)
{
    if (a.counts) hipLaunchKernelGGL((consistency_kernel<QUANT, PX, true>), grid, dim3(256), 0, s, a);
    else          hipLaunchKernelGGL((consistency_kernel<QUANT, PX, false>), grid, dim3(256), 0, s, a);
}

}  // namespace

extern "C" {

int ofl_consistency_dev(const float *f, const uint8_t *fm, const float *b, const uint8_t *bm, int sign,
                        int H, int W, int batch, float alpha, float beta,
                        uint8_t *consistent, uint8_t *covered, float *residual, uint32_t *counts,
                        int quant, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_consistency_args("ofl_consistency", f, fm, b, bm, sign, H, W, batch, alpha, beta, consistent, quant));
    if (!host_aligned(f, 8) || !host_aligned(b, 8)) return fail(OFL_E_INVALID, "ofl_consistency: f and b must be 8-byte aligned");
    if (!host_aligned(residual, 4) || !host_aligned(counts, 4)) return fail(OFL_E_INVALID, "ofl_consistency: residual and counts must be 4-byte aligned");
    CArgs a = { f, b, fm, bm, consistent, covered, residual, counts, H, W, sign, alpha, beta };
    // two pixels per lane need both of them in the row (even W: the fields' offsets are then even too) and aligned pointers
    const bool px2 = W % 2 == 0 && host_aligned(f, 16) && host_aligned(fm, 2) && host_aligned(consistent, 2) &&
                     host_aligned(covered, 2) && host_aligned(residual, 8);
    const int cols = px2 ? 128 : 64;
    const dim3 grid((unsigned)((W + cols - 1) / cols), (unsigned)((H + 3) / 4), (unsigned)batch);
    hipStream_t s = stream_of(stream);
    if (quant == OFL_QUANT_OPENCV) { if (px2) launch_consistency<OFL_QUANT_OPENCV, 2>(a, grid, s); else launch_consistency<OFL_QUANT_OPENCV, 1>(a, grid, s); }
    else                           { if (px2) launch_consistency<OFL_QUANT_EXACT, 2>(a, grid, s);  else launch_consistency<OFL_QUANT_EXACT, 1>(a, grid, s); }
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_consistency(const float *f, const uint8_t *fm, const float *b, const uint8_t *bm, int sign,
                    int H, int W, int batch, float alpha, float beta,
                    uint8_t *consistent, uint8_t *covered, float *residual, uint32_t *counts_host, int quant)
{
    OFL_TRY(need_device());
    OFL_TRY(check_consistency_args("ofl_consistency", f, fm, b, bm, sign, H, W, batch, alpha, beta, consistent, quant));
    const size_t n = (size_t)batch * H * W;
    HostStage st("ofl_consistency");
    auto df = st.in(f, n * 2), db = st.in(b, n * 2);
    auto dfm = st.in(fm, n), dbm = st.in(bm, n);
    auto con = st.out(consistent, n), cov = st.out(covered, n);
    auto res = st.out(residual, n);
    auto cnt = st.out(counts_host, (size_t)batch * 2, true);      // the launch adds to the counts
    OFL_TRY(st.upload());
    OFL_TRY(ofl_consistency_dev(df, dfm, db, dbm, sign, H, W, batch, alpha, beta, con, cov, res, cnt, quant, st.stream()));
    return st.download();
}

}  // extern "C"
