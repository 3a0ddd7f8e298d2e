// ofl_census.hip -- K22: census distance of a warp over a window (gfx950).
//
// K21 asks whether a pixel looks the same where the field sends it and compares raw values; K22 compares the ORDER of the
// intensities in a K x K window around the pixel, in `near` and in the warped `far`, so a change of exposure or gain that
// keeps the order costs nothing (Zabih & Woodfill; the ternary census of UnFlow / DDFlow / ARFlow / UFlow / SMURF).
// Per item n and pixel q, every operation float32 and rounded once, exactly as K21 computes them:
//     tap(q), w_c(q), am(q);  cov1(q) = f.mask & near_mask & (am == 1.0f)                       -- K21's `covered`
//     A(q) = (near_0 + ... + near_(C-1)) * inv_c,  B(q) = (w_0 + ... + w_(C-1)) * inv_c           -- ascending c from +0.0f
//     member(q) = q inside the frame & cov1(q)
// and for the pixel p and every offset d = (dx, dy), |dx|, |dy| <= r = K / 2, d != 0:
//     a = A(p + d) - A(p),  b = B(p + d) - B(p)
//     hard:  s(v) = v > delta ? 1 : (v < -delta ? -1 : 0);  t_d = s(a) != s(b) ? 1.0f : 0.0f
//     soft:  rho(v) = v / sqrtf(noise + v * v);  g = rho(a) - rho(b);  q = g * g;  t_d = q / (knee + q)
//     t_d = +0.0f where !member(p + d)                                                            -- a select, not a product
//     R_dy = t_(-r,dy) + ... + t_(r,dy) from +0.0f;  S = R_(-r) + ... + R_r from +0.0f;  n = the member offsets
//     covered = cov1(p) & (n >= min_count);  e = S / (float)n;  err = covered ? e : 0.0f;  within = covered & (e <= tau)
// There is no zero-flow short cut.  16-bit elements are widened exactly.
//
// One workgroup of 256 threads per tile of 64 x 16 pixels of one item (K16's shape), lanes along x.
//   Staging  stage_warped_tile (ofl_photo_dev.h, shared with K23): the (64 + 2r) x (16 + 2r) pixels of the tile and its halo are
//            dealt to the threads, up to 7 each, and A, B and member go to LDS: two float planes and one byte plane, kept
//            apart, so a wave reads 64 consecutive words.  The warped image is never written.
//   Window   a thread owns 4 consecutive rows of one column.  It walks the K + 3 tile rows its four windows span once; of
//            each it reads the K values of A, B and member into registers and adds that row's R_dy to every centre whose
//            window holds the row -- ascending rows are ascending dy for each centre, so the stated order is kept -- which
//            takes (K + 3) K LDS reads per plane where four separate walks take 4 K^2.  The row loop is a real loop (its
//            body holds 4 K terms; unrolled it would be 4 K^2 of them, 196 correctly rounded rho pairs at K = 7); every
//            register array is indexed by unrolled constants only, so nothing goes to scratch.  The centre's own position
//            adds +0.0f, which is exact because every term is >= +0 or NaN.  A row's member count is formed once and serves
//            its four centres.  Hard mode counts its terms in an integer and converts once: every partial sum of the stated
//            order is an integer of at most 48, exact in float32, so the bits are the same, and s(a) != s(b) is four
//            compares and mask logic.
// Epilogue: window_finish (ofl_photo_dev.h, shared with K26) -- covered, the stores of error_store and the counts in K21's
// scheme (ballot + popcount, at most one integer atomicAdd per workgroup and counter); no other atomics, no workspace, 64-bit
// element offsets.  36 instantiations: 3 element types x 2 quant x 3 windows x 2 modes.
//
// OUT OF SCOPE: C > 4 and a per-channel census, luma weights, gradient constancy (SSIM is K26), windows above 7 or not square, a
// reduction of the map, a backward pass, mixed element types or layouts, integer tensors.
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_photo_dev.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

struct CArgs {                              // PairArgs' members by name, in the order the kernel was measured with (ofl_photo_dev.h)
    const void    *near, *far;
    const float   *flow;
    const uint8_t *fmask, *near_mask, *far_mask;
    float         *err;
    uint8_t       *covered, *within;
    uint32_t      *counts;
    int            N, C, H, W, sign, min_count;
    float          p0, p1, tau, inv_c;      // hard: p0 = delta; soft: p0 = noise, p1 = knee
    size_t         step;
    size_t         s_px, s_ch;
};

// hard mode: s(a) != s(b).  delta >= 0, so v > delta and v < -delta exclude each other and the two signs are equal exactly when
// both comparisons agree: four compares and mask logic, no select
__device__ __forceinline__ bool census_differs(float a, float b, float delta)
{
    return ((a > delta) != (b > delta)) | ((a < -delta) != (b < -delta));           // a NaN compares false twice: s = 0
}

// soft mode: t_d of one offset from a = A(p + d) - A(p) and b = B(p + d) - B(p)
__device__ __forceinline__ float census_soft(float a, float b, float noise, float knee)
{
    const float ra = __fdiv_rn(a, sqrtf(__fadd_rn(noise, __fmul_rn(a, a))));
    const float rb = __fdiv_rn(b, sqrtf(__fadd_rn(noise, __fmul_rn(b, b))));
    const float g = __fsub_rn(ra, rb), q = __fmul_rn(g, g);
    return __fdiv_rn(q, __fadd_rn(knee, q));
}

template <int E, int QUANT, int K, int MODE>
__global__ __launch_bounds__(256)
void census_kernel(const CArgs a)
{
    constexpr int R = K / 2, TW = kTX + 2 * R, TH = kTY + 2 * R, NE = TW * TH;
    __shared__ float   s_a[NE], s_b[NE];
    __shared__ uint8_t s_m[NE];

    const int n = blockIdx.z, x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;

    stage_warped_tile<E, QUANT, R, kTX, kTY>(a, n, x0, y0, s_a, s_b, s_m);           // ofl_photo_dev.h
    __syncthreads();

    // ------------------------------------------------------------------------------------------ window
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int top = kRows * wave;                           // the first tile row of this thread's windows
    float ca[kRows], cb[kRows], S[kRows];
    int   cnt[kRows], diff[kRows];
    bool  cm[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int at = (top + R + j) * TW + lane + R;
        ca[j] = s_a[at]; cb[j] = s_b[at]; cm[j] = s_m[at] != 0;
        S[j] = 0.0f; cnt[j] = 0; diff[j] = 0;
    }
    const float p0 = a.p0, p1 = a.p1;
#pragma unroll 1
    for (int i = 0; i < K + kRows - 1; ++i) {
        const int at = (top + i) * TW + lane;
        float ra[K], rb[K];
        bool  rm[K];
        int   members = 0;                                                  // of this tile row: the same for every centre
#pragma unroll
        for (int d = 0; d < K; ++d) { ra[d] = s_a[at + d]; rb[d] = s_b[at + d]; rm[d] = s_m[at + d] != 0; members += rm[d] ? 1 : 0; }
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            if ((unsigned)(i - j) > (unsigned)(2 * R)) continue;            // uniform: dy = i - j - R outside the window
            const bool mid = i - j == R;                                    // the centre's own row: d = R is the centre itself
            cnt[j] += members - (mid && rm[R] ? 1 : 0);
            if constexpr (MODE == OFL_CENSUS_HARD) {
                // every term is 0 or 1, so every partial sum of the stated order is an integer of at most 48 and exact in
                // float32: the terms are counted, and the count is converted once -- the same bits
#pragma unroll
                for (int d = 0; d < K; ++d)
                    diff[j] += rm[d] && !(d == R && mid) && census_differs(__fsub_rn(ra[d], ca[j]), __fsub_rn(rb[d], cb[j]), p0) ? 1 : 0;
            } else {
                float row = 0.0f;
#pragma unroll
                for (int d = 0; d < K; ++d) {
                    const float t = census_soft(__fsub_rn(ra[d], ca[j]), __fsub_rn(rb[d], cb[j]), p0, p1);
                    row = __fadd_rn(row, rm[d] && !(d == R && mid) ? t : 0.0f);
                }
                S[j] = __fadd_rn(S[j], row);
            }
        }
    }

    float e[kRows];                                                                 // hard: the count, converted once
#pragma unroll
    for (int j = 0; j < kRows; ++j) e[j] = __fdiv_rn(MODE == OFL_CENSUS_HARD ? (float)diff[j] : S[j], (float)cnt[j]);
    window_finish(a, n, x0, y0, cm, cnt, e);                                        // ofl_photo_dev.h
}

int check_census_args(const char *who, const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                      const void *flow, const void *fmask, int sign, int window, int mode, float p0, float p1, int min_count,
                      float tau, const void *err, const void *within, int quant)
{
    OFL_TRY(check_error_map_inputs(who, near, far, flow, fmask, elem, layout, N, C, OFL_CENSUS_MAX_C, H, W, sign, quant));
    if (window != 3 && window != 5 && window != 7) return fail(OFL_E_INVALID, "%s: window must be 3, 5 or 7, got %d", who, window);
    if (mode == OFL_CENSUS_HARD) {
        if (!finite_not_negative(p0)) return fail(OFL_E_INVALID, "%s: delta must be finite and not negative (got %g)", who, (double)p0);
    } else if (mode == OFL_CENSUS_SOFT) {
        if (!finite_positive(p0)) return fail(OFL_E_INVALID, "%s: noise must be finite and positive (got %g)", who, (double)p0);
        if (!finite_positive(p1)) return fail(OFL_E_INVALID, "%s: knee must be finite and positive (got %g)", who, (double)p1);
    } else {
        return fail(OFL_E_INVALID, "%s: bad mode %d", who, mode);
    }
    if (min_count < 1 || min_count > window * window - 1)
        return fail(OFL_E_INVALID, "%s: min_count must be in [1, %d], got %d", who, window * window - 1, min_count);
    return check_error_map_outputs(who, err, within, tau);
}

template <int E, int QUANT, int K>
void launch_census(const CArgs &a, int mode, hipStream_t s)
{
    const dim3 grid = window_grid(a.N, a.H, a.W);
    if (mode == OFL_CENSUS_HARD) hipLaunchKernelGGL((census_kernel<E, QUANT, K, OFL_CENSUS_HARD>), grid, dim3(256), 0, s, a);
    else                         hipLaunchKernelGGL((census_kernel<E, QUANT, K, OFL_CENSUS_SOFT>), grid, dim3(256), 0, s, a);
}

}  // namespace

extern "C" {

int ofl_census_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                   const float *flow, const uint8_t *fmask, int flow_shared, int sign,
                   const uint8_t *near_mask, const uint8_t *far_mask,
                   int window, int mode, float p0, float p1, int min_count, float tau,
                   float *err, uint8_t *covered, uint8_t *within, uint32_t *counts, int quant, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_census_args("ofl_census", near, far, elem, layout, N, C, H, W, flow, fmask, sign, window, mode, p0, p1, min_count, tau,
                              err, within, quant));
    CArgs a;
    OFL_TRY(error_map_fill("ofl_census", a, near, far, elem, layout, N, C, H, W, flow, fmask, flow_shared != 0, sign, near_mask, far_mask,
                           err, covered, within, counts, tau));
    a.min_count = min_count;
    a.p0 = p0; a.p1 = p1;
    hipStream_t s = stream_of(stream);
    with_elem(elem, [&](auto E) { with_quant(quant, [&](auto Q) {
        switch (window) {
        case 3:  launch_census<E.value, Q.value, 3>(a, mode, s); break;
        case 5:  launch_census<E.value, Q.value, 5>(a, mode, s); break;
        default: launch_census<E.value, Q.value, 7>(a, mode, s); break;
        }
    }); });
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_census(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
               const float *flow, const uint8_t *fmask, int flow_shared, int sign,
               const uint8_t *near_mask, const uint8_t *far_mask,
               int window, int mode, float p0, float p1, int min_count, float tau,
               float *err, uint8_t *covered, uint8_t *within, uint32_t *counts_host, int quant)
{
    OFL_TRY(need_device());
    OFL_TRY(check_census_args("ofl_census", near, far, elem, layout, N, C, H, W, flow, fmask, sign, window, mode, p0, p1, min_count, tau,
                              err, within, quant));
    return error_map_host("ofl_census", ofl_census_dev, near, far, elem, layout, N, C, H, W, flow, fmask, flow_shared, sign, near_mask, far_mask,
                          err, covered, within, counts_host, quant, window, mode, p0, p1, min_count, tau);
}

}  // extern "C"
