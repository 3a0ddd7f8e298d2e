// ofl_ssim.hip -- K26: structural similarity of a warp over a window (gfx950).
//
// K21 compares raw values and K22 their order; K26 compares the local mean, variance and covariance of the intensities in a
// K x K weighted window around the pixel, in `near` and in the warped `far`: Wang et al.'s SSIM (the 11 x 11 Gaussian window)
// and, with a uniform window, the avg_pool2d form in the photometric loss of UnFlow / DDFlow / ARFlow / UFlow / SMURF.  The
// output is the dissimilarity (1 - SSIM) / 2 in [0, 1].  Per item n and pixel q, every operation float32 and rounded once:
//     tap(q), w_c(q), am(q), cov1(q), A(q), B(q)                                              -- K22's (stage_warped_tile)
//     member(q) = q inside the frame & cov1(q)
// and for the pixel p, the window rows dy = -r ... r and in each dx = -r ... r (the centre included), q = p + (dx, dy):
//     ga = g[dx+r] * A(q);  gb = g[dx+r] * B(q)
//     the six terms g[dx+r], ga, gb, ga * A(q), gb * B(q), ga * B(q), each +0.0f where !member(q)         -- a select
//     R^k_dy = the row sum of term k in ascending dx from +0.0f
//     S^k = g[0] * R^k_(-r) + ... + g[K-1] * R^k_r, one product and one addition a row, ascending dy, from +0.0f
//     (Wt, Sa, Sb, Saa, Sbb, Sab) = S^0 ... S^5;  n = the members of the window
//     mu_a = Sa / Wt;  mu_b = Sb / Wt;  va = Saa / Wt - mu_a * mu_a;  vb = Sbb / Wt - mu_b * mu_b;  vab = Sab / Wt - mu_a * mu_b
//     num = (2 * (mu_a * mu_b) + c1) * (2 * vab + c2);  den = ((mu_a * mu_a + mu_b * mu_b) + c1) * ((va + vb) + c2)
//     s = num / den;  e = (1 - s) * 0.5;  e = e < 0 ? 0 : (e > 1 ? 1 : e)                                 -- a NaN stays a NaN
//     covered = cov1(p) & (n >= min_count);  err = covered ? e : 0.0f;  within = covered & (e <= tau)
// There is no zero-flow short cut.  16-bit elements are widened exactly.
//
// One workgroup of 256 threads per tile of 64 x 16 pixels of one item (K22's frame), lanes along x.
//   Staging  stage_warped_tile (ofl_photo_dev.h), unchanged: the (64 + 2r) x (16 + 2r) pixels of the tile and its halo are
//            dealt to the threads, up to 8 each at r = 5, and A, B and member go to LDS: two float planes and one byte
//            plane.  Nothing else is in LDS but the eight words of the counts: 9 (64 + 2r)(16 + 2r) bytes rounded up to 16,
//            plus 32 -- 10736, 12272, 13904 and 17360 bytes for K = 3, 5, 7, 11.  The warped image is never written.
//   Window   a thread owns 4 consecutive rows of one column.  It walks the K + 3 tile rows its four windows span once; of
//            each it reads the K values of A, B and member and forms the six row sums ONCE -- they do not depend on the
//            centre -- and then adds g[dy + r] * R to every centre whose window holds the row: ascending tile rows are
//            ascending dy for each centre, so the stated order is kept.  That is (K + 3) K LDS reads a plane where four
//            separate walks take 4 K^2, and 6 K row terms a tile row where K22's soft mode has 4 K.  The row loop is a
//            real loop: unrolled, the compiler hoists the LDS reads of all K + 3 rows and K = 11 drops to one wave per
//            SIMD with spilled scalars.  Every register array is indexed by unrolled constants only; the taps are passed
//            by value, the column's tap at a constant offset of the kernel arguments and the row's tap g[i - j] by a
//            wave-uniform index -- a scalar load, no register array --, so nothing goes to scratch.
// Epilogue: window_finish (ofl_photo_dev.h, shared with K22) -- covered, the stores of error_store and the counts in K21's
// scheme (ballot + popcount, at most one integer atomicAdd per workgroup and counter); no other atomics, no workspace, 64-bit
// element offsets.  24 instantiations: 3 element types x 2 quant x 4 windows.
//
// OUT OF SCOPE: C > 4 and a per-channel SSIM, luma weights, sample (N - 1) moments, windows that are not square or of another
// size, MS-SSIM, the three components as outputs, gradient constancy, a reduction of the map, PSNR, a backward pass, mixed
// element types or layouts, integer tensors.
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_photo_dev.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

constexpr int kMaxTaps = 11;

struct SArgs {                              // PairArgs' members by name, in K22's order (ofl_photo_dev.h); the taps behind
    const void    *near, *far;
    const float   *flow;
    const uint8_t *fmask, *near_mask, *far_mask;
    float         *err;
    uint8_t       *covered, *within;
    uint32_t      *counts;
    int            N, C, H, W, sign, min_count;
    float          c1, c2, tau, inv_c;
    size_t         step;
    size_t         s_px, s_ch;
    float          g[kMaxTaps];             // the 1-D window, by value: g[0 ... K-1]
};

// (1 - SSIM) / 2 of the six weighted sums, clamped to [0, 1]; a NaN stays a NaN
__device__ __forceinline__ float ssim_error(const float (&S)[6], float c1, float c2)
{
    const float mu_a = __fdiv_rn(S[1], S[0]), mu_b = __fdiv_rn(S[2], S[0]);
    const float aa = __fmul_rn(mu_a, mu_a), bb = __fmul_rn(mu_b, mu_b), ab = __fmul_rn(mu_a, mu_b);
    const float va = __fsub_rn(__fdiv_rn(S[3], S[0]), aa), vb = __fsub_rn(__fdiv_rn(S[4], S[0]), bb);
    const float vab = __fsub_rn(__fdiv_rn(S[5], S[0]), ab);
    const float num = __fmul_rn(__fadd_rn(__fmul_rn(2.0f, ab), c1), __fadd_rn(__fmul_rn(2.0f, vab), c2));
    const float den = __fmul_rn(__fadd_rn(__fadd_rn(aa, bb), c1), __fadd_rn(__fadd_rn(va, vb), c2));
    const float e = __fmul_rn(__fsub_rn(1.0f, __fdiv_rn(num, den)), 0.5f);
    return e < 0.0f ? 0.0f : (e > 1.0f ? 1.0f : e);
}

template <int E, int QUANT, int K>
__global__ __launch_bounds__(256)
void ssim_kernel(const SArgs a)
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
    float S[kRows][6];
    int   cnt[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        cnt[j] = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) S[j][k] = 0.0f;
    }
#pragma unroll 1
    for (int i = 0; i < K + kRows - 1; ++i) {
        const int at = (top + i) * TW + lane;
        float row[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};                 // of this tile row: the same for every centre
        int   members = 0;
#pragma unroll
        for (int d = 0; d < K; ++d) {
            const float A = s_a[at + d], B = s_b[at + d], g = a.g[d];
            const bool  m = s_m[at + d] != 0;
            const float ga = __fmul_rn(g, A), gb = __fmul_rn(g, B);
            const float t[6] = {g, ga, gb, __fmul_rn(ga, A), __fmul_rn(gb, B), __fmul_rn(ga, B)};
#pragma unroll
            for (int k = 0; k < 6; ++k) row[k] = __fadd_rn(row[k], m ? t[k] : 0.0f);
            members += m ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            if ((unsigned)(i - j) > (unsigned)(2 * R)) continue;            // uniform: dy = i - j - R outside the window
            const float gy = a.g[i - j];                                    // uniform: a scalar load from the kernel arguments
#pragma unroll
            for (int k = 0; k < 6; ++k) S[j][k] = __fadd_rn(S[j][k], __fmul_rn(gy, row[k]));
            cnt[j] += members;
        }
    }

    bool  cm[kRows];
    float e[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) { cm[j] = s_m[(top + R + j) * TW + lane + R] != 0; e[j] = ssim_error(S[j], a.c1, a.c2); }
    window_finish(a, n, x0, y0, cm, cnt, e);                                        // ofl_photo_dev.h
}

int check_ssim_args(const char *who, const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                    const void *flow, const void *fmask, int sign, int window, const float *taps, float c1, float c2,
                    int min_count, float tau, const void *err, const void *within, int quant)
{
    OFL_TRY(check_error_map_inputs(who, near, far, flow, fmask, elem, layout, N, C, OFL_SSIM_MAX_C, H, W, sign, quant));
    if (window != 3 && window != 5 && window != 7 && window != 11)
        return fail(OFL_E_INVALID, "%s: window must be 3, 5, 7 or 11, got %d", who, window);
    if (!taps) return fail(OFL_E_INVALID, "%s: taps must not be NULL (a host pointer to %d float32 values)", who, window);
    for (int i = 0; i < window; ++i)
        if (!finite_positive(taps[i])) return fail(OFL_E_INVALID, "%s: taps[%d] must be finite and positive (got %g)", who, i, (double)taps[i]);
    if (!finite_positive(c1)) return fail(OFL_E_INVALID, "%s: c1 must be finite and positive (got %g)", who, (double)c1);
    if (!finite_positive(c2)) return fail(OFL_E_INVALID, "%s: c2 must be finite and positive (got %g)", who, (double)c2);
    if (min_count < 1 || min_count > window * window)
        return fail(OFL_E_INVALID, "%s: min_count must be in [1, %d], got %d", who, window * window, min_count);
    return check_error_map_outputs(who, err, within, tau);
}

template <int E, int QUANT, int K>
void launch_ssim(const SArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL((ssim_kernel<E, QUANT, K>), window_grid(a.N, a.H, a.W), dim3(256), 0, s, a);
}

}  // namespace

extern "C" {

int ofl_ssim_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                 const float *flow, const uint8_t *fmask, int flow_shared, int sign,
                 const uint8_t *near_mask, const uint8_t *far_mask,
                 int window, const float *taps, float c1, float c2, int min_count, float tau,
                 float *err, uint8_t *covered, uint8_t *within, uint32_t *counts, int quant, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_ssim_args("ofl_ssim", near, far, elem, layout, N, C, H, W, flow, fmask, sign, window, taps, c1, c2, min_count, tau,
                            err, within, quant));
    SArgs a;
    OFL_TRY(error_map_fill("ofl_ssim", a, near, far, elem, layout, N, C, H, W, flow, fmask, flow_shared != 0, sign, near_mask, far_mask,
                           err, covered, within, counts, tau));
    a.min_count = min_count;
    a.c1 = c1; a.c2 = c2;
    for (int i = 0; i < kMaxTaps; ++i) a.g[i] = i < window ? taps[i] : 0.0f;        // read here: the caller may free them on return
    hipStream_t s = stream_of(stream);
    with_elem(elem, [&](auto E) { with_quant(quant, [&](auto Q) {
        switch (window) {
        case 3:  launch_ssim<E.value, Q.value, 3>(a, s); break;
        case 5:  launch_ssim<E.value, Q.value, 5>(a, s); break;
        case 7:  launch_ssim<E.value, Q.value, 7>(a, s); break;
        default: launch_ssim<E.value, Q.value, 11>(a, s); break;
        }
    }); });
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_ssim(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
             const float *flow, const uint8_t *fmask, int flow_shared, int sign,
             const uint8_t *near_mask, const uint8_t *far_mask,
             int window, const float *taps, float c1, float c2, int min_count, float tau,
             float *err, uint8_t *covered, uint8_t *within, uint32_t *counts_host, int quant)
{
    OFL_TRY(need_device());
    OFL_TRY(check_ssim_args("ofl_ssim", near, far, elem, layout, N, C, H, W, flow, fmask, sign, window, taps, c1, c2, min_count, tau,
                            err, within, quant));
    return error_map_host("ofl_ssim", ofl_ssim_dev, near, far, elem, layout, N, C, H, W, flow, fmask, flow_shared, sign, near_mask, far_mask,
                          err, covered, within, counts_host, quant, window, taps, c1, c2, min_count, tau);
}

}  // extern "C"
