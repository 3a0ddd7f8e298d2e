// ofl_inverse_search.hip -- K24: dense inverse search of a field on two images (gfx950).
//
// K23 moves a vector a fraction of a pixel; K24 finds it: the patch inverse search and the densification of Dense Inverse
// Search (Kroeger et al., ECCV 2016; OpenCV's DISOpticalFlow), the partner of the variational refinement.  Every patch of
// P x P pixels on a grid of stride S takes `iterations` inverse-compositional Lucas-Kanade translation steps on the channel
// means of the two images, then every pixel takes the weighted average of the patches that cover it.  The definition, with
// the order of every float32 operation, is the K24 block of include/ofl.h; tests/inverse_search_ref.py restates it in NumPy
// and the device equals it bit for bit.  Every operation is float32 and rounded once (no FMA); the divisions are the
// correctly rounded ones.
//
// Launches, all on one stream, three of them:
//   setup    one thread per pixel: A and Bm, the channel means of `near` and of the UNWARPED `far`, two float32 planes in the
//            workspace, so that a tap of the search costs one plane whatever C is.  3 instantiations (element type).
//   search   one wave per 8 x 8 patch, lane = ly * 8 + lx; for P = 4 a wave holds four patches of 16 lanes.  T, gx and gy
//            stay in registers for all iterations; every sum of a patch is an xor butterfly across its lanes (masks 1, 2, 4,
//            ...), which is the pairwise tree of the definition because float addition is commutative, and leaves the same
//            bits in every lane, so the stop rules are uniform over a patch and are applied by predication: every lane runs
//            to the end of the loop, or until no patch of the wave is still searching.  No LDS, no atomics, 12 bytes
//            written per patch.  4 instantiations: P in {4, 8} x quant.
//   densify  one thread per pixel: loops over the patches that contain it (at most ceil(P / S) + 1 per axis) in row-major
//            grid order, samples Bm once per patch and writes out and out_mask.  2 instantiations (quant).
// Workspace, caller-provided: 8 N H W bytes (A, Bm) plus 12 bytes per patch where the caller passes no patch buffers.
// 64-bit offsets across items; inside one plane H * W < 2^31.
//
// OUT OF SCOPE: OpenCV's spatial propagation between neighbouring patches and its early-exit heuristics, patches of 12 / 16
// px, per-channel residuals and C > 4, near_mask / far_mask, affine patch models, a pyramid or a fused multi-level launch
// (device.estimate_flow loops over levels in Python), a backward pass.
#include <math.h>
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_host_stage.h"
#include "ofl_photo_dev.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

struct IArgs : PairArgs {                   // flow NULL: the zero field; fmask NULL: all set; near_mask, far_mask: NULL
    float         *pa, *pb;                 // the planes A and Bm, [N][H][W]
    float2        *pv;                      // patch vectors [N][ny][nx]
    float         *pssd;                    // patch ssd [N][ny][nx] or NULL
    int            ny, nx, stride, iterations, normalise;
    float          floor;
    float         *out;
    uint8_t       *out_mask;
};

// origin i of the patch grid along an axis of length n: 0, S, 2 S, ... and n - P for the last
__device__ __forceinline__ int origin_of(int i, int stride, int last) { return min(i * stride, last); }

template <int E>
__global__ __launch_bounds__(256)
void isearch_setup_kernel(const IArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t hw = (size_t)a.H * a.W, pix = (size_t)y * a.W + x, item = (size_t)blockIdx.z;
    a.pa[item * hw + pix] = channel_mean<E>(a.near, item * a.C * hw, pix, a.s_px, a.s_ch, a.C, a.inv_c);
    a.pb[item * hw + pix] = channel_mean<E>(a.far, item * a.C * hw, pix, a.s_px, a.s_ch, a.C, a.inv_c);
}

// S(q, u): the bilinear blend of the plane at q + sign * u, the position clamped to the frame first.  u is finite.  After
// the clamp only the taps at column W or row H can lie outside; they count as +0.0f (K21's rule) and carry the weight 0.
template <int QUANT>
__device__ __forceinline__ float sample_clamped(const float *__restrict__ plane, int x, int y, float ux, float uy, int sign, int H, int W)
{
    const float px = fminf(fmaxf(map_coord(x, ux, sign), 0.0f), (float)(W - 1));
    const float py = fminf(fmaxf(map_coord(y, uy, sign), 0.0f), (float)(H - 1));
    const Tap tp = make_tap<QUANT>(px, py);
    bool in[4];
    int  off[4];
    tap_frame(tp, H, W, in, off);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t = plane[off[k]];
        v[k] = in[k] ? t : 0.0f;
    }
    return blend4(v[0], v[1], v[2], v[3], tp);
}

// the tree sum of the definition over the P * P lanes of a patch; every lane of the patch gets the same bits
template <int P>
__device__ __forceinline__ float patch_sum(float v)
{
#pragma unroll
    for (int m = 1; m < P * P; m <<= 1) v = __fadd_rn(v, __shfl_xor(v, m));
    return v;
}

template <int P, int QUANT>
__global__ __launch_bounds__(256)
void isearch_search_kernel(const IArgs a)
{
    constexpr int PP = P * P, PER_WAVE = 64 / PP;
    constexpr float kInv = 1.0f / (float)PP, kFar = (float)PP;
    const int H = a.H, W = a.W, sign = a.sign;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_patch = a.ny * a.nx;
    int patch = (blockIdx.x * 4 + wave) * PER_WAVE + lane / PP;
    if (PER_WAVE == 1 && patch >= n_patch) return;                       // wave-uniform
    const bool real = patch < n_patch;                                   // P = 4: the surplus patches of the last wave repeat the last one
    patch = min(patch, n_patch - 1);
    const int iy = patch / a.nx, ix = patch - iy * a.nx;
    const int ox = origin_of(ix, a.stride, W - P), oy = origin_of(iy, a.stride, H - P);
    const int l = lane & (PP - 1), x = ox + l % P, y = oy + l / P;
    const size_t hw = (size_t)H * W, item = (size_t)blockIdx.y;
    const float *__restrict__ pa = a.pa + item * hw, *__restrict__ pb = a.pb + item * hw;
    const int at = y * W + x;

    float2 u0 = make_float2(0.0f, 0.0f);
    if (a.flow) {
        const size_t c = item * hw + (size_t)(oy + P / 2) * W + (ox + P / 2);
        const float2 f = *reinterpret_cast<const float2 *>(a.flow + 2 * c);
        if ((a.fmask ? a.fmask[c] != 0 : true) && finite32(f.x) && finite32(f.y)) u0 = f;
    }

    const float Ac = pa[at];
    const float Ax = __fmul_rn(0.5f, __fsub_rn(x + 1 < W ? pa[at + 1] : Ac, x > 0 ? pa[at - 1] : Ac));
    const float Ay = __fmul_rn(0.5f, __fsub_rn(y + 1 < H ? pa[at + W] : Ac, y > 0 ? pa[at - W] : Ac));
    const float gx = sign > 0 ? Ax : -Ax, gy = sign > 0 ? Ay : -Ay;
    const float T = a.normalise ? __fsub_rn(Ac, __fmul_rn(patch_sum<P>(Ac), kInv)) : Ac;
    const float H11 = patch_sum<P>(__fmul_rn(gx, gx)), H12 = patch_sum<P>(__fmul_rn(gx, gy)), H22 = patch_sum<P>(__fmul_rn(gy, gy));
    const float det = __fsub_rn(__fmul_rn(H11, H22), __fmul_rn(H12, H12));

    float2 u = u0, ubest = u0;
    float s = sample_clamped<QUANT>(pb, x, y, u.x, u.y, sign, H, W);
    if (a.normalise) s = __fsub_rn(s, __fmul_rn(patch_sum<P>(s), kInv));
    float r = __fsub_rn(s, T);
    float best = patch_sum<P>(__fmul_rn(r, r));
    if (!finite32(best)) best = INFINITY;
    bool searching = finite32(det) && det > 0.0f;

    for (int it = 0; it < a.iterations; ++it) {
        if (!__any(searching)) break;
        const float b1 = patch_sum<P>(__fmul_rn(r, gx)), b2 = patch_sum<P>(__fmul_rn(r, gy));
        const float du = __fdiv_rn(__fsub_rn(__fmul_rn(H22, b1), __fmul_rn(H12, b2)), det);
        const float dv = __fdiv_rn(__fsub_rn(__fmul_rn(H11, b2), __fmul_rn(H12, b1)), det);
        const float nx_ = __fsub_rn(u.x, du), ny_ = __fsub_rn(u.y, dv);
        const float ex = __fsub_rn(nx_, u0.x), ey = __fsub_rn(ny_, u0.y);
        const float d2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
        searching = searching && finite32(nx_) && finite32(ny_) && !(d2 > kFar);
        if (searching) u = make_float2(nx_, ny_);                        // a patch that stopped keeps its finite u: every tap stays defined
        s = sample_clamped<QUANT>(pb, x, y, u.x, u.y, sign, H, W);
        if (a.normalise) s = __fsub_rn(s, __fmul_rn(patch_sum<P>(s), kInv));
        const float rn = __fsub_rn(s, T);
        const float ssd = patch_sum<P>(__fmul_rn(rn, rn));
        if (searching) {
            r = rn;
            if (ssd < best) { best = ssd; ubest = u; }
        }
    }
    if (real && l == 0) {
        const size_t p = item * n_patch + patch;
        a.pv[p] = ubest;
        if (a.pssd) a.pssd[p] = best;
    }
}

template <int QUANT>
__global__ __launch_bounds__(256)
void isearch_densify_kernel(const IArgs a, int P)
{
    const int H = a.H, W = a.W;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t hw = (size_t)H * W, item = (size_t)blockIdx.z, pix = (size_t)y * W + x;
    const float *__restrict__ pb = a.pb + item * hw;
    const float2 *__restrict__ pv = a.pv + item * a.ny * a.nx;
    const float Aq = a.pa[item * hw + pix];
    const int S = a.stride;
    // the patches that contain x: origins are monotone, the last one is W - P
    const int ix0 = min(max(0, (x - P + S) / S), a.nx - 1), ix1 = x >= W - P ? a.nx - 1 : x / S;
    const int iy0 = min(max(0, (y - P + S) / S), a.ny - 1), iy1 = y >= H - P ? a.ny - 1 : y / S;
    float sw = 0.0f, sx = 0.0f, sy = 0.0f;
    for (int iy = iy0; iy <= iy1; ++iy) {
        for (int ix = ix0; ix <= ix1; ++ix) {
            const float2 u = pv[iy * a.nx + ix];
            const float d = fabsf(__fsub_rn(sample_clamped<QUANT>(pb, x, y, u.x, u.y, a.sign, H, W), Aq));
            const float w = __fdiv_rn(1.0f, d < a.floor ? a.floor : d);                   // a NaN difference stays a NaN weight
            sw = __fadd_rn(sw, w);
            sx = __fadd_rn(sx, __fmul_rn(w, u.x));
            sy = __fadd_rn(sy, __fmul_rn(w, u.y));
        }
    }
    const float ox = __fdiv_rn(sx, sw), oy = __fdiv_rn(sy, sw);
    const bool ok = finite32(ox) && finite32(oy);
    reinterpret_cast<float2 *>(a.out)[item * hw + pix] = ok ? make_float2(ox, oy) : make_float2(0.0f, 0.0f);
    a.out_mask[item * hw + pix] = ok ? 1 : 0;
}

int grid_count(int n, int P, int S) { return (n - P) / S + 1 + ((n - P) % S != 0 ? 1 : 0); }

int check_isearch_dims(const char *who, int N, int H, int W, int patch, int stride)
{
    if (N < 1 || N > 65535) return fail(OFL_E_INVALID, "%s: N must be in [1, 65535], got %d", who, N);
    OFL_TRY(check_field_dims(who, H, W));
    if (patch != 4 && patch != 8) return fail(OFL_E_INVALID, "%s: patch must be 4 or 8, got %d", who, patch);
    if (stride < 1 || stride > patch) return fail(OFL_E_INVALID, "%s: stride must be in [1, patch = %d], got %d", who, patch, stride);
    if (H < patch || W < patch) return fail(OFL_E_INVALID, "%s: a %d x %d image holds no %d x %d patch", who, H, W, patch, patch);
    return OFL_OK;
}

int check_isearch_args(const char *who, const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                       int sign, int patch, int stride, int iterations, float floor, const void *out, const void *out_mask, int quant)
{
    if (!near || !far || !out || !out_mask) return fail(OFL_E_INVALID, "%s: NULL pointer (near, far, out and out_mask are required)", who);
    OFL_TRY(check_pair_args(who, elem, layout, N, C, OFL_ISEARCH_MAX_C, H, W, sign, quant));
    OFL_TRY(check_isearch_dims(who, N, H, W, patch, stride));
    if (iterations < 1 || iterations > OFL_ISEARCH_MAX_ITER)
        return fail(OFL_E_INVALID, "%s: iterations must be in [1, %d], got %d", who, OFL_ISEARCH_MAX_ITER, iterations);
    if (!finite_positive(floor)) return fail(OFL_E_INVALID, "%s: floor must be finite and positive (got %g)", who, (double)floor);
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_inverse_search_workspace_bytes(int N, int H, int W, int patch, int stride, size_t *bytes)
{
    const char *who = "ofl_inverse_search_workspace_bytes";
    if (!bytes) return fail(OFL_E_INVALID, "%s: NULL pointer", who);
    OFL_TRY(check_isearch_dims(who, N, H, W, patch, stride));
    const size_t np = (size_t)grid_count(H, patch, stride) * grid_count(W, patch, stride);
    *bytes = (size_t)N * H * W * 8 + (size_t)N * np * 12;
    return OFL_OK;
}

int ofl_inverse_search_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                           const float *flow, const uint8_t *fmask, int sign, int patch, int stride, int iterations,
                           int normalise, float floor, void *workspace, size_t workspace_bytes,
                           float *out, uint8_t *out_mask, float *patch_vecs, float *patch_ssd, int quant, void *stream)
{
    const char *who = "ofl_inverse_search";
    OFL_TRY(need_device());
    OFL_TRY(check_isearch_args(who, near, far, elem, layout, N, C, H, W, sign, patch, stride, iterations, floor, out, out_mask, quant));
    const int ny = grid_count(H, patch, stride), nx = grid_count(W, patch, stride);
    const size_t px = (size_t)N * H * W, np = (size_t)N * ny * nx;
    const bool own = !patch_vecs || !patch_ssd;                         // the patch records live in the workspace
    const size_t need = px * 8 + (own ? np * 12 : 0);
    if (!workspace || workspace_bytes < need)
        return fail(OFL_E_INVALID, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace ? workspace_bytes : (size_t)0);
    OFL_TRY(check_pair_alignment(who, near, far, elem));
    if (!host_aligned(flow, 8) || !host_aligned(out, 8) || !host_aligned(workspace, 8) || !host_aligned(patch_vecs, 8) || !host_aligned(patch_ssd, 4))
        return fail(OFL_E_INVALID, "%s: flow, out, patch_vecs and the workspace must be 8-byte, patch_ssd 4-byte aligned", who);
    const size_t tb = px * C * (elem == OFL_EL_F32 ? 4 : 2);
    const void *ins[4] = { near, far, flow, fmask };
    const size_t in_bytes[4] = { tb, tb, px * 8, px };
    void *outs[5] = { workspace, out, out_mask, patch_vecs, patch_ssd };
    const size_t out_bytes[5] = { need, px * 8, px, np * 8, np * 4 };
    for (int i = 0; i < 5; ++i) {
        for (int j = 0; j < 4; ++j)
            if (overlap(outs[i], out_bytes[i], ins[j], in_bytes[j])) return fail(OFL_E_INVALID, "%s: an output or the workspace overlaps an input", who);
        for (int j = i + 1; j < 5; ++j)
            if (overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return fail(OFL_E_INVALID, "%s: the outputs and the workspace overlap", who);
    }
    IArgs a;
    pair_fill(a, near, far, layout, N, C, H, W, flow, fmask, false, sign, nullptr, nullptr);
    a.pa = static_cast<float *>(workspace);
    a.pb = a.pa + px;
    a.pv = patch_vecs ? reinterpret_cast<float2 *>(patch_vecs) : reinterpret_cast<float2 *>(a.pb + px);
    a.pssd = patch_ssd;
    a.ny = ny; a.nx = nx; a.stride = stride; a.iterations = iterations; a.normalise = normalise ? 1 : 0;
    a.floor = floor;
    a.out = out; a.out_mask = out_mask;

    hipStream_t s = stream_of(stream);
    const dim3 block(256), full((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)N);
    with_elem(elem, [&](auto E) { hipLaunchKernelGGL((isearch_setup_kernel<E.value>), full, block, 0, s, a); });
    const int per_block = patch == 8 ? 4 : 16;
    const dim3 sgrid((unsigned)((ny * nx + per_block - 1) / per_block), (unsigned)N);
    with_quant(quant, [&](auto Q) {
        if (patch == 8) hipLaunchKernelGGL((isearch_search_kernel<8, Q.value>), sgrid, block, 0, s, a);
        else            hipLaunchKernelGGL((isearch_search_kernel<4, Q.value>), sgrid, block, 0, s, a);
        hipLaunchKernelGGL((isearch_densify_kernel<Q.value>), full, block, 0, s, a, patch);
    });
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_inverse_search(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                       const float *flow, const uint8_t *fmask, int sign, int patch, int stride, int iterations,
                       int normalise, float floor, float *out, uint8_t *out_mask, float *patch_vecs, float *patch_ssd, int quant)
{
    const char *who = "ofl_inverse_search";
    OFL_TRY(need_device());
    OFL_TRY(check_isearch_args(who, near, far, elem, layout, N, C, H, W, sign, patch, stride, iterations, floor, out, out_mask, quant));
    size_t need = 0;
    OFL_TRY(ofl_inverse_search_workspace_bytes(N, H, W, patch, stride, &need));
    const size_t px = (size_t)N * H * W, np = (size_t)N * grid_count(H, patch, stride) * grid_count(W, patch, stride);
    const size_t bytes = px * C * (elem == OFL_EL_F32 ? 4 : 2);
    HostStage st(who);
    auto dn = st.in(near, bytes), df = st.in(far, bytes);
    auto dfl = st.in(flow, px * 2);
    auto dfm = st.in(fmask, px);
    auto dout = st.out(out, px * 2);
    auto dom = st.out(out_mask, px);
    auto dpv = st.out(patch_vecs, np * 2);
    auto dps = st.out(patch_ssd, np);
    auto ws = st.scratch<void>(need);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_inverse_search_dev(dn, df, elem, layout, N, C, H, W, dfl, dfm, sign, patch, stride, iterations, normalise, floor,
                                   ws, need, dout, dom, dpv, dps, quant, st.stream()));
    return st.download();
}

}  // extern "C"
