// ofl_refine.hip -- K23: variational refinement of a field on two images (gfx950).
//
// Every other kernel of the device chain scores a field or moves existing vectors around; K23 moves a vector a fraction of a
// pixel towards where the images say it belongs: the variational refinement of Brox et al. (ECCV 2004) without the
// gradient-constancy term, the last step of EpicFlow, DeepFlow, RICFlow and DIS.  ONE linearisation (one warp),
// `fixed_point` lagged-weight updates, `sor` red-black SOR sweeps per update.  The definition, with the order of every
// float32 operation, is the K23 block of include/ofl.h; tests/refine_ref.py restates it in NumPy and the device equals it
// bit for bit.  Every operation is float32 and rounded once (no FMA); sqrtf and the divisions are the correctly rounded ones.
//
// Launches, all on one stream, 1 + fixed_point * (1 + 2 * sor) + 1 of them (57 at the defaults):
//   setup    one workgroup of 256 threads per tile of 64 x 16 pixels of one item.  stage_warped_tile (ofl_photo_dev.h, K22's
//            staging) warps the tile and a halo of 1 into LDS: A, B and K21's covered.  A thread then owns 4 consecutive rows
//            of one column (K22's split) and writes gx, gy, Iz, the flags (bit 0: domain, bit 1: data) and d = 0.  The warped
//            image is never written.  6 instantiations: 3 element types x 2 quant.
//   weights  one thread per pixel: wD from the current d, and s from the central differences of U = u + du, V = v + dv.
//   sweep    one thread per pixel of ONE colour (x = 2 * lane + row parity): reads its own values and its four neighbours',
//            which are all of the other colour, and updates its d in place -- so the result does not depend on how the
//            sweep is scheduled.  The edge weights 0.5 (s + s') and sigma are formed here from s: two adds and a product per
//            edge cost less than four more planes of traffic.
//   finish   out = u + du, v + dv on the domain, the input bits elsewhere.
// Workspace, caller-provided, 29 bytes per pixel: d (float2), gx, gy, Iz, wD, s (float), flags (uint8).  No atomics, no
// LDS outside the setup, 64-bit offsets across items.  Several sweeps on one LDS tile whose halo covers them are not built.
//
// OUT OF SCOPE: the gradient-constancy term, per-channel data terms and C > 4, a loop over warps or a pyramid inside the
// call, image-driven (edge-aware) smoothness weights, a choice of omega, an energy read-back, a backward pass, mixed element
// types or layouts.
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_host_stage.h"
#include "ofl_photo_dev.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

constexpr int kBY = 4;                  // rows of a weights / sweep / finish block of 64 x 4 threads
constexpr uint8_t kDom = 1, kData = 2;  // the flag bits

struct RArgs : PairArgs {               // the setup tile kTX x kTY and a setup thread's kRows are stage_warped_tile's
    const uint8_t *valid;
    float2        *d;
    float         *gx, *gy, *iz, *wd, *s;
    uint8_t       *flags, *data;
    float         *out;
    float          alpha, delta, zeta2, eps2, omega;
};

// the four neighbours in the order of the definition: up, left, right, down
__device__ __forceinline__ int nb_dx(int k) { return k == 1 ? -1 : (k == 2 ? 1 : 0); }
__device__ __forceinline__ int nb_dy(int k) { return k == 0 ? -1 : (k == 3 ? 1 : 0); }

template <int E, int QUANT>
__global__ __launch_bounds__(256)
void refine_setup_kernel(const RArgs a)
{
    constexpr int R = 1, TW = kTX + 2 * R, TH = kTY + 2 * R, NE = TW * TH;
    __shared__ float   s_a[NE], s_b[NE];
    __shared__ uint8_t s_m[NE];

    const int H = a.H, W = a.W;
    const int n = blockIdx.z, x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
    const size_t hw = (size_t)H * W;

    stage_warped_tile<E, QUANT, R, kTX, kTY>(a, n, x0, y0, s_a, s_b, s_m);
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = x0 + lane;
    if (x >= W) return;
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int ty = kRows * wave + j, y = y0 + ty;
        if (y >= H) break;
        const int at = (ty + R) * TW + lane + R;
        const size_t p = (size_t)n * hw + (size_t)y * W + x;
        const float2 f = *reinterpret_cast<const float2 *>(a.flow + 2 * p);
        const bool dom = a.fmask[p] != 0 && (a.valid ? a.valid[p] != 0 : true) && finite32(f.x) && finite32(f.y);
        const bool up = y > 0, left = x > 0, right = x + 1 < W, down = y + 1 < H;     // the neighbour is inside the frame
        const float Bc = s_b[at];
        const float Bx = __fmul_rn(0.5f, __fsub_rn(right ? s_b[at + 1] : Bc, left ? s_b[at - 1] : Bc));
        const float By = __fmul_rn(0.5f, __fsub_rn(down ? s_b[at + TW] : Bc, up ? s_b[at - TW] : Bc));
        const float gx = a.sign >= 0 ? Bx : -Bx, gy = a.sign >= 0 ? By : -By;
        const float iz = __fsub_rn(Bc, s_a[at]);
        const bool data = dom && s_m[at] != 0 && (!up || s_m[at - TW] != 0) && (!left || s_m[at - 1] != 0) &&
                          (!right || s_m[at + 1] != 0) && (!down || s_m[at + TW] != 0) &&
                          finite32(gx) && finite32(gy) && finite32(iz);
        a.gx[p] = gx;
        a.gy[p] = gy;
        a.iz[p] = iz;
        a.d[p] = make_float2(0.0f, 0.0f);
        a.flags[p] = (dom ? kDom : 0) | (data ? kData : 0);
        if (a.data) a.data[p] = data ? 1 : 0;
    }
}

// one fixed-point iteration's lagged weights from the current d: wD (data term) and s (smoothness) of every domain pixel
__global__ __launch_bounds__(256)
void refine_weights_kernel(const RArgs a)
{
    const int H = a.H, W = a.W;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)blockIdx.z * H * W + (size_t)y * W + x;
    const uint8_t fl = a.flags[p];
    if (!(fl & kDom)) return;
    const float2 *flow = reinterpret_cast<const float2 *>(a.flow);
    const float2 f = flow[p], d = a.d[p];
    const float gx = a.gx[p], gy = a.gy[p], iz = a.iz[p];

    const float r = __fadd_rn(__fadd_rn(iz, __fmul_rn(gx, d.x)), __fmul_rn(gy, d.y));
    const float nn = __fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), a.zeta2);
    const float t = __fdiv_rn(__fmul_rn(r, r), nn);
    const float wd = __fdiv_rn(a.delta, __fmul_rn(nn, sqrtf(__fadd_rn(t, a.eps2))));
    a.wd[p] = (fl & kData) ? wd : 0.0f;

    const float Uc = __fadd_rn(f.x, d.x), Vc = __fadd_rn(f.y, d.y);
    float U[4], V[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = x + nb_dx(k), yy = y + nb_dy(k);
        const bool in = (unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H;
        const size_t q = in ? p + (ptrdiff_t)nb_dy(k) * W + nb_dx(k) : p;
        const bool nb = in && (a.flags[q] & kDom);
        const float2 fq = flow[q], dq = a.d[q];
        U[k] = nb ? __fadd_rn(fq.x, dq.x) : Uc;
        V[k] = nb ? __fadd_rn(fq.y, dq.y) : Vc;
    }
    const float Ux = __fmul_rn(0.5f, __fsub_rn(U[2], U[1])), Uy = __fmul_rn(0.5f, __fsub_rn(U[3], U[0]));
    const float Vx = __fmul_rn(0.5f, __fsub_rn(V[2], V[1])), Vy = __fmul_rn(0.5f, __fsub_rn(V[3], V[0]));
    float g = __fadd_rn(__fmul_rn(Ux, Ux), __fmul_rn(Uy, Uy));
    g = __fadd_rn(g, __fmul_rn(Vx, Vx));
    g = __fadd_rn(g, __fmul_rn(Vy, Vy));
    g = __fadd_rn(g, a.eps2);
    a.s[p] = __fdiv_rn(a.alpha, sqrtf(g));
}

// one half-sweep: the domain pixels of `colour` = (x + y) & 1, each from its own values and the other colour's
__global__ __launch_bounds__(256)
void refine_sweep_kernel(const RArgs a, int colour)
{
    const int H = a.H, W = a.W;
    const int y = blockIdx.y * kBY + threadIdx.y;
    const int x = 2 * (blockIdx.x * 64 + threadIdx.x) + ((y + colour) & 1);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)blockIdx.z * H * W + (size_t)y * W + x;
    if (!(a.flags[p] & kDom)) return;
    const float2 *flow = reinterpret_cast<const float2 *>(a.flow);
    const float2 f = flow[p], d = a.d[p];
    const float gx = a.gx[p], gy = a.gy[p], iz = a.iz[p], wd = a.wd[p], sc = a.s[p];

    float sigma = 0.0f, tu[4], tv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = x + nb_dx(k), yy = y + nb_dy(k);
        const bool in = (unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H;
        const size_t q = in ? p + (ptrdiff_t)nb_dy(k) * W + nb_dx(k) : p;
        const bool nb = in && (a.flags[q] & kDom);
        const float2 fq = flow[q], dq = a.d[q];
        const float w = nb ? __fmul_rn(0.5f, __fadd_rn(sc, a.s[q])) : 0.0f;
        sigma = __fadd_rn(sigma, w);
        tu[k] = nb ? __fmul_rn(w, __fsub_rn(__fadd_rn(fq.x, dq.x), f.x)) : 0.0f;
        tv[k] = nb ? __fmul_rn(w, __fsub_rn(__fadd_rn(fq.y, dq.y), f.y)) : 0.0f;
    }
    const float pg = __fmul_rn(wd, gx), qg = __fmul_rn(wd, gy);
    const float a11 = __fmul_rn(pg, gx), a12 = __fmul_rn(pg, gy), a22 = __fmul_rn(qg, gy);
    const float b1 = -__fmul_rn(pg, iz), b2 = -__fmul_rn(qg, iz);

    float num = __fsub_rn(b1, __fmul_rn(a12, d.y));
#pragma unroll
    for (int k = 0; k < 4; ++k) num = __fadd_rn(num, tu[k]);
    const float den_u = __fadd_rn(a11, sigma);
    const float du_s = __fdiv_rn(num, den_u);
    const float du_n = __fadd_rn(d.x, __fmul_rn(a.omega, __fsub_rn(du_s, d.x)));
    const bool ok_u = den_u != 0.0f && finite32(du_n);

    num = __fsub_rn(b2, __fmul_rn(a12, ok_u ? du_s : d.x));
#pragma unroll
    for (int k = 0; k < 4; ++k) num = __fadd_rn(num, tv[k]);
    const float den_v = __fadd_rn(a22, sigma);
    const float dv_s = __fdiv_rn(num, den_v);
    const float dv_n = __fadd_rn(d.y, __fmul_rn(a.omega, __fsub_rn(dv_s, d.y)));
    const bool ok_v = den_v != 0.0f && finite32(dv_n);

    a.d[p] = make_float2(ok_u ? du_n : d.x, ok_v ? dv_n : d.y);
}

__global__ __launch_bounds__(256)
void refine_finish_kernel(const RArgs a)
{
    const int H = a.H, W = a.W;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)blockIdx.z * H * W + (size_t)y * W + x;
    float2 f = reinterpret_cast<const float2 *>(a.flow)[p];
    if (a.flags[p] & kDom) {
        const float2 d = a.d[p];
        if (d.x != 0.0f) f.x = __fadd_rn(f.x, d.x);             // d = 0 keeps the bits, the sign of a zero included
        if (d.y != 0.0f) f.y = __fadd_rn(f.y, d.y);
    }
    reinterpret_cast<float2 *>(a.out)[p] = f;
}

int check_refine_args(const char *who, const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                      const void *flow, const void *fmask, int sign, float alpha, float delta, float zeta, float eps,
                      int fixed_point, int sor, float omega, const void *out, int quant)
{
    if (!near || !far || !flow || !fmask || !out) return fail(OFL_E_INVALID, "%s: NULL pointer (near, far, flow, fmask and out are required)", who);
    OFL_TRY(check_pair_args(who, elem, layout, N, C, OFL_REFINE_MAX_C, H, W, sign, quant));
    if (!finite_not_negative(alpha)) return fail(OFL_E_INVALID, "%s: alpha must be finite and not negative (got %g)", who, (double)alpha);
    if (!finite_not_negative(delta)) return fail(OFL_E_INVALID, "%s: delta must be finite and not negative (got %g)", who, (double)delta);
    if (!finite_positive(zeta)) return fail(OFL_E_INVALID, "%s: zeta must be finite and positive (got %g)", who, (double)zeta);
    if (!finite_positive(eps)) return fail(OFL_E_INVALID, "%s: eps must be finite and positive (got %g)", who, (double)eps);
    if (!finite_positive(zeta * zeta) || !finite_positive(eps * eps))
        return fail(OFL_E_INVALID, "%s: zeta^2 and eps^2 must be finite and positive in float32", who);
    if (fixed_point < 1 || fixed_point > OFL_REFINE_MAX_ITER) return fail(OFL_E_INVALID, "%s: fixed_point must be in [1, %d], got %d", who, OFL_REFINE_MAX_ITER, fixed_point);
    if (sor < 1 || sor > OFL_REFINE_MAX_ITER) return fail(OFL_E_INVALID, "%s: sor must be in [1, %d], got %d", who, OFL_REFINE_MAX_ITER, sor);
    if (!(omega > 0.0f && omega < 2.0f)) return fail(OFL_E_INVALID, "%s: omega must lie in (0, 2) (got %g)", who, (double)omega);
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_refine_workspace_bytes(int N, int H, int W, size_t *bytes)
{
    if (!bytes) return fail(OFL_E_INVALID, "ofl_refine_workspace_bytes: NULL pointer");
    if (N < 1 || N > 65535) return fail(OFL_E_INVALID, "ofl_refine_workspace_bytes: N must be in [1, 65535], got %d", N);
    OFL_TRY(check_field_dims("ofl_refine_workspace_bytes", H, W));
    *bytes = (size_t)N * H * W * 29;
    return OFL_OK;
}

int ofl_refine_dev(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
                   const float *flow, const uint8_t *fmask, int sign,
                   const uint8_t *near_mask, const uint8_t *far_mask, const uint8_t *valid,
                   float alpha, float delta, float zeta, float eps, int fixed_point, int sor, float omega,
                   void *workspace, size_t workspace_bytes, float *out, uint8_t *data, int quant, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_refine_args("ofl_refine", near, far, elem, layout, N, C, H, W, flow, fmask, sign, alpha, delta, zeta, eps,
                              fixed_point, sor, omega, out, quant));
    size_t need = 0;
    OFL_TRY(ofl_refine_workspace_bytes(N, H, W, &need));
    if (!workspace || workspace_bytes < need)
        return fail(OFL_E_INVALID, "ofl_refine: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    OFL_TRY(check_pair_alignment("ofl_refine", near, far, elem));
    if (!host_aligned(flow, 8) || !host_aligned(out, 8) || !host_aligned(workspace, 8))
        return fail(OFL_E_INVALID, "ofl_refine: flow, out and the workspace must be 8-byte aligned");
    const size_t px = (size_t)N * H * W, tb = px * C * (elem == OFL_EL_F32 ? 4 : 2);
    if (overlap(out, px * 8, flow, px * 8) || overlap(out, px * 8, near, tb) || overlap(out, px * 8, far, tb) ||
        overlap(out, px * 8, fmask, px) || overlap(out, px * 8, near_mask, px) || overlap(out, px * 8, far_mask, px) ||
        overlap(out, px * 8, valid, px) || overlap(out, px * 8, data, px))
        return fail(OFL_E_INVALID, "ofl_refine: out overlaps another argument");
    if (overlap(workspace, need, out, px * 8) || overlap(workspace, need, flow, px * 8) || overlap(workspace, need, near, tb) ||
        overlap(workspace, need, far, tb) || overlap(workspace, need, fmask, px) || overlap(workspace, need, near_mask, px) ||
        overlap(workspace, need, far_mask, px) || overlap(workspace, need, valid, px) || overlap(workspace, need, data, px))
        return fail(OFL_E_INVALID, "ofl_refine: the workspace overlaps an argument");
    RArgs a;
    pair_fill(a, near, far, layout, N, C, H, W, flow, fmask, false, sign, near_mask, far_mask);
    a.valid = valid;
    a.d = static_cast<float2 *>(workspace);
    a.gx = reinterpret_cast<float *>(a.d + px);
    a.gy = a.gx + px; a.iz = a.gy + px; a.wd = a.iz + px; a.s = a.wd + px;
    a.flags = reinterpret_cast<uint8_t *>(a.s + px);
    a.data = data; a.out = out;
    a.alpha = alpha; a.delta = delta; a.zeta2 = zeta * zeta; a.eps2 = eps * eps; a.omega = omega;

    hipStream_t s = stream_of(stream);
    const dim3 tiles = window_grid(N, H, W);
    with_elem(elem, [&](auto E) { with_quant(quant, [&](auto Q) {
        hipLaunchKernelGGL((refine_setup_kernel<E.value, Q.value>), tiles, dim3(256), 0, s, a);
    }); });
    const dim3 block(64, kBY);
    const dim3 full((unsigned)((W + 63) / 64), (unsigned)((H + kBY - 1) / kBY), (unsigned)N);
    const dim3 half((unsigned)((W + 127) / 128), (unsigned)((H + kBY - 1) / kBY), (unsigned)N);
    for (int i = 0; i < fixed_point; ++i) {
        hipLaunchKernelGGL(refine_weights_kernel, full, block, 0, s, a);
        for (int j = 0; j < sor; ++j) {
            hipLaunchKernelGGL(refine_sweep_kernel, half, block, 0, s, a, 0);
            hipLaunchKernelGGL(refine_sweep_kernel, half, block, 0, s, a, 1);
        }
    }
    hipLaunchKernelGGL(refine_finish_kernel, full, block, 0, s, a);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_refine(const void *near, const void *far, int elem, int layout, int N, int C, int H, int W,
               const float *flow, const uint8_t *fmask, int sign,
               const uint8_t *near_mask, const uint8_t *far_mask, const uint8_t *valid,
               float alpha, float delta, float zeta, float eps, int fixed_point, int sor, float omega,
               float *out, uint8_t *data, int quant)
{
    OFL_TRY(need_device());
    OFL_TRY(check_refine_args("ofl_refine", near, far, elem, layout, N, C, H, W, flow, fmask, sign, alpha, delta, zeta, eps,
                              fixed_point, sor, omega, out, quant));
    size_t need = 0;
    OFL_TRY(ofl_refine_workspace_bytes(N, H, W, &need));
    const size_t px = (size_t)N * H * W;
    const size_t bytes = px * C * (elem == OFL_EL_F32 ? 4 : 2);
    HostStage st("ofl_refine");
    auto dn = st.in(near, bytes), df = st.in(far, bytes);
    auto dfl = st.in(flow, px * 2);
    auto dfm = st.in(fmask, px), dnm = st.in(near_mask, px), dam = st.in(far_mask, px), dv = st.in(valid, px);
    auto dout = st.out(out, px * 2);
    auto dd = st.out(data, px);
    auto ws = st.scratch<void>(need);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_refine_dev(dn, df, elem, layout, N, C, H, W, dfl, dfm, sign, dnm, dam, dv, alpha, delta, zeta, eps, fixed_point, sor,
                           omega, ws, need, dout, dd, quant, st.stream()));
    return st.download();
}

}  // extern "C"
