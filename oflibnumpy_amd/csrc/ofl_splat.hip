// ofl_splat.hip -- K20: forward warp of tensors and fields by bilinear splatting (gfx950); the definition is in include/ofl.h.
// Every source pixel adds its four bilinear taps, times an importance factor, to int64 fixed-point accumulators of the
// target pixels; a final pass turns the sums into the output.  Integer atomic adds and integer atomic maxima commute, so the
// result is a function of the inputs alone -- tests/splat_ref.py restates it with np.add.at on int64 and the device result
// is compared byte for byte.  Every float operation is float32 and rounded once, in the order stated in the header.
//
//   max_kernel         softmax only: zmax[field][target] = max of zs over the taps that exist there, an atomic max on the
//                      order-preserving int32 key of the float (the plane starts at the smallest key).
//   accum_kernel       a group of 2^sh lanes per (item, source pixel) -- sh = 0 in the planar layout, where consecutive lanes
//                      read consecutive pixels of one channel plane, and 2^sh = the power of two that holds C + 1, 64 at
//                      most, in channels-last, where consecutive lanes read consecutive channels of one pixel.  Every lane of
//                      a group forms the same taps; lane j takes the channels j, j + 2^sh, ... and the weight plane counts as
//                      channel C.  Accumulators are channels-last [N][H][W][C + 1], so the adds of one tap are adjacent.  An
//                      add of the integer 0 is left out (it changes nothing).
//   finish_kernel      one lane per output element in the output's memory order, plus one per pixel for weight and valid.
// No loop depends on the data: a field that contracts everything into one pixel costs contention, not iterations.  Offsets are
// 64-bit.  Taps of neighbouring lanes that hit one target are NOT combined before the atomic.
#include <stddef.h>
#include "ofl_common.h"
#include "ofl_elem.h"
#include "ofl_exp32.h"
#include "ofl_host_stage.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

constexpr int    kThreads  = 256;
constexpr float  kCoordMax = 1073741824.0f;             // 2^30
constexpr double kValMax   = 4611686018427387904.0;     // 2^62
constexpr double kTwo32    = 4294967296.0;
constexpr size_t kMaxLanes = (size_t)1 << 38;           // lanes of one launch: 2^30 blocks

struct SArgs {
    const void    *src;
    const float2  *flow;
    const uint8_t *fmask;
    const float   *z;
    int64_t       *acc;
    int32_t       *zmax;
    void          *dst;
    uint8_t       *valid;
    float         *weight;
    uint32_t      *counters;
    double         val_scale, out_scale;      // 2^frac_bits; 2^-frac_bits (SUM) or 2^(32 - frac_bits)
    int64_t        min_d;                     // the integer nearest to min_weight * 2^32
    float          alpha;
    int            n, c, h, w, shared, mode, sh;
};

// order-preserving int32 key of a float that is not NaN, and its inverse (the same map)
__device__ __forceinline__ int32_t float_key(float f)
{
    const int32_t b = (int32_t)__float_as_uint(f);
    return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float key_float(int32_t k) { return __uint_as_float((uint32_t)(k ^ ((k >> 31) & 0x7fffffff))); }

struct Landing {
    int   ix, iy;          // the top-left tap
    float w[4];            // (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy
    float zs;              // alpha * z (softmax), else unused
    bool  ok;
};

// steps 1 and 2 of the definition for the source pixel (x, y) of field plane `fp` (pixel offset of the field)
template <bool SOFTMAX>
__device__ __forceinline__ Landing landing(const SArgs &a, size_t fq, int x, int y)
{
    Landing l;
    l.ok = false; l.ix = l.iy = 0; l.zs = 0.0f;
    l.w[0] = l.w[1] = l.w[2] = l.w[3] = 0.0f;
    if (a.fmask[fq] == 0) return l;
    const float2 f = a.flow[fq];
    if (!__builtin_isfinite(f.x) || !__builtin_isfinite(f.y)) return l;
    const float px = __fadd_rn((float)x, f.x), py = __fadd_rn((float)y, f.y);
    if (!(fabsf(px) < kCoordMax) || !(fabsf(py) < kCoordMax)) return l;
    if (SOFTMAX) {
        l.zs = __fmul_rn(a.alpha, a.z[fq]);
        if (!__builtin_isfinite(l.zs)) return l;
    }
    const float x0 = floorf(px), y0 = floorf(py);
    const float fx = __fsub_rn(px, x0), fy = __fsub_rn(py, y0);
    const float gx = __fsub_rn(1.0f, fx), gy = __fsub_rn(1.0f, fy);
    l.w[0] = __fmul_rn(gx, gy); l.w[1] = __fmul_rn(fx, gy);
    l.w[2] = __fmul_rn(gx, fy); l.w[3] = __fmul_rn(fx, fy);
    l.ix = (int)x0; l.iy = (int)y0;
    l.ok = true;
    return l;
}

// tap k of a landing exists: its weight is not 0 and its pixel lies inside the frame
__device__ __forceinline__ bool tap_exists(const Landing &l, int k, int h, int w, int &tx, int &ty)
{
    tx = l.ix + (k & 1); ty = l.iy + (k >> 1);
    return l.w[k] != 0.0f && tx >= 0 && tx < w && ty >= 0 && ty < h;
}

__global__ __launch_bounds__(kThreads)
void max_kernel(const SArgs a)
{
    const size_t hw = (size_t)a.h * a.w, p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= hw) return;
    const size_t plane = (size_t)blockIdx.y * hw;
    const int y = (int)(p / a.w), x = (int)(p - (size_t)y * a.w);
    const Landing l = landing<true>(a, plane + p, x, y);
    if (!l.ok) return;
    const int32_t key = float_key(l.zs);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int tx, ty;
        if (tap_exists(l, k, a.h, a.w, tx, ty)) atomicMax(a.zmax + plane + (size_t)ty * a.w + tx, key);
    }
}

__device__ __forceinline__ void add64(int64_t *p, int64_t v)
{
    if (v != 0) atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

template <int E, int LAYOUT, bool SOFTMAX>
__global__ __launch_bounds__(kThreads)
void accum_kernel(const SArgs a)
{
    typedef typename Elem<E>::T T;
    const size_t hw = (size_t)a.h * a.w, t = (size_t)blockIdx.x * kThreads + threadIdx.x, p = t >> a.sh;
    if (p >= hw) return;
    const int sub = (int)(t & (((size_t)1 << a.sh) - 1)), step = 1 << a.sh, C = a.c;
    const size_t n = blockIdx.y, fplane = a.shared ? 0 : n * hw;
    const int y = (int)(p / a.w), x = (int)(p - (size_t)y * a.w);
    const Landing l = landing<SOFTMAX>(a, fplane + p, x, y);
    if (!l.ok) {
        if (sub == 0 && (n == 0 || !a.shared) && a.counters) atomicAdd(a.counters, 1u);
        return;
    }
    float    we[4];
    int64_t *tgt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int tx, ty;
        tgt[k] = nullptr;
        we[k]  = 0.0f;
        if (tap_exists(l, k, a.h, a.w, tx, ty)) {
            const size_t q = (size_t)ty * a.w + tx;
            float e = 1.0f;
            if (SOFTMAX) {
                const float d = __fsub_rn(l.zs, key_float(a.zmax[fplane + q]));
                e = d < -87.0f ? 0.0f : exp32(d);
            }
            we[k]  = __fmul_rn(l.w[k], e);
            tgt[k] = a.acc + (n * hw + q) * (size_t)(C + 1);
        }
    }
    const T *src = static_cast<const T *>(a.src);
#pragma unroll 1
    for (int c = sub; c <= C; c += step) {
        if (c == C) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (tgt[k]) add64(tgt[k] + C, __double2ll_rn((double)we[k] * kTwo32));
            break;
        }
        const size_t si = LAYOUT == OFL_TENSOR_NCHW ? (n * C + c) * hw + p : (n * hw + p) * C + c;
        const float v = Elem<E>::to_f32(src[si]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!tgt[k]) continue;
            const double d = (double)__fmul_rn(we[k], v) * a.val_scale;
            if (!(fabs(d) < kValMax)) {                        // NaN, or beyond what an accumulator is given
                if (a.counters) atomicAdd(a.counters + 1, 1u);
                continue;
            }
            add64(tgt[k] + c, __double2ll_rn(d));
        }
    }
}

template <int E, int LAYOUT>
__global__ __launch_bounds__(kThreads)
void finish_kernel(const SArgs a)
{
    typedef typename Elem<E>::T T;
    const size_t hw = (size_t)a.h * a.w, C1 = (size_t)a.c + 1;
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= hw * C1) return;
    const size_t n = blockIdx.y;
    size_t p, c;
    if (LAYOUT == OFL_TENSOR_NCHW) { c = t / hw; p = t - c * hw; }
    else                           { p = t / C1; c = t - p * C1; }
    const int64_t *acc = a.acc + (n * hw + p) * C1;
    const int64_t D = acc[a.c];
    const bool ok = D >= a.min_d;
    if (c == (size_t)a.c) {
        if (n == 0 || !a.shared) {
            const size_t q = (a.shared ? 0 : n * hw) + p;
            if (a.valid)  a.valid[q]  = ok ? 1 : 0;
            if (a.weight) a.weight[q] = (float)((double)D * (1.0 / kTwo32));
        }
        return;
    }
    const double A = (double)acc[c];
    float o;
    if (a.mode == OFL_SPLAT_SUM) o = (float)(A * a.out_scale);
    else                         o = ok ? (float)((A / (double)D) * a.out_scale) : 0.0f;
    const size_t di = LAYOUT == OFL_TENSOR_NCHW ? (n * a.c + c) * hw + p : (n * hw + p) * a.c + c;
    static_cast<T *>(a.dst)[di] = Elem<E>::from_f32(o);
}

template <int E, int LAYOUT>
void launch(const SArgs &a, hipStream_t s)
{
    const size_t hw = (size_t)a.h * a.w;
    const dim3 ga((unsigned)(((hw << a.sh) + kThreads - 1) / kThreads), (unsigned)a.n);
    if (a.mode == OFL_SPLAT_SOFTMAX) {
        const dim3 gm((unsigned)((hw + kThreads - 1) / kThreads), (unsigned)(a.shared ? 1 : a.n));
        hipLaunchKernelGGL(max_kernel, gm, dim3(kThreads), 0, s, a);
        hipLaunchKernelGGL((accum_kernel<E, LAYOUT, true>), ga, dim3(kThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL((accum_kernel<E, LAYOUT, false>), ga, dim3(kThreads), 0, s, a);
    }
    const dim3 gf((unsigned)((hw * ((size_t)a.c + 1) + kThreads - 1) / kThreads), (unsigned)a.n);
    hipLaunchKernelGGL((finish_kernel<E, LAYOUT>), gf, dim3(kThreads), 0, s, a);
}

template <int E>
void launch_layout(const SArgs &a, int layout, hipStream_t s)
{
    if (layout == OFL_TENSOR_NCHW) launch<E, OFL_TENSOR_NCHW>(a, s);
    else                           launch<E, OFL_TENSOR_NHWC>(a, s);
}

size_t elem_bytes(int elem) { return elem == OFL_EL_F32 ? 4 : 2; }

size_t acc_bytes(int N, int C, int H, int W) { return (size_t)N * ((size_t)C + 1) * H * W * 8; }
size_t zmax_count(int N, int H, int W, int shared) { return (size_t)(shared ? 1 : N) * H * W; }

int check_sizes(const char *who, int N, int C, int H, int W, int mode)
{
    OFL_TRY(check_field_dims(who, H, W));
    if (N < 1 || N > 65535 || C < 0 || C > 65535)
        return fail(OFL_E_INVALID, "%s: N in [1, 65535] and C in [0, 65535] (got %d and %d)", who, N, C);
    if (mode != OFL_SPLAT_SUM && mode != OFL_SPLAT_AVERAGE && mode != OFL_SPLAT_SOFTMAX)
        return fail(OFL_E_INVALID, "%s: mode must be OFL_SPLAT_SUM, OFL_SPLAT_AVERAGE or OFL_SPLAT_SOFTMAX (got %d)", who, mode);
    if ((size_t)H * W * ((size_t)C + 1) > kMaxLanes || ((size_t)H * W << 6) > kMaxLanes)
        return fail(OFL_E_INVALID, "%s: %d x %d pixels of %d channels are more than one launch addresses", who, H, W, C);
    return OFL_OK;
}

int check_splat_args(const char *who, const void *src, int elem, int layout, int N, int C, int H, int W, const float *flow,
                     const uint8_t *fmask, int flow_shared, const float *z, float alpha, int mode, int frac_bits, float min_weight,
                     const void *dst, const uint8_t *valid, const float *weight)
{
    OFL_TRY(check_sizes(who, N, C, H, W, mode));
    if (!flow || !fmask) return fail(OFL_E_INVALID, "%s: NULL pointer (flow and fmask are required)", who);
    if (C > 0 && (!src || !dst)) return fail(OFL_E_INVALID, "%s: NULL pointer (src and dst are required when C > 0)", who);
    if (C == 0 && !valid && !weight) return fail(OFL_E_INVALID, "%s: C = 0 needs valid or weight", who);
    if (elem != OFL_EL_F16 && elem != OFL_EL_BF16 && elem != OFL_EL_F32)
        return fail(OFL_E_INVALID, "%s: elem must be OFL_EL_F16, OFL_EL_BF16 or OFL_EL_F32 (got %d)", who, elem);
    if (layout != OFL_TENSOR_NCHW && layout != OFL_TENSOR_NHWC) return fail(OFL_E_INVALID, "%s: bad layout %d", who, layout);
    if (mode == OFL_SPLAT_SOFTMAX && !z) return fail(OFL_E_INVALID, "%s: OFL_SPLAT_SOFTMAX needs the importance z", who);
    if (mode == OFL_SPLAT_SOFTMAX && !__builtin_isfinite(alpha)) return fail(OFL_E_INVALID, "%s: alpha must be finite", who);
    if (frac_bits < 0 || frac_bits > 40) return fail(OFL_E_INVALID, "%s: frac_bits must be in [0, 40] (got %d)", who, frac_bits);
    if (!(min_weight >= 0x1p-20f && min_weight <= 1.0f))
        return fail(OFL_E_INVALID, "%s: min_weight must be in [2^-20, 1] (got %g)", who, (double)min_weight);
    const size_t hw = (size_t)H * W, fields = flow_shared ? 1 : (size_t)N, tb = (size_t)N * C * hw * elem_bytes(elem);
    const void *outs[3] = { C ? dst : nullptr, valid, weight };
    const size_t out_bytes[3] = { tb, fields * hw, fields * hw * 4 };
    const void *ins[4] = { C ? src : nullptr, flow, fmask, mode == OFL_SPLAT_SOFTMAX ? z : nullptr };
    const size_t in_bytes[4] = { tb, fields * hw * 8, fields * hw, fields * hw * 4 };
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 4; ++i)
            if (overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return fail(OFL_E_INVALID, "%s: outputs must not overlap inputs", who);
        for (int i = 0; i < o; ++i)
            if (overlap(outs[o], out_bytes[o], outs[i], out_bytes[i])) return fail(OFL_E_INVALID, "%s: outputs overlap each other", who);
    }
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_splat_workspace_bytes(int N, int C, int H, int W, int flow_shared, int mode, size_t *bytes)
{
    if (!bytes) return fail(OFL_E_INVALID, "ofl_splat_workspace_bytes: NULL pointer");
    OFL_TRY(check_sizes("ofl_splat_workspace_bytes", N, C, H, W, mode));
    *bytes = acc_bytes(N, C, H, W) + (mode == OFL_SPLAT_SOFTMAX ? 4 * zmax_count(N, H, W, flow_shared) : 0);
    return OFL_OK;
}

int ofl_splat_dev(const void *src, int elem, int layout, int N, int C, int H, int W,
                  const float *flow, const uint8_t *fmask, int flow_shared, const float *z, float alpha,
                  int mode, int frac_bits, float min_weight, void *workspace, size_t workspace_bytes,
                  void *dst, uint8_t *valid, float *weight, uint32_t *counters, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_splat_args("ofl_splat", src, elem, layout, N, C, H, W, flow, fmask, flow_shared, z, alpha, mode, frac_bits,
                             min_weight, dst, valid, weight));
    size_t need = 0;
    OFL_TRY(ofl_splat_workspace_bytes(N, C, H, W, flow_shared, mode, &need));
    if (!workspace || workspace_bytes < need)
        return fail(OFL_E_INVALID, "ofl_splat: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    if (!host_aligned(workspace, 8) || !host_aligned(flow, 8))
        return fail(OFL_E_INVALID, "ofl_splat: workspace and flow must be 8-byte aligned");
    if (!host_aligned(src, (unsigned)elem_bytes(elem)) || !host_aligned(dst, (unsigned)elem_bytes(elem)))
        return fail(OFL_E_INVALID, "ofl_splat: src and dst must be aligned to the element size");
    if (!host_aligned(z, 4) || !host_aligned(weight, 4) || !host_aligned(counters, 4))
        return fail(OFL_E_INVALID, "ofl_splat: z, weight and counters must be 4-byte aligned");
    const size_t fpx = (size_t)(flow_shared ? 1 : N) * H * W, tb = (size_t)N * C * H * W * elem_bytes(elem);
    if (overlap(workspace, need, dst, tb) || overlap(workspace, need, src, tb) || overlap(workspace, need, flow, fpx * 8) ||
        overlap(workspace, need, fmask, fpx) || overlap(workspace, need, z, fpx * 4) || overlap(workspace, need, valid, fpx) ||
        overlap(workspace, need, weight, fpx * 4) || overlap(workspace, need, counters, 8))
        return fail(OFL_E_INVALID, "ofl_splat: the workspace overlaps an argument");

    SArgs a;
    a.src = src; a.flow = reinterpret_cast<const float2 *>(flow); a.fmask = fmask; a.z = z;
    a.acc = static_cast<int64_t *>(workspace);
    a.zmax = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + acc_bytes(N, C, H, W));
    a.dst = dst; a.valid = valid; a.weight = weight; a.counters = counters;
    a.val_scale = __builtin_ldexp(1.0, frac_bits);
    a.out_scale = __builtin_ldexp(1.0, mode == OFL_SPLAT_SUM ? -frac_bits : 32 - frac_bits);
    a.min_d = (int64_t)__builtin_rint((double)min_weight * kTwo32);
    a.alpha = alpha; a.n = N; a.c = C; a.h = H; a.w = W; a.shared = flow_shared ? 1 : 0; a.mode = mode;
    a.sh = 0;
    if (layout == OFL_TENSOR_NHWC) while ((1 << a.sh) < C + 1 && a.sh < 6) ++a.sh;

    hipStream_t s = stream_of(stream);
    OFL_HIP(hipMemsetAsync(workspace, 0, acc_bytes(N, C, H, W), s));
    if (mode == OFL_SPLAT_SOFTMAX) OFL_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.zmax), (int)0x80000000u, zmax_count(N, H, W, flow_shared), s));
    if (elem == OFL_EL_F16)       launch_layout<OFL_EL_F16>(a, layout, s);
    else if (elem == OFL_EL_BF16) launch_layout<OFL_EL_BF16>(a, layout, s);
    else                          launch_layout<OFL_EL_F32>(a, layout, s);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_splat(const void *src, int elem, int layout, int N, int C, int H, int W,
              const float *flow, const uint8_t *fmask, int flow_shared, const float *z, float alpha,
              int mode, int frac_bits, float min_weight, void *dst, uint8_t *valid, float *weight, uint32_t *counters_host)
{
    OFL_TRY(need_device());
    OFL_TRY(check_splat_args("ofl_splat", src, elem, layout, N, C, H, W, flow, fmask, flow_shared, z, alpha, mode, frac_bits,
                             min_weight, dst, valid, weight));
    size_t need = 0;
    OFL_TRY(ofl_splat_workspace_bytes(N, C, H, W, flow_shared, mode, &need));
    const size_t hw = (size_t)H * W, fields = flow_shared ? 1 : (size_t)N, tb = (size_t)N * C * hw * elem_bytes(elem);
    HostStage st("ofl_splat");
    auto ds = st.in(C ? src : nullptr, tb);
    auto df = st.in(flow, fields * hw * 2);
    auto dm = st.in(fmask, fields * hw);
    auto dz = st.in(mode == OFL_SPLAT_SOFTMAX ? z : nullptr, fields * hw);
    auto od = st.out(C ? dst : nullptr, tb);
    auto ov = st.out(valid, fields * hw);
    auto ow = st.out(weight, fields * hw);
    auto oc = st.out(counters_host, 2, true);
    auto ws = st.scratch<void>(need);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_splat_dev(ds, elem, layout, N, C, H, W, df, dm, flow_shared, dz, alpha, mode, frac_bits, min_weight,
                          ws, need, od, ov, ow, oc, st.stream()));
    return st.download();
}

}  // extern "C"
