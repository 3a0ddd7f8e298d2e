// ofl_visualise.hip -- K7: flow fields rendered as HSV / RGB / BGR colour images (Flow.visualise, flow_class.py:869-951).
// Two kernel families, every launch serving a whole batch of fields of one shape:
//   range select  exact order statistics lo / hi of the thresholded magnitudes (the two values np.percentile(mag, 99)
//                 interpolates between) and their maximum, per field: a three-pass radix select over the float bits
//                 (magnitudes are >= 0, so their bits sort as uint32) with LDS histograms merged by integer atomics;
//                 then NumPy's lerp and the reference's fallbacks on the device.  No host synchronisation.
//   render        threshold -> magnitude, angle -> H, S, V -> mask dimming / mask border -> uint8 bytes.
#include "ofl_common.h"
#include <algorithm>

#pragma clang fp contract(off)

using namespace ofl;

namespace {

// ----------------------------------------------------------------------------- per-pixel arithmetic
// Magnitude and angle restate cv2.cartToPolar(u, v, angleInDegrees=True) (OpenCV 4.x magnitude / fastAtan2) in float32,
// one rounding per operation.
constexpr float kRadToDeg = (float)(180.0 / 3.141592653589793);
constexpr float kP1 = 0.9997878412794807f * kRadToDeg;
constexpr float kP3 = -0.3258083974640975f * kRadToDeg;
constexpr float kP5 = 0.1555786518463281f * kRadToDeg;
constexpr float kP7 = -0.04432655554792128f * kRadToDeg;
constexpr float kDblEps = (float)2.220446049250313080847e-16;      // (float)DBL_EPSILON

// threshold_vectors (utils.py:310-315): a component with -th < c < th becomes +0
__device__ __forceinline__ float vis_th(float c, float th) { return (c < th && c > -th) ? 0.0f : c; }

// sqrtf, not __fsqrt_rn: the latter is the 1-ulp v_sqrt_f32 in this toolchain (no OCML_BASIC_ROUNDED_OPERATIONS), sqrtf the
// correctly rounded sequence NumPy's float32 sqrt agrees with (one 1080p field had a blue byte off by one)
__device__ __forceinline__ float vis_mag(float u, float v)
{
    return sqrtf(__fadd_rn(__fmul_rn(u, u), __fmul_rn(v, v)));
}

__device__ __forceinline__ float vis_angle(float u, float v)
{
    const float ax = fabsf(u), ay = fabsf(v);
    const bool steep = !(ax >= ay);
    const float c = __fdiv_rn(steep ? ax : ay, __fadd_rn(steep ? ay : ax, kDblEps));
    const float c2 = __fmul_rn(c, c);
    float a = __fadd_rn(__fmul_rn(kP7, c2), kP5);
    a = __fadd_rn(__fmul_rn(a, c2), kP3);
    a = __fadd_rn(__fmul_rn(a, c2), kP1);
    a = __fmul_rn(a, c);
    if (steep) a = __fsub_rn(90.0f, a);
    if (u < 0.0f) a = __fsub_rn(180.0f, a);
    if (v < 0.0f) a = __fsub_rn(360.0f, a);
    return a;
}

// ----------------------------------------------------------------------------- range select
// Digits of the magnitude bits: 11 / 11 / 10, most significant first.  Every 32-bit pattern (NaN, -NaN, Inf included)
// maps to an in-range bin of every pass.
constexpr int kBins = 2048;
constexpr int kStateWords = 16;                      // per field: prefix lo, prefix hi, rank lo, rank hi, max bits, pad
constexpr int kFieldWords = 2 * kBins + kStateWords;    // two histograms (ranks lo, hi) + state
constexpr int kSelUnroll = 4;                        // float4 loads (pixel pairs) in flight per thread
constexpr size_t kSelPairsPerBlock = 256 * kSelUnroll * 4;   // 8192 px per workgroup

__device__ __forceinline__ int digit_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__device__ __forceinline__ uint32_t digit_mask(int pass) { return pass == 2 ? 0x3ffu : 0x7ffu; }

// A lane's run of equal bins: consecutive pixels of a smooth field mostly share a bin, so one LDS atomic per run
// instead of one per pixel keeps same-address serialisation down.
struct Run {
    uint32_t bin = 0, cnt = 0;
    __device__ __forceinline__ void add(uint32_t *h, uint32_t b)
    {
        if (b != bin) {
            if (cnt) atomicAdd(&h[bin], cnt);
            bin = b;
            cnt = 0;
        }
        ++cnt;
    }
    __device__ __forceinline__ void flush(uint32_t *h) { if (cnt) atomicAdd(&h[bin], cnt); cnt = 0; }
};

__global__ void vis_init_kernel(uint32_t *__restrict__ ws, uint32_t lo, uint32_t hi)
{
    uint32_t *fw = ws + (size_t)blockIdx.x * kFieldWords;
    for (int i = threadIdx.x; i < kFieldWords; i += blockDim.x) {
        uint32_t v = 0;
        if (i == 2 * kBins + 2) v = lo;
        if (i == 2 * kBins + 3) v = hi;
        fw[i] = v;
    }
}

// One pass: per-workgroup LDS histograms of this pass's digit over the pixels whose higher digits equal the prefix of
// rank lo (histogram 0) or of rank hi (histogram 1; only while the two prefixes differ), merged into the field's global
// histograms with one atomic per non-empty bin.  Pass 0 also takes the maximum.  grid = (workgroups per field, batch).
__global__ __launch_bounds__(256)
void vis_hist_kernel(const float *__restrict__ flow, size_t n, float th, int pass, uint32_t *__restrict__ ws)
{
    __shared__ uint32_t h[2][kBins];
    __shared__ uint32_t block_max;
    const int f = blockIdx.y;
    uint32_t *fw = ws + (size_t)f * kFieldWords;
    const uint32_t *st = fw + 2 * kBins;
    const uint32_t pl = st[0], ph = st[1];
    const bool same = pl == ph;
    const int shift = digit_shift(pass), pshift = pass == 1 ? 21 : 10;
    const uint32_t dmask = digit_mask(pass);
    for (int i = threadIdx.x; i < 2 * kBins; i += 256) (&h[0][0])[i] = 0;
    if (threadIdx.x == 0) block_max = 0;
    __syncthreads();

    Run r0, r1;
    uint32_t mx = 0;
    auto take = [&](float u, float v) {
        const uint32_t k = __float_as_uint(vis_mag(vis_th(u, th), vis_th(v, th)));
        if (pass == 0) {
            r0.add(h[0], k >> 21);
            mx = max(mx, k);
        } else {
            const uint32_t p = k >> pshift, d = (k >> shift) & dmask;
            if (p == pl) r0.add(h[0], d);
            if (!same && p == ph) r1.add(h[1], d);
        }
    };

    const float *fl = flow + (size_t)f * n * 2;
    const size_t head = (reinterpret_cast<uintptr_t>(fl) & 15) ? 1 : 0;       // odd n: every other field starts 8 B off
    const size_t n2 = (n - head) / 2;
    const float4 *f4 = reinterpret_cast<const float4 *>(fl + 2 * head);
    for (size_t c0 = (size_t)blockIdx.x * kSelPairsPerBlock; c0 < n2; c0 += (size_t)gridDim.x * kSelPairsPerBlock) {
        for (size_t c = c0; c < c0 + kSelPairsPerBlock && c < n2; c += 256 * kSelUnroll) {
            float4 q[kSelUnroll];
#pragma unroll
            for (int k = 0; k < kSelUnroll; ++k) {
                const size_t i = c + (size_t)k * 256 + threadIdx.x;
                q[k] = i < n2 ? f4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
#pragma unroll
            for (int k = 0; k < kSelUnroll; ++k) {
                if (c + (size_t)k * 256 + threadIdx.x >= n2) continue;
                take(q[k].x, q[k].y);
                take(q[k].z, q[k].w);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (head) take(fl[0], fl[1]);
        if ((n - head) & 1) take(fl[2 * (n - 1)], fl[2 * (n - 1) + 1]);
    }
    r0.flush(h[0]);
    r1.flush(h[1]);
    if (pass == 0) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
        if ((threadIdx.x & 63) == 0 && mx) atomicMax(&block_max, mx);
    }
    __syncthreads();
    uint32_t *g = fw;
    for (int b = threadIdx.x; b < kBins; b += 256) {
        if (h[0][b]) atomicAdd(&g[b], h[0][b]);
        if (!same && h[1][b]) atomicAdd(&g[kBins + b], h[1][b]);
    }
    if (pass == 0 && threadIdx.x == 0 && block_max) atomicMax(&fw[2 * kBins + 4], block_max);
}

// Exclusive scan of one value per thread over a 256-thread workgroup (wave scans through shuffles, wave totals via LDS).
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wave_tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)s, off);
        if (lane >= off) s += o;
    }
    if (lane == 63) wave_tot[wave] = s;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; ++w) before += wave_tot[w];
    __syncthreads();
    return before + s - v;
}

// The bin of each rank in this pass's histograms: prefix <- prefix * bins + digit, rank <- rank - count before the bin.
// Zeroes the histograms for the next pass.  After the last pass, NumPy's lerp (numpy/lib/_function_base_impl.py _lerp) and
// the fallbacks of flow_class.py:910-916 give range_out[f].  grid = batch, block = 256.
__global__ __launch_bounds__(256)
void vis_select_kernel(uint32_t *__restrict__ ws, int pass, float gamma, float *__restrict__ range_out)
{
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t res[4];
    uint32_t *fw = ws + (size_t)blockIdx.x * kFieldWords;
    uint32_t *st = fw + 2 * kBins;
    const uint32_t pl = st[0], ph = st[1], rl = st[2], rh = st[3];
    const bool same = pl == ph;
    const int nb = pass == 2 ? 1024 : 2048, per = nb / 256, bits = pass == 2 ? 10 : 11;
    if (threadIdx.x == 0) { res[0] = pl; res[1] = ph; res[2] = rl; res[3] = rh; }
    for (int t = 0; t < 2; ++t) {
        const uint32_t *hist = fw + ((t == 1 && !same) ? kBins : 0);
        const uint32_t k = t ? rh : rl;
        const int b0 = threadIdx.x * per;
        uint32_t sum = 0;
        for (int j = 0; j < per; ++j) sum += hist[b0 + j];
        uint32_t before = block_exclusive_scan(sum, wave_tot);
        if (k >= before && k - before < sum) {
            for (int j = 0; j < per; ++j) {
                const uint32_t c = hist[b0 + j];
                if (k - before < c) {
                    res[t] = ((t ? ph : pl) << bits) | (uint32_t)(b0 + j);
                    res[2 + t] = k - before;
                    break;
                }
                before += c;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * kBins; i += 256) fw[i] = 0;
    if (threadIdx.x == 0) {
        st[0] = res[0]; st[1] = res[1]; st[2] = res[2]; st[3] = res[3];
        if (pass == 2) {
            const float a = __uint_as_float(res[0]), b = __uint_as_float(res[1]);
            const float d = __fsub_rn(b, a);
            const float p = gamma >= 0.5f ? __fsub_rn(b, __fmul_rn(d, __fsub_rn(1.0f, gamma))) : __fadd_rn(a, __fmul_rn(d, gamma));
            const float mx = __uint_as_float(st[4]);
            range_out[blockIdx.x] = p > 0.0f ? p : (mx > 0.0f ? mx : 1.0f);
        }
    }
}

// ----------------------------------------------------------------------------- render
// One pixel of thresholded components u, v: H, S, V of flow_class.py:889-922 and the bytes of :925-947.  hsv: rint; rgb / bgr: the float64 arithmetic
// NumPy's promotions give (i = int64(h * 6) makes f = h * 6 - i and all that follows float64).
__device__ __forceinline__ uint32_t vis_pixel(float u, float v, bool m, bool border, bool show_mask, float range, int mode)
{
    const float mag = vis_mag(u, v);
    float a = vis_angle(u, v);
    if (a >= 360.0f) a = __fsub_rn(a, 360.0f);                         // np.mod(a, 360) for a in [0, 360]
    float Hh = __fmul_rn(a, 0.5f);
    float S = __fdiv_rn(__fmul_rn(mag, 255.0f), range);
    S = fminf(fmaxf(S, 0.0f), 255.0f);
    float V = (show_mask && !m) ? 180.0f : 255.0f;
    if (border) Hh = S = V = 0.0f;
    if (mode == OFL_VIS_HSV)
        return (uint32_t)(uint8_t)(int)rintf(Hh) | ((uint32_t)(uint8_t)(int)rintf(S) << 8) | ((uint32_t)(uint8_t)(int)rintf(V) << 16);
    const float h = __fdiv_rn(Hh, 180.0f), s = __fdiv_rn(S, 255.0f), vv = __fdiv_rn(V, 255.0f);
    const float h6 = __fmul_rn(h, 6.0f);
    const int i = (int)h6;                                            // truncation, as np.int_
    const double fd = __dsub_rn((double)h6, (double)i), td = __dsub_rn(1.0, fd);
    const double sd = (double)s, vd = (double)vv;
    const double c0 = __dmul_rn(__dsub_rn(1.0, __dmul_rn(sd, 0.0)), vd);
    const double c1 = __dmul_rn(__dsub_rn(1.0, __dmul_rn(sd, 1.0)), vd);
    const double c2 = __dmul_rn(__dsub_rn(1.0, __dmul_rn(sd, fd)), vd);
    const double c3 = __dmul_rn(__dsub_rn(1.0, __dmul_rn(sd, td)), vd);
    double r, g, b;
    switch (((i % 6) + 6) % 6) {
    case 0:  r = c0; g = c3; b = c1; break;
    case 1:  r = c2; g = c0; b = c1; break;
    case 2:  r = c1; g = c0; b = c3; break;
    case 3:  r = c1; g = c2; b = c0; break;
    case 4:  r = c3; g = c1; b = c0; break;
    default: r = c0; g = c1; b = c2; break;
    }
    const uint32_t R = (uint8_t)(int)rint(__dmul_rn(r, 255.0)), G = (uint8_t)(int)rint(__dmul_rn(g, 255.0)),
                   B = (uint8_t)(int)rint(__dmul_rn(b, 255.0));
    return mode == OFL_VIS_BGR ? (B | (G << 8) | (R << 16)) : (R | (G << 8) | (B << 16));
}

struct VisArgs {
    const float *flow;
    const uint8_t *mask;
    int H, W;
    size_t n, total;
    float th;
    const float *range_dev;
    float range_const;
    int mode, flags;
    uint8_t *out;
};

// mask-true pixel with a mask-false 4-neighbour or on the image frame (findContours + drawContours(thickness=1))
__device__ __forceinline__ bool vis_border(const VisArgs &A, size_t fbase, int x, int y)
{
    if (x == 0 || y == 0 || x == A.W - 1 || y == A.H - 1) return true;
    if (!A.mask) return false;
    const uint8_t *m = A.mask + fbase + (size_t)y * A.W + x;
    return !m[-1] || !m[1] || !m[-(ptrdiff_t)A.W] || !m[A.W];
}

__device__ __forceinline__ uint32_t vis_one(const VisArgs &A, float u, float v, bool m, size_t f, int x, int y)
{
    const bool show = (A.flags & OFL_VIS_SHOW_MASK) != 0;
    const bool border = (A.flags & OFL_VIS_MASK_BORDERS) && m && vis_border(A, f * A.n, x, y);
    const float range = A.range_dev ? A.range_dev[f] : A.range_const;
    return vis_pixel(vis_th(u, A.th), vis_th(v, A.th), m, border, show, range, A.mode);
}

// Four pixels per lane and step: two 16-byte loads of vectors, one mask word, three dwords of output.  The batch is one
// linear run of batch * H * W pixels; a group of four may straddle rows and fields.  WIDE 0 serves vectors 8 bytes off the
// 16-byte grid or a mask off the 4-byte grid (a view inside a batch of odd fields): the same four pixels per lane from
// four 8-byte loads and four mask bytes.
template <int WIDE>
__global__ __launch_bounds__(256)
void vis_render_kernel(VisArgs A)
{
    const size_t groups = A.total / 4, stride = (size_t)gridDim.x * blockDim.x;
    const float4 *f4 = reinterpret_cast<const float4 *>(A.flow);
    const float2 *f2 = reinterpret_cast<const float2 *>(A.flow);
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        float4 a, b;
        uint32_t mw = 0x01010101u;
        if (WIDE) {
            a = f4[2 * g];
            b = f4[2 * g + 1];
            if (A.mask) mw = reinterpret_cast<const uint32_t *>(A.mask)[g];
        } else {
            const float2 p0 = f2[4 * g], p1 = f2[4 * g + 1], p2 = f2[4 * g + 2], p3 = f2[4 * g + 3];
            a = make_float4(p0.x, p0.y, p1.x, p1.y);
            b = make_float4(p2.x, p2.y, p3.x, p3.y);
            if (A.mask) {
                const uint8_t *m = A.mask + 4 * g;
                mw = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
            }
        }
        const size_t p0 = 4 * g;
        size_t f = p0 / A.n;
        const size_t r = p0 - f * A.n;
        int y = (int)(r / (size_t)A.W), x = (int)(r - (size_t)y * A.W);
        const float uu[4] = {a.x, a.z, b.x, b.z}, vv[4] = {a.y, a.w, b.y, b.w};
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            px[j] = vis_one(A, uu[j], vv[j], ((mw >> (8 * j)) & 0xffu) != 0, f, x, y);
            if (++x == A.W) {
                x = 0;
                if (++y == A.H) { y = 0; ++f; }
            }
        }
        uint32_t *o = reinterpret_cast<uint32_t *>(A.out) + 3 * g;
        o[0] = px[0] | (px[1] << 24);
        o[1] = (px[1] >> 8) | (px[2] << 16);
        o[2] = (px[2] >> 16) | (px[3] << 8);
    }
    if (blockIdx.x == 0 && threadIdx.x < (A.total & 3)) {                 // tail: one byte triple per lane
        const size_t p = groups * 4 + threadIdx.x, f = p / A.n, r = p - f * A.n;
        const int y = (int)(r / (size_t)A.W), x = (int)(r - (size_t)y * A.W);
        const uint32_t c = vis_one(A, A.flow[2 * p], A.flow[2 * p + 1], A.mask ? A.mask[p] != 0 : true, f, x, y);
        A.out[3 * p] = (uint8_t)c;
        A.out[3 * p + 1] = (uint8_t)(c >> 8);
        A.out[3 * p + 2] = (uint8_t)(c >> 16);
    }
}

int vis_stream_grid(size_t items)
{
    size_t nb = (items + 255) / 256;
    return (int)(nb < 1 ? 1 : (nb < 0x7fffffff ? nb : 0x7fffffff));
}

}  // namespace

extern "C" {

int ofl_visualise_workspace_bytes(int H, int W, int batch, size_t *bytes)
{
    if (!bytes || H <= 0 || W <= 0 || batch <= 0) return fail(OFL_E_INVALID, "ofl_visualise_workspace_bytes: bad arguments");
    *bytes = (size_t)batch * kFieldWords * sizeof(uint32_t);
    return OFL_OK;
}

int ofl_visualise_range_dev(const float *flow, int H, int W, int batch, float threshold, size_t lo, size_t hi, float gamma,
                            void *workspace, size_t workspace_bytes, float *range_out, void *stream)
{
    OFL_TRY(need_device());
    if (!flow || !workspace || !range_out || H <= 0 || W <= 0 || batch <= 0 || batch > 65535)
        return fail(OFL_E_INVALID, "ofl_visualise_range: bad arguments");
    const size_t n = (size_t)H * W;
    if (n > 0xffffffffu || lo > hi || hi >= n) return fail(OFL_E_INVALID, "ofl_visualise_range: ranks %zu, %zu outside a field of %zu px", lo, hi, n);
    if (workspace_bytes < (size_t)batch * kFieldWords * sizeof(uint32_t))
        return fail(OFL_E_INVALID, "ofl_visualise_range: workspace of %zu bytes is too small", workspace_bytes);
    if (reinterpret_cast<uintptr_t>(flow) & 7) return fail(OFL_E_INVALID, "ofl_visualise_range: flow must be 8-byte aligned");
    hipStream_t s = stream_of(stream);
    uint32_t *ws = (uint32_t *)workspace;
    hipLaunchKernelGGL(vis_init_kernel, dim3(batch), dim3(256), 0, s, ws, (uint32_t)lo, (uint32_t)hi);
    const size_t per_field = (n / 2 + kSelPairsPerBlock - 1) / kSelPairsPerBlock;
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>(per_field, 4096));
    for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(vis_hist_kernel, dim3(gx, batch), dim3(256), 0, s, flow, n, threshold, pass, ws);
        hipLaunchKernelGGL(vis_select_kernel, dim3(batch), dim3(256), 0, s, ws, pass, gamma, range_out);
    }
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_visualise_dev(const float *flow, const uint8_t *mask, int H, int W, int batch, float threshold,
                      const float *range_dev, float range_const, int mode, int flags, uint8_t *out, void *stream)
{
    OFL_TRY(need_device());
    if (!flow || !out || H <= 0 || W <= 0 || batch <= 0) return fail(OFL_E_INVALID, "ofl_visualise: bad arguments");
    if (mode != OFL_VIS_HSV && mode != OFL_VIS_RGB && mode != OFL_VIS_BGR) return fail(OFL_E_INVALID, "ofl_visualise: mode %d", mode);
    if (flags & ~(OFL_VIS_SHOW_MASK | OFL_VIS_MASK_BORDERS)) return fail(OFL_E_INVALID, "ofl_visualise: flags 0x%x", flags);
    if ((reinterpret_cast<uintptr_t>(flow) & 7) || (reinterpret_cast<uintptr_t>(out) & 3))
        return fail(OFL_E_INVALID, "ofl_visualise: flow must be 8-byte, out 4-byte aligned");
    const bool wide = !(reinterpret_cast<uintptr_t>(flow) & 15) && !(reinterpret_cast<uintptr_t>(mask) & 3);
    if (!range_dev && !(range_const > 0.0f)) return fail(OFL_E_INVALID, "ofl_visualise: range_const must be > 0");
    VisArgs A;
    A.flow = flow; A.mask = mask; A.H = H; A.W = W;
    A.n = (size_t)H * W; A.total = A.n * batch;
    A.th = threshold; A.range_dev = range_dev; A.range_const = range_const;
    A.mode = mode; A.flags = flags; A.out = out;
    const dim3 grid(vis_stream_grid(A.total / 4)), block(256);
    if (wide) hipLaunchKernelGGL((vis_render_kernel<1>), grid, block, 0, stream_of(stream), A);
    else      hipLaunchKernelGGL((vis_render_kernel<0>), grid, block, 0, stream_of(stream), A);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

}  // extern "C"
