// ofl_error.hip -- K14: an estimated field against a ground truth (gfx950): end-point error, threshold and outlier counts and
// the error by speed of the ground truth, one 96-byte record (struct ofl_flow_error, include/ofl.h) per pair.
//
// Per pixel, float32 and one rounding per operation (__fsub_rn / __fmul_rn / __fadd_rn, no contraction; sqrtf is the
// correctly rounded one, see the note above vis_mag in ofl_visualise.hip):
//     du = est.u - gt.u;  dv = est.v - gt.v;  epe = sqrtf(du*du + dv*dv);  g = sqrtf(gt.u*gt.u + gt.v*gt.v)
//     eval = gt.mask & (est_mask ? est.mask : 1);  ok = eval & isfinite(epe);  bad = eval & !isfinite(epe)
//     over[k] = ok & (epe > thr[k]);  outlier = ok & (epe > out_abs) & (epe > out_rel * g);  bin = #{j : g >= edges[j]}
//
// A pure stream: 18 B/px read, nothing written per pixel unless a map is asked for, no LDS staging of data, no atomics.
// blockIdx = (chunk, pair); a chunk is kChunk = 4096 consecutive pixels of the pair.  Thread t of chunk c owns the pixels
// c * 4096 + s * 1024 + 4 * t + j (s, j < 4) IN EVERY INSTANTIATION, so the order of additions is a function of H * W alone:
//   wide     est / gt 16-byte, masks 4-byte aligned (maps likewise), and with batch > 1 also H * W % 4 == 0 (otherwise every
//            second pair sits 8 bytes off the 16-byte grid): per step and field two 16-byte loads and one 4-byte mask word;
//   generic  everything else: 8-byte and 1-byte loads.
// Both ask for all four steps' loads before the first use, and both finish the last quad of a pair whose pixel count is no
// multiple of 4 pixel by pixel.  A thread adds its <= 16 terms per sum in pixel order; a wave reduces by the six-level xor
// butterfly of ofl_fit.hip (a + b == b + a: every lane holds the same bits); the four wave values are added in order; the
// workgroup writes one partial (6 doubles + 12 uint32) to the workspace, stored [pair][sum][chunk] so that the finishing
// kernel reads it coalesced.  Counts are popcount(ballot): wave-uniform, in scalar registers.
// Which maps are written is a template argument (no pointer test inside the body): 2 paths x 4 = 8 instantiations.
// error_finish_kernel, one workgroup per pair: thread t adds the partials t, t + 256, ... in order, then butterfly, then the
// waves in order.  Longest chain of additions: 16 + 6 + 3 + ceil(chunks / 256) + 6 + 3.
#include <stddef.h>
#include "ofl_common.h"
#include "ofl_host_stage.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

constexpr int kChunk = 4096, kThreads = 256, kSteps = 4, kStepPx = kChunk / kSteps;
constexpr int kSums = 6, kWords = 12;                     // per partial: 6 doubles, 11 counts + the maximum's bits
constexpr size_t kPartialBytes = kSums * sizeof(double) + kWords * sizeof(uint32_t);

static_assert(sizeof(struct ofl_flow_error) == 96 && offsetof(struct ofl_flow_error, sum_epe) == 48, "record layout");
static_assert(offsetof(struct ofl_flow_error, max_epe_bits) == 4 * (kWords - 1), "record layout");

struct EArgs {
    const float   *est, *gt;
    const uint8_t *em, *gm;          // em may be NULL
    float         *epe_map;
    uint8_t       *out_map;
    double        *psum;             // [batch][kSums][chunks]
    uint32_t      *pcnt;             // [batch][kWords][chunks]
    uint32_t       hw, chunks;
    float          thr[4], edges[3], out_abs, out_rel;
};

struct Quad { float4 a, b; uint32_t m; };        // four vectors (u0 v0 u1 v1 | u2 v2 u3 v3) and their four mask bytes

// the quad at pixel `at` of a field of which `left` pixels remain (>= 4: whole; 1..3: the pair's last, pixel by pixel)
// FULL: the whole chunk lies inside the pair, nothing is tested
template <bool WIDE, bool FULL>
__device__ __forceinline__ Quad load_quad(const float *__restrict__ f, const uint8_t *__restrict__ m, size_t at, uint32_t left)
{
    Quad q;
    q.a = q.b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    q.m = 0;
    if (FULL || left >= 4) {
        if (WIDE) {
            q.a = *reinterpret_cast<const float4 *>(f + 2 * at);
            q.b = *reinterpret_cast<const float4 *>(f + 2 * at + 4);
            q.m = m ? *reinterpret_cast<const uint32_t *>(m + at) : 0x01010101u;
        } else {
            const float2 p0 = *reinterpret_cast<const float2 *>(f + 2 * at), p1 = *reinterpret_cast<const float2 *>(f + 2 * at + 2);
            const float2 p2 = *reinterpret_cast<const float2 *>(f + 2 * at + 4), p3 = *reinterpret_cast<const float2 *>(f + 2 * at + 6);
            q.a = make_float4(p0.x, p0.y, p1.x, p1.y);
            q.b = make_float4(p2.x, p2.y, p3.x, p3.y);
            q.m = m ? (uint32_t)m[at] | ((uint32_t)m[at + 1] << 8) | ((uint32_t)m[at + 2] << 16) | ((uint32_t)m[at + 3] << 24) : 0x01010101u;
        }
    } else if (left > 0) {
        const float2 p0 = *reinterpret_cast<const float2 *>(f + 2 * at);
        q.a.x = p0.x; q.a.y = p0.y;
        q.m = m ? (uint32_t)m[at] : 1u;
        if (left > 1) {
            const float2 p1 = *reinterpret_cast<const float2 *>(f + 2 * at + 2);
            q.a.z = p1.x; q.a.w = p1.y;
            q.m |= (m ? (uint32_t)m[at + 1] : 1u) << 8;
        }
        if (left > 2) {
            const float2 p2 = *reinterpret_cast<const float2 *>(f + 2 * at + 4);
            q.b.x = p2.x; q.b.y = p2.y;
            q.m |= (m ? (uint32_t)m[at + 2] : 1u) << 16;
        }
    }
    return q;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
    return v;
}

// the four wave values of every sum and word -> one value per sum and word in threads 0 .. kWords - 1
struct BlockOut { double sum; uint32_t word; };

__device__ __forceinline__ BlockOut block_reduce(const double (&sum)[kSums], const uint32_t (&word)[kWords])
{
    __shared__ double   wsum[4][kSums];
    __shared__ uint32_t wword[4][kWords];
    const int wave = threadIdx.x >> 6, t = threadIdx.x;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < kSums; ++s) wsum[wave][s] = sum[s];
#pragma unroll
        for (int k = 0; k < kWords; ++k) wword[wave][k] = word[k];
    }
    __syncthreads();
    BlockOut o = { 0.0, 0u };
    if (t < kSums) o.sum = ((wsum[0][t] + wsum[1][t]) + wsum[2][t]) + wsum[3][t];
    if (t < kWords - 1) o.word = wword[0][t] + wword[1][t] + wword[2][t] + wword[3][t];
    if (t == kWords - 1) o.word = max(max(wword[0][t], wword[1][t]), max(wword[2][t], wword[3][t]));
    return o;
}

// one chunk: the loads, the per-pixel arithmetic and the thread's sums.  FULL (the chunk lies inside the pair: all chunks of a
// pair but possibly its last) has no test and no branch around its loads.
template <bool WIDE, int MAPS, bool FULL>
__device__ __forceinline__ void error_chunk(const EArgs &a, double (&sum)[kSums], uint32_t (&word)[kWords])
{
    const uint32_t chunk = blockIdx.x, pair = blockIdx.y, hw = a.hw;
    const size_t item = (size_t)pair * hw;
    const uint32_t q0 = chunk * (uint32_t)kChunk + 4u * threadIdx.x;             // < 2^31 + 4096

    Quad e[kSteps], g[kSteps];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const uint32_t q = q0 + (uint32_t)(s * kStepPx), left = q < hw ? hw - q : 0u;
        e[s] = load_quad<WIDE, FULL>(a.est + 2 * item, a.em ? a.em + item : nullptr, q, left);
        g[s] = load_quad<WIDE, FULL>(a.gt + 2 * item, a.gm + item, q, left);
    }

    uint32_t mx = 0;
    // popcount of a wave's ballot: wave-uniform, so the counts live in scalar registers
    auto count = [](bool p) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(p)); };
    const float thr0 = a.thr[0], thr1 = a.thr[1], thr2 = a.thr[2], thr3 = a.thr[3], e0 = a.edges[0], e1 = a.edges[1], e2 = a.edges[2];
    const float out_abs = a.out_abs, out_rel = a.out_rel;
    uint32_t n_ge[3] = {0, 0, 0};                              // ok pixels with g >= edges[j]: nested, the edges ascend

#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const float eu[4] = {e[s].a.x, e[s].a.z, e[s].b.x, e[s].b.z}, ev[4] = {e[s].a.y, e[s].a.w, e[s].b.y, e[s].b.w};
        const float gu[4] = {g[s].a.x, g[s].a.z, g[s].b.x, g[s].b.z}, gv[4] = {g[s].a.y, g[s].a.w, g[s].b.y, g[s].b.w};
        float    em_out[4];
        uint32_t ob = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float du = __fsub_rn(eu[j], gu[j]), dv = __fsub_rn(ev[j], gv[j]);
            const float epe = sqrtf(__fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv)));
            const float gm = sqrtf(__fadd_rn(__fmul_rn(gu[j], gu[j]), __fmul_rn(gv[j], gv[j])));
            // a pixel past the end of the pair has a clear gt mask byte: it is in no count
            const bool eval = (((g[s].m >> (8 * j)) & 0xffu) != 0) & (((e[s].m >> (8 * j)) & 0xffu) != 0);
            const bool fin = (__float_as_uint(epe) & 0x7f800000u) != 0x7f800000u;
            const bool ok = eval & fin;
            // outside `ok` the error compares as -1 (below every threshold, none is negative) and the speed as NaN (in no
            // comparison), so every test below carries `ok` without a further AND
            const float ek = ok ? epe : -1.0f, gk = ok ? gm : __uint_as_float(0x7fc00000u);
            const bool ge0 = gk >= e0, ge1 = gk >= e1, ge2 = gk >= e2;
            const bool outlier = (ek > out_abs) & (ek > __fmul_rn(out_rel, gm));
            word[0] += count(ok);
            word[1] += count(eval & !fin);
            word[2] += count(ek > thr0);
            word[3] += count(ek > thr1);
            word[4] += count(ek > thr2);
            word[5] += count(ek > thr3);
            word[6] += count(outlier);
            n_ge[0] += count(ge0);
            n_ge[1] += count(ge1);
            n_ge[2] += count(ge2);
            const float t = ok ? epe : 0.0f;                   // adding +0.0 to a sum that is >= +0.0 changes no bit
            const double d = (double)t;
            mx = max(mx, __float_as_uint(t));
            sum[0] += d;
            sum[1] += d * d;
            sum[2] += (double)(ge0 ? 0.0f : t);                // bin 0: below the first edge (t = 0 outside `ok`)
            sum[3] += (double)((ge0 & !ge1) ? t : 0.0f);
            sum[4] += (double)((ge1 & !ge2) ? t : 0.0f);
            sum[5] += (double)(ge2 ? t : 0.0f);
            em_out[j] = t;
            ob |= (outlier ? 1u : 0u) << (8 * j);
        }
        if (MAPS) {
            const uint32_t q = q0 + (uint32_t)(s * kStepPx), left = q < hw ? hw - q : 0u;
            const size_t at = item + q;
            if (WIDE && (FULL || left >= 4)) {
                if (MAPS & 1) *reinterpret_cast<float4 *>(a.epe_map + at) = make_float4(em_out[0], em_out[1], em_out[2], em_out[3]);
                if (MAPS & 2) *reinterpret_cast<uint32_t *>(a.out_map + at) = ob;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (FULL || (uint32_t)j < left) {
                        if (MAPS & 1) a.epe_map[at + j] = em_out[j];
                        if (MAPS & 2) a.out_map[at + j] = (uint8_t)((ob >> (8 * j)) & 1u);
                    }
                }
            }
        }
    }

    word[7] = word[0] - n_ge[0];                               // n_bin: differences of the nested counts, exact
    word[8] = n_ge[0] - n_ge[1];
    word[9] = n_ge[1] - n_ge[2];
    word[10] = n_ge[2];
    word[kWords - 1] = mx;                                     // per lane; the wave's maximum is taken by the caller
}

// MAPS: bit 0 the epe_map, bit 1 the outlier_map is written (a template argument, so that the body has no branch on a pointer)
template <bool WIDE, int MAPS>
__global__ __launch_bounds__(kThreads)
void error_kernel(const EArgs a)
{
    const uint32_t chunk = blockIdx.x, pair = blockIdx.y;
    double   sum[kSums];
    uint32_t word[kWords];
#pragma unroll
    for (int s = 0; s < kSums; ++s) sum[s] = 0.0;
#pragma unroll
    for (int k = 0; k < kWords; ++k) word[k] = 0;
    if ((uint64_t)(chunk + 1) * kChunk <= a.hw) error_chunk<WIDE, MAPS, true>(a, sum, word);
    else                                        error_chunk<WIDE, MAPS, false>(a, sum, word);
#pragma unroll
    for (int s = 0; s < kSums; ++s) sum[s] = wave_sum(sum[s]);
    word[kWords - 1] = wave_max(word[kWords - 1]);
    const BlockOut o = block_reduce(sum, word);
    if (threadIdx.x < kSums)  a.psum[((size_t)pair * kSums + threadIdx.x) * a.chunks + chunk] = o.sum;
    if (threadIdx.x < kWords) a.pcnt[((size_t)pair * kWords + threadIdx.x) * a.chunks + chunk] = o.word;
}

// one workgroup per pair: thread t takes the partials t, t + 256, ... in order, then butterfly, then the waves in order
__global__ __launch_bounds__(kThreads)
void error_finish_kernel(const double *__restrict__ psum, const uint32_t *__restrict__ pcnt, uint32_t chunks,
                         struct ofl_flow_error *__restrict__ records)
{
    const uint32_t pair = blockIdx.x;
    double   sum[kSums];
    uint32_t word[kWords];
#pragma unroll
    for (int s = 0; s < kSums; ++s) sum[s] = 0.0;
#pragma unroll
    for (int k = 0; k < kWords; ++k) word[k] = 0;
    for (uint32_t i = threadIdx.x; i < chunks; i += kThreads) {
#pragma unroll
        for (int s = 0; s < kSums; ++s) sum[s] += psum[((size_t)pair * kSums + s) * chunks + i];
#pragma unroll
        for (int k = 0; k < kWords - 1; ++k) word[k] += pcnt[((size_t)pair * kWords + k) * chunks + i];
        word[kWords - 1] = max(word[kWords - 1], pcnt[((size_t)pair * kWords + (kWords - 1)) * chunks + i]);
    }
#pragma unroll
    for (int s = 0; s < kSums; ++s) sum[s] = wave_sum(sum[s]);
#pragma unroll
    for (int k = 0; k < kWords - 1; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) word[k] += (uint32_t)__shfl_xor((int)word[k], off);
    }
    word[kWords - 1] = wave_max(word[kWords - 1]);
    const BlockOut o = block_reduce(sum, word);
    char *rec = reinterpret_cast<char *>(records + pair);
    if (threadIdx.x < kWords) reinterpret_cast<uint32_t *>(rec)[threadIdx.x] = o.word;
    if (threadIdx.x < kSums)  reinterpret_cast<double *>(rec + offsetof(struct ofl_flow_error, sum_epe))[threadIdx.x] = o.sum;
}

template <bool WIDE>
void launch_error(int maps, const EArgs &a, dim3 grid, hipStream_t s)
{
    switch (maps) {
    case 0:  hipLaunchKernelGGL((error_kernel<WIDE, 0>), grid, dim3(kThreads), 0, s, a); break;
    case 1:  hipLaunchKernelGGL((error_kernel<WIDE, 1>), grid, dim3(kThreads), 0, s, a); break;
    case 2:  hipLaunchKernelGGL((error_kernel<WIDE, 2>), grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((error_kernel<WIDE, 3>), grid, dim3(kThreads), 0, s, a); break;
    }
}

inline uint32_t chunks_of(int H, int W) { return (uint32_t)(((int64_t)H * W + kChunk - 1) / kChunk); }

int check_error_args(const char *who, const void *est, const void *gt, const void *gt_mask, int H, int W, int batch,
                     const float *thr, float out_abs, float out_rel, const float *edges, const void *records)
{
    if (!est || !gt || !gt_mask || !thr || !edges || !records)
        return fail(OFL_E_INVALID, "%s: NULL pointer (est, gt, gt_mask, thr, edges and records are required)", who);
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31))
        return fail(OFL_E_INVALID, "%s: H, W must be >= 1 with H * W < 2^31 (got %d x %d)", who, H, W);
    if (batch < 1 || batch > 65535) return fail(OFL_E_INVALID, "%s: batch must be in [1, 65535], got %d", who, batch);
    for (int k = 0; k < 4; ++k)
        if (!(thr[k] >= 0.0f)) return fail(OFL_E_INVALID, "%s: thr[%d] must not be NaN or negative (got %g)", who, k, (double)thr[k]);
    if (!(out_abs >= 0.0f) || !(out_rel >= 0.0f))
        return fail(OFL_E_INVALID, "%s: out_abs and out_rel must not be NaN or negative (got %g, %g)", who, (double)out_abs, (double)out_rel);
    for (int j = 0; j < 3; ++j)
        if (!(edges[j] >= 0.0f)) return fail(OFL_E_INVALID, "%s: edges[%d] must not be NaN or negative (got %g)", who, j, (double)edges[j]);
    if (edges[1] < edges[0] || edges[2] < edges[1])
        return fail(OFL_E_INVALID, "%s: edges must be ascending (got %g, %g, %g)", who, (double)edges[0], (double)edges[1], (double)edges[2]);
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_flow_error_workspace_bytes(int H, int W, int batch, size_t *bytes)
{
    if (!bytes) return fail(OFL_E_INVALID, "ofl_flow_error_workspace_bytes: NULL pointer");
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) || batch < 1 || batch > 65535)
        return fail(OFL_E_INVALID, "ofl_flow_error_workspace_bytes: H, W >= 1, H * W < 2^31 and batch in [1, 65535] (got %d x %d, %d)", H, W, batch);
    *bytes = (size_t)batch * chunks_of(H, W) * kPartialBytes;
    return OFL_OK;
}

int ofl_flow_error_dev(const float *est, const uint8_t *est_mask, const float *gt, const uint8_t *gt_mask,
                       int H, int W, int batch, const float thr[4], float out_abs, float out_rel, const float edges[3],
                       void *workspace, size_t workspace_bytes, struct ofl_flow_error *records,
                       float *epe_map, uint8_t *outlier_map, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_error_args("ofl_flow_error", est, gt, gt_mask, H, W, batch, thr, out_abs, out_rel, edges, records));
    const uint32_t chunks = chunks_of(H, W);
    const size_t need = (size_t)batch * chunks * kPartialBytes;
    if (!workspace || workspace_bytes < need)
        return fail(OFL_E_INVALID, "ofl_flow_error: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    if (!host_aligned(est, 8) || !host_aligned(gt, 8) || !host_aligned(workspace, 8) || !host_aligned(records, 8) || !host_aligned(epe_map, 4))
        return fail(OFL_E_INVALID, "ofl_flow_error: est, gt, workspace and records must be 8-byte, epe_map 4-byte aligned");
    EArgs a;
    a.est = est; a.gt = gt; a.em = est_mask; a.gm = gt_mask; a.epe_map = epe_map; a.out_map = outlier_map;
    a.psum = static_cast<double *>(workspace);
    a.pcnt = reinterpret_cast<uint32_t *>(a.psum + (size_t)batch * chunks * kSums);
    a.hw = (uint32_t)((int64_t)H * W); a.chunks = chunks;
    for (int k = 0; k < 4; ++k) a.thr[k] = thr[k];
    for (int j = 0; j < 3; ++j) a.edges[j] = edges[j];
    a.out_abs = out_abs; a.out_rel = out_rel;
    // the wide path: every pair's base on the 16-byte (vectors, epe_map) and 4-byte (masks, outlier_map) grid
    const bool wide = host_aligned(est, 16) && host_aligned(gt, 16) && host_aligned(est_mask, 4) && host_aligned(gt_mask, 4) &&
                      host_aligned(epe_map, 16) && host_aligned(outlier_map, 4) && (batch == 1 || a.hw % 4 == 0);
    const int maps = (epe_map ? 1 : 0) | (outlier_map ? 2 : 0);
    const dim3 grid(chunks, (unsigned)batch);
    hipStream_t s = stream_of(stream);
    if (wide) launch_error<true>(maps, a, grid, s);
    else      launch_error<false>(maps, a, grid, s);
    OFL_HIP(hipGetLastError());
    hipLaunchKernelGGL(error_finish_kernel, dim3((unsigned)batch), dim3(kThreads), 0, s, a.psum, a.pcnt, chunks, records);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_flow_error(const float *est, const uint8_t *est_mask, const float *gt, const uint8_t *gt_mask,
                   int H, int W, int batch, const float thr[4], float out_abs, float out_rel, const float edges[3],
                   struct ofl_flow_error *records_host, float *epe_map, uint8_t *outlier_map)
{
    OFL_TRY(need_device());
    OFL_TRY(check_error_args("ofl_flow_error", est, gt, gt_mask, H, W, batch, thr, out_abs, out_rel, edges, records_host));
    const size_t n = (size_t)batch * H * W, wsb = (size_t)batch * chunks_of(H, W) * kPartialBytes;
    HostStage st("ofl_flow_error");
    auto de = st.in(est, n * 2), dg = st.in(gt, n * 2);
    auto dem = st.in(est_mask, n), dgm = st.in(gt_mask, n);
    auto ws = st.scratch<char>(wsb);
    auto rec = st.out(records_host, (size_t)batch);
    auto epe = st.out(epe_map, n);
    auto om = st.out(outlier_map, n);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_flow_error_dev(de, dem, dg, dgm, H, W, batch, thr, out_abs, out_rel, edges, ws, wsb, rec, epe, om, st.stream()));
    return st.download();
}

}  // extern "C"
