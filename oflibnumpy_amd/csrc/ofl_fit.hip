// ofl_fit.hip -- K8: the O(H*W) passes of fitting a 3x3 matrix to a flow field (Flow.matrix, flow_class.py:797-867).
// The correspondences src -> dst are never materialised: every kernel rebuilds them per pixel from the grid, the vector
// and `sign` in float64.  Four kernel families:
//   sums     float64 sums over the (gated) correspondences -- second-order moments, the 9x9 L^T L of the normalised DLT,
//            one Gauss-Newton step's J^T J / J^T r / cost -- as per-workgroup partials that a finishing kernel adds in a
//            fixed order: no floating-point atomics, a grid that depends on H * W only, bit-identical repeats;
//   score    exact inlier counts of K models from one read of the field (LDS counters, integer atomics);
//   median   the two order statistics of the residual bits the median interpolates between, for K models: a three-pass
//            radix select (11 / 11 / 10 bits) with LDS histograms, no host synchronisation between passes;
//   sample   valid pixels by rank (a count / scan index of 4096-px chunks) and a gather of vectors and mask bytes.
#include "ofl_common.h"
#include <algorithm>

#pragma clang fp contract(off)

using namespace ofl;

namespace {

// ----------------------------------------------------------------------------- the field, four pixels per lane and step
struct FitField {
    const float *flow;
    const uint8_t *mask;
    uint32_t n;           // H * W
    int W, sign;
};

constexpr int kFitUnroll = 4;                                // groups of four pixels in flight per thread
constexpr uint32_t kFitGroups = 256 * kFitUnroll;            // groups per chunk
constexpr uint32_t kFitChunk = kFitGroups * 4;               // 4096 px per chunk (one workgroup of the sum kernels)

inline uint32_t fit_chunks(size_t n) { return (uint32_t)std::max<size_t>(1, (n / 4 + kFitGroups - 1) / kFitGroups); }

struct FitTile {
    float4 a[kFitUnroll], b[kFitUnroll];       // vectors of pixels 0, 1 and 2, 3 of each group
    uint32_t m[kFitUnroll];                    // their mask bytes; 0 for a group beyond the field
    int x[kFitUnroll], y[kFitUnroll];          // position of pixel 0
};

// every load of the tile is issued before the first value is looked at.  WIDE 1: vectors on the 16-byte, mask on the 4-byte
// grid.  WIDE 0 (a view inside a batch of odd fields): the same groups per lane from 8-byte and 1-byte loads, so that every
// sum adds the same terms in the same order.
template <int WIDE>
__device__ __forceinline__ void fit_load(const FitField &A, uint32_t chunk, FitTile &T)
{
    const uint32_t groups = A.n / 4;
    const float4 *f4 = reinterpret_cast<const float4 *>(A.flow);
    const float2 *f2 = reinterpret_cast<const float2 *>(A.flow);
    const uint32_t *mw = reinterpret_cast<const uint32_t *>(A.mask);
#pragma unroll
    for (int k = 0; k < kFitUnroll; ++k) {
        const uint32_t g = chunk * kFitGroups + (uint32_t)k * 256 + threadIdx.x;
        const bool in = g < groups;
        if (WIDE) {
            T.a[k] = in ? f4[2 * (size_t)g] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            T.b[k] = in ? f4[2 * (size_t)g + 1] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            T.m[k] = in ? (mw ? mw[g] : 0x01010101u) : 0u;
        } else {
            const float2 z = make_float2(0.0f, 0.0f);
            const float2 p0 = in ? f2[4 * (size_t)g] : z, p1 = in ? f2[4 * (size_t)g + 1] : z;
            const float2 p2 = in ? f2[4 * (size_t)g + 2] : z, p3 = in ? f2[4 * (size_t)g + 3] : z;
            T.a[k] = make_float4(p0.x, p0.y, p1.x, p1.y);
            T.b[k] = make_float4(p2.x, p2.y, p3.x, p3.y);
            uint32_t m = in ? 0x01010101u : 0u;
            if (in && A.mask) {
                const uint8_t *mb = A.mask + 4 * (size_t)g;
                m = (uint32_t)mb[0] | ((uint32_t)mb[1] << 8) | ((uint32_t)mb[2] << 16) | ((uint32_t)mb[3] << 24);
            }
            T.m[k] = m;
        }
        const uint32_t p = 4 * g;
        T.y[k] = (int)(p / (uint32_t)A.W);
        T.x[k] = (int)(p - (uint32_t)T.y[k] * (uint32_t)A.W);
    }
}

// fn(x, y, u, v) for every pixel of the tile whose mask byte is not 0, in a fixed order
template <typename F>
__device__ __forceinline__ void fit_each(const FitField &A, const FitTile &T, F &&fn)
{
#pragma unroll
    for (int k = 0; k < kFitUnroll; ++k) {
        if (!T.m[k]) continue;
        const float uu[4] = {T.a[k].x, T.a[k].z, T.b[k].x, T.b[k].z}, vv[4] = {T.a[k].y, T.a[k].w, T.b[k].y, T.b[k].w};
        int x = T.x[k], y = T.y[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((T.m[k] >> (8 * j)) & 0xffu) fn(x, y, uu[j], vv[j]);
            if (++x == A.W) { x = 0; ++y; }
        }
    }
}

// the n % 4 pixels behind the last group
template <typename F>
__device__ __forceinline__ void fit_tail(const FitField &A, uint32_t chunk, F &&fn)
{
    if (chunk != 0 || threadIdx.x != 0) return;
    for (uint32_t p = (A.n / 4) * 4; p < A.n; ++p) {
        if (A.mask && !A.mask[p]) continue;
        const int y = (int)(p / (uint32_t)A.W);
        fn((int)(p - (uint32_t)y * (uint32_t)A.W), y, A.flow[2 * (size_t)p], A.flow[2 * (size_t)p + 1]);
    }
}

// ----------------------------------------------------------------------------- correspondence, residual, gate
struct Corr { double x, y, X, Y; };          // src (x, y) -> dst (X, Y)

__device__ __forceinline__ bool fit_finite(float a, float b)
{
    return (fabsf(a) <= 3.402823466e38f) && (fabsf(b) <= 3.402823466e38f);   // false for NaN / Inf
}

// ref 's' (sign +1): src = grid, dst = src + v;  ref 't' (sign -1): dst = grid, src = dst - v.  float64 from the float32
// vector: exact.  false for a non-finite vector.
__device__ __forceinline__ bool fit_corr(int sign, int px, int py, float u, float v, Corr &c)
{
    if (!fit_finite(u, v)) return false;
    const double gx = (double)px, gy = (double)py;
    if (sign >= 0) { c.x = gx; c.y = gy; c.X = gx + (double)u; c.Y = gy + (double)v; }
    else           { c.X = gx; c.Y = gy; c.x = gx - (double)u; c.y = gy - (double)v; }
    return true;
}

// The residual of ofl.h: squared reprojection error in float64, one rounding to float32; NaN / Inf (w == 0, overflow)
// become +Inf, which is above every threshold and ranks last.
__device__ __forceinline__ float fit_residual(const double *M, const Corr &c)
{
    const double w  = (M[6] * c.x + M[7] * c.y) + M[8];
    const double px = ((M[0] * c.x + M[1] * c.y) + M[2]) / w;
    const double py = ((M[3] * c.x + M[4] * c.y) + M[5]) / w;
    const double dx = px - c.X, dy = py - c.Y;
    const float r = (float)(dx * dx + dy * dy);
    return r <= 3.402823466e38f ? r : __uint_as_float(0x7f800000u);
}

struct FitGate {
    double m[9];
    float thr;
    int on;
};

__device__ __forceinline__ bool fit_pass(const FitGate &G, const Corr &c) { return !G.on || fit_residual(G.m, c) <= G.thr; }

// ----------------------------------------------------------------------------- float64 sums
enum { FIT_MOMENTS = 0, FIT_DLT = 1, FIT_GN = 2 };
constexpr int kSumsMoments = 16, kSumsDlt = 47, kSumsGn = 47, kSumsMax = 47;

struct FitSumArgs {
    FitField f;
    FitGate g;
    double norm[6];       // moments: origin (ox, oy); dlt / gn: cx, cy, s, cX, cY, S
    double model[9];      // gn: the homography in normalised coordinates
};

template <int KIND> struct FitSums;
template <> struct FitSums<FIT_MOMENTS> { static constexpr int S = kSumsMoments; };
template <> struct FitSums<FIT_DLT>     { static constexpr int S = kSumsDlt; };
template <> struct FitSums<FIT_GN>      { static constexpr int S = kSumsGn; };

template <int KIND>
__device__ __forceinline__ void fit_terms(const FitSumArgs &P, const Corr &c, double *acc)
{
    if (KIND == FIT_MOMENTS) {
        const double v[5] = {c.x - P.norm[0], c.y - P.norm[1], c.X - P.norm[0], c.Y - P.norm[1], 1.0};
        int t = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = i; j < 5; ++j) acc[t++] += v[i] * v[j];
    } else {
        const double x = (c.x - P.norm[0]) * P.norm[2], y = (c.y - P.norm[1]) * P.norm[2];
        const double X = (c.X - P.norm[3]) * P.norm[5], Y = (c.Y - P.norm[4]) * P.norm[5];
        if (KIND == FIT_DLT) {
            const double a1[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -(X * x), -(X * y), -X};
            const double a2[9] = {0.0, 0.0, 0.0, x, y, 1.0, -(Y * x), -(Y * y), -Y};
            int t = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j) acc[t++] += a1[i] * a1[j] + a2[i] * a2[j];
            acc[45] += 1.0;
        } else {
            const double *h = P.model;
            const double w  = (h[6] * x + h[7] * y) + h[8];
            const double px = ((h[0] * x + h[1] * y) + h[2]) / w;
            const double py = ((h[3] * x + h[4] * y) + h[5]) / w;
            const double rx = px - X, ry = py - Y;
            const double xw = x / w, yw = y / w, iw = 1.0 / w;
            const double j1[8] = {xw, yw, iw, 0.0, 0.0, 0.0, -(x * px) / w, -(y * px) / w};
            const double j2[8] = {0.0, 0.0, 0.0, xw, yw, iw, -(x * py) / w, -(y * py) / w};
            int t = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = i; j < 8; ++j) acc[t++] += j1[i] * j1[j] + j2[i] * j2[j];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[36 + i] += j1[i] * rx + j2[i] * ry;
            acc[44] += rx * rx + ry * ry;
            acc[45] += 1.0;
        }
    }
}

// One chunk per workgroup.  Per thread: its <= 16 (+ 3 tail) terms in pixel order; per wave: a six-level xor butterfly
// (a + b == b + a, so every lane holds the same bits); per workgroup: ((w0 + w1) + w2) + w3 -> partial[chunk][s].
template <int KIND, int WIDE>
__global__ __launch_bounds__(256)
void fit_sum_kernel(FitSumArgs P, double *__restrict__ partial)
{
    constexpr int S = FitSums<KIND>::S;
    __shared__ double wsum[4][S];
    double acc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = 0.0;
    auto take = [&](int x, int y, float u, float v) {
        Corr c;
        if (!fit_corr(P.f.sign, x, y, u, v, c)) { acc[S - 1] += 1.0; return; }
        if (fit_pass(P.g, c)) fit_terms<KIND>(P, c, acc);
    };
    FitTile T;
    fit_load<WIDE>(P.f, blockIdx.x, T);
    fit_each(P.f, T, take);
    fit_tail(P.f, blockIdx.x, take);
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[s] += __shfl_xor(acc[s], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < S; ++s) wsum[threadIdx.x >> 6][s] = acc[s];
    }
    __syncthreads();
    if (threadIdx.x < S)
        partial[(size_t)blockIdx.x * S + threadIdx.x] =
            ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
}

// out[s] = (((p[0][s] + p[1][s]) + p[2][s]) + ...): one thread per sum, chunks in order
__global__ void fit_finish_kernel(const double *__restrict__ partial, uint32_t chunks, int S, double *__restrict__ out)
{
    const int s = threadIdx.x;
    if (s >= S) return;
    double v = 0.0;
    uint32_t b = 0;
    for (; b + 16 <= chunks; b += 16) {              // sixteen loads in flight, added in the same order
        double t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = partial[(size_t)(b + k) * S + s];
#pragma unroll
        for (int k = 0; k < 16; ++k) v += t[k];
    }
    for (; b < chunks; ++b) v += partial[(size_t)b * S + s];
    out[s] = v;
}

// ----------------------------------------------------------------------------- score: K inlier counts
constexpr int kScoreMax = 32;
struct FitModels { double m[kScoreMax][9]; };

template <int WIDE>
__global__ __launch_bounds__(256)
void fit_score_kernel(FitField A, FitModels M, int K, float thr, uint32_t chunks, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t lc[kScoreMax];
    if (threadIdx.x < kScoreMax) lc[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        FitTile T;
        fit_load<WIDE>(A, chunk, T);
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const double *Mk = M.m[k];
            uint32_t c = 0;
            auto take = [&](int x, int y, float u, float v) {
                Corr cr;
                if (fit_corr(A.sign, x, y, u, v, cr) && fit_residual(Mk, cr) <= thr) ++c;
            };
            fit_each(A, T, take);
            fit_tail(A, chunk, take);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off);
            if ((threadIdx.x & 63) == 0 && c) atomicAdd(&lc[k], c);
        }
    }
    __syncthreads();
    if (threadIdx.x < K && lc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], lc[threadIdx.x]);
}

// ----------------------------------------------------------------------------- median: radix select over the residual bits
// Digits 11 / 11 / 10, most significant first; residuals are >= 0 (or +Inf), so their bits sort as uint32.
constexpr int kBins = 2048;
constexpr int kStateWords = 16;                          // per model: prefix lo, prefix hi, rank lo, rank hi, pad
constexpr int kModelWords = 2 * kBins + kStateWords;     // two histograms (ranks lo, hi) + state
constexpr int kMedModels = 3;                            // models per launch: 3 x 2 x 8 KiB of LDS histograms
struct FitModels3 { double m[kMedModels][9]; };

__device__ __forceinline__ int fit_digit_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }

// a lane's run of equal bins costs one LDS atomic
struct FitRun {
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

__global__ void fit_med_init_kernel(uint32_t *__restrict__ ws, uint32_t lo, uint32_t hi)
{
    uint32_t *mw = ws + (size_t)blockIdx.x * kModelWords;
    for (int i = threadIdx.x; i < kModelWords; i += blockDim.x) {
        uint32_t v = 0;
        if (i == 2 * kBins + 2) v = lo;
        if (i == 2 * kBins + 3) v = hi;
        mw[i] = v;
    }
}

// One pass for nm models: LDS histograms of this pass's digit over the residuals whose higher digits equal the prefix of
// rank lo (histogram 0) or of rank hi (histogram 1, only while the prefixes differ), merged with one atomic per used bin.
template <int WIDE>
__global__ __launch_bounds__(256)
void fit_med_hist_kernel(FitField A, FitModels3 M, int nm, int pass, uint32_t chunks, uint32_t *__restrict__ ws)
{
    __shared__ uint32_t h[kMedModels][2][kBins];
    for (int i = threadIdx.x; i < kMedModels * 2 * kBins; i += 256) (&h[0][0][0])[i] = 0;
    __syncthreads();
    const int shift = fit_digit_shift(pass), pshift = pass == 1 ? 21 : 10;
    const uint32_t dmask = pass == 2 ? 0x3ffu : 0x7ffu;
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        FitTile T;
        fit_load<WIDE>(A, chunk, T);
#pragma unroll 1
        for (int k = 0; k < nm; ++k) {
            const uint32_t *st = ws + (size_t)k * kModelWords + 2 * kBins;
            const uint32_t pl = st[0], ph = st[1];
            const bool same = pl == ph;
            const double *Mk = M.m[k];
            uint32_t *h0 = h[k][0], *h1 = h[k][1];
            FitRun r0, r1;
            auto take = [&](int x, int y, float u, float v) {
                Corr c;
                if (!fit_corr(A.sign, x, y, u, v, c)) return;
                const uint32_t key = __float_as_uint(fit_residual(Mk, c));
                if (pass == 0) {
                    r0.add(h0, key >> 21);
                } else {
                    const uint32_t p = key >> pshift, d = (key >> shift) & dmask;
                    if (p == pl) r0.add(h0, d);
                    if (!same && p == ph) r1.add(h1, d);
                }
            };
            fit_each(A, T, take);
            fit_tail(A, chunk, take);
            r0.flush(h0);
            r1.flush(h1);
        }
    }
    __syncthreads();
    for (int k = 0; k < nm; ++k) {
        uint32_t *g = ws + (size_t)k * kModelWords;
        for (int b = threadIdx.x; b < kBins; b += 256) {
            if (h[k][0][b]) atomicAdd(&g[b], h[k][0][b]);
            if (h[k][1][b]) atomicAdd(&g[kBins + b], h[k][1][b]);
        }
    }
}

// exclusive scan of one value per thread over a 256-thread workgroup
__device__ __forceinline__ uint32_t fit_block_scan(uint32_t v, uint32_t *wave_tot)
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

// The bin of each rank: prefix <- prefix * bins + digit, rank <- rank - count before the bin; histograms zeroed for the
// next pass.  The last pass writes the two residuals' bits to out[2 * model], out[2 * model + 1].  grid = models.
__global__ __launch_bounds__(256)
void fit_med_select_kernel(uint32_t *__restrict__ ws, int pass, uint32_t *__restrict__ out)
{
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t res[4];
    uint32_t *mw = ws + (size_t)blockIdx.x * kModelWords;
    uint32_t *st = mw + 2 * kBins;
    const uint32_t pl = st[0], ph = st[1], rl = st[2], rh = st[3];
    const bool same = pl == ph;
    const int nb = pass == 2 ? 1024 : 2048, per = nb / 256, bits = pass == 2 ? 10 : 11;
    if (threadIdx.x == 0) { res[0] = pl << bits; res[1] = ph << bits; res[2] = rl; res[3] = rh; }
    __syncthreads();
    for (int t = 0; t < 2; ++t) {
        const uint32_t *hist = mw + ((t == 1 && !same) ? kBins : 0);
        const uint32_t k = t ? rh : rl;
        const int b0 = threadIdx.x * per;
        uint32_t sum = 0;
        for (int j = 0; j < per; ++j) sum += hist[b0 + j];
        uint32_t before = fit_block_scan(sum, wave_tot);
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
    for (int i = threadIdx.x; i < 2 * kBins; i += 256) mw[i] = 0;
    if (threadIdx.x == 0) {
        st[0] = res[0]; st[1] = res[1]; st[2] = res[2]; st[3] = res[3];
        if (pass == 2) { out[2 * blockIdx.x] = res[0]; out[2 * blockIdx.x + 1] = res[1]; }
    }
}

// ----------------------------------------------------------------------------- sampling: valid pixels by rank, gather
// A pixel is valid when its mask byte is not 0 and its vector is finite.  The index is the exclusive scan of the valid
// counts of consecutive 4096-px ranges: scan[0 .. ranges], scan[ranges] = all valid pixels.
__device__ __forceinline__ bool fit_valid(const FitField &A, uint32_t p)
{
    if (A.mask && !A.mask[p]) return false;
    const float2 f = reinterpret_cast<const float2 *>(A.flow)[p];
    return fit_finite(f.x, f.y);
}

__global__ __launch_bounds__(256)
void fit_count_kernel(FitField A, uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    uint32_t c = 0;
    for (int j = 0; j < (int)(kFitChunk / 256); ++j) {
        const uint64_t p = (uint64_t)blockIdx.x * kFitChunk + (uint32_t)j * 256 + threadIdx.x;
        if (p < A.n && fit_valid(A, (uint32_t)p)) ++c;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&tot, c);
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256)
void fit_scan_kernel(const uint32_t *__restrict__ cnt, uint32_t ranges, uint32_t *__restrict__ scan)
{
    __shared__ uint32_t wave_tot[4];
    const uint32_t per = (ranges + 255) / 256, b0 = threadIdx.x * per, b1 = min(b0 + per, ranges);
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; ++b) sum += cnt[b];
    uint32_t before = fit_block_scan(sum, wave_tot);
    for (uint32_t b = b0; b < b1; ++b) { scan[b] = before; before += cnt[b]; }
    if (b0 < ranges && b1 == ranges) scan[ranges] = before;
}

// idx[q] = the pixel index of the ranks[q]-th valid pixel (row-major order), 0xffffffff when there are fewer
__global__ void fit_pick_kernel(FitField A, const uint32_t *__restrict__ scan, uint32_t ranges, const uint32_t *__restrict__ ranks,
                                uint32_t count, uint32_t *__restrict__ idx)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    uint32_t r = ranks[q], found = 0xffffffffu;
    if (r < scan[ranges]) {
        uint32_t lo = 0, hi = ranges - 1;                 // the last range with scan[range] <= r
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) / 2;
            if (scan[mid] <= r) lo = mid; else hi = mid - 1;
        }
        r -= scan[lo];
        const uint64_t p0 = (uint64_t)lo * kFitChunk, p1 = p0 + kFitChunk < A.n ? p0 + kFitChunk : (uint64_t)A.n;
        for (uint64_t p = p0; p < p1; ++p) {
            if (!fit_valid(A, (uint32_t)p)) continue;
            if (r == 0) { found = (uint32_t)p; break; }
            --r;
        }
    }
    idx[q] = found;
}

// out[q] = { idx, bits of u, bits of v, mask byte } -- { idx, 0, 0, 0 } for an index outside the field
__global__ void fit_gather_kernel(FitField A, const uint32_t *__restrict__ idx, uint32_t count, uint32_t *__restrict__ out)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    const uint32_t p = idx[q];
    uint4 o = make_uint4(p, 0u, 0u, 0u);
    if (p < A.n) {
        const float2 f = reinterpret_cast<const float2 *>(A.flow)[p];
        o.y = __float_as_uint(f.x);
        o.z = __float_as_uint(f.y);
        o.w = A.mask ? (uint32_t)A.mask[p] : 1u;
    }
    reinterpret_cast<uint4 *>(out)[q] = o;
}

// ----------------------------------------------------------------------------- host side
struct FitLayout {
    uint32_t chunks, ranges;
    size_t partial_off, med_off, cnt_off, scan_off, bytes;
};

FitLayout fit_layout(size_t n)
{
    FitLayout L;
    L.chunks = fit_chunks(n);
    L.ranges = (uint32_t)((n + kFitChunk - 1) / kFitChunk);
    L.partial_off = 0;
    L.med_off = (size_t)L.chunks * kSumsMax * sizeof(double);
    L.cnt_off = L.med_off + (size_t)kMedModels * kModelWords * sizeof(uint32_t);
    L.scan_off = L.cnt_off + (((size_t)L.ranges * sizeof(uint32_t) + 15) & ~(size_t)15);
    L.bytes = L.scan_off + ((((size_t)L.ranges + 1) * sizeof(uint32_t) + 15) & ~(size_t)15);
    return L;
}

// wide: vectors on the 16-byte and mask on the 4-byte grid, what the float4 / mask-word loads of fit_load<1> need; the
// sampling kernels (count, pick, gather) load 8-byte vectors and mask bytes in either case
int fit_field(const char *who, const float *flow, const uint8_t *mask, int H, int W, int sign, FitField &A, bool *wide = nullptr)
{
    if (!flow || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "%s: bad arguments", who);
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "%s: sign must be +1 or -1", who);
    if ((size_t)H * W > 0x7fffffffu) return fail(OFL_E_INVALID, "%s: fields of more than 2^31 - 1 px are not supported", who);
    if (reinterpret_cast<uintptr_t>(flow) & 7) return fail(OFL_E_INVALID, "%s: flow must be 8-byte aligned", who);
    if (wide) *wide = !(reinterpret_cast<uintptr_t>(flow) & 15) && !(reinterpret_cast<uintptr_t>(mask) & 3);
    A.flow = flow; A.mask = mask; A.n = (uint32_t)((size_t)H * W); A.W = W; A.sign = sign;
    return OFL_OK;
}

int fit_gate(const char *who, const double *gate_model, float gate_thr, FitGate &G)
{
    G.on = gate_model ? 1 : 0;
    G.thr = gate_thr;
    for (int i = 0; i < 9; ++i) G.m[i] = gate_model ? gate_model[i] : 0.0;
    if (gate_model && !(gate_thr >= 0.0f)) return fail(OFL_E_INVALID, "%s: the gate threshold must be >= 0", who);
    return OFL_OK;
}

template <int KIND>
int fit_sums(const char *who, const float *flow, const uint8_t *mask, int H, int W, int sign, const double *norm, int n_norm,
             const double *model, const double *gate_model, float gate_thr, void *workspace, size_t workspace_bytes,
             double *out, void *stream)
{
    OFL_TRY(need_device());
    FitSumArgs P;
    bool wide;
    OFL_TRY(fit_field(who, flow, mask, H, W, sign, P.f, &wide));
    OFL_TRY(fit_gate(who, gate_model, gate_thr, P.g));
    if (!norm || !out || !workspace || (KIND == FIT_GN && !model)) return fail(OFL_E_INVALID, "%s: NULL pointer", who);
    const FitLayout L = fit_layout(P.f.n);
    if (workspace_bytes < L.bytes) return fail(OFL_E_INVALID, "%s: workspace of %zu bytes is too small", who, workspace_bytes);
    for (int i = 0; i < 6; ++i) P.norm[i] = i < n_norm ? norm[i] : 0.0;
    for (int i = 0; i < 9; ++i) P.model[i] = model ? model[i] : 0.0;
    hipStream_t s = stream_of(stream);
    double *partial = reinterpret_cast<double *>((char *)workspace + L.partial_off);
    if (wide) hipLaunchKernelGGL((fit_sum_kernel<KIND, 1>), dim3(L.chunks), dim3(256), 0, s, P, partial);
    else      hipLaunchKernelGGL((fit_sum_kernel<KIND, 0>), dim3(L.chunks), dim3(256), 0, s, P, partial);
    hipLaunchKernelGGL(fit_finish_kernel, dim3(1), dim3(64), 0, s, (const double *)partial, L.chunks, FitSums<KIND>::S, out);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

unsigned fit_stream_grid(uint32_t chunks, uint32_t per_block)
{
    return (unsigned)std::max<uint32_t>(1, (chunks + per_block - 1) / per_block);
}

}  // namespace

extern "C" {

int ofl_fit_workspace_bytes(int H, int W, size_t *bytes)
{
    if (!bytes || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_fit_workspace_bytes: bad arguments");
    *bytes = fit_layout((size_t)H * W).bytes;
    return OFL_OK;
}

int ofl_fit_moments_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *origin,
                        const double *gate_model, float gate_thr, void *workspace, size_t workspace_bytes,
                        double *sums, void *stream)
{
    return fit_sums<FIT_MOMENTS>("ofl_fit_moments", flow, mask, H, W, sign, origin, 2, nullptr, gate_model, gate_thr,
                                 workspace, workspace_bytes, sums, stream);
}

int ofl_fit_dlt_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *norm,
                    const double *gate_model, float gate_thr, void *workspace, size_t workspace_bytes,
                    double *sums, void *stream)
{
    return fit_sums<FIT_DLT>("ofl_fit_dlt", flow, mask, H, W, sign, norm, 6, nullptr, gate_model, gate_thr,
                             workspace, workspace_bytes, sums, stream);
}

int ofl_fit_gn_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *norm, const double *model,
                   const double *gate_model, float gate_thr, void *workspace, size_t workspace_bytes,
                   double *sums, void *stream)
{
    return fit_sums<FIT_GN>("ofl_fit_gn", flow, mask, H, W, sign, norm, 6, model, gate_model, gate_thr,
                            workspace, workspace_bytes, sums, stream);
}

int ofl_fit_score_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *models, int K,
                      float thr, uint32_t *counts, void *stream)
{
    OFL_TRY(need_device());
    FitField A;
    bool wide;
    OFL_TRY(fit_field("ofl_fit_score", flow, mask, H, W, sign, A, &wide));
    if (!models || !counts || K < 1 || K > kScoreMax) return fail(OFL_E_INVALID, "ofl_fit_score: K must be in [1, %d]", kScoreMax);
    FitModels M;
    memset(&M, 0, sizeof(M));
    memcpy(M.m, models, (size_t)K * 9 * sizeof(double));
    hipStream_t s = stream_of(stream);
    OFL_HIP(hipMemsetAsync(counts, 0, (size_t)K * sizeof(uint32_t), s));
    const uint32_t chunks = fit_chunks(A.n);
    const dim3 grid(fit_stream_grid(chunks, 2)), block(256);
    if (wide) hipLaunchKernelGGL((fit_score_kernel<1>), grid, block, 0, s, A, M, K, thr, chunks, counts);
    else      hipLaunchKernelGGL((fit_score_kernel<0>), grid, block, 0, s, A, M, K, thr, chunks, counts);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_fit_median_dev(const float *flow, const uint8_t *mask, int H, int W, int sign, const double *models, int K,
                       size_t rank_lo, size_t rank_hi, void *workspace, size_t workspace_bytes, uint32_t *out, void *stream)
{
    OFL_TRY(need_device());
    FitField A;
    bool wide;
    OFL_TRY(fit_field("ofl_fit_median", flow, mask, H, W, sign, A, &wide));
    if (!models || !out || !workspace || K < 1) return fail(OFL_E_INVALID, "ofl_fit_median: bad arguments");
    if (rank_lo > rank_hi || rank_hi >= A.n) return fail(OFL_E_INVALID, "ofl_fit_median: ranks %zu, %zu outside a field of %u px", rank_lo, rank_hi, A.n);
    const FitLayout L = fit_layout(A.n);
    if (workspace_bytes < L.bytes) return fail(OFL_E_INVALID, "ofl_fit_median: workspace of %zu bytes is too small", workspace_bytes);
    hipStream_t s = stream_of(stream);
    uint32_t *ws = reinterpret_cast<uint32_t *>((char *)workspace + L.med_off);
    const unsigned grid = fit_stream_grid(L.chunks, 4);
    for (int k0 = 0; k0 < K; k0 += kMedModels) {
        const int nm = std::min(kMedModels, K - k0);
        FitModels3 M;
        memset(&M, 0, sizeof(M));
        memcpy(M.m, models + (size_t)k0 * 9, (size_t)nm * 9 * sizeof(double));
        hipLaunchKernelGGL(fit_med_init_kernel, dim3(nm), dim3(256), 0, s, ws, (uint32_t)rank_lo, (uint32_t)rank_hi);
        for (int pass = 0; pass < 3; ++pass) {
            if (wide) hipLaunchKernelGGL((fit_med_hist_kernel<1>), dim3(grid), dim3(256), 0, s, A, M, nm, pass, L.chunks, ws);
            else      hipLaunchKernelGGL((fit_med_hist_kernel<0>), dim3(grid), dim3(256), 0, s, A, M, nm, pass, L.chunks, ws);
            hipLaunchKernelGGL(fit_med_select_kernel, dim3(nm), dim3(256), 0, s, ws, pass, out + 2 * (size_t)k0);
        }
    }
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_fit_index_dev(const float *flow, const uint8_t *mask, int H, int W, void *workspace, size_t workspace_bytes, void *stream)
{
    OFL_TRY(need_device());
    FitField A;
    OFL_TRY(fit_field("ofl_fit_index", flow, mask, H, W, 1, A));
    const FitLayout L = fit_layout(A.n);
    if (!workspace || workspace_bytes < L.bytes) return fail(OFL_E_INVALID, "ofl_fit_index: workspace of %zu bytes is too small", workspace_bytes);
    hipStream_t s = stream_of(stream);
    uint32_t *cnt = reinterpret_cast<uint32_t *>((char *)workspace + L.cnt_off);
    uint32_t *scan = reinterpret_cast<uint32_t *>((char *)workspace + L.scan_off);
    hipLaunchKernelGGL(fit_count_kernel, dim3(L.ranges), dim3(256), 0, s, A, cnt);
    hipLaunchKernelGGL(fit_scan_kernel, dim3(1), dim3(256), 0, s, (const uint32_t *)cnt, L.ranges, scan);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_fit_pick_dev(const float *flow, const uint8_t *mask, int H, int W, const void *workspace, size_t workspace_bytes,
                     const uint32_t *ranks, size_t count, uint32_t *idx, void *stream)
{
    OFL_TRY(need_device());
    FitField A;
    OFL_TRY(fit_field("ofl_fit_pick", flow, mask, H, W, 1, A));
    const FitLayout L = fit_layout(A.n);
    if (!workspace || workspace_bytes < L.bytes) return fail(OFL_E_INVALID, "ofl_fit_pick: workspace of %zu bytes is too small", workspace_bytes);
    if (!ranks || !idx || count > 0x7fffffffu) return fail(OFL_E_INVALID, "ofl_fit_pick: bad arguments");
    if (count == 0) return OFL_OK;
    const uint32_t *scan = reinterpret_cast<const uint32_t *>((const char *)workspace + L.scan_off);
    hipLaunchKernelGGL(fit_pick_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, stream_of(stream), A, scan, L.ranges, ranks,
                       (uint32_t)count, idx);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_fit_gather_dev(const float *flow, const uint8_t *mask, int H, int W, const uint32_t *idx, size_t count,
                       uint32_t *out, void *stream)
{
    OFL_TRY(need_device());
    FitField A;
    OFL_TRY(fit_field("ofl_fit_gather", flow, mask, H, W, 1, A));
    if (!idx || !out || count > 0x7fffffffu || (reinterpret_cast<uintptr_t>(out) & 15))
        return fail(OFL_E_INVALID, "ofl_fit_gather: bad arguments (out must be 16-byte aligned)");
    if (count == 0) return OFL_OK;
    hipLaunchKernelGGL(fit_gather_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, stream_of(stream), A, idx, (uint32_t)count, out);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

}  // extern "C"
