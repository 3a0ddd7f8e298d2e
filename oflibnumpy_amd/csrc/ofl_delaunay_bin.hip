// ofl_delaunay_bin.hip -- K3 exact path, binning (the map of the path: ofl_delaunay.hip): bounding box and grid parameters,
// the counting sorts of the kept points (fine buckets) and of the unfinished points (coarse buckets), the scans, the
// removal of exact duplicates, the grids of dense clusters, and the ordered compaction that makes every list of the path.
#include "ofl_delaunay_dev.h"

using namespace ofl;
using namespace ofl_sc;
using namespace ofl_dl;
using namespace ofl_dlw;

namespace {

// a point with a NaN / Inf position cannot be a site (the reference's Flow refuses such vectors; behind the bare C ABI they
// are dropped like masked-out points instead of sending bucket indices out of range)
__device__ __forceinline__ bool finite_pt(double x, double y) { return isfinite(x) && isfinite(y); }

// exclusive scan of one value per thread over a 256-thread block; `total` = block sum (valid in all threads)
__device__ __forceinline__ unsigned block_exscan(unsigned v, unsigned &total)
{
    __shared__ unsigned s_w[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, off);
        if (lane >= off) inc += t;
    }
    __syncthreads();
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int k = 0; k < w; ++k) base += s_w[k];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return base + inc - v;
}

// ------------------------------------------------------------------------------------------------ binning
__global__ __launch_bounds__(256)
void dl_bbox_kernel(const float *__restrict__ flow, int sign, const uint8_t *__restrict__ pmask, int H, int W,
                    unsigned long long *__restrict__ partial)      // [workgroups][5]: keys of min x, max x, min y, max y; points kept
{
    const int x = blockIdx.x * 32 + (threadIdx.x & 31);
    double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
    unsigned cnt = 0;
    if (x < W)
        for (int y = blockIdx.y * 8 + (threadIdx.x >> 5); y < H; y += gridDim.y * 8) {
            if (!kept_pt(pmask, (size_t)y * W + x)) continue;
            const D2 p = point_of(flow, sign, W, x, y);
            if (!finite_pt(p.x, p.y)) continue;
            x0 = fmin(x0, p.x); x1 = fmax(x1, p.x); y0 = fmin(y0, p.y); y1 = fmax(y1, p.y);
            ++cnt;
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        x0 = fmin(x0, __hiloint2double(__shfl_xor(__double2hiint(x0), off), __shfl_xor(__double2loint(x0), off)));
        x1 = fmax(x1, __hiloint2double(__shfl_xor(__double2hiint(x1), off), __shfl_xor(__double2loint(x1), off)));
        y0 = fmin(y0, __hiloint2double(__shfl_xor(__double2hiint(y0), off), __shfl_xor(__double2loint(y0), off)));
        y1 = fmax(y1, __hiloint2double(__shfl_xor(__double2hiint(y1), off), __shfl_xor(__double2loint(y1), off)));
        cnt += (unsigned)__shfl_xor((int)cnt, off);
    }
    // One record per workgroup, reduced by dl_params_kernel.  (Atomics on the header -- five per workgroup, then one set per
    // workgroup -- are executed one after the other at the memory side: a thousand workgroups spent 50 of this kernel's 67 us
    // at 4K queueing for ONE cache line, and twice the workgroups took twice as long.)
    __shared__ double s_b[4][4];
    __shared__ unsigned s_c[4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_b[0][w] = x0; s_b[1][w] = x1; s_b[2][w] = y0; s_b[3][w] = y1; s_c[w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0;
        for (int k = 0; k < 4; ++k) { x0 = fmin(x0, s_b[0][k]); x1 = fmax(x1, s_b[1][k]); y0 = fmin(y0, s_b[2][k]); y1 = fmax(y1, s_b[3][k]); c += s_c[k]; }
        unsigned long long *rec = partial + 5 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        rec[0] = c ? okey(x0) : ~0ull; rec[1] = c ? okey(x1) : 0ull; rec[2] = c ? okey(y0) : ~0ull; rec[3] = c ? okey(y1) : 0ull; rec[4] = c;
    }
}

__global__ __launch_bounds__(256)
void dl_params_kernel(DlHead *head, unsigned long long bcap, int H, int W, int slab, int row0, int rows,
                      const unsigned long long *__restrict__ partial, unsigned n_partial)
{
    {   // the bounding box and the number of kept points from dl_bbox_kernel's records
        unsigned long long k0 = ~0ull, k1 = 0ull, k2 = ~0ull, k3 = 0ull, c = 0ull;
        for (unsigned i = threadIdx.x; i < n_partial; i += 256) {
            const unsigned long long *rec = partial + 5 * (size_t)i;
            k0 = rec[0] < k0 ? rec[0] : k0; k1 = rec[1] > k1 ? rec[1] : k1;
            k2 = rec[2] < k2 ? rec[2] : k2; k3 = rec[3] > k3 ? rec[3] : k3; c += rec[4];
        }
        __shared__ unsigned long long s_k[5][256];
        s_k[0][threadIdx.x] = k0; s_k[1][threadIdx.x] = k1; s_k[2][threadIdx.x] = k2; s_k[3][threadIdx.x] = k3; s_k[4][threadIdx.x] = c;
        __syncthreads();
        for (int half = 128; half > 0; half >>= 1) {
            if ((int)threadIdx.x < half) {
                const int t = threadIdx.x, u = t + half;
                s_k[0][t] = s_k[0][u] < s_k[0][t] ? s_k[0][u] : s_k[0][t]; s_k[1][t] = s_k[1][u] > s_k[1][t] ? s_k[1][u] : s_k[1][t];
                s_k[2][t] = s_k[2][u] < s_k[2][t] ? s_k[2][u] : s_k[2][t]; s_k[3][t] = s_k[3][u] > s_k[3][t] ? s_k[3][u] : s_k[3][t];
                s_k[4][t] += s_k[4][u];
            }
            __syncthreads();
        }
        if (threadIdx.x != 0) return;
        k0 = s_k[0][0]; k1 = s_k[1][0]; k2 = s_k[2][0]; k3 = s_k[3][0]; c = s_k[4][0];
        head->kx0 = k0; head->kx1 = k1; head->ky0 = k2; head->ky1 = k3; head->kept = (unsigned)c;
    }
    Grid g;
    g.ox = 0.0; g.oy = 0.0; g.s = 1.0; g.inv_s = 1.0; g.gx = 1; g.gy = 1;
    const unsigned n = head->kept;
    if (n > 0) {
        double x0 = okey_inv(head->kx0), x1 = okey_inv(head->kx1), y0 = okey_inv(head->ky0), y1 = okey_inv(head->ky1);
        // The grid covers at most the image and a margin of W + H around it: a handful of garbage vectors (1e9 marks
        // "unknown" in some flow files) must not blow the buckets up to thousands of sites each.  Sites beyond it fall
        // into the border buckets (Grid::bx / by clamp) -- seen from any site inside, such a site is at least as far away
        // as its bucket, which is all the ring searches rely on; the outliers themselves never close within the rings and
        // end in the passes that run until the candidates are exhausted.
        const double m = (double)W + (double)H;
        x0 = fmax(x0, fmin(-m, x1 - 1.0)); x1 = fmin(x1, fmax((double)W + m, x0 + 1.0));
        y0 = fmax(y0, fmin(-m, y1 - 1.0)); y1 = fmin(y1, fmax((double)H + m, y0 + 1.0));
        const double bw = x1 - x0, bh = y1 - y0;
        // every point on one spot or on one axis-parallel line: nothing to triangulate (Qhull: "initial simplex is flat")
        if (n >= 3 && (!(okey_inv(head->kx1) > okey_inv(head->kx0)) || !(okey_inv(head->ky1) > okey_inv(head->ky0)))) atomicOr(&head->err, kErrDegenerate);
        double s = sqrt(fmax(bw * bh, 1e-300) / (double)n);             // ~1 point per bucket
        s = fmax(s, (bw + bh) / (double)n);
        if (!(s > 0.0) || !isfinite(s)) s = 1.0;
        for (int it = 0; it < 64; ++it) {
            const double fx = floor(bw / s) + 1.0, fy = floor(bh / s) + 1.0;
            if (fx * fy <= (double)bcap && fx < 2e9 && fy < 2e9) break;
            s *= 1.5;
        }
        g.ox = x0; g.oy = y0; g.s = s; g.inv_s = 1.0 / s;
        g.gx = (int)(floor(bw / s) + 1.0); g.gy = (int)(floor(bh / s) + 1.0);
        // Cell vertices farther than this from their site count as FAR: they are excluded by the cone they lie in rather than by
        // the reach of the near ones.  A straight border that float32 leaves 1e-5 px rough has sliver triangles with
        // circumcentres 1e4 px out, a wavy one (3 px over 100 px) 400 - 4 000 px out: as near vertices their reach covers every
        // candidate of the left-over sweep.  kFarBuckets point spacings (never more than the data's own extent) is where the
        // rim of a hole -- whose cells do reach that far, in all directions -- still pays nothing for it.
        const double t = fmin(kFarBuckets * s, 1.5 * (bw + bh) + 8.0 * s);
        head->far_t2 = t * t;
    } else head->far_t2 = 1.0;
    head->grid = g;
    // slab mode: stars from cells / fans / clip only within kSlabMargin buckets of the band's rows (the first and the last
    // band of a field are open-ended: sites warp beyond the frame)
    const double inf = __longlong_as_double(0x7FF0000000000000ll), m = (double)kSlabMargin * g.s;
    head->need_lo = (!slab || row0 <= 0) ? -inf : (double)row0 - m;
    head->need_hi = (!slab || row0 + rows >= H) ? inf : (double)(row0 + rows - 1) + m;
    // (sites beyond the grid are clamped into its border buckets: a star next to those may hold a neighbour that is "within
    // the rings" by bucket number only -- a slab that comes this close to the border rows takes everything beyond them, too)
    if (head->need_lo < g.oy + (double)(kRings + 2) * g.s) head->need_lo = -inf;
    if (head->need_hi > g.oy + (double)(g.gy - kRings - 2) * g.s) head->need_hi = inf;
    head->slab_stamp = slab ? slab_stamp_of(H, W, row0, rows) : 0u;
    Grid g1 = g;                                     // coarse grid of the unfinished points: kMidScale fine buckets per cell
    g1.s = g.s * kMidScale; g1.inv_s = 1.0 / g1.s;
    g1.gx = (g.gx + kMidScale - 1) / kMidScale; g1.gy = (g.gy + kMidScale - 1) / kMidScale;
    head->grid1 = g1;
}

// the same three binning steps for the unfinished points (ranks into far_idx) on the coarse grid
__global__ __launch_bounds__(256)
void dl_count1_kernel(const float *__restrict__ flow, int sign, int W, const DlHead *__restrict__ head,
                      const unsigned *__restrict__ far_idx, unsigned *__restrict__ bcount)
{
    const Grid g = head->grid1;
    for (unsigned r = blockIdx.x * 256 + threadIdx.x; r < head->n_far; r += gridDim.x * 256) {      // (sized on the device: no read-back of the count)
        const P2 p = PosFn(flow, sign, W)((int)far_idx[r]);
        atomicAdd(&bcount[(size_t)g.by(p.y) * g.gx + g.bx(p.x)], 1u);
    }
}

__global__ __launch_bounds__(256)
void dl_fill1_kernel(const float *__restrict__ flow, int sign, int W, const DlHead *__restrict__ head,
                     const unsigned *__restrict__ far_idx, const unsigned *__restrict__ bstart,
                     unsigned *__restrict__ cursor, unsigned *__restrict__ sorted)
{
    const Grid g = head->grid1;
    for (unsigned r = blockIdx.x * 256 + threadIdx.x; r < head->n_far; r += gridDim.x * 256) {
        const P2 p = PosFn(flow, sign, W)((int)far_idx[r]);
        const size_t b = (size_t)g.by(p.y) * g.gx + g.bx(p.x);
        sorted[bstart[b] + atomicAdd(&cursor[b], 1u)] = r;
    }
}

__global__ __launch_bounds__(256)
void dl_count_kernel(const float *__restrict__ flow, int sign, const uint8_t *__restrict__ pmask, int H, int W,
                     const DlHead *__restrict__ head, unsigned *__restrict__ bcount, unsigned char *__restrict__ dup,
                     unsigned *__restrict__ slot)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W || !kept_pt(pmask, i)) return;
    const Grid g = head->grid;
    const P2 p = PosFn(flow, sign, W)((int)i);
    if (!finite_pt(p.x, p.y)) { dup[i] = 1; return; }      // not a site (flagged like a dropped duplicate)
    // the count a site draws is its slot in the bucket (any order will do: the buckets are sorted by index afterwards), so the
    // fill pass needs neither a second atomic per site nor a zeroed array of bucket cursors (265 MB at 8K)
    slot[i] = atomicAdd(&bcount[(size_t)g.by(p.y) * g.gx + g.bx(p.x)], 1u);
}

// exclusive scan in three launches: sums of 8192-element chunks, ONE workgroup scans up to 8192 of those sums in place,
// then every chunk is scanned with its offset (round 2 walked 2048-element levels: seven launches for the bucket counts of
// a 4K field, five for every compaction -- a dozen scans per call made 42 tiny launches)
constexpr int kScanBig = 8192;             // elements per block: 256 threads x 32

__global__ __launch_bounds__(256)
void dl_scan_reduce_kernel(const unsigned *__restrict__ in, size_t n, unsigned *__restrict__ sums)
{
    const size_t base = (size_t)blockIdx.x * kScanBig + (size_t)threadIdx.x * 32;
    unsigned v = 0;
    if (base + 32 <= n) {
        const uint4 *q = reinterpret_cast<const uint4 *>(in + base);
#pragma unroll
        for (int k = 0; k < 8; ++k) { const uint4 t = q[k]; v += t.x + t.y + t.z + t.w; }
    } else {
        for (int k = 0; k < 32; ++k) if (base + k < n) v += in[base + k];
    }
    unsigned total;
    (void)block_exscan(v, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256)
void dl_scan_apply_kernel(unsigned *__restrict__ data, size_t n, const unsigned *__restrict__ offsets)
{
    const size_t base = (size_t)blockIdx.x * kScanBig + (size_t)threadIdx.x * 32;
    unsigned e[32], v = 0;
    const bool whole = base + 32 <= n;
    if (whole) {
        const uint4 *q = reinterpret_cast<const uint4 *>(data + base);
#pragma unroll
        for (int k = 0; k < 8; ++k) { const uint4 t = q[k]; e[4 * k] = t.x; e[4 * k + 1] = t.y; e[4 * k + 2] = t.z; e[4 * k + 3] = t.w; }
    } else {
#pragma unroll
        for (int k = 0; k < 32; ++k) e[k] = base + k < n ? data[base + k] : 0u;
    }
#pragma unroll
    for (int k = 0; k < 32; ++k) v += e[k];
    unsigned total;
    unsigned run = block_exscan(v, total) + (offsets ? offsets[blockIdx.x] : 0u);
    if (whole) {
        uint4 *q = reinterpret_cast<uint4 *>(data + base);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uint4 t;
            t.x = run; run += e[4 * k]; t.y = run; run += e[4 * k + 1]; t.z = run; run += e[4 * k + 2]; t.w = run; run += e[4 * k + 3];
            q[k] = t;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 32; ++k) { if (base + k < n) data[base + k] = run; run += e[k]; }
    }
}

// one workgroup of 1024: in-place exclusive scan of up to 8192 values
__global__ __launch_bounds__(1024)
void dl_scan_small_kernel(unsigned *__restrict__ data, unsigned n)
{
    __shared__ unsigned s_w[16];
    const unsigned base = threadIdx.x * 8;
    unsigned e[8], v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { e[k] = base + k < n ? data[base + k] : 0u; v += e[k]; }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    unsigned run = inc - v;
    for (int k = 0; k < w; ++k) run += s_w[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) { if (base + k < n) data[base + k] = run; run += e[k]; }
}

__global__ __launch_bounds__(256)
void dl_fill_kernel(const float *__restrict__ flow, int sign, const uint8_t *__restrict__ pmask, int H, int W,
                    const DlHead *__restrict__ head, const unsigned *__restrict__ bstart, const unsigned *__restrict__ slot,
                    unsigned *__restrict__ sorted, const unsigned char *__restrict__ dup)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W || !kept_pt(pmask, i) || dup[i]) return;
    const Grid g = head->grid;
    const P2 p = PosFn(flow, sign, W)((int)i);
    const size_t b = (size_t)g.by(p.y) * g.gx + g.bx(p.x);
    sorted[bstart[b] + slot[i]] = (unsigned)i;
}

// ascending point index inside every bucket (the fill order is not deterministic)
__global__ __launch_bounds__(256)
void dl_sort_kernel(const DlHead *__restrict__ head, int coarse, const unsigned *__restrict__ bstart, unsigned *__restrict__ sorted)
{
    const size_t nb = coarse ? (size_t)head->grid1.gx * head->grid1.gy : (size_t)head->grid.gx * head->grid.gy;
    for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < nb; b += (size_t)gridDim.x * 256) {
        const unsigned lo = bstart[b], hi = bstart[b + 1];
        // (a heavy bucket of the fine grid keeps its fill order here: dl_sub_bin_kernel re-orders it cell by cell, every cell by
        // index, whatever order it finds; a coarse bucket of more than 256 unfinished sites keeps its fill order)
        if (hi - lo < 2 || hi - lo > (coarse ? 256u : kHeavy)) continue;
        for (unsigned i = lo + 1; i < hi; ++i) {
            const unsigned v = sorted[i];
            unsigned j = i;
            while (j > lo && sorted[j - 1] > v) { sorted[j] = sorted[j - 1]; --j; }
            sorted[j] = v;
        }
    }
}

// positions (and point indices) in the order of a list: MODE 0 `list` holds point indices, 1 ranks into far_idx, 2 indices
// into left_idx (ranks of ranks)
template <int MODE>
__global__ __launch_bounds__(256)
void dl_list_xy_kernel(const float *__restrict__ flow, int sign, int W, const DlHead *__restrict__ head,
                       const unsigned *__restrict__ list, const unsigned *__restrict__ far_idx,
                       P2 *__restrict__ xy, unsigned *__restrict__ pt)
{
    const unsigned n = MODE == 0 ? head->kept : (MODE == 1 ? head->n_far : head->n_left);
    const PosFn pos(flow, sign, W);
    for (unsigned j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const unsigned i = MODE == 0 ? list[j] : far_idx[list[j]];
        xy[j] = pos((int)i);
        if (pt) pt[j] = i;
    }
}

// Exact duplicates (folded integer-valued fields: BASELINE config 5 puts several sites on most lattice nodes): Qhull keeps
// ONE vertex per location and which one is its own business, so only the smallest index of a location stays a site here.
// The others are flagged, and their entries in the bucket list are blanked (index 0xFFFFFFFF: every consumer skips
// negative candidates) -- a field with five sheets builds a fifth of the stars.
__global__ __launch_bounds__(256)
void dl_dedupe_kernel(DlHead *__restrict__ head, const unsigned *__restrict__ bstart, unsigned *__restrict__ sorted,
                      const P2 *__restrict__ sorted_xy, unsigned char *__restrict__ dup)
{
    const size_t nb = (size_t)head->grid.gx * head->grid.gy;
    for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < nb; b += (size_t)gridDim.x * 256) {
        const unsigned lo = bstart[b], hi = bstart[b + 1];
        if (hi - lo > kDedupeSmall) atomicAdd(&head->n_big, hi - lo);     // rare: dl_big_* below take these buckets
        if (hi - lo > kHeavy) head->any_heavy = 1u;                       // rare: dl_sub_bin_kernel gives these buckets grids of their own
        if (hi - lo < 2 || hi - lo > kDedupeSmall) continue;
        for (unsigned j = lo + 1; j < hi; ++j) {
            const P2 q = sorted_xy[j];
            bool same = false;
            for (unsigned i = lo; i < j && !same; ++i) same = sorted[i] != 0xFFFFFFFFu && sorted_xy[i].x == q.x && sorted_xy[i].y == q.y;
            if (same) { dup[sorted[j]] = 1; sorted[j] = 0xFFFFFFFFu; }
        }
    }
}

// Buckets of more than kDedupeSmall entries -- a flow that collapses a whole block of the image onto one pixel is legal
// input to Flow.apply, and Qhull (option Qc) treats coincident points as ONE vertex -- drop their duplicates through an
// open-addressing table of point indices keyed by the position's bits (`table`: T = 2^k >= 2 n_big entries of the
// neighbour pool, which nothing uses yet): insertion keeps the SMALLEST index of every location, a second pass over the
// entries blanks the others.  All three kernels return at once when no such bucket exists (n_big == 0).
__device__ __forceinline__ unsigned dl_big_size(const DlHead *head, unsigned long long cap)
{
    unsigned long long t = 1024;
    while (t < 2ull * head->n_big && 2 * t <= cap) t <<= 1;   // a power of two (cap = pool entries >= 8 n > 4 n_big: never binding)
    return (unsigned)t;
}

__device__ __forceinline__ unsigned dl_pos_hash(const P2 &q)
{
    unsigned long long a = (unsigned long long)__double_as_longlong(q.x), b = (unsigned long long)__double_as_longlong(q.y);
    a ^= a >> 33; a *= 0xff51afd7ed558ccdull; a ^= a >> 33;
    b ^= b >> 29; b *= 0xc4ceb9fe1a85ec53ull; b ^= b >> 32;
    a ^= b + 0x9e3779b97f4a7c15ull + (a << 6) + (a >> 2);
    return (unsigned)(a ^ (a >> 32));
}

__global__ __launch_bounds__(256)
void dl_big_clear_kernel(const DlHead *__restrict__ head, unsigned *__restrict__ table, unsigned long long cap)
{
    if (head->n_big == 0) return;
    const unsigned T = dl_big_size(head, cap);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < T; i += gridDim.x * 256) table[i] = 0xFFFFFFFFu;
}

// PASS 0: insert (smallest index of a location wins), PASS 1: blank every entry that is not its location's smallest index
template <int PASS>
__global__ __launch_bounds__(256)
void dl_big_kernel(DlHead *__restrict__ head, const unsigned *__restrict__ bstart, unsigned *__restrict__ sorted,
                   const P2 *__restrict__ sorted_xy, unsigned char *__restrict__ dup, unsigned *__restrict__ table,
                   unsigned long long cap, size_t n_entries, const float *__restrict__ flow, int sign, int W)
{
    if (head->n_big == 0) return;
    const unsigned T = dl_big_size(head, cap), mask = T - 1;
    const Grid g = head->grid;
    const PosFn pos(flow, sign, W);
    n_entries = bstart[(size_t)g.gx * g.gy];                   // the filled part of `sorted`
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n_entries; j += (size_t)gridDim.x * 256) {
        const unsigned c = sorted[j];
        if (c == 0xFFFFFFFFu) continue;
        const P2 q = sorted_xy[j];
        const size_t b = (size_t)g.by(q.y) * g.gx + g.bx(q.x);
        const unsigned cnt = bstart[b + 1] - bstart[b];
        if (cnt <= kDedupeSmall) continue;
        unsigned h = dl_pos_hash(q) & mask;
        for (unsigned probe = 0; probe < T; ++probe, h = (h + 1) & mask) {
            if (PASS == 0) {
                const unsigned cur = atomicCAS(&table[h], 0xFFFFFFFFu, c);
                if (cur == 0xFFFFFFFFu) break;                           // a new location
                const P2 o = pos((int)cur);                              // (whatever index the slot holds now or later: the same location)
                if (o.x == q.x && o.y == q.y) { atomicMin(&table[h], c); break; }
            } else {
                const unsigned cur = table[h];
                if (cur == 0xFFFFFFFFu) break;                           // (cannot happen: every entry was inserted)
                const P2 o = pos((int)cur);
                if (o.x == q.x && o.y == q.y) {
                    if (cur != c) { dup[c] = 1; sorted[j] = 0xFFFFFFFFu; }
                    break;
                }
            }
        }
    }
}

// A grid of its own for every heavy bucket (ofl_dl::SubGrid; the list of their numbers comes from dl_compact_kernel<5>): one
// workgroup per bucket measures the bounding box of the bucket's entries, lays K x K cells over it -- K = ceil(sqrt(m / 2)),
// at most 256 -- counts, scans and re-orders the bucket's stretch of `sorted` / `sorted_xy` cell by cell (through the scratch
// arrays: entries move within [lo, hi) only) and sorts every cell by point index, so that the order of a cluster's sites --
// and with it the order in which every star meets its neighbours -- does not depend on the order the fill pass happened to
// leave (buckets of more than 256 entries keep their fill order in dl_sort_kernel).
__global__ __launch_bounds__(256)
void dl_sub_bin_kernel(DlHead *head, const unsigned *__restrict__ bstart, unsigned *__restrict__ sorted, P2 *__restrict__ sorted_xy,
                       const unsigned *__restrict__ heavy_bucket, SubGrid *__restrict__ info, unsigned *__restrict__ sub_start,
                       unsigned long long sub_cap, unsigned *__restrict__ tmp_idx, P2 *__restrict__ tmp_xy, unsigned *__restrict__ tmp_slot)
{
    __shared__ unsigned long long s_k[4];
    __shared__ unsigned s_off, s_carry;
    const int t = threadIdx.x;
    const unsigned n_heavy = head->n_heavy;
    for (unsigned h = blockIdx.x; h < n_heavy; h += gridDim.x) {
        __syncthreads();
        const size_t b = heavy_bucket[h];
        const unsigned lo = bstart[b], hi = bstart[b + 1], m = hi - lo;
        if (t < 4) s_k[t] = (t & 1) ? 0ull : ~0ull;            // ordered keys of xmin, xmax, ymin, ymax
        __syncthreads();
        double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
        for (unsigned j = lo + t; j < hi; j += 256) {
            const P2 q = sorted_xy[j];
            x0 = fmin(x0, q.x); x1 = fmax(x1, q.x); y0 = fmin(y0, q.y); y1 = fmax(y1, q.y);
        }
        if (x0 <= x1) { atomicMin(&s_k[0], okey(x0)); atomicMax(&s_k[1], okey(x1)); atomicMin(&s_k[2], okey(y0)); atomicMax(&s_k[3], okey(y1)); }
        __syncthreads();
        x0 = okey_inv(s_k[0]); x1 = okey_inv(s_k[1]); y0 = okey_inv(s_k[2]); y1 = okey_inv(s_k[3]);
        int K = (int)ceil(sqrt(0.5 * (double)m));
        K = K < 1 ? 1 : (K > 256 ? 256 : K);
        double cs = fmax(x1 - x0, y1 - y0) / (double)K * 1.0000001;
        if (!(cs > 0.0) || !isfinite(cs)) { K = 1; cs = 1.0; }   // (every entry on one spot: duplicates that were blanked, one live site)
        Grid g;
        g.ox = x0; g.oy = y0; g.s = cs; g.inv_s = 1.0 / cs; g.gx = K; g.gy = K;
        const unsigned cells = (unsigned)(K * K);
        if (t == 0) s_off = atomicAdd(&head->sub_used, cells + 1u);
        __syncthreads();
        const unsigned off = s_off;
        if ((unsigned long long)off + cells + 1u > sub_cap) { if (t == 0) atomicOr(&head->err, kErrDegenerate); continue; }   // (cannot happen: DlWs::sub_cap)
        unsigned *st = sub_start + off;
        for (unsigned c = t; c <= cells; c += 256) st[c] = 0u;
        __syncthreads();
        for (unsigned j = lo + t; j < hi; j += 256) {
            const P2 q = sorted_xy[j];
            tmp_slot[j] = atomicAdd(&st[(unsigned)g.by(q.y) * (unsigned)K + (unsigned)g.bx(q.x)], 1u);
        }
        __syncthreads();
        if (t == 0) s_carry = lo;
        __syncthreads();
        for (unsigned base = 0; base <= cells; base += 1024u) {       // counts -> absolute starts, in place
            unsigned e[4], v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { const unsigned i = base + 4u * t + k; e[k] = i <= cells ? st[i] : 0u; v += e[k]; }
            unsigned total;
            unsigned run = block_exscan(v, total) + s_carry;
#pragma unroll
            for (int k = 0; k < 4; ++k) { const unsigned i = base + 4u * t + k; if (i <= cells) st[i] = run; run += e[k]; }
            __syncthreads();
            if (t == 0) s_carry += total;
            __syncthreads();
        }
        for (unsigned j = lo + t; j < hi; j += 256) {
            const P2 q = sorted_xy[j];
            const unsigned dst = st[(unsigned)g.by(q.y) * (unsigned)K + (unsigned)g.bx(q.x)] + tmp_slot[j];
            tmp_idx[dst] = sorted[j]; tmp_xy[dst] = q;
        }
        __syncthreads();
        for (unsigned j = lo + t; j < hi; j += 256) { sorted[j] = tmp_idx[j]; sorted_xy[j] = tmp_xy[j]; }
        __syncthreads();
        for (unsigned c = t; c < cells; c += 256) {                   // every cell ascending by point index (blanked entries last)
            const unsigned a = st[c], e = st[c + 1];
            for (unsigned i = a + 1; i < e; ++i) {
                const unsigned v = sorted[i];
                const P2 q = sorted_xy[i];
                unsigned j = i;
                while (j > a && sorted[j - 1] > v) { sorted[j] = sorted[j - 1]; sorted_xy[j] = sorted_xy[j - 1]; --j; }
                sorted[j] = v; sorted_xy[j] = q;
            }
        }
        if (t == 0) { SubGrid sg; sg.g = g; sg.off = off; sg.pad = 0u; info[h] = sg; }
    }
}

// compaction in ascending order: MODE 0 = points with deg == kDegFar -> far_idx, MODE 1 = ranks with far_deg == kDegLeft -> left_idx,
// MODE 2 = points with deg == kDegFan -> todo_idx (what the cell pass left to the fan pass),
// MODE 3 = points with deg == kDegTodo -> the clip pass's list (a list in BUCKET order -- entries of `sorted` -- was measured:
// no faster on any field, BASELINE config 5 included, and its compaction costs 0.2 ms more at 4K: the gather of deg[sorted[j]])
// MODE 1 also lists the ranks the wave pass finished beyond kMidRings coarse rings (aux = far_wide): they are not computed
// again, but the workgroup pass searches the coarse grid only that far around a point, and a neighbour whose own cell
// reaches farther would otherwise be missing from its candidates.
// the flags of the eight elements [base, base + 8) as bits (base a multiple of 8; elements at or beyond n are not flagged):
// one 8-byte load of the degree bytes -- or two 16-byte loads of the ranks' words and one 8-byte load of `aux`
template <int MODE>
__device__ __forceinline__ unsigned flagged8(const void *src, const unsigned char *aux, size_t base, size_t n, int W, int H);

template <int MODE>
__device__ __forceinline__ bool flagged(const void *src, const unsigned char *aux, size_t i)
{
    if (MODE == 5) return ((const unsigned *)src)[i + 1] - ((const unsigned *)src)[i] > kHeavy;      // (src = bstart: a heavy bucket)
    if (MODE == 3) return ((const unsigned char *)src)[i] == kDegTodo;
    return MODE == 0 ? ((const unsigned char *)src)[i] == kDegFar
         : MODE == 2 ? ((const unsigned char *)src)[i] == kDegFan : (((const unsigned *)src)[i] == kDegLeft || aux[i] != 0);
}

// Ordered compaction in ONE launch (decoupled look-back).  A workgroup draws a SUPER TILE of kCompactTiles x kScanChunk elements by
// ticket -- so a tile's predecessors are resident or done when it starts waiting for them -- counts it, publishes the count
// as (flag | value) in one word (1 << 30: the tile's own aggregate, 1 << 31: the inclusive prefix) with agent-scope (sc1)
// stores, and its first wave looks back 64 tiles at a time (sc1 loads: the per-XCD L2s are not coherent) until it meets an
// inclusive word; then the super tile is walked a second time (its flags come from L2) and the list is written.  A 4K field is
// 254 super tiles -- one per CU, one look-back window deep: with one tile per 2048 elements the thousands of tiles that start
// together each walked back over all the others (65 us per list; the three-kernel count / scan / write it replaced: 27 us).
// state[0] = the ticket counter, state[4 + t] = tile t's word; zeroed by the caller.
template <int MODE>
__device__ __forceinline__ unsigned flagged8(const void *src, const unsigned char *aux, size_t base, size_t n, int W, int H)
{
    unsigned bits = 0;
    if (MODE == 4) {
        // MODE 4: the sites the site-wise raster has to look at -- a star of 1 .. kSlots neighbours, and not clean (aux = the
        // tile flags): the clean ones are drawn cell by cell
        if (base >= n) return 0u;
        const uint2 w = base + 8 <= n ? *reinterpret_cast<const uint2 *>((const unsigned char *)src + base) : make_uint2(0u, 0u);
        int y = (int)((float)base / (float)W);
        int x = (int)((long long)base - (long long)y * W);
        while (x < 0) { --y; x += W; }
        while (x >= W) { ++y; x -= W; }
        const int tiles_x = (W + 31) / 32;
        // (eight sites of one row whose cells all lie in clean tiles: nothing to list -- four bytes instead of thirty-two)
        if (x + 7 < W && x >= 2 && y >= 2 && x + 7 <= W - 3 && y <= H - 2) {
            const int tx0 = (x - 2) >> 5, tx1 = (x + 8) >> 5, ty0 = (y - 2) >> 3, ty1 = y >> 3;
            if (aux[ty0 * tiles_x + tx0] && aux[ty0 * tiles_x + tx1] && aux[ty1 * tiles_x + tx0] && aux[ty1 * tiles_x + tx1]) return 0u;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned d = base + 8 <= n ? (((k < 4 ? w.x : w.y) >> (8 * (k & 3))) & 0xFFu) : (base + k < n ? ((const unsigned char *)src)[base + k] : 0u);
            if (d >= 1u && d <= (unsigned)kSlots && !site_clean(aux, x, y, W, H, tiles_x)) bits |= 1u << k;
            if (++x == W) { x = 0; ++y; }
        }
        return bits;
    }
    if (MODE == 5) {
        if (base + 8 <= n) {
            const uint4 a = *reinterpret_cast<const uint4 *>((const unsigned *)src + base), b = *reinterpret_cast<const uint4 *>((const unsigned *)src + base + 4);
            const unsigned e[9] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, ((const unsigned *)src)[base + 8] };
#pragma unroll
            for (int k = 0; k < 8; ++k) if (e[k + 1] - e[k] > kHeavy) bits |= 1u << k;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) if (base + k < n && flagged<5>(src, aux, base + k)) bits |= 1u << k;
        }
        return bits;
    }
    if (base + 8 <= n) {
        if (MODE != 1) {
            const unsigned char want = MODE == 3 ? kDegTodo : (MODE == 0 ? kDegFar : kDegFan);
            const uint2 w = *reinterpret_cast<const uint2 *>((const unsigned char *)src + base);
#pragma unroll
            for (int k = 0; k < 8; ++k) if ((((k < 4 ? w.x : w.y) >> (8 * (k & 3))) & 0xFFu) == want) bits |= 1u << k;
        } else {
            const uint4 a = *reinterpret_cast<const uint4 *>((const unsigned *)src + base), b = *reinterpret_cast<const uint4 *>((const unsigned *)src + base + 4);
            const uint2 x = *reinterpret_cast<const uint2 *>(aux + base);
            const unsigned d[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
            for (int k = 0; k < 8; ++k) if (d[k] == kDegLeft || (((k < 4 ? x.x : x.y) >> (8 * (k & 3))) & 0xFFu) != 0u) bits |= 1u << k;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) if (base + k < n && flagged<MODE>(src, aux, base + k)) bits |= 1u << k;
    }
    return bits;
}

constexpr int kCompactTiles = 16;
template <int MODE>
__global__ __launch_bounds__(256)
void dl_compact_kernel(const void *__restrict__ src, const unsigned char *__restrict__ aux, DlHead *head, size_t n_fixed,
                       unsigned *__restrict__ state, unsigned *__restrict__ list, unsigned *__restrict__ rank_of, int W = 0, int H = 0)
{
    __shared__ unsigned s_tile, s_prefix;
    if (threadIdx.x == 0) s_tile = atomicAdd(&state[0], 1u);
    __syncthreads();
    const unsigned tile = s_tile;
    // (MODE 5, the heavy buckets: nothing to look at unless the dedupe pass met one -- every tile then publishes an empty prefix)
    const size_t n = MODE == 5 ? (head->any_heavy ? (size_t)head->grid.gx * head->grid.gy : 0) : (MODE != 1 ? n_fixed : head->n_far);
    const size_t base0 = (size_t)tile * kCompactTiles * kScanChunk + (size_t)threadIdx.x * 8;
    unsigned v = 0;
    unsigned keep[kCompactTiles / 4];                     // the flag bits of the thread's 16 x 8 elements: the second walk does not evaluate them again
#pragma unroll
    for (int c = 0; c < kCompactTiles; ++c) {
        const unsigned b8 = flagged8<MODE>(src, aux, base0 + (size_t)c * kScanChunk, n, W, H);
        v += (unsigned)__popc(b8);
        if ((c & 3) == 0) keep[c >> 2] = b8; else keep[c >> 2] |= b8 << (8 * (c & 3));
    }
    unsigned total;
    (void)block_exscan(v, total);
    if (threadIdx.x < 64) {
        unsigned *st = state + 4;
        const int lane = threadIdx.x;
        if (tile > 0 && lane == 0) __hip_atomic_store(&st[tile], 0x40000000u | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned prefix = 0;
        for (long long hi = (long long)tile - 1; hi >= 0;) {
            const long long j = hi - lane;
            unsigned w;
            for (;;) {
                w = j >= 0 ? __hip_atomic_load(&st[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0x80000000u;     // (before tile 0: an inclusive 0)
                if (!__ballot(w == 0u)) break;
                __builtin_amdgcn_s_sleep(1);
            }
            const unsigned long long inc = __ballot((w & 0x80000000u) != 0u);
            const int stop = inc ? __ffsll((long long)inc) - 1 : 63;          // the nearest inclusive word of the window (lane 0 = nearest tile)
            unsigned v2 = lane <= stop ? (w & 0x3FFFFFFFu) : 0u;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v2 += (unsigned)__shfl_xor((int)v2, off);
            prefix += v2;
            if (inc) break;
            hi -= 64;
        }
        if (lane == 0) {
            __hip_atomic_store(&st[tile], 0x80000000u | (prefix + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_prefix = prefix;
        }
    }
    __syncthreads();
    unsigned run = s_prefix;
#pragma unroll
    for (int c = 0; c < kCompactTiles; ++c) {
        const size_t base = base0 + (size_t)c * kScanChunk;
        if (base - (size_t)threadIdx.x * 8 >= n) break;        // (uniform: the whole chunk lies beyond the end)
        const unsigned bits = (keep[c >> 2] >> (8 * (c & 3))) & 0xFFu, cv = (unsigned)__popc(bits);
        unsigned ctotal;
        unsigned at = run + block_exscan(cv, ctotal);
        run += ctotal;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if ((bits >> k) & 1u) {
                if (MODE == 0 && rank_of) rank_of[(base + k) * kSlots] = at;     // an unfinished point's first neighbour slot holds its rank
                if (MODE != 5 || at < n_fixed) list[at] = (unsigned)(base + k);
                ++at;
            }
    }
    if (tile == gridDim.x - 1 && threadIdx.x == 0) {
        unsigned cnt = s_prefix + total;
        if (MODE == 0 && (unsigned long long)n_fixed * kSlots + (unsigned long long)cnt * kFarK >= 0xFFFFFFF0ull) {
            atomicOr(&head->err, 8u);                      // the unfinished stars exceed the triangle-id space: none is built, the caller is told
            cnt = 0;
        }
        if ((MODE == 0 && cnt > kMaxFar) || (MODE == 1 && cnt > kMaxLeft)) { atomicOr(&head->err, kErrDegenerate); cnt = 0; }
        if (head->err & kErrDegenerate) cnt = 0;           // a degenerate point set: no star pass runs (their loops are sized for ordinary buckets)
        if (MODE == 5 && cnt > n_fixed) { atomicOr(&head->err, kErrDegenerate); cnt = 0; }       // (n_fixed: the capacity of the list; cannot happen by its bound)
        if (MODE == 0) head->n_far = cnt; else if (MODE == 1) head->n_left = cnt; else if (MODE == 2) head->n_fan = cnt;
        else if (MODE == 3) head->n_todo = cnt; else if (MODE == 4) head->n_raster = cnt; else head->n_heavy = cnt;
    }
}

int scan_exclusive(unsigned *data, size_t n, unsigned *tmp, hipStream_t s)
{
    if (n <= (size_t)kScanBig) {
        hipLaunchKernelGGL(dl_scan_small_kernel, dim3(1), dim3(1024), 0, s, data, (unsigned)n);
    } else {
        const size_t m = (n + kScanBig - 1) / kScanBig;                // chunk sums; tmp holds them (and the next level's, recursively)
        hipLaunchKernelGGL(dl_scan_reduce_kernel, dim3((unsigned)m), dim3(256), 0, s, (const unsigned *)data, n, tmp);
        OFL_TRY(scan_exclusive(tmp, m, tmp + (m + 63) / 64 * 64, s));
        hipLaunchKernelGGL(dl_scan_apply_kernel, dim3((unsigned)m), dim3(256), 0, s, data, n, (const unsigned *)tmp);
    }
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

unsigned blocks_of(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

template <int LIST>
void compact_launch(size_t n_elems, const void *src, const unsigned char *aux, DlWs &ws, size_t n_fixed, unsigned *list, unsigned *rank_of,
                    int W, int H, hipStream_t s)
{
    const unsigned tiles = blocks_of(n_elems, kScanChunk);
    hipLaunchKernelGGL(dl_compact_kernel<LIST>, dim3((tiles + kCompactTiles - 1) / kCompactTiles), dim3(256), 0, s, src, aux, ws.head, n_fixed,
                       ws.cstate + LIST * ws.cstride, list, rank_of, W, H);
}

}  // namespace

// the host side of the stage: what each entry reads, writes and borrows is stated at its declaration (ofl_delaunay_ws.h)
namespace ofl_dlw {

int bin_sites(const DlIn &in, DlWs &ws, hipStream_t s, bool slab, int row0, int rows)
{
    const size_t n = (size_t)in.H * in.W;
    OFL_HIP(hipMemsetAsync(ws.bstart, 0, (ws.bcap + 1) * 4, s));
    const unsigned nblk = blocks_of(n, 256), bblk = std::min<unsigned>(blocks_of(ws.bcap, 256), 65535u);
    const dim3 bgrid((in.W + 31) / 32, std::max(1, std::min((in.H + 7) / 8, 4096 / ((in.W + 31) / 32) + 1)));
    unsigned long long *partial = (unsigned long long *)ws.pool;        // BORROWED: the neighbour pool is free until the cooperative passes; 8 n + 65 536 words
    unsigned *slot = ws.todo_idx;                                       // BORROWED: the fan pass's list is free until the cells are done
    hipLaunchKernelGGL(dl_bbox_kernel, bgrid, dim3(256), 0, s, in.flow, in.sign_pp, in.pmask, in.H, in.W, partial);
    hipLaunchKernelGGL(dl_params_kernel, dim3(1), dim3(256), 0, s, ws.head, (unsigned long long)ws.bcap, in.H, in.W, slab ? 1 : 0, row0, rows,
                       partial, bgrid.x * bgrid.y);
    OFL_HIP(hipMemsetAsync(ws.dup, 0, n, s));
    hipLaunchKernelGGL(dl_count_kernel, dim3(nblk), dim3(256), 0, s, in.flow, in.sign_pp, in.pmask, in.H, in.W, ws.head, ws.bstart, ws.dup, slot);
    OFL_HIP(hipGetLastError());
    OFL_TRY(scan_exclusive(ws.bstart, ws.bcap + 1, ws.scan_tmp, s));
    hipLaunchKernelGGL(dl_fill_kernel, dim3(nblk), dim3(256), 0, s, in.flow, in.sign_pp, in.pmask, in.H, in.W, ws.head, ws.bstart, slot, ws.sorted, ws.dup);
    hipLaunchKernelGGL(dl_sort_kernel, dim3(bblk), dim3(256), 0, s, ws.head, 0, ws.bstart, ws.sorted);
    hipLaunchKernelGGL(dl_list_xy_kernel<0>, dim3(std::min<unsigned>(nblk, 65535u)), dim3(256), 0, s, in.flow, in.sign_pp, in.W, ws.head,
                       ws.sorted, nullptr, ws.sorted_xy, nullptr);
    hipLaunchKernelGGL(dl_dedupe_kernel, dim3(bblk), dim3(256), 0, s, ws.head, ws.bstart, ws.sorted, ws.sorted_xy, ws.dup);
    {   // buckets too large for the pairwise dedupe (whole image blocks collapsed onto one spot): no-ops when there are none
        const dim3 gb(std::min<unsigned>(nblk, 16384u));
        unsigned *table = (unsigned *)ws.pool;                          // BORROWED, as above (the partials are spent)
        const unsigned long long cap = ws.pool_cap;
        hipLaunchKernelGGL(dl_big_clear_kernel, gb, dim3(256), 0, s, ws.head, table, cap);
        auto big = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, gb, dim3(256), 0, s, ws.head, ws.bstart, ws.sorted, ws.sorted_xy, ws.dup, table, cap, n, in.flow, in.sign_pp, in.W);
        };
        big(dl_big_kernel<0>);
        big(dl_big_kernel<1>);
    }
    return OFL_OK;
}

int bin_clusters(const DlIn &in, DlWs &ws, hipStream_t s)
{
    OFL_TRY(compact_reset(ws, kListHeavy, kListHeavy, s));
    compact_list(kListHeavy, in, ws, s);
    // BORROWED: far_off, left_xy and far_deg are free until the unfinished points are listed
    hipLaunchKernelGGL(dl_sub_bin_kernel, dim3(1024), dim3(256), 0, s, ws.head, ws.bstart, ws.sorted, ws.sorted_xy, ws.heavy_bucket, ws.heavy_info,
                       ws.sub_start, (unsigned long long)ws.sub_cap, /* tmp_idx */ ws.far_off, /* tmp_xy */ ws.left_xy, /* tmp_slot */ ws.far_deg);
    return OFL_OK;
}

int compact_reset(DlWs &ws, int first, int last, hipStream_t s)
{
    OFL_HIP(hipMemsetAsync(ws.cstate + first * ws.cstride, 0, (size_t)(last - first + 1) * ws.cstride * 4, s));
    return OFL_OK;
}

void compact_list(int list, const DlIn &in, DlWs &ws, hipStream_t s)
{
    const size_t n = (size_t)in.H * in.W;
    switch (list) {      //                          elements  source      aux          n_fixed        list (BORROWED: ofl_delaunay_ws.h)  rank_of
    case kListFar:    compact_launch<kListFar>   (n,       ws.deg,     nullptr,     ws, n,            ws.far_idx,      ws.nbr,  0, 0, s); break;
    case kListLeft:   compact_launch<kListLeft>  (n,       ws.far_deg, ws.far_wide, ws, 0,            ws.left_idx,     nullptr, 0, 0, s); break;      // (sized by head->n_far)
    case kListFan:    compact_launch<kListFan>   (n,       ws.deg,     nullptr,     ws, n,            ws.todo_idx,     nullptr, 0, 0, s); break;
    case kListTodo:   compact_launch<kListTodo>  (n,       ws.deg,     nullptr,     ws, n,            ws.far_idx,      nullptr, 0, 0, s); break;      // (far_idx is free until the unfinished points are listed)
    case kListRaster: compact_launch<kListRaster>(n,       ws.deg,     ws.tileflag, ws, n,            ws.todo_idx,     nullptr, in.W, in.H, s); break; // (the fan pass's list is free again)
    case kListHeavy:  compact_launch<kListHeavy> (ws.bcap, ws.bstart,  nullptr,     ws, ws.heavy_cap, ws.heavy_bucket, nullptr, 0, 0, s); break;
    }
}

int bin_unfinished(const DlIn &in, DlWs &ws, hipStream_t s)
{
    const unsigned rblk = std::min<unsigned>(blocks_of((size_t)in.H * in.W, 256), 2048u);
    OFL_HIP(hipMemsetAsync(ws.b1start, 0, (ws.b1cap + 1) * 4, s));
    OFL_HIP(hipMemsetAsync(ws.b1cursor, 0, ws.b1cap * 4, s));
    hipLaunchKernelGGL(dl_count1_kernel, dim3(rblk), dim3(256), 0, s, in.flow, in.sign_pp, in.W, ws.head, ws.far_idx, ws.b1start);
    OFL_TRY(scan_exclusive(ws.b1start, ws.b1cap + 1, ws.scan_tmp, s));
    hipLaunchKernelGGL(dl_fill1_kernel, dim3(rblk), dim3(256), 0, s, in.flow, in.sign_pp, in.W, ws.head, ws.far_idx, ws.b1start, ws.b1cursor, ws.sorted1);
    hipLaunchKernelGGL(dl_sort_kernel, dim3(std::min<unsigned>(blocks_of(ws.b1cap, 256), 65535u)), dim3(256), 0, s, ws.head, 1, ws.b1start, ws.sorted1);
    hipLaunchKernelGGL(dl_list_xy_kernel<1>, dim3(rblk), dim3(256), 0, s, in.flow, in.sign_pp, in.W, ws.head, ws.sorted1, ws.far_idx,
                       ws.sorted1_xy, ws.sorted1_pt);
    return OFL_OK;
}

void bin_leftover(const DlIn &in, DlWs &ws, hipStream_t s)
{
    const unsigned rblk = std::min<unsigned>(blocks_of((size_t)in.H * in.W, 256), 2048u);
    hipLaunchKernelGGL(dl_list_xy_kernel<2>, dim3(rblk), dim3(256), 0, s, in.flow, in.sign_pp, in.W, ws.head, ws.left_idx, ws.far_idx, ws.left_xy, ws.left_pt);
}

}  // namespace ofl_dlw
