// ofl_delaunay_stars.hip -- K3 exact path, the per-thread star passes (the map of the path: ofl_delaunay.hip): mesh cells
// and the sites they settle, mesh fans, the clip pass, the second per-thread pass over the unfinished points.  The geometry
// of each is in ofl_delaunay_core.h.
#include "ofl_delaunay_dev.h"

using namespace ofl;
using namespace ofl_sc;
using namespace ofl_dl;
using namespace ofl_dlw;

namespace {

// every how-manieth grid cell dl_cell_sample_kernel looks at (about 4 096 of them)
__host__ __device__ inline size_t fan_sample_stride(size_t n) { return n / 4096 + 1; }

// Is the mesh worth proposing stars from?  On a strongly sheared field (BASELINE config 5: every source row slides 1 .. 19 px
// against the next, 42 % of the sites are duplicates) the Delaunay neighbours of a site have nothing to do with its grid
// neighbours: no cell verifies, and the cell, cell-flag and fan passes (0.6 ms at 8K) verify nothing.  dl_cell_sample_kernel
// runs the cell test on every fan_sample_stride-th grid cell BEFORE those passes (a few thousand cells, whatever the slab: the
// ranks of a slab-wise call and a whole-field call must decide alike -- which pass settles a site shows in the order of its
// neighbours, hence in triangle ids and ties); when at least 64 samples have four kept corners and fewer than 1 in 128 of those
// verify, all three passes step aside and every site goes to the clip pass.  A speed decision only: the clip pass computes the
// same stars the cells and fans would have verified.
__device__ __forceinline__ bool dl_skip_mesh(const DlHead *head) { return head->sample_all >= 64u && head->sample_ok * 128u < head->sample_all; }

// ------------------------------------------------------------------------------------------------ stars, mesh-cell pass
// One thread per grid cell: both triangles of an intact, convex, positively oriented cell are verified ONCE against the
// sites under their circumcircles (ofl_dl::cell_verify) instead of three times from their three vertices; then one thread
// per site reads the flags of its four cells -- all verified: the star is written without touching a candidate.
__global__ __launch_bounds__(256)
void dl_cell_kernel(const float *__restrict__ flow, int sign, const uint8_t *__restrict__ pmask, int H, int W,
                    const DlHead *__restrict__ head, const unsigned *__restrict__ bstart,
                    const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy, const unsigned char *__restrict__ dup,
                    unsigned char *__restrict__ cellflag, unsigned char *__restrict__ tileflag, int tiles_x, int ntiles)
{
    const unsigned per = gridDim.x >> 3;                        // (grid padded to a multiple of 8) one contiguous eighth per XCD
    const int tile = (int)((blockIdx.x & 7u) * per + (blockIdx.x >> 3));
    if (tile >= ntiles) return;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x = tx * 32 + (threadIdx.x & 31), y = ty * 8 + (threadIdx.x >> 5);
    const bool in_grid = x < W && y < H;
    const size_t ia = in_grid ? (size_t)y * W + x : 0;
    int flag = 0;
    if (in_grid && x < W - 1 && y < H - 1 && !(head->err & kErrDegenerate) && !dl_skip_mesh(head) &&
        kept_pt(pmask, ia) && kept_pt(pmask, ia + 1) && kept_pt(pmask, ia + W) && kept_pt(pmask, ia + W + 1) &&
        !(dup[ia] | dup[ia + 1] | dup[ia + W] | dup[ia + W + 1])) {
        const D2 a = point_of(flow, sign, W, x, y), b = point_of(flow, sign, W, x + 1, y);
        const D2 c = point_of(flow, sign, W, x + 1, y + 1), d = point_of(flow, sign, W, x, y + 1);
        // (slab mode: a cell none of whose corners gets a star here is not looked at -- every site that does get one still
        // finds all four of its cells verified, so its star comes out of the same pass as in a whole-field run)
        const double lo = head->need_lo, hi = head->need_hi;
        if (fmax(fmax(a.y, b.y), fmax(c.y, d.y)) >= lo && fmin(fmin(a.y, b.y), fmin(c.y, d.y)) <= hi)
        flag = cell_verify((int)ia, W, P2{ a.x, a.y }, P2{ b.x, b.y }, P2{ c.x, c.y }, P2{ d.x, d.y }, head->grid, bstart, sorted, sorted_xy,
                           PosFn(flow, sign, W), kFanSpan);
    }
    if (in_grid) cellflag[ia] = (unsigned char)flag;
    // a CLEAN tile: every one of its 256 cells verified (tiles that reach the last row or column of sites never are)
    const int clean = __syncthreads_and(flag != 0);
    if (threadIdx.x == 0) tileflag[tile] = clean ? 1 : 0;
}

// the sample of grid cells that decides whether the mesh is a guide to this triangulation at all (dl_skip_mesh)
__global__ __launch_bounds__(256)
void dl_cell_sample_kernel(const float *__restrict__ flow, int sign, const uint8_t *__restrict__ pmask, int H, int W,
                           DlHead *__restrict__ head, const unsigned *__restrict__ bstart,
                           const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy, const unsigned char *__restrict__ dup)
{
    const size_t n = (size_t)H * W, stride = fan_sample_stride(n);
    const size_t ia = ((size_t)blockIdx.x * 256 + threadIdx.x) * stride;
    unsigned all = 0, ok = 0;
    if (ia < n && !(head->err & kErrDegenerate)) {
        const int y = (int)(ia / (unsigned)W), x = (int)(ia - (size_t)y * W);
        if (x < W - 1 && y < H - 1 &&
            kept_pt(pmask, ia) && kept_pt(pmask, ia + 1) && kept_pt(pmask, ia + W) && kept_pt(pmask, ia + W + 1) &&
            !(dup[ia] | dup[ia + 1] | dup[ia + W] | dup[ia + W + 1])) {
            const D2 a = point_of(flow, sign, W, x, y), b = point_of(flow, sign, W, x + 1, y);
            const D2 c = point_of(flow, sign, W, x + 1, y + 1), d = point_of(flow, sign, W, x, y + 1);
            all = 1;
            ok = cell_verify((int)ia, W, P2{ a.x, a.y }, P2{ b.x, b.y }, P2{ c.x, c.y }, P2{ d.x, d.y }, head->grid, bstart, sorted, sorted_xy,
                             PosFn(flow, sign, W), kFanSpan) != 0 ? 1u : 0u;
        }
    }
    const unsigned long long ball = __ballot(all != 0), bok = __ballot(ok != 0);
    if ((threadIdx.x & 63) == 0) {
        if (ball) atomicAdd(&head->sample_all, (unsigned)__popcll(ball));
        if (bok) atomicAdd(&head->sample_ok, (unsigned)__popcll(bok));
    }
}

__global__ __launch_bounds__(256)
void dl_site_cells_kernel(const float *__restrict__ flow, int sign, const uint8_t *__restrict__ pmask, int H, int W, const DlHead *__restrict__ head,
                          const unsigned char *__restrict__ dup, const unsigned char *__restrict__ cellflag,
                          unsigned char *__restrict__ deg, unsigned *__restrict__ nbr)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)H * W) return;
    if (!kept_pt(pmask, p) || dup[p]) { deg[p] = 0; return; }
    if (head->err & kErrDegenerate) { deg[p] = kDegTodo; return; }           // (no star pass runs on a refused point set)
    const int y = (int)(p / (unsigned)W), x = (int)(p - (size_t)y * W);
    if (head->need_lo > -1e300 || head->need_hi < 1e300) {   // slab mode: no star for a site outside the slab (degree 0: nothing is drawn from it, nothing looks it up)
        const D2 q = point_of(flow, sign, W, x, y);
        if (!(q.y >= head->need_lo && q.y <= head->need_hi)) { deg[p] = 0; return; }
    }
    int n = 0;
    if (x > 0 && y > 0 && x < W - 1 && y < H - 1) {
        unsigned out[8];
        n = star_from_cells((int)p, W, cellflag[p], cellflag[p - 1], cellflag[p - W - 1], cellflag[p - W], out);
        if (n > 0) {
            uint4 *row = reinterpret_cast<uint4 *>(nbr + p * kSlots);
            row[0] = make_uint4(out[0], out[1], out[2], out[3]);
            row[1] = make_uint4(out[4], n > 5 ? out[5] : 0u, n > 6 ? out[6] : 0u, n > 7 ? out[7] : 0u);
        }
    }
    deg[p] = n > 0 ? (unsigned char)n : (dl_skip_mesh(head) ? kDegTodo : kDegFan);      // (no fans either on a mesh that is no guide)
}

// ------------------------------------------------------------------------------------------------ stars, mesh-fan pass
// One thread per point: a point whose eight grid neighbours are kept proposes the star of the cell-wise mesh and verifies
// it against the sites under its circumcircles (ofl_dl::star_fan).  Verified stars are final; everything else is marked
// for the clip pass.
__global__ __launch_bounds__(kFanBlock, 5)                    // (five waves per SIMD: the pass waits on its candidate loads)
void dl_star_fan_kernel(const float *__restrict__ flow, int sign, const uint8_t *__restrict__ pmask, int H, int W,
                        const DlHead *__restrict__ head, const unsigned *__restrict__ todo, const unsigned *__restrict__ bstart,
                        const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy, const unsigned char *__restrict__ dup,
                        unsigned char *__restrict__ deg, unsigned *__restrict__ nbr)
{
    __shared__ P2 s_rel[8][kFanBlock];
    const unsigned n_fan = head->n_fan;                         // the sites the cell pass did not settle, in index order (none when dl_skip_mesh)
    for (unsigned i = blockIdx.x * kFanBlock + threadIdx.x; i < n_fan; i += gridDim.x * kFanBlock) {
        const size_t p = todo[i];
        const int y = (int)(p / (unsigned)W), x = (int)(p - (size_t)y * W);
        // which of the eight grid neighbours exist: inside the grid, kept by the point mask, not a dropped duplicate
        unsigned kept8 = 0;
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) {
            const int dx = (int)((0x901Au >> (2 * sl)) & 3u) - 1, dy = (int)((0x01A9u >> (2 * sl)) & 3u) - 1;
            const bool in = (unsigned)(x + dx) < (unsigned)W && (unsigned)(y + dy) < (unsigned)H;
            const size_t q = in ? (size_t)((long long)p + dx + (long long)dy * W) : p;
            if (in && kept_pt(pmask, q) && !dup[q]) kept8 |= 1u << sl;
        }
        int n = 0;
        {
            const Grid g = head->grid;
            const PosFn pos(flow, sign, W);
            auto npos = [&](int sl) {                               // slot -> grid offset at compile time (the loops over slots are unrolled)
                const int dx = (int)((0x901Au >> (2 * sl)) & 3u) - 1, dy = (int)((0x01A9u >> (2 * sl)) & 3u) - 1;
                const D2 q = point_of(flow, sign, W, x + dx, y + dy);
                return P2{ q.x, q.y };
            };
            const D2 c = point_of(flow, sign, W, x, y);
            n = star_fan((int)p, W, P2{ c.x, c.y }, kept8, pos, npos, g, bstart, sorted, sorted_xy, kFanSpan, &s_rel[0][threadIdx.x], kFanBlock,
                         nbr + p * kSlots);
        }
        deg[p] = n > 0 ? (unsigned char)n : kDegTodo;
    }
}

// ------------------------------------------------------------------------------------------------ stars, clip pass (near)
// One thread per point the cells and fans did not settle, in index order.  (Round 3 measured two spatially coherent
// schedules for BASELINE config 5, whose source rows scatter over hundreds of buckets: one wave per 8 x 8 bucket tile -- half
// empty waves, 24 -> 46 ms -- and a list compacted in bucket order -- no change: the pass is bound by the divergent clip
// code of its 64 lanes, not by where the candidates come from.)
// waves per SIMD of the per-thread pass, measured (product flags, same box): 4 waves per SIMD (116 VGPRs, cells of 12) config 5 22.88 ms, 5 waves (96 VGPRs + 9 spilled,
// cells of 10: 7 680 B of LDS per wave) 21.86 ms, 6 waves (80 + 18 spilled, cells of 8) 22.69 ms; cells of 10 at 4 waves: 22.90 ms
constexpr int kNearWaves = 5;
template <bool HEAVY>       // false: every site of the list; true (a second launch, at once over when no bucket is heavy): the sites the first one marked kDegHeavy
__global__ __launch_bounds__(64, HEAVY ? 1 : kNearWaves)
void dl_star_near_kernel(const float *__restrict__ flow, int sign, const uint8_t *__restrict__ pmask, const unsigned char *__restrict__ dup, int H, int W,
                         const DlHead *__restrict__ head, const unsigned *__restrict__ todo,
                         const unsigned *__restrict__ bstart,
                         const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy,
                         unsigned char *__restrict__ deg, unsigned *__restrict__ nbr,
                         const unsigned *__restrict__ heavy_bucket, const SubGrid *__restrict__ heavy_info, const unsigned *__restrict__ sub_start)
{
    __shared__ float s_vx[kNearCap][64], s_vy[kNearCap][64];
    __shared__ int   s_tag[kNearCap][64];
    const unsigned n_todo = head->n_todo;
    const Grid g = head->grid;
    const PosFn pos(flow, sign, W);
    const SubGrids subs{ heavy_bucket, heavy_info, sub_start, head->n_heavy };       // (dense clusters: ofl_dl::apply_heavy_run)
    const SubGrids *sub = subs.n ? &subs : nullptr;
    if (HEAVY && !sub) return;
    for (unsigned base = blockIdx.x * 64; base < n_todo; base += gridDim.x * 64) {
        if (base + threadIdx.x >= n_todo) return;
        const size_t p = todo[base + threadIdx.x];
        if (HEAVY && deg[p] != kDegHeavy) continue;
        PolyT<float> P{ &s_vx[0][threadIdx.x], &s_vy[0][threadIdx.x], &s_tag[0][threadIdx.x], 64, kNearCap, 0 };
        int rings_done;
        const P2 pp = pos((int)p);
        // A cell that is still unbounded after kOpenRings rings is clipped with the site's GRID neighbours before it is given
        // up: across a tear of the mesh (a motion boundary) the neighbour on the other side closes the cell, and a closed cell
        // finishes in the second per-thread pass within a few coarse rings instead of waiting for the far side to turn up
        // (64-px stripes at 4K: that pass 1.09 -> 0.35 ms; hull points stay open, as they must).
        auto rescue = [&](PolyT<float> &Q) -> int {
            const int y = (int)(p / (unsigned)W), x = (int)(p - (size_t)y * W);
            auto rel = [&](int t) { const P2 v = pos(t); return P2{ v.x - pp.x, v.y - pp.y }; };
#pragma unroll 1
            for (int sl = 0; sl < 8; ++sl) {
                const int dx = (int)((0x901Au >> (2 * sl)) & 3u) - 1, dy = (int)((0x01A9u >> (2 * sl)) & 3u) - 1;
                if ((unsigned)(x + dx) >= (unsigned)W || (unsigned)(y + dy) >= (unsigned)H) continue;
                const size_t q = (size_t)((long long)p + dx + (long long)dy * W);
                if (!kept_pt(pmask, q) || dup[q]) continue;
                const P2 C = rel((int)q);
                if (C.x == 0.0 && C.y == 0.0) continue;
                if (poly_clip(Q, C, (int)q, (int)p, rel) < 0) return -1;
            }
            return 0;
        };
        // (a tighter bound -- reach beyond 1 .. 16 times the ring search's own radius -- was measured: no further gain)
        const int rc = star_near<HEAVY>(P, (int)p, pp, g, bstart, sorted, pos, kRings, sorted_xy, kOpenRings, &rings_done, rescue, 4.0 * head->far_t2, sub);
        if (!HEAVY && rc == 2) { deg[p] = kDegHeavy; continue; }
        bool ok = rc == 1;
        for (int k = 0; ok && k < P.n; ++k) ok = P.T(k) >= 0;
        if (!ok) {
            // unfinished: the edges of the cell so far -- their sites in cyclic order, box sides (negative) included -- seed
            // the later passes, which rebuild the cell from them in one step (slot 0 will hold the point's rank, slot 1 the
            // number of seeds, slot 14 the last fine ring that was applied completely)
            deg[p] = kDegFar;
            for (int k = 0; k < P.n; ++k) nbr[p * kSlots + 2 + k] = (unsigned)P.T(k);
            nbr[p * kSlots + 1] = (unsigned)P.n;
            nbr[p * kSlots + 14] = (unsigned)rings_done;
            continue;
        }
        deg[p] = (unsigned char)P.n;
        for (int k = 0; k < P.n; ++k) nbr[p * kSlots + k] = (unsigned)P.T(k);
    }
}

// ------------------------------------------------------------------------------------------------ stars, second per-thread pass
// One thread per unfinished point that is not on the image border (those are hull points more often than not): the cell
// is rebuilt from its seeds and finished against the coarse grid of unfinished points (ofl_dl::star_near2).  What closes
// here -- the rims of tears at motion boundaries, of small holes -- becomes an ordinary small star; the rest stays
// marked for the cooperative passes.
__global__ __launch_bounds__(64)
void dl_star_near2_kernel(const float *__restrict__ flow, int sign, int H, int W, const DlHead *__restrict__ head,
                          const unsigned *__restrict__ far_idx, const unsigned *__restrict__ bstart,
                          const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy,
                          const unsigned *__restrict__ b1start, const unsigned *__restrict__ sorted1_pt,
                          const P2 *__restrict__ sorted1_xy, unsigned char *__restrict__ deg, unsigned *__restrict__ nbr,
                          unsigned *__restrict__ far_deg, unsigned char *__restrict__ far_wide, unsigned min_points,
                          const unsigned *__restrict__ heavy_bucket, const SubGrid *__restrict__ heavy_info, const unsigned *__restrict__ sub_start)
{
    __shared__ float s_vx[kSlots][64], s_vy[kSlots][64];
    __shared__ int   s_tag[kSlots][64];
    const unsigned n_far = head->n_far;
    if (n_far < min_points) return;                        // (a per-thread pass needs tens of thousands of points to fill the chip)
    for (unsigned rank = blockIdx.x * 64 + threadIdx.x; rank < n_far; rank += gridDim.x * 64) {
    const int p = (int)far_idx[rank];
    const int py = (int)((unsigned)p / (unsigned)W), px = p - py * W;
    if (px == 0 || py == 0 || px == W - 1 || py == H - 1) continue;
    const Grid g = head->grid, g1 = head->grid1;
    const PosFn pos(flow, sign, W);
    unsigned *row = nbr + (size_t)p * kSlots;
    const int ns = min((int)row[1], kSlots - 4);
    PolyT<float> P{ &s_vx[0][threadIdx.x], &s_vy[0][threadIdx.x], &s_tag[0][threadIdx.x], 64, kSlots, 0 };
    const SubGrids subs{ heavy_bucket, heavy_info, sub_start, head->n_heavy };
    const int rc = star_near2(P, p, pos(p), row + 2, ns, (int)row[14], kRings, g, bstart, sorted, sorted_xy,
                              kNear2Rings, g1, b1start, sorted1_pt, sorted1_xy, pos, kNear2Open, 4.0 * head->far_t2, subs.n ? &subs : nullptr);
    if (rc != 1) continue;
    for (int k = 0; k < P.n; ++k) row[k] = (unsigned)P.T(k);
    deg[p] = (unsigned char)P.n;
    far_deg[rank] = 0;                                     // not a cooperative-pass star: nothing in the pool
    far_wide[rank] = 0;                                    // (its reach is within the coarse rings every later pass searches)
    }
}

}  // namespace

// the host side of the stage: what each entry reads, writes and borrows is stated at its declaration (ofl_delaunay_ws.h)
namespace ofl_dlw {

void stars_mesh(const DlIn &in, DlWs &ws, hipStream_t s)
{
    const size_t n = (size_t)in.H * in.W;
    const unsigned sblk = (unsigned)((n / fan_sample_stride(n) + 1 + 255) / 256);
    hipLaunchKernelGGL(dl_cell_sample_kernel, dim3(sblk), dim3(256), 0, s, in.flow, in.sign_pp, in.pmask, in.H, in.W, ws.head, ws.bstart,
                       ws.sorted, ws.sorted_xy, ws.dup);
    const int ctx = (in.W + 31) / 32, cty = (in.H + 7) / 8;
    hipLaunchKernelGGL(dl_cell_kernel, dim3((unsigned)((ctx * cty + 7) / 8 * 8)), dim3(256), 0, s, in.flow, in.sign_pp, in.pmask, in.H, in.W,
                       ws.head, ws.bstart, ws.sorted, ws.sorted_xy, ws.dup, ws.cellflag, ws.tileflag, ctx, ctx * cty);
    hipLaunchKernelGGL(dl_site_cells_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in.flow, in.sign_pp, in.pmask, in.H, in.W, ws.head,
                       ws.dup, ws.cellflag, ws.deg, ws.nbr);
}

void stars_fan(const DlIn &in, DlWs &ws, hipStream_t s)
{
    const size_t n = (size_t)in.H * in.W;
    hipLaunchKernelGGL(dl_star_fan_kernel, dim3(std::min<unsigned>((unsigned)((n + kFanBlock - 1) / kFanBlock), 16384u)), dim3(kFanBlock), 0, s,
                       in.flow, in.sign_pp, in.pmask, in.H, in.W, ws.head, ws.todo_idx, ws.bstart, ws.sorted, ws.sorted_xy, ws.dup, ws.deg, ws.nbr);
}

void stars_clip(const DlIn &in, DlWs &ws, hipStream_t s)
{
    const unsigned waves = (unsigned)(((size_t)in.H * in.W + 63) / 64);
    const unsigned *todo = ws.far_idx;                     // BORROWED: far_idx is free until the unfinished points are listed
    auto clip = [&](auto kernel, unsigned max_groups) {
        hipLaunchKernelGGL(kernel, dim3(std::min<unsigned>(waves, max_groups)), dim3(64), 0, s, in.flow, in.sign_pp, in.pmask, ws.dup, in.H, in.W,
                           ws.head, todo, ws.bstart, ws.sorted, ws.sorted_xy, ws.deg, ws.nbr, ws.heavy_bucket, ws.heavy_info, ws.sub_start);
    };
    clip(dl_star_near_kernel<false>, 16384u);
    clip(dl_star_near_kernel<true>, 2048u);
}

void stars_near2(const DlIn &in, DlWs &ws, hipStream_t s)
{
    // (experiments build only) OFL_DL_NEAR2_MIN = 0 runs the per-thread pass on the smallest field: tests/test_gpu_scatter_exact.py
    const unsigned near2_min = (unsigned)OFL_KNOB_INT("OFL_DL_NEAR2_MIN", (int)kNear2MinPoints);
    const unsigned waves = (unsigned)(((size_t)in.H * in.W + 63) / 64);
    hipLaunchKernelGGL(dl_star_near2_kernel, dim3(std::min<unsigned>(waves, 8192u)), dim3(64), 0, s, in.flow, in.sign_pp, in.H, in.W,
                       ws.head, ws.far_idx, ws.bstart, ws.sorted, ws.sorted_xy, ws.b1start, ws.sorted1_pt, ws.sorted1_xy,
                       ws.deg, ws.nbr, ws.far_deg, ws.far_wide, near2_min, ws.heavy_bucket, ws.heavy_info, ws.sub_start);
}

}  // namespace ofl_dlw
