// ofl_delaunay.hip -- K3 exact path: a real Delaunay triangulation of the warped points on the GPU.
//
// Replaces scipy.interpolate.griddata(points, values, grid, 'linear') (src/oflibnumpy/utils.py:253) for every field
// whose cell-wise mesh is NOT provably the Delaunay triangulation (ofl_scatter_walk.hip certifies the others):
// folded meshes (motion boundaries, the tiled Sintel field of BASELINE config 5 as loaded), dropped points (holes and
// speckle of the point mask), curved mesh borders (pockets between the mesh and its convex hull), sheared cells.
//
//   bin      the kept points are counting-sorted into a bucket grid over their bounding box (~1 point per bucket); exact
//            duplicates of a site are dropped (the smallest index of a location stays)
//   stars    four passes, cheapest first (ofl_delaunay_core.h holds the geometry, shared with the CPU test build):
//            mesh fans   one thread per point VERIFIES the star the warped grid proposes (empty circumcircles against the
//                        sites of the buckets under them) -- the interior of every smooth piece of the field;
//            clip        one thread per remaining point builds its Voronoi cell by half-plane clipping in growing bucket
//                        rings (in-circle decisions, security radius);
//            rims        cells that are not final within the rings -- rims of tears and holes -- against a coarse grid of
//                        the unfinished points only: per thread when there are tens of thousands, one wave per point else;
//            hull        what is still left (unbounded cells) by one workgroup per point against all other left-over
//                        points (every Delaunay neighbour of an unfinished point beyond the ring search is itself unfinished)
//   raster   every star's triangles (p, n_k, n_k+1) are scan-converted with SciPy's inclusion rule; atomicMin keeps
//            the smallest triangle id per node -- each triangle is emitted by all three of its sites, so stars that
//            disagree on an exactly co-circular cell (where Qhull itself is arbitrary) still tile the hull
//   resolve  float64 barycentric interpolation from the owner triangle, vertices in canonical order so that all
//            copies of a triangle give the same bits; nodes without an owner are outside the convex hull (NaN -> 0)
//
// Everything is a pure function of the inputs (buckets are sorted by point index, far points are compacted in
// index order, triangle ids derive from point indices), so row bands concatenate to the full result bit for bit.
//
// The kernels live in one file per stage; this file strings the stages together (exact_stars, exact_finish) and holds the
// entries ofl_scatter_dev.h declares and the exchange of the slab mode:
//   ofl_delaunay_ws.h        constants, device header, workspace and its layout, the stages' entry points with what each reads,
//                            writes and borrows
//   ofl_delaunay_dev.h       device helpers of more than one stage
//   ofl_delaunay_bin.hip     bin; the scans and the ordered compaction behind every list
//   ofl_delaunay_stars.hip   stars: mesh cells, mesh fans, clip, second per-thread pass
//   ofl_delaunay_far.hip     stars: rims (wave pass) and hull (left-over passes)
//   ofl_delaunay_raster.hip  raster, resolve, query positions
#include "ofl_delaunay_dev.h"
#include <limits>

using namespace ofl;
using namespace ofl_sc;
using namespace ofl_dl;
using namespace ofl_dlw;

namespace {

// ------------------------------------------------------------------------------------------------ slab mode: the exchange
// BASELINE config 5 ('s' at 4320 x 7680) over several GPUs: rank r builds the cell / fan / clip stars of ITS slab only (the
// bulk of the time), the ranks exchange the sites those passes left unfinished -- tens of thousands out of tens of millions --
// and every rank finishes ALL of them, since the later passes search nothing but the unfinished sites beyond the fine rings
// (a Delaunay neighbour of an unfinished site out there is itself unfinished) and a triangle of such a site can cross any
// band.  List layout: word 0 = entries, word 1 = the rank's error bits, words 2 - 3 = 0, then one neighbour row (kSlots
// words: seeds as the clip pass left them) per unfinished site with the site's index in slot 0 (which holds nothing yet).
constexpr unsigned kSlabHead = 4;

__global__ __launch_bounds__(256)
void dl_slab_emit_kernel(const float *__restrict__ flow, int sign, int W, size_t n, const DlHead *__restrict__ head,
                         const unsigned char *__restrict__ deg, const unsigned *__restrict__ nbr, double own_lo, double own_hi,
                         unsigned *__restrict__ list, unsigned cap)
{
    const PosFn pos(flow, sign, W);
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        if (deg[p] != kDegFar) continue;
        const P2 q = pos((int)p);
        if (!(q.y >= own_lo && q.y < own_hi)) continue;             // another rank's to report (the bands tile the real line)
        const unsigned slot = atomicAdd(&list[0], 1u);
        if (slot >= cap) continue;                                  // (the reader sees entries > capacity)
        const uint4 *src = reinterpret_cast<const uint4 *>(nbr + p * kSlots);
        uint4 *dst = reinterpret_cast<uint4 *>(list + kSlabHead + (size_t)slot * kSlots);
        uint4 r0 = src[0];
        r0.x = (unsigned)p;
        dst[0] = r0; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && head->err) atomicOr(&list[1], head->err);
}

__global__ __launch_bounds__(256)
void dl_slab_absorb_kernel(DlHead *__restrict__ head, const unsigned *__restrict__ lists, size_t stride_words, int n_lists, unsigned cap,
                           size_t n, unsigned char *__restrict__ deg, unsigned *__restrict__ nbr)
{
    for (int r = 0; r < n_lists; ++r) {
        const unsigned *list = lists + (size_t)r * stride_words;
        const unsigned total = list[0], cnt = total < cap ? total : cap;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const unsigned e = list[1] | (total > cap ? kErrSlabList : 0u);
            if (e) atomicOr(&head->err, e);
        }
        for (unsigned k = blockIdx.x * 256 + threadIdx.x; k < cnt; k += gridDim.x * 256) {
            const uint4 *src = reinterpret_cast<const uint4 *>(list + kSlabHead + (size_t)k * kSlots);
            const uint4 r0 = src[0];
            const size_t p = r0.x;
            // not a list of this field?  (the later passes take positions from the seeds' site numbers: none may leave the field)
            const uint4 r1 = src[1], r2 = src[2], r3 = src[3];
            const unsigned sd[12] = { r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y };
            const unsigned ns = r0.y < (unsigned)(kSlots - 4) ? r0.y : (unsigned)(kSlots - 4);
            bool bad = p >= n;
#pragma unroll
            for (unsigned k2 = 0; k2 < (unsigned)(kSlots - 4); ++k2) bad = bad || (k2 < ns && sd[k2] >= n && sd[k2] < 0xFFFFFFFCu);      // (-1 .. -4: box sides)
            if (bad) { atomicOr(&head->err, kErrSlabList); continue; }
            deg[p] = kDegFar;
            uint4 *dst = reinterpret_cast<uint4 *>(nbr + p * kSlots);
            dst[0] = r0; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
        }
    }
}

// Bins and the stars that cells, fans and the clip pass settle; what they leave is marked kDegFar with its seeds.
// `slab`: only for the sites within kSlabMargin buckets of rows [row0, row0 + rows) -- every triangle that reaches those rows
// has ALL its vertices there or is a triangle of an unfinished site: a finished star's neighbours lie within kRings + 1
// buckets of its site per axis (clip pass: a cell is final only when twice its reach is covered by the rings searched; cells
// and fans: circumcircles within kFanSpan buckets), so a triangle with one finished vertex spans at most 2 (kRings + 1) bucket
// rows.  The copy of a triangle that is drawn is the one of its smallest-index vertex -- whose star is therefore built here
// whenever the triangle matters, with the same neighbour order as in a whole-field run (the passes read the bins of ALL
// sites either way): owner ids, and with them every tie on a shared edge, come out the same.
int exact_stars(const DlIn &in, int row0, int rows, bool slab, void *workspace, size_t workspace_bytes, hipStream_t s, DlWs &ws)
{
    const size_t n = (size_t)in.H * in.W;
    if (n >= (1ull << 27)) return fail(OFL_E_INVALID, "ofl_scatter_linear: the exact path takes fields below 2^27 pixels");
    if (workspace_bytes < ofl_sc::exact_workspace_bytes(in.H, in.W)) return fail(OFL_E_INVALID, "ofl_scatter_linear: workspace too small for the exact path");
    ws = carve_band(workspace, in.H, in.W, row0, rows);
    OFL_HIP(hipMemsetAsync(ws.owner + (size_t)row0 * in.W, 0xFF, (size_t)rows * in.W * 4, s));
    DlHead init;
    memset(&init, 0, sizeof(init));
    init.kx0 = init.ky0 = ~0ull;
    OFL_HIP(hipMemcpyAsync(ws.head, &init, sizeof(init), hipMemcpyHostToDevice, s));
    OFL_TRY(bin_sites(in, ws, s, slab, row0, rows));
    OFL_TRY(compact_reset(ws, kListFan, kListTodo, s));
    OFL_TRY(bin_clusters(in, ws, s));
    // mesh cells (one verification per triangle), the sites they settle, then the fans of the rest (compacted in index order)
    stars_mesh(in, ws, s);
    compact_list(kListFan, in, ws, s);
    stars_fan(in, ws, s);
    // what cells and fans did not settle, in index order, for the clip pass
    compact_list(kListTodo, in, ws, s);
    stars_clip(in, ws, s);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

// The unfinished sites in index order, their stars (second per-thread pass, wave pass, workgroup pass) and the owner map
// of rows [row0, row0 + rows).  Asynchronous unless the caller asks for the counts.
int exact_finish(const DlIn &in, int row0, int rows, uint64_t *info_host, hipStream_t s, DlWs &ws, unsigned &far_base_out,
                 int &late_error)      // OFL_E_NOPOINTS / capacity errors known only after the fact: the owner map is complete (empty) all the same
{
    late_error = OFL_OK;
    // unfinished points in index order
    OFL_TRY(compact_reset(ws, kListFar, kListLeft, s));
    OFL_TRY(compact_reset(ws, kListRaster, kListRaster, s));
    compact_list(kListFar, in, ws, s);
    OFL_HIP(hipGetLastError());
    // From here on every launch is sized on the device: fixed grids walk the unfinished points, whose numbers stay in the
    // header.  Nothing is read back unless the caller asks for the counts (info_host) -- then ONE read-back at the end,
    // which also carries the errors that cannot be known earlier (no point kept, a capacity exceeded).
    const unsigned far_base = (unsigned)((unsigned long long)in.H * in.W * kSlots);
    // coarse grid of the unfinished points, per-thread / wave pass, then the workgroup pass for what is still left
    OFL_TRY(bin_unfinished(in, ws, s));
    stars_near2(in, ws, s);
    stars_rim(in, ws, s);
    OFL_HIP(hipGetLastError());
    compact_list(kListLeft, in, ws, s);
    bin_leftover(in, ws, s);
    stars_leftover(in, ws, s);
    OFL_HIP(hipGetLastError());
    raster_cells(in, ws, s, far_base);
    compact_list(kListRaster, in, ws, s);
    raster_sites(in, ws, s, far_base);
    far_base_out = far_base;
    OFL_HIP(hipGetLastError());
    if (info_host) {
        DlHead h;
        OFL_HIP(hipMemcpyAsync(&h, ws.head, sizeof(h), hipMemcpyDeviceToHost, s));
        OFL_HIP(hipStreamSynchronize(s));
        info_host[0] = h.kept; info_host[1] = h.n_far; info_host[2] = h.n_left;
        if (h.err) {
            // a capacity or degeneracy error leaves SOME stars rasterised: blank the owner map, so that the result is what
            // include/ofl.h promises for an error -- all zero, all invalid -- rather than a partial warp
            OFL_HIP(hipMemsetAsync(ws.owner + (size_t)row0 * in.W, 0xFF, (size_t)rows * in.W * 4, s));
        }
        if (h.kept == 0) late_error = fail(OFL_E_NOPOINTS, "ofl_scatter_linear: no valid source points");
        else if (h.err) late_error = fail(OFL_E_INVALID, "ofl_scatter_linear: exact path capacity exceeded (flags %u: 1 = star of more than %d "
                                              "neighbours, 2 = neighbour pool, 4 = large-triangle list, 8 = unfinished stars beyond the "
                                              "triangle-id space, 16 = degenerate point set: thousands of coincident points or hundreds of "
                                              "thousands of unbounded cells; 32 = slab mode: a rank's list of unfinished sites exceeded its buffer)", h.err, kFarCap);
    }
    return OFL_OK;
}

// Bins, stars and the owner map of rows [row0, row0 + rows) in one go (every star of the field: one GPU, or replicated ranks).
int exact_prepare(const DlIn &in, int row0, int rows, void *workspace, size_t workspace_bytes, uint64_t *info_host, hipStream_t s,
                  DlWs &ws, unsigned &far_base_out, int &late_error)
{
    late_error = OFL_OK;
    OFL_TRY(exact_stars(in, row0, rows, false, workspace, workspace_bytes, s, ws));
    return exact_finish(in, row0, rows, info_host, s, ws, far_base_out, late_error);
}

}  // namespace

namespace ofl_sc {

size_t exact_workspace_bytes(int H, int W)
{
    size_t total = 0;
    (void)carve_exact(nullptr, H, W, &total);
    return total;
}

// rows [row0, row0 + rows) of the grid result through the exact path
template <typename VT>
int exact_scatter(const float *flow, int sign_pp, const uint8_t *pmask, const VT *vals, int C, const uint8_t *vmask,
                  int H, int W, int row0, int rows, VT *out, uint8_t *valid, int valid_rule,
                  void *workspace, size_t workspace_bytes, uint64_t *info_host, hipStream_t s)
{
    const DlIn in{ flow, sign_pp, pmask, H, W };
    DlWs ws;
    unsigned far_base = 0;
    int late = OFL_OK;
    OFL_TRY(exact_prepare(in, row0, rows, workspace, workspace_bytes, info_host, s, ws, far_base, late));
    // (the outputs are written even when the call reports no points / a refused point set: all zero, all invalid)
    resolve_rows<VT>(in, ws, s, far_base, vals, C, vmask, row0, rows, out, valid, valid_rule);
    OFL_HIP(hipGetLastError());
    return late;
}

// arbitrary positions through the exact path (see walk_query_launch for the two layouts)
int exact_query(const float *flow, int sign_pp, const uint8_t *pmask, const float *vals, int C, const uint8_t *vmask,
                int H, int W, const void *query, size_t n, bool sparse, void *out, uint8_t *valid, int valid_rule,
                void *workspace, size_t workspace_bytes, uint64_t *info_host, hipStream_t s)
{
    const DlIn in{ flow, sign_pp, pmask, H, W };
    DlWs ws;
    unsigned far_base = 0;
    int late = OFL_OK;
    OFL_TRY(exact_prepare(in, 0, H, workspace, workspace_bytes, info_host, s, ws, far_base, late));
    if (n == 0) return late;
    query_points(in, ws, s, far_base, vals, C, vmask, query, n, sparse, out, valid, valid_rule);
    OFL_HIP(hipGetLastError());
    return late;
}

// slab mode, step 1: the stars of the slab around rows [row0, row0 + rows) and the list of the unfinished sites this rank
// reports (those whose position lies in [row0, row0 + rows); the first band is open towards -inf, the last towards +inf)
int exact_slab_stars(const float *flow, int sign_pp, const uint8_t *pmask, int H, int W, int row0, int rows,
                     uint32_t *list, size_t list_bytes, void *workspace, size_t workspace_bytes, hipStream_t s)
{
    if (list_bytes < (kSlabHead + kSlots) * 4) return fail(OFL_E_INVALID, "ofl_scatter_slab_stars: list buffer too small");
    const DlIn in{ flow, sign_pp, pmask, H, W };
    DlWs ws;
    OFL_TRY(exact_stars(in, row0, rows, true, workspace, workspace_bytes, s, ws));
    const size_t n = (size_t)H * W;
    const size_t cap = std::min<size_t>((list_bytes / 4 - kSlabHead) / kSlots, 0xFFFFFFFFu);
    const double inf = std::numeric_limits<double>::infinity();
    OFL_HIP(hipMemsetAsync(list, 0, kSlabHead * 4, s));
    hipLaunchKernelGGL(dl_slab_emit_kernel, dim3(std::min<unsigned>((unsigned)((n + 255) / 256), 4096u)), dim3(256), 0, s, flow, sign_pp, W, n,
                       ws.head, ws.deg, ws.nbr, row0 <= 0 ? -inf : (double)row0, row0 + rows >= H ? inf : (double)(row0 + rows), list, (unsigned)cap);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

// slab mode, step 2: the lists of ALL ranks (this rank's included; `n_lists` buffers of `stride_bytes` each, as an all-gather
// leaves them) are merged into the star state step 1 left in `workspace`; then the unfinished stars, the owner map and the
// result of the band, exactly as a whole-field call produces them.
int exact_slab_finish(const float *flow, int sign_pp, const float *vals, int C, const uint8_t *vmask, int H, int W, int row0, int rows,
                      const uint32_t *lists, size_t stride_bytes, int n_lists, float *out, uint8_t *valid, int valid_rule,
                      void *workspace, size_t workspace_bytes, uint64_t *info_host, hipStream_t s)
{
    if (workspace_bytes < exact_workspace_bytes(H, W)) return fail(OFL_E_INVALID, "ofl_scatter_slab_finish: workspace too small");
    if (n_lists < 1 || stride_bytes % 16 || stride_bytes < (kSlabHead + kSlots) * 4)
        return fail(OFL_E_INVALID, "ofl_scatter_slab_finish: bad list layout");
    const DlIn in{ flow, sign_pp, nullptr, H, W };          // (no pass of step 2 looks at the point mask)
    DlWs ws = carve_band(workspace, H, W, row0, rows);
    const size_t n = (size_t)H * W;
    const size_t cap = std::min<size_t>((stride_bytes / 4 - kSlabHead) / kSlots, 0xFFFFFFFFu);
    {   // Is this the state step 1 left for THIS band?  Everything below trusts the lists and counts in the workspace: a
        // foreign one must not reach a kernel.  (One 4-byte read-back; the call synchronises at its end anyway.  The stamp is
        // cleared right away: a state is finished once.)
        unsigned stamp = 0;
        OFL_HIP(hipMemcpyAsync(&stamp, &ws.head->slab_stamp, 4, hipMemcpyDeviceToHost, s));
        OFL_HIP(hipStreamSynchronize(s));
        if (stamp != slab_stamp_of(H, W, row0, rows)) {
            if (C > 0) OFL_HIP(hipMemsetAsync(out, 0, (size_t)rows * W * C * sizeof(float), s));
            if (valid) OFL_HIP(hipMemsetAsync(valid, 0, (size_t)rows * W, s));
            return fail(OFL_E_INVALID, "ofl_scatter_slab_finish: the workspace does not hold the state ofl_scatter_slab_stars_dev left for rows "
                                       "[%d, %d) (another call used it in between, or step 1 ran for another band)", row0, row0 + rows);
        }
        OFL_HIP(hipMemsetAsync(&ws.head->slab_stamp, 0, 4, s));
    }
    hipLaunchKernelGGL(dl_slab_absorb_kernel, dim3(256), dim3(256), 0, s, ws.head, lists, stride_bytes / 4, n_lists, (unsigned)cap, n, ws.deg, ws.nbr);
    OFL_HIP(hipGetLastError());
    unsigned far_base = 0;
    int late = OFL_OK;
    uint64_t info_local[3];
    // (always read the counts back: an error bit another rank raised must blank this band too, and the exchange has
    // synchronised the ranks a moment ago anyway)
    OFL_TRY(exact_finish(in, row0, rows, info_host ? info_host : info_local, s, ws, far_base, late));
    resolve_rows<float>(in, ws, s, far_base, vals, C, vmask, row0, rows, out, valid, valid_rule);
    OFL_HIP(hipGetLastError());
    return late;
}

template int exact_scatter<float>(const float *, int, const uint8_t *, const float *, int, const uint8_t *, int, int, int, int,
                                  float *, uint8_t *, int, void *, size_t, uint64_t *, hipStream_t);
template int exact_scatter<double>(const float *, int, const uint8_t *, const double *, int, const uint8_t *, int, int, int, int,
                                   double *, uint8_t *, int, void *, size_t, uint64_t *, hipStream_t);

}  // namespace ofl_sc
