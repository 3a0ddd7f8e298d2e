// ofl_delaunay_ws.h -- what the stage files of the K3 exact path (ofl_delaunay*.hip) share on the host side: the tuning
// constants, the device header, the workspace and where its parts lie, and the entry points of the stages.  Everything up
// to the entry points is plain host arithmetic, nothing of HIP: tests/native/dl_layout_cpu.cpp compiles it with plain g++.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "ofl_delaunay_core.h"
#if defined(__HIPCC__)
#include "ofl_scatter_dev.h"
#endif

namespace ofl_dlw {

using ofl_dl::Grid;
using ofl_dl::P2;
using ofl_dl::SubGrid;
using ofl_dl::kHeavy;

constexpr int      kRings    = 6;        // bucket rings of the per-thread star pass
constexpr int      kOpenRings = 2;       // ... of which a cell still unbounded after this many is handed on at once
constexpr int      kNearCap  = 10;       // polygon capacity of the per-thread pass (float32 cell in LDS)
constexpr int      kSlots    = 16;       // neighbour slots per point
constexpr int      kNear2Rings = 6;      // coarse rings of the second per-thread pass ...
constexpr unsigned kNear2MinPoints = 32768;   // unfinished points below which the second per-thread pass is skipped
constexpr int      kNear2Open = 3;       // ... which gives up a cell that is still unbounded after this many
constexpr int      kMidCap   = 256;      // polygon capacity of the wave pass (unfinished points against the coarse grid of unfinished points)
constexpr int      kMidRings = 8;        // rings of that coarse grid every unfinished point is given ...
constexpr int      kMidRingsMax = 160;   // ... and the rings a BOUNDED cell may go on for (rims of large holes) before it is left to the workgroup pass
constexpr double   kFarBuckets = 256.0;  // far threshold of the cooperative cells, in buckets (dl_params_kernel)
constexpr int      kFarList  = 48;       // cell vertices beyond the data (unbounded directions, sliver fans of a straight border) tested one by one
constexpr int      kMidScale = 8;        // ... whose cells are this many fine buckets wide
constexpr int      kFarCap   = 2560;     // polygon capacity of the workgroup pass (LDS: 20 B per vertex)
constexpr unsigned kDegLeft  = 0xFFFFFFFFu;   // far_deg marker: not finished by the wave pass
constexpr unsigned kFarK     = 4096;     // triangle-id stride of a far point (>= kFarCap)
constexpr unsigned kNoOwner  = 0xFFFFFFFFu;
constexpr int      kSmallArea = 1024;
constexpr int      kLocateRings = 2;     // bucket rings dl_locate_brute searches when the visibility walk got stuck
constexpr unsigned char kDegFar = 0xFF;
constexpr unsigned char kDegTodo = 0xFE;  // not settled by the mesh-fan pass: the clip pass builds this star
constexpr unsigned char kDegFan = 0xFD;   // not settled by the mesh-cell pass: the fan pass looks at this site
constexpr unsigned char kDegHeavy = 0xFC; // the clip pass met a dense cluster around this site: the heavy-bucket launch of the clip pass builds this star
constexpr int      kFanSpan  = 6;        // buckets per axis a fan's circumcircles may span (wider: clip pass)
constexpr int      kFanBlock = 128;
constexpr unsigned kDedupeSmall = 64;     // buckets up to this size drop their duplicates by pairwise comparison (quadratic, one thread), larger ones through a hash table
constexpr unsigned kMaxFar   = 1u << 20;  // unfinished stars ...
constexpr unsigned kMaxLeft  = 1u << 18;  // ... and stars for the workgroup pass (quadratic in their number) before the call gives up
constexpr unsigned kErrDegenerate = 16u;  // err bit: one of the three limits above -- Qhull, too, refuses such input ("initial simplex is flat")
constexpr unsigned kErrSlabList = 32u;    // err bit (slab mode): a rank's list of unfinished sites did not fit the buffer the caller gave it, or is not a list of this field
constexpr int      kSlabMargin = 2 * (kRings + 1) + 2;   // buckets around a row band within which the slab mode builds every star (see exact_stars)
constexpr int      kScanChunk = 2048;    // elements per block of the scan kernels (256 threads x 8)

struct DlHead {                           // device header of the exact path (256 bytes)
    unsigned long long kx0, kx1, ky0, ky1;   // ordered keys of the bounding box while it is reduced
    Grid     grid, grid1;                    // fine buckets (all kept points), coarse buckets (unfinished points)
    unsigned kept, n_far, n_left, pool_used, err;    // err bit 0: far polygon overflow, bit 1: pool overflow, bit 2: big list overflow, bit 3: triangle-id space
    unsigned long long big_n;
    unsigned n_todo;                                 // points the mesh-fan pass left to the clip pass
    unsigned n_fan;                                  // points the mesh-cell pass left to the fan pass
    double   far_t2;                                 // squared distance beyond which a cell vertex counts as "far" (well outside the data)
    unsigned n_big;                                  // sorted entries that live in buckets of more than kDedupeSmall entries
    unsigned any_heavy;                              // some bucket holds more than kHeavy entries (else the heavy-bucket passes return at once)
    double   need_lo, need_hi;                       // slab mode: only sites with need_lo <= y <= need_hi get a star from cells / fans / clip (else -inf, +inf)
    unsigned slab_stamp;                             // slab mode: slab_stamp_of(field, band) step 1 ran for (0: not a slab state)
    unsigned sample_all, sample_ok;                  // dl_cell_sample_kernel: sampled grid cells with four kept corners / of those, verified
    unsigned n_raster;                               // sites the site-wise raster looks at (stars of 1 .. kSlots neighbours outside the clean tiles)
    unsigned n_heavy;                                // buckets of more than kHeavy entries (dense clusters): they get grids of their own
    unsigned sub_used;                               // words of DlWs::sub_start handed out to those grids
};
static_assert(sizeof(DlHead) <= 256, "DlHead");
#if defined(__HIPCC__)                    // (the constant lives with the device helpers: every build of the library checks it)
static_assert(offsetof(DlHead, slab_stamp) == ofl_sc::kSlabStampAt, "ofl_scatter_dev.h: kSlabStampAt");
#endif

// The six lists of the path, each made by ONE ordered compaction (dl_compact_kernel<LIST>, ofl_delaunay_bin.hip: compact_list);
// list K keeps its ticket and tile words in slot K of DlWs::cstate.  (Plain ints, not an enum: they are the kernel's
// template argument.)      elements kept, in ascending order               -> destination                  count
constexpr int kListFar    = 0;   // points with deg == kDegFar                  -> far_idx; rank -> nbr slot 0  head->n_far
constexpr int kListLeft   = 1;   // ranks with far_deg == kDegLeft, or far_wide -> left_idx                     head->n_left
constexpr int kListFan    = 2;   // points with deg == kDegFan                  -> todo_idx                     head->n_fan
constexpr int kListTodo   = 3;   // points with deg == kDegTodo                 -> far_idx (borrowed)           head->n_todo
constexpr int kListRaster = 4;   // points with a star of 1 .. kSlots neighbours outside the clean tiles -> todo_idx (borrowed)   head->n_raster
constexpr int kListHeavy  = 5;   // buckets of more than kHeavy entries         -> heavy_bucket                 head->n_heavy
constexpr int kLists      = 6;

struct DlWs {
    DlHead   *head;
    unsigned *bstart;      // [bcap + 1] counts -> exclusive starts
    unsigned *scan_tmp;    // block sums of the scan levels
    unsigned *sorted;      // [N] point indices bucket by bucket
    unsigned char *deg;    // [N] 0 .. 16, kDegTodo, kDegFar
    unsigned *todo_idx;    // [N] points for the fan pass (what the cell pass did not settle), ascending
    unsigned char *cellflag; // [N] per grid cell (x, y): 0 = not verified, 1 / 2 = both triangles Delaunay, diagonal a - c / b - d (ofl_dl::cell_verify)
    unsigned char *tileflag; // [ceil(W / 32) * ceil(H / 8)] 1 = every cell of the 32 x 8 tile is verified (a CLEAN tile)
    unsigned char *dup;    // [N] 1 = an exact duplicate of a site with a smaller index (not a site of the triangulation)
    unsigned *nbr;         // [N][kSlots]
    unsigned *far_idx;     // [N]
    unsigned *far_deg;     // [N]
    unsigned *far_off;     // [N]
    unsigned char *far_wide; // [N] 1 = finished by the wave pass BEYOND the coarse rings the workgroup pass searches: stays a candidate of its sweeps
    unsigned *left_idx;    // [N] ranks of the points the wave pass could not finish
    unsigned *b1start;     // [b1cap + 1] coarse buckets of the unfinished points
    unsigned *b1cursor;    // [b1cap]
    unsigned *sorted1;     // [N] their ranks bucket by bucket
    P2       *sorted_xy;   // [N] positions in `sorted` order
    P2       *sorted1_xy;  // [N] positions in `sorted1` order
    unsigned *sorted1_pt;  // [N] point indices in `sorted1` order
    P2       *left_xy;     // [N] positions of the left-over points, in left_idx order
    unsigned *left_pt;     // [N] their point indices
    double   *left_box;    // [N / 256 + 1][2][8] oriented boxes of the two image halves of 256 consecutive left-over points
    int      *pool;        // [pool_cap] neighbour lists of the far points (negative: unbounded gap)
    unsigned *cstate;      // [kLists][cstride] ticket + tile words of the ordered compactions (dl_compact_kernel)
    unsigned *heavy_bucket; // [heavy_cap] numbers of the buckets of more than kHeavy entries, ascending
    SubGrid  *heavy_info;  // [heavy_cap] their grids
    unsigned *sub_start;   // [sub_cap] cell starts of those grids (absolute positions in `sorted`)
    unsigned *big;         // [big_cap] triangle ids with a large bounding box
    uint32_t *owner;       // [H][W] (biased by the first row of the band)
    size_t    bcap, b1cap, pool_cap, big_cap, cstride, heavy_cap, sub_cap;
    int       oy0, oy1;
};

// what every pass reads of the call: the field, its sign with the point precision folded in (+-1 / +-2), the point mask (or NULL)
struct DlIn { const float *flow; int sign_pp; const uint8_t *pmask; int H, W; };

// ------------------------------------------------------------------------------------------------ workspace layout
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline size_t scan_tmp_elems(size_t n)
{
    size_t t = 0;
    while (n > 8192) { n = (n + 8191) / 8192; t += (n + 63) / 64 * 64; }
    return t + 64;
}

struct Sizes { size_t n, bcap, b1cap, pool_cap, big_cap; };

inline Sizes sizes_for(int H, int W)
{
    Sizes z;
    z.n = (size_t)H * W;
    z.bcap = z.n + z.n / 4 + 4096;  // ~ one site per bucket needs n + O(sqrt n) buckets; dl_params_kernel widens the buckets of a point set
                                    // whose shape would need more (2 n + 1 in the worst case: all sites on one slanted line)
    z.b1cap = z.bcap / 6 + 64;      // ceil(gx / 8) * ceil(gy / 8) <= gx gy / 64 + (gx + gy) / 8 + 1 with gx gy <= bcap, gx + gy <= bcap + 1
    z.pool_cap = 8 * z.n + 65536;
    z.big_cap = 6 * z.n + 1024;
    return z;
}

// one part as carve_exact laid it out: `bytes` is what it holds, its slot runs on to the next 256-byte boundary
struct DlPart { const char *name; size_t offset, bytes; };

// The workspace of a field of H x W points, part by part (about 235 bytes per point): every part starts on a 256-byte
// boundary, in the order of the table below; `total` receives the bytes ofl_scatter_workspace_bytes promises for the path,
// `parts` the table itself.  No offset may move: step 1 of the slab mode leaves its state here for step 2, which carves again.
inline DlWs carve_exact(void *base, int H, int W, size_t *total = nullptr, std::vector<DlPart> *parts = nullptr)
{
    const Sizes z = sizes_for(H, W);
    const size_t n = z.n;
    DlWs ws;
    size_t at = 0;
    auto take = [&](auto *&member, const char *name, size_t count) {      // `count` elements of the member's type at the next boundary
        const size_t bytes = count * sizeof(*member);
        member = reinterpret_cast<decltype(+member)>(reinterpret_cast<uintptr_t>(base) + at);
        if (parts) parts->push_back(DlPart{ name, at, bytes });
        at += align_up(bytes, 256);
    };
    ws.bcap = z.bcap; ws.b1cap = z.b1cap; ws.pool_cap = z.pool_cap; ws.big_cap = z.big_cap;
    ws.cstride = align_up(std::max(n, ws.bcap) / kScanChunk + 5, 64);
    ws.heavy_cap = n / kHeavy + 64;         // (a heavy bucket holds more than kHeavy of the n entries)
    ws.sub_cap = n + ws.heavy_cap + 64;     // (a grid of K x K cells for m entries: K = ceil(sqrt(m / 2)), K * K + 1 <= m for m > kHeavy)
    take(ws.head,         "head",         1);
    take(ws.bstart,       "bstart",       ws.bcap + 1);
    take(ws.scan_tmp,     "scan_tmp",     scan_tmp_elems(ws.bcap + 1));
    take(ws.sorted,       "sorted",       n);
    take(ws.deg,          "deg",          n);
    take(ws.todo_idx,     "todo_idx",     n);
    take(ws.cellflag,     "cellflag",     n);
    take(ws.tileflag,     "tileflag",     (size_t)((W + 31) / 32) * ((H + 7) / 8));
    take(ws.dup,          "dup",          n);
    take(ws.nbr,          "nbr",          n * kSlots);
    take(ws.far_idx,      "far_idx",      n);
    take(ws.far_deg,      "far_deg",      n);
    take(ws.far_off,      "far_off",      n);
    take(ws.far_wide,     "far_wide",     n);
    take(ws.left_idx,     "left_idx",     n);
    take(ws.b1start,      "b1start",      ws.b1cap + 1);
    take(ws.b1cursor,     "b1cursor",     ws.b1cap);
    take(ws.sorted1,      "sorted1",      n);
    take(ws.sorted_xy,    "sorted_xy",    n);
    take(ws.sorted1_xy,   "sorted1_xy",   n);
    take(ws.sorted1_pt,   "sorted1_pt",   n);
    take(ws.left_xy,      "left_xy",      n);
    take(ws.left_pt,      "left_pt",      n);
    take(ws.left_box,     "left_box",     (n / 256 + 1) * 16);
    take(ws.pool,         "pool",         ws.pool_cap);
    take(ws.cstate,       "cstate",       kLists * ws.cstride);
    take(ws.heavy_bucket, "heavy_bucket", ws.heavy_cap);
    take(ws.heavy_info,   "heavy_info",   ws.heavy_cap);
    take(ws.sub_start,    "sub_start",    ws.sub_cap);
    take(ws.big,          "big",          ws.big_cap);
    take(ws.owner,        "owner",        n);
    ws.oy0 = 0; ws.oy1 = H;
    if (total) *total = at;
    return ws;
}

// the workspace of a call that produces rows [row0, row0 + rows): `owner` is indexed by the field's own row numbers
inline DlWs carve_band(void *workspace, int H, int W, int row0, int rows)
{
    DlWs ws = carve_exact(workspace, H, W);
    ws.oy0 = row0; ws.oy1 = row0 + rows;
    ws.owner -= (size_t)row0 * W;
    return ws;
}

inline unsigned walk_groups(size_t n) { return (unsigned)std::min<size_t>(n, 16384); }      // workgroups of the passes that walk ranks

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------ the stages
// The host side of every stage: exactly its launches and memsets, in stream order; ofl_delaunay.hip strings them together.
// For each: the DlWs members it READS (written by an earlier stage), WRITES, and BORROWS as scratch from the stage that owns
// them -- the contract that breaks silently when a pass moves.  DlHead fields are named where another stage depends on them.
// The int-returning ones report a failed HIP call (OFL_E_HIP); the others only launch, and the driver polls the launch
// errors where it always did.

// ---- ofl_delaunay_bin.hip
// Bounding box, grid parameters, the counting sort of all kept points into the fine buckets, exact duplicates dropped.
//   reads    --  (the header as exact_stars initialised it)
//   writes   head (kept, grid, grid1, far_t2, need_lo / need_hi, slab_stamp, n_big, any_heavy), bstart, scan_tmp, dup, sorted,
//            sorted_xy
//   borrows  pool      from the cooperative star passes (stars_rim, stars_leftover), free until they run: first the
//                      bounding-box partials of dl_bbox_kernel (40 bytes per workgroup in 8 n + 65 536 words), then the
//                      hash table of the dl_big_* kernels
//            todo_idx  from the fan pass (its list, kListFan), free until the cells are done: the slot every site drew in
//                      its bucket, dl_count_kernel -> dl_fill_kernel
int bin_sites(const DlIn &in, DlWs &ws, hipStream_t s, bool slab, int row0, int rows);

// Dense clusters: the buckets of more than kHeavy entries get grids of their own (two launches that return at once without
// such a bucket).
//   reads    head (any_heavy, grid), bstart
//   writes   cstate[kListHeavy], heavy_bucket, head (n_heavy, sub_used), heavy_info, sub_start; sorted and sorted_xy are
//            re-ordered inside the heavy buckets
//   borrows  far_off, far_deg  from the passes over the unfinished points (stars_near2 onwards), free until those points are
//                      listed: dl_sub_bin_kernel's scratch for point indices and cell slots
//            left_xy   from bin_leftover, free until then: its scratch for positions
int bin_clusters(const DlIn &in, DlWs &ws, hipStream_t s);

// Zeroes the cstate slots of lists first .. last (one memset): before the first compact_list of each of them.
int compact_reset(DlWs &ws, int first, int last, hipStream_t s);

// One ordered compaction; source, destination and count of each list are in the table above.
//   reads    cstate[list] (zeroed), the list's source: deg | far_deg, far_wide | deg, tileflag | bstart
//   writes   the list's destination and its count in the header; kListFar also the rank of every unfinished point (nbr slot 0)
//   borrows  far_idx   (kListTodo) from kListFar, free until the unfinished points are listed: the clip pass's list
//            todo_idx  (kListRaster) from the fan pass, free again once the fans are done: the site-wise raster's list
void compact_list(int list, const DlIn &in, DlWs &ws, hipStream_t s);

// The same binning for the unfinished points (ranks into far_idx) on the coarse grid.
//   reads    head (n_far, grid1), far_idx
//   writes   b1start, b1cursor, scan_tmp, sorted1, sorted1_xy, sorted1_pt
int bin_unfinished(const DlIn &in, DlWs &ws, hipStream_t s);

// Positions and point indices of the left-over points, in left_idx order.
//   reads    head (n_left), left_idx, far_idx
//   writes   left_xy, left_pt
void bin_leftover(const DlIn &in, DlWs &ws, hipStream_t s);

// ---- ofl_delaunay_stars.hip
// Mesh cells (one verification per triangle) and the sites they settle; the others are marked kDegFan (or kDegTodo).
//   reads    head (grid, need_lo / need_hi, err), bstart, sorted, sorted_xy, dup
//   writes   head (sample_all, sample_ok), cellflag, tileflag, deg, nbr
void stars_mesh(const DlIn &in, DlWs &ws, hipStream_t s);

// Mesh fans of the sites in list kListFan; what does not verify is marked kDegTodo.
//   reads    head (n_fan, grid), todo_idx, bstart, sorted, sorted_xy, dup
//   writes   deg, nbr
void stars_fan(const DlIn &in, DlWs &ws, hipStream_t s);

// Clip pass over list kListTodo, then its second launch for the sites it marked kDegHeavy; unfinished cells are marked
// kDegFar and leave their seeds in the neighbour row.
//   reads    head (n_todo, n_heavy, grid, far_t2), far_idx (as the list kListTodo left it), bstart, sorted, sorted_xy, dup,
//            heavy_bucket, heavy_info, sub_start
//   writes   deg, nbr
void stars_clip(const DlIn &in, DlWs &ws, hipStream_t s);

// Second per-thread pass: unfinished points (not on the image border) against the coarse grid of unfinished points.
//   reads    head (n_far, grid, grid1, far_t2, n_heavy), far_idx, nbr (seeds), bstart, sorted, sorted_xy, b1start, sorted1_pt,
//            sorted1_xy, heavy_bucket, heavy_info, sub_start
//   writes   deg, nbr, far_deg, far_wide
void stars_near2(const DlIn &in, DlWs &ws, hipStream_t s);

// ---- ofl_delaunay_far.hip
// Wave pass: one wave per unfinished point; what it cannot finish is marked kDegLeft.
//   reads    head (n_far, grid, grid1, far_t2), far_idx, deg, nbr (seeds), bstart, sorted, sorted_xy, b1start, sorted1_pt, sorted1_xy
//   writes   far_deg, far_off, far_wide, pool, head (pool_used, err)
void stars_rim(const DlIn &in, DlWs &ws, hipStream_t s);

// Left-over passes: boxes of every 256 left-over points, then single waves with the small cell capacity, then workgroups
// with the large one for the few cells that overflowed it.
//   reads    head (n_left, grid, grid1, far_t2), left_idx, left_pt, left_xy, far_idx, nbr (seeds), bstart, sorted, sorted_xy,
//            b1start, sorted1_pt, sorted1_xy
//   writes   left_box, far_deg, far_off, pool, head (pool_used, err)
void stars_leftover(const DlIn &in, DlWs &ws, hipStream_t s);

// ---- ofl_delaunay_raster.hip
// Cell-wise raster of the clean tiles.
//   reads    tileflag, cellflag
//   writes   owner (rows oy0 .. oy1), big, head (big_n, err)
void raster_cells(const DlIn &in, const DlWs &ws, hipStream_t s, unsigned far_base);

// Site-wise raster of list kListRaster, wave-wise raster of the unfinished points' stars, then the large triangles.
//   reads    head (n_raster, n_far, big_n), todo_idx (as the list kListRaster left it), deg, nbr, cellflag, far_idx, far_deg,
//            far_off, pool, big
//   writes   owner (rows oy0 .. oy1), big, head (big_n, err)
void raster_sites(const DlIn &in, const DlWs &ws, hipStream_t s, unsigned far_base);

// Values and validity of rows [row0, row0 + rows) from the owner map.
//   reads    owner, deg, nbr, far_idx, far_deg, far_off, pool
template <typename VT>
void resolve_rows(const DlIn &in, const DlWs &ws, hipStream_t s, unsigned far_base, const VT *vals, int C, const uint8_t *vmask,
                  int row0, int rows, VT *out, uint8_t *valid, int valid_rule);

// Values and validity at arbitrary positions: a visibility walk through the stars (see walk_query_launch for the two layouts).
//   reads    head (grid), bstart, sorted, sorted_xy, deg, nbr, far_idx, far_deg, far_off, pool
void query_points(const DlIn &in, const DlWs &ws, hipStream_t s, unsigned far_base, const float *vals, int C, const uint8_t *vmask,
                  const void *query, size_t n, bool sparse, void *out, uint8_t *valid, int valid_rule);
#endif

}  // namespace ofl_dlw
