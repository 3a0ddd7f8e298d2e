// ofl_delaunay_raster.hip -- K3 exact path, from stars to values (the map of the path: ofl_delaunay.hip): the stars'
// triangles are scan-converted into the owner map (cell-wise on clean tiles, site-wise elsewhere, wave-wise for the large
// ones), the owner map is resolved into values and validity, and arbitrary positions walk through the stars.
#include "ofl_delaunay_dev.h"

using namespace ofl;
using namespace ofl_sc;
using namespace ofl_dl;
using namespace ofl_dlw;

namespace {

// ------------------------------------------------------------------------------------------------ raster
struct TriRef { unsigned i0, i1, i2; bool ok; };

__device__ __forceinline__ TriRef dl_decode(unsigned id, unsigned far_base, const DlWs &ws)
{
    TriRef r;
    r.ok = false;
    if (id < far_base) {
        const unsigned p = id / kSlots, k = id % kSlots, d = ws.deg[p];
        if (d > kSlots || k >= d) return r;
        r.i0 = p; r.i1 = ws.nbr[(size_t)p * kSlots + k]; r.i2 = ws.nbr[(size_t)p * kSlots + (k + 1 == d ? 0 : k + 1)];
        r.ok = true;
    } else {
        const unsigned rank = (id - far_base) / kFarK, k = (id - far_base) % kFarK, d = ws.far_deg[rank];
        if (d == kDegLeft || k >= d) return r;
        const unsigned off = ws.far_off[rank];
        const int a = ws.pool[off + k], b = ws.pool[off + (k + 1 == d ? 0 : k + 1)];
        if (a < 0 || b < 0 || a == b) return r;
        r.i0 = ws.far_idx[rank]; r.i1 = (unsigned)a; r.i2 = (unsigned)b;
        r.ok = true;
    }
    canonical3(r.i0, r.i1, r.i2);
    return r;
}

__device__ __forceinline__ TriBox box_rows(const D2 &p0, const D2 &p1, const D2 &p2, int W, int H, const DlWs &ws)
{
    TriBox b = tri_box(p0, p1, p2, W, H);
    b.y0 = max(b.y0, ws.oy0);
    b.y1 = min(b.y1, ws.oy1 - 1);
    return b;
}

__device__ __forceinline__ D2 pt(const PosFn &pos, unsigned i) { const P2 p = pos((int)i); return D2{ p.x, p.y }; }

// does the star of site s list b right after a (cyclically)?  Stars of more than 64 neighbours are not searched.
__device__ __forceinline__ bool star_has(const DlWs &ws, unsigned s, unsigned a, unsigned b)
{
    const unsigned d = ws.deg[s];
    if (d <= kSlots) {
        // the whole row in four 16-byte loads that are in flight together (a loop that stops at the match is a chain of
        // dependent 4-byte loads: this look-up is most of the small-triangle raster's time)
        const uint4 *row = reinterpret_cast<const uint4 *>(ws.nbr + (size_t)s * kSlots);
        const uint4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
        const unsigned v[kSlots] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w };
        bool has = false;
#pragma unroll
        for (int k = 0; k < kSlots; ++k) {
            const unsigned nxt = (unsigned)(k + 1) < d ? v[(k + 1) & (kSlots - 1)] : v[0];      // (k + 1 == d == 16 wraps to v[0] either way)
            has = has || ((unsigned)k < d && v[k] == a && nxt == b);
        }
        return has;
    }
    if (d != kDegFar) return false;
    const unsigned rank = ws.nbr[(size_t)s * kSlots], fd = ws.far_deg[rank];
    if (fd == kDegLeft || fd > 64) return false;
    const int *pl = ws.pool + ws.far_off[rank];
    for (unsigned k = 0; k < fd; ++k)
        if (pl[k] == (int)a) return pl[k + 1 == fd ? 0 : k + 1] == (int)b;
    return false;
}

// scan conversion of ONE triangle by one thread (vertices in canonical rotation: every copy sets up the same edge functions);
// large bounding boxes go to the list swept by whole waves
__device__ __forceinline__ void raster_tri(unsigned id, const D2 &q0, const D2 &q1, const D2 &q2, int H, int W, const DlWs &ws)
{
    const TriBox b = box_rows(q0, q1, q2, W, H, ws);
    if (b.x1 < b.x0 || b.y1 < b.y0) return;
    const long long area = (long long)(b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1);
    if (area > kSmallArea) {
        const unsigned long long slot = atomicAdd(&ws.head->big_n, 1ull);
        if (slot < ws.big_cap) ws.big[slot] = id; else atomicOr(&ws.head->err, 4u);
        return;
    }
    TriEdge te;
    if (!tri_setup(q0, q1, q2, te)) return;
    for (int gy = b.y0; gy <= b.y1; ++gy)
        for (int gx = b.x0; gx <= b.x1; ++gx)
            if (tri_inside(te, (double)gx, (double)gy)) atomicMin(&ws.owner[(size_t)gy * W + gx], id);
    // (per-row intervals as in dl_raster_big_kernel were measured here for the wide boxes of sheared lattices: the extra
    // registers and code slow every field down by 4 - 10 %, config 5 included)
}

// one triangle of a star by one thread.  Every triangle is listed by
// each of its three sites; the copy of the site with the smallest index is the one that is drawn -- unless that
// site's star does not list the triangle (stars that disagree on a co-circular cell), in which case this copy is drawn too.
// `trust`: bit 0 = `self` was settled by the mesh-cell pass (its neighbours are grid neighbours), bits 1 .. 4 = so were its
// grid neighbours NW, N, NE, W -- the only ones with a smaller index.  A star that came from the cell flags lists every
// triangle of its four (verified) cells, so the copy held by such a neighbour IS drawn and this one need not look it up.
__device__ __forceinline__ void thread_raster(unsigned id, unsigned self, const PosFn &pos, int H, int W, const DlWs &ws, unsigned far_base,
                                              unsigned trust = 0)
{
    const TriRef tr = dl_decode(id, far_base, ws);
    if (!tr.ok) return;
    if (tr.i0 != self) {
        bool skip = false;
        if (trust & 1u) {
            const int dv = (int)self - (int)tr.i0;
            skip = (dv == W + 1 && (trust & 2u)) || (dv == W && (trust & 4u)) || (dv == W - 1 && (trust & 8u)) || (dv == 1 && (trust & 16u));
        }
        if (skip || star_has(ws, tr.i0, tr.i1, tr.i2)) return;
    }
    raster_tri(id, pt(pos, tr.i0), pt(pos, tr.i1), pt(pos, tr.i2), H, W, ws);
}

// Cell-centric raster of the intact parts of the mesh: one thread per grid cell of a clean tile draws the cell's two
// triangles -- corner positions from two coalesced rows of the flow, no star to decode, no look-up into another site's star --
// with exactly the ids the site-wise raster gives them: a triangle belongs to its smallest-index vertex s, and when s is a
// clean site (site_clean) its position k in s's star follows from s's own cell flags:
//   diagonal a - c:  (a, b, c) = a's triangle 0 (E, SE),  (a, c, d) = a's triangle 1 (SE, S)
//   diagonal b - d:  (a, b, d) = a's triangle 0 (E, S),   (b, c, d) = b's triangle (S, SW): k = 1 + [b's own cell has diagonal a - c]
// (a = (x, y), b = (x + 1, y), c = (x + 1, y + 1), d = (x, y + 1): a < b < d < c in index order).  Triangles whose owner is
// not clean -- rims of holes and tears, neighbourhoods of dropped points -- stay with the site-wise raster, which in turn
// returns at once for clean sites: whole waves of it, since cleanliness goes by tiles.  An intact mesh with a hole or a
// moving object in it is drawn almost entirely here (4K: 0.49 -> 0.27 ms); on a field that is broken all over (speckled
// point masks, BASELINE config 5) no tile is clean and this kernel ends after one byte per workgroup.
__global__ __launch_bounds__(256)
void dl_raster_cells_kernel(const float *__restrict__ flow, int sign, int H, int W, DlWs ws, unsigned far_base, int tiles_x, int ntiles)
{
    const unsigned per = gridDim.x >> 3;                        // (grid padded to a multiple of 8) one contiguous eighth per XCD
    const int tile = (int)((blockIdx.x & 7u) * per + (blockIdx.x >> 3));
    if (tile >= ntiles || !ws.tileflag[tile]) return;           // (the owner of a triangle is clean only if the cell's own tile is)
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x = tx * 32 + (threadIdx.x & 31), y = ty * 8 + (threadIdx.x >> 5);
    const size_t ia = (size_t)y * W + x;
    const unsigned f = ws.cellflag[ia];                         // (a clean tile lies inside the grid, all flags non-zero)
    const bool sa = site_clean(ws.tileflag, x, y, W, H, tiles_x);
    const bool sb = f == 2 && site_clean(ws.tileflag, x + 1, y, W, H, tiles_x);
    if (!sa && !sb) return;
    const D2 a = point_of(flow, sign, W, x, y), b = point_of(flow, sign, W, x + 1, y);
    const D2 c = point_of(flow, sign, W, x + 1, y + 1), d = point_of(flow, sign, W, x, y + 1);
    if (sa) {
        raster_tri((unsigned)ia * kSlots, a, b, f == 1 ? c : d, H, W, ws);
        if (f == 1) raster_tri((unsigned)ia * kSlots + 1u, a, c, d, H, W, ws);
    }
    if (sb) raster_tri((unsigned)(ia + 1) * kSlots + 1u + (ws.cellflag[ia + 1] == 1 ? 1u : 0u), b, c, d, H, W, ws);
}

__global__ __launch_bounds__(256)
void dl_raster_small_kernel(const float *__restrict__ flow, int sign, int H, int W, DlWs ws, unsigned far_base, const unsigned *__restrict__ list)
{
    // The sites that are not clean, compacted in index order (dl_compact_kernel<4>): on a field with a few tears or holes they
    // are the rims -- one or two sites of 64 -- and a wave that also held the 62 clean ones ran as long as its rim sites took
    // (64-px stripes at 4K: 0.93 ms, every wave crossing a tear).
    // Workgroups go round-robin over the 8 XCDs: give each XCD one contiguous eighth of the list, so that the neighbour
    // rows a point looks up (the stars of the sites above and below it) are in ITS L2
    // (a row band draws from the sites around its rows only -- often one contiguous stretch of indices, which that mapping
    // would hand to a single XCD: 3.1 ms instead of 0.5 for an eighth of config 5 -- so bands keep the round-robin order)
    const unsigned n_list = ws.head->n_raster;
    const unsigned nb = (n_list + 255u) / 256u, per = (nb + 7u) / 8u;
    const PosFn pos(flow, sign, W);
    for (unsigned blk0 = blockIdx.x; blk0 < per * 8u; blk0 += gridDim.x) {
        const unsigned blk = ws.oy1 - ws.oy0 < H ? blk0 : (blk0 & 7u) * per + (blk0 >> 3);
        const unsigned i = blk * 256u + threadIdx.x;
        if (blk >= nb || i >= n_list) continue;
        const size_t p = list[i];
        const unsigned d = ws.deg[p];
        // which of this site and its four smaller-index grid neighbours were settled from the cell flags (three dword loads)
        unsigned trust = 0;
        {
            const int y = (int)(p / (unsigned)W), x = (int)(p - (size_t)y * W);
            if (x >= 2 && y >= 2 && x <= W - 3 && y <= H - 2) {
                const unsigned char *f = ws.cellflag + (size_t)(y - 2) * W + (x - 2);
                struct __attribute__((packed, aligned(1))) U32u { unsigned v; };
                const unsigned r0 = reinterpret_cast<const U32u *>(f)->v, r1 = reinterpret_cast<const U32u *>(f + W)->v,
                               r2 = reinterpret_cast<const U32u *>(f + 2 * (size_t)W)->v;
                auto nz = [](unsigned r, int k) { return ((r >> (8 * k)) & 0xFFu) != 0u; };
                if (nz(r2, 2) && nz(r2, 1) && nz(r1, 1) && nz(r1, 2)) {
                    trust = 1u;
                    if (nz(r1, 1) && nz(r1, 0) && nz(r0, 0) && nz(r0, 1)) trust |= 2u;       // NW
                    if (nz(r1, 2) && nz(r1, 1) && nz(r0, 1) && nz(r0, 2)) trust |= 4u;       // N
                    if (nz(r1, 3) && nz(r1, 2) && nz(r0, 2) && nz(r0, 3)) trust |= 8u;       // NE
                    if (nz(r2, 1) && nz(r2, 0) && nz(r1, 0) && nz(r1, 1)) trust |= 16u;      // W
                }
            }
        }
        for (unsigned k = 0; k < d; ++k) thread_raster((unsigned)p * kSlots + k, (unsigned)p, pos, H, W, ws, far_base, trust);
    }
}

// one WAVE per unfinished point (their stars run to hundreds of triangles: a thread per point would crawl)
__global__ __launch_bounds__(256)
void dl_raster_far_kernel(const float *__restrict__ flow, int sign, int H, int W, DlWs ws, unsigned far_base)
{
    const PosFn pos(flow, sign, W);
    const unsigned n_far = ws.head->n_far;
    for (unsigned rank = blockIdx.x * 4 + (threadIdx.x >> 6); rank < n_far; rank += gridDim.x * 4) {
        const unsigned d = ws.far_deg[rank];
        if (d == kDegLeft) continue;
        const unsigned self = ws.far_idx[rank];
        for (unsigned k = threadIdx.x & 63; k < d; k += 64) thread_raster(far_base + rank * kFarK + k, self, pos, H, W, ws, far_base);
    }
}

// One wave per large triangle, row by row: the three edge functions are linear in x, so each row's covered interval is
// solved for (padded by a node on each side; tri_inside still decides every node) and only that interval is walked.  A
// sliver from a hull point to a far outlier has the whole frame as its bounding box and covers a handful of nodes:
// box-wise it cost 130 000 steps at 4K, row-wise 2 160.
__global__ __launch_bounds__(256)
void dl_raster_big_kernel(const float *__restrict__ flow, int sign, int H, int W, DlWs ws, unsigned far_base)
{
    unsigned long long n = ws.head->big_n;
    if (n > ws.big_cap) n = ws.big_cap;
    const PosFn pos(flow, sign, W);
    const int lane = threadIdx.x & 63;
    for (unsigned long long j = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += (unsigned long long)gridDim.x * 4) {
        const unsigned id = ws.big[j];
        const TriRef tr = dl_decode(id, far_base, ws);
        if (!tr.ok) continue;
        const D2 q0 = pt(pos, tr.i0), q1 = pt(pos, tr.i1), q2 = pt(pos, tr.i2);
        const TriBox b = box_rows(q0, q1, q2, W, H, ws);
        if (b.x1 < b.x0 || b.y1 < b.y0) continue;
        TriEdge te;
        if (!tri_setup(q0, q1, q2, te)) continue;
        // w_k(dx, dy) = A_k dx + B_k(dy) >= -tol with dx = gx - p0.x, the sign of det folded in (tri_inside)
        const double sg = te.det < 0 ? -1.0 : 1.0;
        const double A1 = sg * te.e2y, A2 = -sg * te.e1y, A0 = sg * (te.e1y - te.e2y);
        for (int gy = b.y0; gy <= b.y1; ++gy) {
            const double dy = (double)gy - te.p0.y;
            const double B1 = -sg * te.e2x * dy, B2 = sg * te.e1x * dy, B0 = sg * (te.det + (te.e2x - te.e1x) * dy);
            double lo = -1e300, hi = 1e300;
            const double Ak[3] = { A0, A1, A2 }, Bk[3] = { B0, B1, B2 };
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                // the bound of an almost horizontal edge (tiny A) is ill-conditioned: its slack grows with the rounding of
                // B / A, so that no node tri_inside accepts can fall outside (a wide slack merely restricts nothing)
                const double bnd = (-te.tol - Bk[k]) / Ak[k];
                const double slack = 1.0 + 8e-15 * ((fabs(Bk[k]) + te.tol) / fabs(Ak[k]) + fabs(bnd) + fabs(te.p0.x));
                if (Ak[k] > 0.0) lo = fmax(lo, bnd - slack);
                else if (Ak[k] < 0.0) hi = fmin(hi, bnd + slack);
            }
            // the interval in node coordinates (NaN-safe: an unordered compare keeps the box)
            const double xl = lo + te.p0.x, xh = hi + te.p0.x;
            int xa = b.x0, xb = b.x1;
            if (xl > (double)xa) xa = xl >= (double)xb + 1.0 ? xb + 1 : (int)floor(xl);
            if (xh < (double)xb) xb = xh <= (double)xa - 1.0 ? xa - 1 : (int)ceil(xh);
            for (int gx = xa + lane; gx <= xb; gx += 64)
                if (tri_inside(te, (double)gx, (double)gy)) atomicMin(&ws.owner[(size_t)gy * W + gx], id);
        }
    }
}

// ------------------------------------------------------------------------------------------------ resolve
template <typename VT>
__global__ __launch_bounds__(256)
void dl_resolve_kernel(const float *__restrict__ flow, int sign, const VT *__restrict__ vals, int C,
                       const uint8_t *__restrict__ vmask, int H, int W, int row0, int rows,
                       VT *__restrict__ out, uint8_t *__restrict__ valid, int valid_rule, DlWs ws, unsigned far_base)
{
    const int x = blockIdx.x * 32 + (threadIdx.x & 31);
    const int yl = blockIdx.y * 8 + (threadIdx.x >> 5), y = row0 + yl;
    if (x >= W || yl >= rows) return;
    const size_t o = (size_t)yl * W + x;
    const unsigned id = ws.owner[(size_t)y * W + x];
    TriRef tr;
    tr.ok = false;
    if (id != kNoOwner) tr = dl_decode(id, far_base, ws);
    if (!tr.ok) {
        for (int c = 0; c < C; ++c) out[o * C + c] = (VT)0;                  // outside the convex hull: NaN -> 0, utils.py:254
        if (valid) valid[o] = 0;
        return;
    }
    const PosFn pos(flow, sign, W);
    const size_t vi[3] = { tr.i0, tr.i1, tr.i2 };
    double c0, c1, c2;
    (void)bary(pt(pos, tr.i0), pt(pos, tr.i1), pt(pos, tr.i2), (double)x, (double)y, c0, c1, c2);
    resolve_emit(vals, C, vmask, vi, c0, c1, c2, valid_rule, out, valid, o);
}

// ------------------------------------------------------------------------------------------------ arbitrary positions
// neighbour k of site u (cyclic); -1 = an unbounded gap of the star (or no star)
struct StarRef { const unsigned *small; const int *far; unsigned d; };

__device__ __forceinline__ StarRef star_of(const DlWs &ws, unsigned u)
{
    StarRef r;
    r.small = nullptr; r.far = nullptr; r.d = 0;
    const unsigned d = ws.deg[u];
    if (d >= 1 && d <= kSlots) { r.small = ws.nbr + (size_t)u * kSlots; r.d = d; }
    else if (d == kDegFar) {
        const unsigned rank = ws.nbr[(size_t)u * kSlots], fd = ws.far_deg[rank];
        if (fd != kDegLeft && fd > 0) { r.far = ws.pool + ws.far_off[rank]; r.d = fd; }
    }
    return r;
}

__device__ __forceinline__ int star_at(const StarRef &s, unsigned k) { return s.small ? (int)s.small[k] : s.far[k]; }

// Last resort of dl_locate: the stars of the sites in the bucket rings around the position, triangle by triangle.  The walk
// below needs stars that AGREE along its way (the edge it leaves through must be listed by the star it enters); where four
// sites are co-circular they need not -- on an integer-valued field that is every cell -- and a walk that meets such a pair
// used to give up: 0.17 % of the positions of mode 2 't' on such fields came back "outside" although SciPy finds them inside
// (tools/soak_scatter.py --mode query).  Whatever the stars disagree on, their triangles together cover the hull, and none
// spans an unbounded gap: a position that lies in no triangle of any site within `rings` buckets IS outside (or in a triangle
// larger than that: rims of holes -- the walk finds those, they are not what it stumbles over).
__device__ bool dl_locate_brute(const DlWs &ws, const PosFn &pos, double qx, double qy, int rings, TriRef &tr, double &c0, double &c1, double &c2)
{
    const Grid g = ws.head->grid;
    const int bx = g.bx(qx), by = g.by(qy);
    const D2 q{ qx, qy };
    for (int r = 0; r <= rings; ++r)
        for (int row = by - r; row <= by + r; ++row) {
            if (row < 0 || row >= g.gy) continue;
            const bool full = row == by - r || row == by + r;
            for (int part = 0; part < (full ? 1 : 2); ++part) {
                int x0 = full ? bx - r : (part ? bx + r : bx - r), x1 = full ? bx + r : x0;
                if (!full && (x0 < 0 || x0 >= g.gx)) continue;
                x0 = max(x0, 0); x1 = min(x1, g.gx - 1);
                if (x1 < x0) continue;
                for (unsigned j = ws.bstart[(size_t)row * g.gx + x0]; j < ws.bstart[(size_t)row * g.gx + x1 + 1]; ++j) {
                    const unsigned sidx = ws.sorted[j];
                    if (sidx == 0xFFFFFFFFu) continue;
                    const StarRef ss = star_of(ws, sidx);
                    if (ss.d < 2) continue;
                    const D2 pa = pt(pos, sidx);
                    int n0 = star_at(ss, ss.d - 1);
                    D2 p0 = n0 >= 0 ? pt(pos, (unsigned)n0) : D2{ 0.0, 0.0 };
                    for (unsigned k = 0; k < ss.d; ++k) {
                        const int n1 = star_at(ss, k);
                        const D2 p1 = n1 >= 0 ? pt(pos, (unsigned)n1) : D2{ 0.0, 0.0 };
                        if (n0 >= 0 && n1 >= 0 && n0 != n1) {
                            const double det = cross2(pa, p0, p1);
                            if (det != 0.0) {
                                const double sg = det > 0.0 ? 1.0 : -1.0, tol = kEps * fabs(det);
                                const double wa = sg * cross2(p0, p1, q), wb = sg * cross2(p1, pa, q), wc = sg * cross2(pa, p0, q);
                                if (wa >= -tol && wb >= -tol && wc >= -tol) {
                                    tr.i0 = sidx; tr.i1 = (unsigned)n0; tr.i2 = (unsigned)n1; tr.ok = true;
                                    canonical3(tr.i0, tr.i1, tr.i2);
                                    (void)bary(pt(pos, tr.i0), pt(pos, tr.i1), pt(pos, tr.i2), qx, qy, c0, c1, c2);
                                    return true;
                                }
                            }
                        }
                        n0 = n1; p0 = p1;
                    }
                }
            }
        }
    return false;
}

// The triangle of the triangulation that contains (qx, qy): a visibility walk from the owner triangle of the grid node
// next to the position.  Stepping over the edge u -> v of the counter-clockwise triangle (u, v, w) leads to the triangle
// (u, x, v) with x the neighbour BEFORE v in u's star; a gap there means the position is outside the convex hull.
__device__ bool dl_locate(const DlWs &ws, unsigned far_base, const PosFn &pos, int H, int W, double qx, double qy,
                          TriRef &tr, double &c0, double &c1, double &c2)
{
    if (!(qx == qx && qy == qy)) return false;
    const int nx = (int)fmin(fmax(rint(qx), 0.0), (double)(W - 1)), ny = (int)fmin(fmax(rint(qy), 0.0), (double)(H - 1));
    unsigned id = kNoOwner;
    for (int r = 0; r <= 2 && id == kNoOwner; ++r)
        for (int dy = -r; dy <= r && id == kNoOwner; ++dy)
            for (int dx = -r; dx <= r && id == kNoOwner; ++dx) {
                if (max(abs(dx), abs(dy)) != r) continue;
                const int x = nx + dx, y = ny + dy;
                if (x < 0 || y < 0 || x >= W || y >= H) continue;
                id = ws.owner[(size_t)y * W + x];
            }
    if (id == kNoOwner) {
        // No owned node next to the position (it lies outside the image, or the hull does not cover the image there): seed
        // the walk from the point set instead -- the first site in growing bucket rings around the position that has a star
        // with two consecutive real neighbours.  A position inside the hull is reached from ANY triangle.
        const Grid g = ws.head->grid;
        const int bx = g.bx(qx), by = g.by(qy);
        const int rmax = max(max(bx, g.gx - 1 - bx), max(by, g.gy - 1 - by));
        bool seeded = false;
        for (int r = 0; r <= rmax && r <= 512 && !seeded; ++r)
            for (int row = by - r; row <= by + r && !seeded; ++row) {
                if (row < 0 || row >= g.gy) continue;
                const bool full = row == by - r || row == by + r;
                for (int part = 0; part < (full ? 1 : 2) && !seeded; ++part) {
                    int x0 = full ? bx - r : (part ? bx + r : bx - r), x1 = full ? bx + r : x0;
                    if (!full && (x0 < 0 || x0 >= g.gx)) continue;
                    x0 = max(x0, 0); x1 = min(x1, g.gx - 1);
                    if (x1 < x0) continue;
                    for (unsigned j = ws.bstart[(size_t)row * g.gx + x0]; j < ws.bstart[(size_t)row * g.gx + x1 + 1] && !seeded; ++j) {
                        const unsigned sidx = ws.sorted[j];
                        if (sidx == 0xFFFFFFFFu) continue;
                        const StarRef ss = star_of(ws, sidx);
                        for (unsigned k = 0; k < ss.d && !seeded; ++k) {
                            const int n0 = star_at(ss, k), n1 = star_at(ss, k + 1 == ss.d ? 0 : k + 1);
                            if (n0 < 0 || n1 < 0 || n0 == n1) continue;
                            tr.i0 = sidx; tr.i1 = (unsigned)n0; tr.i2 = (unsigned)n1; tr.ok = true;
                            seeded = true;
                        }
                    }
                }
            }
        if (!seeded) return false;
    } else {
        tr = dl_decode(id, far_base, ws);
        if (!tr.ok) return dl_locate_brute(ws, pos, qx, qy, kLocateRings, tr, c0, c1, c2);
    }
    unsigned a = tr.i0, b = tr.i1, c = tr.i2;
    D2 pa = pt(pos, a), pb = pt(pos, b), pc = pt(pos, c);
    if (cross2(pa, pb, pc) < 0.0) { const unsigned t = b; b = c; c = t; const D2 tp = pb; pb = pc; pc = tp; }     // counter-clockwise
    for (int step = 0; step < 16384; ++step) {
        // edge functions of q (positive inside)
        const double det = cross2(pa, pb, pc);
        if (!(det > 0.0)) return dl_locate_brute(ws, pos, qx, qy, kLocateRings, tr, c0, c1, c2);
        const double wa = cross2(pb, pc, D2{ qx, qy }), wb = cross2(pc, pa, D2{ qx, qy }), wc = cross2(pa, pb, D2{ qx, qy });
        const double tol = kEps * det;
        if (wa >= -tol && wb >= -tol && wc >= -tol) {
            tr.i0 = a; tr.i1 = b; tr.i2 = c;
            canonical3(tr.i0, tr.i1, tr.i2);
            tr.ok = true;
            (void)bary(pt(pos, tr.i0), pt(pos, tr.i1), pt(pos, tr.i2), qx, qy, c0, c1, c2);
            return true;
        }
        // leave through the most violated edge: wa belongs to edge b -> c, wb to c -> a, wc to a -> b
        unsigned u, v;
        D2 pu, pv;
        if (wa <= wb && wa <= wc) { u = b; v = c; pu = pb; pv = pc; }
        else if (wb <= wc)        { u = c; v = a; pu = pc; pv = pa; }
        else                      { u = a; v = b; pu = pa; pv = pb; }
        // the triangle on the other side of u -> v: the neighbour BEFORE v in u's star -- or, where u's star does not list v
        // (stars that disagree on a co-circular cell), the neighbour AFTER u in v's star, which is the same site when both do
        int x = -2;                                         // -2: neither star lists the edge, -1: an unbounded gap
        {
            const StarRef su = star_of(ws, u);
            unsigned k = 0;
            while (k < su.d && star_at(su, k) != (int)v) ++k;
            if (k < su.d) x = star_at(su, k == 0 ? su.d - 1 : k - 1);
        }
        if (x == -2) {
            const StarRef sv = star_of(ws, v);
            unsigned k = 0;
            while (k < sv.d && star_at(sv, k) != (int)u) ++k;
            if (k < sv.d) x = star_at(sv, k + 1 == sv.d ? 0 : k + 1);
        }
        if (x == -1) return false;                                     // an unbounded gap: outside the convex hull
        D2 px = x >= 0 ? pt(pos, (unsigned)x) : D2{ 0.0, 0.0 };
        if (x < 0 || !(cross2(pu, px, pv) > 0.0)) {
            // Neither star lists the edge, or the order of a star is no guide here (hull stars of lattice fields repeat a
            // neighbour around a collinear run: a, b, a): choose the apex GEOMETRICALLY -- among the neighbours of u and of v
            // that lie on the far side of u -> v, the one whose circle through u and v holds none of the others.
            int best = -1;
            D2 pbest{ 0.0, 0.0 };
            for (int side = 0; side < 2; ++side) {
                const StarRef sn = star_of(ws, side ? v : u);
                for (unsigned k = 0; k < sn.d; ++k) {
                    const int n = star_at(sn, k);
                    if (n < 0 || n == (int)u || n == (int)v || n == best) continue;
                    const D2 pn = pt(pos, (unsigned)n);
                    if (!(cross2(pu, pn, pv) > 0.0)) continue;
                    if (best < 0 || incircle(pu, pbest, pv, pn) > 0.0) { best = n; pbest = pn; }
                }
            }
            if (best < 0) return dl_locate_brute(ws, pos, qx, qy, kLocateRings, tr, c0, c1, c2);
            x = best; px = pbest;
        }
        // new triangle (u, x, v), counter-clockwise
        a = u; pa = pu; b = (unsigned)x; pb = px; c = v; pc = pv;
    }
    return dl_locate_brute(ws, pos, qx, qy, kLocateRings, tr, c0, c1, c2);
}

template <bool SPARSE>
__global__ __launch_bounds__(256)
void dl_query_kernel(const float *__restrict__ flow, int sign, const float *__restrict__ vals, int C,
                     const uint8_t *__restrict__ vmask, int H, int W, const void *__restrict__ query, size_t n,
                     void *__restrict__ out, uint8_t *__restrict__ valid, int valid_rule, DlWs ws, unsigned far_base)
{
    const PosFn pos(flow, sign, W);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        double qx, qy;
        if (SPARSE) { qx = ((const double *)query)[2 * i]; qy = ((const double *)query)[2 * i + 1]; }
        else { const float2 q = ((const float2 *)query)[i]; qx = (double)q.x; qy = (double)q.y; }
        TriRef tr;
        double c0 = 0, c1 = 0, c2 = 0;
        const bool found = dl_locate(ws, far_base, pos, H, W, qx, qy, tr, c0, c1, c2);
        if (SPARSE) {
            double *o = (double *)out + i * C;
            for (int c = 0; c < C; ++c)
                o[c] = found ? c0 * (double)vals[(size_t)tr.i0 * C + c] + c1 * (double)vals[(size_t)tr.i1 * C + c] +
                               c2 * (double)vals[(size_t)tr.i2 * C + c] : 0.0;
            valid[i] = found ? 1 : 0;
        } else if (found) {
            const size_t vi[3] = { tr.i0, tr.i1, tr.i2 };
            resolve_emit(vals, C, vmask, vi, c0, c1, c2, valid_rule, (float *)out, valid, i);
        } else {
            for (int c = 0; c < C; ++c) ((float *)out)[i * C + c] = 0.0f;
            if (valid) valid[i] = 0;
        }
    }
}

}  // namespace

// the host side of the stage: what each entry reads, writes and borrows is stated at its declaration (ofl_delaunay_ws.h)
namespace ofl_dlw {

void raster_cells(const DlIn &in, const DlWs &ws, hipStream_t s, unsigned far_base)
{
    const int ctx = (in.W + 31) / 32, cty = (in.H + 7) / 8;
    hipLaunchKernelGGL(dl_raster_cells_kernel, dim3((unsigned)((ctx * cty + 7) / 8 * 8)), dim3(256), 0, s, in.flow, in.sign_pp, in.H, in.W, ws, far_base,
                       ctx, ctx * cty);
}

void raster_sites(const DlIn &in, const DlWs &ws, hipStream_t s, unsigned far_base)
{
    const size_t n = (size_t)in.H * in.W;
    const unsigned nblk = (unsigned)((n + 255) / 256);
    const unsigned *list = ws.todo_idx;                    // BORROWED: the fan pass's list is free again
    hipLaunchKernelGGL(dl_raster_small_kernel, dim3(std::min<unsigned>((nblk + 7) / 8 * 8, 32768u)), dim3(256), 0, s, in.flow, in.sign_pp, in.H, in.W, ws,
                       far_base, list);
    hipLaunchKernelGGL(dl_raster_far_kernel, dim3(std::min<unsigned>(walk_groups(n), 4096u)), dim3(256), 0, s, in.flow, in.sign_pp, in.H, in.W, ws, far_base);
    hipLaunchKernelGGL(dl_raster_big_kernel, dim3((unsigned)rt().n_cu * 4), dim3(256), 0, s, in.flow, in.sign_pp, in.H, in.W, ws, far_base);
}

template <typename VT>
void resolve_rows(const DlIn &in, const DlWs &ws, hipStream_t s, unsigned far_base, const VT *vals, int C, const uint8_t *vmask,
                  int row0, int rows, VT *out, uint8_t *valid, int valid_rule)
{
    const dim3 grid((in.W + 31) / 32, (rows + 7) / 8);
    hipLaunchKernelGGL(dl_resolve_kernel<VT>, grid, dim3(256), 0, s, in.flow, in.sign_pp, vals, C, vmask, in.H, in.W, row0, rows,
                       out, valid, valid_rule, ws, far_base);
}

template void resolve_rows<float>(const DlIn &, const DlWs &, hipStream_t, unsigned, const float *, int, const uint8_t *, int, int, float *, uint8_t *, int);
template void resolve_rows<double>(const DlIn &, const DlWs &, hipStream_t, unsigned, const double *, int, const uint8_t *, int, int, double *, uint8_t *, int);

void query_points(const DlIn &in, const DlWs &ws, hipStream_t s, unsigned far_base, const float *vals, int C, const uint8_t *vmask,
                  const void *query, size_t n, bool sparse, void *out, uint8_t *valid, int valid_rule)
{
    const size_t nb = (n + 255) / 256;
    const dim3 grid((unsigned)(nb < (1u << 20) ? nb : (1u << 20)));
    if (sparse)
        hipLaunchKernelGGL(dl_query_kernel<true>, grid, dim3(256), 0, s, in.flow, in.sign_pp, vals, C, vmask, in.H, in.W, query, n, out, valid, valid_rule, ws, far_base);
    else
        hipLaunchKernelGGL(dl_query_kernel<false>, grid, dim3(256), 0, s, in.flow, in.sign_pp, vals, C, vmask, in.H, in.W, query, n, out, valid, valid_rule, ws, far_base);
}

}  // namespace ofl_dlw
