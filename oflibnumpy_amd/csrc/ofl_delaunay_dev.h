// ofl_delaunay_dev.h -- device helpers that more than one stage file of the K3 exact path (ofl_delaunay*.hip) uses; a helper
// of one stage lives in that stage's file.
#pragma once
#include "ofl_scatter_dev.h"
#include "ofl_delaunay_core.h"
#include "ofl_delaunay_ws.h"

namespace ofl_dlw {

using ofl_sc::D2;
using ofl_sc::point_of;

// ordered keys: doubles as integers that compare the same way (for atomicMin / atomicMax)
__device__ __forceinline__ unsigned long long okey(double d)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double okey_inv(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)b);
}

struct PosFn {
    const float *flow; int sign, W; float inv_w;
    __device__ __forceinline__ PosFn(const float *f, int s, int w) : flow(f), sign(s), W(w), inv_w(1.0f / (float)w) {}
    __device__ __forceinline__ P2 operator()(int i) const
    {
        // row of point i without an integer division: float estimate (i < 2^27, error < 16 rows... corrected exactly)
        int y = (int)((float)i * inv_w);
        int r = i - y * W;
        while (r < 0) { --y; r += W; }
        while (r >= W) { ++y; r -= W; }
        const D2 p = point_of(flow, sign, W, r, y);
        return P2{ p.x, p.y };
    }
};

__device__ __forceinline__ bool kept_pt(const uint8_t *pmask, size_t i) { return !pmask || pmask[i] != 0; }

// what step 1 of the slab mode leaves in the header for step 2 to recognise: the band and the field it ran for (never 0)
__host__ __device__ inline unsigned slab_stamp_of(int H, int W, int row0, int rows)
{
    const unsigned v = ((unsigned)row0 * 65536u + (unsigned)rows) ^ ((unsigned)H * 2654435761u) ^ ((unsigned)W * 40503u);
    return v ? v : 1u;
}

// Is grid site (x, y) CLEAN: do the four cells around it, and the four cells around each of its grid neighbours NW, N, NE and W
// (the only ones with a smaller index), all lie in clean tiles (dl_cell_kernel: every cell of the 32 x 8 tile verified)?  Then
// its star and theirs were written from cell flags (dl_site_cells_kernel; ofl_dl::star_from_cells: E, SE?, S, SW?, W, NW?, N,
// NE?), every triangle it lists is a triangle of a verified cell and is owned by a site whose star lists it: the triangles a
// clean site OWNS are drawn cell by cell (dl_raster_cells_kernel) with the ids the site-wise raster would give them, and that
// raster has nothing to do for a clean site.  The cells in question are [x - 2, x + 1] x [y - 2, y]: at most four tiles.
__device__ __forceinline__ bool site_clean(const unsigned char *__restrict__ tileflag, int x, int y, int W, int H, int tiles_x)
{
    if (x < 2 || y < 2 || x > W - 3 || y > H - 2) return false;
    const int tx0 = (x - 2) >> 5, tx1 = (x + 1) >> 5, ty0 = (y - 2) >> 3, ty1 = y >> 3;
    return tileflag[ty0 * tiles_x + tx0] && tileflag[ty0 * tiles_x + tx1] && tileflag[ty1 * tiles_x + tx0] && tileflag[ty1 * tiles_x + tx1];
}

}  // namespace ofl_dlw
