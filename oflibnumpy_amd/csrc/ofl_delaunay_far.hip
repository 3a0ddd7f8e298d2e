// ofl_delaunay_far.hip -- K3 exact path, the cooperative star passes (the map of the path: ofl_delaunay.hip): one wave or one
// workgroup per unfinished point, its cell in LDS -- the wave pass against the coarse grid of unfinished points, then the
// left-over passes against all other left-over points.
#include "ofl_delaunay_dev.h"

using namespace ofl;
using namespace ofl_sc;
using namespace ofl_dl;
using namespace ofl_dlw;

namespace {

// Bounds of every 256 consecutive left-over points (one workgroup each): the sweeps of the workgroup pass skip the chunks
// that cannot hold a cutting site.  Left-over points are mostly image-border points in index order -- the top row, then the
// left and right columns in turns, then the bottom row -- so a chunk is split by image half (x < W / 2 or not) and each
// half gets an ORIENTED box along the line from its first to its last point: a piece of one border side is a thin sliver
// whatever the rotation of the field (an axis-aligned box of a slanted side holds the whole hull).
// box[chunk][half] = { ox, oy, ax, ay, t0, t1, s0, s1 }: origin, unit axis, ranges along the axis and along (-ay, ax);
// t0 > t1: the half is empty.
__global__ __launch_bounds__(256)
void dl_left_box_kernel(const DlHead *__restrict__ head, int W, const unsigned *__restrict__ left_pt,
                        const P2 *__restrict__ left_xy, double *__restrict__ box)
{
    __shared__ unsigned s_first[2], s_last[2];
    __shared__ unsigned long long s_k[2][4];               // ordered keys of t0 (min), t1 (max), s0 (min), s1 (max)
    const unsigned n = head->n_left;
    const int t = threadIdx.x;
    for (unsigned chunk = blockIdx.x; chunk * 256u < n; chunk += gridDim.x) {
        __syncthreads();
        if (t < 2) { s_first[t] = 0xFFFFFFFFu; s_last[t] = 0u; s_k[t][0] = ~0ull; s_k[t][1] = 0ull; s_k[t][2] = ~0ull; s_k[t][3] = 0ull; }
        __syncthreads();
        const unsigned j = chunk * 256 + t;
        const bool in = j < n;
        P2 q{ 0.0, 0.0 };
        int half = 0;
        if (in) {
            q = left_xy[j];
            half = (int)(left_pt[j] % (unsigned)W) * 2 >= W ? 1 : 0;
            atomicMin(&s_first[half], j);
            atomicMax(&s_last[half], j);
        }
        __syncthreads();
        double ax = 1.0, ay = 0.0, ox = 0.0, oy = 0.0;
        if (in) {
            const P2 o = left_xy[s_first[half]], e = left_xy[s_last[half]];
            const double dx = e.x - o.x, dy = e.y - o.y, len = sqrt(dx * dx + dy * dy);
            ox = o.x; oy = o.y;
            if (len > 0.0 && isfinite(len)) { ax = dx / len; ay = dy / len; }
            const double rx = q.x - ox, ry = q.y - oy, tt = rx * ax + ry * ay, ss = ry * ax - rx * ay;
            atomicMin(&s_k[half][0], okey(tt)); atomicMax(&s_k[half][1], okey(tt));
            atomicMin(&s_k[half][2], okey(ss)); atomicMax(&s_k[half][3], okey(ss));
        }
        __syncthreads();
        if (t < 2) {
            double *b = box + ((size_t)chunk * 2 + t) * 8;
            if (s_first[t] == 0xFFFFFFFFu) { b[4] = 1.0; b[5] = 0.0; }          // empty half
            else {
                const P2 o = left_xy[s_first[t]], e = left_xy[s_last[t]];
                const double dx = e.x - o.x, dy = e.y - o.y, len = sqrt(dx * dx + dy * dy);
                double axx = 1.0, ayy = 0.0;
                if (len > 0.0 && isfinite(len)) { axx = dx / len; ayy = dy / len; }       // (the same expressions as above: the same axis)
                b[0] = o.x; b[1] = o.y; b[2] = axx; b[3] = ayy;
                b[4] = okey_inv(s_k[t][0]); b[5] = okey_inv(s_k[t][1]); b[6] = okey_inv(s_k[t][2]); b[7] = okey_inv(s_k[t][3]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ stars, cooperative passes
// One workgroup of NT threads per unfinished point.  The cell lives in LDS; candidates are tested NT at a time against
// the current cell (one candidate per thread), and the few that cut it are applied one after the other, nearest first,
// by the whole workgroup (vertex flags and the shift of the surviving vertices in parallel).
//   wave pass (CAP 256, NT 64): fine buckets around the point, then rings of the COARSE grid of unfinished points with
//     the security-radius test -- rims of holes, motion boundaries, anything whose cell spans tens of pixels;
//   left-over pass (CAP 384, NT 64; then CAP 2560, NT 256 for the few cells that overflow): what is left -- hull points
//     (unbounded cells: the points of the image border come here directly), rims of very large holes, fan apexes of
//     border pockets -- against the same candidates plus ALL other points left (a Delaunay neighbour of a left-over point
//     beyond the coarse rings is itself left over).  A hull cell has half a dozen edges and most chunks of the sweep cut
//     nothing: the pass waits -- on the chain of loads that finds the point and its seeds, on votes -- far more than it
//     computes, so it runs as single waves, which puts four times as many points in flight per CU as workgroups of 256
//     did (121 VGPRs, 9.4 KB of LDS: 16 per CU), and since a vote within one wave costs next to nothing, every step of 64
//     candidates is tested against the cell as it stands (4K, axis-parallel border: 0.77 -> 0.38 ms; a rotated border:
//     1.25 -> 1.17 ms).
template <int CAP, int NT>
struct FarLds {
    double vx[CAP], vy[CAP];
    int    tag[CAP];
    unsigned char cut[CAP];
    int    cidx[1];            // the candidate being applied (far_chunks)
    unsigned clist[NT];        // chunk numbers the sweep of the workgroup pass keeps (of a group of NT chunks)
    double ccx[1], ccy[1];
    unsigned long long hit[NT / 64];
    double wmax[NT / 64], wfar[NT / 64];
    unsigned run_lo[64];       // candidate runs of the current step (ranges of a sorted list) ...
    int    run_pre[65];        // ... and the exclusive prefix of their lengths
    int    n, a, ncut, nstart, status;
    // Candidate rejection: a site can only cut a vertex v if it is closer than 2 |v| to the cell's site.  Vertices well
    // outside the data (|v|^2 > t2: the box vertices of an unbounded cell, the circumcentres of sliver triangles along a
    // straight border) would make that radius useless, so they are listed and tested one by one; reach2 covers the rest.
    double reach2;             // (2 * farthest NEAR vertex)^2; 1e300 when the far list overflowed (every vertex is tested)
    double t2;
    int    nfar;
    int    farlist[kFarList];
    // The far vertices of a convex cell are ONE run of the polygon, seen from the site inside a cone of directions (the
    // outward normal cone of a hull point).  When the run [f0, f1] spans less than a half turn, v . c over the run is
    // bounded by its two ends, and a site whose direction lies outside the cone with
    // max(v0 . c / |v0|, v1 . c / |v1|) * vmax < |c|^2 / 2 (minus the margin of vertex_cut) cuts none of them: two dot
    // products instead of the list.  cone = 0 when the run is not unique or too wide.
    int    cone, nrun, f0, f1;
    double c0x, c0y, c1x, c1y, kcone;    // unit directions of the run's ends, 0.999 / (2 * largest |v| in it)
};

template <int CAP, int NT>
__device__ void far_shift(FarLds<CAP, NT> &L, int s0, int s1, int d0)
{
    // moves vertices [s0, s1) to [d0, d0 + s1 - s0); ranges may overlap; all threads of the workgroup take part
    if (d0 == s0 || s1 <= s0) return;
    const int t = threadIdx.x;
    if (d0 < s0) {
        for (int base = s0; base < s1; base += NT) {
            const int k = base + t;
            double x = 0, y = 0; int g = 0;
            if (k < s1) { x = L.vx[k]; y = L.vy[k]; g = L.tag[k]; }
            __syncthreads();
            if (k < s1) { L.vx[k - s0 + d0] = x; L.vy[k - s0 + d0] = y; L.tag[k - s0 + d0] = g; }
            __syncthreads();
        }
    } else {
        for (int end = s1; end > s0; end -= NT) {
            const int k = end - 1 - t;
            double x = 0, y = 0; int g = 0;
            if (k >= s0) { x = L.vx[k]; y = L.vy[k]; g = L.tag[k]; }
            __syncthreads();
            if (k >= s0) { L.vx[k - s0 + d0] = x; L.vy[k - s0 + d0] = y; L.tag[k - s0 + d0] = g; }
            __syncthreads();
        }
    }
}

// reach, far list and far cone of the current cell; all threads, ends with a barrier
template <int CAP, int NT>
__device__ __noinline__ void far_refresh(FarLds<CAP, NT> &L)
{
    const int t = threadIdx.x, n = L.n;
    const double t2 = L.t2;
    if (t == 0) { L.nfar = 0; L.nrun = 0; L.f0 = 0; L.f1 = 0; }
    __syncthreads();
    double r2 = 0.0, f2 = 0.0;
    for (int k = t; k < n; k += NT) {
        const double v2 = L.vx[k] * L.vx[k] + L.vy[k] * L.vy[k];
        const bool far = v2 > t2;
        L.cut[k] = far ? 1 : 0;                           // (far_apply rewrites the flags before it reads them)
        if (far) { const int slot = atomicAdd(&L.nfar, 1); if (slot < kFarList) L.farlist[slot] = k; f2 = fmax(f2, v2); }
        else r2 = fmax(r2, v2);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        r2 = fmax(r2, __hiloint2double(__shfl_xor(__double2hiint(r2), off), __shfl_xor(__double2loint(r2), off)));
        f2 = fmax(f2, __hiloint2double(__shfl_xor(__double2hiint(f2), off), __shfl_xor(__double2loint(f2), off)));
    }
    if (NT > 64) { if ((t & 63) == 0) { L.wmax[t >> 6] = r2; L.wfar[t >> 6] = f2; } }
    __syncthreads();
    for (int k = t; k < n; k += NT)
        if (L.cut[k]) {
            if (!L.cut[k == 0 ? n - 1 : k - 1]) { atomicAdd(&L.nrun, 1); L.f0 = k; }
            if (!L.cut[k + 1 == n ? 0 : k + 1]) L.f1 = k;
        }
    __syncthreads();
    if (t == 0) {
        double m = r2, fm = f2;
        if (NT > 64) { m = 0.0; fm = 0.0; for (int w = 0; w < NT / 64; ++w) { m = fmax(m, L.wmax[w]); fm = fmax(fm, L.wfar[w]); } }
        const bool listed = L.nfar <= kFarList;
        L.reach2 = 4.0 * m;
        L.cone = 0;
        if (L.nfar > 0 && L.nrun == 1) {
            const double ax = L.vx[L.f0], ay = L.vy[L.f0], bx = L.vx[L.f1], by = L.vy[L.f1];
            const double na = sqrt(ax * ax + ay * ay), nb = sqrt(bx * bx + by * by);
            const double c0x = ax / na, c0y = ay / na, c1x = bx / nb, c1y = by / nb;
            // counter-clockwise from f0 to f1 by less than a half turn, with room to spare (or a single far vertex)
            if (L.f0 == L.f1 || (c0x * c1y - c0y * c1x > 1e-6 || (c0x * c1x + c0y * c1y > 0.5 && c0x * c1y - c0y * c1x >= 0.0))) {
                const double vmax = sqrt(fm);
                L.c0x = c0x; L.c0y = c0y; L.c1x = c1x; L.c1y = c1y; L.kcone = 0.999 / (2.0 * vmax);
                L.cone = isfinite(vmax) && isfinite(c0x + c0y + c1x + c1y) ? 1 : 0;
            }
        }
        if (!listed && !L.cone) L.reach2 = 1e300;         // neither a list nor a cone: every vertex is tested
        else if (!listed) L.nfar = -L.nfar;              // a cone without a list: sites the cone cannot reject test every vertex
    }
    __syncthreads();
}

// Ties on coincident vertices can leave more than one run of cut vertices (ofl_dl::poly_cutmask): the first run that holds a
// vertex cut beyond the margin is the one that goes -- the first run if none does.  L.cut holds vertex_cut_ex's 0 / 1 / 2,
// L.a receives the start of the run; all threads, ends with a barrier.  (Not inlined: the workgroup pass sits at 121 VGPRs --
// four waves per SIMD -- and this rare step must not take a register from its sweeps.)
template <int CAP, int NT>
__device__ __noinline__ void far_pick_run(FarLds<CAP, NT> &L)
{
    const int t = threadIdx.x, n = L.n;
    __syncthreads();
    if (t == 0) L.a = 0x7fffffff;
    __syncthreads();
    for (int k = t; k < n; k += NT)
        if (L.cut[k] && !L.cut[k == 0 ? n - 1 : k - 1]) {
            bool sure = false;
            for (int m = k, c = 0; c < n && L.cut[m]; m = m + 1 == n ? 0 : m + 1, ++c) sure = sure || L.cut[m] == 2;
            atomicMin(&L.a, (sure ? 0 : 1 << 24) | k);
        }
    __syncthreads();
    if (t == 0) L.a &= 0xFFFFFF;
    __syncthreads();
}

template <int CAP, int NT, class RelFn>
__device__ void far_apply(FarLds<CAP, NT> &L, const P2 &C, int ctag, int ptag, RelFn rel)
{
    // cooperative version of ofl_dl::poly_clip
    __syncthreads();                                   // the previous application has been read by every thread
    const int t = threadIdx.x, n = L.n;
    const double h = 0.5 * (C.x * C.x + C.y * C.y);
    Poly P{ L.vx, L.vy, L.tag, 1, CAP, n };
    if (t == 0) { L.a = 0x7fffffff; L.ncut = 0; L.nstart = 0; }
    __syncthreads();
    int mine = 0;
    bool weak = false;
    for (int k = t; k < n; k += NT) {
        const int c = vertex_cut_ex(P, k, n, C, ctag, ptag, h, rel);
        L.cut[k] = (unsigned char)c; mine += c != 0; weak = weak || c == 1;
    }
    if (mine) atomicAdd(&L.ncut, mine);
    if (weak) L.nstart = 1;                            // (any vertex decided by the predicate or a tie rule: look at the runs below)
    __syncthreads();
    const int ncut = L.ncut;
    if (ncut == 0 || ncut == n) return;
    for (int k = t; k < n; k += NT)
        if (L.cut[k] && !L.cut[k == 0 ? n - 1 : k - 1]) atomicMin(&L.a, k);
    __syncthreads();
    if (L.nstart) far_pick_run(L);                    // (rare: a vertex decided by the predicate or a tie rule)
    const int a = L.a;
    int len = 0;
    while (L.cut[(a + len) % n]) ++len;               // every thread walks the (short) run: uniform result
    const int b = (a + len - 1) % n, ia = a == 0 ? n - 1 : a - 1, ib = (b + 1) % n;
    const int n2 = n - len + 2;
    if (n2 > CAP) { if (t == 0) L.status |= 1; return; }
    const int tb = L.tag[b];
    const P2 v1 = cut_point(L.tag[ia], C, h, rel, L.vx[ia], L.vy[ia], L.vx[a], L.vy[a]);
    const P2 v2 = cut_point(tb, C, h, rel, L.vx[b], L.vy[b], L.vx[ib], L.vy[ib]);
    __syncthreads();
    if (a <= b) {
        far_shift(L, b + 1, n, a + 2);
        if (t == 0) {
            L.vx[a] = v1.x; L.vy[a] = v1.y; L.tag[a] = ctag;
            L.vx[a + 1] = v2.x; L.vy[a + 1] = v2.y; L.tag[a + 1] = tb;
        }
    } else {
        const int m = a - (b + 1);
        far_shift(L, b + 1, a, 0);
        if (t == 0) {
            L.vx[m] = v1.x; L.vy[m] = v1.y; L.tag[m] = ctag;
            L.vx[m + 1] = v2.x; L.vy[m + 1] = v2.y; L.tag[m + 1] = tb;
        }
    }
    if (t == 0) L.n = n2;
    __syncthreads();
    far_refresh(L);
}

// does candidate `cand` at q cut the cell as it stands?  (per thread; C receives its relative position)
template <int CAP, int NT, class RelFn>
__device__ __forceinline__ bool far_test(const FarLds<CAP, NT> &L, int p, const P2 &pp, int cand, const P2 &q, RelFn rel, P2 &C)
{
    bool hit = false;
    C = P2{ 0.0, 0.0 };
    if (cand >= 0 && cand != p) {
        C.x = q.x - pp.x; C.y = q.y - pp.y;
        const double d2 = C.x * C.x + C.y * C.y;
        if (d2 != 0.0) {
            const int n = L.n;
            const double h = 0.5 * d2;
            Poly P{ const_cast<double *>(L.vx), const_cast<double *>(L.vy), const_cast<int *>(L.tag), 1, CAP, n };
            bool all = d2 < L.reach2, some = !all && L.nfar != 0;
            if (some && L.cone) {
                // vmax max(d0 . c, d1 . c, 0) - |c|^2 / 2 < -(margin of vertex_cut) = -1e-9 (|vx cx| + |vy cy| + |c|^2 / 2)
                const double m0 = L.c0x * C.x + L.c0y * C.y, m1 = L.c1x * C.x + L.c1y * C.y;
                const bool inside = L.c0x * C.y - L.c0y * C.x >= 0.0 && C.x * L.c1y - C.y * L.c1x >= 0.0;
                if (!inside && fmax(fmax(m0, m1), 0.0) + 1e-9 * (fabs(C.x) + fabs(C.y)) < d2 * L.kcone) some = false;
            }
            if (some && L.nfar < 0) { all = true; some = false; }
            // Every vertex, or the far list: four at a time.  The first look of vertex_cut -- is v . c - h beyond the margin,
            // either way? -- needs a vertex and the two tags beside it; a loop that asks vertex_cut one vertex after the other
            // (and stops at the first cut) is a chain of dependent LDS reads, 100+ cycles each, which is what the sweeps of
            // these passes spent their time on.  Here the reads of four vertices are in flight together, the look is taken on
            // all four, and only a vertex inside the margin goes through vertex_cut itself (same decision: its own first look).
            const int cnt = all ? n : (some ? L.nfar : 0);
            for (int i0 = 0; i0 < cnt && !hit; i0 += 4) {
                int kk[4], ta[4], tb[4];
                double x[4], y[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) kk[j] = i0 + j < cnt ? (all ? i0 + j : L.farlist[i0 + j]) : -1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = kk[j] < 0 ? 0 : kk[j];
                    ta[j] = L.tag[k == 0 ? n - 1 : k - 1]; tb[j] = L.tag[k]; x[j] = L.vx[k]; y[j] = L.vy[k];
                }
                unsigned unsure = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (kk[j] < 0 || cand == ta[j] || cand == tb[j]) continue;      // (the candidate already carries an edge at this vertex)
                    const double tx = x[j] * C.x, ty = y[j] * C.y, d = tx + ty - h, m = kDecide * (fabs(tx) + fabs(ty) + h);
                    if (d > m) hit = true;
                    else if (!(d < -m)) unsure |= 1u << j;
                }
                if (!hit && unsure) {
#pragma unroll 1
                    for (int j = 0; j < 4 && !hit; ++j)
                        if ((unsure >> j) & 1u) hit = vertex_cut(P, kk[j], n, C, cand, p, h, rel);
                }
            }
        }
    }
    return hit;
}

// K steps of up to NT candidates each (thread t holds candidates cand[0 .. K), or -1) under ONE vote per round.  Most steps
// cut nothing: they cost one barrier (the vote); the cell is only touched -- and the workgroup only synchronises further --
// when some candidate cuts it.  The candidates that do are applied NEAREST FIRST: they arrive in bucket or index order,
// and applied in that order a row of sites that approaches the cell's site clips it once per site (stripes, folds, a wavy
// image border: a step of 64 sites meant up to 64 cooperative clips of which the last few survive), whereas after the
// nearest ones most of the others no longer cut anything, which far_apply finds out with one cooperative pass over the
// vertices (a lane per vertex) and no clip.  A candidate that does not cut the cell now cannot cut the smaller cell
// later, so the flags taken before the first vote stay valid.
template <int K, int CAP, int NT, class RelFn>
__device__ void far_chunks(FarLds<CAP, NT> &L, int p, const P2 &pp, const int (&cand)[K], const P2 (&q)[K], RelFn rel)
{
    const int t = threadIdx.x;
    unsigned pend = 0;                                     // bit k: candidate k of this lane cuts the cell as it stands now
    double d2[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { P2 C; if (far_test(L, p, pp, cand[k], q[k], rel, C)) pend |= 1u << k; d2[k] = C.x * C.x + C.y * C.y; }
    for (;;) {
        double best = 1e300;
        int bestk = -1;
#pragma unroll
        for (int k = 0; k < K; ++k) if (((pend >> k) & 1u) && d2[k] < best) { best = d2[k]; bestk = k; }
        // (every application below ends with a barrier: the cell is stable here.  A single wave votes with a ballot:
        // __syncthreads_or is a workgroup reduction through LDS, a hundred instructions for every step of every sweep)
        if (NT == 64 ? (__ballot(bestk >= 0) == 0ull) : !__syncthreads_or(bestk >= 0)) return;
        // the nearest cutting candidate of the workgroup: lowest lane of the wave minimum, lowest wave of equal minima
        double wmin = best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            wmin = fmin(wmin, __hiloint2double(__shfl_xor(__double2hiint(wmin), off), __shfl_xor(__double2loint(wmin), off)));
        const unsigned long long eq = __ballot(bestk >= 0 && best == wmin);
        const int lead = (t & ~63) + (eq ? __ffsll((long long)eq) - 1 : 0);
        bool mine = t == lead && eq != 0;
        if (NT > 64) {
            if (mine) L.wmax[t >> 6] = wmin;
            if ((t & 63) == 0 && eq == 0) L.wmax[t >> 6] = 1e300;
            __syncthreads();
            int wbest = 0;
            for (int w = 1; w < NT / 64; ++w) if (L.wmax[w] < L.wmax[wbest]) wbest = w;
            mine = mine && (t >> 6) == wbest;
        }
        if (mine) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (k == bestk) { L.cidx[0] = cand[k]; L.ccx[0] = q[k].x - pp.x; L.ccy[0] = q[k].y - pp.y; }
            pend &= ~(1u << bestk);
        }
        __syncthreads();
        far_apply(L, P2{ L.ccx[0], L.ccy[0] }, L.cidx[0], p, rel);
    }
}

template <int CAP, int NT, class RelFn>
__device__ void far_chunk(FarLds<CAP, NT> &L, int p, const P2 &pp, int cand, const P2 &q, RelFn rel)
{
    const int c1[1] = { cand };
    const P2  q1[1] = { q };
    far_chunks<1>(L, p, pp, c1, q1, rel);
}

// The runs in L.run_lo / L.run_pre (lengths, turned into a prefix here) are walked as ONE dense list, NT candidates per
// step; `map` turns an entry of the sorted list into a point index.
template <int CAP, int NT, class RelFn>
__device__ void far_dense(FarLds<CAP, NT> &L, int p, const P2 &pp, int nruns, RelFn rel,
                          const unsigned *__restrict__ list_pt, const P2 *__restrict__ list_xy)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int r = 0; r < nruns; ++r) { const int c = L.run_pre[r]; L.run_pre[r] = acc; acc += c; }
        L.run_pre[nruns] = acc;
    }
    __syncthreads();
    const int total = L.run_pre[nruns];
    for (int base = 0; base < total; base += NT) {
        const int gidx = base + (int)threadIdx.x;
        int cand = -1;
        P2 q{ 0.0, 0.0 };
        if (gidx < total) {
            int r = 0;
            while (L.run_pre[r + 1] <= gidx) ++r;
            const unsigned j = L.run_lo[r] + (unsigned)(gidx - L.run_pre[r]);
            cand = (int)list_pt[j];
            q = list_xy[j];
        }
        far_chunk(L, p, pp, cand, q, rel);
    }
}

// one run = the buckets [x0, x1] of row `row` of grid g (empty when outside)
template <int CAP, int NT>
__device__ __forceinline__ void far_set_run(FarLds<CAP, NT> &L, int slot, const Grid &g, const unsigned *__restrict__ bstart,
                                            int row, int x0, int x1)
{
    unsigned lo = 0, cnt = 0;
    x0 = max(x0, 0); x1 = min(x1, g.gx - 1);
    if (row >= 0 && row < g.gy && x1 >= x0) {
        lo = bstart[(size_t)row * g.gx + x0];
        cnt = bstart[(size_t)row * g.gx + x1 + 1] - lo;
    }
    L.run_lo[slot] = lo; L.run_pre[slot] = (int)cnt;
}

// candidates of the fine buckets within kRings of the point's bucket
template <int CAP, int NT, class RelFn>
__device__ void far_near_rows(FarLds<CAP, NT> &L, int p, const P2 &pp, const Grid &g, const unsigned *__restrict__ bstart,
                              const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy, RelFn rel)
{
    const int t = threadIdx.x, bx = g.bx(pp.x), by = g.by(pp.y);
    __syncthreads();
    if (t <= 2 * kRings) far_set_run(L, t, g, bstart, (t & 1) ? by - ((t + 1) >> 1) : by + (t >> 1), bx - kRings, bx + kRings);      // (rows from the point's own outwards)
    far_dense(L, p, pp, 2 * kRings + 1, rel, sorted, sorted_xy);
}

// The unfinished points in the coarse cells at Chebyshev distance (ra, rb] from the point's cell (ra = -1: the whole square
// of radius rb): full rows above and below, the two side stretches of the rows in between; runs go through the run list
// 64 at a time.
template <int CAP, int NT, class RelFn>
__device__ void far_coarse_annulus(FarLds<CAP, NT> &L, int p, const P2 &pp, int ra, int rb, const Grid &g1,
                                   const unsigned *__restrict__ b1start, const unsigned *__restrict__ sorted1_pt,
                                   const P2 *__restrict__ sorted1_xy, RelFn rel)
{
    const int t = threadIdx.x, bx = g1.bx(pp.x), by = g1.by(pp.y);
    const int nt = rb - ra, nm = ra >= 0 ? 2 * ra + 1 : 0, total = 2 * nt + 2 * nm;
    for (int b0 = 0; b0 < total; b0 += 64) {
        const int cnt = min(64, total - b0);
        __syncthreads();
        if (t < cnt) {
            const int i = b0 + t;
            if (ra < 0) {
                // the whole square: rows from the point's own outwards, nearest first (from the top row down, the sites of a
                // stretch of border arrive APPROACHING the nearest one, and each of them clips the cell)
                const int k = i >> 1;
                far_set_run(L, t, g1, b1start, (i & 1) ? by - k : by + k, bx - rb, bx + rb);
            }
            else if (i < nt) far_set_run(L, t, g1, b1start, by - rb + i, bx - rb, bx + rb);
            else if (i < 2 * nt) far_set_run(L, t, g1, b1start, by + ra + 1 + (i - nt), bx - rb, bx + rb);
            else {
                const int m = i - 2 * nt, row = by - ra + (m >> 1);
                if (m & 1) far_set_run(L, t, g1, b1start, row, bx + ra + 1, bx + rb);
                else       far_set_run(L, t, g1, b1start, row, bx - rb, bx - ra - 1);
            }
        }
        far_dense(L, p, pp, cnt, rel, sorted1_pt, sorted1_xy);
    }
}

// The cell the per-thread pass left in the point's neighbour slots (the sites of its edges in cyclic order, box sides
// included): rebuilt in one step -- vertex k is where the lines of edges k - 1 and k meet, one lane each -- instead of one
// cooperative clip per site (eight clips of a dozen barriers each were a third of the workgroup pass).  Should a vertex
// not come out finite, the sites are applied as candidates the old way.
template <int CAP, int NT, class RelFn>
__device__ void far_seeds(FarLds<CAP, NT> &L, int p, const P2 &pp, const unsigned *__restrict__ nbr, const PosFn &pos, RelFn rel)
{
    const unsigned *sd = nbr + (size_t)p * kSlots;
    const int ns = min((int)sd[1], kSlots - 4), t = threadIdx.x;
    bool bad = ns < 3;
    double vx = 0.0, vy = 0.0;
    int tag = 0;
    if (t < ns && !bad) {
        double ax, ay, ah, bx, by, bh;
        tag = (int)sd[2 + t];
        edge_line((int)sd[2 + (t == 0 ? ns - 1 : t - 1)], rel, ax, ay, ah);
        edge_line(tag, rel, bx, by, bh);
        const double det = ax * by - bx * ay;
        vx = (ah * by - bh * ay) / det; vy = (ax * bh - bx * ah) / det;
        bad = det == 0.0 || !(isfinite(vx) && isfinite(vy)) || fabs(vx) > 4.0 * kBox || fabs(vy) > 4.0 * kBox;
    }
    if (NT == 64 ? (__ballot(bad) == 0ull) : !__syncthreads_or(bad)) {
        if (t < ns) { L.vx[t] = vx; L.vy[t] = vy; L.tag[t] = tag; }
        if (t == 0) L.n = ns;
        __syncthreads();
        far_refresh(L);
        return;
    }
    const int cand = t < ns ? (int)sd[2 + t] : -1;
    far_chunk(L, p, pp, cand, cand >= 0 ? pos(cand) : pp, rel);
}

template <int CAP, int NT>
__device__ void far_store(FarLds<CAP, NT> &L, unsigned rank, DlHead *head, unsigned *__restrict__ far_deg,
                          unsigned *__restrict__ far_off, int *__restrict__ pool, unsigned long long pool_cap, unsigned *s_off)
{
    const int t = threadIdx.x, n = L.n;
    if (t == 0) {
        *s_off = atomicAdd(&head->pool_used, (unsigned)n);
        if (L.status) atomicOr(&head->err, 1u);
    }
    __syncthreads();
    const unsigned off = *s_off;
    if ((unsigned long long)off + n > pool_cap) {
        if (t == 0) { atomicOr(&head->err, 2u); far_deg[rank] = 0; far_off[rank] = 0; }
        return;
    }
    for (int k = t; k < n; k += NT) pool[off + k] = L.tag[k];
    if (t == 0) { far_deg[rank] = (unsigned)n; far_off[rank] = off; }
}

__device__ void mid_point(FarLds<kMidCap, 64> &L, unsigned &s_off, unsigned rank,
                          const float *__restrict__ flow, int sign, int H, int W, DlHead *head,
                        const unsigned *__restrict__ bstart, const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy,
                        const unsigned *__restrict__ b1start, const unsigned *__restrict__ sorted1_pt, const P2 *__restrict__ sorted1_xy,
                        const unsigned *__restrict__ far_idx, const unsigned char *__restrict__ deg, const unsigned *__restrict__ nbr,
                        unsigned *__restrict__ far_deg, unsigned *__restrict__ far_off, int *__restrict__ pool, unsigned long long pool_cap,
                        unsigned char *__restrict__ far_wide)
{
    const int t = threadIdx.x;
    const int p = (int)far_idx[rank];
    if (deg[p] != kDegFar) return;                         // finished by the second per-thread pass
    // Points of the image border are hull points more often than not: their cells never close, whatever this pass applies
    // (it used to give them kMidRings rings, which the next pass then applied again).  They go straight to the left-over list.
    const int py = (int)((unsigned)p / (unsigned)W), px = p - py * W;
    if (px == 0 || py == 0 || px == W - 1 || py == H - 1) {
        if (t == 0) { far_deg[rank] = kDegLeft; far_wide[rank] = 0; }
        return;
    }
    const Grid g = head->grid, g1 = head->grid1;
    const PosFn pos(flow, sign, W);
    const P2 pp = pos(p);
    auto rel = [&](int q) { const P2 v = pos(q); return P2{ v.x - pp.x, v.y - pp.y }; };
    if (t == 0) {
        Poly P{ L.vx, L.vy, L.tag, 1, kMidCap, 0 };
        poly_init(P);
        L.n = P.n; L.status = 0; L.t2 = head->far_t2;
    }
    __syncthreads();
    far_refresh(L);
    far_seeds(L, p, pp, nbr, pos, rel);
    far_near_rows(L, p, pp, g, bstart, sorted, sorted_xy, rel);
    // Rings of the coarse grid until the cell is final: every unfinished point within twice its farthest vertex has been
    // applied -- points in unvisited coarse cells are at least r * s1 away (finished points farther than the fine rings
    // cannot be neighbours: they would not have finished) -- or the rings have left the grid (rims of holes and tears: their
    // cells close once the far side has been applied).
    const int rmax = kMidRingsMax;
    const int cbx = g1.bx(pp.x), cby = g1.by(pp.y);
    const int rgrid = max(max(cbx, g1.gx - 1 - cbx), max(cby, g1.gy - 1 - cby));
    bool done = false;
    int ra = -1;                                           // the last ring applied
    for (; ra < rmax && !done;) {
        // ring by ring while the cell is small; then annuli that grow by half their radius (one pass over their rows
        // instead of one per ring: the rim of a large hole needs a hundred rings)
        const int rb = ra < kMidRings ? ra + 1 : min(ra + max(ra / 2, 1), rmax);
        far_coarse_annulus(L, p, pp, ra, rb, g1, b1start, sorted1_pt, sorted1_xy, rel);
        double r2 = 0.0;
        const int n = L.n;
        for (int k = t; k < n; k += 64) r2 = fmax(r2, L.vx[k] * L.vx[k] + L.vy[k] * L.vy[k]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            r2 = fmax(r2, __hiloint2double(__shfl_xor(__double2hiint(r2), off), __shfl_xor(__double2loint(r2), off)));
        const double cover = (double)rb * g1.s;
        done = cover * cover >= 4.0 * r2 || rb >= rgrid;
        if (L.status) break;
        ra = rb;
    }
    __syncthreads();
    if (t == 0) far_wide[rank] = (done && !L.status && ra > kMidRings) ? 1 : 0;
    if (!done || L.status) { if (t == 0) far_deg[rank] = kDegLeft; return; }
    far_store(L, rank, head, far_deg, far_off, pool, pool_cap, &s_off);
}

// one wave per unfinished point; the grid is fixed and walks the ranks (their number stays on the device)
__global__ __launch_bounds__(64, 4)                        // (the pass waits on loads and votes: four waves per SIMD)
void dl_star_mid_kernel(const float *__restrict__ flow, int sign, int H, int W, DlHead *head,
                        const unsigned *__restrict__ bstart, const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy,
                        const unsigned *__restrict__ b1start, const unsigned *__restrict__ sorted1_pt, const P2 *__restrict__ sorted1_xy,
                        const unsigned *__restrict__ far_idx, const unsigned char *__restrict__ deg, const unsigned *__restrict__ nbr,
                        unsigned *__restrict__ far_deg, unsigned *__restrict__ far_off, int *__restrict__ pool, unsigned long long pool_cap,
                        unsigned char *__restrict__ far_wide)
{
    __shared__ FarLds<kMidCap, 64> L;
    __shared__ unsigned s_off;
    const unsigned n_far = head->n_far;
    for (unsigned rank = blockIdx.x; rank < n_far; rank += gridDim.x) {
        __syncthreads();                                   // the previous point's cell has been stored by every thread
        mid_point(L, s_off, rank, flow, sign, H, W, head, bstart, sorted, sorted_xy, b1start, sorted1_pt, sorted1_xy, far_idx, deg, nbr,
                  far_deg, far_off, pool, pool_cap, far_wide);
    }
}

template <int CAP, int NT>
__device__ void far_point(FarLds<CAP, NT> &L, unsigned &s_off, unsigned li, unsigned n_left,
                          const float *__restrict__ flow, int sign, int H, int W, DlHead *head,
                        const unsigned *__restrict__ bstart, const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy,
                        const unsigned *__restrict__ b1start, const unsigned *__restrict__ sorted1_pt, const P2 *__restrict__ sorted1_xy,
                        const unsigned *__restrict__ far_idx, const unsigned *__restrict__ left_idx,
                        const unsigned *__restrict__ left_pt, const P2 *__restrict__ left_xy, const double *__restrict__ left_box,
                        const unsigned *__restrict__ nbr, unsigned *__restrict__ far_deg, unsigned *__restrict__ far_off, int *__restrict__ pool,
                        unsigned long long pool_cap)
{
    const int t = threadIdx.x;
    const unsigned rank = left_idx[li];
    const int p = (int)left_pt[li];                      // (= far_idx[rank], and its position: one round trip instead of three)
    const P2 pp = left_xy[li];
    if (far_deg[rank] != kDegLeft) return;               // finished by the pass with the smaller capacity
    const Grid g = head->grid, g1 = head->grid1;
    const PosFn pos(flow, sign, W);
    auto rel = [&](int q) { const P2 v = pos(q); return P2{ v.x - pp.x, v.y - pp.y }; };
    if (t == 0) {
        Poly P{ L.vx, L.vy, L.tag, 1, CAP, 0 };
        poly_init(P);
        L.n = P.n; L.status = 0; L.t2 = head->far_t2;
    }
    __syncthreads();
    far_refresh(L);
    far_seeds(L, p, pp, nbr, pos, rel);
    far_near_rows(L, p, pp, g, bstart, sorted, sorted_xy, rel);
    far_coarse_annulus(L, p, pp, -1, kMidRings, g1, b1start, sorted1_pt, sorted1_xy, rel);
    // (Round 4 measured five more forms of this pass, each bit-identical in its results, none faster -- profiles/HISTORY.md: the
    // chunks nearest first with the box test repeated before every chunk (+ 2 .. 7 %); a chunk's 256 candidates in one round trip
    // under one vote (+ 15 .. 20 %); 5 and 6 waves per SIMD instead of 4 (no change); the sites in another order (no change);
    // scan first, clip afterwards -- every candidate only TESTED against the cell as it stands, loads of four to eight steps in
    // flight, the few cutters noted in LDS, sorted by distance and then clipped (+ 20 .. 60 %; with far_test / far_apply /
    // far_chunks out of line, a third of the code size: + 30 .. 100 %).  PMC: 7 000 vector + 5 000 scalar + 970 LDS + 120 memory
    // instructions per site, 81 % of the wave cycles waiting, 1 500 of 4 096 wave slots occupied on average.)
    // Every other left-over point -- but only the chunks of 256 whose bounding box could hold a site that cuts the cell AS IT
    // STANDS (later the cell only shrinks: its reach falls, its far vertices stay inside the present cone and below the present
    // largest distance, so what cannot cut now cannot cut later).  The test is far_test's, applied to a box: nearer than the
    // reach of the near vertices, or not excluded by the far cone.
    const unsigned n_chunks = (n_left + 255) / 256;
    // could chunk ck hold a site that cuts the cell as it stands now?
    auto chunk_keep = [&](unsigned ck) -> bool {
        bool keep = false;
#pragma unroll 1
        for (int half = 0; half < 2 && !keep; ++half) {
            const double *b = left_box + ((size_t)ck * 2 + half) * 8;
            const double ax = b[2], ay = b[3], t0 = b[4], t1 = b[5], s0 = b[6], s1 = b[7];
            if (!(t0 <= t1)) continue;                       // empty half
            const double rx = b[0] - pp.x, ry = b[1] - pp.y;              // the box origin seen from the site
            const double tp = -(rx * ax + ry * ay), sp = -(ry * ax - rx * ay);        // the site in the box frame
            const double dt = fmax(fmax(t0 - tp, tp - t1), 0.0), ds = fmax(fmax(s0 - sp, sp - s1), 0.0), dmin2 = dt * dt + ds * ds;
            if (dmin2 < L.reach2) { keep = true; break; }
            if (L.nfar == 0) continue;
            if (!L.cone) { keep = true; break; }
            double mmax = 0.0, amax = 0.0;
            bool right0 = true, left1 = true;                // every corner strictly outside one side of the cone?
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double tt = (k & 1) ? t1 : t0, ss = (k & 2) ? s1 : s0;
                const double cx = rx + tt * ax - ss * ay, cy = ry + tt * ay + ss * ax;
                mmax = fmax(mmax, fmax(L.c0x * cx + L.c0y * cy, L.c1x * cx + L.c1y * cy));
                amax = fmax(amax, fabs(cx) + fabs(cy));
                right0 = right0 && (L.c0x * cy - L.c0y * cx < 0.0);
                left1 = left1 && (cx * L.c1y - cy * L.c1x < 0.0);
            }
            // (the corners are rounded: a margin of 1e-9 of their size on the dot products, as on the sites themselves)
            if (!((right0 || left1) && mmax + 2e-9 * amax < dmin2 * L.kcone)) keep = true;
        }
        return keep;
    };
    for (unsigned cbase = 0; cbase < n_chunks; cbase += NT) {
        __syncthreads();
        const unsigned ck = cbase + t;
        const bool keep = ck < n_chunks && chunk_keep(ck);
        // ordered compaction of the kept chunk numbers of this group
        const unsigned long long bal = __ballot(keep);
        if ((t & 63) == 0) L.hit[t >> 6] = bal;
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int w = 0; w < NT / 64; ++w) { const unsigned c = (unsigned)__popcll(L.hit[w]); if (w < (t >> 6)) before += c; total += c; }
        if (keep) L.clist[before + (unsigned)__popcll(bal & ((1ull << (t & 63)) - 1ull))] = ck;
        __syncthreads();
        constexpr int kVote = NT == 64 ? 1 : 4;            // steps under one vote (a wave's own vote is cheap)
        constexpr int kPer = 256 / NT;                     // steps of NT candidates per chunk of 256
        for (unsigned k0 = 0; k0 < total * kPer; k0 += kVote) {
            int cand[kVote];
            P2  q[kVote];
            unsigned cks[kVote];
#pragma unroll
            for (int k = 0; k < kVote; ++k) cks[k] = (k0 + k) / kPer < total ? L.clist[(k0 + k) / kPer] : 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < kVote; ++k) {
                const unsigned j = cks[k] * 256u + ((k0 + k) % kPer) * NT + t;
                const bool in = cks[k] != 0xFFFFFFFFu && j < n_left;
                cand[k] = in ? (int)left_pt[j] : -1;
                q[k] = in ? left_xy[j] : pp;
            }
            far_chunks<kVote>(L, p, pp, cand, q, rel);
        }
    }
    __syncthreads();
    if (CAP < kFarCap && L.status) return;               // overflow of the small capacity: far_deg stays kDegLeft for the next pass
    far_store(L, rank, head, far_deg, far_off, pool, pool_cap, &s_off);
}

constexpr int kFarWaves = 4;        // waves per SIMD of the single-wave form
constexpr int kFarSmallCap = 384;   // its cell capacity
template <int CAP, int NT>          // first single waves with a small cell capacity, then -- for the few fans that overflowed it -- workgroups with the large one
__global__ __launch_bounds__(NT, NT == 64 ? kFarWaves : 1)
void dl_star_far_kernel(const float *__restrict__ flow, int sign, int H, int W, DlHead *head,
                        const unsigned *__restrict__ bstart, const unsigned *__restrict__ sorted, const P2 *__restrict__ sorted_xy,
                        const unsigned *__restrict__ b1start, const unsigned *__restrict__ sorted1_pt, const P2 *__restrict__ sorted1_xy,
                        const unsigned *__restrict__ far_idx, const unsigned *__restrict__ left_idx,
                        const unsigned *__restrict__ left_pt, const P2 *__restrict__ left_xy, const double *__restrict__ left_box,
                        const unsigned *__restrict__ nbr, unsigned *__restrict__ far_deg, unsigned *__restrict__ far_off, int *__restrict__ pool,
                        unsigned long long pool_cap)
{
    __shared__ FarLds<CAP, NT> L;
    __shared__ unsigned s_off;
    const unsigned n_left = head->n_left;
    for (unsigned lb = blockIdx.x; lb < n_left; lb += gridDim.x) {
        __syncthreads();
        const unsigned li = lb;
        far_point<CAP, NT>(L, s_off, li, n_left, flow, sign, H, W, head, bstart, sorted, sorted_xy, b1start, sorted1_pt, sorted1_xy, far_idx,
                       left_idx, left_pt, left_xy, left_box, nbr, far_deg, far_off, pool, pool_cap);
    }
}

}  // namespace

// the host side of the stage: what each entry reads, writes and borrows is stated at its declaration (ofl_delaunay_ws.h)
namespace ofl_dlw {

void stars_rim(const DlIn &in, DlWs &ws, hipStream_t s)
{
    hipLaunchKernelGGL(dl_star_mid_kernel, dim3(walk_groups((size_t)in.H * in.W)), dim3(64), 0, s, in.flow, in.sign_pp, in.H, in.W, ws.head,
                       ws.bstart, ws.sorted, ws.sorted_xy, ws.b1start, ws.sorted1_pt, ws.sorted1_xy, ws.far_idx, ws.deg, ws.nbr,
                       ws.far_deg, ws.far_off, ws.pool, (unsigned long long)ws.pool_cap, ws.far_wide);
}

void stars_leftover(const DlIn &in, DlWs &ws, hipStream_t s)
{
    const size_t n = (size_t)in.H * in.W;
    const unsigned rblk = std::min<unsigned>((unsigned)((n + 255) / 256), 2048u), walk = walk_groups(n);
    hipLaunchKernelGGL(dl_left_box_kernel, dim3(rblk), dim3(256), 0, s, ws.head, in.W, ws.left_pt, ws.left_xy, ws.left_box);
    auto far = [&](auto kernel, unsigned groups, unsigned threads) {
        hipLaunchKernelGGL(kernel, dim3(groups), dim3(threads), 0, s, in.flow, in.sign_pp, in.H, in.W, ws.head,
                           ws.bstart, ws.sorted, ws.sorted_xy, ws.b1start, ws.sorted1_pt, ws.sorted1_xy, ws.far_idx, ws.left_idx,
                           ws.left_pt, ws.left_xy, ws.left_box, ws.nbr, ws.far_deg, ws.far_off, ws.pool, (unsigned long long)ws.pool_cap);
    };
    far(dl_star_far_kernel<kFarSmallCap, 64>, walk, 64);
    far(dl_star_far_kernel<kFarCap, 256>, std::min<unsigned>(walk, 2048u), 256);
}

}  // namespace ofl_dlw
