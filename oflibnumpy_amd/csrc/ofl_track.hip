// ofl_track.hip -- K10: point tracking on HBM-resident fields and points (gfx950).
// Replaces the NumPy halves of track_pts (utils.py:547-622) and Flow.track (flow_class.py:755-795): the points stay on
// the device between steps, the field is never moved.  Every result is the float64 sequence the host path computes
// (sample_points_kernel's bilinear sample, then one float64 add), so no operation here may be contracted into an FMA.
//
// Latency-bound kernels: each step of a point is four dependent 8-byte gathers.  Nothing is staged in LDS and no lane
// talks to another; throughput comes from the number of points in flight, so the kernels are held to 64 VGPRs (eight
// waves per SIMD) and issue the four taps of a step together.
#include "ofl_common.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

// The reference's area test, utils.py:596-597: 0 <= row <= H - 1 and 0 <= col <= W - 1.  False for NaN.
__device__ __forceinline__ bool in_area(double r, double c, int H, int W)
{
    return (r >= 0.0) && (r <= (double)(H - 1)) && (c >= 0.0) && (c <= (double)(W - 1));
}

// map[rint(r)][rint(c)] (np.round: round-half-even), 0 when the rounded position is no pixel of the field (NaN included).
__device__ __forceinline__ uint32_t status_at(const uint8_t *__restrict__ map, int H, int W, double r, double c)
{
    const double rr = rint(r), rc = rint(c);
    if (!((rr >= 0.0) && (rr <= (double)(H - 1)) && (rc >= 0.0) && (rc <= (double)(W - 1)))) return 0u;
    return map[(size_t)(int)rr * W + (int)rc] ? 1u : 0u;
}

// One bilinear step of a point INSIDE the area: p + sample(p), sample exactly as sample_points_kernel (ofl_stats.hip)
// computes it -- clipped corner indices, weights from the clipped corners (0 on the last row and column), the sum taken
// left to right -- followed by the float64 add of utils.py:617.
__device__ __forceinline__ void bilinear_step(const float2 *__restrict__ f, int H, int W, double &ver, double &hor)
{
    const int v0 = (int)floor(ver), h0 = (int)floor(hor);
    const int v0c = min(max(v0, 0), H - 1), h0c = min(max(h0, 0), W - 1);
    const int v1c = min(max(v0 + 1, 0), H - 1), h1c = min(max(h0 + 1, 0), W - 1);
    const float2 da = f[(size_t)v0c * W + h0c];
    const float2 db = f[(size_t)v1c * W + h0c];
    const float2 dc = f[(size_t)v0c * W + h1c];
    const float2 dd = f[(size_t)v1c * W + h1c];
    const double w_a = ((double)v1c - ver) * ((double)h1c - hor), w_b = ((double)v1c - ver) * (hor - (double)h0c);
    const double w_c = (ver - (double)v0c) * ((double)h1c - hor), w_d = (ver - (double)v0c) * (hor - (double)h0c);
    const double sv = ((w_a * (double)da.y + w_b * (double)db.y) + w_c * (double)dc.y) + w_d * (double)dd.y;
    const double su = ((w_a * (double)da.x + w_b * (double)db.x) + w_c * (double)dc.x) + w_d * (double)dd.x;
    ver = ver + sv;
    hor = hor + su;
}

__device__ __forceinline__ bool field_moves(const uint32_t *__restrict__ stats, int b)
{
    return !stats || (stats[b] & OFL_STAT_NONZERO_TH) != 0u;     // is_zero_flow(flow, thresholded=True) is the identity, utils.py:588
}

__device__ __forceinline__ void store_point(void *__restrict__ out, size_t i, double r, double c, int int_out)
{
    if (int_out) reinterpret_cast<int2 *>(out)[i] = make_int2((int)rint(r), (int)rint(c));      // np.round(..).astype('i')
    else         reinterpret_cast<double2 *>(out)[i] = make_double2(r, c);
}

// ref 's', bilinear sampling.  CHAIN = false: lane (b, p) applies field b to point p, out[b][p]; a point outside the area is
// left unchanged and counted.  CHAIN = true: lane p takes its point through fields 0 .. B-1, position in registers; a point
// whose position before step k is outside the area is frozen there and lost_at[p] = k.
template <bool CHAIN>
__global__ __launch_bounds__(256, 8)
void track_bilinear_kernel(const float *__restrict__ flows, int B, int H, int W, const double *__restrict__ pts, size_t n,
                           const uint32_t *__restrict__ stats, const uint8_t *__restrict__ valid, int int_out,
                           void *__restrict__ out, uint8_t *__restrict__ status, uint32_t *__restrict__ outside,
                           int32_t *__restrict__ lost_at, double *__restrict__ path)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t px = (size_t)H * W;
    if (CHAIN) {
        if (i >= n) return;
        const double2 p0 = reinterpret_cast<const double2 *>(pts)[i];
        double ver = p0.x, hor = p0.y;
        int lost = -1;
        uint32_t ok = 1u;
        if (path) reinterpret_cast<double2 *>(path)[i] = p0;
        for (int k = 0; k < B; ++k) {
            if (lost < 0) {
                if (!in_area(ver, hor, H, W)) {
                    lost = k;
                    ok = 0u;
                } else {
                    if (valid) ok &= status_at(valid + (size_t)k * px, H, W, ver, hor);
                    if (field_moves(stats, k)) bilinear_step(reinterpret_cast<const float2 *>(flows) + (size_t)k * px, H, W, ver, hor);
                }
            }
            if (path) reinterpret_cast<double2 *>(path)[(size_t)(k + 1) * n + i] = make_double2(ver, hor);
        }
        store_point(out, i, ver, hor, int_out);
        lost_at[i] = lost;
        if (status) status[i] = (uint8_t)ok;
    } else {
        if (i >= (size_t)B * n) return;
        const int b = (int)(i / n);
        const size_t p = i - (size_t)b * n;
        const double2 p0 = reinterpret_cast<const double2 *>(pts)[p];
        double ver = p0.x, hor = p0.y;
        if (status) status[i] = (uint8_t)status_at(valid + (size_t)b * px, H, W, ver, hor);
        if (field_moves(stats, b)) {
            if (in_area(ver, hor, H, W)) bilinear_step(reinterpret_cast<const float2 *>(flows) + (size_t)b * px, H, W, ver, hor);
            else atomicAdd(outside, 1u);
        }
        store_point(out, i, ver, hor, int_out);
    }
}

// ref 's', integer points: (double)p + (double)flow[row, col, ::-1] (utils.py:591).  Indices outside [0, H) x [0, W) are
// counted and left unchanged.
template <typename I>
__global__ __launch_bounds__(256, 8)
void track_pixels_kernel(const float *__restrict__ flow, int H, int W, const I *__restrict__ pts, size_t n,
                         const uint32_t *__restrict__ stats, const uint8_t *__restrict__ valid, int int_out,
                         void *__restrict__ out, uint8_t *__restrict__ status, uint32_t *__restrict__ outside)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const I r = pts[2 * i], c = pts[2 * i + 1];
    const bool inside = r >= 0 && r < (I)H && c >= 0 && c < (I)W;
    double ver = (double)r, hor = (double)c;
    if (status) status[i] = (uint8_t)((inside && valid[(size_t)r * W + (size_t)c]) ? 1u : 0u);
    if (field_moves(stats, 0)) {
        if (inside) {
            const float2 f = reinterpret_cast<const float2 *>(flow)[(size_t)r * W + (size_t)c];
            ver = ver + (double)f.y;
            hor = hor + (double)f.x;
        } else {
            atomicAdd(outside, 1u);
        }
    }
    store_point(out, i, ver, hor, int_out);
}

// (row, col) points of any accepted dtype -> the float64 (x, y) queries of ofl_scatter_query_dev (pts[:, ::-1].astype(float64))
template <typename T>
__global__ __launch_bounds__(256)
void track_query_points_kernel(const T *__restrict__ pts, size_t n, double *__restrict__ query_xy)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    reinterpret_cast<double2 *>(query_xy)[i] = make_double2((double)pts[2 * i + 1], (double)pts[2 * i]);
}

// The tail of the query paths (ref 't', s_exact_mode; utils.py:603-618): swap the interpolated (u, v) back to (row, col),
// add, and treat the points griddata found no triangle for.  step < 0, one call of track_pts: such a point becomes (0, 0).
// step >= 0, step `step` of a sequence: it is lost -- frozen where it is, lost_at[i] = step -- and a point lost earlier stays
// frozen; status[i] is ANDed over the steps and 0 for lost points.
__global__ __launch_bounds__(256, 8)
void track_query_epilogue_kernel(const double *__restrict__ query_xy, const double *__restrict__ vals_uv,
                                 const uint8_t *__restrict__ found, size_t n, int H, int W,
                                 const uint32_t *__restrict__ stats, const uint8_t *__restrict__ valid, int step,
                                 double *__restrict__ out_rc, int32_t *__restrict__ out_int, double *__restrict__ next_query_xy,
                                 uint8_t *__restrict__ status, int32_t *__restrict__ lost_at)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double2 q = reinterpret_cast<const double2 *>(query_xy)[i];
    double ver = q.y, hor = q.x;
    const bool moves = field_moves(stats, 0);
    const bool hit = found[i] != 0;
    uint32_t ok = valid ? status_at(valid, H, W, ver, hor) : 1u;
    if (step < 0) {
        if (moves) {
            if (hit) {
                const double2 uv = reinterpret_cast<const double2 *>(vals_uv)[i];
                ver = ver + uv.y;
                hor = hor + uv.x;
            } else {
                ver = 0.0;                  // warped[~found] = 0, utils.py:616-618
                hor = 0.0;
            }
        }
    } else {
        int lost = step > 0 ? lost_at[i] : -1;
        if (step > 0 && status) ok &= (uint32_t)status[i];
        if (lost < 0 && moves) {
            if (hit) {
                const double2 uv = reinterpret_cast<const double2 *>(vals_uv)[i];
                ver = ver + uv.y;
                hor = hor + uv.x;
            } else {
                lost = step;
            }
        }
        if (lost >= 0) ok = 0u;
        lost_at[i] = lost;
    }
    if (out_rc) reinterpret_cast<double2 *>(out_rc)[i] = make_double2(ver, hor);
    if (out_int) reinterpret_cast<int2 *>(out_int)[i] = make_int2((int)rint(ver), (int)rint(hor));
    if (next_query_xy) reinterpret_cast<double2 *>(next_query_xy)[i] = make_double2(hor, ver);
    if (status) status[i] = (uint8_t)ok;
}

int point_grid(const char *who, size_t items, unsigned &grid)
{
    const size_t nb = (items + 255) / 256;
    if (nb > 0x7fffffffull) return fail(OFL_E_INVALID, "%s: too many points for one launch", who);
    grid = (unsigned)nb;
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_track_bilinear_dev(const float *flows, int B, int H, int W, int chain, const double *pts_rc, size_t n,
                           const uint32_t *stats, const uint8_t *valid, int int_out, void *out, uint8_t *status,
                           uint32_t *outside_count, int32_t *lost_at, double *path, void *stream)
{
    OFL_TRY(need_device());
    if (!flows || B <= 0 || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_track_bilinear: bad field arguments");
    if (n == 0) return OFL_OK;
    if (!pts_rc || !out) return fail(OFL_E_INVALID, "ofl_track_bilinear: NULL pointer");
    if ((status != nullptr) != (valid != nullptr)) return fail(OFL_E_INVALID, "ofl_track_bilinear: status and valid come together");
    if (chain ? !lost_at : !outside_count)
        return fail(OFL_E_INVALID, "ofl_track_bilinear: %s", chain ? "a sequence needs lost_at" : "independent fields need outside_count");
    if (!chain && path) return fail(OFL_E_INVALID, "ofl_track_bilinear: a path exists only in a sequence");
    if (n > (~(size_t)0) / 32 / (size_t)B) return fail(OFL_E_INVALID, "ofl_track_bilinear: B * n overflows");
    unsigned grid = 0;
    OFL_TRY(point_grid("ofl_track_bilinear", chain ? n : (size_t)B * n, grid));
    hipStream_t s = stream_of(stream);
    if (chain)
        hipLaunchKernelGGL(track_bilinear_kernel<true>, dim3(grid), dim3(256), 0, s, flows, B, H, W, pts_rc, n, stats, valid,
                           int_out, out, status, outside_count, lost_at, path);
    else
        hipLaunchKernelGGL(track_bilinear_kernel<false>, dim3(grid), dim3(256), 0, s, flows, B, H, W, pts_rc, n, stats, valid,
                           int_out, out, status, outside_count, lost_at, path);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_track_pixels_dev(const float *flow, int H, int W, const void *pts_rc, int pts_dtype, size_t n,
                         const uint32_t *stats, const uint8_t *valid, int int_out, void *out, uint8_t *status,
                         uint32_t *outside_count, void *stream)
{
    OFL_TRY(need_device());
    if (!flow || H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_track_pixels: bad field arguments");
    if (pts_dtype != OFL_TRACK_I32 && pts_dtype != OFL_TRACK_I64) return fail(OFL_E_INVALID, "ofl_track_pixels: points must be int32 or int64");
    if (n == 0) return OFL_OK;
    if (!pts_rc || !out || !outside_count) return fail(OFL_E_INVALID, "ofl_track_pixels: NULL pointer");
    if ((status != nullptr) != (valid != nullptr)) return fail(OFL_E_INVALID, "ofl_track_pixels: status and valid come together");
    unsigned grid = 0;
    OFL_TRY(point_grid("ofl_track_pixels", n, grid));
    hipStream_t s = stream_of(stream);
    if (pts_dtype == OFL_TRACK_I32)
        hipLaunchKernelGGL(track_pixels_kernel<int32_t>, dim3(grid), dim3(256), 0, s, flow, H, W, (const int32_t *)pts_rc, n, stats,
                           valid, int_out, out, status, outside_count);
    else
        hipLaunchKernelGGL(track_pixels_kernel<int64_t>, dim3(grid), dim3(256), 0, s, flow, H, W, (const int64_t *)pts_rc, n, stats,
                           valid, int_out, out, status, outside_count);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_track_query_points_dev(const void *pts_rc, int pts_dtype, size_t n, double *query_xy, void *stream)
{
    OFL_TRY(need_device());
    if (pts_dtype != OFL_TRACK_F64 && pts_dtype != OFL_TRACK_I32 && pts_dtype != OFL_TRACK_I64)
        return fail(OFL_E_INVALID, "ofl_track_query_points: points must be float64, int32 or int64");
    if (n == 0) return OFL_OK;
    if (!pts_rc || !query_xy) return fail(OFL_E_INVALID, "ofl_track_query_points: NULL pointer");
    unsigned grid = 0;
    OFL_TRY(point_grid("ofl_track_query_points", n, grid));
    hipStream_t s = stream_of(stream);
    if (pts_dtype == OFL_TRACK_F64)
        hipLaunchKernelGGL(track_query_points_kernel<double>, dim3(grid), dim3(256), 0, s, (const double *)pts_rc, n, query_xy);
    else if (pts_dtype == OFL_TRACK_I32)
        hipLaunchKernelGGL(track_query_points_kernel<int32_t>, dim3(grid), dim3(256), 0, s, (const int32_t *)pts_rc, n, query_xy);
    else
        hipLaunchKernelGGL(track_query_points_kernel<int64_t>, dim3(grid), dim3(256), 0, s, (const int64_t *)pts_rc, n, query_xy);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_track_query_epilogue_dev(const double *query_xy, const double *vals_uv, const uint8_t *found, size_t n, int H, int W,
                                 const uint32_t *stats, const uint8_t *valid, int step, double *out_rc, int32_t *out_int,
                                 double *next_query_xy, uint8_t *status, int32_t *lost_at, void *stream)
{
    OFL_TRY(need_device());
    if (H <= 0 || W <= 0) return fail(OFL_E_INVALID, "ofl_track_query_epilogue: bad shape");
    if (n == 0) return OFL_OK;
    if (!query_xy || !vals_uv || !found || (!out_rc && !out_int && !next_query_xy)) return fail(OFL_E_INVALID, "ofl_track_query_epilogue: NULL pointer");
    if ((status != nullptr) != (valid != nullptr)) return fail(OFL_E_INVALID, "ofl_track_query_epilogue: status and valid come together");
    if (step >= 0 && !lost_at) return fail(OFL_E_INVALID, "ofl_track_query_epilogue: a sequence step needs lost_at");
    unsigned grid = 0;
    OFL_TRY(point_grid("ofl_track_query_epilogue", n, grid));
    hipLaunchKernelGGL(track_query_epilogue_kernel, dim3(grid), dim3(256), 0, stream_of(stream), query_xy, vals_uv, found, n, H, W,
                       stats, valid, step, out_rc, out_int, next_query_xy, status, lost_at);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

}  // extern "C"
