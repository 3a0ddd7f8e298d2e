// ofl_fill.hip -- K15: the vectors of masked-out pixels from the nearest valid pixel (gfx950); the definition is in
// include/ofl.h.  Exact integer arithmetic throughout: squared distances stay below 2^31 (H, W <= 32766).
//
// fill_row_kernel, one workgroup of 256 threads per row of one field.  A wave takes the 64-pixel words w, w + 4, ... of the
// row: every lane loads its mask byte (and its valid byte; the loads of four words are asked for together), the ballot of
// the 64 source bits goes to LDS together with the word's first and last source column.  An inclusive prefix maximum of the last columns and a suffix minimum of the first
// columns over the <= 512 words (Hillis-Steele in LDS, ceil(log2(words)) steps) is the carry across words.  Then every lane
// finds the nearest set bit at or below its own (clz of the word masked to bits 0 .. lane) and at or above it (ffs of the
// word shifted down by lane), falls back to the carry of the neighbouring word, and keeps the nearer one -- the left one on a
// tie, which is the smaller column.  The signed offset goes to the workspace as int16, 2 B/px, lanes along x; kNone
// (-32768, outside +-32765) where the row has no source or the nearest lies beyond max_d2.
//
// fill_col_kernel, 256 consecutive columns of four consecutive rows per workgroup, lanes along x, the rows one after the
// other: starting from the row's own offset a lane scans the rows y - k and y + k for k = 1, 2, ..., reads their offsets
// (coalesced, 2 B/lane), and keeps the minimum of k^2 + off^2.  The offsets of eight steps (16 loads) are asked for
// together and then judged in the order of k, each step behind the same stop test, so the result is that of the step-by-step
// scan.  The candidate rows are met in the order y, y - 1, y + 1, y - 2, ...: a row above has a smaller qy than all
// rows met before and takes a tie (<=), a row below has a larger one and needs to be strictly nearer (<).  No farther row
// can win once k^2 > min(best, max_d2): equal is not enough, a row above at distance k with offset 0 still takes the tie.
// Which outputs exist is a template argument (no pointer test in the body): 14 instantiations of the column pass, 2 of the
// row pass (with and without `valid`).
#include <stddef.h>
#include "ofl_common.h"
#include "ofl_host_stage.h"

using namespace ofl;

namespace {

constexpr int      kThreads = 256, kMaxDim = 32766, kMaxWords = (kMaxDim + 63) / 64;
constexpr int      kRowWords = 4;                          // row pass: 64-pixel words per wave and round of loads
constexpr int      kColRows = 4, kScan = 8;                 // column pass: rows per workgroup, scan steps per round of loads
constexpr int      kNone = -32768;                          // the workspace's "no source": offsets reach +-32765
constexpr uint32_t kFar = 0xFFFFFFFFu;                      // d2 of a pixel that is not filled
constexpr int      kNoCol = 0x7FFFFFFF;

static_assert(kMaxWords == 512 && 2 * (int64_t)(kMaxDim - 1) * (kMaxDim - 1) < ((int64_t)1 << 31), "limits");

struct FArgs {
    const uint2   *vecs;             // 8 bytes per pixel, moved as two words
    const uint8_t *mask, *valid;
    int16_t       *off;              // the workspace: [batch][H][W]
    uint2         *out_vecs;
    uint8_t       *out_mask;
    int32_t       *index;
    uint32_t      *d2;
    int            H, W;
    uint32_t       cap;              // max_d2, or 2^31 - 1 for "no limit": every distance is below it
};

template <bool VALID>
__global__ __launch_bounds__(kThreads)
void fill_row_kernel(const FArgs a)
{
    __shared__ uint64_t bits[kMaxWords];
    __shared__ int      last[kMaxWords], first[kMaxWords];
    const int W = a.W, words = (W + 63) >> 6, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const size_t base = ((size_t)blockIdx.y * a.H + blockIdx.x) * (size_t)W;

    // kRowWords words per wave and round: their loads are asked for together, then one ballot per word
    for (int w0 = wave; w0 < words; w0 += kRowWords * (kThreads / 64)) {
        uint32_t m[kRowWords];
#pragma unroll
        for (int j = 0; j < kRowWords; ++j) {
            const int x = (w0 + j * (kThreads / 64)) * 64 + lane;
            m[j] = 0;
            if (x < W) {
                m[j] = a.mask[base + x];
                if (VALID) m[j] &= a.valid[base + x];
            }
        }
#pragma unroll
        for (int j = 0; j < kRowWords; ++j) {
            const int w = w0 + j * (kThreads / 64);
            if (w >= words) break;                                               // wave-uniform
            const uint64_t b = __builtin_amdgcn_ballot_w64(m[j] != 0);
            if (lane == 0) {
                bits[w] = b;
                last[w] = b ? w * 64 + 63 - __clzll((long long)b) : -1;
                first[w] = b ? w * 64 + __ffsll((unsigned long long)b) - 1 : kNoCol;
            }
        }
    }
    __syncthreads();
    // last[w] <- the last source column of the words 0 .. w, first[w] <- the first source column of the words w .. end
    for (int d = 1; d < words; d <<= 1) {
        int l[2], f[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = t + j * kThreads;
            l[j] = -1; f[j] = kNoCol;
            if (i < words) {
                l[j] = last[i]; f[j] = first[i];
                if (i >= d) l[j] = max(l[j], last[i - d]);
                if (i + d < words) f[j] = min(f[j], first[i + d]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = t + j * kThreads;
            if (i < words) { last[i] = l[j]; first[i] = f[j]; }
        }
        __syncthreads();
    }

    for (int w = wave; w < words; w += kThreads / 64) {
        const int x = w * 64 + lane;
        const uint64_t b = bits[w];
        const uint64_t lo = b & (~0ull >> (63 - lane)), hi = b >> lane;          // the bits 0 .. lane; the bits lane .. 63 moved down
        int left = w > 0 ? last[w - 1] : -1, right = w + 1 < words ? first[w + 1] : kNoCol;
        if (lo) left = w * 64 + 63 - __clzll((long long)lo);
        if (hi) right = x + __ffsll((unsigned long long)hi) - 1;
        const int dl = left >= 0 ? x - left : kNoCol, dr = right != kNoCol ? right - x : kNoCol;
        int off = dl <= dr ? -dl : dr;                                           // a tie: the smaller column
        if (min(dl, dr) == kNoCol || (uint32_t)(off * off) > a.cap) off = kNone;
        if (x < W) a.off[base + x] = (int16_t)off;
    }
}

template <bool VECS, bool MASK, bool INDEX, bool D2>
__global__ __launch_bounds__(kThreads)
void fill_col_kernel(const FArgs a)
{
    const int W = a.W, H = a.H, x = blockIdx.x * kThreads + threadIdx.x;
    if (x >= W) return;
    const size_t item = (size_t)blockIdx.z * H * (size_t)W;
    const int16_t *__restrict__ col = a.off + item + x;                          // col[r * W]: this column's offset in row r
    const int y0 = blockIdx.y * kColRows, y1 = min(y0 + kColRows, H);

    for (int y = y0; y < y1; ++y) {
        const size_t here = (size_t)y * W + x;
        uint32_t best = kFar, bound = a.cap;                                     // bound = min(best, cap)
        int by = y, bo = 0;
        {
            const int o = col[(size_t)y * W];
            if (o != kNone) { best = bound = (uint32_t)(o * o); bo = o; }        // the row pass has applied the cap
        }
        const int up = y, down = H - 1 - y, reach = max(up, down);
        // kScan steps per round: their 2 * kScan loads are asked for together, then the rows are judged in the order of k
        for (int k0 = 1; k0 <= reach && (uint32_t)(k0 * k0) <= bound; k0 += kScan) {
            int ou[kScan], od[kScan];
#pragma unroll
            for (int j = 0; j < kScan; ++j) {
                const int k = k0 + j;
                ou[j] = k <= up ? (int)col[(size_t)(y - k) * W] : kNone;
                od[j] = k <= down ? (int)col[(size_t)(y + k) * W] : kNone;
            }
#pragma unroll
            for (int j = 0; j < kScan; ++j) {
                const int k = k0 + j;
                const uint32_t kk = (uint32_t)(k * k);
                if (kk > bound) break;                                           // no farther row can win; equal still can
                if (ou[j] != kNone) {
                    const uint32_t d = kk + (uint32_t)(ou[j] * ou[j]);
                    if (d <= bound) { best = bound = d; by = y - k; bo = ou[j]; }        // a row above takes a tie
                }
                if (od[j] != kNone) {
                    const uint32_t d = kk + (uint32_t)(od[j] * od[j]);
                    if (d <= bound && d != best) { best = bound = d; by = y + k; bo = od[j]; }      // a row below: strictly nearer only
                }
            }
        }

        const bool filled = best != kFar;
        const size_t near = filled ? (size_t)by * W + (size_t)(x + bo) : here;
        if (INDEX) a.index[item + here] = filled ? (int32_t)near : -1;
        if (D2)    a.d2[item + here] = best;
        if (MASK)  a.out_mask[item + here] = filled ? 1 : 0;
        if (VECS)  a.out_vecs[item + here] = a.vecs[item + near];
    }
}

template <bool VECS, bool MASK>
void launch_col(int outs, const FArgs &a, dim3 grid, hipStream_t s)
{
    switch (outs) {
    case 0:  hipLaunchKernelGGL((fill_col_kernel<VECS, MASK, false, false>), grid, dim3(kThreads), 0, s, a); break;
    case 1:  hipLaunchKernelGGL((fill_col_kernel<VECS, MASK, true, false>), grid, dim3(kThreads), 0, s, a); break;
    case 2:  hipLaunchKernelGGL((fill_col_kernel<VECS, MASK, false, true>), grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((fill_col_kernel<VECS, MASK, true, true>), grid, dim3(kThreads), 0, s, a); break;
    }
}

// without vectors index or d2 exists (check_fill_args): outs 0 is never asked for there
template <bool MASK>
void launch_col_plain(int outs, const FArgs &a, dim3 grid, hipStream_t s)
{
    switch (outs) {
    case 1:  hipLaunchKernelGGL((fill_col_kernel<false, MASK, true, false>), grid, dim3(kThreads), 0, s, a); break;
    case 2:  hipLaunchKernelGGL((fill_col_kernel<false, MASK, false, true>), grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((fill_col_kernel<false, MASK, true, true>), grid, dim3(kThreads), 0, s, a); break;
    }
}

inline bool sizes_ok(int H, int W, int batch) { return H >= 1 && W >= 1 && H <= kMaxDim && W <= kMaxDim && batch >= 1 && batch <= 65535; }

int check_fill_args(const char *who, const void *vecs, const void *mask, const void *valid, int H, int W, int batch, int max_d2,
                    const void *out_vecs, const void *out_mask, const void *index, const void *d2)
{
    if (!mask) return fail(OFL_E_INVALID, "%s: NULL pointer (mask is required)", who);
    if ((vecs == nullptr) != (out_vecs == nullptr))
        return fail(OFL_E_INVALID, "%s: vecs and out_vecs must both be given or both be NULL", who);
    if (!vecs && !index && !d2)
        return fail(OFL_E_INVALID, "%s: nothing to write (without vectors, index or d2 is required)", who);
    if (!sizes_ok(H, W, batch))
        return fail(OFL_E_INVALID, "%s: H, W must be in [1, %d] and batch in [1, 65535] (got %d x %d, %d)", who, kMaxDim, H, W, batch);
    if (max_d2 < -1) return fail(OFL_E_INVALID, "%s: max_d2 must be >= 0, or -1 for no limit (got %d)", who, max_d2);
    if ((vecs && out_vecs == vecs) || (out_mask && (out_mask == mask || out_mask == valid)))
        return fail(OFL_E_INVALID, "%s: outputs must not alias inputs", who);
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_fill_workspace_bytes(int H, int W, int batch, size_t *bytes)
{
    if (!bytes) return fail(OFL_E_INVALID, "ofl_fill_workspace_bytes: NULL pointer");
    if (!sizes_ok(H, W, batch))
        return fail(OFL_E_INVALID, "ofl_fill_workspace_bytes: H, W in [1, %d] and batch in [1, 65535] (got %d x %d, %d)", kMaxDim, H, W, batch);
    *bytes = (size_t)batch * H * W * sizeof(int16_t);
    return OFL_OK;
}

int ofl_fill_dev(const float *vecs, const uint8_t *mask, const uint8_t *valid, int H, int W, int batch, int max_d2,
                 void *workspace, size_t workspace_bytes, float *out_vecs, uint8_t *out_mask, int32_t *index, uint32_t *d2,
                 void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_fill_args("ofl_fill", vecs, mask, valid, H, W, batch, max_d2, out_vecs, out_mask, index, d2));
    const size_t need = (size_t)batch * H * W * sizeof(int16_t);
    if (!workspace || workspace_bytes < need)
        return fail(OFL_E_INVALID, "ofl_fill: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    if (!host_aligned(vecs, 8) || !host_aligned(out_vecs, 8) || !host_aligned(index, 4) || !host_aligned(d2, 4) || !host_aligned(workspace, 2))
        return fail(OFL_E_INVALID, "ofl_fill: vecs and out_vecs must be 8-byte, index and d2 4-byte, workspace 2-byte aligned");
    FArgs a;
    a.vecs = reinterpret_cast<const uint2 *>(vecs); a.mask = mask; a.valid = valid;
    a.off = static_cast<int16_t *>(workspace);
    a.out_vecs = reinterpret_cast<uint2 *>(out_vecs); a.out_mask = out_mask; a.index = index; a.d2 = d2;
    a.H = H; a.W = W;
    a.cap = max_d2 < 0 ? 0x7FFFFFFFu : (uint32_t)max_d2;
    hipStream_t s = stream_of(stream);
    const dim3 rows((unsigned)H, (unsigned)batch);
    if (valid) hipLaunchKernelGGL(fill_row_kernel<true>, rows, dim3(kThreads), 0, s, a);
    else       hipLaunchKernelGGL(fill_row_kernel<false>, rows, dim3(kThreads), 0, s, a);
    OFL_HIP(hipGetLastError());
    const dim3 grid((unsigned)((W + kThreads - 1) / kThreads), (unsigned)((H + kColRows - 1) / kColRows), (unsigned)batch);
    const int outs = (index ? 1 : 0) | (d2 ? 2 : 0);
    if (vecs) {
        if (out_mask) launch_col<true, true>(outs, a, grid, s);
        else          launch_col<true, false>(outs, a, grid, s);
    } else {
        if (out_mask) launch_col_plain<true>(outs, a, grid, s);
        else          launch_col_plain<false>(outs, a, grid, s);
    }
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_fill(const float *vecs, const uint8_t *mask, const uint8_t *valid, int H, int W, int batch, int max_d2,
             float *out_vecs, uint8_t *out_mask, int32_t *index, uint32_t *d2)
{
    OFL_TRY(need_device());
    OFL_TRY(check_fill_args("ofl_fill", vecs, mask, valid, H, W, batch, max_d2, out_vecs, out_mask, index, d2));
    const size_t n = (size_t)batch * H * W, wsb = n * sizeof(int16_t);
    HostStage st("ofl_fill");
    auto dv = st.in(vecs, n * 2);
    auto dm = st.in(mask, n), dva = st.in(valid, n);
    auto ws = st.scratch<char>(wsb);
    auto ov = st.out(out_vecs, n * 2);
    auto om = st.out(out_mask, n);
    auto ix = st.out(index, n);
    auto dd = st.out(d2, n);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_fill_dev(dv, dm, dva, H, W, batch, max_d2, ws, wsb, ov, om, ix, dd, st.stream()));
    return st.download();
}

}  // extern "C"
