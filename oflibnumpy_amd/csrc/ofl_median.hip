// ofl_median.hip -- K16: the mask-aware median filter of flow fields (gfx950); the definition is in include/ofl.h.
// No float operation touches a vector: a float becomes its key, a uint32 whose unsigned order is the order of the floats
// (-0.0 below +0.0, NaNs beyond the infinities by sign and payload), keys are compared and moved, and the chosen key is
// turned back into the four bytes it came from.
//
// median_kernel<K, VALID, ONLY, MASK>, one workgroup of 256 threads per tile of 64 x 16 pixels, lanes along x.  The tile
// plus its halo of K / 2 pixels -- (64 + 2r) x (16 + 2r) -- is staged once in LDS as two planes of keys (u and v apart, so
// that a wave reads 64 consecutive words of one plane: no bank conflict) and one plane of member bytes; a pixel outside
// the frame or outside mask & valid is no member and its keys are 0xFFFFFFFF (a thread asks for the loads of all its halo
// pixels, up to seven, before it keys and stores the first).  The member bytes are summed along x into a
// fourth plane, so that a pixel finds its count n with K reads down its column.  Then every wave takes four rows of the
// tile: a lane reads the K * K keys of one component into registers, sorts them with the network of ofl_median_net.h --
// every index a constant, so there is no scratch -- and picks the rank (n - 1) >> 1 by a chain of selects over the ranks
// 0 .. (K * K - 1) / 2 that can be asked for.  The sentinels sort last; the chosen rank is below n, so a real key that
// equals the sentinel yields the same bytes.  Two wave-uniform short cuts, neither changes a result: a wave none of whose
// pixels is to be filtered (only == 0 throughout, or fewer than min_count members) skips the selection, and a wave whose
// pixels all have a full window takes the fixed rank, for which the compiler keeps a median network only.
// A pixel that is not filtered re-reads its own vector: its key in LDS may have been replaced by the sentinel.
// Which of valid, only and out_mask exist is a template argument (no pointer test in the body): 24 instantiations.
#include <stddef.h>
#include "ofl_common.h"
#include "ofl_host_stage.h"
#include "ofl_median_net.h"

using namespace ofl;

namespace {

constexpr int kThreads = 256, kTileX = 64, kTileY = 16;
// waves per SIMD the register allocator is asked to leave room for (tests/test_median_resources.py): 49 keys are live at K = 7
constexpr int med_waves(int k) { return k == 7 ? 5 : 8; }
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

static_assert(kTileX == 64 && kTileY % (kThreads / 64) == 0, "a wave is one tile row of 64 pixels");

struct MArgs {
    const uint2   *vecs;             // 8 bytes per pixel, moved as two words
    const uint8_t *mask, *valid, *only;
    uint2         *out_vecs;
    uint8_t       *out_mask;
    int            H, W, tiles_x, min_count;
};

__device__ __forceinline__ uint32_t key_of(uint32_t bits) { return bits ^ ((uint32_t)((int32_t)bits >> 31) | 0x80000000u); }
__device__ __forceinline__ uint32_t bits_of(uint32_t key) { return (key >> 31) ? key ^ 0x80000000u : ~key; }

// the key of rank `rank` (FULL: of the middle rank) among the K x K keys at w[dy * PW + dx]
template <int K, int PW, bool FULL>
__device__ __forceinline__ uint32_t select_rank(const uint32_t *w, int rank)
{
    constexpr int N = K * K;
    uint32_t a[N];
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) a[dy * K + dx] = w[dy * PW + dx];
    net_sort<N>(a);
    if (FULL) return a[(N - 1) / 2];
    uint32_t r = a[0];
#pragma unroll
    for (int i = 1; i <= (N - 1) / 2; ++i) r = rank == i ? a[i] : r;
    return r;
}

template <int K, bool VALID, bool ONLY, bool MASK>
__global__ __launch_bounds__(kThreads, med_waves(K))
void median_kernel(const MArgs a)
{
    constexpr int R = K / 2, PW = kTileX + 2 * R, PH = kTileY + 2 * R, PN = PW * PH;
    __shared__ uint32_t ku[PN], kv[PN];
    __shared__ uint8_t  member[PN], row_count[PH * kTileX];
    const int H = a.H, W = a.W, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int x0 = tile_x * kTileX, y0 = tile_y * kTileY;
    const size_t item = (size_t)blockIdx.y * H * (size_t)W;

    // the loads of a thread's kStage halo pixels are asked for together, then keyed and stored
    constexpr int kStage = (PN + kThreads - 1) / kThreads;
    uint2    f[kStage];
    uint32_t m[kStage];
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
        const int i = t + j * kThreads, py = i / PW, px = i - py * PW, y = y0 + py - R, x = x0 + px - R;
        f[j] = make_uint2(0, 0); m[j] = 0;
        if (i < PN && x >= 0 && x < W && y >= 0 && y < H) {
            const size_t q = item + (size_t)y * W + x;
            f[j] = a.vecs[q];
            m[j] = a.mask[q];
            if (VALID) m[j] &= a.valid[q];
        }
    }
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
        const int i = t + j * kThreads;
        if (i < PN) {
            ku[i] = m[j] ? key_of(f[j].x) : kNoKey;
            kv[i] = m[j] ? key_of(f[j].y) : kNoKey;
            member[i] = m[j] ? 1 : 0;
        }
    }
    __syncthreads();
    for (int i = t; i < PH * kTileX; i += kThreads) {
        const uint8_t *m = member + (i >> 6) * PW + (i & 63);
        int s = 0;
#pragma unroll
        for (int dx = 0; dx < K; ++dx) s += m[dx];
        row_count[i] = (uint8_t)s;
    }
    __syncthreads();

    const int x = x0 + lane;
#pragma unroll 1
    for (int ly = wave; ly < kTileY; ly += kThreads / 64) {
        const int y = y0 + ly;
        if (y >= H) break;                                                       // wave-uniform, and no barrier follows
        const bool in = x < W;
        int n = 0;
#pragma unroll
        for (int dy = 0; dy < K; ++dy) n += row_count[(ly + dy) * kTileX + lane];
        const size_t p = item + (size_t)y * W + (in ? x : 0);
        bool target = in;
        if (ONLY && in) target = a.only[p] != 0;
        const bool ok = target && n >= a.min_count;

        uint32_t mu = 0, mv = 0;
        if (__builtin_amdgcn_ballot_w64(ok) != 0) {
            const uint32_t *wu = ku + ly * PW + lane, *wv = kv + ly * PW + lane;
            if (__builtin_amdgcn_ballot_w64(ok && n != K * K) == 0) {
                mu = select_rank<K, PW, true>(wu, 0);
                mv = select_rank<K, PW, true>(wv, 0);
            } else {
                const int rank = (n - 1) >> 1;
                mu = select_rank<K, PW, false>(wu, rank);
                mv = select_rank<K, PW, false>(wv, rank);
            }
        }
        if (in) {
            uint2 o = make_uint2(bits_of(mu), bits_of(mv));
            if (!ok) o = a.vecs[p];
            a.out_vecs[p] = o;
            if (MASK) {
                uint8_t om = ok ? 1 : 0;
                if (ONLY && !target) om = a.mask[p] != 0 ? 1 : 0;
                a.out_mask[p] = om;
            }
        }
    }
}

template <int K, bool VALID, bool ONLY>
void launch_mask(bool mask, const MArgs &a, dim3 grid, hipStream_t s)
{
    if (mask) hipLaunchKernelGGL((median_kernel<K, VALID, ONLY, true>), grid, dim3(kThreads), 0, s, a);
    else      hipLaunchKernelGGL((median_kernel<K, VALID, ONLY, false>), grid, dim3(kThreads), 0, s, a);
}

template <int K>
void launch_k(const MArgs &a, dim3 grid, hipStream_t s)
{
    const bool mask = a.out_mask != nullptr;
    if (a.valid) { if (a.only) launch_mask<K, true, true>(mask, a, grid, s);  else launch_mask<K, true, false>(mask, a, grid, s); }
    else         { if (a.only) launch_mask<K, false, true>(mask, a, grid, s); else launch_mask<K, false, false>(mask, a, grid, s); }
}

int check_median_args(const char *who, const void *vecs, const void *mask, const void *valid, const void *only, int H, int W,
                      int batch, int ksize, int min_count, const void *out_vecs, const void *out_mask)
{
    if (!vecs || !mask || !out_vecs) return fail(OFL_E_INVALID, "%s: NULL pointer (vecs, mask and out_vecs are required)", who);
    if (H < 1 || W < 1 || batch < 1 || batch > 65535)
        return fail(OFL_E_INVALID, "%s: H, W must be positive and batch in [1, 65535] (got %d x %d, %d)", who, H, W, batch);
    const uint64_t tiles = (uint64_t)((W + kTileX - 1) / kTileX) * (uint64_t)((H + kTileY - 1) / kTileY);
    if (tiles > 0x7FFFFFFFull) return fail(OFL_E_INVALID, "%s: a field of %d x %d has more tiles than one launch takes", who, H, W);
    if (ksize != 3 && ksize != 5 && ksize != 7) return fail(OFL_E_INVALID, "%s: ksize must be 3, 5 or 7 (got %d)", who, ksize);
    if (min_count < 1 || min_count > ksize * ksize)
        return fail(OFL_E_INVALID, "%s: min_count must be in [1, %d] for ksize %d (got %d)", who, ksize * ksize, ksize, min_count);
    const size_t n = (size_t)batch * H * W;
    const void *ins[4] = { vecs, mask, valid, only };
    const size_t in_bytes[4] = { n * 8, n, n, n };
    for (int i = 0; i < 4; ++i)
        if (overlap(out_vecs, n * 8, ins[i], in_bytes[i]) || overlap(out_mask, n, ins[i], in_bytes[i]))
            return fail(OFL_E_INVALID, "%s: outputs must not overlap inputs", who);
    if (overlap(out_vecs, n * 8, out_mask, n)) return fail(OFL_E_INVALID, "%s: out_vecs and out_mask overlap", who);
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_median_dev(const float *vecs, const uint8_t *mask, const uint8_t *valid, const uint8_t *only, int H, int W, int batch,
                   int ksize, int min_count, float *out_vecs, uint8_t *out_mask, void *stream)
{
    OFL_TRY(need_device());
    OFL_TRY(check_median_args("ofl_median", vecs, mask, valid, only, H, W, batch, ksize, min_count, out_vecs, out_mask));
    if (!host_aligned(vecs, 8) || !host_aligned(out_vecs, 8))
        return fail(OFL_E_INVALID, "ofl_median: vecs and out_vecs must be 8-byte aligned");
    MArgs a;
    a.vecs = reinterpret_cast<const uint2 *>(vecs); a.mask = mask; a.valid = valid; a.only = only;
    a.out_vecs = reinterpret_cast<uint2 *>(out_vecs); a.out_mask = out_mask;
    a.H = H; a.W = W; a.tiles_x = (W + kTileX - 1) / kTileX; a.min_count = min_count;
    const dim3 grid((unsigned)a.tiles_x * (unsigned)((H + kTileY - 1) / kTileY), (unsigned)batch);
    hipStream_t s = stream_of(stream);
    if (ksize == 3)      launch_k<3>(a, grid, s);
    else if (ksize == 5) launch_k<5>(a, grid, s);
    else                 launch_k<7>(a, grid, s);
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_median(const float *vecs, const uint8_t *mask, const uint8_t *valid, const uint8_t *only, int H, int W, int batch,
               int ksize, int min_count, float *out_vecs, uint8_t *out_mask)
{
    OFL_TRY(need_device());
    OFL_TRY(check_median_args("ofl_median", vecs, mask, valid, only, H, W, batch, ksize, min_count, out_vecs, out_mask));
    const size_t n = (size_t)batch * H * W;
    HostStage st("ofl_median");
    auto dv = st.in(vecs, n * 2);
    auto dm = st.in(mask, n), dva = st.in(valid, n), don = st.in(only, n);
    auto ov = st.out(out_vecs, n * 2);
    auto om = st.out(out_mask, n);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_median_dev(dv, dm, dva, don, H, W, batch, ksize, min_count, ov, om, st.stream()));
    return st.download();
}

}  // extern "C"
