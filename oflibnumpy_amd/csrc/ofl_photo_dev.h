// ofl_photo_dev.h -- device helpers that K21 (ofl_photometric.hip) and K22 (ofl_census.hip) share: the frame test of a
// tap, the `covered` rule of a pixel and the per-item counts of a workgroup.
#pragma once
#include "ofl_common.h"

namespace ofl {

// the four in-frame flags and in-plane offsets of a tap (inside one plane: H * W < 2^31)
__device__ __forceinline__ void tap_frame(const Tap &tp, int H, int W, bool (&in)[4], int (&off)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = tp.iy + (k >> 1), xx = tp.ix + (k & 1);
        in[k]  = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        off[k] = in[k] ? yy * W + xx : 0;
    }
}

// K12's `valid` ANDed with near_mask; the masks are those of this pixel's field (near_mask, far_mask may be NULL)
__device__ __forceinline__ bool photo_covered(const uint8_t *fmask, const uint8_t *near_mask, const uint8_t *far_mask,
                                              size_t field, size_t pix, const Tap &tp, const bool (&in)[4], const int (&off)[4])
{
    const uint8_t *fm = far_mask ? far_mask + field : nullptr;
    float m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = in[k] ? ((fm ? fm[off[k]] != 0 : true) ? 1.0f : 0.0f) : 0.0f;
    bool cov = (blend4(m[0], m[1], m[2], m[3], tp) == 1.0f) & (fmask[field + pix] != 0);
    if (near_mask) cov &= near_mask[field + pix] != 0;
    return cov;
}

// the covered and within pixels of this wave (n_cov, n_wi: wave-uniform) -> the block's two counts -> at most one atomicAdd
// per counter; every thread of a block of 4 waves calls this
__device__ __forceinline__ void photo_count(uint32_t *counts, int n, uint32_t n_cov, uint32_t n_wi)
{
    __shared__ uint32_t s_n[4][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { s_n[wave][0] = n_cov; s_n[wave][1] = n_wi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t c0 = s_n[0][0] + s_n[1][0] + s_n[2][0] + s_n[3][0], c1 = s_n[0][1] + s_n[1][1] + s_n[2][1] + s_n[3][1];
        if (c0) atomicAdd(counts + 2 * (size_t)n, c0);
        if (c1) atomicAdd(counts + 2 * (size_t)n + 1, c1);
    }
}

}  // namespace ofl
