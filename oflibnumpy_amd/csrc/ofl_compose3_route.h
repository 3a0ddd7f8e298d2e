// ofl_compose3_route.h -- which kernel ofl_compose3_dev launches for a field shape (plain C++, no HIP: tests compile it on the host).
#pragma once
#include <stdint.h>

namespace ofl {

// The tiled mode-3 kernel addresses every plane of a field pair as a wave-uniform field base plus a 32-bit BYTE offset, so the
// largest plane, the float2 vectors (8 B/px), must stay below 4 GiB.  Larger fields (H * W >= 2^29, e.g. 23200 x 23200) and odd
// widths take the generic per-pixel kernel, which addresses with size_t.
constexpr bool c3_tiled_fits(int H, int W)
{
    return W % 2 == 0 && (uint64_t)H * (uint64_t)W * 8u < (uint64_t(1) << 32);
}

}  // namespace ofl
