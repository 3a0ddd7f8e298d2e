// ofl_pairs.h -- shared by the kernels that fetch the two horizontally adjacent taps of a row with ONE load and read masks from
// unaligned addresses: K1 (ofl_gather.hip), K2 (ofl_compose3.hip), K4 (ofl_resize.hip) and the scatter walk (ofl_scatter_walk.hip).
#pragma once
#include <stdint.h>

namespace ofl {

typedef float v4f __attribute__((ext_vector_type(4)));
struct __attribute__((aligned(8))) Pair2 { float lo_u, lo_v, hi_u, hi_v; };   // taps (ix, ix+1) of a float2 field: ONE 16-byte load
struct __attribute__((packed, aligned(1))) U32u { uint32_t v; };               // a 4-byte load from any address
struct __attribute__((packed, aligned(1))) U16u { uint16_t v; };               // a 2-byte load from any address

// the transposed-gather form of K2 and of K1's float images (rotated sampling grids, ofl_compose3.hip)
constexpr int kXpRowF2 = 128 + 4;             // LDS row stride in float2 (padding spreads the 8 rows over the banks)
constexpr int kXposeRows = 6;                 // source rows one streamed 128-px segment may cross before we transpose

}  // namespace ofl
