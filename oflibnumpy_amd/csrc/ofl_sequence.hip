// ofl_sequence.hip -- K25: a sequence of fields of one reference accumulated into one field in a single launch (gfx950).
//
// A sequence is L fields of one shape and reference, field k mapping frame k to frame k + 1.  sign = +1 ('s') walks them in
// the order k = 0, 1, ..., L - 1, sign = -1 ('t') in the order k = L - 1, ..., 0.  Per pixel (x, y), with k0 the first field
// of the walk:
//     acc = f_k0[y][x];  m = mask_k0[y][x]
//     for every later k of the walk:
//         tap   = make_tap<quant>(map_coord(x, acc.u, sign), map_coord(y, acc.v, sign))
//         s     = blend4 of f_k's four taps (0 outside the frame);  am = blend4 of mask_k's taps as 0.0f / 1.0f
//         m     = m & (am == 1.0f)
//         acc   = (acc.u + s.u, acc.v + s.v)                                -- one __fadd_rn each
// which is ofl_compose3_dev with fb = acc and fa = f_k, folded over the sequence, bit for bit:
//     's'   F <- F.combine_with(f_k, 3)   for k = 1 ... L - 1
//     't'   G <- f_k.combine_with(G, 3)   for k = L - 2 ... 0
// For 't' this RIGHT fold is the only association that is a per-pixel walk; the left fold (((f_0 (+) f_1) (+) f_2) ...)
// interpolates the accumulated field and is NOT what this kernel computes.  No pixel reads another pixel's accumulated value, so
// the vector stays in two registers over the whole sequence.  There is no zero-flow short cut (as in K13) and no early exit that
// changes a value: a lane whose four taps lie outside the frame skips its loads, the result is the same.  make_tap, map_coord
// and blend4 are ofl_common.h's, so the non-finite rules of include/ofl.h (K1 / K2 / K12 / K13) hold unchanged.
//
// Mapping: consistency_kernel's.  Lanes run along x, a block of 4 waves covers 4 rows x 64 columns, blockIdx = (tile column,
// tile row, sequence): no index division.  Every tap is its own guarded 8-byte load and 1-byte mask load; offsets inside one
// field are int (H * W < 2^31), offsets across fields size_t.  The partial results and lost_at are uniform run-time branches.
// No LDS, no atomics, no workspace.  Each lane makes L - 1 DEPENDENT gathers: occupancy is what hides them.
// Reads 9 B/px per field; writes 9 B/px, + 9 L with the partials, + 4 with lost_at.
#include "ofl_common.h"
#include "ofl_host_stage.h"

#pragma clang fp contract(off)

using namespace ofl;

namespace {

struct SArgs {
    const float   *flows;
    const uint8_t *masks;
    float         *out, *part_vecs;
    uint8_t       *mout, *part_masks;
    int32_t       *lost_at;
    int            H, W, L, sign;
};

template <int QUANT>
__global__ __launch_bounds__(256)
void sequence_kernel(const SArgs a)
{
    const int H = a.H, W = a.W, L = a.L, sign = a.sign;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = blockIdx.y * 4 + wave, x = blockIdx.x * 64 + lane;
    if (y >= H || x >= W) return;
    const size_t hw = (size_t)H * W;
    const int    px = y * W + x;                                       // inside one field: H * W < 2^31
    int k = sign > 0 ? 0 : L - 1;
    size_t field = (size_t)blockIdx.z * L + k;                         // across fields: 64 bits

    const float2 first = *reinterpret_cast<const float2 *>(a.flows + 2 * (field * hw + px));
    float accu = first.x, accv = first.y;
    bool  m = a.masks[field * hw + px] != 0;
    int   lost = m ? -1 : k;
    if (a.part_vecs) {
        *reinterpret_cast<float2 *>(a.part_vecs + 2 * (field * hw + px)) = first;
        a.part_masks[field * hw + px] = m ? 1 : 0;
    }
    for (int i = 1; i < L; ++i) {
        k += sign;
        field = sign > 0 ? field + 1 : field - 1;
        const float   *__restrict__ f  = a.flows + 2 * field * hw;
        const uint8_t *__restrict__ fm = a.masks + field * hw;
        const Tap tp = make_tap<QUANT>(map_coord(x, accu, sign), map_coord(y, accv, sign));
        float u[4], v[4], w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = tp.iy + (j >> 1), xx = tp.ix + (j & 1);
            const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            const int s = in ? yy * W + xx : 0;
            const float2 t = in ? *reinterpret_cast<const float2 *>(f + 2 * (size_t)s) : make_float2(0.0f, 0.0f);
            u[j] = t.x;
            v[j] = t.y;
            w[j] = (in && fm[s] != 0) ? 1.0f : 0.0f;
        }
        const float su = blend4(u[0], u[1], u[2], u[3], tp), sv = blend4(v[0], v[1], v[2], v[3], tp);
        m = m & (blend4(w[0], w[1], w[2], w[3], tp) == 1.0f);
        accu = __fadd_rn(accu, su);
        accv = __fadd_rn(accv, sv);
        if (!m && lost < 0) lost = k;
        if (a.part_vecs) {
            *reinterpret_cast<float2 *>(a.part_vecs + 2 * (field * hw + px)) = make_float2(accu, accv);
            a.part_masks[field * hw + px] = m ? 1 : 0;
        }
    }
    const size_t at = (size_t)blockIdx.z * hw + px;
    *reinterpret_cast<float2 *>(a.out + 2 * at) = make_float2(accu, accv);
    a.mout[at] = m ? 1 : 0;
    if (a.lost_at) a.lost_at[at] = lost;
}

int check_sequence_args(const char *who, const void *flows, const void *masks, int sign, int H, int W, int L, int S,
                        const void *out, const void *mout, const void *part_vecs, const void *part_masks, const void *lost_at, int quant)
{
    if (!flows || !masks || !out || !mout) return fail(OFL_E_INVALID, "%s: NULL pointer (flows, masks, out and mout are required)", who);
    // the taps are int16 inside cv2.remap, as for ofl_compose3
    OFL_TRY(check_field_dims(who, H, W));
    if (L < 1) return fail(OFL_E_INVALID, "%s: L must be at least 1, got %d", who, L);
    if (S < 1 || S > 65535) return fail(OFL_E_INVALID, "%s: S must be in [1, 65535], got %d", who, S);
    if (sign != 1 && sign != -1) return fail(OFL_E_INVALID, "%s: sign must be +1 or -1", who);
    if (quant != OFL_QUANT_OPENCV && quant != OFL_QUANT_EXACT) return fail(OFL_E_INVALID, "%s: bad quant", who);
    if ((part_vecs == nullptr) != (part_masks == nullptr))
        return fail(OFL_E_INVALID, "%s: part_vecs and part_masks must be given together or not at all", who);
    const size_t px = (size_t)S * H * W, all = px * L;
    const void *ins[2] = { flows, masks };
    const size_t in_bytes[2] = { all * 8, all };
    const void *outs[5] = { out, mout, part_vecs, part_masks, lost_at };
    const size_t out_bytes[5] = { px * 8, px, all * 8, all, px * 4 };
    for (int i = 0; i < 5; ++i) {
        for (int j = 0; j < 2; ++j)
            if (overlap(outs[i], out_bytes[i], ins[j], in_bytes[j])) return fail(OFL_E_INVALID, "%s: outputs must not overlap inputs", who);
        for (int j = i + 1; j < 5; ++j)
            if (overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return fail(OFL_E_INVALID, "%s: the outputs overlap each other", who);
    }
    return OFL_OK;
}

}  // namespace

extern "C" {

int ofl_compose_sequence_dev(const float *flows, const uint8_t *masks, int sign, int H, int W, int L, int S,
                             float *out, uint8_t *mout, float *part_vecs, uint8_t *part_masks, int32_t *lost_at,
                             int quant, void *stream)
{
    const char *who = "ofl_compose_sequence";
    OFL_TRY(need_device());
    OFL_TRY(check_sequence_args(who, flows, masks, sign, H, W, L, S, out, mout, part_vecs, part_masks, lost_at, quant));
    if (!host_aligned(flows, 8) || !host_aligned(out, 8) || !host_aligned(part_vecs, 8))
        return fail(OFL_E_INVALID, "%s: flows, out and part_vecs must be 8-byte aligned", who);
    if (!host_aligned(lost_at, 4)) return fail(OFL_E_INVALID, "%s: lost_at must be 4-byte aligned", who);
    const SArgs a = { flows, masks, out, part_vecs, mout, part_masks, lost_at, H, W, L, sign };
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)S);
    hipStream_t s = stream_of(stream);
    with_quant(quant, [&](auto Q) { hipLaunchKernelGGL((sequence_kernel<Q.value>), grid, dim3(256), 0, s, a); });
    OFL_HIP(hipGetLastError());
    return OFL_OK;
}

int ofl_compose_sequence(const float *flows, const uint8_t *masks, int sign, int H, int W, int L, int S,
                         float *out, uint8_t *mout, float *part_vecs, uint8_t *part_masks, int32_t *lost_at, int quant)
{
    const char *who = "ofl_compose_sequence";
    OFL_TRY(need_device());
    OFL_TRY(check_sequence_args(who, flows, masks, sign, H, W, L, S, out, mout, part_vecs, part_masks, lost_at, quant));
    const size_t px = (size_t)S * H * W, all = px * L;
    HostStage st(who);
    auto df = st.in(flows, all * 2);
    auto dm = st.in(masks, all);
    auto dout = st.out(out, px * 2);
    auto dmout = st.out(mout, px);
    auto dpv = st.out(part_vecs, all * 2);
    auto dpm = st.out(part_masks, all);
    auto dlost = st.out(lost_at, px);
    OFL_TRY(st.upload());
    OFL_TRY(ofl_compose_sequence_dev(df, dm, sign, H, W, L, S, dout, dmout, dpv, dpm, dlost, quant, st.stream()));
    return st.download();
}

}  // extern "C"
