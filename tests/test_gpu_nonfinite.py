"""GPU suite: flow vectors with NaN, Inf and out-of-int32 components through the kernels that turn a vector into an address --
K2 (ofl_compose3_dev, ofl_compose3_bits_dev), K1 (ofl_gather_bilinear_dev, _batch_dev, ofl_gather_rows_dev), K12
(ofl_gather_tensor_dev) and K13 (ofl_consistency_dev) -- against the oracle on the cases of tests/nonfinite_cases.py, whose
docstring argues kernel by kernel why these inputs cannot leave a kernel's own memory.

Masks, validity, covered, consistent and the counts are byte-equal to the reference; float outputs have NaN where the
reference has NaN (x86 and the GPU may hand on different payloads) and identical bytes everywhere else, +-Inf and -0.0
included.  Every output sits between 0xA5 guard bytes (tests/devmem.py) and every input is read back unchanged."""
import functools

import numpy as np
import pytest

import consistency_ref as C
import devmem as D
import gather_cases as G
import gather_census as gc
import nonfinite_cases as N
import tensor_ref as T
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64
QUANTS = [O.QUANT_OPENCV, O.QUANT_EXACT]
SIGNS = [-1, 1]
FIELDS = [(s, k) for s in N.SHAPES for k in N.KINDS]
IDS = ["{}x{}x{}-{}".format(*s, k) for s, k in FIELDS]


class Inputs:
    """uploaded inputs of one case; unchanged() reads every one back"""

    def __init__(self, **arrays):
        self.host = {k: np.ascontiguousarray(a) for k, a in arrays.items() if a is not None}
        self.bufs = {k: D.place(a) for k, a in self.host.items()}

    def ptr(self, name):
        return self.bufs[name][1] if name in self.bufs else None

    def buf(self, name):
        return self.bufs[name][0]

    def unchanged(self, tag):
        for k, a in self.host.items():
            got = self.bufs[k][0].to_host((a.nbytes,), np.uint8)
            assert np.array_equal(got, a.reshape(-1).view(np.uint8)), ("input changed", k, tag)


def out_buf(want):
    return D.guarded(want.nbytes, GUARD)


def read(buf, want):
    return D.read_guarded(buf, 0, want.nbytes, GUARD, want.dtype, want.shape)


def check_floats(buf, want, tag):
    assert N.same_floats(read(buf, want), want), tag


def check_bytes(buf, want, tag):
    np.testing.assert_array_equal(read(buf, want), want, err_msg=str(tag))


# ================================================================================================ K2
@functools.lru_cache(maxsize=None)
def want_compose(shape, kind, placement, sign, quant):
    c = N.case(shape, kind, placement, sign)
    res = [O.compose3_raw(c['fa'][b], c['ma'][b], c['fb'][b], c['mb'][b], sign, quant) for b in range(shape[0])]
    out, m = np.stack([r[0] for r in res]), np.stack([r[1] for r in res]).astype(np.uint8)
    out.flags.writeable = m.flags.writeable = False
    return out, m


def check_flag_words(words, fa, ma, fb, mb, tag):
    """test_gpu_compose3_paths._run's reading of the flag words: 4..7 exact on fb; on fa the tiled kernel (even W) sets 0/1 as
    certificates and leaves 2/3 alone, the generic kernel (odd W) sets all four exactly"""
    tiled = fb.shape[2] % 2 == 0
    for b in range(fb.shape[0]):
        w = [bool(x) for x in words[b]]
        exact_b = [not O.is_zero_raw(fb[b], mb[b], False), not O.is_zero_raw(fb[b], mb[b], True),
                   not O.is_zero_raw(fb[b], None, False), not O.is_zero_raw(fb[b], None, True)]
        exact_a = [not O.is_zero_raw(fa[b], ma[b], False), not O.is_zero_raw(fa[b], ma[b], True),
                   not O.is_zero_raw(fa[b], None, False), not O.is_zero_raw(fa[b], None, True)]
        assert w[4:8] == exact_b, (tag, b, words[b])
        if tiled:
            assert not w[2] and not w[3], (tag, b, words[b])
            assert (not w[0] or exact_a[0]) and (not w[1] or exact_a[1]), (tag, b, words[b])
        else:
            assert w[0:4] == exact_a, (tag, b, words[b])


def run_compose(gpu, fa, ma, fb, mb, sign, want, tag, quants=QUANTS, bits=True):
    """ofl_compose3_dev with and without the flag words in every quantisation of `quants`, ofl_compose3_bits_dev on even widths;
    want(quant) -> (out, mask)"""
    from oflibnumpy_amd import device as dev
    nat, lib = gpu.native, gpu.native.load()
    B, H, W = fb.shape[:3]
    ins = Inputs(fa=fa, ma=ma, fb=fb, mb=mb)
    for quant in quants:
        w_out, w_m = want(quant)
        for stats_on in (True, False):
            out, mout = out_buf(w_out), out_buf(w_m)
            stats = dev.DeviceBuffer.zeros(B * 8 * 4) if stats_on else None
            nat.check(lib.ofl_compose3_dev(ins.ptr('fa'), ins.ptr('ma'), ins.ptr('fb'), ins.ptr('mb'), sign, H, W, B, out.ptr, mout.ptr,
                                           stats.ptr if stats_on else None, quant, None))
            t = (tag, 'quant', quant, 'stats', stats_on)
            check_bytes(mout, w_m, t)
            check_floats(out, w_out, t)
            if stats_on:
                check_flag_words(stats.to_host((B, 8), np.uint32), fa, ma, fb, mb, t)
    if bits and W % 2 == 0 and O.QUANT_OPENCV in quants:
        w_out, w_m = want(O.QUANT_OPENCV)
        ba, bb = dev.mask_pack(ins.buf('ma'), H, W, B), dev.mask_pack(ins.buf('mb'), H, W, B)
        out, bo, stats = out_buf(w_out), dev.DeviceBuffer.zeros(dev.mask_bits_bytes(H, W, B)), dev.DeviceBuffer.zeros(B * 8 * 4)
        dev.compose3_bits_launch(ins.buf('fa'), ba, ins.buf('fb'), bb, sign, (H, W), out, bo, stats, batch=B)
        np.testing.assert_array_equal(dev.mask_unpack(bo, H, W, B).to_host((B, H, W), np.uint8), w_m, err_msg=str((tag, 'bits')))
        check_floats(out, w_out, (tag, 'bits'))
        check_flag_words(stats.to_host((B, 8), np.uint32), fa, ma, fb, mb, (tag, 'bits'))
    ins.unchanged(tag)


@pytest.mark.parametrize("shape,kind", FIELDS, ids=IDS)
def test_compose3(gpu, shape, kind):
    for placement in N.PLACEMENTS:
        for sign in SIGNS:
            c = N.case(shape, kind, placement, sign)
            run_compose(gpu, c['fa'], c['ma'], c['fb'], c['mb'], sign,
                        lambda quant: want_compose(shape, kind, placement, sign, quant), (shape, kind, placement, sign))


# ================================================================================================ K1
F32_EQ, F32_EXACT = ('eq', 0, 0, G.EQ1), ('exact_eq', 1, 0, G.EQ1)
U8_FIX, U8_RNE = ('fix_ge', 0, 0, G.GE_HALF), ('rne_gt', 0, 1, G.GT_HALF)


def gather_variants(shape):
    """(entry, dtype, C, image shape, placement of the flow, mode, (source mask, flow mask, validity), extra) over one field
    [B, H, W, 2]: paired and generic kernels by the image's width and channel count"""
    B, H, W = shape
    v = [('single', gc.F32, 2, (H, W), 'frame', F32_EQ, (True, True, True), {}),
         ('single', gc.F32, 2, (H, W), 'frame', F32_EXACT, (True, True, True), {}),
         ('single', gc.F32, 1, (H, W), 'frame', F32_EQ, (False, False, True), {}),
         ('single', gc.F32, 3, (H, W), 'frame', F32_EXACT, (False, True, True), {}),
         ('single', gc.F32, 6, (H, W), 'frame', F32_EQ, (True, True, True), {}),            # six channels: the generic kernel
         ('single', gc.U8, 3, (H, W), 'frame', U8_FIX, (True, False, True), {}),
         ('single', gc.U8, 1, (H, W), 'frame', U8_RNE, (False, True, True), {}),
         ('single', gc.U8, 4, (H, W), 'frame', U8_FIX, (False, False, False), {}),
         # a flow smaller than the image: even offsets (16-byte aligned pairs when W is even), odd offsets and an odd / even image
         ('single', gc.F32, 2, (H + 5, W + 4), 'even', F32_EQ, (True, True, True), {}),
         ('single', gc.U8, 3, (H + 5, W + 5), 'odd', U8_FIX, (True, True, True), {}),
         ('single', gc.F32, 1, (H + 5, W + 5), 'odd', F32_EXACT, (False, True, True), {}),
         ('batch', gc.F32, 2, (H, W), 'frame', F32_EQ, (True, True, True), dict(batch=B, shared=False)),
         ('batch', gc.U8, 3, (H, W), 'frame', U8_FIX, (True, True, True), dict(batch=B, shared=True))]
    if H >= 11:                                  # a band that starts inside a tile and ends inside the next
        for dtype, C, mode in ((gc.F32, 2, F32_EQ), (gc.U8, 1, U8_RNE)):
            v.append(('rows', dtype, C, (H, W), 'frame', mode, (True, True, True), dict(row0=5, rows=6, pad_top=5, fH=6)))
    return v


def gather_arrays(c, case, rng):
    """the arrays of G.build's layout for one variant: the case's bad field as the flow, its fa as a float image of two channels"""
    H, W, C, B = c['H'], c['W'], c['C'], c['batch']
    nsrc = 1 if c['shared'] else B
    first = 0 if c['entry'] == 'batch' else 1 % case['fb'].shape[0]               # single launches: the second field, if there is one
    r0 = c['row0'] if c['entry'] == 'rows' else 0                                  # a row band brings the band's rows of the field
    flow = case['fb'][first:first + B, r0:r0 + c['fH']]
    fmask = case['mb'][first:first + B, r0:r0 + c['fH']] if c['fmask'] else None
    if c['dtype'] == gc.F32 and C == 2 and (H, W) == case['fb'].shape[1:3]:
        src = case['fa'][first:first + nsrc]
    elif c['dtype'] == gc.F32:
        src = (rng.standard_normal((nsrc, H, W, C)) * 100).astype(np.float32)
    else:
        src = rng.integers(0, 255, (nsrc, H, W, C), endpoint=True).astype(np.uint8)
    smask = (rng.random((nsrc, H, W)) > 0.15).astype(np.uint8) if c['smask'] else None
    return dict(src=np.ascontiguousarray(src), flow=np.ascontiguousarray(flow), smask=smask,
                fmask=None if fmask is None else np.ascontiguousarray(fmask))


@pytest.mark.parametrize("shape,kind", FIELDS, ids=IDS)
def test_gather(gpu, oracle, shape, kind):
    nat, lib = gpu.native, gpu.native.load()
    codes = {gc.U8: nat.U8, gc.F32: nat.F32}
    rng = np.random.default_rng(11)
    for placement in N.PLACEMENTS:
        for k, (entry, dtype, C, image, place, mode, masks, extra) in enumerate(gather_variants(shape)):
            sign = SIGNS[k % 2]
            case = N.case(shape, kind, placement, sign)
            c = G._case(entry, dtype, C, image, kind, place, mode, sign, masks, **extra)
            assert (c['fH'], c['fW']) == (extra.get('fH', shape[1]), shape[2])
            a = gather_arrays(c, case, rng)
            want_img, want_val = G.expected(c, a, oracle)
            tag = (c['id'], placement)
            ins = Inputs(**a)
            dst = out_buf(want_img)
            valid = out_buf(want_val) if c['valid'] else None
            vp = valid.ptr if c['valid'] else None
            if entry == 'single':
                nat.check(lib.ofl_gather_bilinear_dev(ins.ptr('src'), codes[dtype], C, c['H'], c['W'], ins.ptr('flow'), c['fH'], c['fW'],
                                                      c['pad_top'], c['pad_left'], sign, ins.ptr('smask'), ins.ptr('fmask'), dst.ptr, vp,
                                                      c['quant'], c['arith'], c['rule'], None))
            elif entry == 'rows':
                nat.check(lib.ofl_gather_rows_dev(ins.ptr('src'), codes[dtype], C, c['H'], c['W'], c['row0'], c['rows'], ins.ptr('flow'), sign,
                                                  ins.ptr('smask'), ins.ptr('fmask'), dst.ptr, vp, c['quant'], c['arith'], c['rule'], None))
            else:
                nat.check(lib.ofl_gather_bilinear_batch_dev(ins.ptr('src'), int(c['shared']), codes[dtype], C, c['H'], c['W'], c['batch'],
                                                            ins.ptr('flow'), c['fH'], c['fW'], c['pad_top'], c['pad_left'], sign,
                                                            ins.ptr('smask'), int(c['shared']), ins.ptr('fmask'), dst.ptr, vp,
                                                            c['quant'], c['arith'], c['rule'], None))
            if dtype == gc.F32:
                check_floats(dst, want_img, tag)
            else:
                check_bytes(dst, want_img, tag)
            if c['valid']:
                check_bytes(valid, want_val, tag)
            ins.unchanged(tag)


# ================================================================================================ K12
def run_tensor(gpu, src, dtype, layout, vecs, fmask, tmask, quant, tag):
    """ofl_gather_tensor_dev on a planar host tensor `src` [N, C, H, W] against tensor_ref.warp; vecs / fmask shared ([H, W, ..])
    or per item ([N, H, W, ..]); tmask [H, W] (shared) or None"""
    nat, lib = gpu.native, gpu.native.load()
    n, ch, h, w = src.shape
    mem = src if layout == 'chw' else np.ascontiguousarray(np.moveaxis(src, 1, -1))
    with np.errstate(invalid='ignore', over='ignore'):
        want, want_valid = T.warp(mem, dtype, layout, vecs, fmask, tmask, quant)
    want_valid = np.ascontiguousarray(want_valid).astype(np.uint8)
    shared = vecs.ndim == 3
    ins = Inputs(src=mem, flow=vecs, fmask=np.ascontiguousarray(fmask).astype(np.uint8), smask=None if tmask is None else tmask.astype(np.uint8))
    dst, valid = out_buf(want), out_buf(want_valid)
    nat.check(lib.ofl_gather_tensor_dev(ins.ptr('src'), {'float32': nat.EL_F32, 'float16': nat.EL_F16}[dtype],
                                        {'chw': nat.TENSOR_NCHW, 'hwc': nat.TENSOR_NHWC}[layout], n, ch, h, w, ins.ptr('flow'), int(shared), -1,
                                        ins.ptr('smask'), 1, ins.ptr('fmask'), dst.ptr, valid.ptr, quant, None))
    check_bytes(valid, want_valid, tag)
    check_floats(dst, want, tag)
    ins.unchanged(tag)


@pytest.mark.parametrize("shape,kind", FIELDS, ids=IDS)
def test_tensor(gpu, shape, kind):
    B, H, W = shape
    combos = [(d, l, sh) for d in ('float32', 'float16') for l in T.LAYOUTS for sh in (True, False)]
    for pi, placement in enumerate(N.PLACEMENTS):
        c = N.case(shape, kind, placement, -1)                     # reference 't'
        for i, (dtype, layout, shared) in enumerate(combos):
            # every (type, layout, shared) meets both quantisations over the two placements, a target mask every other time
            quant = QUANTS[(i // 4 + i + pi) % 2]
            tmask = c['ma'][0] if (i ^ (i >> 1)) & 1 else None
            src = T.values((2 if shared else B, 3, H, W), dtype, seed=i)
            vecs, fmask = (c['fb'][0], c['mb'][0]) if shared else (c['fb'], c['mb'])
            run_tensor(gpu, src, dtype, layout, vecs, fmask, tmask, quant, (shape, kind, placement, dtype, layout, shared, quant))


# ================================================================================================ K13
def run_consistency(gpu, f, fm, b, bm, sign, quant, tag):
    """ofl_consistency_dev on the stacked pairs [B, H, W, ..]: with counts, covered and residual, and bare"""
    from oflibnumpy_amd import device as dev
    nat, lib = gpu.native, gpu.native.load()
    B, H, W = f.shape[:3]
    with np.errstate(invalid='ignore', over='ignore'):
        want = [C.consistency(f[i], fm[i], b[i], bm[i], sign, quant=quant) for i in range(B)]
    con, cov = (np.stack([w[j] for w in want]).astype(np.uint8) for j in (0, 1))
    res = np.stack([w[2] for w in want])
    cnt = np.array([w[3] for w in want], np.uint32)
    ins = Inputs(f=f, fm=fm, b=b, bm=bm)
    for full in (True, False):
        d_con = out_buf(con)
        d_cov, d_res = (out_buf(cov), out_buf(res)) if full else (None, None)
        d_cnt = dev.DeviceBuffer.zeros(B * 8) if full else None
        nat.check(lib.ofl_consistency_dev(ins.ptr('f'), ins.ptr('fm'), ins.ptr('b'), ins.ptr('bm'), sign, H, W, B, np.float32(C.ALPHA),
                                          np.float32(C.BETA), d_con.ptr, d_cov.ptr if full else None, d_res.ptr if full else None,
                                          d_cnt.ptr if full else None, quant, None))
        check_bytes(d_con, con, (tag, full))
        if full:
            check_bytes(d_cov, cov, tag)
            check_floats(d_res, res, tag)
            np.testing.assert_array_equal(d_cnt.to_host((B, 2), np.uint32), cnt, err_msg=str(tag))
    ins.unchanged(tag)


@pytest.mark.parametrize("shape,kind", FIELDS, ids=IDS)
def test_consistency(gpu, shape, kind):
    for placement in N.PLACEMENTS:
        for sign in SIGNS:
            c = N.case(shape, kind, placement, sign)
            for quant in QUANTS:
                run_consistency(gpu, c['fb'], c['mb'], c['fa'], c['ma'], sign, quant, (shape, kind, placement, sign, quant))


# ================================================================================================ NaN / Inf in the SAMPLED data
def test_a_tap_of_weight_zero_carries_its_nan(gpu, oracle):
    """finite flows over fa / an image / b with NaN and Inf in them: a tap of weight 0 still multiplies (0 * NaN, 0 * Inf), in
    every kernel and on every path, exactly as in the oracle"""
    nat, lib = gpu.native, gpu.native.load()
    fa, ma, fb, mb = N.poisoned_source()
    B, H, W = fb.shape[:3]

    def want(quant):
        r = [O.compose3_raw(fa[b], ma[b], fb[b], mb[b], -1, quant) for b in range(B)]
        return np.stack([x[0] for x in r]), np.stack([x[1] for x in r]).astype(np.uint8)
    assert not np.isfinite(want(O.QUANT_OPENCV)[0]).all()
    run_compose(gpu, fa, ma, fb, mb, -1, want, 'poisoned fa')
    for quant in QUANTS:
        run_consistency(gpu, fb, mb, fa, ma, -1, quant, ('poisoned b', quant))
        # K1, paired and (one column more) generic: the two-channel float image fa
        for pad in (0, 1):
            img = np.ascontiguousarray(np.pad(fa[0], ((0, 0), (0, pad), (0, 0))))
            flow = np.ascontiguousarray(np.pad(fb[0], ((0, 0), (0, pad), (0, 0))))
            w_img, w_val = oracle.gather_bilinear(img, flow, -1, want_valid=True, quant=quant)
            ins = Inputs(src=img, flow=flow)
            dst, val = out_buf(w_img), out_buf(w_val.astype(np.uint8))
            nat.check(lib.ofl_gather_bilinear_dev(ins.ptr('src'), nat.F32, 2, H, W + pad, ins.ptr('flow'), H, W + pad, 0, 0, -1, None, None,
                                                  dst.ptr, val.ptr, quant, nat.ARITH_NATIVE, nat.RULE_EQ1, None))
            check_floats(dst, w_img, ('poisoned image', quant, pad))
            check_bytes(val, w_val.astype(np.uint8), ('poisoned image', quant, pad))
            ins.unchanged(('poisoned image', quant, pad))
        # K12: the same image as a float32 tensor of two channels, both layouts
        src = np.ascontiguousarray(np.moveaxis(fa, -1, 1))
        for layout in T.LAYOUTS:
            run_tensor(gpu, src, 'float32', layout, fb, mb, None, quant, ('poisoned tensor', layout, quant))
