"""K24 (ofl_inverse_search.hip): the dense inverse search of a field on the device, bit for bit against
tests/inverse_search_ref.py (the oracle's gather plus float32 NumPy in the stated order), and through every layer: the raw
ABI, DeviceFlow.inverse_search, DeviceFlowBatch.inverse_search, Flow.inverse_search and inverse_search_flow; then
DeviceTensor.halve and estimate_flow.  Nothing here has a tolerance: vectors and patch_ssd are compared through their bits,
masks with array_equal.  (8, 8) is one patch of 8, (8, 21) one row of patches with an added last origin, (19, 70) and
(37, 131) have added origins on both axes and patch counts that fill the last wave of a P = 4 launch only in part,
(64, 256) with two items is an exact grid."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import interop_ref as R
import inverse_search_ref as I
import nonfinite_cases as NF
import tensor_ref as T

pytestmark = pytest.mark.gpu
nat = of.native
F32, U8 = np.float32, np.uint8
EL = {'float32': nat.EL_F32, 'float16': nat.EL_F16, 'bfloat16': nat.EL_BF16}
LAYOUT = {'chw': nat.TENSOR_NCHW, 'hwc': nat.TENSOR_NHWC}
bits = I.bits


def up(a):
    a = np.ascontiguousarray(a)
    return dev.DeviceBuffer.from_host(a.view(U8) if a.dtype == np.bool_ else a)


def ptr(x):
    return None if x is None else x.ptr


def raw_call(near, far, dtype, layout, f, fm, sign, quant=nat.QUANT_EXACT, patches=True, **kw):
    """ofl_inverse_search_dev on host arrays: near, far planar (n, c, h, w) as stored in `dtype`, uploaded in the memory order
    of `layout`; f (n, h, w, 2) or None, fm (n, h, w) or None -> dict(vecs, mask, patch_vecs, patch_ssd) on the host (the two
    last None without `patches`: the records then live in the workspace)"""
    n, c, h, w = near.shape
    p = dict(I.DEFAULTS, **kw)
    ny, nx = len(I.origins(h, p['patch'], p['stride'])), len(I.origins(w, p['patch'], p['stride']))
    px, npatch = n * h * w, n * ny * nx
    d_near, d_far = up(I.in_layout(near, layout)), up(I.in_layout(far, layout))
    d_f = None if f is None else up(np.ascontiguousarray(f, F32))
    d_fm = None if fm is None else up(fm)
    ws = 8 * px + (0 if patches else 12 * npatch)
    work, d_out, d_mask = dev.DeviceBuffer(ws), dev.DeviceBuffer(px * 8), dev.DeviceBuffer(px)
    d_pv, d_ps = (dev.DeviceBuffer(npatch * 8), dev.DeviceBuffer(npatch * 4)) if patches else (None, None)
    nat.check(nat.load().ofl_inverse_search_dev(d_near.ptr, d_far.ptr, EL[dtype], LAYOUT[layout], n, c, h, w, ptr(d_f), ptr(d_fm), sign,
                                                p['patch'], p['stride'], p['iterations'], 1 if p['normalise'] else 0, F32(p['floor']),
                                                work.ptr, ws, d_out.ptr, d_mask.ptr, ptr(d_pv), ptr(d_ps), quant, None))
    return dict(vecs=d_out.to_host((n, h, w, 2), F32), mask=d_mask.to_host((n, h, w), U8),
                patch_vecs=d_pv.to_host((n, ny, nx, 2), F32) if patches else None,
                patch_ssd=d_ps.to_host((n, ny, nx), F32) if patches else None)


def check(got, want, what):
    for key in ('patch_vecs', 'patch_ssd', 'vecs'):
        if got[key] is not None:
            assert got[key].shape == want[key].shape, (what, key)
            assert np.array_equal(bits(got[key]), bits(want[key])), "{}: {}, {} of {} words differ".format(
                what, key, int((bits(got[key]) != bits(want[key])).sum()), got[key].size)
    np.testing.assert_array_equal(got['mask'], want['mask'].astype(U8), err_msg="{}: mask".format(what))


def run_case(shape, sign, quant, layout, dtype, c, n=1, seed=1, init=True, **kw):
    k = I.case(seed, shape, sign, quant, c, dtype, n, init, tuple(sorted(kw.items())))
    got = raw_call(k['near'], k['far'], dtype, layout, k['f'], k['fm'], sign, quant, **kw)
    check(got, k['want'], (shape, sign, quant, layout, dtype, c, n, init, kw))
    return got, k


# ---------------------------------------------------------------------------------------------- 1: the rotation
DIMS = [('patch', (4, 8)), ('stride', (1, 3, 4, 'P')), ('dtype', tuple(T.DTYPES)), ('layout', tuple(T.LAYOUTS)), ('c', (1, 2, 3, 4)),
        ('sign', tuple(I.SIGNS)), ('quant', tuple(I.QUANTS)), ('normalise', (True, False)), ('iterations', (1, 3, 12))]


def rotation():
    """settings such that each value of each of the nine dimensions meets each value of each other dimension at least once:
    a greedy pairwise cover over a fixed enumeration, so the list is the same in every run"""
    names = [d[0] for d in DIMS]
    every = list(itertools.product(*(d[1] for d in DIMS)))
    pairs = lambda row: {(i, row[i], j, row[j]) for i in range(len(row)) for j in range(i + 1, len(row))}
    todo = set().union(*(pairs(r) for r in every))
    rng, out = np.random.default_rng(24), []
    while todo:
        pick = [every[i] for i in rng.choice(len(every), 200, replace=False)]
        best = max(pick, key=lambda r: len(pairs(r) & todo))
        if not pairs(best) & todo:
            best = max(every, key=lambda r: len(pairs(r) & todo))
        todo -= pairs(best)
        out.append(dict(zip(names, best)))
    return out


ROTATION = rotation()


def test_the_rotation_reaches_every_pair_of_settings():
    assert len(ROTATION) <= 40
    for (a, va), (b, vb) in itertools.combinations(DIMS, 2):
        seen = {(r[a], r[b]) for r in ROTATION}
        assert seen == set(itertools.product(va, vb)), (a, b)


@pytest.mark.parametrize("i", range(len(ROTATION)))
def test_every_pair_of_settings(gpu, i):
    r = ROTATION[i]
    stride = r['patch'] if r['stride'] == 'P' else r['stride']
    run_case((19, 70), r['sign'], r['quant'], r['layout'], r['dtype'], r['c'], seed=i, patch=r['patch'], stride=stride,
             normalise=r['normalise'], iterations=r['iterations'])


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_planar_and_channels_last_give_identical_bytes(gpu, dtype):
    for c in (1, 3, 4):
        a, _ = run_case((19, 70), -1, nat.QUANT_EXACT, 'chw', dtype, c, iterations=3)
        b, _ = run_case((19, 70), -1, nat.QUANT_EXACT, 'hwc', dtype, c, iterations=3)
        assert all(a[key].tobytes() == b[key].tobytes() for key in a)


# ---------------------------------------------------------------------------------------------- 2: shapes
# at every shape both patch sizes, signs, quant, layouts, every dtype, an init with holes and no init occur at least once
THIN = [(1, nat.QUANT_EXACT, 'chw', 'float32', 3, True, dict()),
        (-1, nat.QUANT_OPENCV, 'hwc', 'float16', 1, False, dict(patch=4, stride=3, iterations=3)),
        (1, nat.QUANT_OPENCV, 'chw', 'bfloat16', 4, True, dict(patch=8, stride=8, normalise=False)),
        (-1, nat.QUANT_EXACT, 'hwc', 'float32', 2, False, dict(patch=4, stride=1, iterations=5, floor=0.25))]


@pytest.mark.parametrize("shape, n", [((8, 8), 1), ((8, 21), 1), ((19, 70), 1), ((37, 131), 1), ((64, 256), 2)],
                         ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else "n{}".format(s))
def test_shapes(gpu, shape, n):
    for sign, quant, layout, dtype, c, init, kw in THIN:
        (got, k) = run_case(shape, sign, quant, layout, dtype, c, n=n, init=init, **kw)
        if shape == (8, 8) and kw.get('patch', 8) == 8:
            assert got['patch_vecs'].shape == (1, 1, 1, 2)                # one patch, one wave
    if n > 1:
        assert got['vecs'][0].tobytes() != got['vecs'][1].tobytes()


def test_the_search_moves_most_patches_and_none_farther_than_its_size(gpu):
    for patch, stride in ((8, 4), (4, 2)):
        got, k = run_case((37, 131), 1, nat.QUANT_EXACT, 'chw', 'float32', 3, seed=3, patch=patch, stride=stride)
        d = got['patch_vecs'].astype(np.float64) - k['want']['u0']
        assert ((d * d).sum(axis=-1) <= patch * patch).all() and (k['want']['kbest'] > 0).mean() > 0.5
        assert got['mask'].all()


# ---------------------------------------------------------------------------------------------- 3: non-finite values, flat images
def test_non_finite_image_values(gpu):
    shape, sign, c = (19, 70), 1, 3
    k = I.case(7, shape, sign, nat.QUANT_EXACT, c)
    near, far = k['near'].copy(), k['far'].copy()
    near[0, 1, 9, 30], near[0, 2, 16, 63] = np.nan, np.inf
    far[0, 2, 5, 50], far[0, 0, 12, 20] = np.nan, -np.inf
    for quant, (patch, stride) in itertools.product(I.QUANTS, ((8, 4), (4, 3))):
        want = I.restate(near, far, k['f'], k['fm'], sign, quant=quant, patch=patch, stride=stride)
        for layout in T.LAYOUTS:
            got = raw_call(near, far, 'float32', layout, k['f'], k['fm'], sign, quant, patch=patch, stride=stride)
            check(got, want, (quant, patch, layout))
            assert np.isfinite(got['vecs']).all() and np.isfinite(got['patch_vecs']).all()
            assert 0 < (got['mask'] == 0).sum() < 0.5 * got['mask'].size and np.isinf(got['patch_ssd']).any()
            assert not got['vecs'][got['mask'] == 0].any()


@pytest.mark.parametrize("kind", ['random', 'shift'])
def test_non_finite_vectors(gpu, kind):
    """init fields with NaN and Inf vectors (nonfinite_cases): a patch whose centre holds one starts from zero, no output is
    ever non-finite"""
    B, h, w = shape = (1, 19, 70)
    k = NF.case(shape, kind, 'sprinkle')
    c, sign = 2, k['sign']
    rng = np.random.default_rng(h + w)
    far = (128 + rng.standard_normal((B, c, h, w)) * 40).astype(F32)
    near = (128 + rng.standard_normal((B, c, h, w)) * 40).astype(F32)
    for quant, layout, stride in itertools.product(I.QUANTS, T.LAYOUTS, (1, 4)):
        want = I.restate(near, far, k['fb'], k['mb'], sign, quant=quant, stride=stride)
        got = raw_call(near, far, 'float32', layout, k['fb'], k['mb'], sign, quant, stride=stride)
        check(got, want, (kind, quant, layout, stride))
        assert np.isfinite(got['vecs']).all() and np.isfinite(got['patch_vecs']).all() and got['mask'].all()
        if stride == 1:
            oys, oxs = np.array(I.origins(h, 8, 1)) + 4, np.array(I.origins(w, 8, 1)) + 4
            assert (~np.isfinite(k['fb'][0][oys[:, None], oxs[None, :]]).all(axis=-1)).any()     # a centre with a bad vector exists


def test_a_flat_image_returns_the_init(gpu):
    shape = (19, 70)
    k = I.case(2, shape, 1, nat.QUANT_EXACT, 1)
    flat = np.full((1, 2) + shape, 93.5, F32)
    for patch, stride, layout in ((8, 4, 'chw'), (4, 3, 'hwc')):
        want = I.restate(flat, flat, k['f'], k['fm'], 1, patch=patch, stride=stride)
        got = raw_call(flat, flat, 'float32', layout, k['f'], k['fm'], 1, patch=patch, stride=stride)
        check(got, want, (patch, stride))
        assert np.array_equal(bits(got['patch_vecs']), bits(want['u0'])) and got['mask'].all()


# ---------------------------------------------------------------------------------------------- 4: batches
@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_a_batch_equals_its_single_calls(gpu, layout):
    shape, sign, c, n = (37, 131), -1, 3, 3
    k = I.case(8, shape, sign, nat.QUANT_EXACT, c, 'float16', n, True, (('iterations', 5),))
    near, far = (dev.DeviceTensor.from_host(I.in_layout(k[name], layout), layout) for name in ('near', 'far'))
    batch = DeviceFlowBatch.from_flows([of.Flow(k['f'][i], 't', k['fm'][i]) for i in range(n)])
    out, pv, ps, grid = batch.inverse_search(near, far, iterations=5, return_patches=True)
    assert isinstance(out, DeviceFlowBatch) and (out.n, out.shape, out.ref) == (n, shape, 't') and grid == k['want']['grid']
    got = dict(vecs=out.vecs.to_host((n,) + shape + (2,), F32), mask=out.mask.to_host((n,) + shape, U8),
               patch_vecs=pv.to_host((n,) + grid + (2,), F32), patch_ssd=ps.to_host((n,) + grid, F32))
    check(got, k['want'], "batch")
    for i in range(n):
        one_near, one_far = (dev.DeviceTensor.from_host(I.in_layout(k[name][i:i + 1], layout, False), layout) for name in ('near', 'far'))
        single = dev.DeviceFlow.from_host(k['f'][i], 't', k['fm'][i]).inverse_search(one_near, one_far, iterations=5)
        assert single.vecs.to_host(shape + (2,), F32).tobytes() == got['vecs'][i].tobytes()
        assert single.mask.to_host(shape, U8).tobytes() == got['mask'][i].tobytes()
    assert len({got['vecs'][i].tobytes() for i in range(n)}) == n


# ---------------------------------------------------------------------------------------------- 5: every layer
@pytest.mark.parametrize("ref", ['s', 't'])
def test_host_forms_equal_the_device_form(gpu, ref):
    shape, sign, c = (37, 131), (1 if ref == 's' else -1), 3
    k = I.case(9, shape, sign, nat.QUANT_EXACT, c)
    want = k['want']
    near, far = I.in_layout(k['near'], 'hwc', False), I.in_layout(k['far'], 'hwc', False)
    f, fm = k['f'][0], k['fm'][0]
    flow = dev.DeviceFlow.from_host(f, ref, fm)
    # a float32 DeviceImage is an 'hwc' tensor
    out, pv, ps, grid = flow.inverse_search(dev.DeviceImage.from_host(near), dev.DeviceImage.from_host(far), return_patches=True)
    assert isinstance(out, dev.DeviceFlow) and (out.shape, out.ref) == (shape, ref) and grid == want['grid']
    d_vecs, d_mask = out.vecs.to_host(shape + (2,), F32), out.mask.to_host(shape, U8)
    check(dict(vecs=d_vecs[None], mask=d_mask[None], patch_vecs=pv.to_host((1,) + grid + (2,), F32),
               patch_ssd=ps.to_host((1,) + grid, F32)), want, "device")
    # the raw ABI, with patch buffers and with the records in the workspace
    with_buffers = raw_call(k['near'], k['far'], 'float32', 'chw', k['f'], k['fm'], sign)
    without = raw_call(k['near'], k['far'], 'float32', 'chw', k['f'], k['fm'], sign, patches=False)
    check(with_buffers, want, "raw")
    check(without, want, "raw, no patch buffers")
    assert with_buffers['vecs'].tobytes() == without['vecs'].tobytes() and with_buffers['mask'].tobytes() == without['mask'].tobytes()
    # Flow.inverse_search: channels last, planar, one plane
    h_out, h_pv, h_ps, h_grid = of.Flow(f, ref, fm).inverse_search(near, far, return_patches=True)
    assert isinstance(h_out, of.Flow) and h_out.ref == ref and h_grid == grid and h_out.mask.dtype == np.bool_
    assert h_out.vecs.tobytes() == d_vecs.tobytes() and h_out.mask.view(U8).tobytes() == d_mask.tobytes()
    assert np.array_equal(bits(h_pv), bits(want['patch_vecs'][0])) and np.array_equal(bits(h_ps), bits(want['patch_ssd'][0]))
    p_out = of.Flow(f, ref, fm).inverse_search(k['near'][0], k['far'][0], layout='chw')
    assert p_out.vecs.tobytes() == d_vecs.tobytes()
    g_out = of.Flow(f, ref, fm).inverse_search(k['near'][0, 0], k['far'][0, 0], patch=4, stride=2, quant=nat.QUANT_OPENCV)
    one = I.restate(k['near'][:, :1], k['far'][:, :1], f, fm, sign, quant=nat.QUANT_OPENCV, patch=4, stride=2)
    assert np.array_equal(bits(g_out.vecs), bits(one['vecs'][0]))
    # arrays in, with and without the mask
    a = of.inverse_search_flow(f, near, far, ref, fm)
    assert a.dtype == F32 and a.tobytes() == d_vecs.tobytes()
    full = I.restate(k['near'], k['far'], f, None, sign)
    assert np.array_equal(bits(of.inverse_search_flow(f, near, far, ref)), bits(full['vecs'][0]))
    # the zero field is what flow = NULL means
    zero = I.restate(k['near'], k['far'], None, None, sign)
    z = dev.DeviceFlow.zero(shape, ref).inverse_search(dev.DeviceImage.from_host(near), dev.DeviceImage.from_host(far))
    assert np.array_equal(bits(z.vecs.to_host(shape + (2,), F32)), bits(zero['vecs'][0]))
    check(raw_call(k['near'], k['far'], 'float32', 'hwc', None, None, sign), zero, "flow = NULL")


def test_the_raw_host_entry(gpu):
    shape, sign, c, dtype, n = (19, 70), -1, 4, 'float16', 2
    h, w = shape
    k = I.case(6, shape, sign, nat.QUANT_OPENCV, c, dtype, n)
    ny, nx = k['want']['grid']
    for layout in T.LAYOUTS:
        near, far = I.in_layout(k['near'], layout), I.in_layout(k['far'], layout)
        f, fm = np.ascontiguousarray(k['f'], F32), np.ascontiguousarray(k['fm']).view(U8)
        got = dict(vecs=np.empty((n, h, w, 2), F32), mask=np.empty((n, h, w), U8), patch_vecs=np.empty((n, ny, nx, 2), F32),
                   patch_ssd=np.empty((n, ny, nx), F32))
        nat.check(nat.load().ofl_inverse_search(near.ctypes.data, far.ctypes.data, EL[dtype], LAYOUT[layout], n, c, h, w, f.ctypes.data,
                                                fm.ctypes.data, sign, 8, 4, 12, 1, F32(1.0), got['vecs'].ctypes.data, got['mask'].ctypes.data,
                                                got['patch_vecs'].ctypes.data, got['patch_ssd'].ctypes.data, nat.QUANT_OPENCV))
        check(got, k['want'], layout)


def test_uint8_images_equal_their_float32_conversion(gpu):
    shape = (19, 70)
    rng = np.random.default_rng(3)
    k = I.case(3, shape, -1, nat.QUANT_EXACT, 3)
    img0 = np.clip(np.rint(I.in_layout(k['near'], 'hwc', False)), 0, 255).astype(np.uint8)
    img1 = np.clip(np.rint(I.in_layout(k['far'], 'hwc', False) + rng.uniform(-2, 2, shape + (3,))), 0, 255).astype(np.uint8)
    a = of.inverse_search_flow(k['f'][0], img0, img1, 't', k['fm'][0])
    b = of.inverse_search_flow(k['f'][0], img0.astype(F32), img1.astype(F32), 't', k['fm'][0])
    want = I.restate(np.moveaxis(img0.astype(F32), -1, 0)[None], np.moveaxis(img1.astype(F32), -1, 0)[None], k['f'][0], k['fm'][0], -1)
    assert a.tobytes() == b.tobytes() and np.array_equal(bits(a), bits(want['vecs'][0])) and (bits(a) != bits(k['f'][0])).any()


# ---------------------------------------------------------------------------------------------- 6: halve
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_halve_equals_the_restatement(gpu, dtype, layout):
    for shape in ((1, 5, 7), (3, 6, 8), (4, 7, 7), (2, 3, 9, 14), (1, 2, 2), (2, 5, 2, 131)):
        batched = len(shape) == 4
        planar = T.values(shape if batched else (1,) + shape, dtype, seed=sum(shape))
        t = dev.DeviceTensor.from_host(T.from_planar(planar, layout, batched), layout, dtype='bfloat16' if dtype == 'bfloat16' else None)
        half = t.halve()
        want = I.halve(planar, dtype)
        assert half.shape == shape[:-2] + (shape[-2] // 2, shape[-1] // 2) and (half.layout, half.dtype) == (layout, dtype)
        got = T.to_planar(half.to_host(), layout)
        assert got.shape == want.shape and np.array_equal(T.raw(got), T.raw(want)), (shape, dtype, layout)
        if dtype != 'bfloat16':
            assert np.array_equal(T.raw(of.halve_tensor(T.from_planar(planar, layout, batched), layout)), T.raw(T.from_planar(want, layout, batched)))
    with pytest.raises(ValueError, match="Error halving tensor: a 1 x 8 tensor has no 2 x 2 mean"):
        dev.DeviceTensor.from_host(np.zeros((3, 1, 8), F32)).halve()


# ---------------------------------------------------------------------------------------------- 7: estimate_flow
def tensors_of(i, layout='chw'):
    shape, v, levels, border, zero = I.KNOWN[i]
    near, far = I.shifted_pair(shape, v)
    return (dev.DeviceTensor.from_host(I.in_layout(near, layout, False), layout), dev.DeviceTensor.from_host(I.in_layout(far, layout, False), layout),
            near, far)


@pytest.mark.parametrize("levels", [2, 3])
def test_estimate_flow_is_the_chain_of_device_methods(gpu, levels):
    near, far, _, _ = tensors_of(2)
    shape = (128, 192)
    for refine, kw in ((True, dict()), (False, dict(patch=4, stride=2, iterations=5))):
        got = dev.estimate_flow(near, far, 's', levels, refine=refine, refine_args=dict(sor=3) if refine else None, **kw)
        pyramid = [(near, far)]
        for _ in range(levels - 1):
            pyramid.append((pyramid[-1][0].halve(), pyramid[-1][1].halve()))
        flow = dev.DeviceFlow.zero((shape[0] >> (levels - 1), shape[1] >> (levels - 1)), 's')
        for level in range(levels - 1, -1, -1):
            flow = flow.inverse_search(*pyramid[level], **kw)
            if refine:
                flow = flow.refine(*pyramid[level], sor=3)
            if level:
                flow = flow.resize(2)
        assert isinstance(got, dev.DeviceFlow) and (got.shape, got.ref) == (shape, 's')
        assert got.vecs.to_host(shape + (2,), F32).tobytes() == flow.vecs.to_host(shape + (2,), F32).tobytes()
        assert got.mask.to_host(shape, U8).tobytes() == flow.mask.to_host(shape, U8).tobytes()


def test_estimate_flow_without_refinement_equals_the_restatement(gpu):
    near, far, _, _ = tensors_of(2)
    got = dev.estimate_flow(near, far, 's', 2, refine=False)
    want = I.known(2)
    assert np.array_equal(bits(got.vecs.to_host((128, 192, 2), F32)), bits(want['vecs']))
    np.testing.assert_array_equal(got.mask.to_host((128, 192), U8), want['mask'].astype(U8))


def test_estimate_flow_finds_the_known_shift_with_the_defaults(gpu):
    """(5.3, -3.7) on (128, 192): the zero field's error is 6.4637; below a tenth of it is asked for"""
    shape, v, levels, border, zero = I.KNOWN[2]
    near, far, h_near, h_far = tensors_of(2)
    got = dev.estimate_flow(near, far)
    assert got.ref == 's'
    e = I.epe(got.vecs.to_host(shape + (2,), F32), v, border)
    print("estimate_flow, defaults:", e, "of", zero)
    assert e < 0.1 * zero and got.mask.to_host(shape, U8).all()
    # the host form, ref 't': the vectors sit on img2's pixels and point from img1 to img2, the same translation
    flow = of.estimate_flow(h_near[0, 0], h_far[0, 0])
    assert isinstance(flow, of.Flow) and flow.ref == 't' and flow.shape == shape
    e_t = I.epe(flow.vecs, v, border)
    print("of.estimate_flow, ref 't':", e_t)
    assert e_t < 0.1 * zero
    # an init: the result of the first call, refined by a second one
    again = dev.estimate_flow(near, far, levels=1, init=got)
    assert I.epe(again.vecs.to_host(shape + (2,), F32), v, border) < 0.1 * zero


def test_estimate_flow_refuses_sizes_that_do_not_halve(gpu):
    t = dev.DeviceTensor.from_host(np.zeros((1, 100, 192), F32))
    with pytest.raises(ValueError, match="Error estimating flow: .*pad"):
        dev.estimate_flow(t, t, levels=4)
    with pytest.raises(ValueError, match="Error estimating flow: .*pad"):
        of.estimate_flow(np.zeros((100, 192), F32), np.zeros((100, 192), F32), levels=4)
    assert dev.estimate_flow(t, t, levels=3).shape == (100, 192)
    with pytest.raises(TypeError, match="Error estimating flow: near needs to be a DeviceTensor"):
        dev.estimate_flow(np.zeros((1, 32, 32), F32), t)
    with pytest.raises(ValueError, match="Error estimating flow: init needs to be a DeviceFlow of shape"):
        dev.estimate_flow(t, t, init=dev.DeviceFlow.zero((50, 96), 's'))


# ---------------------------------------------------------------------------------------------- 8: errors
def test_method_errors(gpu):
    prefix = "Error searching flow: "
    f = dev.DeviceFlow.zero((16, 24), 't')
    t = lambda shape, layout='chw', dtype=np.float32: dev.DeviceTensor.from_host(np.zeros(shape, dtype), layout)
    a = t((3, 16, 24))
    with pytest.raises(ValueError, match=prefix + "the tensors need the same shape"):
        f.inverse_search(a, t((4, 16, 24)))
    with pytest.raises(TypeError, match=prefix + "the tensors need the same dtype, got float32 and float16"):
        f.inverse_search(a, t((3, 16, 24), dtype=np.float16))
    with pytest.raises(ValueError, match=prefix + r"tensors and flow need the same height and width, got \(16, 24\) and \(16, 25\)"):
        dev.DeviceFlow.zero((16, 25), 't').inverse_search(a, a)
    with pytest.raises(TypeError, match=prefix + "near needs to be a DeviceTensor or a float32 DeviceImage, got ndarray"):
        f.inverse_search(np.zeros((3, 16, 24), F32), a)
    with pytest.raises(ValueError, match=prefix + r"the tensors need 1 to 4 channels \(grey, two-plane, RGB, RGBA\), got 5"):
        f.inverse_search(t((5, 16, 24)), t((5, 16, 24)))
    with pytest.raises(ValueError, match=prefix + r"one field takes tensors of shape \(C, H, W\) or \(1, C, H, W\)"):
        f.inverse_search(t((2, 3, 16, 24)), t((2, 3, 16, 24)))
    with pytest.raises(ValueError, match=prefix + "patch must be 4 or 8, got 12"):
        f.inverse_search(a, a, patch=12)
    with pytest.raises(ValueError, match=prefix + r"stride must be in \[1, patch = 8\], got 9"):
        f.inverse_search(a, a, stride=9)
    with pytest.raises(TypeError, match=prefix + "floor must be a number"):
        f.inverse_search(a, a, floor=None)
    with pytest.raises(ValueError, match=prefix + "a 6 x 24 field holds no patch of 8"):
        dev.DeviceFlow.zero((6, 24), 't').inverse_search(t((1, 6, 24)), t((1, 6, 24)))
    b = DeviceFlowBatch.from_flows([of.Flow.zero((16, 24), 't')] * 2)
    with pytest.raises(ValueError, match=prefix + r"a batch of 2 fields takes tensors of shape \(2, C, H, W\)"):
        b.inverse_search(a, a)
    out = f.inverse_search(t((1, 3, 16, 24)), t((1, 3, 16, 24)))
    assert out.vecs.to_host((16, 24, 2), F32).tobytes() == bytes(16 * 24 * 8) and out.mask.to_host((16, 24), U8).all()


def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    h, w = 16, 24
    n, npatch = h * w, 3 * 5
    t, f, fm = dev.DeviceBuffer.zeros(n * 5 * 4), dev.DeviceBuffer.zeros(n * 8), dev.DeviceBuffer.zeros(n)
    out, mask, work = dev.DeviceBuffer.zeros(n * 8 + 8), dev.DeviceBuffer.zeros(n), dev.DeviceBuffer.zeros(8 * n + 12 * npatch + 8)
    pv, ps = dev.DeviceBuffer.zeros(npatch * 8 + 8), dev.DeviceBuffer.zeros(npatch * 4)
    nat.check(lib.ofl_memset(out.ptr, 7, n * 8, None))
    nat.check(lib.ofl_memset(mask.ptr, 7, n, None))

    def call(near=t.ptr, far=t.ptr, elem=nat.EL_F32, layout=nat.TENSOR_NCHW, N=1, C=3, hh=h, ww=w, flow=f.ptr, fmask=fm.ptr, sign=1,
             patch=8, stride=4, iterations=12, floor=F32(1), ws=work.ptr, ws_bytes=8 * n + 12 * npatch, o=out.ptr, om=mask.ptr,
             v=None, s=None, quant=nat.QUANT_EXACT):
        return lib.ofl_inverse_search_dev(near, far, elem, layout, N, C, hh, ww, flow, fmask, sign, patch, stride, iterations, 1, floor,
                                          ws, ws_bytes, o, om, v, s, quant, None)

    for kw in (dict(near=None), dict(far=None), dict(o=None), dict(om=None), dict(elem=nat.EL_F64), dict(elem=9), dict(layout=2),
               dict(N=0), dict(N=65536), dict(C=0), dict(C=5), dict(hh=7), dict(ww=32767), dict(patch=4, ww=3), dict(sign=0),
               dict(patch=6), dict(patch=16), dict(stride=0), dict(stride=9), dict(patch=4, stride=5), dict(iterations=0), dict(iterations=33),
               dict(floor=F32(0)), dict(floor=F32(-1)), dict(floor=F32('nan')), dict(floor=F32('inf')), dict(quant=7),
               dict(ws=None), dict(ws_bytes=8 * n + 12 * npatch - 1), dict(v=pv.ptr, ws_bytes=8 * n), dict(ws=work.ptr + 4),
               dict(near=t.ptr + 2), dict(flow=f.ptr + 4), dict(o=out.ptr + 4), dict(v=pv.ptr + 4, s=ps.ptr), dict(v=pv.ptr, s=ps.ptr + 2),
               dict(o=f.ptr), dict(ws=out.ptr), dict(o=t.ptr), dict(om=fm.ptr), dict(v=out.ptr, s=ps.ptr), dict(v=pv.ptr, s=pv.ptr)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_inverse_search" in nat.last_error(), kw
    dev.sync()
    assert (out.to_host((n * 8,), U8) == 7).all() and (mask.to_host((n,), U8) == 7).all()         # nothing was launched
    assert call() == nat.OK and call(v=pv.ptr, s=ps.ptr, ws_bytes=8 * n) == nat.OK and call(flow=None, fmask=None) == nat.OK
    assert not out.to_host((n * 2,), F32).any() and mask.to_host((n,), U8).all()                  # flat images, the zero field
    for bad in (dict(src=None), dict(dst=None), dict(elem=nat.EL_F64), dict(layout=3), dict(h=1), dict(w=1), dict(C=0), dict(dst='src')):
        a = dict(src=t.ptr, elem=nat.EL_F32, layout=nat.TENSOR_NCHW, N=1, C=3, h=h, w=w, dst=out.ptr)
        a.update(bad)
        if a['dst'] == 'src':
            a['dst'] = a['src']
        assert lib.ofl_tensor_halve_dev(a['src'], a['elem'], a['layout'], a['N'], a['C'], a['h'], a['w'], a['dst'], None) == nat.E_INVALID, bad
        assert "ofl_tensor_halve" in nat.last_error()
