"""K21 (ofl_photometric.hip): the photometric error of a warp on the device, bit for bit against tests/photometric_ref.py
(the oracle's gather plus float32 NumPy in the stated order), against K12 on the device itself, and through every layer:
the raw ABI, DeviceFlow.photometric, DeviceFlowBatch.photometric, Flow.photometric and photometric_error.  Nothing here has
a tolerance: masks and counts are compared with array_equal, errors through their bits (a NaN may carry any payload)."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import devmem
import interop_ref as R
import nonfinite_cases as NF
import photometric_ref as P
import splat_ref as S
import tensor_ref as T

pytestmark = pytest.mark.gpu
nat = of.native
F32, U8 = np.float32, np.uint8
METRIC_CODE = {'l1': nat.PHOTO_L1, 'l2': nat.PHOTO_L2, 'charbonnier': nat.PHOTO_CHARBONNIER}
EL = {'float32': nat.EL_F32, 'float16': nat.EL_F16, 'bfloat16': nat.EL_BF16}
LAYOUT = {'chw': nat.TENSOR_NCHW, 'hwc': nat.TENSOR_NHWC}


def up(a):
    a = np.ascontiguousarray(a)
    return dev.DeviceBuffer.from_host(a.view(U8) if a.dtype == np.bool_ else a)


def ptr(x):
    return None if x is None else x.ptr


def raw_call(near, far, dtype, layout, f, fm, sign, metric='l1', eps=P.EPS, tau=None, near_mask=None, far_mask=None,
             quant=nat.QUANT_OPENCV, shared=True, err=True, covered=True, counts=True):
    """ofl_photometric_dev on host arrays: near, far planar (n, c, h, w) as stored in `dtype`, uploaded in the memory order of
    `layout` -> (err | None, covered | None, within | None, counts | None) on the host, each (n, h, w) / (n, 2)"""
    n, c, h, w = near.shape
    px = n * h * w
    d_near, d_far = up(P.in_layout(near, layout)), up(P.in_layout(far, layout))
    d_f, d_fm = up(np.ascontiguousarray(f, F32)), up(fm)
    d_nm, d_am = (None if m is None else up(m) for m in (near_mask, far_mask))
    d_err = dev.DeviceBuffer(px * 4) if err else None
    d_cov = dev.DeviceBuffer(px) if covered else None
    d_wi = dev.DeviceBuffer(px) if tau is not None else None
    d_cnt = dev.DeviceBuffer.zeros(n * 8) if counts else None
    nat.check(nat.load().ofl_photometric_dev(d_near.ptr, d_far.ptr, EL[dtype], LAYOUT[layout], n, c, h, w, d_f.ptr, d_fm.ptr,
                                             1 if shared else 0, sign, ptr(d_nm), ptr(d_am), METRIC_CODE[metric], F32(eps),
                                             F32(0 if tau is None else tau), ptr(d_err), ptr(d_cov), ptr(d_wi), ptr(d_cnt), quant, None))
    return (d_err.to_host((n, h, w), F32) if err else None, d_cov.to_host((n, h, w), U8) if covered else None,
            d_wi.to_host((n, h, w), U8) if tau is not None else None, d_cnt.to_host((n, 2), np.uint32) if counts else None)


def check(got, want, what, tau=True):
    """(err, covered, within, counts) as raw_call gives them against restate()'s dict; None outputs are skipped"""
    err, cov, wi, cnt = got
    if err is not None:
        assert P.same_floats(err, want['err']), "{}: err".format(what)
    if cov is not None:
        np.testing.assert_array_equal(cov, want['covered'].astype(U8), err_msg="{}: covered".format(what))
    if wi is not None:
        np.testing.assert_array_equal(wi, want['within'].astype(U8), err_msg="{}: within".format(what))
    if cnt is not None:
        assert [tuple(int(v) for v in row) for row in cnt] == [(a, b if wi is not None else 0) for a, b in want['counts']], what
        if cov is not None:
            assert [int(v) for v in cnt[:, 0]] == [int(v) for v in cov.sum(axis=(1, 2))], what
        if wi is not None:
            assert [int(v) for v in cnt[:, 1]] == [int(v) for v in wi.sum(axis=(1, 2))], what


def run_case(shape, sign, quant, metric, layout, dtype, c, n=1, seed=1):
    k = P.case(seed, shape, sign, quant, c, dtype, metric, n)
    got = raw_call(k['near'], k['far'], dtype, layout, k['f'], k['fm'], sign, metric, tau=k['tau'], quant=quant)
    check(got, k['want'], (shape, sign, quant, metric, layout, dtype, c, n))
    return got


# ---------------------------------------------------------------------------------------------- 1: channels x layout x dtype
@pytest.mark.parametrize("c", P.CHANNELS)
def test_every_channel_count_layout_and_dtype(gpu, c):
    """(19, 70): every C x layout x dtype; sign, quant and metric rotate through the product so that each occurs"""
    base = P.CHANNELS.index(c)
    for i, (dtype, layout) in enumerate(itertools.product(T.DTYPES, T.LAYOUTS)):
        idx = base * 6 + i
        sign, quant, metric = P.SIGNS[idx % 2], P.QUANTS[(idx // 2) % 2], P.METRICS[idx % 3]
        run_case((19, 70), sign, quant, metric, layout, dtype, c)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_planar_and_channels_last_give_identical_bytes(gpu, dtype):
    for c, metric in ((3, 'l1'), (33, 'l2'), (130, 'charbonnier')):
        a = run_case((19, 70), -1, nat.QUANT_OPENCV, metric, 'chw', dtype, c)
        b = run_case((19, 70), -1, nat.QUANT_OPENCV, metric, 'hwc', dtype, c)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# ---------------------------------------------------------------------------------------------- 2: shapes
# thinned product: at every shape each sign, quant, metric, layout and dtype occurs at least once
THIN = [(1, nat.QUANT_OPENCV, 'l1', 'chw', 'float32', 3), (-1, nat.QUANT_EXACT, 'l2', 'hwc', 'float16', 5),
        (1, nat.QUANT_EXACT, 'charbonnier', 'chw', 'bfloat16', 4), (-1, nat.QUANT_OPENCV, 'l1', 'hwc', 'float32', 33),
        (1, nat.QUANT_OPENCV, 'l2', 'chw', 'float16', 17), (-1, nat.QUANT_EXACT, 'charbonnier', 'hwc', 'bfloat16', 1)]


@pytest.mark.parametrize("shape", P.TINY + P.SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_shapes(gpu, shape):
    for sign, quant, metric, layout, dtype, c in THIN:
        run_case(shape, sign, quant, metric, layout, dtype, c)


# ---------------------------------------------------------------------------------------------- 3: batches
@pytest.mark.parametrize("layout, dtype", [('chw', 'float32'), ('hwc', 'float16')])
def test_three_items_share_one_field(gpu, layout, dtype):
    shape, sign, c = (19, 70), -1, 5
    k = P.case(4, shape, sign, nat.QUANT_OPENCV, c, dtype, 'l1', 3)
    got = raw_call(k['near'], k['far'], dtype, layout, k['f'], k['fm'], sign, tau=k['tau'])
    check(got, k['want'], "three items")
    for i in range(3):                                    # each item alone gives the same bytes
        one = raw_call(k['near'][i:i + 1], k['far'][i:i + 1], dtype, layout, k['f'], k['fm'], sign, tau=k['tau'])
        assert one[0].tobytes() == got[0][i].tobytes() and one[1].tobytes() == got[1][i].tobytes()
        np.testing.assert_array_equal(one[3][0], got[3][i])
    # the method: one field serves every item of a batched tensor
    flow = dev.DeviceFlow.from_host(k['f'], 't', k['fm'])
    kw = dict(dtype='bfloat16') if dtype == 'bfloat16' else {}
    near_t = dev.DeviceTensor.from_host(P.in_layout(k['near'], layout), layout, **kw)
    far_t = dev.DeviceTensor.from_host(P.in_layout(k['far'], layout), layout, **kw)
    err, cov, wi, cnt = flow.photometric(near_t, far_t, threshold=float(k['tau']), return_counts=True)
    full = (3,) + shape
    check((err.to_host(full, F32), cov.to_host(full, U8), wi.to_host(full, U8), np.array(cnt, np.uint32)), k['want'], "method")
    assert all(isinstance(v, int) for row in cnt for v in row) and len(cnt) == 3
    assert len(flow.photometric(near_t, far_t)) == 2 and len(flow.photometric(near_t, far_t, threshold=0.1)) == 3


@pytest.mark.parametrize("shape", [(37, 53), (5, 7)], ids=lambda s: "{}x{}".format(*s))
@pytest.mark.parametrize("ref", ['s', 't'])
def test_batch_method_per_item_fields_and_masks_and_field_views(gpu, shape, ref):
    """three different fields with their own masks in a batch of an odd pixel count: the fields 1 and 2 start at odd mask
    addresses and, for field 1, on an 8-byte but not 16-byte boundary"""
    h, w = shape
    assert (h * w) % 2 == 1
    sign, c, layout, dtype = (1 if ref == 's' else -1), 5, 'hwc', 'float32'
    rng = np.random.default_rng(9)
    fs, fms, nears, fars = [], [], [], []
    for i in range(3):
        f, fm = P.field(rng, shape)
        near, far = P.tensors(rng, 1, c, f, sign, dtype)
        fs.append(f), fms.append(fm), nears.append(near[0]), fars.append(far[0])
    f, fm, near, far = np.stack(fs), np.stack(fms), np.stack(nears), np.stack(fars)
    nm, am = np.ones((3, h, w), U8), np.ones((3, h, w), U8)
    for i in range(3):
        nm[i, i:h // 2, w // 2:] = 0
        am[i, h // 2:, i:w // 3] = 0
    first = P.restate(near, far, f, fm, sign, near_mask=nm, far_mask=am)
    tau = F32(np.median(first['e'][first['covered']]))
    want = P.restate(near, far, f, fm, sign, tau=tau, near_mask=nm, far_mask=am)
    b = DeviceFlowBatch(3, shape, ref)
    v, m = np.ascontiguousarray(f, F32), np.ascontiguousarray(fm).view(U8)
    nat.check(nat.load().ofl_upload(b.vecs.ptr, v.ctypes.data, v.nbytes, None))
    nat.check(nat.load().ofl_upload(b.mask.ptr, m.ctypes.data, m.nbytes, None))
    dev.sync()
    near_t, far_t = dev.DeviceTensor.from_host(P.in_layout(near, layout), layout), dev.DeviceTensor.from_host(P.in_layout(far, layout), layout)
    d_nm, d_am = up(nm), up(am)
    err, cov, wi, cnt = b.photometric(near_t, far_t, threshold=float(tau), near_mask=d_nm, far_mask=d_am, return_counts=True)
    full = (3,) + shape
    check((err.to_host(full, F32), cov.to_host(full, U8), wi.to_host(full, U8), cnt), want, "batch")
    assert cnt.shape == (3, 2) and len(b.photometric(near_t, far_t)) == 2
    for i in range(3):                                    # field(i): a view inside the batch, with item i's tensors and masks
        view = b.field(i)
        ni = dev.DeviceTensor.from_host(P.in_layout(near[i:i + 1], layout, False), layout)
        fi = dev.DeviceTensor.from_host(P.in_layout(far[i:i + 1], layout, False), layout)
        e1, c1, w1 = view.photometric(ni, fi, threshold=float(tau), near_mask=d_nm.view(i * h * w, h * w), far_mask=d_am.view(i * h * w, h * w))
        assert e1.to_host(shape, F32).tobytes() == err.to_host(full, F32)[i].tobytes()
        np.testing.assert_array_equal(c1.to_host(shape, U8), want['covered'][i].astype(U8))
        np.testing.assert_array_equal(w1.to_host(shape, U8), want['within'][i].astype(U8))
    with pytest.raises(ValueError, match="a batch of 3 fields"):
        b.photometric(dev.DeviceTensor.from_host(P.in_layout(near[:2], layout), layout), dev.DeviceTensor.from_host(P.in_layout(far[:2], layout), layout))


# ---------------------------------------------------------------------------------------------- 4: masks, optional outputs
@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_masks_and_optional_outputs(gpu, layout):
    shape, sign, c, dtype = (37, 131), 1, 3, 'float32'
    h, w = shape
    k = P.case(5, shape, sign, nat.QUANT_OPENCV, c, dtype, 'l1')
    near_hole, far_hole = np.ones(shape, U8), np.ones(shape, U8)
    near_hole[3:9, 100:] = 0
    far_hole[h // 2:3 * h // 4, w // 2:3 * w // 4] = 0
    # every combination of err, covered, within and counts in which err or within is there
    outputs = [o for o in itertools.product([True, False], repeat=4) if o[0] or o[2]]
    assert len(outputs) == 12
    for nm, am in ((near_hole, None), (None, far_hole), (near_hole, far_hole)):
        wants = {wi: P.restate(R.to_f32(k['near'], dtype), R.to_f32(k['far'], dtype), k['f'], k['fm'], sign,
                               tau=k['tau'] if wi else None, near_mask=nm, far_mask=am) for wi in (True, False)}
        assert wants[True]['covered'].sum() < k['want']['covered'].sum()      # the hole takes pixels away
        for e, cv, wi, cn in outputs:
            got = raw_call(k['near'], k['far'], dtype, layout, k['f'], k['fm'], sign, tau=k['tau'] if wi else None, near_mask=nm,
                           far_mask=am, err=e, covered=cv, counts=cn)
            assert (got[0] is not None, got[1] is not None, got[2] is not None, got[3] is not None) == (e, cv, wi, cn)
            check(got, wants[wi], (layout, nm is not None, am is not None, e, cv, wi, cn))


def test_guard_bytes_around_the_three_outputs(gpu):
    shape, sign, c, dtype, guard = (19, 70), -1, 4, 'float16', 256
    h, w = shape
    k = P.case(6, shape, sign, nat.QUANT_EXACT, c, dtype, 'l2', 2)
    px = 2 * h * w
    for layout in T.LAYOUTS:
        d_near, d_far = up(P.in_layout(k['near'], layout)), up(P.in_layout(k['far'], layout))
        d_f, d_fm = up(k['f']), up(k['fm'])
        g_err, g_cov, g_wi = devmem.guarded(px * 4, guard, 4), devmem.guarded(px, guard, 1), devmem.guarded(px, guard, 3)
        nat.check(nat.load().ofl_photometric_dev(d_near.ptr, d_far.ptr, EL[dtype], LAYOUT[layout], 2, c, h, w, d_f.ptr, d_fm.ptr, 1, sign,
                                                 None, None, nat.PHOTO_L2, F32(P.EPS), k['tau'], g_err.ptr + 4, g_cov.ptr + 1,
                                                 g_wi.ptr + 3, None, nat.QUANT_EXACT, None))
        dev.sync()
        got = (devmem.read_guarded(g_err, 4, px * 4, guard, F32, (2, h, w)), devmem.read_guarded(g_cov, 1, px, guard, U8, (2, h, w)),
               devmem.read_guarded(g_wi, 3, px, guard, U8, (2, h, w)), None)
        check(got, k['want'], layout)
        for buf, a in ((d_near, P.in_layout(k['near'], layout)), (d_far, P.in_layout(k['far'], layout))):     # inputs unchanged
            assert buf.to_host(a.shape, a.dtype).tobytes() == a.tobytes()


# ---------------------------------------------------------------------------------------------- 5: against K12 on the device
@pytest.mark.parametrize("quant", P.QUANTS)
@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_l1_against_zero_equals_the_tensor_warp(gpu, layout, quant):
    shape, c = (37, 131), 1
    h, w = shape
    k = P.case(3, shape, -1, quant, c)
    far = dev.DeviceTensor.from_host(P.in_layout(k['far'], layout, False), layout)
    zero = dev.DeviceTensor(dev.DeviceBuffer.zeros(far.nbytes), far.shape, far.dtype, far.layout)
    # 't': the method against apply_tensor
    flow = dev.DeviceFlow.from_host(k['f'], 't', k['fm'])
    warped, valid = flow.apply_tensor(far, quant=quant)
    err, cov = flow.photometric(zero, far, quant=quant)
    wv, vv = warped.to_host().reshape(shape), valid.to_host(shape, U8)
    np.testing.assert_array_equal(cov.to_host(shape, U8), vv)
    assert err.to_host(shape, F32).tobytes() == np.where(vv != 0, np.abs(wv), F32(0)).astype(F32).tobytes()
    # 's': the same field read forward, against the gather_tensor launch wrapper with sign +1
    dst, valid = dev.gather_tensor(far.buf, 'float32', layout, 1, c, h, w, flow.vecs, True, +1, fmask=flow.mask, want_valid=True, quant=quant)
    err, cov = dev.DeviceFlow.from_host(k['f'], 's', k['fm']).photometric(zero, far, quant=quant)
    wv, vv = dst.to_host(shape, F32), valid.to_host(shape, U8)
    np.testing.assert_array_equal(cov.to_host(shape, U8), vv)
    assert err.to_host(shape, F32).tobytes() == np.where(vv != 0, np.abs(wv), F32(0)).astype(F32).tobytes()


# ---------------------------------------------------------------------------------------------- 6: non-finite values
NF_SHAPES = [(1, 3, 5), (2, 13, 130)]          # nonfinite_cases' two smallest shapes with more than one row


@pytest.mark.parametrize("shape", NF_SHAPES, ids=lambda s: "{}x{}x{}".format(*s))
@pytest.mark.parametrize("kind, placement", [('random', 'sprinkle'), ('shift', 'class'), ('outside', 'sprinkle'), ('rotate', 'class')])
def test_non_finite_vectors(gpu, shape, kind, placement):
    """fields with NaN and Inf vectors: covered is K12's valid on the same fields, err the restatement's"""
    B, h, w = shape
    k = NF.case(shape, kind, placement)
    c, sign = 3, k['sign']
    rng = np.random.default_rng(B * h + w)
    far = rng.standard_normal((B, c, h, w)).astype(F32)
    near = rng.standard_normal((B, c, h, w)).astype(F32)
    for quant, layout in itertools.product(P.QUANTS, T.LAYOUTS):
        want = P.restate(near, far, k['fb'], k['mb'], sign, far_mask=k['ma'], quant=quant)
        got = raw_call(near, far, 'float32', layout, k['fb'], k['mb'], sign, far_mask=k['ma'], quant=quant, shared=False)
        check(got, want, (shape, kind, placement, quant, layout))
        dst, valid = dev.gather_tensor(up(P.in_layout(far, layout)), 'float32', layout, B, c, h, w, up(k['fb']), False, sign,
                                       smask=up(k['ma']), smask_shared=False, fmask=up(k['mb']), want_valid=True, quant=quant)
        np.testing.assert_array_equal(got[1], valid.to_host((B, h, w), U8))


@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_non_finite_tensor_values(gpu, layout):
    """a NaN and an Inf in far and in near: `covered` does not change, no affected pixel is within, a NaN gives a NaN error and
    an Inf the error the arithmetic of the definition gives (|Inf - w| = Inf under L1; NaN where a tap of weight 0 meets it)"""
    shape, sign, c, dtype = (19, 70), -1, 5, 'float32'
    k = P.case(7, shape, sign, nat.QUANT_EXACT, c, dtype, 'l1')
    clean = k['want']
    near, far = k['near'].copy(), k['far'].copy()
    cov_px = np.argwhere(clean['covered'][0])
    (y0, x0), (y1, x1) = cov_px[len(cov_px) // 3], cov_px[2 * len(cov_px) // 3]
    near[0, 1, y0, x0], near[0, 4, y1, x1] = np.nan, np.inf
    far[0, 2, shape[0] // 2, shape[1] // 2], far[0, 0, shape[0] // 3, shape[1] // 3] = np.nan, -np.inf
    want = P.restate(near, far, k['f'], k['fm'], sign, tau=k['tau'], quant=nat.QUANT_EXACT)
    bad = ~np.isfinite(want['e']) & want['covered']
    assert bad[0, y0, x0] and bad[0, y1, x1] and bad.sum() >= 4 and np.isnan(want['err'][0, y0, x0]) and np.isnan(want['err'][bad]).any()
    got = raw_call(near, far, dtype, layout, k['f'], k['fm'], sign, tau=k['tau'], quant=nat.QUANT_EXACT)
    check(got, want, layout)
    np.testing.assert_array_equal(got[1], clean['covered'].astype(U8))
    assert not np.isfinite(got[0][bad]).any() and not got[2][bad].any() and np.isnan(got[0][0, y0, x0])
    assert got[0][~bad].tobytes() == clean['err'][~bad].tobytes()


# ---------------------------------------------------------------------------------------------- 7: the error as an importance
@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_error_feeds_softmax_splatting(gpu, layout):
    shape, c = (19, 70), 3
    k = P.case(8, shape, 1, nat.QUANT_OPENCV, c)
    flow = dev.DeviceFlow.from_host(k['f'], 's', k['fm'])
    near_t = dev.DeviceTensor.from_host(P.in_layout(k['near'], layout, False), layout)
    far_t = dev.DeviceTensor.from_host(P.in_layout(k['far'], layout, False), layout)
    error, _ = flow.photometric(near_t, far_t)
    assert isinstance(error, dev.DeviceBuffer) and error.nbytes == shape[0] * shape[1] * 4
    out, valid = flow.splat(near_t, 'softmax', importance=error, alpha=-20.0)
    r = S.splat(R.to_f32(k['near'], 'float32'), k['f'], k['fm'], 'softmax', z=k['want']['err'][0], alpha=-20.0)
    assert T.to_planar(out.to_host(), layout).tobytes() == r['out'].tobytes()
    assert valid.to_host(shape, U8).tobytes() == r['valid'].tobytes()
    assert r['valid'].any() and not r['valid'].all()


# ---------------------------------------------------------------------------------------------- 8: the host forms
@pytest.mark.parametrize("ref", ['s', 't'])
def test_host_forms_equal_the_device_form(gpu, ref):
    shape, sign, c = (37, 131), (1 if ref == 's' else -1), 3
    k = P.case(9, shape, sign, nat.QUANT_OPENCV, c, 'float32', 'charbonnier')
    want, tau = k['want'], float(k['tau'])
    near, far = P.in_layout(k['near'], 'hwc', False), P.in_layout(k['far'], 'hwc', False)
    flow = dev.DeviceFlow.from_host(k['f'], ref, k['fm'])
    # a float32 DeviceImage is an 'hwc' tensor
    d_err, d_cov, d_wi = flow.photometric(dev.DeviceImage.from_host(near), dev.DeviceImage.from_host(far), 'charbonnier', threshold=tau)
    d = (d_err.to_host(shape, F32), d_cov.to_host(shape, U8), d_wi.to_host(shape, U8))
    check((d[0][None], d[1][None], d[2][None], None), want, "device")
    h_err, h_cov, h_wi = of.Flow(k['f'], ref, k['fm']).photometric(near, far, 'charbonnier', threshold=tau)
    assert h_err.dtype == F32 and h_cov.dtype == h_wi.dtype == np.bool_ and h_err.shape == h_cov.shape == shape
    assert h_err.tobytes() == d[0].tobytes() and h_cov.tobytes() == d[1].tobytes() and h_wi.tobytes() == d[2].tobytes()
    # planar arrays with layout='chw'; one plane as (H, W)
    p_err, p_cov = of.Flow(k['f'], ref, k['fm']).photometric(k['near'][0], k['far'][0], 'charbonnier', layout='chw')
    assert p_err.tobytes() == d[0].tobytes() and p_cov.tobytes() == d[1].tobytes()
    g_err, _ = of.Flow(k['f'], ref, k['fm']).photometric(k['near'][0, 0], k['far'][0, 0])
    one = P.restate(k['near'][:, :1], k['far'][:, :1], k['f'], k['fm'], sign)
    assert P.same_floats(g_err, one['err'][0])
    # arrays in, with and without the mask
    a_err, a_cov, a_wi = of.photometric_error(k['f'], near, far, ref, k['fm'], metric='charbonnier', threshold=tau)
    assert a_err.tobytes() == d[0].tobytes() and a_cov.tobytes() == d[1].tobytes() and a_wi.tobytes() == d[2].tobytes()
    n_err, n_cov = of.photometric_error(k['f'], near, far, ref)
    full = P.restate(k['near'], k['far'], k['f'], np.ones(shape, bool), sign)
    assert P.same_floats(n_err, full['err'][0]) and np.array_equal(n_cov, full['covered'][0])


def test_uint8_images_equal_their_float32_conversion(gpu):
    shape = (19, 70)
    rng = np.random.default_rng(3)
    img0, img1 = rng.integers(0, 256, shape + (3,), dtype=np.uint8), rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    f, fm = P.field(rng, shape)
    flow = of.Flow(f, 't', fm)
    a = flow.photometric(img0, img1, 'l2', threshold=60.0)
    b = flow.photometric(img0.astype(F32), img1.astype(F32), 'l2', threshold=60.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == 3
    want = P.restate(np.moveaxis(img0.astype(F32), -1, 0)[None], np.moveaxis(img1.astype(F32), -1, 0)[None], f, fm, -1, metric='l2', tau=60.0)
    assert P.same_floats(a[0], want['err'][0]) and np.array_equal(a[1], want['covered'][0]) and np.array_equal(a[2], want['within'][0])
    assert 0 < a[2].sum() < a[1].sum()


# ---------------------------------------------------------------------------------------------- 9: errors
def test_method_errors(gpu):
    prefix = "Error computing photometric error: "
    f = dev.DeviceFlow.zero((6, 9), 't')
    t = lambda shape, layout='chw', dtype=np.float32: dev.DeviceTensor.from_host(np.zeros(shape, dtype), layout)
    a = t((3, 6, 9))
    with pytest.raises(ValueError, match=prefix + "the tensors need the same shape"):
        f.photometric(a, t((4, 6, 9)))
    with pytest.raises(TypeError, match=prefix + "the tensors need the same dtype, got float32 and float16"):
        f.photometric(a, t((3, 6, 9), dtype=np.float16))
    with pytest.raises(ValueError, match=prefix + "the tensors need the same layout, got 'chw' and 'hwc'"):
        f.photometric(t((6, 6, 6)), dev.DeviceTensor(a.buf, (6, 6, 6), 'float32', 'hwc'))
    with pytest.raises(ValueError, match=prefix + r"tensors and flow need the same height and width, got \(6, 9\) and \(6, 10\)"):
        dev.DeviceFlow.zero((6, 10), 't').photometric(a, a)
    with pytest.raises(TypeError, match=prefix + "near needs to be a DeviceTensor or a float32 DeviceImage, got ndarray"):
        f.photometric(np.zeros((3, 6, 9), F32), a)
    with pytest.raises(TypeError, match=prefix + "far as a DeviceImage needs to be float32, got uint8"):
        f.photometric(a, dev.DeviceImage.from_host(np.zeros((6, 9, 3), np.uint8)))
    with pytest.raises(ValueError, match=prefix + "metric must be 'l1', 'l2' or 'charbonnier', got 'ssim'"):
        f.photometric(a, a, metric='ssim')
    with pytest.raises(ValueError, match=prefix + "threshold must be finite and not negative"):
        f.photometric(a, a, threshold=-1)
    with pytest.raises(TypeError, match=prefix + "eps must be a number or None"):
        f.photometric(a, a, eps=True)
    with pytest.raises(TypeError, match=prefix + "near_mask needs to be a DeviceBuffer"):
        f.photometric(a, a, near_mask=np.ones((6, 9), U8))
    with pytest.raises(ValueError, match=prefix + "far_mask needs to hold 54 bytes"):
        f.photometric(a, a, far_mask=dev.DeviceBuffer(10))
    # the host forms
    h = of.Flow.zero((6, 9), 't')
    with pytest.raises(ValueError, match=prefix + "the arrays need the same shape"):
        h.photometric(np.zeros((6, 9, 3), F32), np.zeros((6, 9, 4), F32))
    with pytest.raises(TypeError, match=prefix + "the arrays need the same dtype"):
        h.photometric(np.zeros((6, 9, 3), F32), np.zeros((6, 9, 3), np.float16))
    with pytest.raises(ValueError, match=prefix + "arrays and flow need the same height and width"):
        h.photometric(np.zeros((6, 8, 3), F32), np.zeros((6, 8, 3), F32))
    with pytest.raises(ValueError, match=prefix + "metric must be"):
        of.photometric_error(np.zeros((6, 9, 2), F32), np.zeros((6, 9), F32), np.zeros((6, 9), F32), 't', metric='census')
    with pytest.raises(TypeError, match=prefix + "far needs to have dtype float32, float16 or uint8, got float64"):
        h.photometric(np.zeros((6, 9, 3), F32), np.zeros((6, 9, 3)))


def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    n = 6 * 9
    t, f, fm = dev.DeviceBuffer.zeros(n * 3 * 4), dev.DeviceBuffer.zeros(n * 8), dev.DeviceBuffer.zeros(n)
    err, wi = dev.DeviceBuffer.zeros(n * 4 + 4), dev.DeviceBuffer.zeros(n)
    nat.check(lib.ofl_memset(err.ptr, 7, n * 4, None))
    nat.check(lib.ofl_memset(wi.ptr, 7, n, None))

    def call(near=t.ptr, far=t.ptr, elem=nat.EL_F32, layout=nat.TENSOR_NCHW, N=1, C=3, h=6, w=9, flow=f.ptr, fmask=fm.ptr, sign=1,
             metric=nat.PHOTO_L1, eps=F32(1e-3), tau=F32(1), e=err.ptr, within=wi.ptr, quant=nat.QUANT_OPENCV):
        return lib.ofl_photometric_dev(near, far, elem, layout, N, C, h, w, flow, fmask, 1, sign, None, None, metric, eps, tau,
                                       e, None, within, None, quant, None)

    for kw in (dict(near=None), dict(far=None), dict(flow=None), dict(fmask=None), dict(elem=nat.EL_F64), dict(elem=9), dict(layout=2),
               dict(N=0), dict(N=65536), dict(C=0), dict(C=65536), dict(h=0), dict(w=32767), dict(sign=0), dict(metric=3), dict(metric=-1),
               dict(eps=F32(-1)), dict(eps=F32('nan')), dict(eps=F32('inf')), dict(tau=F32(-1)), dict(tau=F32('nan')), dict(tau=F32('inf')),
               dict(e=None, within=None), dict(quant=7), dict(near=t.ptr + 2), dict(flow=f.ptr + 4), dict(e=err.ptr + 2)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_photometric" in nat.last_error(), kw
    dev.sync()
    assert (err.to_host((n * 4,), U8) == 7).all() and (wi.to_host((n,), U8) == 7).all()          # nothing was launched
    assert call(tau=F32('nan'), within=None) == nat.OK              # tau is looked at only when within is asked for
    assert call() == nat.OK
    assert not err.to_host((n,), F32).any() and not wi.to_host((n,), U8).any()                   # empty masks: nothing is covered
