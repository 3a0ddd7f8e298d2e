"""K26 (ofl_ssim.hip): the structural dissimilarity of a warp on the device, bit for bit against tests/ssim_ref.py (the
oracle's gather plus float32 NumPy in the stated order), against K21 on the device itself, and through every layer: the raw
ABI, DeviceFlow.ssim, DeviceFlowBatch.ssim, Flow.ssim and ssim_error.  Nothing here has a tolerance: masks and counts are
compared with array_equal, errors through their bits (a NaN may carry any payload).  The tile is 64 x 16: (19, 70) and
(37, 131) cross its seams raggedly -- with a halo of 5 at window 11 --, (64, 256) is an exact multiple, and the tiny shapes
put the whole frame inside one window."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import census_ref as Cn
import interop_ref as R
import nonfinite_cases as NF
import photometric_ref as P
import ssim_ref as Sm
import tensor_ref as T
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu
nat = of.native
F32, U8 = np.float32, np.uint8
EL = {'float32': nat.EL_F32, 'float16': nat.EL_F16, 'bfloat16': nat.EL_BF16}
LAYOUT = {'chw': nat.TENSOR_NCHW, 'hwc': nat.TENSOR_NHWC}
VARIANTS = [(K, w) for w in Sm.WEIGHTS for K in Sm.WINDOWS]           # (window, weighting)
PREFIX = "Error computing structural similarity: "


def up(a):
    a = np.ascontiguousarray(a)
    return dev.DeviceBuffer.from_host(a.view(U8) if a.dtype == np.bool_ else a)


def ptr(x):
    return None if x is None else x.ptr


def raw_call(near, far, dtype, layout, f, fm, sign, K, g, min_count, tau=None, near_mask=None, far_mask=None, c1=Sm.C1, c2=Sm.C2,
             quant=nat.QUANT_OPENCV, shared=True, err=True, covered=True, counts=True, start=None):
    """ofl_ssim_dev on host arrays: near, far planar (n, c, h, w) as stored in `dtype`, uploaded in the memory order of
    `layout`; start: the (n, 2) uint32 the counts begin at (None: zeros) -> (err | None, covered | None, within | None,
    counts | None) on the host, each (n, h, w) / (n, 2)"""
    n, c, h, w = near.shape
    px = n * h * w
    d_near, d_far = up(Sm.in_layout(near, layout)), up(Sm.in_layout(far, layout))
    d_f, d_fm = up(np.ascontiguousarray(f, F32)), up(fm)
    d_nm, d_am = (None if m is None else up(m) for m in (near_mask, far_mask))
    d_err = dev.DeviceBuffer(px * 4) if err else None
    d_cov = dev.DeviceBuffer(px) if covered else None
    d_wi = dev.DeviceBuffer(px) if tau is not None else None
    d_cnt = (dev.DeviceBuffer.zeros(n * 8) if start is None else up(np.ascontiguousarray(start, np.uint32))) if counts else None
    g = np.ascontiguousarray(g, F32)
    nat.check(nat.load().ofl_ssim_dev(d_near.ptr, d_far.ptr, EL[dtype], LAYOUT[layout], n, c, h, w, d_f.ptr, d_fm.ptr,
                                      1 if shared else 0, sign, ptr(d_nm), ptr(d_am), K, g.ctypes.data, F32(c1), F32(c2), min_count,
                                      F32(0 if tau is None else tau), ptr(d_err), ptr(d_cov), ptr(d_wi), ptr(d_cnt), quant, None))
    return (d_err.to_host((n, h, w), F32) if err else None, d_cov.to_host((n, h, w), U8) if covered else None,
            d_wi.to_host((n, h, w), U8) if tau is not None else None, d_cnt.to_host((n, 2), np.uint32) if counts else None)


def check(got, want, what, start=0):
    """(err, covered, within, counts) as raw_call gives them against restate()'s dict; None outputs are skipped"""
    err, cov, wi, cnt = got
    if err is not None:
        assert Sm.same_floats(err, want['err']), "{}: err".format(what)
    if cov is not None:
        np.testing.assert_array_equal(cov, want['covered'].astype(U8), err_msg="{}: covered".format(what))
    if wi is not None:
        np.testing.assert_array_equal(wi, want['within'].astype(U8), err_msg="{}: within".format(what))
    if cnt is not None:
        assert [tuple(int(v) - start for v in row) for row in cnt] == [(a, b if wi is not None else 0) for a, b in want['counts']], what


def run_case(shape, sign, quant, variant, layout, dtype, c, n=1, seed=1):
    K, weights = variant
    k = Sm.case(seed, shape, sign, quant, c, dtype, K, weights, n)
    got = raw_call(k['near'], k['far'], dtype, layout, k['f'], k['fm'], sign, K, k['g'], k['min_count'], k['tau'], quant=quant)
    check(got, k['want'], (shape, sign, quant, variant, layout, dtype, c, n))
    return got


def widened(k, dtype='float32'):
    return R.to_f32(k['near'], dtype), R.to_f32(k['far'], dtype)


# ---------------------------------------------------------------------------------------------- 1: channels x layout x dtype
def rotation(c):
    """the six (dtype, layout) of channel count c with their (sign, quant, (K, weights)): over the 24 combinations every
    sign, quant, window and weighting occurs with every dtype and with every layout more than once"""
    out = []
    for i, (dtype, layout) in enumerate(itertools.product(T.DTYPES, T.LAYOUTS)):
        idx = (c - 1) * 6 + i
        out.append((Sm.SIGNS[(idx + idx // 6) % 2], Sm.QUANTS[(idx // 2 + idx // 12) % 2], VARIANTS[(idx // 2) % 8], layout, dtype))
    return out


def test_the_rotation_reaches_every_setting():
    seen = [r for c in (1, 2, 3, 4) for r in rotation(c)]
    assert len(seen) == 24 and len(set(seen)) == 24
    flat = [(s, q, K, w, layout, dtype) for s, q, (K, w), layout, dtype in seen]
    for cls_col, classes in ((5, T.DTYPES), (4, T.LAYOUTS)):
        for cls in classes:
            mine = [r for r in flat if r[cls_col] == cls]
            for col, values in enumerate((Sm.SIGNS, Sm.QUANTS, Sm.WINDOWS, Sm.WEIGHTS)):
                for v in values:
                    assert sum(1 for r in mine if r[col] == v) >= 2, (cls, col, v)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_every_channel_count_layout_and_dtype(gpu, c):
    for sign, quant, variant, layout, dtype in rotation(c):
        run_case((19, 70), sign, quant, variant, layout, dtype, c)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_planar_and_channels_last_give_identical_bytes(gpu, dtype):
    for c, variant in ((1, (3, 'uniform')), (3, (11, 'gaussian')), (4, (5, 'gaussian')), (2, (7, 'uniform'))):
        a = run_case((19, 70), -1, nat.QUANT_OPENCV, variant, 'chw', dtype, c)
        b = run_case((19, 70), -1, nat.QUANT_OPENCV, variant, 'hwc', dtype, c)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 2: shapes
# thinned product: at every shape each window -- 11 twice --, weighting, sign, quant, layout and dtype occurs at least once
THIN = [(1, nat.QUANT_OPENCV, (11, 'gaussian'), 'chw', 'float32', 3), (-1, nat.QUANT_EXACT, (3, 'uniform'), 'hwc', 'float16', 1),
        (1, nat.QUANT_EXACT, (5, 'gaussian'), 'chw', 'bfloat16', 4), (-1, nat.QUANT_OPENCV, (7, 'uniform'), 'hwc', 'float32', 2),
        (-1, nat.QUANT_EXACT, (11, 'uniform'), 'hwc', 'float16', 4)]


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (5, 7)] + Sm.SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_shapes(gpu, shape):
    for sign, quant, variant, layout, dtype, c in THIN:
        got = run_case(shape, sign, quant, variant, layout, dtype, c)
        assert shape not in Sm.SHAPES or got[3][0, 0] > 0


# ---------------------------------------------------------------------------------------------- 3: min_count
@pytest.mark.parametrize("K, weights", [(3, 'gaussian'), (5, 'uniform'), (7, 'gaussian'), (11, 'uniform'), (11, 'gaussian')])
def test_min_count_at_one_at_half_and_at_the_default(gpu, K, weights):
    shape, sign, c = (37, 131), 1, 3
    k = Sm.case(3, shape, sign, nat.QUANT_OPENCV, c, 'float32', K, weights)
    near, far = widened(k)
    sizes = []
    for min_count in (1, (K * K + 1) // 2, K * K):
        want = Sm.restate(near, far, k['f'], k['fm'], sign, K=K, g=k['g'], min_count=min_count, tau=k['tau'])
        got = raw_call(k['near'], k['far'], 'float32', 'chw', k['f'], k['fm'], sign, K, k['g'], min_count, k['tau'])
        check(got, want, (K, weights, min_count))
        sizes.append(int(got[3][0, 0]))
    assert sizes[0] > sizes[1] > sizes[2] > 0
    # the default of the method is the full window
    flow = dev.DeviceFlow.from_host(k['f'], 's', k['fm'])
    near_t, far_t = dev.DeviceTensor.from_host(k['near'][0], 'chw'), dev.DeviceTensor.from_host(k['far'][0], 'chw')
    err, cov = flow.ssim(near_t, far_t, K, weights)
    check((err.to_host((1,) + shape, F32), cov.to_host((1,) + shape, U8), None, None), want, "default")


def test_a_window_larger_than_the_frame_covers_nothing_at_the_default(gpu):
    shape = (5, 7)
    k = Sm.case(1, shape, 1, nat.QUANT_OPENCV, 3, 'float32', 11, 'gaussian')
    got = raw_call(k['near'], k['far'], 'float32', 'hwc', k['f'], k['fm'], 1, 11, k['g'], 121, k['tau'])
    assert not got[1].any() and not got[2].any() and got[0].view(np.uint32).max() == 0 and not got[3].any()
    assert k['want']['covered'].any()                                    # with min_count = 1 the same inputs are covered


# ---------------------------------------------------------------------------------------------- 4: masks and batches
@pytest.mark.parametrize("layout, dtype, variant", [('chw', 'float32', (11, 'gaussian')), ('hwc', 'float16', (5, 'uniform'))])
def test_three_items_share_one_field(gpu, layout, dtype, variant):
    shape, sign, c = (19, 70), -1, 3
    K, weights = variant
    k = Sm.case(2, shape, sign, nat.QUANT_OPENCV, c, dtype, K, weights, 3)     # a seed at which every item meets the share conditions
    args = (k['f'], k['fm'], sign, K, k['g'], k['min_count'], k['tau'])
    got = raw_call(k['near'], k['far'], dtype, layout, *args)
    check(got, k['want'], "three items")
    for i in range(3):                                    # each item alone gives the same bytes
        one = raw_call(k['near'][i:i + 1], k['far'][i:i + 1], dtype, layout, *args)
        assert all(a[0].tobytes() == b[i].tobytes() for a, b in zip(one, got))
    # the counts are ADDED to what is there
    start = np.full((3, 2), 1000, np.uint32)
    check(raw_call(k['near'], k['far'], dtype, layout, *args, start=start), k['want'], "counts from 1000", start=1000)
    # the method: one field serves every item of a batched tensor
    flow = dev.DeviceFlow.from_host(k['f'], 't', k['fm'])
    near_t = dev.DeviceTensor.from_host(Sm.in_layout(k['near'], layout), layout)
    far_t = dev.DeviceTensor.from_host(Sm.in_layout(k['far'], layout), layout)
    err, cov, wi, cnt = flow.ssim(near_t, far_t, K, weights, min_count=k['min_count'], threshold=float(k['tau']), return_counts=True)
    full = (3,) + shape
    check((err.to_host(full, F32), cov.to_host(full, U8), wi.to_host(full, U8), np.array(cnt, np.uint32)), k['want'], "method")
    assert all(isinstance(v, int) for row in cnt for v in row) and len(cnt) == 3
    assert len(flow.ssim(near_t, far_t, K, weights)) == 2 and len(flow.ssim(near_t, far_t, K, weights, threshold=0.1)) == 3


@pytest.mark.parametrize("shape", [(37, 53), (5, 7)], ids=lambda s: "{}x{}".format(*s))
@pytest.mark.parametrize("ref", ['s', 't'])
def test_batch_method_per_item_fields_and_masks_and_field_views(gpu, shape, ref):
    """three different fields with their own masks in a batch of an odd pixel count (flow_shared = 0): the fields 1 and 2
    start at odd mask addresses and, for field 1, on an 8-byte but not 16-byte boundary"""
    h, w = shape
    assert (h * w) % 2 == 1
    sign, c, layout, dtype, K = (1 if ref == 's' else -1), 3, 'hwc', 'float32', 11
    min_count = 1 if shape == (5, 7) else 61
    g = Sm.taps(K)
    rng = np.random.default_rng(9)
    fs, fms, nears, fars = [], [], [], []
    for i in range(3):
        f, fm = P.field(rng, shape)
        near, far = Cn.tensors(rng, 1, c, f, sign, dtype, 255.0)
        fs.append(f), fms.append(fm), nears.append(near[0]), fars.append(far[0])
    f, fm, near, far = np.stack(fs), np.stack(fms), np.stack(nears), np.stack(fars)
    nm, am = np.ones((3, h, w), U8), np.ones((3, h, w), U8)
    for i in range(3):
        nm[i, i:h // 2, 3 * w // 4:] = 0
        am[i, 3 * h // 4:, i:w // 3] = 0
    first = Sm.restate(near, far, f, fm, sign, K=K, g=g, min_count=min_count, near_mask=nm, far_mask=am)
    tau = F32(np.median(first['e'][first['covered']]))
    want = Sm.restate(near, far, f, fm, sign, K=K, g=g, min_count=min_count, tau=tau, near_mask=nm, far_mask=am)
    assert all(a >= b > 0 for a, b in want['counts'])
    got = raw_call(near, far, dtype, layout, f, fm, sign, K, g, min_count, tau, near_mask=nm, far_mask=am, shared=False)
    check(got, want, "raw, per item")
    for i in range(3):
        one = raw_call(near[i:i + 1], far[i:i + 1], dtype, layout, f[i], fm[i], sign, K, g, min_count, tau, near_mask=nm[i], far_mask=am[i])
        assert all(a[0].tobytes() == b[i].tobytes() for a, b in zip(one, got))
    b = DeviceFlowBatch(3, shape, ref)
    v, m = np.ascontiguousarray(f, F32), np.ascontiguousarray(fm).view(U8)
    nat.check(nat.load().ofl_upload(b.vecs.ptr, v.ctypes.data, v.nbytes, None))
    nat.check(nat.load().ofl_upload(b.mask.ptr, m.ctypes.data, m.nbytes, None))
    dev.sync()
    near_t, far_t = dev.DeviceTensor.from_host(Sm.in_layout(near, layout), layout), dev.DeviceTensor.from_host(Sm.in_layout(far, layout), layout)
    d_nm, d_am = up(nm), up(am)
    err, cov, wi, cnt = b.ssim(near_t, far_t, min_count=min_count, threshold=float(tau), near_mask=d_nm, far_mask=d_am, return_counts=True)
    full = (3,) + shape
    check((err.to_host(full, F32), cov.to_host(full, U8), wi.to_host(full, U8), cnt), want, "batch")
    assert cnt.shape == (3, 2) and len(b.ssim(near_t, far_t, min_count=min_count)) == 2
    for i in range(3):                                    # field(i): a view inside the batch, with item i's tensors and masks
        view = b.field(i)
        ni = dev.DeviceTensor.from_host(Sm.in_layout(near[i:i + 1], layout, False), layout)
        fi = dev.DeviceTensor.from_host(Sm.in_layout(far[i:i + 1], layout, False), layout)
        e1, c1, w1 = view.ssim(ni, fi, min_count=min_count, threshold=float(tau), near_mask=d_nm.view(i * h * w, h * w),
                               far_mask=d_am.view(i * h * w, h * w))
        assert e1.to_host(shape, F32).tobytes() == err.to_host(full, F32)[i].tobytes()
        np.testing.assert_array_equal(c1.to_host(shape, U8), want['covered'][i].astype(U8))
        np.testing.assert_array_equal(w1.to_host(shape, U8), want['within'][i].astype(U8))
    with pytest.raises(ValueError, match=PREFIX + "a batch of 3 fields"):
        b.ssim(dev.DeviceTensor.from_host(Sm.in_layout(near[:2], layout), layout), dev.DeviceTensor.from_host(Sm.in_layout(far[:2], layout), layout))


@pytest.mark.parametrize("layout, variant", [('chw', (11, 'gaussian')), ('hwc', (7, 'uniform'))])
def test_masks_and_optional_outputs(gpu, layout, variant):
    shape, sign, c, dtype = (37, 131), 1, 3, 'float32'
    h, w = shape
    K, weights = variant
    k = Sm.case(5, shape, sign, nat.QUANT_OPENCV, c, dtype, K, weights)
    near, far = widened(k)
    near_hole, far_hole = np.ones(shape, U8), np.ones(shape, U8)
    near_hole[3:9, 100:] = 0
    far_hole[h // 2:3 * h // 4, w // 2:3 * w // 4] = 0
    # every combination of err, covered, within and counts in which err or within is there: err only and within only among them
    outputs = [o for o in itertools.product([True, False], repeat=4) if o[0] or o[2]]
    assert len(outputs) == 12 and (True, False, False, False) in outputs and (False, False, True, False) in outputs
    for nm, am in ((near_hole, None), (None, far_hole), (near_hole, far_hole)):
        wants = {wi: Sm.restate(near, far, k['f'], k['fm'], sign, K=K, g=k['g'], min_count=k['min_count'],
                                tau=k['tau'] if wi else None, near_mask=nm, far_mask=am) for wi in (True, False)}
        assert wants[True]['covered'].sum() < k['want']['covered'].sum()      # the hole takes pixels away
        for e, cv, wi, cn in outputs:
            got = raw_call(k['near'], k['far'], dtype, layout, k['f'], k['fm'], sign, K, k['g'], k['min_count'],
                           k['tau'] if wi else None, near_mask=nm, far_mask=am, err=e, covered=cv, counts=cn)
            assert (got[0] is not None, got[1] is not None, got[2] is not None, got[3] is not None) == (e, cv, wi, cn)
            check(got, wants[wi], (layout, nm is not None, am is not None, e, cv, wi, cn))


@pytest.mark.parametrize("K, min_count", [(3, 9), (5, 13), (7, 1), (11, 61), (11, 121)])
def test_covered_is_k21s_covered_eroded_with_the_centre_counted(gpu, K, min_count):
    shape = (37, 131)
    k = Sm.case(3, shape, 1, nat.QUANT_OPENCV, 1, 'float32', K, 'uniform')
    flow = dev.DeviceFlow.from_host(k['f'], 's', k['fm'])
    hole = np.ones(shape, U8)
    hole[20:30, 90:120] = 0
    near_t, far_t = dev.DeviceTensor.from_host(k['near'][0], 'chw'), dev.DeviceTensor.from_host(k['far'][0], 'chw')
    _, cov1 = flow.photometric(near_t, far_t, far_mask=up(hole))
    _, cov = flow.ssim(near_t, far_t, K, 'uniform', min_count=min_count, far_mask=up(hole))
    cov1, cov = cov1.to_host((1,) + shape, U8) != 0, cov.to_host((1,) + shape, U8) != 0
    assert not (cov & ~cov1).any() and cov.any()
    np.testing.assert_array_equal(cov, Sm.eroded(cov1, K, min_count))


# ---------------------------------------------------------------------------------------------- 5: non-finite values
@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_non_finite_tensor_values(gpu, layout):
    """a NaN and an Inf in far and in near: `covered` does not change; a non-finite intensity at a member makes the error of
    every covered pixel that has it in its window a NaN, exactly as restated, and a NaN at a pixel that is no member reaches
    nothing"""
    shape, sign, c, dtype, K = (19, 70), -1, 3, 'float32', 5
    k = Sm.case(7, shape, sign, nat.QUANT_EXACT, c, dtype, K, 'gaussian')
    clean = k['want']
    near, far = k['near'].copy(), k['far'].copy()
    cov_px = np.argwhere(clean['covered'][0])
    (y0, x0), (y1, x1) = cov_px[len(cov_px) // 3], cov_px[2 * len(cov_px) // 3]
    hole = np.argwhere(~clean['cov1'][0])[0]                             # no member of any window
    near[0, 1, y0, x0], near[0, 2, y1, x1], near[0, 0, hole[0], hole[1]] = np.nan, np.inf, np.nan
    far[0, 2, shape[0] // 2, shape[1] // 2], far[0, 0, shape[0] // 3, shape[1] // 3] = np.nan, -np.inf
    want = Sm.restate(near, far, k['f'], k['fm'], sign, K=K, g=k['g'], min_count=k['min_count'], tau=k['tau'], quant=nat.QUANT_EXACT)
    got = raw_call(near, far, dtype, layout, k['f'], k['fm'], sign, K, k['g'], k['min_count'], k['tau'], quant=nat.QUANT_EXACT)
    check(got, want, layout)
    np.testing.assert_array_equal(got[1], clean['covered'].astype(U8))
    assert np.isnan(got[0][0, y0, x0]) and np.isnan(got[0][0, y1, x1]) and not got[2][np.isnan(got[0])].any()
    only_near = raw_call(near, k['far'], dtype, layout, k['f'], k['fm'], sign, K, k['g'], k['min_count'], quant=nat.QUANT_EXACT)
    bad = np.isnan(only_near[0][0])
    near_bad = np.zeros(shape, bool)
    near_bad[max(0, y0 - 2):y0 + 3, max(0, x0 - 2):x0 + 3] = near_bad[max(0, y1 - 2):y1 + 3, max(0, x1 - 2):x1 + 3] = True
    np.testing.assert_array_equal(bad, near_bad & clean['covered'][0])   # the hole's NaN reached nothing


@pytest.mark.parametrize("kind", ['random', 'shift'])
def test_non_finite_vectors(gpu, kind):
    """fields with NaN and Inf vectors: the error is the restatement's, cov1 K21's on the same fields"""
    B, h, w = shape = (1, 19, 70)
    k = NF.case(shape, kind, 'sprinkle')
    c, sign, K = 2, k['sign'], 3
    rng = np.random.default_rng(h + w)
    far = (rng.standard_normal((B, c, h, w)) * 40).astype(F32)
    near = (rng.standard_normal((B, c, h, w)) * 40).astype(F32)
    for quant, layout, weights in itertools.product(Sm.QUANTS, T.LAYOUTS, Sm.WEIGHTS):
        g = Sm.taps(K, weights)
        want = Sm.restate(near, far, k['fb'], k['mb'], sign, K=K, g=g, min_count=3, tau=0.5, far_mask=k['ma'], quant=quant)
        got = raw_call(near, far, 'float32', layout, k['fb'], k['mb'], sign, K, g, 3, 0.5, far_mask=k['ma'], quant=quant, shared=False)
        check(got, want, (kind, quant, layout, weights))
        assert want['covered'].any()


# ---------------------------------------------------------------------------------------------- 6: known answers
def method(flow, near, far, *a, **kw):
    """DeviceFlow.ssim on planar host arrays (1, c, h, w) -> host arrays (h, w)"""
    res = flow.ssim(dev.DeviceTensor.from_host(near[0], 'chw'), dev.DeviceTensor.from_host(far[0], 'chw'), *a, **kw)
    shape = near.shape[2:]
    return tuple(r.to_host(shape, F32 if i == 0 else U8) for i, r in enumerate(res))


@pytest.mark.parametrize("sign", Sm.SIGNS)
def test_near_equal_to_the_warped_far_has_no_error(gpu, sign):
    near, far, f, fm = Cn.translation(sign=sign)
    flow = dev.DeviceFlow.from_host(f, 's' if sign > 0 else 't', fm)
    for K, weights in VARIANTS:
        err, cov, wi = method(flow, near, far, K, weights, threshold=0.0)
        assert err.view(np.uint32).max() == 0 and np.array_equal(wi, cov)
        assert cov.sum() == (37 - 2 - 2 * (K // 2)) * (131 - 3 - 2 * (K // 2))
        err, cov = method(flow, near, far, K, weights, min_count=1)
        assert err.view(np.uint32).max() == 0 and cov.sum() == (37 - 2) * (131 - 3)


@pytest.mark.parametrize("c", [1, 4])
def test_two_constant_images_under_a_uniform_window(gpu, c):
    shape, a0, b0 = (19, 70), 100.0, 141.0
    near, far = np.full((1, c) + shape, a0, F32), np.full((1, c) + shape, b0, F32)
    flow = dev.DeviceFlow.from_host(np.zeros(shape + (2,), F32), 't', np.ones(shape, bool))
    want = Sm.constants(a0, b0)
    for K in Sm.WINDOWS:
        err, cov = method(flow, near, far, K, 'uniform', min_count=1)
        assert cov.all() and (err.view(np.uint32) == want.view(np.uint32)).all(), K


@pytest.mark.parametrize("K, weights", [(3, 'uniform'), (7, 'gaussian'), (11, 'gaussian')])
def test_one_differing_pixel_reaches_its_window_and_no_further(gpu, K, weights):
    at, r = (18, 60), K // 2
    near, far, f, fm = Cn.translation()
    near = near.copy()
    near[0, :, at[0], at[1]] = 1000.0
    want = Sm.restate(near, far, f, fm, 1, K=K, g=Sm.taps(K, weights), min_count=1)
    err, cov = method(dev.DeviceFlow.from_host(f, 's', fm), near, far, K, weights, min_count=1)
    assert Sm.same_floats(err, want['err'][0]) and np.array_equal(cov, want['covered'][0].astype(U8))
    block = np.zeros((37, 131), bool)
    block[at[0] - r:at[0] + r + 1, at[1] - r:at[1] + r + 1] = True
    assert (err[~block].view(np.uint32) == 0).all() and (err[block] > 0).all()


# ---------------------------------------------------------------------------------------------- 7: every layer
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("variant", [(11, 'gaussian'), (5, 'uniform')])
def test_host_forms_equal_the_device_form(gpu, ref, variant):
    shape, sign, c = (37, 131), (1 if ref == 's' else -1), 3
    K, weights = variant
    k = Sm.case(9, shape, sign, nat.QUANT_OPENCV, c, 'float32', K, weights)
    want, tau = k['want'], float(k['tau'])
    near, far = Sm.in_layout(k['near'], 'hwc', False), Sm.in_layout(k['far'], 'hwc', False)
    kw = dict(window=K, weights=weights, min_count=k['min_count'], threshold=tau)
    flow = dev.DeviceFlow.from_host(k['f'], ref, k['fm'])
    # a float32 DeviceImage is an 'hwc' tensor
    d = tuple(r.to_host(shape, F32 if i == 0 else U8) for i, r in enumerate(flow.ssim(dev.DeviceImage.from_host(near), dev.DeviceImage.from_host(far), **kw)))
    check((d[0][None], d[1][None], d[2][None], None), want, "device")
    t = tuple(r.to_host(shape, F32 if i == 0 else U8) for i, r in enumerate(
        flow.ssim(dev.DeviceTensor.from_host(k['near'][0], 'chw'), dev.DeviceTensor.from_host(k['far'][0], 'chw'), **kw)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(t, d))
    h_err, h_cov, h_wi = of.Flow(k['f'], ref, k['fm']).ssim(near, far, **kw)
    assert h_err.dtype == F32 and h_cov.dtype == h_wi.dtype == np.bool_ and h_err.shape == h_cov.shape == shape
    assert h_err.tobytes() == d[0].tobytes() and h_cov.tobytes() == d[1].tobytes() and h_wi.tobytes() == d[2].tobytes()
    # planar arrays with layout='chw'; one plane as (H, W)
    p_err, p_cov, _ = of.Flow(k['f'], ref, k['fm']).ssim(k['near'][0], k['far'][0], layout='chw', **kw)
    assert p_err.tobytes() == d[0].tobytes() and p_cov.tobytes() == d[1].tobytes()
    g_err, g_cov, _ = of.Flow(k['f'], ref, k['fm']).ssim(k['near'][0, 0], k['far'][0, 0], **kw)
    one = Sm.restate(k['near'][:, :1], k['far'][:, :1], k['f'], k['fm'], sign, K=K, g=k['g'], min_count=k['min_count'])
    assert Sm.same_floats(g_err, one['err'][0]) and np.array_equal(g_cov, one['covered'][0])
    # arrays in, with and without the mask; the defaults: Wang's 11 x 11 Gaussian window, the full window required
    a_err, a_cov, a_wi = of.ssim_error(k['f'], near, far, ref, k['fm'], **kw)
    assert a_err.tobytes() == d[0].tobytes() and a_cov.tobytes() == d[1].tobytes() and a_wi.tobytes() == d[2].tobytes()
    n_err, n_cov = of.ssim_error(k['f'], near, far, ref)
    full = Sm.restate(k['near'], k['far'], k['f'], np.ones(shape, bool), sign)
    assert Sm.same_floats(n_err, full['err'][0]) and np.array_equal(n_cov, full['covered'][0]) and n_cov.any()


def test_the_raw_host_entry(gpu):
    shape, sign, c, K, dtype = (19, 70), -1, 4, 11, 'float16'
    h, w = shape
    k = Sm.case(6, shape, sign, nat.QUANT_EXACT, c, dtype, K, 'gaussian', 2)
    for layout in T.LAYOUTS:
        near, far = Sm.in_layout(k['near'], layout), Sm.in_layout(k['far'], layout)
        f, fm = np.ascontiguousarray(k['f'], F32), np.ascontiguousarray(k['fm']).view(U8)
        err, cov, wi, cnt = np.empty((2, h, w), F32), np.empty((2, h, w), U8), np.empty((2, h, w), U8), np.zeros((2, 2), np.uint32)
        nat.check(nat.load().ofl_ssim(near.ctypes.data, far.ctypes.data, EL[dtype], LAYOUT[layout], 2, c, h, w, f.ctypes.data, fm.ctypes.data,
                                      1, sign, None, None, K, k['g'].ctypes.data, k['c1'], k['c2'], k['min_count'], k['tau'],
                                      err.ctypes.data, cov.ctypes.data, wi.ctypes.data, cnt.ctypes.data, nat.QUANT_EXACT))
        check((err, cov, wi, cnt), k['want'], layout)


def test_uint8_images_equal_their_float32_conversion(gpu):
    shape = (19, 70)
    rng = np.random.default_rng(3)
    img1 = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    f, fm = P.field(rng, shape)
    planes = np.moveaxis(img1.astype(F32), -1, 0)[None]
    img0 = np.stack([O.gather_bilinear(np.ascontiguousarray(planes[0, i]), f, -1, quant=O.QUANT_EXACT) for i in range(3)], axis=-1)
    img0 = np.clip(np.rint(img0 + rng.uniform(-12, 12, img0.shape)), 0, 255).astype(np.uint8)
    for kw, ref_kw in ((dict(window=5, weights='gaussian', sigma=1.0, min_count=13, threshold=0.006), dict(K=5, g=Sm.taps(5, 'gaussian', 1.0), min_count=13, tau=0.006)),
                       (dict(window=3, weights='uniform', data_range=1.0, k1=2.55, k2=7.65, min_count=4, threshold=0.006),
                        dict(K=3, g=Sm.taps(3, 'uniform'), c1=F32(2.55 ** 2), c2=F32(7.65 ** 2), min_count=4, tau=0.006))):
        a = of.ssim_error(f, img0, img1, 't', fm, **kw)
        b = of.ssim_error(f, img0.astype(F32), img1.astype(F32), 't', fm, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == 3
        want = Sm.restate(np.moveaxis(img0.astype(F32), -1, 0)[None], planes, f, fm, -1, **ref_kw)
        assert Sm.same_floats(a[0], want['err'][0]) and np.array_equal(a[1], want['covered'][0]) and np.array_equal(a[2], want['within'][0])
        assert 0 < a[2].sum() < a[1].sum()


# ---------------------------------------------------------------------------------------------- 8: errors
def test_method_errors(gpu):
    f = dev.DeviceFlow.zero((6, 9), 't')
    t = lambda shape, layout='chw', dtype=np.float32: dev.DeviceTensor.from_host(np.zeros(shape, dtype), layout)
    a = t((3, 6, 9))
    with pytest.raises(ValueError, match=PREFIX + "the tensors need the same shape"):
        f.ssim(a, t((4, 6, 9)))
    with pytest.raises(TypeError, match=PREFIX + "the tensors need the same dtype, got float32 and float16"):
        f.ssim(a, t((3, 6, 9), dtype=np.float16))
    with pytest.raises(ValueError, match=PREFIX + "the tensors need the same layout, got 'chw' and 'hwc'"):
        f.ssim(t((6, 6, 6)), dev.DeviceTensor(a.buf, (6, 6, 6), 'float32', 'hwc'))
    with pytest.raises(ValueError, match=PREFIX + r"tensors and flow need the same height and width, got \(6, 9\) and \(6, 10\)"):
        dev.DeviceFlow.zero((6, 10), 't').ssim(a, a)
    with pytest.raises(TypeError, match=PREFIX + "near needs to be a DeviceTensor or a float32 DeviceImage, got ndarray"):
        f.ssim(np.zeros((3, 6, 9), F32), a)
    with pytest.raises(TypeError, match=PREFIX + "far as a DeviceImage needs to be float32, got uint8"):
        f.ssim(a, dev.DeviceImage.from_host(np.zeros((6, 9, 3), np.uint8)))
    with pytest.raises(ValueError, match=PREFIX + r"the tensors need 1 to 4 channels \(grey, two-plane, RGB, RGBA\), got 5"):
        f.ssim(t((5, 6, 9)), t((5, 6, 9)))
    with pytest.raises(ValueError, match=PREFIX + "window must be 3, 5, 7 or 11, got 9"):
        f.ssim(a, a, window=9)
    with pytest.raises(ValueError, match=PREFIX + "weights must be 'gaussian' or 'uniform', got 'hann'"):
        f.ssim(a, a, weights='hann')
    with pytest.raises(ValueError, match=PREFIX + "sigma belongs to weights 'gaussian'"):
        f.ssim(a, a, weights='uniform', sigma=1.5)
    with pytest.raises(ValueError, match=PREFIX + "k1 must be finite and positive"):
        f.ssim(a, a, k1=0)
    with pytest.raises(TypeError, match=PREFIX + "data_range must be a number"):
        f.ssim(a, a, data_range=True)
    with pytest.raises(ValueError, match=PREFIX + r"min_count must be in \[1, 25\] for window 5, got 26"):
        f.ssim(a, a, 5, min_count=26)
    with pytest.raises(ValueError, match=PREFIX + "threshold must be finite and not negative"):
        f.ssim(a, a, threshold=-1)
    with pytest.raises(TypeError, match=PREFIX + "near_mask needs to be a DeviceBuffer"):
        f.ssim(a, a, near_mask=np.ones((6, 9), U8))
    with pytest.raises(ValueError, match=PREFIX + "far_mask needs to hold 54 bytes"):
        f.ssim(a, a, far_mask=dev.DeviceBuffer(10))


def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    n = 6 * 9
    t, f, fm = dev.DeviceBuffer.zeros(n * 5 * 4), dev.DeviceBuffer.zeros(n * 8), dev.DeviceBuffer.zeros(n)
    err, wi = dev.DeviceBuffer.zeros(n * 4 + 4), dev.DeviceBuffer.zeros(n)
    nat.check(lib.ofl_memset(err.ptr, 7, n * 4, None))
    nat.check(lib.ofl_memset(wi.ptr, 7, n, None))
    good = np.ones(11, F32)

    def taps_with(i, v):
        g = good.copy()
        g[i] = v
        return g

    def call(near=t.ptr, far=t.ptr, elem=nat.EL_F32, layout=nat.TENSOR_NCHW, N=1, C=3, h=6, w=9, flow=f.ptr, fmask=fm.ptr, sign=1,
             window=3, taps=good, c1=Sm.C1, c2=Sm.C2, min_count=9, tau=F32(1), e=err.ptr, within=wi.ptr, quant=nat.QUANT_OPENCV):
        return lib.ofl_ssim_dev(near, far, elem, layout, N, C, h, w, flow, fmask, 1, sign, None, None, window,
                                None if taps is None else taps.ctypes.data, F32(c1), F32(c2), min_count, tau, e, None, within, None, quant, None)

    texts = [
        (dict(near=None), "ofl_ssim: NULL pointer (near, far, flow and fmask are required)"),
        (dict(fmask=None), "ofl_ssim: NULL pointer (near, far, flow and fmask are required)"),
        (dict(window=9), "ofl_ssim: window must be 3, 5, 7 or 11, got 9"),
        (dict(window=4), "ofl_ssim: window must be 3, 5, 7 or 11, got 4"),
        (dict(window=13), "ofl_ssim: window must be 3, 5, 7 or 11, got 13"),
        (dict(taps=None), "ofl_ssim: taps must not be NULL (a host pointer to 3 float32 values)"),
        (dict(taps=taps_with(2, 0.0)), "ofl_ssim: taps[2] must be finite and positive (got 0)"),
        (dict(taps=taps_with(0, -1.0)), "ofl_ssim: taps[0] must be finite and positive (got -1)"),
        (dict(taps=taps_with(1, np.nan)), "ofl_ssim: taps[1] must be finite and positive (got nan)"),
        (dict(window=11, min_count=121, taps=taps_with(10, np.inf)), "ofl_ssim: taps[10] must be finite and positive (got inf)"),
        (dict(c1=0.0), "ofl_ssim: c1 must be finite and positive (got 0)"),
        (dict(c1=np.nan), "ofl_ssim: c1 must be finite and positive (got nan)"),
        (dict(c2=-1.0), "ofl_ssim: c2 must be finite and positive (got -1)"),
        (dict(c2=np.inf), "ofl_ssim: c2 must be finite and positive (got inf)"),
        (dict(min_count=0), "ofl_ssim: min_count must be in [1, 9], got 0"),
        (dict(min_count=10), "ofl_ssim: min_count must be in [1, 9], got 10"),
        (dict(window=11, min_count=122), "ofl_ssim: min_count must be in [1, 121], got 122"),
        (dict(e=None, within=None), "ofl_ssim: one of err and within is required"),
        (dict(tau=F32(-1)), "ofl_ssim: tau must be finite and not negative (got -1)"),
        (dict(tau=F32('nan')), "ofl_ssim: tau must be finite and not negative (got nan)"),
        (dict(near=t.ptr + 2), "ofl_ssim: near and far must be aligned to the element size"),
        (dict(flow=f.ptr + 4), "ofl_ssim: flow must be 8-byte aligned"),
        (dict(e=err.ptr + 2), "ofl_ssim: err and counts must be 4-byte aligned"),
    ]
    for kw, text in texts:
        assert call(**kw) == nat.E_INVALID, kw
        assert nat.last_error() == text, kw
    for kw in (dict(far=None), dict(flow=None), dict(elem=nat.EL_F64), dict(layout=2), dict(N=0), dict(N=65536), dict(C=0), dict(C=5),
               dict(h=0), dict(w=32767), dict(sign=0), dict(window=1), dict(tau=F32('inf')), dict(quant=7), dict(far=t.ptr + 1)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_ssim" in nat.last_error(), kw
    dev.sync()
    assert (err.to_host((n * 4,), U8) == 7).all() and (wi.to_host((n,), U8) == 7).all()          # nothing was launched
    assert call(tau=F32('nan'), within=None) == nat.OK              # tau is looked at only when within is asked for
    assert call(taps=taps_with(3, np.nan)) == nat.OK                # window 3 reads three taps
    assert call() == nat.OK
    assert not err.to_host((n,), F32).any() and not wi.to_host((n,), U8).any()                   # empty masks: nothing is covered


def test_shared_arguments_are_refused_in_the_words_of_census(gpu):
    """one invalid shared argument at a time: the code and the text are check_pair_args' / check_pair_alignment's, as
    ofl_census gives them, with the name exchanged -- at both entries of both families"""
    lib = nat.load()
    px = 8 * 8
    bufs = [dev.DeviceBuffer.zeros(b) for b in (px * 3 * 4 + 8, px * 8, px, px * 4, px)]
    hosts = [np.zeros(b, U8) for b in (px * 3 * 4 + 8, px * 8, px, px * 4, px)]
    g = np.ones(3, F32)
    good = dict(elem=nat.EL_F32, layout=nat.TENSOR_NCHW, N=1, C=3, H=8, W=8, sign=1, quant=nat.QUANT_OPENCV)

    def both(on_device, near_offset=0, **change):
        a = dict(good, **change)
        t, fl, fm, out, o1 = (b.ptr for b in bufs) if on_device else (x.ctypes.data for x in hosts)
        tail = (None,) if on_device else ()
        head = (t + near_offset, t, a['elem'], a['layout'], a['N'], a['C'], a['H'], a['W'], fl, fm, 1, a['sign'], None, None)
        rc_s = getattr(lib, "ofl_ssim_dev" if on_device else "ofl_ssim")(*head, 3, g.ctypes.data, Sm.C1, Sm.C2, 9, F32(0), out, o1, None, None, a['quant'], *tail)
        text_s = nat.last_error()
        rc_c = getattr(lib, "ofl_census_dev" if on_device else "ofl_census")(*head, 3, nat.CENSUS_HARD, F32(0), F32(0), 8, F32(0), out, o1, None, None, a['quant'], *tail)
        return rc_s, text_s, rc_c, nat.last_error()

    for on_device in (True, False):
        for change in (dict(elem=7), dict(layout=5), dict(N=0), dict(C=0), dict(C=5), dict(H=0), dict(sign=0), dict(quant=2)):
            rc_s, text_s, rc_c, text_c = both(on_device, **change)
            assert rc_s == rc_c == nat.E_INVALID and text_s.startswith("ofl_ssim: "), (on_device, change)
            assert text_s == text_c.replace("ofl_census", "ofl_ssim"), (on_device, change, text_s, text_c)
    rc_s, text_s, rc_c, text_c = both(True, near_offset=1)
    assert rc_s == rc_c == nat.E_INVALID and text_s == "ofl_ssim: near and far must be aligned to the element size" == text_c.replace("ofl_census", "ofl_ssim")
    assert both(True)[::2] == (nat.OK, nat.OK) and both(False)[::2] == (nat.OK, nat.OK)
