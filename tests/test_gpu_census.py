"""K22 (ofl_census.hip): the census distance of a warp on the device, bit for bit against tests/census_ref.py (the oracle's
gather plus float32 NumPy in the stated order), against K21 on the device itself, and through every layer: the raw ABI,
DeviceFlow.census, DeviceFlowBatch.census, Flow.census and census_error.  Nothing here has a tolerance: masks and counts are
compared with array_equal, distances through their bits (a NaN may carry any payload).  The tile is 64 x 16: (19, 70) and
(37, 131) cross its seams raggedly, (64, 256) is an exact multiple."""
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
import tensor_ref as T
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu
nat = of.native
F32, U8 = np.float32, np.uint8
MODE_CODE = {'hard': nat.CENSUS_HARD, 'soft': nat.CENSUS_SOFT}
EL = {'float32': nat.EL_F32, 'float16': nat.EL_F16, 'bfloat16': nat.EL_BF16}
LAYOUT = {'chw': nat.TENSOR_NCHW, 'hwc': nat.TENSOR_NHWC}
VARIANTS = [('soft', 0.0), ('hard', 0.0), ('hard', 2.0)]          # (mode, delta): see census_ref.case


def up(a):
    a = np.ascontiguousarray(a)
    return dev.DeviceBuffer.from_host(a.view(U8) if a.dtype == np.bool_ else a)


def ptr(x):
    return None if x is None else x.ptr


def raw_call(near, far, dtype, layout, f, fm, sign, K, mode, p0, p1, min_count, tau=None, near_mask=None, far_mask=None,
             quant=nat.QUANT_OPENCV, shared=True, err=True, covered=True, counts=True):
    """ofl_census_dev on host arrays: near, far planar (n, c, h, w) as stored in `dtype`, uploaded in the memory order of
    `layout` -> (err | None, covered | None, within | None, counts | None) on the host, each (n, h, w) / (n, 2)"""
    n, c, h, w = near.shape
    px = n * h * w
    d_near, d_far = up(Cn.in_layout(near, layout)), up(Cn.in_layout(far, layout))
    d_f, d_fm = up(np.ascontiguousarray(f, F32)), up(fm)
    d_nm, d_am = (None if m is None else up(m) for m in (near_mask, far_mask))
    d_err = dev.DeviceBuffer(px * 4) if err else None
    d_cov = dev.DeviceBuffer(px) if covered else None
    d_wi = dev.DeviceBuffer(px) if tau is not None else None
    d_cnt = dev.DeviceBuffer.zeros(n * 8) if counts else None
    nat.check(nat.load().ofl_census_dev(d_near.ptr, d_far.ptr, EL[dtype], LAYOUT[layout], n, c, h, w, d_f.ptr, d_fm.ptr,
                                        1 if shared else 0, sign, ptr(d_nm), ptr(d_am), K, MODE_CODE[mode], F32(p0), F32(p1), min_count,
                                        F32(0 if tau is None else tau), ptr(d_err), ptr(d_cov), ptr(d_wi), ptr(d_cnt), quant, None))
    return (d_err.to_host((n, h, w), F32) if err else None, d_cov.to_host((n, h, w), U8) if covered else None,
            d_wi.to_host((n, h, w), U8) if tau is not None else None, d_cnt.to_host((n, 2), np.uint32) if counts else None)


def check(got, want, what):
    """(err, covered, within, counts) as raw_call gives them against restate()'s dict; None outputs are skipped"""
    err, cov, wi, cnt = got
    if err is not None:
        assert Cn.same_floats(err, want['err']), "{}: err".format(what)
    if cov is not None:
        np.testing.assert_array_equal(cov, want['covered'].astype(U8), err_msg="{}: covered".format(what))
    if wi is not None:
        np.testing.assert_array_equal(wi, want['within'].astype(U8), err_msg="{}: within".format(what))
    if cnt is not None:
        assert [tuple(int(v) for v in row) for row in cnt] == [(a, b if wi is not None else 0) for a, b in want['counts']], what


def run_case(shape, sign, quant, K, variant, layout, dtype, c, n=1, seed=1):
    mode, delta = variant
    k = Cn.case(seed, shape, sign, quant, c, dtype, K, mode, n, delta)
    got = raw_call(k['near'], k['far'], dtype, layout, k['f'], k['fm'], sign, K, mode, k['p0'], k['p1'], k['min_count'], k['tau'], quant=quant)
    check(got, k['want'], (shape, sign, quant, K, variant, layout, dtype, c, n))
    return got


def widened(k, dtype='float32'):
    return R.to_f32(k['near'], dtype), R.to_f32(k['far'], dtype)


# ---------------------------------------------------------------------------------------------- 1: channels x layout x dtype
def rotation(c):
    """the six (dtype, layout) of channel count c with their (sign, quant, K, variant): over the 24 combinations every sign,
    quant, window and variant occurs with every dtype and layout class more than once"""
    out = []
    for i, (dtype, layout) in enumerate(itertools.product(T.DTYPES, T.LAYOUTS)):
        idx = (c - 1) * 6 + i
        out.append((Cn.SIGNS[idx % 2], Cn.QUANTS[(idx // 2) % 2], Cn.WINDOWS[(idx + idx // 6) % 3], VARIANTS[(idx // 2 + idx // 6) % 3], layout, dtype))
    return out


def test_the_rotation_reaches_every_setting():
    seen = [r for c in (1, 2, 3, 4) for r in rotation(c)]
    assert len(seen) == 24
    for col, values in enumerate((Cn.SIGNS, Cn.QUANTS, Cn.WINDOWS, VARIANTS, T.LAYOUTS, T.DTYPES)):
        assert {r[col] for r in seen} == set(values)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_every_channel_count_layout_and_dtype(gpu, c):
    for sign, quant, K, variant, layout, dtype in rotation(c):
        run_case((19, 70), sign, quant, K, variant, layout, dtype, c)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_planar_and_channels_last_give_identical_bytes(gpu, dtype):
    for c, K, variant in ((1, 3, VARIANTS[1]), (3, 7, VARIANTS[0]), (4, 5, VARIANTS[2])):
        a = run_case((19, 70), -1, nat.QUANT_OPENCV, K, variant, 'chw', dtype, c)
        b = run_case((19, 70), -1, nat.QUANT_OPENCV, K, variant, 'hwc', dtype, c)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 2: shapes
# thinned product: at every shape each window, mode, sign, quant, layout and dtype occurs at least once
THIN = [(1, nat.QUANT_OPENCV, 7, VARIANTS[0], 'chw', 'float32', 3), (-1, nat.QUANT_EXACT, 3, VARIANTS[1], 'hwc', 'float16', 1),
        (1, nat.QUANT_EXACT, 5, VARIANTS[2], 'chw', 'bfloat16', 4), (-1, nat.QUANT_OPENCV, 3, VARIANTS[0], 'hwc', 'float32', 2),
        (1, nat.QUANT_OPENCV, 7, VARIANTS[1], 'chw', 'float16', 4), (-1, nat.QUANT_EXACT, 5, VARIANTS[0], 'hwc', 'bfloat16', 3)]


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (5, 7)] + Cn.SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_shapes(gpu, shape):
    for sign, quant, K, variant, layout, dtype, c in THIN:
        run_case(shape, sign, quant, K, variant, layout, dtype, c)


# ---------------------------------------------------------------------------------------------- 3: min_count
@pytest.mark.parametrize("K", Cn.WINDOWS)
@pytest.mark.parametrize("mode", Cn.MODES)
def test_min_count_at_one_at_half_and_at_the_default(gpu, K, mode):
    shape, sign, c = (37, 131), 1, 3
    k = Cn.case(3, shape, sign, nat.QUANT_OPENCV, c, 'float32', K, mode)
    near, far = widened(k)
    sizes = []
    for min_count in (1, (K * K - 1) // 2, K * K - 1):
        want = Cn.restate(near, far, k['f'], k['fm'], sign, K=K, mode=mode, p0=k['p0'], p1=k['p1'], min_count=min_count, tau=k['tau'])
        got = raw_call(k['near'], k['far'], 'float32', 'chw', k['f'], k['fm'], sign, K, mode, k['p0'], k['p1'], min_count, k['tau'])
        check(got, want, (K, mode, min_count))
        sizes.append(int(got[3][0, 0]))
    assert sizes[0] > sizes[1] > sizes[2] > 0
    # the default of the method is the full window
    flow = dev.DeviceFlow.from_host(k['f'], 's', k['fm'])
    near_t, far_t = dev.DeviceTensor.from_host(k['near'][0], 'chw'), dev.DeviceTensor.from_host(k['far'][0], 'chw')
    kw = dict(delta=float(k['p0'])) if mode == 'hard' else {}
    err, cov = flow.census(near_t, far_t, K, mode, **kw)
    check((err.to_host((1,) + shape, F32), cov.to_host((1,) + shape, U8), None, None), want, "default")


def test_a_window_larger_than_the_frame_covers_nothing_at_the_default(gpu):
    shape = (5, 7)
    for mode in Cn.MODES:
        k = Cn.case(1, shape, 1, nat.QUANT_OPENCV, 3, 'float32', 7, mode)
        got = raw_call(k['near'], k['far'], 'float32', 'hwc', k['f'], k['fm'], 1, 7, mode, k['p0'], k['p1'], 48, k['tau'])
        assert not got[1].any() and not got[2].any() and got[0].view(np.uint32).max() == 0 and not got[3].any()
        assert k['want']['covered'].any()                                # with min_count = 1 the same inputs are covered


# ---------------------------------------------------------------------------------------------- 4: batches
@pytest.mark.parametrize("layout, dtype, K, variant", [('chw', 'float32', 7, VARIANTS[0]), ('hwc', 'float16', 5, VARIANTS[2])])
def test_three_items_share_one_field(gpu, layout, dtype, K, variant):
    shape, sign, c = (19, 70), -1, 3
    mode, delta = variant
    k = Cn.case(4, shape, sign, nat.QUANT_OPENCV, c, dtype, K, mode, 3, delta)
    args = (k['f'], k['fm'], sign, K, mode, k['p0'], k['p1'], k['min_count'], k['tau'])
    got = raw_call(k['near'], k['far'], dtype, layout, *args)
    check(got, k['want'], "three items")
    for i in range(3):                                    # each item alone gives the same bytes
        one = raw_call(k['near'][i:i + 1], k['far'][i:i + 1], dtype, layout, *args)
        assert all(a[0].tobytes() == b[i].tobytes() for a, b in zip(one, got))
    # the method: one field serves every item of a batched tensor
    flow = dev.DeviceFlow.from_host(k['f'], 't', k['fm'])
    near_t = dev.DeviceTensor.from_host(Cn.in_layout(k['near'], layout), layout)
    far_t = dev.DeviceTensor.from_host(Cn.in_layout(k['far'], layout), layout)
    kw = dict(delta=delta) if mode == 'hard' else {}
    err, cov, wi, cnt = flow.census(near_t, far_t, K, mode, min_count=k['min_count'], threshold=float(k['tau']), return_counts=True, **kw)
    full = (3,) + shape
    check((err.to_host(full, F32), cov.to_host(full, U8), wi.to_host(full, U8), np.array(cnt, np.uint32)), k['want'], "method")
    assert all(isinstance(v, int) for row in cnt for v in row) and len(cnt) == 3
    assert len(flow.census(near_t, far_t, K, mode)) == 2 and len(flow.census(near_t, far_t, K, mode, threshold=0.1)) == 3


@pytest.mark.parametrize("shape", [(37, 53), (5, 7)], ids=lambda s: "{}x{}".format(*s))
@pytest.mark.parametrize("ref", ['s', 't'])
def test_batch_method_per_item_fields_and_masks_and_field_views(gpu, shape, ref):
    """three different fields with their own masks in a batch of an odd pixel count (flow_shared = 0): the fields 1 and 2
    start at odd mask addresses and, for field 1, on an 8-byte but not 16-byte boundary"""
    h, w = shape
    assert (h * w) % 2 == 1
    sign, c, layout, dtype, K = (1 if ref == 's' else -1), 3, 'hwc', 'float32', 5
    min_count = 1 if shape == (5, 7) else 12
    rng = np.random.default_rng(9)
    fs, fms, nears, fars = [], [], [], []
    for i in range(3):
        f, fm = P.field(rng, shape)
        near, far = Cn.tensors(rng, 1, c, f, sign, dtype, 255.0)
        fs.append(f), fms.append(fm), nears.append(near[0]), fars.append(far[0])
    f, fm, near, far = np.stack(fs), np.stack(fms), np.stack(nears), np.stack(fars)
    nm, am = np.ones((3, h, w), U8), np.ones((3, h, w), U8)
    for i in range(3):
        nm[i, i:h // 2, w // 2:] = 0
        am[i, h // 2:, i:w // 3] = 0
    first = Cn.restate(near, far, f, fm, sign, K=K, min_count=min_count, near_mask=nm, far_mask=am)
    tau = F32(np.median(first['e'][first['covered']]))
    want = Cn.restate(near, far, f, fm, sign, K=K, min_count=min_count, tau=tau, near_mask=nm, far_mask=am)
    assert all(a >= b > 0 for a, b in want['counts'])
    # the raw entry with per-item fields, and each item alone
    p0, p1 = Cn.params('soft')
    got = raw_call(near, far, dtype, layout, f, fm, sign, K, 'soft', p0, p1, min_count, tau, near_mask=nm, far_mask=am, shared=False)
    check(got, want, "raw, per item")
    for i in range(3):
        one = raw_call(near[i:i + 1], far[i:i + 1], dtype, layout, f[i], fm[i], sign, K, 'soft', p0, p1, min_count, tau, near_mask=nm[i], far_mask=am[i])
        assert all(a[0].tobytes() == b[i].tobytes() for a, b in zip(one, got))
    b = DeviceFlowBatch(3, shape, ref)
    v, m = np.ascontiguousarray(f, F32), np.ascontiguousarray(fm).view(U8)
    nat.check(nat.load().ofl_upload(b.vecs.ptr, v.ctypes.data, v.nbytes, None))
    nat.check(nat.load().ofl_upload(b.mask.ptr, m.ctypes.data, m.nbytes, None))
    dev.sync()
    near_t, far_t = dev.DeviceTensor.from_host(Cn.in_layout(near, layout), layout), dev.DeviceTensor.from_host(Cn.in_layout(far, layout), layout)
    d_nm, d_am = up(nm), up(am)
    err, cov, wi, cnt = b.census(near_t, far_t, K, min_count=min_count, threshold=float(tau), near_mask=d_nm, far_mask=d_am, return_counts=True)
    full = (3,) + shape
    check((err.to_host(full, F32), cov.to_host(full, U8), wi.to_host(full, U8), cnt), want, "batch")
    assert cnt.shape == (3, 2) and len(b.census(near_t, far_t, K, min_count=min_count)) == 2
    for i in range(3):                                    # field(i): a view inside the batch, with item i's tensors and masks
        view = b.field(i)
        ni = dev.DeviceTensor.from_host(Cn.in_layout(near[i:i + 1], layout, False), layout)
        fi = dev.DeviceTensor.from_host(Cn.in_layout(far[i:i + 1], layout, False), layout)
        e1, c1, w1 = view.census(ni, fi, K, min_count=min_count, threshold=float(tau), near_mask=d_nm.view(i * h * w, h * w),
                                 far_mask=d_am.view(i * h * w, h * w))
        assert e1.to_host(shape, F32).tobytes() == err.to_host(full, F32)[i].tobytes()
        np.testing.assert_array_equal(c1.to_host(shape, U8), want['covered'][i].astype(U8))
        np.testing.assert_array_equal(w1.to_host(shape, U8), want['within'][i].astype(U8))
    with pytest.raises(ValueError, match="Error computing census distance: a batch of 3 fields"):
        b.census(dev.DeviceTensor.from_host(Cn.in_layout(near[:2], layout), layout), dev.DeviceTensor.from_host(Cn.in_layout(far[:2], layout), layout))


# ---------------------------------------------------------------------------------------------- 5: masks, optional outputs
@pytest.mark.parametrize("layout, variant", [('chw', VARIANTS[0]), ('hwc', VARIANTS[1])])
def test_masks_and_optional_outputs(gpu, layout, variant):
    shape, sign, c, dtype, K = (37, 131), 1, 3, 'float32', 5
    h, w = shape
    mode, delta = variant
    k = Cn.case(5, shape, sign, nat.QUANT_OPENCV, c, dtype, K, mode, 1, delta)
    near, far = widened(k)
    near_hole, far_hole = np.ones(shape, U8), np.ones(shape, U8)
    near_hole[3:9, 100:] = 0
    far_hole[h // 2:3 * h // 4, w // 2:3 * w // 4] = 0
    # every combination of err, covered, within and counts in which err or within is there
    outputs = [o for o in itertools.product([True, False], repeat=4) if o[0] or o[2]]
    assert len(outputs) == 12
    for nm, am in ((near_hole, None), (None, far_hole), (near_hole, far_hole)):
        wants = {wi: Cn.restate(near, far, k['f'], k['fm'], sign, K=K, mode=mode, p0=k['p0'], p1=k['p1'], min_count=k['min_count'],
                                tau=k['tau'] if wi else None, near_mask=nm, far_mask=am) for wi in (True, False)}
        assert wants[True]['covered'].sum() < k['want']['covered'].sum()      # the hole takes pixels away
        for e, cv, wi, cn in outputs:
            got = raw_call(k['near'], k['far'], dtype, layout, k['f'], k['fm'], sign, K, mode, k['p0'], k['p1'], k['min_count'],
                           k['tau'] if wi else None, near_mask=nm, far_mask=am, err=e, covered=cv, counts=cn)
            assert (got[0] is not None, got[1] is not None, got[2] is not None, got[3] is not None) == (e, cv, wi, cn)
            check(got, wants[wi], (layout, nm is not None, am is not None, e, cv, wi, cn))


# ---------------------------------------------------------------------------------------------- 6: known answers
def method(flow, near, far, *a, **kw):
    """DeviceFlow.census on planar host arrays (1, c, h, w) -> host arrays (h, w)"""
    res = flow.census(dev.DeviceTensor.from_host(near[0], 'chw'), dev.DeviceTensor.from_host(far[0], 'chw'), *a, **kw)
    shape = near.shape[2:]
    return tuple(r.to_host(shape, F32 if i == 0 else U8) for i, r in enumerate(res))


@pytest.mark.parametrize("sign", Cn.SIGNS)
def test_a_gain_and_an_offset_cost_nothing(gpu, sign):
    near, far, f, fm = Cn.translation(sign=sign, lo=64)
    near = near * F32(0.5) + F32(16)                                       # exact
    flow = dev.DeviceFlow.from_host(f, 's' if sign > 0 else 't', fm)
    err, cov, wi = method(flow, near, far, 7, 'hard', threshold=0.0)
    assert cov.sum() == (37 - 2 - 6) * (131 - 3 - 6) and err.view(np.uint32).max() == 0 and np.array_equal(wi, cov)
    l1, cov1 = flow.photometric(dev.DeviceTensor.from_host(near[0], 'chw'), dev.DeviceTensor.from_host(far[0], 'chw'))
    assert (l1.to_host((37, 131), F32)[cov != 0] > 10).all()             # K21 reads the same pair as an error everywhere


@pytest.mark.parametrize("sign", Cn.SIGNS)
def test_integer_translation_has_no_distance(gpu, sign):
    near, far, f, fm = Cn.translation(sign=sign)
    flow = dev.DeviceFlow.from_host(f, 's' if sign > 0 else 't', fm)
    for K, mode in itertools.product(Cn.WINDOWS, Cn.MODES):
        err, cov, wi = method(flow, near, far, K, mode, threshold=0.0)
        assert err.view(np.uint32).max() == 0 and np.array_equal(wi, cov)
        assert cov.sum() == (37 - 2 - 2 * (K // 2)) * (131 - 3 - 2 * (K // 2))


@pytest.mark.parametrize("K", Cn.WINDOWS)
def test_one_differing_pixel_reaches_its_window_and_no_further(gpu, K):
    at, r = (18, 60), K // 2
    near, far, f, fm = Cn.reach(at=at)
    want = Cn.restate(near, far, f, fm, 1, K=K, mode='hard', p0=0.0, min_count=1)
    err, cov = method(dev.DeviceFlow.from_host(f, 's', fm), near, far, K, 'hard', min_count=1)
    assert Cn.same_floats(err, want['err'][0]) and np.array_equal(cov, want['covered'][0].astype(U8))
    block = np.zeros((37, 131), bool)
    block[at[0] - r:at[0] + r + 1, at[1] - r:at[1] + r + 1] = True
    assert (err[~block] == 0).all() and err[at] == 1 and (want['n'][0][block] == K * K - 1).all()
    block[at] = False
    assert (err[block] == F32(1) / F32(K * K - 1)).all()


@pytest.mark.parametrize("K, min_count", [(3, 8), (5, 12), (7, 1), (7, 48)])
def test_covered_is_k21s_covered_eroded_by_the_member_count(gpu, K, min_count):
    shape = (37, 131)
    k = Cn.case(3, shape, 1, nat.QUANT_OPENCV, 1, 'float32', K, 'hard')
    flow = dev.DeviceFlow.from_host(k['f'], 's', k['fm'])
    hole = np.ones(shape, U8)
    hole[20:30, 90:120] = 0
    near_t, far_t = dev.DeviceTensor.from_host(k['near'][0], 'chw'), dev.DeviceTensor.from_host(k['far'][0], 'chw')
    _, cov1 = flow.photometric(near_t, far_t, far_mask=up(hole))
    _, cov = flow.census(near_t, far_t, K, 'hard', min_count=min_count, far_mask=up(hole))
    cov1, cov = cov1.to_host((1,) + shape, U8) != 0, cov.to_host((1,) + shape, U8) != 0
    assert not (cov & ~cov1).any() and cov.any()
    np.testing.assert_array_equal(cov, Cn.eroded(cov1, K, min_count))


# ---------------------------------------------------------------------------------------------- 7: non-finite values
@pytest.mark.parametrize("mode", Cn.MODES)
@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_non_finite_tensor_values(gpu, layout, mode):
    """a NaN and an Inf in far and in near: `covered` does not change; a non-finite intensity at a member reaches every pixel
    that has it in its window and no other -- soft: a NaN distance there; hard: a NaN compares false twice, an Inf
    difference has a sign"""
    shape, sign, c, dtype, K = (19, 70), -1, 3, 'float32', 5
    k = Cn.case(7, shape, sign, nat.QUANT_EXACT, c, dtype, K, mode)
    clean = k['want']
    near, far = k['near'].copy(), k['far'].copy()
    cov_px = np.argwhere(clean['covered'][0])
    (y0, x0), (y1, x1) = cov_px[len(cov_px) // 3], cov_px[2 * len(cov_px) // 3]
    near[0, 1, y0, x0], near[0, 2, y1, x1] = np.nan, np.inf
    far[0, 2, shape[0] // 2, shape[1] // 2], far[0, 0, shape[0] // 3, shape[1] // 3] = np.nan, -np.inf
    kw = dict(K=K, mode=mode, p0=k['p0'], p1=k['p1'], min_count=k['min_count'], tau=k['tau'], quant=nat.QUANT_EXACT)
    want = Cn.restate(near, far, k['f'], k['fm'], sign, **kw)
    got = raw_call(near, far, dtype, layout, k['f'], k['fm'], sign, K, mode, k['p0'], k['p1'], k['min_count'], k['tau'], quant=nat.QUANT_EXACT)
    check(got, want, (layout, mode))
    np.testing.assert_array_equal(got[1], clean['covered'].astype(U8))
    changed = got[0].view(np.uint32) != clean['err'].view(np.uint32)
    near_bad = np.zeros(shape, bool)
    near_bad[max(0, y0 - 2):y0 + 3, max(0, x0 - 2):x0 + 3] = near_bad[max(0, y1 - 2):y1 + 3, max(0, x1 - 2):x1 + 3] = True
    assert changed[0][near_bad].any() and changed.sum() < 4 * 4 * 25
    if mode == 'soft':
        assert np.isnan(got[0][0, y0, x0]) and np.isnan(got[0][0, y1, x1]) and not got[2][np.isnan(got[0])].any()
    else:
        assert np.isfinite(got[0]).all()


@pytest.mark.parametrize("mode", Cn.MODES)
@pytest.mark.parametrize("kind", ['random', 'shift'])
def test_non_finite_vectors(gpu, kind, mode):
    """fields with NaN and Inf vectors: the distance is the restatement's, cov1 K21's on the same fields"""
    B, h, w = shape = (1, 19, 70)
    k = NF.case(shape, kind, 'sprinkle')
    c, sign, K = 2, k['sign'], 3
    rng = np.random.default_rng(h + w)
    far = (rng.standard_normal((B, c, h, w)) * 40).astype(F32)
    near = (rng.standard_normal((B, c, h, w)) * 40).astype(F32)
    p0, p1 = Cn.params(mode, 2.0)
    for quant, layout in itertools.product(Cn.QUANTS, T.LAYOUTS):
        want = Cn.restate(near, far, k['fb'], k['mb'], sign, K=K, mode=mode, p0=p0, p1=p1, min_count=3, tau=0.5, far_mask=k['ma'], quant=quant)
        got = raw_call(near, far, 'float32', layout, k['fb'], k['mb'], sign, K, mode, p0, p1, 3, 0.5, far_mask=k['ma'], quant=quant, shared=False)
        check(got, want, (kind, mode, quant, layout))
        assert want['covered'].any()


# ---------------------------------------------------------------------------------------------- 8: every layer
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("variant", VARIANTS[::2])
def test_host_forms_equal_the_device_form(gpu, ref, variant):
    shape, sign, c, K = (37, 131), (1 if ref == 's' else -1), 3, 7
    mode, delta = variant
    k = Cn.case(9, shape, sign, nat.QUANT_OPENCV, c, 'float32', K, mode, 1, delta)
    want, tau = k['want'], float(k['tau'])
    near, far = Cn.in_layout(k['near'], 'hwc', False), Cn.in_layout(k['far'], 'hwc', False)
    kw = dict(window=K, mode=mode, min_count=k['min_count'], threshold=tau)
    if mode == 'hard':
        kw['delta'] = delta
    flow = dev.DeviceFlow.from_host(k['f'], ref, k['fm'])
    # a float32 DeviceImage is an 'hwc' tensor
    d = tuple(r.to_host(shape, F32 if i == 0 else U8) for i, r in enumerate(flow.census(dev.DeviceImage.from_host(near), dev.DeviceImage.from_host(far), **kw)))
    check((d[0][None], d[1][None], d[2][None], None), want, "device")
    h_err, h_cov, h_wi = of.Flow(k['f'], ref, k['fm']).census(near, far, **kw)
    assert h_err.dtype == F32 and h_cov.dtype == h_wi.dtype == np.bool_ and h_err.shape == h_cov.shape == shape
    assert h_err.tobytes() == d[0].tobytes() and h_cov.tobytes() == d[1].tobytes() and h_wi.tobytes() == d[2].tobytes()
    # planar arrays with layout='chw'; one plane as (H, W)
    p_err, p_cov, _ = of.Flow(k['f'], ref, k['fm']).census(k['near'][0], k['far'][0], layout='chw', **kw)
    assert p_err.tobytes() == d[0].tobytes() and p_cov.tobytes() == d[1].tobytes()
    g_err, g_cov, _ = of.Flow(k['f'], ref, k['fm']).census(k['near'][0, 0], k['far'][0, 0], **kw)
    one = Cn.restate(k['near'][:, :1], k['far'][:, :1], k['f'], k['fm'], sign, K=K, mode=mode, p0=k['p0'], p1=k['p1'], min_count=k['min_count'])
    assert Cn.same_floats(g_err, one['err'][0]) and np.array_equal(g_cov, one['covered'][0])
    # arrays in, with and without the mask; the defaults
    a_err, a_cov, a_wi = of.census_error(k['f'], near, far, ref, k['fm'], **kw)
    assert a_err.tobytes() == d[0].tobytes() and a_cov.tobytes() == d[1].tobytes() and a_wi.tobytes() == d[2].tobytes()
    n_err, n_cov = of.census_error(k['f'], near, far, ref)
    full = Cn.restate(k['near'], k['far'], k['f'], np.ones(shape, bool), sign)
    assert Cn.same_floats(n_err, full['err'][0]) and np.array_equal(n_cov, full['covered'][0]) and n_cov.any()


def test_the_raw_host_entry(gpu):
    shape, sign, c, K, dtype = (19, 70), -1, 4, 5, 'float16'
    h, w = shape
    k = Cn.case(6, shape, sign, nat.QUANT_EXACT, c, dtype, K, 'soft', 2)
    for layout in T.LAYOUTS:
        near, far = Cn.in_layout(k['near'], layout), Cn.in_layout(k['far'], layout)
        f, fm = np.ascontiguousarray(k['f'], F32), np.ascontiguousarray(k['fm']).view(U8)
        err, cov, wi, cnt = np.empty((2, h, w), F32), np.empty((2, h, w), U8), np.empty((2, h, w), U8), np.zeros((2, 2), np.uint32)
        nat.check(nat.load().ofl_census(near.ctypes.data, far.ctypes.data, EL[dtype], LAYOUT[layout], 2, c, h, w, f.ctypes.data, fm.ctypes.data,
                                        1, sign, None, None, K, nat.CENSUS_SOFT, k['p0'], k['p1'], k['min_count'], k['tau'],
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
    for kw, ref_kw in ((dict(window=5, mode='soft', min_count=12, threshold=0.3), dict(K=5, mode='soft', min_count=12, tau=0.3)),
                       (dict(window=3, mode='hard', delta=2, min_count=4, threshold=0.25), dict(K=3, mode='hard', p0=2.0, min_count=4, tau=0.25))):
        a = of.census_error(f, img0, img1, 't', fm, **kw)
        b = of.census_error(f, img0.astype(F32), img1.astype(F32), 't', fm, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == 3
        want = Cn.restate(np.moveaxis(img0.astype(F32), -1, 0)[None], planes, f, fm, -1, **ref_kw)
        assert Cn.same_floats(a[0], want['err'][0]) and np.array_equal(a[1], want['covered'][0]) and np.array_equal(a[2], want['within'][0])
        assert 0 < a[2].sum() < a[1].sum()


# ---------------------------------------------------------------------------------------------- 9: errors
def test_method_errors(gpu):
    prefix = "Error computing census distance: "
    f = dev.DeviceFlow.zero((6, 9), 't')
    t = lambda shape, layout='chw', dtype=np.float32: dev.DeviceTensor.from_host(np.zeros(shape, dtype), layout)
    a = t((3, 6, 9))
    with pytest.raises(ValueError, match=prefix + "the tensors need the same shape"):
        f.census(a, t((4, 6, 9)))
    with pytest.raises(TypeError, match=prefix + "the tensors need the same dtype, got float32 and float16"):
        f.census(a, t((3, 6, 9), dtype=np.float16))
    with pytest.raises(ValueError, match=prefix + "the tensors need the same layout, got 'chw' and 'hwc'"):
        f.census(t((6, 6, 6)), dev.DeviceTensor(a.buf, (6, 6, 6), 'float32', 'hwc'))
    with pytest.raises(ValueError, match=prefix + r"tensors and flow need the same height and width, got \(6, 9\) and \(6, 10\)"):
        dev.DeviceFlow.zero((6, 10), 't').census(a, a)
    with pytest.raises(TypeError, match=prefix + "near needs to be a DeviceTensor or a float32 DeviceImage, got ndarray"):
        f.census(np.zeros((3, 6, 9), F32), a)
    with pytest.raises(TypeError, match=prefix + "far as a DeviceImage needs to be float32, got uint8"):
        f.census(a, dev.DeviceImage.from_host(np.zeros((6, 9, 3), np.uint8)))
    with pytest.raises(ValueError, match=prefix + r"the tensors need 1 to 4 channels \(grey, two-plane, RGB, RGBA\), got 5"):
        f.census(t((5, 6, 9)), t((5, 6, 9)))
    with pytest.raises(ValueError, match=prefix + "window must be 3, 5 or 7, got 9"):
        f.census(a, a, window=9)
    with pytest.raises(ValueError, match=prefix + "mode must be 'hard' or 'soft', got 'ssim'"):
        f.census(a, a, mode='ssim')
    with pytest.raises(ValueError, match=prefix + "delta belongs to mode 'hard'"):
        f.census(a, a, delta=1.0)
    with pytest.raises(ValueError, match=prefix + "noise must be finite and positive"):
        f.census(a, a, noise=0)
    with pytest.raises(TypeError, match=prefix + "knee must be a number or None"):
        f.census(a, a, knee=True)
    with pytest.raises(ValueError, match=prefix + r"min_count must be in \[1, 24\] for window 5, got 25"):
        f.census(a, a, 5, min_count=25)
    with pytest.raises(ValueError, match=prefix + "threshold must be finite and not negative"):
        f.census(a, a, threshold=-1)
    with pytest.raises(TypeError, match=prefix + "near_mask needs to be a DeviceBuffer"):
        f.census(a, a, near_mask=np.ones((6, 9), U8))
    with pytest.raises(ValueError, match=prefix + "far_mask needs to hold 54 bytes"):
        f.census(a, a, far_mask=dev.DeviceBuffer(10))
    # the host forms
    h = of.Flow.zero((6, 9), 't')
    with pytest.raises(ValueError, match=prefix + "the arrays need the same shape"):
        h.census(np.zeros((6, 9, 3), F32), np.zeros((6, 9, 4), F32))
    with pytest.raises(TypeError, match=prefix + "the arrays need the same dtype"):
        h.census(np.zeros((6, 9, 3), F32), np.zeros((6, 9, 3), np.float16))
    with pytest.raises(ValueError, match=prefix + "arrays and flow need the same height and width"):
        h.census(np.zeros((6, 8, 3), F32), np.zeros((6, 8, 3), F32))
    with pytest.raises(ValueError, match=prefix + "the tensors need 1 to 4 channels"):
        h.census(np.zeros((6, 9, 5), F32), np.zeros((6, 9, 5), F32))
    with pytest.raises(ValueError, match=prefix + "mode must be"):
        of.census_error(np.zeros((6, 9, 2), F32), np.zeros((6, 9), F32), np.zeros((6, 9), F32), 't', mode='census')
    with pytest.raises(TypeError, match=prefix + "far needs to have dtype float32, float16 or uint8, got float64"):
        h.census(np.zeros((6, 9, 3), F32), np.zeros((6, 9, 3)))
    with pytest.raises(ValueError, match=prefix + "layout must be 'chw' or 'hwc'"):
        h.census(np.zeros((6, 9, 3), F32), np.zeros((6, 9, 3), F32), layout='nhwc')


def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    n = 6 * 9
    t, f, fm = dev.DeviceBuffer.zeros(n * 5 * 4), dev.DeviceBuffer.zeros(n * 8), dev.DeviceBuffer.zeros(n)
    err, wi = dev.DeviceBuffer.zeros(n * 4 + 4), dev.DeviceBuffer.zeros(n)
    nat.check(lib.ofl_memset(err.ptr, 7, n * 4, None))
    nat.check(lib.ofl_memset(wi.ptr, 7, n, None))

    def call(near=t.ptr, far=t.ptr, elem=nat.EL_F32, layout=nat.TENSOR_NCHW, N=1, C=3, h=6, w=9, flow=f.ptr, fmask=fm.ptr, sign=1,
             window=3, mode=nat.CENSUS_SOFT, p0=F32(0.81), p1=F32(0.1), min_count=8, tau=F32(1), e=err.ptr, within=wi.ptr,
             quant=nat.QUANT_OPENCV):
        return lib.ofl_census_dev(near, far, elem, layout, N, C, h, w, flow, fmask, 1, sign, None, None, window, mode, p0, p1, min_count, tau,
                                  e, None, within, None, quant, None)

    hard = dict(mode=nat.CENSUS_HARD, p0=F32(0))
    for kw in (dict(near=None), dict(far=None), dict(flow=None), dict(fmask=None), dict(elem=nat.EL_F64), dict(elem=9), dict(layout=2),
               dict(N=0), dict(N=65536), dict(C=0), dict(C=5), dict(h=0), dict(w=32767), dict(sign=0),
               dict(window=4), dict(window=9), dict(window=1), dict(mode=2), dict(mode=-1),
               dict(min_count=0), dict(min_count=9), dict(window=7, min_count=49),
               dict(hard, p0=F32(-1)), dict(hard, p0=F32('nan')), dict(hard, p0=F32('inf')),
               dict(p0=F32(0)), dict(p0=F32(-0.81)), dict(p0=F32('nan')), dict(p0=F32('inf')),
               dict(p1=F32(0)), dict(p1=F32(-0.1)), dict(p1=F32('nan')), dict(p1=F32('inf')),
               dict(tau=F32(-1)), dict(tau=F32('nan')), dict(tau=F32('inf')),
               dict(e=None, within=None), dict(quant=7), dict(near=t.ptr + 2), dict(far=t.ptr + 1), dict(flow=f.ptr + 4), dict(e=err.ptr + 2)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_census" in nat.last_error(), kw
    dev.sync()
    assert (err.to_host((n * 4,), U8) == 7).all() and (wi.to_host((n,), U8) == 7).all()          # nothing was launched
    assert call(tau=F32('nan'), within=None) == nat.OK              # tau is looked at only when within is asked for
    assert call(**dict(hard, p1=F32('nan'))) == nat.OK              # hard mode does not read p1
    assert call() == nat.OK
    assert not err.to_host((n,), F32).any() and not wi.to_host((n,), U8).any()                   # empty masks: nothing is covered
