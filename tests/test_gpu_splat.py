"""GPU suite of the splat (K20): DeviceFlow.splat / coverage / project, DeviceFlowBatch.splat and the host forms against
the NumPy restatement tests/splat_ref.py, BYTE FOR BYTE -- outputs, weight, valid and counters.  The sums are integers, so
there is no tolerance anywhere in this file."""
import functools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import splat_ref as R

pytestmark = pytest.mark.gpu
F32, U8 = np.float32, np.uint8
SHAPES = [(1, 1), (1, 65), (5, 7), (33, 67), (64, 64)]
NP_DTYPE = {"float32": F32, "float16": np.float16, "bfloat16": np.uint16}


def device_tensor(t, elem, layout, batched):
    """float32 (n, c, h, w) -> (DeviceTensor as stored in `layout`, the exact float32 widening (n, c, h, w))"""
    s, wide = R.as_stored(t, elem)
    mem = R.to_layout(s if batched else s[0], layout)
    return dev.DeviceTensor.from_host(mem, layout, "bfloat16" if elem == "bfloat16" else None), wide


def to_logical(a, layout):
    return a if layout == "chw" else np.moveaxis(a, -1, -3)


def run_single(t, elem, layout, batched, v, m, mode, z=None, **kw):
    """DeviceFlow.splat with everything returned, and the restatement -> (got, want) as lists of arrays"""
    dt, wide = device_tensor(t, elem, layout, batched)
    flow = dev.DeviceFlow.from_host(v, 's', m)
    zb = None if z is None else dev.DeviceBuffer.from_host(np.ascontiguousarray(z, F32))
    out, valid, weight, counters = flow.splat(dt, mode, importance=zb, return_weight=True, return_counters=True, **kw)
    assert (out.shape, out.dtype, out.layout) == (dt.shape, dt.dtype, dt.layout)
    h, w = v.shape[:2]
    got = [to_logical(out.to_host(), layout), valid.to_host((h, w), U8), weight.to_host((h, w), F32), np.array(counters, np.uint32)]
    r = R.splat(wide, v, m, mode, z=z, shared=True, **kw)
    want_out = R.stored(r["out"], elem)
    want = [want_out if batched else want_out[0], r["valid"], r["weight"], r["counters"]]
    return got, want


def same(got, want, tag=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (tag, i, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), "{}: result {} differs from the restatement".format(tag, i)


# the product of element types, layouts, modes, channel counts, item counts and shapes, pruned by pairing: every value of
# every axis occurs, every pair (elem, layout), (mode, elem), (C, layout) occurs, every shape occurs with every mode
GRID = [
    ("float32", "chw", "average", 3, 1, (5, 7)), ("float32", "hwc", "sum", 5, 3, (33, 67)), ("float32", "hwc", "softmax", 1, 1, (1, 65)),
    ("float16", "hwc", "average", 64, 1, (33, 67)), ("float16", "chw", "softmax", 2, 3, (5, 7)), ("float16", "chw", "sum", 64, 1, (1, 1)),
    ("bfloat16", "chw", "sum", 1, 3, (1, 65)), ("bfloat16", "hwc", "average", 2, 1, (64, 64)), ("bfloat16", "hwc", "softmax", 5, 3, (33, 67)),
    ("float32", "chw", "softmax", 64, 1, (64, 64)), ("float16", "hwc", "sum", 3, 3, (64, 64)), ("bfloat16", "chw", "average", 5, 1, (1, 1)),
    ("float32", "hwc", "average", 2, 3, (1, 65)), ("float16", "chw", "average", 1, 1, (33, 67)), ("float32", "chw", "sum", 2, 1, (5, 7)),
    ("bfloat16", "chw", "softmax", 3, 1, (1, 1)), ("float16", "hwc", "softmax", 3, 1, (5, 7)), ("bfloat16", "hwc", "sum", 64, 1, (5, 7)),
]


@pytest.mark.parametrize("elem, layout, mode, c, n, shape", GRID)
def test_splat_equals_the_restatement(elem, layout, mode, c, n, shape):
    seed = c + n
    v, m = (R.smooth_field if c % 2 else R.random_field)(shape, seed)
    z = R.importance(shape, seed, spread=60.0) if mode == "softmax" else None
    t = R.tensor(n, c, shape, seed)
    got, want = run_single(t, elem, layout, n > 1, v, m, mode, z=z, alpha=-0.7 if z is not None else 1.0)
    same(got, want, (elem, layout, mode, c, n, shape))


@pytest.mark.parametrize("mode", R.MODES)
def test_splat_contention_every_source_lands_on_one_fractional_target(mode):
    shape = (64, 64)
    yy, xx = np.meshgrid(np.arange(64, dtype=F32), np.arange(64, dtype=F32), indexing="ij")
    v = np.stack([F32(20.25) - xx, F32(30.5) - yy], -1).astype(F32)
    z = R.importance(shape, 1, spread=10.0) if mode == "softmax" else None
    got, want = run_single(R.tensor(1, 3, shape, 1), "float32", "hwc", False, v, np.ones(shape, U8), mode, z=z)
    same(got, want, mode)
    assert (want[2] != 0).sum() == 4                                     # the four pixels around (20.25, 30.5)


def test_splat_landings_on_integers_touch_one_pixel():
    shape = (33, 67)
    rng = np.random.default_rng(5)
    v = rng.integers(-3, 4, shape + (2,)).astype(F32)
    got, want = run_single(R.tensor(1, 2, shape, 2, integers=True), "float32", "chw", False, v, np.ones(shape, U8), "sum")
    same(got, want)
    assert (np.rint(want[2]) == want[2]).all()                           # every weight is a count of whole landings


def test_splat_half_the_taps_outside():
    shape = (5, 67)
    v, m = R.constant_field(shape, 0.0, 0.0)
    v[:, 0, 0] = -0.5                                                    # column 0 lands at x = -0.5
    v[:, -1, 0] = 0.5                                                    # column W - 1 lands at x = W - 0.5
    got, want = run_single(R.tensor(1, 3, shape, 3), "float16", "hwc", False, v, m, "average")
    same(got, want)
    assert (want[2][:, 0] == 0.5).all() and (want[2][:, -1] == 0.5).all()


def test_splat_everything_outside_the_frame():
    shape = (5, 7)
    v, m = R.constant_field(shape, 100.0, -50.0)
    got, want = run_single(R.tensor(3, 2, shape, 4), "float32", "chw", True, v, m, "average")
    same(got, want)
    assert not got[0].any() and not got[1].any() and not got[2].any() and list(got[3]) == [0, 0]


def test_splat_counters_nonfinite_vectors_masked_sources_nan_importance_and_overflow():
    shape = (5, 7)
    v, m = R.smooth_field(shape, 6)
    m[:] = 1
    m[0, 0] = m[2, 3] = 0
    v[1, 1, 0], v[1, 2, 1], v[3, 3, 0], v[4, 4, 1] = np.nan, np.inf, -np.inf, F32(3e38)
    v[4, 5, 0] = F32(2.0 ** 30)
    z = R.importance(shape, 6)
    z[0, 5], z[0, 6] = np.nan, np.inf
    got, want = run_single(R.tensor(1, 3, shape, 6), "float32", "hwc", False, v, m, "softmax", z=z)
    same(got, want)
    assert got[3][0] == 9 and got[3][1] == 0
    t = R.tensor(1, 2, shape, 7)
    t[0, 0, 2, 2], t[0, 1, 3, 1], t[0, 1, 0, 3] = F32(2.0 ** 23), np.nan, np.inf
    got, want = run_single(t, "float32", "chw", False, *R.constant_field(shape, 0.5, 0.0), "sum", frac_bits=40)
    same(got, want)
    assert got[3][1] == 6                                                # three values, two taps each, dropped


@pytest.mark.parametrize("mode", ["average", "sum"])
def test_splat_float16_integer_translation_comes_back_byte_for_byte(mode):
    shape = (33, 67)
    t16, _ = R.as_stored(R.tensor(1, 5, shape, 8), "float16")
    flow = dev.DeviceFlow.from_host(R.constant_field(shape, -4.0, 2.0)[0], 's')
    out, valid = flow.splat(dev.DeviceTensor.from_host(t16[0], 'chw'), mode)
    got = out.to_host()
    assert got[:, 2:, :-4].tobytes() == t16[0][:, :-2, 4:].tobytes()
    assert not got[:, :2].any() and not got[:, :, -4:].any()
    want = np.zeros(shape, U8)
    want[2:, :-4] = 1
    assert valid.to_host(shape, U8).tobytes() == want.tobytes()


def test_splat_locality_case():
    shape = (33, 67)
    v, m, z = R.locality_case(shape)
    got, want = run_single(R.tensor(1, 3, shape, 9), "float16", "chw", False, v, m, "softmax", z=z)
    same(got, want)
    assert (want[2][2:-2, 2:31] > 0).all()


@pytest.mark.parametrize("kind", ["translation", "rotation"])
def test_project_equals_the_restatement_and_is_a_t_field(kind):
    shape = (33, 67)
    if kind == "translation":
        v, m = R.constant_field(shape, 2.25, -1.5)
    else:
        v = of.Flow.from_transforms([['rotation', 30, 15, 30]], shape, 's').vecs.astype(F32)
        m = np.ones(shape, U8)
    p = dev.DeviceFlow.from_host(v, 's', m).project()
    assert isinstance(p, dev.DeviceFlow) and p.ref == 't' and p.shape == shape
    pv, pm = p.to_host()
    r = R.splat(np.moveaxis(v, -1, 0)[None], v, m, "average")
    assert np.ascontiguousarray(pv).tobytes() == np.ascontiguousarray(np.moveaxis(r["out"][0], 0, -1)).tobytes()
    assert np.asarray(pm).astype(U8).tobytes() == r["valid"].tobytes()


def test_coverage_equals_the_weight_of_splat():
    shape = (33, 67)
    v, m = R.random_field(shape, 11)
    flow = dev.DeviceFlow.from_host(v, 's', m)
    weight, valid = flow.coverage()
    _, valid2, weight2 = flow.splat(dev.DeviceTensor.from_host(R.tensor(1, 3, shape)[0], 'chw'), return_weight=True)
    r = R.splat(np.zeros((1, 0) + shape, F32), v, m, "average")
    assert weight.to_host(shape, F32).tobytes() == weight2.to_host(shape, F32).tobytes() == r["weight"].tobytes()
    assert valid.to_host(shape, U8).tobytes() == valid2.to_host(shape, U8).tobytes() == r["valid"].tobytes()
    z = R.importance(shape, 11)
    ws, vs = flow.coverage(importance=dev.DeviceBuffer.from_host(z), alpha=0.5)
    r = R.splat(np.zeros((1, 0) + shape, F32), v, m, "softmax", z=z, alpha=0.5)
    assert ws.to_host(shape, F32).tobytes() == r["weight"].tobytes() and vs.to_host(shape, U8).tobytes() == r["valid"].tobytes()


@functools.lru_cache(maxsize=None)
def batch_inputs():
    shape, n = (5, 7), 3
    fields = [R.random_field(shape, 20 + i, amp=1.5) for i in range(n)]
    z = np.stack([R.importance(shape, 20 + i) for i in range(n)])
    return shape, n, fields, z, R.tensor(n, 3, shape, 20)


def splat_bytes(res, px):
    """(tensor, valid, weight, counters) of a splat whose valid and weight hold `px` pixels -> host arrays"""
    out, valid, weight, counters = res
    return [out.to_host(), valid.to_host((px,), U8), weight.to_host((px,), F32), np.array(counters, np.uint32)]


@pytest.mark.parametrize("mode", ["average", "softmax"])
def test_batch_splat_equals_the_per_field_calls_and_the_restatement(mode):
    shape, n, fields, z, t = batch_inputs()
    zz = z if mode == "softmax" else None
    batch = DeviceFlowBatch.from_flows([of.Flow(v, 's', m.astype(bool)) for v, m in fields])
    dt, wide = device_tensor(t, "float16", "hwc", True)
    zb = None if zz is None else dev.DeviceBuffer.from_host(zz)
    got = splat_bytes(batch.splat(dt, mode, importance=zb, alpha=0.3, return_weight=True, return_counters=True), n * shape[0] * shape[1])
    r = R.splat(wide, np.stack([f[0] for f in fields]), np.stack([f[1] for f in fields]), mode, z=zz, alpha=0.3, shared=False)
    same(got, [R.to_layout(R.stored(r["out"], "float16"), "hwc"), r["valid"].reshape(-1), r["weight"].reshape(-1), r["counters"]])
    px = shape[0] * shape[1]
    for i in range(n):                                                   # ... and views inside the odd-pixel batch of three
        item = dev.DeviceTensor.from_host(np.ascontiguousarray(R.to_layout(R.stored(t, "float16"), "hwc")[i]), 'hwc')
        zi = None if zz is None else dev.DeviceBuffer.from_host(zz[i])
        kw = dict(importance=zi, alpha=0.3, return_weight=True, return_counters=True)
        view = splat_bytes(batch.field(i).splat(item, mode, **kw), px)
        alone = splat_bytes(dev.DeviceFlow.from_host(fields[i][0], 's', fields[i][1]).splat(item, mode, **kw), px)
        same(view[:3], alone[:3], "field {} as a view".format(i))
        assert view[0].tobytes() == got[0][i].tobytes() and view[1].tobytes() == got[1][i * px:(i + 1) * px].tobytes()
        assert view[2].tobytes() == got[2][i * px:(i + 1) * px].tobytes()
        cw, cv = batch.field(i).coverage(), batch.field(i).project().to_host()
        ca = dev.DeviceFlow.from_host(fields[i][0], 's', fields[i][1])
        assert cw[0].to_host((px,), F32).tobytes() == ca.coverage()[0].to_host((px,), F32).tobytes()
        assert np.ascontiguousarray(cv[0]).tobytes() == np.ascontiguousarray(ca.project().to_host()[0]).tobytes()


def test_splat_two_runs_give_identical_bytes():
    shape = (64, 64)
    v, m = R.random_field(shape, 30, amp=0.4)                            # heavy overlap: many sources per target
    flow = dev.DeviceFlow.from_host(v, 's', m)
    dt, _ = device_tensor(R.tensor(1, 5, shape, 30), "float32", "hwc", False)
    z = dev.DeviceBuffer.from_host(R.importance(shape, 30))
    a = splat_bytes(flow.splat(dt, "softmax", importance=z, return_weight=True, return_counters=True), 64 * 64)
    b = splat_bytes(flow.splat(dt, "softmax", importance=z, return_weight=True, return_counters=True), 64 * 64)
    same(a, b)


def test_splat_host_forms_equal_the_device_forms():
    shape = (5, 7)
    v, m = R.random_field(shape, 40, amp=1.5)
    z = R.importance(shape, 40)
    t = R.tensor(2, 3, shape, 40)
    hf, df = of.Flow(v, 's', m.astype(bool)), dev.DeviceFlow.from_host(v, 's', m)
    out, valid, weight, counters = hf.splat(t, 'softmax', importance=z, alpha=0.5, return_weight=True, return_counters=True)
    d = df.splat(dev.DeviceTensor.from_host(t, 'chw'), 'softmax', importance=dev.DeviceBuffer.from_host(z), alpha=0.5,
                 return_weight=True, return_counters=True)
    assert out.dtype == F32 and out.tobytes() == d[0].to_host().tobytes()
    assert valid.dtype == np.bool_ and valid.view(U8).tobytes() == d[1].to_host(shape, U8).tobytes()
    assert weight.tobytes() == d[2].to_host(shape, F32).tobytes() and counters == d[3]
    thw = np.ascontiguousarray(np.moveaxis(t[0], 0, -1)).astype(np.float16)
    o2, v2 = of.splat_flow(v, thw, m.astype(bool), mode='sum', layout='hwc')
    d2 = df.splat(dev.DeviceTensor.from_host(thw, 'hwc'), 'sum')
    assert o2.dtype == np.float16 and o2.tobytes() == d2[0].to_host().tobytes() and v2.view(U8).tobytes() == d2[1].to_host(shape, U8).tobytes()
    w3, v3 = hf.coverage()
    assert w3.tobytes() == df.coverage()[0].to_host(shape, F32).tobytes()
    p, dp = hf.project(), df.project().to_host()
    assert p.ref == 't' and np.ascontiguousarray(p.vecs, F32).tobytes() == np.ascontiguousarray(dp[0]).tobytes()
    assert np.ascontiguousarray(p.mask).view(U8).tobytes() == np.ascontiguousarray(dp[1]).view(U8).tobytes()


def test_splat_with_a_t_field_raises():
    shape = (5, 7)
    flow = dev.DeviceFlow.from_host(np.zeros(shape + (2,), F32), 't')
    dt = dev.DeviceTensor.from_host(np.zeros((2,) + shape, F32), 'chw')
    for call in (lambda: flow.splat(dt), lambda: flow.coverage(), lambda: flow.project()):
        with pytest.raises(ValueError, match="apply_tensor"):
            call()
    with pytest.raises(ValueError, match="splat"):
        dev.DeviceFlow.from_host(np.ones(shape + (2,), F32), 's').apply_tensor(dt)
