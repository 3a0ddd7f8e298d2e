"""Fields, images and points of another framework in and out over the CUDA Array Interface (K11, ofl_interop.hip), bit for
bit against the NumPy restatement tests/interop_ref.py entered through DeviceFlow.from_host.  Foreign memory needs no
framework: it is a DeviceBuffer behind a small object that exposes `__cuda_array_interface__` with NumPy's own byte strides.
Nothing here has a tolerance."""
import ctypes
import gc
import weakref

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import interop_ref as R

pytestmark = pytest.mark.gpu
nat = of.native


class Foreign:
    """`view` (a view of the C-contiguous `parent`, or the parent itself) as device memory of "another framework" """

    def __init__(self, view, parent=None, version=3, stream=None):
        parent = view if parent is None else parent
        assert parent.flags.c_contiguous
        self.buf = dev.DeviceBuffer.from_host(parent)
        offset = view.__array_interface__['data'][0] - parent.__array_interface__['data'][0]
        assert 0 <= offset < max(parent.nbytes, 1)
        self.__cuda_array_interface__ = R.cai_dict(view, self.buf.ptr + offset, version, stream)


def expect(vecs, mask=None):
    """what DeviceFlow.from_host makes of the restated import"""
    return dev.DeviceFlow.from_host(vecs, 't', mask).to_host()


def same(dflow, vecs, mask=None):
    v, m = dflow.to_host()
    wv, wm = expect(vecs, mask)
    assert dflow.shape == vecs.shape[:2] and v.shape == wv.shape
    assert np.array_equal(R.bits(v), R.bits(wv)), "vector bits differ"
    assert np.array_equal(m.view(np.uint8), wm.view(np.uint8)), "mask bytes differ"


def same_batch(batch, vecs, masks=None):
    n, h, w = vecs.shape[:3]
    assert (batch.n, batch.shape) == (n, (h, w))
    v = batch.vecs.to_host((n, h, w, 2), np.float32)
    m = batch.mask.to_host((n, h, w), np.uint8)
    assert np.array_equal(R.bits(v), R.bits(vecs)), "vector bits differ"
    assert np.array_equal(m, np.ones((n, h, w), np.uint8) if masks is None else (masks != 0).astype(np.uint8)), "mask bytes differ"


def source(shape, layout, dtype, seed=0):
    """a source array of the flow `shape` (..., H, W) in `layout` -> (array as the producer holds it, dtype= argument)"""
    full = shape + (2,) if layout == 'hwc' else shape[:-2] + (2,) + shape[-2:]
    return R.flow_values(full, dtype, seed), ('bfloat16' if dtype == 'bfloat16' else None)


# ---------------------------------------------------------------------------------------------- import
@pytest.mark.parametrize("dtype", R.FLOW_DTYPES)
@pytest.mark.parametrize("layout", ['hwc', 'chw'])
def test_import_every_layout_and_dtype(gpu, layout, dtype):
    for shape in R.SHAPES:
        arr, dt = source(shape, layout, dtype)
        got = dev.DeviceFlow.from_external(Foreign(arr), 's', layout=layout, dtype=dt)
        assert got.ref == 's'
        same(got, R.import_flow(arr, layout, dtype))
        if shape[0] != 2 and shape[1] != 2:
            same(dev.DeviceFlow.from_external(Foreign(arr, version=2), dtype=dt), R.import_flow(arr, layout, dtype))    # inferred
        arr, dt = source((3,) + shape, layout, dtype, seed=1)
        same_batch(DeviceFlowBatch.from_external(Foreign(arr), 't', layout=layout, dtype=dt), R.import_flow(arr, layout, dtype))


@pytest.mark.parametrize("dtype", R.FLOW_DTYPES)
def test_import_strided_views(gpu, dtype):
    for h, w in [(5, 7), (3, 130)]:
        # rows 1:H+1 and columns 3::2 of a larger parent, both layouts
        parent = R.flow_values((h + 2, 2 * w + 4, 2), dtype, seed=2)
        view = parent[1:h + 1, 3:3 + 2 * w:2]
        assert view.shape == (h, w, 2)
        dt = 'bfloat16' if dtype == 'bfloat16' else None
        same(dev.DeviceFlow.from_external(Foreign(view, parent), dtype=dt), R.import_flow(view, 'hwc', dtype))
        parent = R.flow_values((2, h + 2, 2 * w + 4), dtype, seed=3)
        view = parent[:, 1:h + 1, 3:3 + 2 * w:2]
        same(dev.DeviceFlow.from_external(Foreign(view, parent), dtype=dt), R.import_flow(view, 'chw', dtype))
        # the first two of three interleaved channels
        parent = R.flow_values((h, w, 3), dtype, seed=4)
        view = parent[..., :2]
        same(dev.DeviceFlow.from_external(Foreign(view, parent), dtype=dt), R.import_flow(view, 'hwc', dtype))
        # one field broadcast to a batch of three (field stride 0), and one row broadcast to a field (row stride 0)
        field = R.flow_values((h, w, 2), dtype, seed=5)
        view = np.broadcast_to(field, (3, h, w, 2))
        same_batch(DeviceFlowBatch.from_external(Foreign(view, field), 't', dtype=dt), R.import_flow(view, 'hwc', dtype))
        row = R.flow_values((2, 1, w), dtype, seed=6)
        view = np.broadcast_to(row, (2, h, w))
        same(dev.DeviceFlow.from_external(Foreign(view, row), layout='chw', dtype=dt), R.import_flow(view, 'chw', dtype))


@pytest.mark.parametrize("dtype", R.FLOW_DTYPES)
def test_import_one_element_off_alignment(gpu, dtype):
    """the wide loads are decided per address: a base one element off the wide grid takes the scalar path and is correct"""
    dt = 'bfloat16' if dtype == 'bfloat16' else None
    for h, w in [(5, 8), (3, 130)]:
        for layout, full in (('hwc', (h, w, 2)), ('chw', (2, h, w))):
            parent = R.flow_values((h * w * 2 + 1,), dtype, seed=7)
            view = parent[1:].reshape(full)
            same(dev.DeviceFlow.from_external(Foreign(view, parent), layout=layout, dtype=dt), R.import_flow(view, layout, dtype))


def test_import_masks(gpu):
    rng = np.random.default_rng(8)
    for h, w in [(1, 5), (5, 7), (3, 130), (2, 1030)]:
        arr, _ = source((h, w), 'chw', 'float16')
        want = R.import_flow(arr, 'chw', 'float16')
        mb = rng.random((h, w)) > 0.4
        for mask in (mb, mb.astype(np.uint8)):                                       # |b1 and |u1
            same(dev.DeviceFlow.from_external(Foreign(arr), mask=Foreign(mask)), want, mb)
        parent = (rng.random((h + 1, 2 * w + 3)) > 0.4).astype(np.uint8)            # a strided external mask
        view = parent[1:, 3:3 + 2 * w:2]
        same(dev.DeviceFlow.from_external(Foreign(arr), mask=Foreign(view, parent)), want, view)
        same(dev.DeviceFlow.from_external(Foreign(arr), mask=mb), want, mb)          # what the other constructors take
        same(dev.DeviceFlow.from_external(Foreign(arr), mask=dev.DeviceBuffer.from_host(mb.view(np.uint8))), want, mb)
        same(dev.DeviceFlow.from_external(Foreign(arr)), want)                       # none: all valid
        two = mb.astype(np.uint8)
        two[-1, -1] = 2
        with pytest.raises(ValueError, match="Values must be 0 or 1"):
            dev.DeviceFlow.from_external(Foreign(arr), mask=Foreign(two))
        # unchecked, any non-zero byte counts as valid
        same(dev.DeviceFlow.from_external(Foreign(arr), mask=Foreign(two), check_finite=False), want, two != 0)
    arr, _ = source((3, 5, 7), 'hwc', 'float32')
    masks = rng.random((3, 5, 7)) > 0.4
    same_batch(DeviceFlowBatch.from_external(Foreign(arr), 't', masks=Foreign(masks)), R.import_flow(arr, 'hwc', 'float32'), masks)
    with pytest.raises(ValueError, match="different shape"):
        dev.DeviceFlow.from_external(Foreign(arr[0]), mask=Foreign(masks[0, :4]))
    with pytest.raises(TypeError):
        dev.DeviceFlow.from_external(Foreign(arr[0]), mask=Foreign(masks[0].astype(np.int16)))


@pytest.mark.parametrize("dtype", R.FLOW_DTYPES)
def test_import_finds_one_nan(gpu, dtype):
    nan = np.uint16(0x7fc0) if dtype == 'bfloat16' else np.nan
    dt = 'bfloat16' if dtype == 'bfloat16' else None
    arr, _ = source((3, 5, 7), 'chw', dtype)
    arr[-1, -1, -1, -1] = nan                                                        # the last pixel of the last field
    with pytest.raises(ValueError, match="contains NaN or Inf"):
        DeviceFlowBatch.from_external(Foreign(arr), 't', dtype=dt)
    b = DeviceFlowBatch.from_external(Foreign(arr), 't', dtype=dt, check_finite=False)          # unchecked: does not raise
    v = b.vecs.to_host((3, 5, 7, 2), np.float32)
    assert np.isnan(v[-1, -1, -1, 1]) and np.isfinite(v).sum() == v.size - 1
    arr, _ = source((3, 130), 'hwc', dtype)
    arr[1, 129, 0] = nan                                                             # in a row tail (130 = 32 * 4 + 2)
    with pytest.raises(ValueError, match="contains NaN or Inf"):
        dev.DeviceFlow.from_external(Foreign(arr), dtype=dt)
    if dtype != 'bfloat16':
        arr[1, 129, 0] = -np.inf
        with pytest.raises(ValueError, match="contains NaN or Inf"):
            dev.DeviceFlow.from_external(Foreign(arr), dtype=dt)


def test_host_memory_is_refused_before_any_launch(gpu):
    class Host:
        def __init__(self, arr):
            self.arr = arr
            self.__cuda_array_interface__ = R.cai_dict(arr, arr.ctypes.data)

    arr = np.zeros((5, 7, 2), np.float32)
    with pytest.raises(ValueError, match="not device memory"):
        dev.DeviceFlow.from_external(Host(arr))
    with pytest.raises(ValueError, match="not device memory"):
        dev.DeviceFlow.from_external(Foreign(arr), mask=Host(np.ones((5, 7), np.uint8)))
    with pytest.raises(ValueError, match="not device memory"):
        dev.DeviceImage.from_external(Host(arr))
    with pytest.raises(ValueError, match="not device memory"):
        dev.DevicePoints.from_external(Host(np.zeros((4, 2), np.float64)))
    # the runtime's error for an unknown address has been cleared: the engine goes on working
    same(dev.DeviceFlow.from_external(Foreign(arr)), arr)


def test_adoption(gpu):
    arr, _ = source((5, 8), 'hwc', 'float32')
    mask = np.random.default_rng(9).random((5, 8)) > 0.4
    fv, fm = Foreign(arr), Foreign(mask)
    alive = weakref.ref(fv), weakref.ref(fm)
    ptrs = fv.buf.ptr, fm.buf.ptr
    f = dev.DeviceFlow.from_external(fv, mask=fm, copy=False)
    assert (f.vecs.ptr, f.mask.ptr) == ptrs                                          # shares the memory
    del fv, fm
    gc.collect()
    assert alive[0]() is not None and alive[1]() is not None                        # the field keeps the producer's objects alive
    same(f, arr, mask)
    with np.errstate(over='ignore'):
        same(f + f, arr + arr, mask)                                                 # and works like any other field
    del f
    gc.collect()
    assert alive[0]() is None and alive[1]() is None
    f = dev.DeviceFlow.from_external(Foreign(arr), copy=False)                       # without a mask: all valid, the library's own
    same(f, arr)
    bad = arr.copy()
    bad[2, 3, 1] = np.inf
    with pytest.raises(ValueError, match="contains NaN or Inf"):
        dev.DeviceFlow.from_external(Foreign(bad), copy=False)                       # checked in place, nothing copied
    assert dev.DeviceFlow.from_external(Foreign(bad), copy=False, check_finite=False).shape == (5, 8)
    # refused for everything that needs a conversion
    chw, _ = source((5, 8), 'chw', 'float32')
    half, _ = source((5, 8), 'hwc', 'float16')
    wide = R.flow_values((5, 16, 2), 'float32')
    flat = R.flow_values((5 * 8 * 2 + 2,), 'float32')
    ones = np.ones((5, 16), np.uint8)
    for obj, kw in ((Foreign(chw), {}), (Foreign(half), {}), (Foreign(wide[:, ::2], wide), {}),
                    (Foreign(flat[2:].reshape(5, 8, 2), flat), {}),                  # 8 bytes off the 16-byte grid
                    (Foreign(arr), {'mask': Foreign(ones[:, ::2], ones)})):                        # a strided external mask
        with pytest.raises(ValueError, match="copy=False"):
            dev.DeviceFlow.from_external(obj, copy=False, **kw)


def test_adopted_memory_outlives_the_field_that_adopted_it(gpu):
    """relabel() shares the field's buffers and * k shares its mask: a derivative that is kept when the adopting field is
    dropped must keep the producer's objects alive -- the owner rides on the buffer view, not on the field"""
    arr, _ = source((5, 8), 'hwc', 'float32')
    arr = np.clip(arr, -1e3, 1e3)
    mask = np.random.default_rng(18).random((5, 8)) > 0.4
    fv, fm = Foreign(arr), Foreign(mask)
    alive = weakref.ref(fv), weakref.ref(fm)
    f = dev.DeviceFlow.from_external(fv, 't', mask=fm, copy=False)
    relabelled, scaled, view = f.relabel('s'), f * 2, f.export(copy=False)
    assert relabelled.vecs.ptr == fv.buf.ptr and scaled.mask.ptr == fm.buf.ptr and view.buf.ptr == fv.buf.ptr
    del f, fv, fm
    gc.collect()
    assert alive[0]() is not None and alive[1]() is not None
    assert relabelled.ref == 's'
    same(relabelled, arr, mask)
    same(scaled, arr * np.float32(2), mask)
    assert np.array_equal(R.bits(view.to_host()), R.bits(arr))
    del relabelled, view
    gc.collect()
    assert alive[0]() is None and alive[1]() is not None                             # the product still shares the mask
    same(scaled, arr * np.float32(2), mask)
    del scaled
    gc.collect()
    assert alive[1]() is None
    img = (np.random.default_rng(19).random((5, 7, 3)) * 200).astype(np.uint8)
    src = Foreign(img)
    alive = weakref.ref(src)
    out = dev.DeviceImage.from_external(src, copy=False).export(copy=False)          # the image itself is dropped at once
    del src
    gc.collect()
    assert alive() is not None and np.array_equal(out.to_host(), img)
    del out
    gc.collect()
    assert alive() is None


# ---------------------------------------------------------------------------------------------- export
def test_export_then_import_is_the_identity(gpu):
    for shape in R.SHAPES:
        arr, _ = source(shape, 'hwc', 'float32')
        f = dev.DeviceFlow.from_host(arr, 't', np.random.default_rng(10).random(shape) > 0.4)
        want_v, want_m = f.to_host()
        for layout in ('hwc', 'chw'):
            out = f.export(layout)
            assert out.__cuda_array_interface__["shape"] == (shape + (2,) if layout == 'hwc' else (2,) + shape)
            back = dev.DeviceFlow.from_external(out, layout=layout, mask=f.export_mask())
            same(back, want_v, want_m)
            assert back.vecs.ptr != f.vecs.ptr


@pytest.mark.parametrize("dtype", ['float32', 'float16', 'bfloat16'])
@pytest.mark.parametrize("layout", ['hwc', 'chw'])
def test_export_dtypes(gpu, layout, dtype):
    for shape in R.SHAPES:
        arr, _ = source(shape, 'hwc', 'float32')
        out = dev.DeviceFlow.from_host(arr, 't').export(layout, dtype)
        cai = out.__cuda_array_interface__
        want = R.export_flow(arr, layout, dtype)
        assert cai["version"] == 3 and cai["strides"] is None and cai["stream"] is None and cai["data"] == (out.buf.ptr, False)
        assert cai["typestr"] == {'float32': '<f4', 'float16': '<f2', 'bfloat16': '<i2'}[dtype] and cai["shape"] == want.shape
        got = out.to_host()
        assert np.array_equal(got.view(np.uint16 if got.itemsize == 2 else np.uint32), want.view(np.uint16 if want.itemsize == 2 else np.uint32))
        arr, _ = source((3,) + shape, 'hwc', 'float32', seed=1)
        b = DeviceFlowBatch.from_external(Foreign(arr), 't', layout='hwc')
        got, want = b.export(layout, dtype).to_host(), R.export_flow(arr, layout, dtype)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint16 if got.itemsize == 2 else np.uint32), want.view(np.uint16 if want.itemsize == 2 else np.uint32))


def test_export_views_and_masks(gpu):
    arr, _ = source((5, 7), 'hwc', 'float32')
    mask = np.random.default_rng(11).random((5, 7)) > 0.4
    f = dev.DeviceFlow.from_host(arr, 't', mask)
    view = f.export(copy=False)
    assert view.buf.ptr == f.vecs.ptr and f.export().buf.ptr != f.vecs.ptr
    assert f.export_mask(copy=False).buf.ptr == f.mask.ptr
    m = f.export_mask()
    assert m.__cuda_array_interface__["typestr"] == '|b1' and m.buf.ptr != f.mask.ptr and np.array_equal(m.to_host(), mask)
    for kw in ({'layout': 'chw'}, {'dtype': 'float16'}, {'dtype': 'bfloat16'}):
        with pytest.raises(ValueError, match="copy=False"):
            f.export(copy=False, **kw)
    with pytest.raises(TypeError):
        f.export(dtype='float64')
    with pytest.raises(ValueError):
        f.export('nchw')
    masks = np.random.default_rng(12).random((3, 5, 7)) > 0.4
    b = DeviceFlowBatch.from_external(Foreign(np.broadcast_to(arr, (3, 5, 7, 2)), arr), 's', masks=Foreign(masks))
    assert np.array_equal(b.export_masks().to_host(), masks) and b.export_masks().__cuda_array_interface__["shape"] == (3, 5, 7)
    assert b.export(copy=False).buf.ptr == b.vecs.ptr


# ---------------------------------------------------------------------------------------------- images and points
@pytest.mark.parametrize("dtype", R.IMAGE_DTYPES)
def test_images_chw_and_hwc(gpu, dtype):
    rng = np.random.default_rng(13)
    for h, w in [(1, 1), (5, 7), (3, 130), (2, 1030)]:
        for c in (1, 3, 4, 6):
            chw = (rng.random((c, h, w)) * 200).astype(dtype)
            img = dev.DeviceImage.from_external(Foreign(chw), layout='chw')
            assert img.shape == (h, w, c) and img.dtype == chw.dtype
            assert np.array_equal(img.to_host(), R.to_hwc(chw))
            back = img.export('chw')
            assert back.__cuda_array_interface__["shape"] == (c, h, w) and back.__cuda_array_interface__["typestr"] == chw.dtype.str
            assert np.array_equal(back.to_host(), chw)
    # strided planes, a strided (H, W, C) view, (H, W), and the contiguous cases: copy and adoption
    parent = (rng.random((3, 7, 20)) * 200).astype(dtype)
    view = parent[:, 1:6, 3:17:2]
    assert np.array_equal(dev.DeviceImage.from_external(Foreign(view, parent), layout='chw').to_host(), R.to_hwc(view))
    parent = (rng.random((6, 9, 4)) * 200).astype(dtype)
    view = parent[1:, ::2, :3]
    assert np.array_equal(dev.DeviceImage.from_external(Foreign(view, parent)).to_host(), view)
    flat = (rng.random((5, 7)) * 200).astype(dtype)
    assert np.array_equal(dev.DeviceImage.from_external(Foreign(flat)).to_host(), flat[..., None])
    hwc = (rng.random((5, 7, 3)) * 200).astype(dtype)
    src = Foreign(hwc)
    copied, adopted = dev.DeviceImage.from_external(src), dev.DeviceImage.from_external(src, copy=False)
    assert copied.buf.ptr != src.buf.ptr and adopted.buf.ptr == src.buf.ptr and adopted.buf.owner is src
    assert np.array_equal(copied.to_host(), hwc) and np.array_equal(adopted.to_host(), hwc)
    assert np.array_equal(copied.export().to_host(), hwc) and copied.export(copy=False).buf.ptr == copied.buf.ptr
    with pytest.raises(ValueError, match="copy=False"):
        dev.DeviceImage.from_external(Foreign(view, parent), copy=False)


def test_points_round_trip(gpu):
    rng = np.random.default_rng(14)
    for dtype in (np.float64, np.int32, np.int64):
        pts = (rng.random((37, 2)) * 50).astype(dtype)
        p = dev.DevicePoints.from_external(Foreign(pts))
        assert (p.n, p.dtype, p.shape) == (37, np.dtype(dtype), (37, 2)) and np.array_equal(p.to_host(), pts)
        out = p.export()
        assert out.__cuda_array_interface__["typestr"] == np.dtype(dtype).str and out.buf.ptr != p.buf.ptr
        assert np.array_equal(dev.DevicePoints.from_external(out).to_host(), pts)
        assert p.export(copy=False).buf.ptr == p.buf.ptr
    wide = np.zeros((37, 4))
    with pytest.raises(ValueError, match="contiguous"):
        dev.DevicePoints.from_external(Foreign(wide[:, :2], wide))


# ---------------------------------------------------------------------------------------------- chains and streams
def test_a_chain_entered_from_outside_equals_the_chain_entered_from_the_host(gpu):
    shape = (60, 90)
    a = of.Flow.from_transforms([['rotation', 45, 30, -20]], shape, 't')
    b = of.Flow.from_transforms([['translation', 4.5, -3.25]], shape, 't')
    img = np.random.default_rng(15).random(shape + (3,), dtype=np.float32)
    pts = np.random.default_rng(16).random((50, 2)) * [shape[0] - 1, shape[1] - 1]
    results = []
    for enter in ('host', 'external'):
        if enter == 'host':
            fa, fb = dev.DeviceFlow.from_host(a.vecs, 't', a.mask), dev.DeviceFlow.from_host(b.vecs, 't', b.mask)
            dimg, dpts = dev.DeviceImage.from_host(img), dev.DevicePoints.from_host(pts)
        else:                       # as a network hands them over: planar half is not exact, so planar float32
            fa = dev.DeviceFlow.from_external(Foreign(R.to_chw(a.vecs)), 't', mask=Foreign(a.mask))
            fb = dev.DeviceFlow.from_external(Foreign(R.to_chw(b.vecs)), 't', mask=Foreign(b.mask))
            dimg, dpts = dev.DeviceImage.from_external(Foreign(R.to_chw(img)), layout='chw'), dev.DevicePoints.from_external(Foreign(pts))
        c = fa.combine_with(fb, 3)
        warped, valid = c.apply(dimg)
        tracked = c.relabel('s').track(dpts)
        results.append((c.export('chw').to_host(), c.export_mask().to_host(), warped.export('chw').to_host(),
                        valid.to_host(shape, np.uint8), tracked.export().to_host()))
    for x, y in zip(*results):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert results[0][1].any() and not results[0][1].all()


def test_a_producer_on_another_stream(gpu):
    """A producer fills the source on a stream of its own and from_external(stream=handle) follows at once; the result shows
    the fill.  This cannot PROVE the ordering -- it may pass without the wait, if the fill happens to finish first; that
    ofl_stream_wait_external records on the producer's stream and waits on the library's is a matter of reading its dozen
    lines (csrc/ofl_runtime.hip).  What the test does pin is that the handle path works end to end and harms nothing."""
    lib = nat.load()
    h, w = 270, 480
    src = Foreign(np.zeros((2, h, w), np.float32))
    dev.sync()
    s = ctypes.c_void_p()
    nat.check(lib.ofl_stream_create(ctypes.byref(s)))
    try:
        nat.check(lib.ofl_memset(src.buf.ptr, 0x3c, h * w * 8, s))                   # every float32 becomes 0x3c3c3c3c
        f = dev.DeviceFlow.from_external(src, stream=s.value)
        v = f.to_host()[0]
        assert (v.view(np.uint32) == 0x3c3c3c3c).all()
        assert dev.external_args(src, stream=s.value).stream == s.value
        for handle in (1, 2):                                                         # the legacy and the per-thread default stream
            same(dev.DeviceFlow.from_external(src, stream=handle), v)
    finally:
        nat.check(lib.ofl_stream_sync(s))
        nat.check(lib.ofl_stream_destroy(s))
