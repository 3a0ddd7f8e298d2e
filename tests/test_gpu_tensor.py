"""K12 (ofl_tensor.hip): many-channel float tensors warped on the device, bit for bit against tests/tensor_ref.py (the oracle,
plane by plane), against K1 on the device itself, and through the resident layer: DeviceTensor, DeviceFlow.apply_tensor,
DeviceFlowBatch.apply_tensors, foreign memory in and out.  Nothing here has a tolerance."""
import ctypes
import functools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
from oracle import np_oracle as O
import interop_ref as R
import tensor_ref as T

pytestmark = pytest.mark.gpu
nat = of.native

SHAPES = [(5, 1), (1, 8), (37, 53), (64, 68), (130, 257)]     # (130, 257): odd remainders of the 4 x 64 / 4 x 128 tiles and of the 64-pixel blocks
# 7: the first count K1 cannot take; 37: no multiple of anything; 130 was chosen against the kernel as it stands: planar,
# kChunk = 32 channels per block -> five chunks, the last of 2 channels; channels last, 64 lanes per wave -> two full waves of
# channels and 2 lanes of a third per pixel (and 256 threads per block: the block's step of 256 elements wraps 130 once or twice)
CHANNELS = [1, 6, 7, 37, 130]
QUANTS = [nat.QUANT_OPENCV, nat.QUANT_EXACT]


def combo(si, ci):
    """the field and the masks of shape si with channel count ci: every shape meets all five fields, every channel count
    meets all five fields, every (dtype, layout) meets all three kinds of masks"""
    shape = SHAPES[si]
    vecs = T.flow(T.FLOWS[(si + ci) % 5], shape, seed=si)
    kind = (si + 2 * ci) % 3
    fmask = [T.mask(shape, 10 + si), np.ones(shape, bool), T.mask(shape, 20 + si)][kind]
    tmask = [T.mask(shape, 30 + ci), None, None][kind]
    return shape, vecs, fmask, tmask


@functools.lru_cache(maxsize=None)
def reference(dtype, si, ci, quant):
    """(source, warped, valid) in planar order, computed once and shared by both layouts; read-only"""
    shape, vecs, fmask, tmask = combo(si, ci)
    src = T.values((CHANNELS[ci],) + shape, dtype, seed=100 * si + ci)
    out, valid = T.warp(src, dtype, 'chw', vecs, fmask, tmask, quant)
    for a in (src, out, valid):
        a.flags.writeable = False
    return src, out, valid


def in_layout(planar, layout):
    return planar if layout == 'chw' else np.ascontiguousarray(np.moveaxis(planar, -3, -1))


def tensor(arr, dtype, layout):
    return dev.DeviceTensor.from_host(arr, layout, 'bfloat16' if dtype == 'bfloat16' else None)


def mask_buf(m):
    return None if m is None else dev.DeviceBuffer.from_host(np.ascontiguousarray(m).view(np.uint8))


def make_batch(vecs, masks):
    """(n, H, W, 2) float32 and (n, H, W) bool -> DeviceFlowBatch, reference 't'"""
    n, h, w = masks.shape
    b = DeviceFlowBatch(n, (h, w), 't')
    v, m = np.ascontiguousarray(vecs, np.float32), np.ascontiguousarray(masks).view(np.uint8)
    nat.check(nat.load().ofl_upload(b.vecs.ptr, v.ctypes.data, v.nbytes, None))
    nat.check(nat.load().ofl_upload(b.mask.ptr, m.ctypes.data, m.nbytes, None))
    dev.sync()
    return b


def same(got, want, what):
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(T.raw(got), T.raw(want), err_msg=what)


# ---------------------------------------------------------------------------------------------- 1: against the oracle
@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_every_shape_and_channel_count_against_the_reference(gpu, dtype, layout):
    for si in range(len(SHAPES)):
        for ci in range(len(CHANNELS)):
            shape, vecs, fmask, tmask = combo(si, ci)
            f = dev.DeviceFlow.from_host(vecs, 't', fmask)
            tm = mask_buf(tmask)
            for quant in QUANTS:
                src, want, want_valid = reference(dtype, si, ci, quant)
                what = "{} {} {} C={} {} quant={}".format(dtype, layout, shape, CHANNELS[ci], T.FLOWS[(si + ci) % 5], quant)
                t = tensor(in_layout(src, layout), dtype, layout)
                out, valid = f.apply_tensor(t, tm, quant)
                assert (out.shape, out.dtype, out.layout) == (t.shape, dtype, layout) and out is not t
                same(out.to_host(), in_layout(want, layout), what)
                np.testing.assert_array_equal(valid.to_host(shape, np.uint8), want_valid.astype(np.uint8), err_msg=what)
                if quant == nat.QUANT_OPENCV:       # the batch call: one field, one item
                    tb = tensor(in_layout(src, layout)[None], dtype, layout)
                    out, valid = make_batch(vecs[None], fmask[None]).apply_tensors(tb, tm)
                    same(out.to_host()[0], in_layout(want, layout), what + " batch")
                    np.testing.assert_array_equal(valid.to_host((1,) + shape, np.uint8)[0], want_valid.astype(np.uint8), err_msg=what)


# ---------------------------------------------------------------------------------------------- 2: against K1 on the device
@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_float32_equals_the_image_gather_kernel(gpu, layout):
    for si, shape in enumerate(SHAPES):
        for c in (1, 6):
            hwc = T.values(shape + (c,), 'float32', seed=si)
            image = dev.DeviceImage.from_host(hwc)
            t = tensor(hwc if layout == 'hwc' else R.to_chw(hwc), 'float32', layout)
            for k, name in enumerate(T.FLOWS):
                f = dev.DeviceFlow.from_host(T.flow(name, shape, seed=k), 't', T.mask(shape, 40 + k))
                for tm in (None, mask_buf(T.mask(shape, 50 + k))):
                    for quant in QUANTS:
                        want, want_valid = f.apply_image(image, tm, quant=quant)
                        out, valid = f.apply_tensor(t, tm, quant)
                        got = out.to_host()
                        same(got if layout == 'hwc' else R.to_hwc(got), want.to_host(), "{} {} C={} {}".format(layout, shape, c, name))
                        np.testing.assert_array_equal(valid.to_host(shape, np.uint8), want_valid.to_host(shape, np.uint8))


# ---------------------------------------------------------------------------------------------- 3: batches
def item(t, i):
    """item i of a batched DeviceTensor, on the same memory"""
    nb = t.nbytes // t.n
    return dev.DeviceTensor(t.buf.view(i * nb, nb), t.shape[1:], t.dtype, t.layout)


@pytest.mark.parametrize("layout", T.LAYOUTS)
def test_a_batch_equals_its_single_calls(gpu, layout):
    n, c, shape = 3, 7, (37, 53)
    vecs = np.stack([T.flow(name, shape, seed=k) for k, name in enumerate(['wobble', 'rotation', 'half'])])
    fmasks = np.stack([T.mask(shape, 60 + k) for k in range(n)])
    tmasks = np.stack([T.mask(shape, 70 + k) for k in range(n)])
    src = T.values(dev.tensor_mem_shape((n, c) + shape, layout), 'float16', seed=7)
    t = tensor(src, 'float16', layout)
    b = make_batch(vecs, fmasks)
    fields = [dev.DeviceFlow.from_host(vecs[i], 't', fmasks[i]) for i in range(n)]
    for masks, shared in ((None, False), (tmasks, False), (tmasks[1], True)):
        out, valid = b.apply_tensors(t, mask_buf(masks), shared_masks=shared)
        assert out.shape == (n, c) + shape
        got, got_valid = out.to_host(), valid.to_host((n,) + shape, np.uint8)
        for i in range(n):
            tm = None if masks is None else mask_buf(masks if shared else masks[i])
            one, one_valid = fields[i].apply_tensor(item(t, i), tm)
            same(got[i], one.to_host(), "item {}".format(i))
            np.testing.assert_array_equal(got_valid[i], one_valid.to_host(shape, np.uint8))
        assert not np.array_equal(got[0], got[1]) and got_valid.any() and not got_valid.all()
    # one field warps every item of a batched tensor
    for tm in (None, mask_buf(tmasks[0])):
        out, valid = fields[1].apply_tensor(t, tm)
        got = out.to_host()
        for i in range(n):
            one, one_valid = fields[1].apply_tensor(item(t, i), tm)
            same(got[i], one.to_host(), "shared field, item {}".format(i))
            np.testing.assert_array_equal(valid.to_host(shape, np.uint8), one_valid.to_host(shape, np.uint8))
    with pytest.raises(ValueError, match="QUANT_OPENCV"):
        b.apply_tensors(t, quant=nat.QUANT_EXACT)


# ---------------------------------------------------------------------------------------------- 4: the zero-flow short cut
def test_a_zero_flow_returns_the_tensor_itself(gpu):
    shape, c = (37, 53), 7
    vecs = np.full(shape + (2,), 5e-4, np.float32)
    fmask, tmask = T.mask(shape, 80), T.mask(shape, 81)
    f = dev.DeviceFlow.from_host(vecs, 't', fmask)
    src = T.values((c,) + shape, 'bfloat16', seed=8)
    t = tensor(src, 'bfloat16', 'chw')
    out, valid = f.apply_tensor(t, mask_buf(tmask))
    assert out is t
    np.testing.assert_array_equal(valid.to_host(shape, np.uint8), (fmask & tmask).astype(np.uint8))
    out, valid = f.apply_tensor(t)
    assert out is t
    np.testing.assert_array_equal(valid.to_host(shape, np.uint8), fmask.astype(np.uint8))
    # the batch call takes no short cut: under the 1/32-px snapping the warp itself is the identity
    out, valid = make_batch(vecs[None], fmask[None]).apply_tensors(tensor(src[None], 'bfloat16', 'chw'), mask_buf(tmask))
    # ... as VALUES: the blend of an identity warp is v * 1 + v01 * 0 + ..., and -0.0 + 0.0 is +0.0 (K1 and the oracle's
    # gather do the same), so a -0.0 comes back as +0.0 -- the one bit the short cut of the single call keeps.  Everything
    # else is the input's bit pattern.
    got = out.to_host()[0]
    minus_zero = src == 0x8000
    assert minus_zero.any()
    np.testing.assert_array_equal(got[~minus_zero], src[~minus_zero])
    assert not (got[minus_zero] & 0x7fff).any()
    np.testing.assert_array_equal(R.bf16_to_f32(got), R.bf16_to_f32(src))
    np.testing.assert_array_equal(valid.to_host(shape, np.uint8), (fmask & tmask).astype(np.uint8))


# ---------------------------------------------------------------------------------------------- 5: foreign memory
class Foreign:
    """`view` (a view of the C-contiguous `parent`, or the parent itself) as device memory of "another framework" """

    def __init__(self, view, parent=None, stream=None):
        parent = view if parent is None else parent
        assert parent.flags.c_contiguous
        self.buf = dev.DeviceBuffer.from_host(parent)
        offset = view.__array_interface__['data'][0] - parent.__array_interface__['data'][0]
        self.__cuda_array_interface__ = R.cai_dict(view, self.buf.ptr + offset, 3, stream)


def test_foreign_tensors_in(gpu):
    parent = T.values((2, 8, 11, 13), 'float16', seed=9)
    src = Foreign(parent)
    adopted = dev.DeviceTensor.from_external(src, copy=False)
    copied = dev.DeviceTensor.from_external(src)
    assert adopted.buf.ptr == src.buf.ptr and adopted.buf.owner is src and copied.buf.ptr != src.buf.ptr
    assert (adopted.shape, adopted.dtype, adopted.layout) == ((2, 8, 11, 13), 'float16', 'chw')
    same(adopted.to_host(), parent, "adopted")
    same(copied.to_host(), parent, "copied")
    # strided views go through the import kernel, in both layouts and element sizes
    for dtype in T.DTYPES:
        dt = 'bfloat16' if dtype == 'bfloat16' else None
        parent = T.values((2, 8, 11, 13), dtype, seed=10)
        for view in (parent[:, 1::2], parent[:, :, 2:9, 3:12], parent[1], parent[0, ::3, 1:]):
            t = dev.DeviceTensor.from_external(Foreign(view, parent), dtype=dt)
            assert t.shape == view.shape and t.layout == 'chw' and t.dtype == dtype
            same(t.to_host(), np.ascontiguousarray(view), "chw view")
            if not view.flags.c_contiguous:
                with pytest.raises(ValueError, match="copy=False"):
                    dev.DeviceTensor.from_external(Foreign(view, parent), dtype=dt, copy=False)
        parent = T.values((2, 11, 13, 8), dtype, seed=11)
        for view in (parent[..., 1::2], parent[:, 2:9, 3:12]):
            t = dev.DeviceTensor.from_external(Foreign(view, parent), layout='hwc', dtype=dt)
            assert t.shape == (2, view.shape[3], view.shape[1], view.shape[2]) and t.layout == 'hwc'
            same(t.to_host(), np.ascontiguousarray(view), "hwc view")


def test_foreign_host_memory_is_refused_before_any_launch(gpu):
    class Host:
        def __init__(self, arr):
            self.arr = arr
            self.__cuda_array_interface__ = R.cai_dict(arr, arr.ctypes.data)

    arr = np.zeros((7, 5, 9), np.float32)
    with pytest.raises(ValueError, match="not device memory"):
        dev.DeviceTensor.from_external(Host(arr))
    with pytest.raises(ValueError, match="not device memory"):
        dev.DeviceTensor.from_external(Host(arr[:, 1:4]))
    same(dev.DeviceTensor.from_external(Foreign(arr)).to_host(), arr, "the engine goes on working")


def test_a_tensor_producer_on_another_stream(gpu):
    """as test_gpu_interop.test_a_producer_on_another_stream: the handle path works end to end; the ordering itself is a
    matter of reading ofl_stream_wait_external"""
    lib = nat.load()
    shape = (16, 135, 240)
    src = Foreign(np.zeros(shape, np.float32))
    dev.sync()
    s = ctypes.c_void_p()
    nat.check(lib.ofl_stream_create(ctypes.byref(s)))
    try:
        nat.check(lib.ofl_memset(src.buf.ptr, 0x3c, int(np.prod(shape)) * 4, s))
        t = dev.DeviceTensor.from_external(src, stream=s.value)
        assert (t.to_host().view(np.uint32) == 0x3c3c3c3c).all()
    finally:
        nat.check(lib.ofl_stream_sync(s))
        nat.check(lib.ofl_stream_destroy(s))


@pytest.mark.parametrize("c", [7, 130])
def test_export_in_the_other_layout_and_back(gpu, c):
    for dtype in T.DTYPES:
        dt = 'bfloat16' if dtype == 'bfloat16' else None
        for mem_shape, layout in (((2, c, 37, 53), 'chw'), ((c, 5, 1), 'chw'), ((2, 37, 53, c), 'hwc'), ((33, 64, c), 'hwc')):
            arr = T.values(mem_shape, dtype, seed=c)
            t = tensor(arr, dtype, layout)
            other = 'hwc' if layout == 'chw' else 'chw'
            out = t.export(other)
            cai = out.__cuda_array_interface__
            assert cai["typestr"] == {'float32': '<f4', 'float16': '<f2', 'bfloat16': '<i2'}[dtype]
            assert cai["shape"] == dev.tensor_mem_shape(t.shape, other)
            want = np.moveaxis(arr, -3, -1) if layout == 'chw' else np.moveaxis(arr, -1, -3)
            same(out.to_host(), np.ascontiguousarray(want), "export {} -> {}".format(layout, other))
            back = dev.DeviceTensor.from_external(out, layout=other, dtype=dt).export(layout)
            same(back.to_host(), arr, "and back")
            assert t.export(copy=False).buf.ptr == t.buf.ptr and t.export().buf.ptr != t.buf.ptr
            with pytest.raises(ValueError, match="copy=False"):
                t.export(other, copy=False)


# ---------------------------------------------------------------------------------------------- 6: offsets beyond 2^31 elements
def test_planar_offsets_beyond_two_to_the_31(gpu):
    """float16 (2049, 1024, 1024): plane 2048 starts exactly at element 2^31.  A wrapped index would leave part of the
    destination at its 0xFF fill or land a plane in the wrong place.  (Channels last is not run at this size -- the host
    cannot stage it cheaply; it goes through the same 64-bit helper, tensor_index.)"""
    lib = nat.load()
    c, h, w = 2049, 1024, 1024
    plane = h * w * 2
    marked = [0, 1023, 2047, 2048]
    vecs = T.flow('rotation', (h, w))
    fmask = np.ones((h, w), bool)
    rng = np.random.default_rng(12)
    planes = rng.standard_normal((len(marked), h, w)).astype(np.float16)
    want, want_valid = T.warp(planes, 'float16', 'chw', vecs, fmask)
    try:
        src, dst = dev.DeviceBuffer(c * plane), dev.DeviceBuffer(c * plane)
        nat.check(lib.ofl_memset(src.ptr, 0, c * plane, None))
        nat.check(lib.ofl_memset(dst.ptr, 0xFF, c * plane, None))
        for k, p in enumerate(marked):
            nat.check(lib.ofl_upload(src.ptr + p * plane, planes[k].ctypes.data, plane, None))
        f = dev.DeviceFlow.from_host(vecs, 't', fmask)
        valid = dev.DeviceBuffer(h * w)
        nat.check(lib.ofl_gather_tensor_dev(src.ptr, nat.EL_F16, nat.TENSOR_NCHW, 1, c, h, w, f.vecs.ptr, 1, -1, None, 1, f.mask.ptr,
                                            dst.ptr, valid.ptr, nat.QUANT_OPENCV, None))
        for k, p in enumerate(marked):
            got = dst.view(p * plane, plane).to_host((h, w), np.uint16)
            assert not (got == 0xFFFF).any(), "plane {} was not written everywhere".format(p)
            np.testing.assert_array_equal(got, T.raw(want[k]), err_msg="plane {}".format(p))
        for p in (1, 2046):
            got = dst.view(p * plane, plane).to_host((h, w), np.uint16)
            assert not got.any(), "plane {} of a zero source is not zero".format(p)
        tail = dst.view(c * plane - 8 * w * 2, 8 * w * 2).to_host((8, w), np.uint16)        # the last rows of the last plane
        np.testing.assert_array_equal(tail, T.raw(want[3])[-8:])
        np.testing.assert_array_equal(valid.to_host((h, w), np.uint8), want_valid.astype(np.uint8))
    finally:
        src = dst = None
        dev.empty_cache()


# ---------------------------------------------------------------------------------------------- 7: refusals of the C entry
def test_the_c_entry_refuses_bad_arguments_before_any_launch(gpu):
    lib = nat.load()
    h, w = 5, 7
    buf = dev.DeviceBuffer.zeros(4 * 2 * h * w * 4)
    flow, fmask, valid = dev.DeviceBuffer.zeros(h * w * 8), dev.DeviceBuffer.zeros(h * w), dev.DeviceBuffer.zeros(4 * h * w)
    good = dict(src=buf.ptr, elem=nat.EL_F32, layout=nat.TENSOR_NCHW, N=1, C=2, H=h, W=w, flow=flow.ptr, flow_shared=1, sign=-1,
                smask=None, smask_shared=1, fmask=fmask.ptr, dst=buf.ptr + 2 * h * w * 4, valid=valid.ptr, quant=nat.QUANT_OPENCV, stream=None)
    assert lib.ofl_gather_tensor_dev(*good.values()) == nat.OK
    for change, word in ((dict(elem=nat.EL_F64), "elem"), (dict(elem=7), "elem"), (dict(C=0), "C must"), (dict(N=65536), "N must"),
                         (dict(layout=2), "layout"), (dict(src=None), "src"), (dict(fmask=None), "fmask"), (dict(H=32767), "H, W")):
        assert lib.ofl_gather_tensor_dev(*dict(good, **change).values()) == nat.E_INVALID, change
        assert word in nat.last_error(), (change, nat.last_error())
    assert lib.ofl_tensor_permute_dev(buf.ptr, buf.ptr, 8, 1, 2, h, w, 1, None) == nat.E_INVALID
    assert lib.ofl_tensor_import_dev(buf.ptr, 4, 0, -1, 0, 0, 0, 1, 2, h, w, buf.ptr, None) == nat.E_INVALID
    dev.sync()
