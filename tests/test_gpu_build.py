"""DeviceFlow constructors, scaling, padding and cropping on the device (K9, ofl_build.hip), bit for bit against the host
Flow doing the same thing -- vectors compared as uint32 (so that -0.0 counts), masks as bytes -- and against the NumPy
restatement tests/build_ref.py."""
import functools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import build_ref as R

pytestmark = pytest.mark.gpu

PADDINGS = ([0, 0, 0, 0], [1, 2, 3, 4], [13, 0, 0, 9], [0, 7, 5, 0])
CROPS = {
    '[2:5]': slice(2, 5),
    '[:, 1:]': (slice(None), slice(1, None)),
    '[::2, ::3]': (slice(None, None, 2), slice(None, None, 3)),
    '[::-1, ::-1]': (slice(None, None, -1), slice(None, None, -1)),
    '[-3:, -2:]': (slice(-3, None), slice(-2, None)),
    '[4:5, 0:1]': (slice(4, 5), slice(0, 1)),
    '[10:2:-3, :]': (slice(10, 2, -3), slice(None)),
}


def same(dflow, flow):
    """a DeviceFlow equals a host Flow: shape, reference, vector bits, mask bytes"""
    v, m = dflow.to_host()
    assert dflow.shape == tuple(flow.shape) and v.shape == flow.vecs.shape and dflow.ref == flow.ref
    assert np.array_equal(R.bits(v), R.bits(flow.vecs)), "vector bits differ"
    assert np.array_equal(m.view(np.uint8), flow.mask.view(np.uint8)), "mask bytes differ"


@functools.lru_cache(maxsize=None)
def host_from_matrix(name, shape, ref):
    return of.Flow.from_matrix(R.MATRICES[name], shape, ref)


@functools.lru_cache(maxsize=None)
def random_flow(shape, seed=0):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(shape + (2,)) * 5).astype(np.float32)
    return of.Flow(v, 't', rng.random(shape) > 0.3)


def shape_mask(shape, seed=1):
    m = np.random.default_rng(seed).random(shape) > 0.3
    return m


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("name", list(R.MATRICES))
def test_from_matrix_and_from_transforms(gpu, name, ref):
    for shape in R.GPU_SHAPES:
        want = host_from_matrix(name, shape, ref)
        m, sign, _ = dev.matrix_args(R.MATRICES[name], shape, ref)
        got = dev.DeviceFlow.from_matrix(R.MATRICES[name], shape, ref)
        same(got, want)
        assert np.array_equal(R.bits(got.to_host()[0]), R.bits(R.flow_from_matrix(m, shape, sign))), (name, ref, shape)
        mask = shape_mask(shape)
        with_mask = of.Flow(want.vecs, ref, mask)
        same(dev.DeviceFlow.from_matrix(R.MATRICES[name], shape, ref, mask), with_mask)
        same(dev.DeviceFlow.from_matrix(R.MATRICES[name], shape, ref, dev.DeviceBuffer.from_host(mask.view(np.uint8))), with_mask)
        if R.TRANSFORMS[name] is not None:
            same(dev.DeviceFlow.from_transforms(R.TRANSFORMS[name], shape, ref), want)
            same(dev.DeviceFlow.from_transforms(R.TRANSFORMS[name], list(shape), ref, mask.astype(np.uint8)), with_mask)


def test_zero_and_copy(gpu):
    mask = shape_mask((7, 9))
    same(dev.DeviceFlow.zero((7, 9), 's', mask), of.Flow.zero((7, 9), 's', mask))
    z = dev.DeviceFlow.zero([3, 257])
    same(z, of.Flow.zero([3, 257]))
    assert z.is_zero(thresholded=False)
    f = random_flow((33, 130))
    d = f.to_device()
    c = d.copy()
    assert c is not d and c.vecs.ptr != d.vecs.ptr and c.mask.ptr != d.mask.ptr
    same(c, f)


def test_from_matrices_equals_single_builds_and_warps_like_an_uploaded_batch(gpu):
    shape, names = (33, 130), ['rotation', 'product', 'projective']
    mats = np.stack([R.MATRICES[n] for n in names])
    px = shape[0] * shape[1]
    for ref in ('s', 't'):
        b = DeviceFlowBatch.from_matrices(mats, shape, ref)
        assert (b.n, b.shape, b.ref) == (3, shape, ref)
        v = b.vecs.to_host((3,) + shape + (2,), np.float32)
        m = b.mask.to_host((3,) + shape, np.uint8)
        assert (m == 1).all()
        for i, n in enumerate(names):
            single = dev.DeviceFlow.from_matrix(R.MATRICES[n], shape, ref).to_host()[0]
            assert np.array_equal(R.bits(v[i]), R.bits(single)), (n, ref)
            assert np.array_equal(R.bits(v[i]), R.bits(host_from_matrix(n, shape, ref).vecs)), (n, ref)
    # an odd number of pixels per field: every second field starts 8 bytes off the 16-byte grid of the wide stores
    odd = DeviceFlowBatch.from_matrices(mats, (7, 9), 's').vecs.to_host((3, 7, 9, 2), np.float32)
    for i, n in enumerate(names):
        assert np.array_equal(R.bits(odd[i]), R.bits(host_from_matrix(n, (7, 9), 's').vecs)), n
    built = DeviceFlowBatch.from_matrices(mats, shape, 't')
    uploaded = DeviceFlowBatch.from_flows([host_from_matrix(n, shape, 't') for n in names])
    imgs = np.random.default_rng(2).random((3,) + shape + (3,), dtype=np.float32)
    ibuf = dev.DeviceBuffer.from_host(imgs)
    outs = []
    for batch in (built, uploaded):
        warped, valid = batch.apply_images(ibuf, np.float32, 3)
        outs.append((warped.to_host(imgs.shape, np.float32), valid.to_host((3,) + shape, np.uint8)))
    assert np.array_equal(R.bits(outs[0][0]), R.bits(outs[1][0])) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][1].any() and not outs[0][1].all()


@pytest.mark.parametrize("shape", [(7, 9), (3, 257), (300, 400)])
def test_multiply_and_divide(gpu, shape):
    f = random_flow(shape)
    d = f.to_device()
    for k in (0.3, -2, 3, [0.5, -2.0], np.array([3, 7]), np.float32([0.1, 0.7])):
        same(d * k, f * k)
        same(d / k, f / k)
        assert (d * k).mask is d.mask                     # buffers are immutable: the mask is shared, not copied
    same(2.5 * d, f * 2.5)
    with np.errstate(all='ignore'):
        v = f.vecs.copy()
        v[0, 0] = 0                                       # 0 / 0 as well as x / 0
        got, m = (dev.DeviceFlow.from_host(v, 't', f.mask) / 0.0).to_host()
        assert np.array_equal(got, v / np.float32(0.0), equal_nan=True) and np.isnan(got[0, 0]).all()
        assert np.array_equal(m, f.mask)
        got = (d / [0.0, 2.0]).to_host()[0]
        assert np.array_equal(got, (f.vecs / np.array([0.0, 2.0])).astype(np.float32), equal_nan=True)


def test_product_recomputes_is_zero(gpu):
    d = dev.DeviceFlow.from_host(np.full((7, 9, 2), 1e-2, np.float32), 't')
    assert not d.is_zero(thresholded=True)                # evaluated and cached on the source
    p = d * 1e-2
    assert p._stats is None and p._certs == {}
    assert p.is_zero(thresholded=True) and not p.is_zero(thresholded=False)
    assert not (p / 1e-2).is_zero(thresholded=True)


@pytest.mark.parametrize("shape", [(5, 4), (33, 130)])
@pytest.mark.parametrize("mode", ['constant', 'edge', 'symmetric'])
def test_pad(gpu, mode, shape):
    f = random_flow(shape)
    d = f.to_device()
    for p in PADDINGS:
        got = d.pad(p, mode)
        same(got, f.pad(p, mode))
        gv, gm = R.pad(f.vecs, f.mask, p, dev._PAD_MODES[mode])
        same(got, of.Flow(gv, 't', gm))
    same(d.pad([1, 0, 0, 2]), f.pad([1, 0, 0, 2]))        # the default mode


@pytest.mark.parametrize("key", list(CROPS))
def test_crop(gpu, key):
    f = random_flow((33, 130))
    item = CROPS[key]
    got = f.to_device()[item]
    same(got, f[item])
    gv, gm = R.crop(f.vecs, f.mask, *(item if isinstance(item, tuple) else (item, slice(None))))
    same(got, of.Flow(gv, 't', gm))


def test_resident_chain_equals_the_host_chain(gpu):
    """from_transforms -> get_padding -> pad -> apply(DeviceImage) -> crop back, nothing crossing to the host in between,
    against the same chain on the host Flow; apply on its own still gives what it gave"""
    tr, shape = [['rotation', 200, 150, -30]], (300, 400)
    f = of.Flow.from_transforms(tr, shape, 't')
    d = dev.DeviceFlow.from_transforms(tr, shape, 't')
    same(d, f)
    p = d.get_padding()
    assert p == f.get_padding() and any(p)
    fp, dp = f.pad(p), d.pad(p)
    same(dp, fp)
    img = np.random.default_rng(4).random(fp.shape + (2,), dtype=np.float32)
    want, want_valid = fp.apply(img, return_valid_area=True)
    warped, valid = dp.apply(dev.DeviceImage.from_host(img))
    assert np.array_equal(R.bits(warped.to_host()), R.bits(want))             # apply itself is untouched
    assert np.array_equal(valid.to_host(fp.shape, np.uint8), want_valid.view(np.uint8))
    # a two-channel float32 image and its valid area have the layout of a field: crop them on the device
    back = dev.DeviceFlow(warped.buf, valid, fp.shape, 't')[p[0]:p[0] + shape[0], p[2]:p[2] + shape[1]]
    v, m = back.to_host()
    assert back.shape == shape
    assert np.array_equal(R.bits(v), R.bits(want[p[0]:p[0] + shape[0], p[2]:p[2] + shape[1]]))
    assert np.array_equal(m, want_valid[p[0]:p[0] + shape[0], p[2]:p[2] + shape[1]])
    assert m.all()                                        # what get_padding is for: every sampling position inside the padded image
    assert not d.apply(dev.DeviceImage.from_host(img[:shape[0], :shape[1]]))[1].to_host(shape, np.uint8).all()   # and not without it
