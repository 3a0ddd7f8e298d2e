"""Point tracking on HBM-resident fields and points (K10, ofl_track.hip): DeviceFlow.track, DeviceFlowBatch.track and
DeviceFlowBatch.track_sequence, bit for bit against the host Flow.track on the same field (which the existing goldens pin
to the reference) and against the NumPy restatement tests/track_ref.py."""
import functools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import track_ref as T

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (64, 96)]            # rows of 53 and 96 pixels: no field row starts where a wave or a workgroup does
COUNTS = [0, 1, 255, 257, 1000]


def transforms(shape):
    h, w = shape
    return [['rotation', (w - 1) / 2, (h - 1) / 2, 9], ['translation', 2.5, -1.75]]


@functools.lru_cache(maxsize=None)
def host_flow(shape, ref, hole=False):
    mask = np.ones(shape, bool)
    if hole:
        mask[shape[0] // 4: shape[0] // 2, shape[1] // 3: 2 * shape[1] // 3] = False
    return of.Flow.from_transforms(transforms(shape), shape, ref, mask)


@functools.lru_cache(maxsize=None)
def device_flow(shape, ref, hole=False):
    return host_flow(shape, ref, hole).to_device()


def inner_points(shape, n, seed=0):
    """float points strictly inside the area"""
    rng = np.random.default_rng(seed + n)
    return rng.random((n, 2)) * (np.array(shape) - 1.0 - 1e-9) + 5e-10


def edge_points(shape):
    """exactly on row 0, row H-1, col 0 and col W-1, and at integer positions"""
    h, w = shape
    p = [[0.0, 3.5], [h - 1.0, 3.5], [2.25, 0.0], [2.25, w - 1.0], [0.0, 0.0], [h - 1.0, w - 1.0], [0.0, w - 1.0], [h - 1.0, 0.0]]
    p += [[float(r), float(c)] for r in range(0, h, 5) for c in range(0, w, 7)]
    return np.array(p)


def wide_points(shape, n, seed=3):
    """float points over the frame and a margin around it: some outside the hull of a 't' field's points"""
    rng = np.random.default_rng(seed + n)
    return rng.random((n, 2)) * (np.array(shape) + 12.0) - 6.0


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), "tracked points differ"
    if got.dtype == np.float64:
        assert np.array_equal(np.signbit(got), np.signbit(want))


# ------------------------------------------------------------------------------ 1. single step, all four paths
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", COUNTS)
def test_bilinear_inside(gpu, shape, n):
    f, d = host_flow(shape, 's'), device_flow(shape, 's')
    pts = inner_points(shape, n)
    got = d.track(pts)
    same(got, f.track(pts).astype(np.float64))
    same(got, T.track(f.vecs, pts))
    same(d.track(dev.DevicePoints.from_host(pts)).to_host(), got)        # resident points: the same bits
    same(d.track(pts.astype(np.float32)), T.track(f.vecs, pts.astype(np.float32).astype(np.float64)))


@pytest.mark.parametrize("shape", SHAPES)
def test_bilinear_edges_and_integer_positions(gpu, shape):
    f, d = host_flow(shape, 's'), device_flow(shape, 's')
    pts = edge_points(shape)
    got = d.track(pts)
    same(got, f.track(pts))
    same(got, T.track(f.vecs, pts))
    h, w = shape
    on_last = (pts[:, 0] == h - 1) | (pts[:, 1] == w - 1)
    assert on_last.sum() >= 5 and np.array_equal(got[on_last], pts[on_last])      # the clipped corner weights give 0 there


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("n", COUNTS)
def test_integer_points(gpu, shape, dtype, n):
    f, d = host_flow(shape, 's'), device_flow(shape, 's')
    rng = np.random.default_rng(n)
    pts = np.stack([rng.integers(0, shape[0], n), rng.integers(0, shape[1], n)], axis=-1).astype(dtype)
    if n >= 4:
        pts[:4] = [[0, 0], [shape[0] - 1, shape[1] - 1], [0, shape[1] - 1], [shape[0] - 1, 0]]
    got = d.track(pts)
    same(got, f.track(pts))
    same(got, T.track(f.vecs, pts))
    same(d.track(dev.DevicePoints.from_host(pts)).to_host(), got)
    same(d.track(pts, int_out=True), f.track(pts, int_out=True))
    same(d.track(pts, s_exact_mode=True), got)                          # integer points take the pixel path first, utils.py:590


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [0, 1, 257])
def test_exact_mode(gpu, shape, n):
    f, d = host_flow(shape, 's'), device_flow(shape, 's')
    pts = np.concatenate([inner_points(shape, n), edge_points(shape)[:8 if n else 0]])
    got = d.track(pts, s_exact_mode=True)
    same(got, f.track(pts, s_exact_mode=True))
    same(d.track(dev.DevicePoints.from_host(pts), s_exact_mode=True).to_host(), got)
    same(d.track(pts, int_out=True, s_exact_mode=True), f.track(pts, int_out=True, s_exact_mode=True))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", COUNTS)
def test_ref_t(gpu, shape, n):
    """points outside the hull of grid - flow become (0, 0), as in the reference"""
    f, d = host_flow(shape, 't'), device_flow(shape, 't')
    pts = wide_points(shape, n)
    want = f.track(pts)
    got = d.track(pts)
    same(got, want)
    if n >= 255:
        zeroed = (want == 0).all(axis=1)
        assert zeroed.any() and not zeroed.all()
    same(d.track(dev.DevicePoints.from_host(pts)).to_host(), got)
    same(d.track(pts, int_out=True), f.track(pts, int_out=True))
    ipts = np.round(inner_points(shape, n)).astype(np.int64)               # integer points on a 't' field: the query path
    same(d.track(ipts), f.track(ipts))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", COUNTS)
def test_int_out(gpu, shape, n):
    f, d = host_flow(shape, 's'), device_flow(shape, 's')
    pts = inner_points(shape, n)
    got = d.track(pts, int_out=True)
    assert got.dtype == np.int32
    same(got, f.track(pts, int_out=True))
    same(got, T.track(f.vecs, pts, int_out=True))
    half = np.array([[1.5, 2.5], [2.5, 3.5], [0.5, 0.5]])                  # np.round: half to even
    zero = of.Flow(np.zeros(shape + (2,), np.float32), 's').to_device()
    same(zero.track(half, int_out=True), np.array([[2, 2], [2, 4], [0, 0]], np.int32))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ref", ['s', 't'])
def test_valid_status(gpu, shape, ref):
    """a field whose mask has a rectangle cleared: status is valid_source() at the rounded points"""
    f, d = host_flow(shape, ref, True), device_flow(shape, ref, True)
    pts = np.concatenate([inner_points(shape, 257), edge_points(shape)])
    want_p, want_s = f.track(pts, get_valid_status=True)
    got_p, got_s = d.track(pts, get_valid_status=True)
    same(got_p, want_p)
    assert got_s.dtype == np.bool_ and np.array_equal(got_s, want_s)
    assert want_s.any() and not want_s.all()
    dp, ds = d.track(dev.DevicePoints.from_host(pts), get_valid_status=True)
    same(dp.to_host(), want_p)
    assert np.array_equal(ds.to_host((len(pts),), np.uint8), want_s.view(np.uint8))
    if ref == 's':
        ref_p, ref_s = T.track(f.vecs, pts, valid=f.valid_source())
        same(got_p, ref_p)
        assert np.array_equal(got_s, ref_s)
        ipts = np.round(pts).astype(np.int64)
        gi, si = d.track(ipts, get_valid_status=True)
        wi, wsi = f.track(ipts, get_valid_status=True)
        same(gi, wi)
        assert np.array_equal(si, wsi)


# ------------------------------------------------------------------------------ 2. the zero-flow rule
@pytest.mark.parametrize("ref", ['s', 't'])
def test_zero_flow_rule(gpu, ref):
    shape = (37, 53)
    pts = np.concatenate([inner_points(shape, 257), edge_points(shape)])
    tiny = of.Flow(np.full(shape + (2,), 5e-4, np.float32), ref)
    small = of.Flow(np.full(shape + (2,), 2e-3, np.float32), ref)
    for kw in ({}, {'s_exact_mode': True}):
        same(tiny.to_device().track(pts, **kw), pts)                       # unchanged, bitwise: not moved by 5e-4
        same(tiny.to_device().track(pts, **kw), tiny.track(pts, **kw))
    ipts = np.round(pts).astype(np.int64)
    same(tiny.to_device().track(ipts), ipts.astype(np.float64))            # float64 where the reference hands `pts` back
    if ref == 's':
        moved = small.to_device().track(pts)
        same(moved, small.track(pts))
        off = (pts[:, 0] < shape[0] - 1) & (pts[:, 1] < shape[1] - 1)
        assert np.all(moved[off] != pts[off])
    outside = [[-5.0, 3.0], [3.0, 400.0]] + ([[np.nan, 1.0]] if ref == 's' else [])      # the reference does not look at the area either
    same(tiny.to_device().track(np.array(outside)), np.array(outside))


# ------------------------------------------------------------------------------ 3. points outside the area
def bad_float_points(shape):
    pts = inner_points(shape, 255)
    a, b = pts.copy(), pts.copy()
    a[100] = [-0.25, 3.0]
    b[254] = [np.nan, 3.0]
    return pts, [a, b]


def test_outside_raises(gpu):
    shape = (37, 53)
    f, d = host_flow(shape, 's'), device_flow(shape, 's')
    good, bad = bad_float_points(shape)
    for pts in bad:
        with pytest.raises(IndexError):
            f.track(pts)
        with pytest.raises(IndexError):
            d.track(pts)
        with pytest.raises(IndexError):
            d.track(dev.DevicePoints.from_host(pts))
    same(d.track(good), f.track(good))
    ipts = np.round(good).astype(np.int64)
    same(d.track(ipts), f.track(ipts))
    ipts[7] = [shape[0], 3]
    with pytest.raises(IndexError):
        f.track(ipts)
    with pytest.raises(IndexError):
        d.track(ipts)
    ipts[7] = [3, -1]                                                      # NumPy would wrap this one around
    with pytest.raises(IndexError):
        d.track(ipts)


def test_batch_outside_raises(gpu):
    shape = (37, 53)
    batch = matrices_batch(shape)
    good, bad = bad_float_points(shape)
    for pts in bad:
        with pytest.raises(IndexError):
            batch.track(pts)
    assert batch.track(good).shape == (batch.n, 255, 2)
    with pytest.raises(TypeError):
        batch.track(np.round(good).astype(np.int64))
    with pytest.raises(ValueError):
        DeviceFlowBatch.from_flows([host_flow(shape, 't')]).track(good)


# ------------------------------------------------------------------------------ 4. independent batch
def matrices(shape):
    h, w = shape
    lists = [[['rotation', (w - 1) / 2, (h - 1) / 2, a], ['translation', tx, ty]]
             for a, tx, ty in ((5, 1.5, -2.0), (-8, 0.25, 0.5), (0, 0, 0), (12, -1.0, 1.0), (0, 3e-4, -2e-4))]
    return np.stack([of.utils.matrix_from_transforms(t) for t in lists])


def matrices_batch(shape):
    return DeviceFlowBatch.from_matrices(matrices(shape), shape, 's')


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", COUNTS)
def test_independent_batch(gpu, shape, n):
    """5 fields (one the identity, one zero under the threshold): row i is DeviceFlow.track on field i"""
    batch = matrices_batch(shape)
    pts = np.concatenate([inner_points(shape, n), edge_points(shape)[:8 if n else 0]])
    got_p, got_s = batch.track(pts, get_valid_status=True)
    assert got_p.shape == (5, len(pts), 2) and got_s.shape == (5, len(pts)) and got_s.dtype == np.bool_
    got_i = batch.track(pts, int_out=True)
    dp = batch.track(dev.DevicePoints.from_host(pts))
    same(dp.to_host(), got_p)
    same(batch.track(pts), got_p)
    for i, m in enumerate(matrices(shape)):
        single = dev.DeviceFlow.from_matrix(m, shape, 's')
        want_p, want_s = single.track(pts, get_valid_status=True)
        same(got_p[i], want_p)
        assert np.array_equal(got_s[i], want_s)
        same(got_i[i], single.track(pts, int_out=True))
        same(batch.field(i).track(pts), want_p)
    if n:
        same(got_p[2], pts)
        same(got_p[4], pts)
        assert not np.array_equal(got_p[0], got_p[1])


# ------------------------------------------------------------------------------ 5. sequences, ref 's'
@functools.lru_cache(maxsize=None)
def sequence():
    """(host flows, batch, valid_source maps, points, track_ref's answer) of the sequence stated in track_ref.py"""
    flows = [of.Flow(v, 's', m) for v, m in T.sequence_fields()]
    valids = [f.valid_source() for f in flows]
    pts = T.sequence_points()
    return flows, DeviceFlowBatch.from_flows(flows), valids, pts, T.track_sequence([f.vecs for f in flows], pts, valids=valids)


def test_sequence_s(gpu):
    flows, batch, valids, pts, (want_p, want_lost, want_s, want_path) = sequence()
    # the case is not vacuous
    survived = want_lost < 0
    assert len(set(want_lost.tolist())) >= 3 and survived.mean() >= 0.25
    assert want_s[survived].any() and not want_s[survived].all()
    assert np.array_equal(want_path[T.SEQ_ZERO_FIELD], want_path[T.SEQ_ZERO_FIELD + 1])

    got_p, got_lost, got_s, got_path = batch.track_sequence(pts, get_valid_status=True, return_path=True)
    same(got_p, want_p)
    assert got_lost.dtype == np.int32 and np.array_equal(got_lost, want_lost)
    assert got_s.dtype == np.bool_ and np.array_equal(got_s, want_s)
    same(got_path, want_path)

    # the loop of single steps on the surviving points
    p, s = pts[survived], np.ones(int(survived.sum()), bool)
    for f in flows:
        p, sk = f.to_device().track(p, get_valid_status=True)
        s &= sk
    same(got_p[survived], p)
    assert np.array_equal(got_s[survived], s)

    # the other argument combinations, resident points
    plain = batch.track_sequence(pts)
    assert len(plain) == 2
    same(plain[0], want_p)
    assert np.array_equal(plain[1], want_lost)
    ints = batch.track_sequence(pts, int_out=True, return_path=True)
    same(ints[0], np.round(want_p).astype('i'))
    same(ints[2], want_path)
    res = batch.track_sequence(dev.DevicePoints.from_host(pts), get_valid_status=True, return_path=True)
    same(res[0].to_host(), want_p)
    assert np.array_equal(res[1].to_host((len(pts),), np.int32), want_lost)
    assert np.array_equal(res[2].to_host((len(pts),), np.uint8), want_s.view(np.uint8))
    same(res[3].to_host(), want_path)


def test_sequence_s_short_and_empty(gpu):
    flows, batch, valids, pts, _ = sequence()
    one = DeviceFlowBatch.from_flows(flows[:1])
    got_p, got_lost, got_s, got_path = one.track_sequence(pts, get_valid_status=True, return_path=True)
    want_p, want_s = flows[0].to_device().track(pts, get_valid_status=True)
    same(got_p, want_p)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_lost, np.full(len(pts), -1, np.int32))
    same(got_path, np.stack([pts, want_p]))
    none = np.zeros((0, 2))
    got_p, got_lost, got_s, got_path = batch.track_sequence(none, get_valid_status=True, return_path=True)
    assert got_p.shape == (0, 2) and got_lost.shape == (0,) and got_s.shape == (0,) and got_path.shape == (len(flows) + 1, 0, 2)
    with pytest.raises(TypeError):
        batch.track_sequence(np.zeros((3, 2), np.int64))
    with pytest.raises(TypeError):
        batch.track_sequence(pts, return_path='yes')


# ------------------------------------------------------------------------------ 6. sequences, ref 't'
def test_sequence_t(gpu):
    """3 fields on 37 x 53, 257 points: the loop of single 't' steps with the points that were not found frozen"""
    shape = (37, 53)
    h, w = shape
    lists = [[['rotation', (w - 1) / 2, (h - 1) / 2, 6], ['translation', 4, 3]],
             [['translation', -6.5, 2.25]],
             [['rotation', 10, 20, -10], ['translation', 5, -4]]]
    flows = [of.Flow.from_transforms(t, shape, 't') for t in lists]
    flows[1].mask = np.arange(h * w).reshape(shape) % 7 != 0
    batch = DeviceFlowBatch.from_flows(flows)
    rng = np.random.default_rng(5)
    pts = rng.random((257, 2)) * (np.array(shape) + 4.0) - 2.0
    want_p, want_lost, want_s, want_path = pts.copy(), np.full(257, -1, np.int32), np.ones(257, bool), [pts.copy()]
    for k, f in enumerate(flows):
        d = f.to_device()
        alive = want_lost < 0
        stepped, sk = d.track(want_p, get_valid_status=True)
        _, found = dev.scatter_query(d.vecs, -1, d.vecs, 2, h, w, want_p[:, ::-1].copy())
        assert np.array_equal(stepped[~found], np.zeros((int((~found).sum()), 2)))       # the single step's "not found"
        want_lost[alive & ~found] = k
        alive &= found
        want_p[alive] = stepped[alive]
        want_s &= sk
        want_s[~alive] = False
        want_path.append(want_p.copy())
    assert len(set(want_lost.tolist())) >= 3 and (want_lost < 0).mean() >= 0.25

    got_p, got_lost, got_s, got_path = batch.track_sequence(pts, get_valid_status=True, return_path=True)
    same(got_p, want_p)
    assert np.array_equal(got_lost, want_lost)
    assert np.array_equal(got_s, want_s)
    same(got_path, np.stack(want_path))
    plain = batch.track_sequence(dev.DevicePoints.from_host(pts), int_out=True)
    same(plain[0].to_host(), np.round(want_p).astype('i'))
    assert np.array_equal(plain[1].to_host((257,), np.int32), want_lost)
    same(batch.track_sequence(pts)[0], want_p)


# ------------------------------------------------------------------------------ 7. residency
def test_sequence_stays_on_the_device(gpu, monkeypatch):
    flows, batch, valids, pts, (want_p, want_lost, want_s, want_path) = sequence()
    dpts = dev.DevicePoints.from_host(pts)
    batch.track_sequence(dpts, get_valid_status=True)                     # warm: the batch's flag words exist
    n, field_bytes = len(pts), T.SEQ_SHAPE[0] * T.SEQ_SHAPE[1]            # the smallest per-field array: one mask
    ups, downs = [], []
    real_up, real_down = dev.DeviceBuffer.from_host.__func__, dev.DeviceBuffer.to_host

    def counting_up(cls, arr, stream=None):
        ups.append(np.asarray(arr).nbytes)
        return real_up(cls, arr, stream)

    def counting_down(self, shape, dtype, stream=None):
        downs.append(int(np.prod(shape)) * np.dtype(dtype).itemsize)
        return real_down(self, shape, dtype, stream)

    monkeypatch.setattr(dev.DeviceBuffer, "from_host", classmethod(counting_up))
    monkeypatch.setattr(dev.DeviceBuffer, "to_host", counting_down)
    p, lost, status = batch.track_sequence(dpts, get_valid_status=True)
    assert ups == [] and downs == []                                       # resident in, resident out: nothing crosses
    p, lost, status = p.to_host(), lost.to_host((n,), np.int32), status.to_host((n,), np.uint8)
    assert sorted(downs) == sorted([n * 16, n * 4, n])
    same(p, want_p)
    assert np.array_equal(lost, want_lost) and np.array_equal(status, want_s.view(np.uint8))

    # one resident step: the 4-byte outside counter comes down, the field does not move
    inside = dev.DevicePoints.from_host(pts)
    assert max(ups) < field_bytes                                          # points only
    d = batch.field(0)
    d.track(inside)                                                        # warm: the field's flag word exists
    del ups[:], downs[:]
    out = d.track(inside)
    assert ups == [] and downs == [4]
    same(out.to_host(), flows[0].track(pts))
