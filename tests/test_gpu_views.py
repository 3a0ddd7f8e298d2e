"""Every DeviceFlow method on views: fields whose vectors start 0 or 8 bytes off the 16-byte grid and whose mask starts
0 .. 3 bytes off the 4-byte grid (tests/view_cases.py), inside uploaded images with poison around them, and fields 1 and 2
of a batch of an odd shape (DeviceFlowBatch.field).  For every method
  (a) the view gives the bytes its aligned twin (DeviceFlow.from_host of the same field) gives,
  (b) those are the bytes of the NumPy restatement or of the host Flow, where tests/ has one,
  (c) both whole images -- poison included -- read back unchanged afterwards.
DESIGN.md ("Where a field may start") has the contract and the route every device entry takes below its alignment."""
import functools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
from oracle import np_oracle as O
import build_ref
import consistency_ref
import error_ref
import fill_ref
import matrix_ref
import median_ref
import test_gpu_matrix as TM
import test_gpu_visualise as TV
import track_ref
import upsample_ref
import view_cases as V
import visualise_ref

pytestmark = pytest.mark.gpu
nat = of.native
F32, U8 = np.float32, np.uint8

# A Delaunay triangulation needs three points that are not on a line: a (1, 3) or (1, 1) field has none, so the scatter
# methods ('s'-reference warps, 't'-reference tracking, switch_ref, invert, valid_*, combine_with 1 / 2) have no host
# answer there (tests/scatter_admissible.py) and run on the other three shapes.
SCATTER_SHAPES = [s for s in V.SHAPES if s[0] > 1]


# ------------------------------------------------------------------------------ the views
class Case:
    """one view of a field, its aligned twin, and the check that the memory around the view is unchanged"""

    def __init__(self, tag, view, twin, images):
        self.tag, self.view, self.twin, self._images = tag, view, twin, images

    def unchanged(self):
        for buf, img in self._images:
            assert buf.to_host((img.size,), U8).tobytes() == img.tobytes(), "{}: memory around the view was written".format(self.tag)


def upload(img):
    buf = dev.DeviceBuffer.from_host(img)
    assert buf.ptr % 16 == 0
    return buf


def byte_view(arr, rm):
    """a uint8 map at an address rm (mod 4), poison around it -> (view, [(buffer, image)])"""
    p = V.place(np.zeros(arr.shape + (2,), F32), arr, 0, rm)
    buf = upload(p.mimg)
    view = buf.view(p.moff, arr.size)
    assert view.ptr % 4 == rm
    return view, [(buf, p.mimg)]


def cases(v, m, ref):
    """Cases of the field (v float32 (H, W, 2), m uint8 (H, W)): the placements its shape runs and, on the shapes that run
    all eight, fields 1 and 2 of a batch of three"""
    shape = v.shape[:2]
    n = shape[0] * shape[1]
    twin = dev.DeviceFlow.from_host(v, ref, m)
    assert twin.vecs.ptr % 16 == 0 and twin.mask.ptr % 4 == 0
    for p in V.placements(v, m, V.residues_for(shape)):
        vbuf, mbuf = upload(p.vimg), upload(p.mimg)
        view = dev.DeviceFlow(vbuf.view(p.voff, 8 * n), mbuf.view(p.moff, n), shape, ref)
        assert (view.vecs.ptr % 16, view.mask.ptr % 4) == (p.rv, p.rm)
        yield Case("{} at ({}, {})".format(shape, p.rv, p.rm), view, twin, [(vbuf, p.vimg), (mbuf, p.mimg)])
    if shape in V.FULL_SHAPES:
        yield from batch_cases(v, m, ref, twin)


def batch_cases(v, m, ref, twin):
    shape = v.shape[:2]
    n = shape[0] * shape[1]
    other_v, other_m = V.random_case(shape, seed=77)
    vimg = np.concatenate([other_v.reshape(-1), v.reshape(-1), v.reshape(-1)]).view(U8)
    mimg = np.concatenate([other_m.reshape(-1), m.reshape(-1), m.reshape(-1)])
    b = DeviceFlowBatch(3, shape, ref)
    nat.check(nat.load().ofl_upload(b.vecs.ptr, vimg.ctypes.data, vimg.size, None))
    nat.check(nat.load().ofl_upload(b.mask.ptr, mimg.ctypes.data, mimg.size, None))
    dev.sync()
    assert b.vecs.ptr % 16 == 0 and b.mask.ptr % 4 == 0
    want = {(37, 53): [(8, 1), (0, 2)], (5, 7): [(8, 3), (0, 2)]}[shape]
    for i in (1, 2):
        f = b.field(i)
        assert (f.vecs.ptr % 16, f.mask.ptr % 4) == want[i - 1]
        yield Case("{} field {} of a batch".format(shape, i), f, twin, [(b.vecs, vimg), (b.mask, mimg)])


def attempt(fn):
    """fn() -> its result, or -- for the errors arguments and degenerate fields raise -- the error as bytes, so that a view
    has to fail exactly like its twin"""
    try:
        return fn()
    except (ValueError, IndexError) as e:
        return np.frombuffer("{}: {}".format(type(e).__name__, e).encode(), U8)


def raised(a):
    return isinstance(a, np.ndarray) and a.dtype == U8 and a.ndim == 1 and a.tobytes().split(b":")[0] in (b"ValueError", b"IndexError")


def flow_bytes(f):
    if isinstance(f, np.ndarray):
        return f
    v, m = f.to_host()
    return np.concatenate([np.array(f.shape, np.uint32).view(U8), np.frombuffer(f.ref.encode(), U8), v.view(U8).reshape(-1), m.view(U8).reshape(-1)])


def host_bytes(f):
    """a host Flow in the form of flow_bytes"""
    if isinstance(f, np.ndarray):
        return f
    v = np.ascontiguousarray(f.vecs, F32)
    return np.concatenate([np.array(f.shape, np.uint32).view(U8), np.frombuffer(f.ref.encode(), U8), v.view(U8).reshape(-1),
                           np.ascontiguousarray(f.mask).view(U8).reshape(-1)])


def check(case, run, want=None):
    """(a), (b) and (c) for the dict of host arrays run(flow) returns"""
    got, twin = run(case.view), run(case.twin)
    assert list(got) == list(twin)
    for k in got:
        a, t = np.ascontiguousarray(got[k]), np.ascontiguousarray(twin[k])
        assert a.dtype == t.dtype and a.shape == t.shape, (case.tag, k)
        assert a.tobytes() == t.tobytes(), "{}: {} differs from the aligned twin".format(case.tag, k)
    for k, w in (want or {}).items():
        w = np.ascontiguousarray(w)
        a = np.ascontiguousarray(got[k])
        assert a.shape == w.shape and a.dtype.itemsize == w.dtype.itemsize, (case.tag, k, a.shape, w.shape, a.dtype, w.dtype)
        assert a.tobytes() == w.tobytes(), "{}: {} differs from the restatement".format(case.tag, k)
    case.unchanged()
    return got


@functools.lru_cache(maxsize=None)
def random_case(shape):
    v, m = V.random_case(shape)
    v.setflags(write=False)
    m.setflags(write=False)
    return v, m


@functools.lru_cache(maxsize=None)
def smooth_case(shape, ref):
    """a rotation by 9 degrees and a translation with a hole in the mask, as test_gpu_track: a regular mesh, whose scatter
    answer is defined"""
    h, w = shape
    mask = np.ones(shape, bool)
    mask[h // 4: h // 2, w // 3: 2 * w // 3] = False
    f = of.Flow.from_transforms([['rotation', (w - 1) / 2, (h - 1) / 2, 9], ['translation', 2.5, -1.75]], shape, ref, mask)
    v = np.ascontiguousarray(f.vecs, F32)
    v.setflags(write=False)
    return v, mask.astype(U8)


# ------------------------------------------------------------------------------ copies and exports
def run_transfer(f):
    c = f.copy()
    assert c.vecs.ptr != f.vecs.ptr and c.mask.ptr != f.mask.ptr
    out = {"to_host v": f.to_host()[0], "to_host m": f.to_host()[1], "copy": flow_bytes(c), "export_mask": f.export_mask().to_host()}
    for layout in ('hwc', 'chw'):
        for dtype in ('float32', 'float16'):
            out["export {} {}".format(layout, dtype)] = f.export(layout, dtype).to_host()
    return out


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_copy_to_host_and_export(gpu, shape):
    v, m = random_case(shape)
    want = {"to_host v": v, "to_host m": m, "export_mask": m, "export hwc float32": v, "export chw float32": v.transpose(2, 0, 1),
            "export hwc float16": v.astype(np.float16), "export chw float16": v.astype(np.float16).transpose(2, 0, 1)}
    for case in cases(v, m, 't'):
        check(case, run_transfer, want)


# ------------------------------------------------------------------------------ K9: scaling, padding, cropping
FACTORS = [0.3, [0.5, -2.0], np.array([3, 7])]
PADDING = [13, 0, 0, 9]
CROPS = {'[::2, ::3]': (slice(None, None, 2), slice(None, None, 3)), '[::-1, ::-1]': (slice(None, None, -1), slice(None, None, -1))}


def run_scale(f):
    out = {}
    for i, k in enumerate(FACTORS):
        out["* {}".format(i)] = flow_bytes(f * k)
        out["/ {}".format(i)] = flow_bytes(f / k)
    return out


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_multiply_and_divide(gpu, shape):
    v, m = random_case(shape)
    host = of.Flow(v, 't', m.astype(bool))
    want = {}
    for i, k in enumerate(FACTORS):
        want["* {}".format(i)] = host_bytes(host * k)
        want["/ {}".format(i)] = host_bytes(host / k)
    for case in cases(v, m, 't'):
        check(case, run_scale, want)
        assert (case.view * 2.0).mask is case.view.mask


def run_pad_crop(f):
    out = {"pad " + mode: flow_bytes(f.pad(PADDING, mode)) for mode in ('constant', 'edge', 'symmetric')}
    out.update({key: flow_bytes(f[item]) for key, item in CROPS.items()})
    return out


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_pad_and_crop(gpu, shape):
    v, m = random_case(shape)
    want = {}
    for mode in ('constant', 'edge', 'symmetric'):
        pv, pm = build_ref.pad(v, m.astype(bool), PADDING, dev._PAD_MODES[mode])
        want["pad " + mode] = host_bytes(of.Flow(pv, 't', pm))
    for key, item in CROPS.items():
        cv, cm = build_ref.crop(v, m.astype(bool), *item)
        want[key] = host_bytes(of.Flow(cv, 't', cm))
    for case in cases(v, m, 't'):
        check(case, run_pad_crop, want)


# ------------------------------------------------------------------------------ K4: resize
SCALES = [0.5, 2, 1.5, (2, 0.5)]


def resizable(shape, scale):
    fy, fx = dev.resize_scales(scale)
    return int(np.rint(shape[0] * fy)) > 0 and int(np.rint(shape[1] * fx)) > 0


def run_resize(f):
    return {"resize {}".format(s): flow_bytes(attempt(lambda: f.resize(s))) for s in SCALES}


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_resize(gpu, shape):
    v, m = random_case(shape)
    want = {}
    for s in SCALES:
        if resizable(shape, s):
            rv, rm = O.resize_flow(v, s, m.astype(bool))
            want["resize {}".format(s)] = host_bytes(of.Flow(rv, 't', rm))
    assert want
    for case in cases(v, m, 't'):
        got = check(case, run_resize, want)
        assert [raised(got["resize {}".format(s)]) for s in SCALES] == [not resizable(shape, s) for s in SCALES]


# ------------------------------------------------------------------------------ K7: visualise
RANGES = (None, 2.5)


def run_visualise(f):
    out = {"range": np.array([f.visualise_range()], np.float64)}
    for mode, sm, smb in TV.COMBOS:
        for rm in RANGES:
            img = f.visualise(mode, sm, smb, rm)
            assert img.shape == f.shape + (3,) and img.dtype == U8
            out["{} {} {} {}".format(mode, sm, smb, rm)] = img.to_host()
    return out


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_visualise(gpu, shape):
    v, m = random_case(shape)
    t = visualise_ref.thresholded(v)
    want = {"range": np.array([visualise_ref.default_range(visualise_ref.magnitude(t[..., 0], t[..., 1]))], np.float64)}
    for mode, sm, smb in TV.COMBOS:
        for rm in RANGES:
            want["{} {} {} {}".format(mode, sm, smb, rm)] = visualise_ref.visualise(v, mode, m.astype(bool), sm, smb, rm)
    for case in cases(v, m, 't'):
        check(case, run_visualise, want)


# ------------------------------------------------------------------------------ K8: the passes and Flow.matrix
FIT_FIELDS = [('holes', 's'), ('noisy', 't')]


def fit_params(shape, H):
    norm = np.array([shape[1] / 2.0, shape[0] / 2.1, 2.0 / shape[1] + 0.01, shape[1] / 1.9, shape[0] / 2.0, 2.0 / shape[0] + 0.02])
    Tn = lambda c, s: np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    Hn = Tn(norm[3:5], norm[5]) @ H @ np.linalg.inv(Tn(norm[0:2], norm[2]))
    return norm, Hn / Hn[2, 2] + 1e-3


def fit_passes(D, shape, H, n):
    """every K8 entry through the FitField D (a dev.FitField or a matrix_ref.Field of n correspondences) -> dict"""
    norm, Hn = fit_params(shape, H)
    models = TM.models_for(H, shape)
    out = {}
    for g, gate in enumerate((None, (H + 1e-5, F32(0.5)), (TM.AFFINE, F32(9.0)))):
        out["moments {}".format(g)] = D.moments(gate=gate)
        out["dlt {}".format(g)] = D.dlt(norm, gate=gate)
        out["gn {}".format(g)] = D.gn(norm, Hn, gate=gate)
    for thr in (9.0, 0.01):
        out["score {}".format(thr)] = D.score(models, F32(thr))
    if n:
        out["median"] = D.median(models, (n - 1) // 2, n // 2)
        out["median ends"] = D.median(models[:1], 0, n - 1)
    if hasattr(D, "index"):
        D.index()
    if n:
        out["pick"] = D.pick(np.concatenate([[0, n - 1, n, n + 7], np.random.default_rng(n).integers(0, n, 60)]))
    return out


@pytest.mark.parametrize("kind,ref", FIT_FIELDS)
@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_fit_passes(gpu, shape, kind, ref):
    """The float64 sums are byte-equal to the aligned twin's -- their addition order is part of K8's contract (include/ofl.h)
    -- and within the bound of that order of the exactly rounded sums of matrix_ref; counts, medians and samples are exact."""
    H = TM.make_field(kind, shape, ref)[2]
    v, m = V.matrix_case(kind, shape, ref)
    F = matrix_ref.Field(v, ref, m)
    F.exact = True
    n = F.idx.size
    sign = -1 if ref == 't' else 1
    want = fit_passes(F, shape, H, n)
    sums = {k: want.pop(k) for k in list(want) if k.split()[0] in ("moments", "dlt", "gn")}
    norm, Hn = fit_params(shape, H)
    for case in cases(v, m, ref):
        got = check(case, lambda f: fit_passes(dev.FitField(f.vecs, f.mask, shape, sign), shape, H, n), want)
        for g, gate in enumerate((None, (H + 1e-5, F32(0.5)), (TM.AFFINE, F32(9.0)))):
            for name, terms in (("moments", F.moments_terms(gate)), ("dlt", F.dlt_terms(norm, gate)), ("gn", F.gn_terms(norm, Hn, gate))):
                key = "{} {}".format(name, g)
                cols = [np.asarray(t) for t in terms]
                assert got[key].dtype == np.float64 and got[key].size == len(cols) + 1 and got[key][-1] == F.nonfinite
                for k, col in enumerate(cols):
                    bound = TM.depth(shape[0] * shape[1]) * 2.0 ** -53 * float(np.sum(np.abs(col)))
                    assert abs(got[key][k] - sums[key][k]) <= bound, (case.tag, key, k)


def run_matrix(f):
    return {"{} {}".format(dof, method): attempt(lambda: f.matrix(dof, method)) for dof, method in TM.COMBOS}


@pytest.mark.parametrize("kind,ref", FIT_FIELDS)
@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_matrix(gpu, shape, kind, ref):
    """(b): the result against matrix_ref within test_gpu_matrix.MARGIN, which that module derives for identical
    sample sets, counts and medians and a different order of the float64 sums; the view has the twin's bytes.  A field
    of fewer correspondences than a minimal set raises on both sides."""
    v, m = V.matrix_case(kind, shape, ref)
    result = None
    for case in cases(v, m, ref):
        result = check(case, run_matrix)                  # the view's, which has the twin's bytes
    for dof, method in TM.COMBOS if shape[0] > 1 else ():           # a one-row field: the view fails as its twin does, no more
        got = result["{} {}".format(dof, method)]
        try:
            want = matrix_ref.matrix(v, ref, m.astype(bool), dof=dof, method=method)
        except ValueError:
            assert raised(got), (dof, method)
            continue
        assert not raised(got) and got.dtype == np.float64 and got.shape == (3, 3), (dof, method)
        print(shape, kind, dof, method, "device vs ref", TM.reldiff(got, want))
        assert TM.reldiff(got, want) <= TM.MARGIN, (dof, method)


def test_the_calls_that_used_to_be_refused(gpu):
    """field 1 of a 37 x 53 batch times two, as an image, as a matrix"""
    v, m = V.matrix_case('holes', (37, 53), 's')
    case = list(batch_cases(v, m, 's', dev.DeviceFlow.from_host(v, 's', m)))[0]
    assert (case.view.vecs.ptr % 16, case.view.mask.ptr % 4) == (8, 1)
    check(case, lambda f: {"* 2.0": flow_bytes(f * 2.0), "rgb": f.visualise('rgb').to_host(), "matrix": f.matrix()})


def test_vectors_off_the_8_byte_grid_are_still_refused(gpu):
    """what cannot be served: a pixel is one 8-byte element.  Refused before anything is launched."""
    shape = (5, 7)
    v, m = random_case(shape)
    p = V.place(v, m, 0, 0)
    vbuf, mbuf = upload(p.vimg), upload(p.mimg)
    f = dev.DeviceFlow(vbuf.view(p.voff + 4, 8 * 35), mbuf.view(p.moff, 35), shape, 't')
    fit = dev.FitField(f.vecs, f.mask, shape, -1)
    for call, message in ((lambda: f * 2.0, "ofl_scale: vecs and out must be 8-byte aligned"),
                          (lambda: f.visualise('rgb', range_max=2.5), "ofl_visualise: flow must be 8-byte, out 4-byte aligned"),
                          (lambda: f.visualise_range(), "ofl_visualise_range: flow must be 8-byte aligned"),
                          (lambda: fit.moments(), "ofl_fit_moments: flow must be 8-byte aligned"),
                          (lambda: fit.score(np.eye(3), 1.0), "ofl_fit_score: flow must be 8-byte aligned"),
                          (lambda: fit.index(), "ofl_fit_index: flow must be 8-byte aligned")):
        with pytest.raises(nat.NativeError) as e:
            call()
        assert message in str(e.value)
    assert vbuf.to_host((p.vimg.size,), U8).tobytes() == p.vimg.tobytes() and mbuf.to_host((p.mimg.size,), U8).tobytes() == p.mimg.tobytes()


# ------------------------------------------------------------------------------ K10: tracking
def track_points(shape):
    h, w = shape
    rng = np.random.default_rng(h * w)
    inner = rng.random((67, 2)) * (np.array(shape) - 1.0)             # inside the area: 0 <= p <= size - 1
    ints = np.stack([rng.integers(0, h, 67), rng.integers(0, w, 67)], axis=-1).astype(np.int64)
    wide = rng.random((67, 2)) * (np.array(shape) + 12.0) - 6.0
    return inner, ints, wide


def run_track(f):
    inner, ints, wide = track_points(f.shape)
    if f.ref == 't':
        return {"t": f.track(wide), "t int_out": f.track(wide, int_out=True), "t ints": f.track(ints)}
    out = {"float": f.track(inner), "int_out": f.track(inner, int_out=True), "ints": f.track(ints), "ints int_out": f.track(ints, int_out=True),
           "resident": f.track(dev.DevicePoints.from_host(inner)).to_host()}
    if f.shape in SCATTER_SHAPES:
        out["exact"] = f.track(inner, s_exact_mode=True)
        pts, status = f.track(inner, get_valid_status=True)
        out["status pts"], out["status"] = pts, status
    return out


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_track_s(gpu, shape):
    v, m = smooth_case(shape, 's')
    inner, ints, _ = track_points(shape)
    want = {"float": track_ref.track(v, inner), "int_out": track_ref.track(v, inner, int_out=True), "ints": track_ref.track(v, ints),
            "ints int_out": track_ref.track(v, ints, int_out=True), "resident": track_ref.track(v, inner)}
    if shape in SCATTER_SHAPES:
        host = of.Flow(v, 's', m.astype(bool))
        want["exact"] = host.track(inner, s_exact_mode=True)
        want["status pts"], want["status"] = host.track(inner, get_valid_status=True)
    for case in cases(v, m, 's'):
        check(case, run_track, want)


@pytest.mark.parametrize("shape", SCATTER_SHAPES, ids=V.shape_id)
def test_track_t(gpu, shape):
    v, m = smooth_case(shape, 't')
    _, ints, wide = track_points(shape)
    host = of.Flow(v, 't', m.astype(bool))
    want = {"t": host.track(wide), "t int_out": host.track(wide, int_out=True), "t ints": host.track(ints)}
    for case in cases(v, m, 't'):
        check(case, run_track, want)


# ------------------------------------------------------------------------------ K1 / K12 / K3: warping
@functools.lru_cache(maxsize=None)
def warp_targets(shape):
    rng = np.random.default_rng(shape[0] * shape[1] + 1)
    img_f = rng.random(shape + (3,), dtype=F32)
    img_b = rng.integers(0, 256, shape + (3,)).astype(U8)
    tmask = (rng.random(shape) > 0.2)
    tensor = rng.standard_normal((5,) + shape).astype(F32)
    return img_f, img_b, tmask, tensor


def run_apply(f):
    img_f, img_b, tmask, tensor = warp_targets(f.shape)
    tm = dev.DeviceBuffer.from_host(tmask.view(U8))
    out = {}
    for name, img in (("float32", img_f), ("uint8", img_b)):
        if f.ref == 's' and name == "uint8":
            continue                                      # 's'-reference warps of device images take float32 only
        for masked in (False, True):
            warped, valid = f.apply(dev.DeviceImage.from_host(img), target_mask=tm if masked else None)
            out["{} {}".format(name, masked)] = warped.to_host()
            out["{} {} valid".format(name, masked)] = valid.to_host(f.shape, U8)
    if f.ref == 't':
        for masked in (False, True):
            warped, valid = f.apply_tensor(dev.DeviceTensor.from_host(tensor), tm if masked else None)
            out["tensor {}".format(masked)] = warped.to_host()
            out["tensor {} valid".format(masked)] = valid.to_host(f.shape, U8)
    return out


def apply_want(v, m, ref):
    shape = v.shape[:2]
    img_f, img_b, tmask, tensor = warp_targets(shape)
    host = of.Flow(v, ref, m.astype(bool))
    want = {}
    for name, img in (("float32", img_f), ("uint8", img_b)):
        if ref == 's' and name == "uint8":
            continue
        for masked in (False, True):
            w, valid = host.apply(img, tmask if masked else None, return_valid_area=True)
            want["{} {}".format(name, masked)], want["{} {} valid".format(name, masked)] = w, valid
    if ref == 't':
        for masked in (False, True):
            planes = [host.apply(np.ascontiguousarray(tensor[c]), tmask if masked else None, return_valid_area=True) for c in range(tensor.shape[0])]
            want["tensor {}".format(masked)] = np.stack([p[0] for p in planes])
            want["tensor {} valid".format(masked)] = planes[0][1]
    return want


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_apply_t(gpu, shape):
    """the gather kernels: a random field (every tap pattern) and the smooth one"""
    for v, m in (random_case(shape), smooth_case(shape, 't')):
        want = apply_want(v, m, 't')
        for case in cases(v, m, 't'):
            check(case, run_apply, want)


@pytest.mark.parametrize("shape", SCATTER_SHAPES, ids=V.shape_id)
def test_apply_s(gpu, shape):
    v, m = smooth_case(shape, 's')
    want = apply_want(v, m, 's')
    for case in cases(v, m, 's'):
        check(case, run_apply, want)


# ------------------------------------------------------------------------------ the flow algebra over gather, scatter and compose
@functools.lru_cache(maxsize=None)
def partner(shape, ref):
    h, w = shape
    f = of.Flow.from_transforms([['scaling', (w - 1) / 2, (h - 1) / 2, 1.1], ['translation', -1.5, 0.75]], shape, ref,
                                np.random.default_rng(h + w).random(shape) > 0.1)
    return f


def run_algebra(f):
    p = partner(f.shape, f.ref).to_device()
    out = {"switch_ref": flow_bytes(f.switch_ref()), "invert": flow_bytes(f.invert()), "invert other": flow_bytes(f.invert('s' if f.ref == 't' else 't')),
           "valid_source": f.valid_source().to_host(f.shape, U8), "valid_target": f.valid_target().to_host(f.shape, U8),
           "apply flow": flow_bytes(f.apply(p)), "applied by": flow_bytes(p.apply(f))}
    for mode in (1, 2, 3):
        out["combine {} self".format(mode)] = flow_bytes(f.combine_with(p, mode))
        out["combine {} arg".format(mode)] = flow_bytes(p.combine_with(f, mode))
    return out


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("shape", SCATTER_SHAPES, ids=V.shape_id)
def test_flow_algebra(gpu, shape, ref):
    v, m = smooth_case(shape, ref)
    host, p = of.Flow(v, ref, m.astype(bool)), partner(shape, ref)
    want = {"switch_ref": host_bytes(host.switch_ref()), "invert": host_bytes(host.invert()),
            "invert other": host_bytes(host.invert('s' if ref == 't' else 't')),
            "valid_source": host.valid_source(), "valid_target": host.valid_target(),
            "apply flow": host_bytes(host.apply(p)), "applied by": host_bytes(p.apply(host))}
    for mode in (1, 2, 3):
        want["combine {} self".format(mode)] = host_bytes(host.combine_with(p, mode))
        want["combine {} arg".format(mode)] = host_bytes(p.combine_with(host, mode))
    for case in cases(v, m, ref):
        check(case, run_algebra, want)


# ------------------------------------------------------------------------------ K13 - K17
@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_consistency_and_error(gpu, shape):
    """the view once as the first and once as the second operand"""
    f, fm, b, bm = consistency_ref.pair(3, shape, -1)
    fm, bm = fm.astype(U8), bm.astype(U8)
    want, sums = {}, {}
    for name, (x, xm, y, ym) in (("first", (f, fm, b, bm)), ("second", (b, bm, f, fm))):
        consistent, covered, residual, counts = consistency_ref.consistency(x, xm, y, ym, -1)
        want[name + " consistent"], want[name + " covered"], want[name + " residual"] = consistent, covered, residual
        want[name + " counts"] = np.array(counts, np.int64)
        e = error_ref.flow_error(x, xm, y, ym)
        want[name + " error words"] = np.array(error_ref.record_words(e), np.uint32)
        want[name + " epe_map"], want[name + " outlier_map"] = e["epe_map"], e["outlier_map"]
        sums[name] = error_ref.record_sums(e)
    other = dev.DeviceFlow.from_host(b, 't', bm)

    def run(x):
        out = {}
        for name, (a, c) in (("first", (x, other)), ("second", (other, x))):
            consistent, covered, residual, counts = a.consistency(c, return_residual=True, return_counts=True)
            out[name + " consistent"], out[name + " covered"] = consistent.to_host(shape, U8), covered.to_host(shape, U8)
            out[name + " residual"], out[name + " counts"] = residual.to_host(shape, F32), np.array(counts, np.int64)
            e = a.error(c, [float(t) for t in error_ref.THR], (float(error_ref.OUT_ABS), float(error_ref.OUT_REL)),
                        [float(t) for t in error_ref.EDGES], return_map=True, return_outliers=True)
            rec = e.read_records()[0].tobytes()
            out[name + " error words"] = np.frombuffer(rec[:48], np.uint32)
            out[name + " error sums"] = np.frombuffer(rec[48:], np.uint64)
            out[name + " epe_map"], out[name + " outlier_map"] = e.epe_map.to_host(shape, F32), e.outlier_map.to_host(shape, U8)
        return out

    for case in cases(f, fm, 't'):
        got = check(case, run, want)
        for name in ("first", "second"):                  # the float64 sums: the twin's bytes, and within the bound of their order
            for g, x in zip(got[name + " error sums"].view(np.float64), sums[name]):
                assert abs(g - x) <= error_ref.depth(shape[0] * shape[1]) * 2.0 ** -53 * x, (case.tag, name)


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_fill_and_median(gpu, shape):
    """`valid` and `only` are views at odd addresses too"""
    v, m = random_case(shape)
    rng = np.random.default_rng(shape[0] + shape[1])
    valid, only = (rng.random(shape) > 0.3).astype(U8), (rng.random(shape) > 0.4).astype(U8)
    want = {}
    for name, val in (("plain", None), ("valid", valid)):
        fv, fmask, index, d2 = fill_ref.fill(v, m, val, 25)
        want["fill " + name] = host_bytes(of.Flow(fv, 't', fmask.astype(bool)))
        want["fill {} index".format(name)], want["fill {} d2".format(name)] = index, d2
    for ksize in (3, 5, 7):
        mv, mm, _ = median_ref.median(v, m, ksize, valid, only, 2)
        want["median {}".format(ksize)] = host_bytes(of.Flow(mv, 't', mm.astype(bool)))
    mv, mm, _ = median_ref.median(v, m, 5)
    want["median plain"] = host_bytes(of.Flow(mv, 't', mm.astype(bool)))
    for case in cases(v, m, 't'):
        rm = case.view.mask.ptr % 4
        (valid_view, images_a), (only_view, images_b) = byte_view(valid, rm), byte_view(only, (rm + 2) % 4 | 1)
        valid_twin, only_twin = dev.DeviceBuffer.from_host(valid), dev.DeviceBuffer.from_host(only)

        def run(f):
            val, onl = (valid_view, only_view) if f is case.view else (valid_twin, only_twin)
            out = {}
            for name, x in (("plain", None), ("valid", val)):
                filled, index, d2 = f.fill(x, 5, return_index=True, return_d2=True)
                out["fill " + name] = flow_bytes(filled)
                out["fill {} index".format(name)], out["fill {} d2".format(name)] = index.to_host(shape, np.int32), d2.to_host(shape, np.uint32)
            for ksize in (3, 5, 7):
                out["median {}".format(ksize)] = flow_bytes(f.median(ksize, val, onl, 2))
            out["median plain"] = flow_bytes(f.median())
            return out

        check(case, run, want)
        for buf, img in images_a + images_b:
            assert buf.to_host((img.size,), U8).tobytes() == img.tobytes(), case.tag


@pytest.mark.parametrize("shape", V.SHAPES, ids=V.shape_id)
def test_upsample_convex(gpu, shape):
    v, m = upsample_ref.vectors(shape), upsample_ref.coarse_mask(shape)
    want, weights = {}, {}
    for f in (2, 8):
        x = upsample_ref.logits(shape, f, 20.0)
        weights[f] = dev.DeviceTensor.from_host(x)
        uv, um = upsample_ref.upsample(v, m, x, f)
        want["x{}".format(f)] = host_bytes(of.Flow(uv, 't', um.astype(bool)))
    for case in cases(v, m, 't'):
        check(case, lambda fl: {"x{}".format(f): flow_bytes(fl.upsample_convex(weights[f], f)) for f in (2, 8)}, want)
