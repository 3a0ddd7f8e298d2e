"""K14 (ofl_error.hip): an estimated field against a ground truth on the device, against tests/error_ref.py and through every
layer: the raw ABI, DeviceFlow.error, DeviceFlowBatch.error, Flow.error and flow_error.  Counts, the maximum's bits and both
maps are compared with array_equal; the float64 sums within depth(H * W) * 2^-53 * sum of the correctly rounded sum (the
bound of their fixed addition order, include/ofl.h) -- there is no other tolerance here."""
import itertools
import math
import os

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
from oflibnumpy_amd.kernels import ERROR_RECORD
from devmem import guarded, read_guarded
import error_ref as E

pytestmark = pytest.mark.gpu
nat = of.native
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 64


def up(a):
    a = np.ascontiguousarray(a)
    return dev.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype == np.bool_ else a)


def workspace(shape, batch):
    n = dev._size_query(nat.load().ofl_flow_error_workspace_bytes, shape[0], shape[1], batch)
    assert n == batch * -(-shape[0] * shape[1] // E.CHUNK) * 96
    return dev.DeviceBuffer(n), n


def raw_call(ptrs, shape, batch=1, est_mask=True, epe_map=True, outlier_map=True, thr=E.THR, out=(E.OUT_ABS, E.OUT_REL), edges=E.EDGES,
             map_shift=(0, 0)):
    """ofl_flow_error_dev on device addresses (est, em, gt, gm) -> (records, epe_map | None, outlier_map | None) on the host.
    The maps are written into 0xA5-filled buffers (at byte offset map_shift into them) whose bytes behind the map must stay."""
    h, w = shape
    n = batch * h * w
    est, em, gt, gm = ptrs
    work, nbytes = workspace(shape, batch)
    rec = dev.DeviceBuffer(batch * 96)
    d_epe = guarded(n * 4, GUARD, map_shift[0]) if epe_map else None
    d_out = guarded(n, GUARD, map_shift[1]) if outlier_map else None
    thr, edges = np.ascontiguousarray(thr, np.float32), np.ascontiguousarray(edges, np.float32)
    nat.check(nat.load().ofl_flow_error_dev(est, em if est_mask else None, gt, gm, h, w, batch, thr.ctypes.data, np.float32(out[0]),
                                            np.float32(out[1]), edges.ctypes.data, work.ptr, nbytes, rec.ptr,
                                            d_epe.ptr + map_shift[0] if epe_map else None, d_out.ptr + map_shift[1] if outlier_map else None, None))
    full = (batch, h, w) if batch > 1 else (h, w)
    res = [rec.to_host((batch,), ERROR_RECORD), None, None]
    for k, (buf, size, shift, dtype) in enumerate(((d_epe, n * 4, map_shift[0], np.float32), (d_out, n, map_shift[1], np.uint8))):
        if buf is not None:
            res[k + 1] = read_guarded(buf, shift, size, GUARD, dtype, full)
    return tuple(res)


def check_record(rec, want, n_px, what):
    words = rec.tobytes()[:48]
    assert np.frombuffer(words, np.uint32).tolist() == E.record_words(want), what
    got = [float(rec["sum_epe"]), float(rec["sum_epe2"])] + [float(v) for v in rec["sum_bin_epe"]]
    for name, g, x in zip(("sum_epe", "sum_epe2", "bin0", "bin1", "bin2", "bin3"), got, E.record_sums(want)):
        bound = E.depth(n_px) * 2.0 ** -53 * x
        print(what, name, "diff", abs(g - x), "bound", bound)
        assert abs(g - x) <= bound, (what, name)


def host_bytes(a):
    return a.view(np.uint8) if a.dtype == np.bool_ else a


# ---------------------------------------------------------------------------------------------- 1: the raw ABI against the restatement
@pytest.mark.parametrize("shape", E.SHAPES)
def test_raw_entry_against_the_reference(gpu, shape):
    n_px = shape[0] * shape[1]
    inputs, _ = E.case(1, shape)
    bufs = [up(a) for a in inputs]
    ptrs = [b.ptr for b in bufs]
    for with_em, with_epe, with_out in itertools.product((True, False), repeat=3):
        _, want = E.case(1, shape, with_em)
        what = "{} est_mask {} epe_map {} outlier_map {}".format(shape, with_em, with_epe, with_out)
        rec, g_epe, g_out = raw_call(ptrs, shape, est_mask=with_em, epe_map=with_epe, outlier_map=with_out)
        check_record(rec[0], want, n_px, what)
        assert (g_epe is None) == (not with_epe) and (g_out is None) == (not with_out)
        if with_epe:
            np.testing.assert_array_equal(g_epe.view(np.uint32), want["epe_map"].view(np.uint32), err_msg=what)
        if with_out:
            np.testing.assert_array_equal(g_out, want["outlier_map"], err_msg=what)
    for buf, a in zip(bufs, inputs):                                   # the inputs are unchanged
        np.testing.assert_array_equal(buf.to_host(a.shape, host_bytes(a).dtype), host_bytes(a))


# ---------------------------------------------------------------------------------------------- 2: determinism, path independence
def test_two_calls_return_identical_bytes(gpu):
    shape = (40, 392)
    bufs = [up(a) for a in E.case(2, shape)[0]]
    ptrs = [b.ptr for b in bufs]
    a, b = raw_call(ptrs, shape), raw_call(ptrs, shape)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("shape", [(5, 7), (17, 241)])
def test_three_pairs_in_one_launch_equal_three_launches(gpu, shape):
    """an odd pixel count: in one launch every second pair sits 8 bytes off the 16-byte grid (the generic path), alone on a
    fresh buffer each pair takes the wide path -- and the records agree byte for byte, the doubles included"""
    n_px = shape[0] * shape[1]
    assert n_px % 4 != 0
    cases = [E.case(seed, shape) for seed in (1, 2, 3)]
    stacked = [up(np.stack([c[0][k] for c in cases])) for k in range(4)]
    rec, g_epe, g_out = raw_call([b.ptr for b in stacked], shape, batch=3)
    for i, (inputs, want) in enumerate(cases):
        single = [up(a) for a in inputs]
        assert all(b.ptr % 16 == 0 for b in single)
        s_rec, s_epe, s_out = raw_call([b.ptr for b in single], shape)
        assert rec[i].tobytes() == s_rec[0].tobytes(), i
        np.testing.assert_array_equal(g_epe[i].view(np.uint32), s_epe.view(np.uint32))
        np.testing.assert_array_equal(g_out[i], s_out)
        check_record(rec[i], want, n_px, "pair {}".format(i))
        np.testing.assert_array_equal(g_epe[i].view(np.uint32), want["epe_map"].view(np.uint32))
        np.testing.assert_array_equal(g_out[i], want["outlier_map"])


@pytest.mark.parametrize("shape", [(19, 70), (40, 392)])
def test_unaligned_even_width_takes_the_generic_path(gpu, shape):
    """an even width whose masks and maps sit at odd addresses, and whose vectors sit 8 bytes off the 16-byte grid, cannot use
    the wide loads: the same bytes come back"""
    n = shape[0] * shape[1]
    inputs, want = E.case(3, shape)
    est, em, gt, gm = [up(a) for a in inputs]
    lib = nat.load()
    aligned = raw_call([est.ptr, em.ptr, gt.ptr, gm.ptr], shape)
    s_est, s_gt, s_em, s_gm = dev.DeviceBuffer(n * 8 + 8), dev.DeviceBuffer(n * 8 + 8), dev.DeviceBuffer(n + 1), dev.DeviceBuffer(n + 3)
    nat.check(lib.ofl_copy_dev(s_est.ptr + 8, est.ptr, n * 8, None))
    nat.check(lib.ofl_copy_dev(s_gt.ptr + 8, gt.ptr, n * 8, None))
    nat.check(lib.ofl_copy_dev(s_em.ptr + 1, em.ptr, n, None))
    nat.check(lib.ofl_copy_dev(s_gm.ptr + 3, gm.ptr, n, None))
    assert (s_est.ptr + 8) % 16 == 8 and (s_em.ptr + 1) % 2 == 1 and (s_gm.ptr + 3) % 2 == 1
    for ptrs, shift in (([est.ptr, s_em.ptr + 1, gt.ptr, s_gm.ptr + 3], (0, 0)),            # the masks alone
                        ([s_est.ptr + 8, em.ptr, s_gt.ptr + 8, gm.ptr], (0, 0)),            # the vectors alone
                        ([est.ptr, em.ptr, gt.ptr, gm.ptr], (4, 1)),                        # the maps alone
                        ([s_est.ptr + 8, s_em.ptr + 1, s_gt.ptr + 8, s_gm.ptr + 3], (12, 3))):
        shifted = raw_call(ptrs, shape, map_shift=shift)
        assert shifted[0].tobytes() == aligned[0].tobytes()
        assert shifted[1].tobytes() == aligned[1].tobytes() and shifted[2].tobytes() == aligned[2].tobytes()
    check_record(aligned[0][0], want, n, "aligned")
    np.testing.assert_array_equal(aligned[1].view(np.uint32), want["epe_map"].view(np.uint32))
    np.testing.assert_array_equal(aligned[2], want["outlier_map"])


# ---------------------------------------------------------------------------------------------- 3: the methods
def make_batch(vecs, masks, ref):
    n, h, w = masks.shape
    b = DeviceFlowBatch(n, (h, w), ref)
    v, m = np.ascontiguousarray(vecs, np.float32), np.ascontiguousarray(masks).view(np.uint8)
    nat.check(nat.load().ofl_upload(b.vecs.ptr, v.ctypes.data, v.nbytes, None))
    nat.check(nat.load().ofl_upload(b.mask.ptr, m.ctypes.data, m.nbytes, None))
    dev.sync()
    return b


def finite_case(seed, shape):
    """a generated case without its NaN / Inf vectors (a Flow refuses them); the two overflowing pixels stay"""
    est, em, gt, gm = E.case(seed, shape)[0]
    fix = lambda a: np.where(np.isfinite(a), a, np.float32(2)).astype(np.float32)
    return fix(est), em, fix(gt), gm


def close(got, want, n_px):
    """a mean or its root: the device's sum within its addition-order bound, plus one rounding each for the restated sum, the
    division on either side and the square root"""
    if isinstance(want, float) and math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= (E.depth(n_px) + 4) * 2.0 ** -53 * abs(want)


def check_stats(s, want, n_px, n_thr=3, n_edges=2):
    x = E.stats(want, n_thr, n_edges)
    assert (s.n, s.n_nonfinite) == (x["n"], x["n_nonfinite"])
    assert repr((s.max, s.over, s.outlier)) == repr((x["max"], x["over"], x["outlier"]))        # from integers: exact
    assert close(s.epe, x["epe"], n_px) and close(s.rmse, x["rmse"], n_px)
    assert len(s.bins) == len(x["bins"]) == n_edges + 1
    for (gn, gmean), (xn, xmean) in zip(s.bins, x["bins"]):
        assert gn == xn and close(gmean, xmean, n_px)


SETTINGS = [dict(), dict(thresholds=(0.5, 2, 4, 8), outlier=(1.5, 0.1), speed_edges=(5, 20, 90)), dict(thresholds=(2,), speed_edges=())]


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("kw", SETTINGS)
def test_all_layers_agree(gpu, ref, kw):
    shape = (40, 392)
    n_px = shape[0] * shape[1]
    seeds = (1, 2, 3)
    cases = [finite_case(seed, shape) for seed in seeds]
    thr, (out_abs, out_rel), edges, n_thr, n_edges = dev.error_args(**kw)
    for use_em in (True, False):
        wants = [E.flow_error(est, em, gt, gm, thr, out_abs, out_rel, edges, use_est_mask=use_em) for est, em, gt, gm in cases]
        est_b = make_batch(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), ref)
        gt_b = make_batch(np.stack([c[2] for c in cases]), np.stack([c[3] for c in cases]), ref)
        res = est_b.error(gt_b, use_est_mask=use_em, return_map=True, return_outliers=True, **kw)
        assert isinstance(res, dev.DeviceFlowError) and res.epe_map is not None and res.outlier_map is not None
        batch_stats = res.read()
        maps, outs = res.epe_map.to_host((3,) + shape, np.float32), res.outlier_map.to_host((3,) + shape, np.uint8)
        assert isinstance(batch_stats, list) and len(batch_stats) == 3
        plain = est_b.error(gt_b, use_est_mask=use_em, **kw)
        assert plain.epe_map is None and plain.outlier_map is None and plain.read() == batch_stats
        for i, ((est, em, gt, gm), want) in enumerate(zip(cases, wants)):
            d_est, d_gt = dev.DeviceFlow.from_host(est, ref, em), dev.DeviceFlow.from_host(gt, ref, gm)
            one = d_est.error(d_gt, use_est_mask=use_em, return_map=True, return_outliers=True, **kw)
            s = one.read()
            assert isinstance(s, of.FlowErrorStats) and s == batch_stats[i]
            check_stats(s, want, n_px, n_thr, n_edges)
            np.testing.assert_array_equal(one.epe_map.to_host(shape, np.float32).view(np.uint32), want["epe_map"].view(np.uint32))
            np.testing.assert_array_equal(one.outlier_map.to_host(shape, np.uint8), want["outlier_map"])
            np.testing.assert_array_equal(maps[i].view(np.uint32), want["epe_map"].view(np.uint32))
            np.testing.assert_array_equal(outs[i], want["outlier_map"])
            assert one.read_records()[0].tobytes() == res.read_records()[i].tobytes()
            h, h_map = of.Flow(est, ref, em).error(of.Flow(gt, ref, gm), use_est_mask=use_em, return_map=True, **kw)
            assert h == s and h_map.dtype == np.float32 and h_map.shape == shape
            np.testing.assert_array_equal(h_map.view(np.uint32), want["epe_map"].view(np.uint32))
            assert of.Flow(est, ref, em).error(of.Flow(gt, ref, gm), use_est_mask=use_em, **kw) == s
            # arrays in: the estimate carries no mask
            a = of.flow_error(est, gt, ref, gm, **kw)
            assert a == of.Flow(est, ref, em).error(of.Flow(gt, ref, gm), use_est_mask=False, **kw)
            if not use_em:
                assert a == s
                a2, a_map = of.flow_error(est, gt, ref, gm, return_map=True, **kw)
                assert a2 == s
                np.testing.assert_array_equal(a_map.view(np.uint32), want["epe_map"].view(np.uint32))
            # the inputs of the device call are unchanged
            v, m = d_est.to_host()
            assert np.array_equal(v, est) and np.array_equal(m, em)
            v, m = d_gt.to_host()
            assert np.array_equal(v, gt) and np.array_equal(m, gm)


def test_an_empty_evaluation_set_reads_as_nan(gpu):
    import warnings
    est, em, gt, gm = finite_case(1, (19, 70))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = dev.DeviceFlow.from_host(est, 't', em).error(dev.DeviceFlow.from_host(gt, 't', np.zeros_like(gm))).read()
        h = of.Flow(est, 't', em).error(of.Flow(gt, 't', np.zeros_like(gm)))
    assert s == h and s.n == 0 and s.n_nonfinite == 0
    assert all(math.isnan(v) for v in (s.epe, s.rmse, s.max, s.outlier) + s.over) and all(b[0] == 0 and math.isnan(b[1]) for b in s.bins)
    no_gt_mask = of.flow_error(est, gt, 't')                      # gt_mask None: all valid
    assert no_gt_mask.n + no_gt_mask.n_nonfinite == 19 * 70 and no_gt_mask.n_nonfinite == 2


def test_method_errors(gpu):
    f = dev.DeviceFlow.zero((6, 9), 't')
    with pytest.raises(ValueError, match="'t'.*'s'"):
        f.error(dev.DeviceFlow.zero((6, 9), 's'))
    with pytest.raises(ValueError, match=r"\(6, 9\).*\(6, 10\)"):
        f.error(dev.DeviceFlow.zero((6, 10), 't'))
    with pytest.raises(TypeError):
        f.error(of.Flow.zero((6, 9), 't'))
    with pytest.raises(ValueError):
        f.error(f, thresholds=-1)
    with pytest.raises(ValueError):
        f.error(f, speed_edges=(40, 10))
    with pytest.raises(TypeError):
        f.error(f, outlier=True)
    b = make_batch(np.zeros((2, 6, 9, 2)), np.ones((2, 6, 9), bool), 't')
    with pytest.raises(TypeError):
        b.error(f)
    with pytest.raises(ValueError):
        b.error(make_batch(np.zeros((3, 6, 9, 2)), np.ones((3, 6, 9), bool), 't'))
    with pytest.raises(ValueError):
        b.error(make_batch(np.zeros((2, 6, 9, 2)), np.ones((2, 6, 9), bool), 's'))
    with pytest.raises(ValueError):
        b.error(b, thresholds=(1, 2, 3, 4, 5))
    s = f.error(f).read()
    assert (s.n, s.epe, s.rmse, s.max, s.over, s.outlier) == (54, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0), 0.0) and s.bins[0] == (54, 0.0)


# ---------------------------------------------------------------------------------------------- 4: the shipped fixtures
@pytest.mark.parametrize("name", ["kitti", "sintel"])
def test_shipped_ground_truth(gpu, name):
    if name == "kitti":
        gt = of.Flow.from_kitti(os.path.join(GOLDEN, "kitti.png"), load_valid=True)
    else:
        gt = of.Flow.from_sintel(os.path.join(GOLDEN, "sintel.flo"), os.path.join(GOLDEN, "sintel_invalid.png"))
    h, w = gt.shape
    gv, gm = np.ascontiguousarray(gt.vecs, np.float32), np.asarray(gt.mask, bool)
    assert 0 < gm.sum() < h * w, "the fixture has valid and invalid pixels"
    rng = np.random.default_rng(11)
    est = (gv + rng.standard_normal((h, w, 2)) * rng.choice(np.array([0.2, 1.0, 4.0]), (h, w, 1))).astype(np.float32)
    valid = np.flatnonzero(gm)
    planted = rng.choice(valid, 5, replace=False)
    est.reshape(-1, 2)[planted[:3], 0] = np.nan
    est.reshape(-1, 2)[planted[3:], 1] = np.inf
    est.reshape(-1, 2)[np.flatnonzero(~gm)[:2]] = np.nan                  # outside the ground truth's mask: not counted
    thr, (out_abs, out_rel), edges, n_thr, n_edges = dev.error_args()
    want = E.flow_error(est, None, gv, gm, thr, out_abs, out_rel, edges)
    res = dev.DeviceFlow.from_host(est, gt.ref).error(gt.to_device(), return_outliers=True)
    rec, s = res.read_records()[0], res.read()
    assert np.frombuffer(rec.tobytes()[:48], np.uint32).tolist() == E.record_words(want)
    assert s.n == int(gm.sum()) - 5 and s.n_nonfinite == 5
    check_stats(s, want, h * w)
    np.testing.assert_array_equal(res.outlier_map.to_host((h, w), np.uint8), want["outlier_map"])
    print(name, (h, w), s)


# ---------------------------------------------------------------------------------------------- 5: errors of the raw entry
def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    h, w = 6, 9
    n = h * w
    vec, msk = dev.DeviceBuffer.zeros(n * 8), dev.DeviceBuffer.zeros(n)
    work, nbytes = workspace((h, w), 1)
    rec = dev.DeviceBuffer(96)
    nat.check(lib.ofl_memset(rec.ptr, 7, 96, None))
    nan, inf = np.float32('nan'), np.float32('inf')

    def call(est=vec.ptr, gt=vec.ptr, gm=msk.ptr, h=h, w=w, batch=1, thr=(1, 3, 5, inf), out=(3, 0.05), edges=(10, 40, inf),
             ws=work.ptr, ws_bytes=nbytes, records=rec.ptr, thr_null=False, edges_null=False):
        t, e = np.array(thr, np.float32), np.array(edges, np.float32)
        return lib.ofl_flow_error_dev(est, None, gt, gm, h, w, batch, None if thr_null else t.ctypes.data, np.float32(out[0]), np.float32(out[1]),
                                      None if edges_null else e.ctypes.data, ws, ws_bytes, records, None, None, None)

    for kw in (dict(gm=None), dict(est=None), dict(gt=None), dict(records=None), dict(ws=None), dict(thr_null=True), dict(edges_null=True),
               dict(edges=(40, 10, inf)), dict(edges=(10, inf, 40)), dict(edges=(nan, 40, inf)), dict(edges=(-1, 40, inf)),
               dict(thr=(1, nan, 5, inf)), dict(thr=(-1, 3, 5, inf)), dict(out=(nan, 0.05)), dict(out=(3, -0.05)),
               dict(ws_bytes=nbytes - 1), dict(ws_bytes=0), dict(batch=0), dict(batch=65536), dict(h=0), dict(w=-1),
               dict(h=65536, w=32768), dict(est=vec.ptr + 4), dict(ws=work.ptr + 4)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_flow_error" in nat.last_error(), kw
    size = dev.ctypes.c_size_t(0)
    assert lib.ofl_flow_error_workspace_bytes(0, 9, 1, dev.ctypes.byref(size)) == nat.E_INVALID
    assert lib.ofl_flow_error_workspace_bytes(6, 9, 1, None) == nat.E_INVALID
    dev.sync()
    assert (rec.to_host((96,), np.uint8) == 7).all()                     # nothing was launched
    assert call() == nat.OK
    got = rec.to_host((1,), ERROR_RECORD)[0]
    assert got.tobytes() == np.zeros(1, ERROR_RECORD).tobytes()          # empty masks: nothing is evaluated
