"""CPU suite: the host half of the flow-error evaluation (K14) -- args.error_args, the argument checks of Flow.error and
flow_error -- and the NumPy restatement tests/error_ref.py: its known answers, and the reach of the generated cases that
test_gpu_error.py compares the kernel with, shown from the restatement alone."""
import math

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import args
from oflibnumpy_amd.kernels import ERROR_RECORD, FlowErrorStats
import error_ref as E

INF = np.float32(np.inf)


# ---------------------------------------------------------------------------------------------- error_args
def test_error_args_defaults_and_padding():
    thr, (out_abs, out_rel), edges, n_thr, n_edges = args.error_args()
    assert thr.dtype == edges.dtype == np.float32 and thr.shape == (4,) and edges.shape == (3,)
    assert thr.tolist() == [1, 3, 5, INF] and edges.tolist() == [10, 40, INF] and (n_thr, n_edges) == (3, 2)
    assert (out_abs, out_rel) == (np.float32(3), np.float32(0.05)) and type(out_abs) is type(out_rel) is np.float32
    thr, out, edges, n_thr, n_edges = args.error_args((0.5,), (2, 0.1), ())
    assert thr.tolist() == [0.5, INF, INF, INF] and edges.tolist() == [INF, INF, INF] and (n_thr, n_edges) == (1, 0)
    assert out == (np.float32(2), np.float32(0.1))
    thr, out, edges, n_thr, n_edges = args.error_args([8, 1, 3, 5], [0, 0], np.array([10.0, 40.0, 90.0]))
    assert thr.tolist() == [8, 1, 3, 5] and edges.tolist() == [10, 40, 90] and (n_thr, n_edges) == (4, 3)      # thresholds need no order
    assert args.error_args(2)[0].tolist() == [2, INF, INF, INF] and args.error_args(speed_edges=np.float32(7))[2].tolist() == [7, INF, INF]
    assert args.error_args(thresholds=(INF,))[0].tolist() == [INF] * 4 and args.error_args(speed_edges=(3, 3))[2].tolist() == [3, 3, INF]
    assert args.error_args(thresholds=(np.int64(2), np.float32(0.25)))[0].tolist() == [2, 0.25, INF, INF]


@pytest.mark.parametrize("bad", [True, np.True_, "1", b"1", [True], ["1"], (1, "3"), [[1, 2]], 1j, [1j], object(), {1, 2}, {1: 2}, [None]])
def test_error_args_type_errors(bad):
    for name in ("thresholds", "speed_edges"):
        with pytest.raises(TypeError):
            args.error_args(**{name: bad})


@pytest.mark.parametrize("bad", [True, "3", 3, 3.0, [True, 0.05], (3, "0.05"), object(), [None, 1]])
def test_error_args_outlier_type_errors(bad):
    with pytest.raises(TypeError):
        args.error_args(outlier=bad)


@pytest.mark.parametrize("bad", [-1, [1, -1e-9], float('nan'), (1, np.float32('nan')), -INF, [1, 2, 3, 4, 5], np.zeros((2, 2))])
def test_error_args_value_errors(bad):
    with pytest.raises(ValueError):
        args.error_args(thresholds=bad)
    if not (isinstance(bad, list) and len(bad) == 2):
        with pytest.raises(ValueError):
            args.error_args(outlier=bad if isinstance(bad, (list, tuple, np.ndarray)) else (bad, 0.05))


@pytest.mark.parametrize("bad", [-1, [10, -40], float('nan'), [1, 2, 3, 4], [40, 10], (10, 40, 39.5), (INF, 5)])
def test_error_args_edge_value_errors(bad):
    with pytest.raises(ValueError):
        args.error_args(speed_edges=bad)


@pytest.mark.parametrize("bad", [(3,), (3, 0.05, 1), (-3, 0.05), (3, float('nan')), ()])
def test_error_args_outlier_value_errors(bad):
    with pytest.raises(ValueError):
        args.error_args(outlier=bad)


def test_host_entry_points_check_arguments_before_the_device():
    """Flow.error and flow_error raise for bad arguments without a device (this suite has none)"""
    f = of.Flow.zero((4, 6), 't')
    with pytest.raises(TypeError):
        f.error(np.zeros((4, 6, 2)))
    with pytest.raises(TypeError):
        f.error(f, thresholds=True)
    with pytest.raises(TypeError):
        f.error(f, return_map=1)
    with pytest.raises(TypeError):
        f.error(f, use_est_mask=0)
    with pytest.raises(ValueError):
        f.error(f, thresholds=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError):
        f.error(f, speed_edges=(40, 10))
    with pytest.raises(ValueError):
        f.error(f, outlier=(3, float('nan')))
    with pytest.raises(ValueError, match="4, 6.*5, 6"):
        f.error(of.Flow.zero((5, 6), 't'))
    with pytest.raises(ValueError, match="'t'.*'s'"):
        f.error(of.Flow.zero((4, 6), 's'))
    with pytest.raises(ValueError):
        of.flow_error(np.zeros((4, 6, 2)), np.zeros((4, 6, 2)), 't', thresholds=-1)
    with pytest.raises(TypeError):
        of.flow_error(np.zeros((4, 6, 2)), np.zeros((4, 6, 2)), 't', outlier=3)
    assert 'flow_error' in of.flow_operations.__all__ and of.flow_error is of.flow_operations.flow_error


# ---------------------------------------------------------------------------------------------- the record and its statistics
def as_record(want):
    r = np.zeros(1, ERROR_RECORD)
    for name in ("n", "n_nonfinite", "n_over", "n_outlier", "n_bin", "max_epe_bits", "sum_epe", "sum_epe2", "sum_bin_epe"):
        r[name] = want[name]
    return r[0]


def test_record_layout():
    assert ERROR_RECORD.itemsize == 96 and ERROR_RECORD.fields["sum_epe"][1] == 48 and ERROR_RECORD.fields["max_epe_bits"][1] == 44
    assert ERROR_RECORD.names == ("n", "n_nonfinite", "n_over", "n_outlier", "n_bin", "max_epe_bits", "sum_epe", "sum_epe2", "sum_bin_epe")


def test_identical_fields_give_all_zeros():
    (est, em, gt, gm), _ = E.case(1, (19, 70))
    finite = np.where(np.isfinite(gt), gt, np.float32(1))
    want = E.flow_error(finite, gm, finite, gm)
    n = int(gm.sum())
    assert E.record_words(want) == [n, 0, 0, 0, 0, 0, 0] + want["n_bin"] + [0] and sum(want["n_bin"]) == n
    assert E.record_sums(want) == [0.0] * 6 and not want["epe_map"].any() and not want["outlier_map"].any()
    s = FlowErrorStats(as_record(want), 4, 3)
    assert (s.n, s.n_nonfinite, s.epe, s.rmse, s.max, s.over, s.outlier) == (n, 0, 0.0, 0.0, 0.0, (0.0,) * 4, 0.0)
    assert [b[0] for b in s.bins] == want["n_bin"] and all(b[1] == 0.0 for b in s.bins)


def test_constant_offset_3_4():
    """est = gt + (3, 4) on small integers (every difference exact): epe = 5 everywhere"""
    rng = np.random.default_rng(5)
    gt = rng.integers(-20, 21, (13, 17, 2)).astype(np.float32)
    est = gt + np.array([3, 4], np.float32)
    ones = np.ones((13, 17), bool)
    thr, (out_abs, out_rel), edges, n_thr, n_edges = args.error_args()
    want = E.flow_error(est, ones, gt, ones, thr, out_abs, out_rel, edges)
    s = FlowErrorStats(as_record(want), n_thr, n_edges)
    assert (s.n, s.n_nonfinite, s.epe, s.rmse, s.max) == (221, 0, 5.0, 5.0, 5.0)
    assert s.over == (1.0, 1.0, 0.0)                     # 5 > 1, 5 > 3, not 5 > 5
    assert len(s.bins) == 3 and sum(b[0] for b in s.bins) == 221 and all(b[1] == 5.0 for b in s.bins if b[0])
    assert s.outlier == float((5 > 0.05 * np.sqrt((gt * gt).sum(-1))).mean())          # 3 px passed everywhere; 5 % of |gt| <= 1.5
    assert repr(E.stats(want)) == repr({"n": s.n, "n_nonfinite": 0, "epe": s.epe, "rmse": s.rmse, "max": s.max, "over": s.over,
                                        "outlier": s.outlier, "bins": s.bins})          # repr: the empty third bin's mean is nan
    assert (want["epe_map"] == 5).all()


def test_empty_evaluation_set_gives_nan_without_a_warning():
    import warnings
    (est, em, gt, gm), _ = E.case(1, (5, 7))
    want = E.flow_error(est, em, gt, np.zeros_like(gm))
    assert E.record_words(want) == [0] * 12 and E.record_sums(want) == [0.0] * 6
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = FlowErrorStats(as_record(want))
    assert s.n == 0 and all(math.isnan(v) for v in (s.epe, s.rmse, s.max, s.outlier) + s.over) and len(s.over) == 3
    assert all(b[0] == 0 and math.isnan(b[1]) for b in s.bins) and len(s.bins) == 3
    assert s == FlowErrorStats(as_record(want)) and s != FlowErrorStats(as_record(E.case(1, (5, 7))[1]))


def test_depth_restates_the_header():
    assert E.depth(1) == E.depth(4096 * 256) == 16 + 6 + 3 + 1 + 6 + 3 and E.depth(4096 * 256 + 1) == 36
    assert E.depth(1040 * 1024) == 36 and E.depth(2160 * 3840) == 16 + 6 + 3 + 8 + 6 + 3


# ---------------------------------------------------------------------------------------------- the generator's reach
@pytest.mark.parametrize("shape", E.SHAPES[1:])
@pytest.mark.parametrize("use_est_mask", [True, False])
def test_generated_cases_populate_every_count(shape, use_est_mask):
    """every count of the record is non-zero and smaller than n, every bin is populated, pixels sit exactly on every threshold
    and one float32 step above it, on every edge, and the two kinds of half-outliers are there: a kernel that got a
    comparison, a mask, the finite rule or a bin wrong cannot pass.  ((1, 1) is there for the index arithmetic only.)"""
    for seed in (1, 2, 3):
        (est, em, gt, gm), want = E.case(seed, shape, use_est_mask)
        n = want["n"]
        words = E.record_words(want)
        print(seed, shape, words, E.ties(want))
        assert all(0 < c < n for c in words[1:11]), words
        assert 0 < n < shape[0] * shape[1] - want["n_nonfinite"]                   # pixels are masked out
        assert want["n_nonfinite"] == 6
        assert sum(want["n_bin"]) == n and all(s > 0 for s in want["sum_bin_epe"])
        on, above = E.ties(want)
        assert min(on) >= 1 and min(above) >= 1
        epe, ok = want["epe"], want["ok"]
        g = np.sqrt((gt.astype(np.float64) ** 2).sum(-1))
        assert all((ok & (g == e)).any() for e in E.EDGES)                          # 6-8-10, 24-32-40, 54-72-90: exact
        assert (ok & (epe > E.OUT_ABS) & ~(epe > E.OUT_REL * g.astype(np.float32))).any()
        assert (ok & ~(epe > E.OUT_ABS) & (epe > E.OUT_REL * g.astype(np.float32))).any()
        assert (ok & (g == 0)).any()
        assert (~np.isfinite(est).all(-1) & gm).any() and (~np.isfinite(gt).all(-1) & gm).any()
        assert (np.isfinite(est).all(-1) & np.isfinite(gt).all(-1) & ~np.isfinite(epe) & gm & em).sum() == 2     # the two overflows
        assert (~em & gm).any() and (~gm).any()
        assert not want["epe_map"][~ok].any() and (want["epe_map"][ok] == epe[ok]).all()
    a, b = E.case(1, shape, True)[1], E.case(1, shape, False)[1]
    assert b["n"] > a["n"]                                                          # the estimate's mask matters


def test_smallest_shape_is_one_evaluated_pixel():
    _, want = E.case(1, (1, 1))
    assert E.record_words(want) == [1, 0, 1, 1, 1, 1, 1, 0, 0, 0, 1, int(np.float32(10).view(np.uint32))]
    assert E.record_sums(want) == [10.0, 100.0, 0.0, 0.0, 0.0, 10.0]
