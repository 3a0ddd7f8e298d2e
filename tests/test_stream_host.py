"""tests/stream_ref.py (the NumPy statement of ofl_stats.hip and of the mask packing) on the CPU: its known answers are the
reference's own (tests/test_flow_class.py:982-1024 there), and what the cases of tests/test_gpu_stream.py reach is shown
here from the restatement alone -- the GPU test runs exactly the cases these generators make."""
import numpy as np
import pytest

from oracle import np_oracle as O
import stream_ref as S
from stream_ref import stats_cases, extent_cases      # noqa: F401  (the generators the GPU test shares)

F32 = np.float32


# ---------------------------------------------------------------------------------------------- known answers of the reference
def test_is_zero_known_answers():
    """a 10 x 10 zero field whose only non-zero vector, (10, 10), sits under the only mask-false pixel"""
    v, m = np.zeros((10, 10, 2), F32), np.ones((10, 10), bool)
    v[0, 0], m[0, 0] = 10, False
    word = S.stats_word(v, m)
    assert word == S.NONZERO | S.NONZERO_TH | S.MASK_HAS_ZERO
    assert not word & S.NONZERO_TH_MASKED            # Flow.is_zero() and is_zero(masked=True) are True
    assert word & S.NONZERO_TH                       # is_zero(masked=False) is False
    assert S.stats_word(v, None) == S.NONZERO_MASKED | S.NONZERO_TH_MASKED | S.NONZERO | S.NONZERO_TH


@pytest.mark.parametrize("ref,masked,want", [('s', False, [5, 0, 0, 3]), ('t', False, [0, 3, 5, 0]),
                                             ('s', True, [3, 0, 0, 1]), ('t', True, [0, 1, 3, 0])])
def test_get_padding_known_answers(ref, masked, want):
    """a rotation by 45 degrees about the origin on 7 x 7, whole and with columns 4.. ('s') or rows 4.. ('t') masked out"""
    mask = np.ones((7, 7), bool)
    if masked and ref == 's':
        mask[:, 4:] = False
    elif masked:
        mask[4:] = False
    f = O.from_transforms([['rotation', 0, 0, 45]], (7, 7), ref, mask)
    assert S.padding(f.vecs, f.mask, 1 if ref == 's' else -1) == want


def test_get_padding_ignores_vectors_below_the_threshold():
    v = np.zeros((7, 7, 2), F32)
    v[..., 0] = np.random.default_rng(0).random((7, 7)) * 1e-4
    assert S.padding(v, np.ones((7, 7), bool), -1) == [0, 0, 0, 0]
    assert S.padding(v, np.ones((7, 7), bool), -1, th=None) == [0, 0, 1, 0]
    with pytest.raises(ValueError):
        S.padding(v, np.zeros((7, 7), bool), -1)
    np.testing.assert_array_equal(S.extent(v, np.zeros((7, 7), bool), 1), np.array([np.inf, -np.inf, np.inf, -np.inf], F32))


# ---------------------------------------------------------------------------------------------- the statistics word
def test_threshold_edges_of_the_word():
    one = lambda u, v: S.stats_word(np.array([[0, 0], [u, v]], F32), None)
    both, plain = 15, S.NONZERO_MASKED | S.NONZERO
    assert one(0, 7e-4) == plain
    assert one(S.TH, 0) == one(-S.TH, 0) == both                            # |c| == threshold is not below it
    assert one(S.BELOW_TH, 0) == one(0, -S.BELOW_TH) == plain
    assert one(S.SUBNORMAL, 0) == plain                                     # a subnormal is not zero
    assert one(0, -0.0) == 0                                                # -0.0 is
    for u, v in ((np.nan, 0), (0, np.nan), (np.inf, 0), (0, -np.inf)):
        assert one(u, v) == both | S.NONFINITE
    assert S.stats_word(np.zeros((0, 2), F32), None) == 0
    assert S.stats_word(np.zeros((3, 2), F32), np.array([1, 0, 1], np.uint8)) == S.MASK_HAS_ZERO
    assert S.stats_word(np.zeros((3, 2), F32), np.array([2, 255, 1], np.uint8)) == 0     # any non-zero byte is "valid"
    # the non-finite bit does not ask the mask
    assert S.stats_word(np.array([[np.nan, 0], [0, 0]], F32), np.array([0, 1], np.uint8)) == S.NONZERO | S.NONZERO_TH | S.NONFINITE | S.MASK_HAS_ZERO


def test_sweep_kinds_give_different_words():
    """the single-cause sweep of the GPU test tells its causes apart: the kinds give seven different words with the mask"""
    words = {}
    for kind, (vec, byte) in S.STATS_KINDS.items():
        v, m = np.zeros((5, 2), F32), np.ones(5, np.uint8)
        v[2], m[2] = vec, byte
        words[kind] = (S.stats_word(v, m), S.stats_word(v, None))
    assert words['a'] == (5, 5) and words['b+'] == words['b-'] == (15, 15) and words['c+'] == words['c-'] == (5, 5)
    assert words['d'] == (5, 5) and words['e'] == (0, 0) and words['f-nan-u'] == words['f-inf'] == (31, 31)
    assert words['g'] == (32, 0) and words['h'] == (4 | 8 | 32, 15) and words['i'] == (4 | 8 | 16 | 32, 31)
    assert len(set(words.values())) == 7


def test_sweep_positions_cross_every_edge():
    for n in S.STATS_SIZES:
        p = S.stats_positions(n)
        assert p[0] == 0 and p[-1] == n - 1 and all(0 <= q < n for q in p)
        if n > S.STATS_WG:          # both sides of every chunk edge of the first workgroup, and of the workgroup edge
            assert all(k * 512 - 1 in p and k * 512 in p for k in range(1, 9))
            assert p[-1] >= S.STATS_WG
    # below, on and past one workgroup; odd sizes (the tail pixel) and even ones; many workgroups
    assert {n // 2 <= 2048 for n in S.STATS_SIZES} == {True, False} and {n & 1 for n in S.STATS_SIZES} == {0, 1}
    assert max(S.STATS_SIZES) // 2 // 2048 >= 10


def test_random_stats_cases_reach_every_bit():
    cases = S.stats_cases()
    with_mask = [S.stats_word(v, m) for _, v, m in cases]
    without = [S.stats_word(v, None) for _, v, m in cases]
    for bit in (1, 2, 4, 8, 16, 32):
        assert any(w & bit for w in with_mask) and any(not w & bit for w in with_mask), bit
    for bit in (1, 2, 4, 8, 16):
        assert any(w & bit for w in without) and any(not w & bit for w in without), bit
    assert not any(w & S.MASK_HAS_ZERO for w in without)             # no mask, no zero byte
    # a non-zero vector only under mask 0: the masked and the unmasked predicates of ONE word differ
    assert any((w & 12) and not (w & 3) for w in with_mask)
    assert any((w & 12) == 4 and not (w & 3) for w in with_mask)     # and so for the thresholded pair alone
    # several workgroups, and a cause that is not in the first one
    assert any(v.shape[0] > 2 * S.STATS_WG for _, v, m in cases)
    assert any(np.flatnonzero(v.any(axis=1)).min(initial=1 << 30) >= S.STATS_WG for _, v, m in cases if v.any() and not np.isnan(v).any())


# ---------------------------------------------------------------------------------------------- axpy
def test_axpy_is_two_roundings():
    a, b = np.array([[1.0, 1.0]], F32), np.array([[3.0, 1e-8]], F32)
    out, mout = S.axpy(a, np.array([1], np.uint8), b, np.array([0], np.uint8), 1.0 / 3.0)
    assert out.dtype == F32 and out[0, 0] == F32(1) + F32(F32(1.0 / 3.0) * F32(3)) and mout[0] == 0
    assert S.axpy(a, None, None, None, -2.75)[1] is None
    np.testing.assert_array_equal(S.axpy(a, None, None, None, -2.75)[0], np.array([[-2.75, -2.75]], F32))


@pytest.mark.parametrize("n", S.AXPY_SIZES)
def test_axpy_inputs_tell_a_fused_multiply_add_apart(n):
    """alpha = 1/3 (and -2.75) on the drawn inputs: some element differs between one rounding and two -- unless n is tiny;
    alpha = +-1 never differs (the product is exact; 0.5 is inexact only where it underflows), which is why these values
    alone cannot see a contraction"""
    a, ma, b, mb = S.axpy_inputs(n)
    assert a.shape == b.shape == (n, 2) and ma.shape == mb.shape == (n,)
    if n >= 255:
        assert S.fused_differs(n, 1.0 / 3.0) > 0 and S.fused_differs(n, -2.75) > 0
    assert S.fused_differs(n, 1.0) == S.fused_differs(n, -1.0) == 0
    assert S.fused_differs(n, 0.5) <= 10                # the planted subnormals
    assert sum(S.fused_differs(k, 1.0 / 3.0) for k in S.AXPY_SIZES) > 100
    assert ma[n - 1] == 255 and mb[n - 1] == 3 and S.axpy(a, ma, b, mb, 1.0)[1][n - 1] == 3 and S.axpy(a, ma, None, None, 1.0)[1][n - 1] == 255
    if n >= 255:
        assert ((ma == 2) & (mb == 128)).any() and not (S.axpy(a, ma, b, mb, 1.0)[1][(ma == 2) & (mb == 128)]).any()
    if n >= 64:                  # the planted values are there
        for x in (a, b):
            assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (np.abs(x) == np.finfo(F32).max).any()
        assert np.signbit(a[a == 0]).any() and (~np.signbit(a[a == 0])).any() and (np.abs(a) == np.finfo(F32).tiny).any()


# ---------------------------------------------------------------------------------------------- extent
def test_extent_cases_reach():
    changed = {1: 0, -1: 0}
    negative = {1: 0, -1: 0}
    for shape in S.EXTENT_SHAPES:
        names = set()
        for name, sign, v, m in S.extent_cases(shape):
            names.add(name)
            if name == "none":
                assert not m.any()
                continue
            if S.padding(v, m, sign) != S.padding(v, m, sign, th=None):      # thresholding changes the answer
                changed[sign] += 1
                assert name == "threshold"
            if name == "threshold":
                assert S.padding(v, m, sign) == [0, 0, 0, 0] and S.padding(v, m, sign, th=None)[0::2] == [1, 1]
            if (S.extent(v, m, sign) < 0).all():
                negative[sign] += 1
            if name == "positive":
                assert (S.extent(v, m, sign) > 0).all()
            if name == "one pixel":
                assert int(m.sum()) == 1
        assert names == {"random", "threshold", "negative", "positive", "one pixel", "none", "minima at pixel 0", "maxima at the last pixel"}
    assert min(changed.values()) >= len(S.EXTENT_SHAPES) and min(negative.values()) >= len(S.EXTENT_SHAPES)


def test_extent_extremes_sit_where_strided_threads_read():
    """(513, 512) is larger than the extent kernel's grid: the maxima of one case sit at a pixel index only a second
    iteration of a thread reaches, the minima of another at index 0"""
    shape = (513, 512)
    assert shape in S.EXTENT_SHAPES and shape[0] * shape[1] > S.EXTENT_GRID_CAP
    for name, sign, v, m in S.extent_cases(shape):
        px, py = S.positions(np.where((v < S.TH) & (v > -S.TH), F32(0), v), sign)
        e = S.extent(v, m, sign)
        if name == "maxima at the last pixel":
            assert int(np.argmax(py)) == int(np.argmax(px)) == px.size - 1 >= S.EXTENT_GRID_CAP and (e[1], e[3]) == (py.max(), px.max())
        if name == "minima at pixel 0":
            assert int(np.argmin(py)) == int(np.argmin(px)) == 0 and (e[0], e[2]) == (py.min(), px.min())


def test_grid_offset_is_one_rounding():
    v = np.array([[[0.1, -0.0], [1e-45, 16777216.0]]], F32)
    for sign in (1, -1):
        want = np.array([[[np.float64(0) + sign * np.float64(F32(0.1)), 0.0], [1 + sign * 1e-45, sign * 16777216.0]]]).astype(F32)
        np.testing.assert_array_equal(S.grid_offset(v, sign).view(np.uint32), want.view(np.uint32))
    for shape in S.GRID_OFFSET_SHAPES:
        f = S.offset_field(shape)
        assert f.shape == shape + (2,) and f.dtype == F32
        if f.size < 600:
            continue
        assert (np.abs(f) > 1e4).any() and np.signbit(f[f == 0]).any() and (~np.signbit(f[f == 0])).any()
        assert ((f != 0) & (np.abs(f) < np.finfo(F32).tiny)).any()


# ---------------------------------------------------------------------------------------------- conversion, sampling
def test_convert_inputs_hold_the_edges():
    for src, dst in S.CONVERT_PAIRS:
        for n in S.CONVERT_SIZES:
            x = S.convert_input(src, dst, n)
            assert x.shape == (n,) and x.dtype == S.DTYPES[src]
            if dst in (S.U8, S.I16, S.U16):            # float32 -> integer: in range and never NaN; astype truncates
                info = np.iinfo(S.DTYPES[dst])
                assert (x >= info.min).all() and (x <= info.max).all()
                if n >= 255:
                    assert (x != np.trunc(x)).any() and x.min() == info.min
                if n == 70001:
                    assert x.max() == info.max and np.unique(S.convert(x, S.DTYPES[dst])).size == int(info.max) - int(info.min) + 1
            elif src in (S.U8, S.I16, S.U16) and n == 70001:
                assert np.unique(x).size == int(np.iinfo(x.dtype).max) - int(np.iinfo(x.dtype).min) + 1
    d = S.convert_input(S.F64_CODE, S.F32_CODE, 255)
    f = S.convert(d, F32)
    assert f[0] == 1 and f[1] == F32(1) + F32(2.0 ** -22) and f[3] == np.nextafter(F32(1), F32(2))      # ties to even, and just above a tie
    assert np.isposinf(f[7]) and np.isfinite(d[7]) and f[9] == np.finfo(F32).max and np.isposinf(f[10])
    assert ((f != 0) & (np.abs(f) < np.finfo(F32).tiny)).any() and f[15] == 0 and f[16] == 2 * S.SUBNORMAL
    assert S.convert(np.array([2.5, -2.5, 254.999], F32), np.int16).tolist() == [2, -2, 254]
    assert len(S.CONVERT_PAIRS) == 9


def test_sample_points_takes_the_reference_weights():
    flow = np.arange(24, dtype=F32).reshape(3, 4, 2)
    pts = np.array([[0.0, 0.0], [1.0, 2.0], [0.5, 0.0], [2.0, 1.5], [2.0, 3.0], [1.25, 2.5]])
    got = S.sample_points(flow, pts)
    assert got.dtype == np.float64 and got.shape == (6, 2)
    # an integer point inside has the weights (1, 0, 0, 0): the pixel itself, (v, u) order
    np.testing.assert_array_equal(got[0], flow[0, 0, ::-1])
    np.testing.assert_array_equal(got[1], flow[1, 2, ::-1])
    # half-way down a column: the reference pairs the (row 0, col 1) sample with the weight of (row 1, col 0), so the point
    # gets half of its RIGHT neighbour, not of the pixel below -- the restatement follows the reference, not the textbook
    np.testing.assert_array_equal(got[2], 0.5 * flow[0, 0, ::-1] + 0.5 * flow[0, 1, ::-1])
    # on the last row / column both clamped neighbours are the point's own row / column and every weight has a factor
    # (last - coordinate) = 0: the reference's result there is 0, not the pixel
    np.testing.assert_array_equal(got[3], [0, 0])
    np.testing.assert_array_equal(got[4], [0, 0])
    for shape in S.SAMPLE_FIELDS:
        for n in S.SAMPLE_COUNTS:
            f, p = S.sample_case(shape, n)
            assert p.shape == (n, 2) and (p >= 0).all() and (p[:, 0] <= shape[0] - 1).all() and (p[:, 1] <= shape[1] - 1).all()
        f, p = S.sample_case(shape, 10000)
        if min(shape) > 1:
            assert ((p[:, 0] == shape[0] - 1) & (p[:, 1] == shape[1] - 1)).any() and (p != np.floor(p)).all(axis=1).any()
            assert ((np.ceil(p) - p > 0) & (np.ceil(p) - p < 1e-12)).any()            # just below an integer


# ---------------------------------------------------------------------------------------------- mask bit planes
def test_pack_bits_layout():
    m = np.zeros((1, 2, 45), np.uint8)
    m[0, 0, 0] = m[0, 0, 31] = m[0, 0, 32] = 1
    m[0, 1, 44] = 200
    bits = S.pack_bits(m, 2, 45, 1)
    assert bits.shape == (1, 2, 2) and bits.dtype == np.uint32
    assert bits.tolist() == [[[0x80000001, 1], [0, 1 << 12]]]
    np.testing.assert_array_equal(S.unpack_bits(bits, 2, 45, 1), (m != 0).astype(np.uint8))
    for H in S.PACK_HEIGHTS:
        for W in S.PACK_WIDTHS:
            for batch in S.PACK_BATCHES:
                for name, mask in S.pack_masks(H, W, batch):
                    b = S.pack_bits(mask, H, W, batch)
                    np.testing.assert_array_equal(S.unpack_bits(b, H, W, batch), (mask != 0).astype(np.uint8))
                    if W % 32:
                        assert not (b[..., -1] >> (W % 32)).any()               # the padding bits of a row are zero
    assert any((mask > 1).any() for _, mask in S.pack_masks(9, 130, 3))


def test_pack_cases_reach_both_load_paths():
    """at a 16-byte aligned plane: rows of 130 bytes start at every even residue mod 16 and rows of 45 bytes at odd ones too, so
    both the 16-byte loads and the byte loop pack whole words inside one plane; narrow rows take the byte loop only"""
    assert S.pack_paths(1, 31, 1) == (0, 1) and S.pack_paths(1, 32, 1) == (1, 0) and S.pack_paths(1, 33, 1) == (1, 1)
    wide, narrow = S.pack_paths(9, 130, 1)
    assert (wide, narrow) == (2 * 4, 9 * 5 - 8)                     # rows 0 and 8 are aligned; the fifth word of a row is partial
    assert S.pack_paths(9, 45, 1) == (1, 17) and S.pack_paths(9, 4112, 3) == (27 * 128, 27)
    assert {(130 * r) % 16 for r in range(9)} == set(range(0, 16, 2)) and {(45 * r) % 16 for r in range(9)} >= {0, 13, 10, 7}
