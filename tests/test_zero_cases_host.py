"""CPU suite for tests/zero_cases.py: the oracle's two forms of the zero-flow predicates and the NumPy restatement of the
statistics word agree on every row, non-finite ones included; every row reaches what its name claims; and the oracle's
combine_with(mode=3) answers that test_gpu_zero_predicates.py compares the device with take no early exit on a pair whose
operand is non-zero only through NaN -- which is what lets those comparisons fail."""
import numpy as np
import pytest

import nonfinite_cases as N
import stream_ref as S
import zero_cases as Z
from oracle import np_oracle as O

BITS = (S.NONZERO_MASKED, S.NONZERO_TH_MASKED, S.NONZERO, S.NONZERO_TH)


def test_values_are_what_their_names_say():
    v = {k: np.array(b, np.uint32).view(np.float32) for k, b in Z.VALUES.items()}
    assert all(np.isnan(v[k]) for k in Z.NAN_VALUES) and np.isinf(v['pinf']) and np.isinf(v['ninf'])
    assert np.signbit(v['nnan']) and not np.signbit(v['pnan']) and Z.VALUES['payload'] & 0x3fffff and not Z.VALUES['snan'] & 0x400000
    assert 0 < v['f5e-4'] < v['below_th'] < v['th'] == Z.TH < v['above_th'] and np.nextafter(v['below_th'], np.float32(1)) == Z.TH
    assert 0 < v['subnormal'] < np.finfo(np.float32).tiny and v['negzero'] == 0 and np.signbit(v['negzero'])
    assert set(Z.NONFINITE_VALUES) == {k for k in v if not np.isfinite(v[k])}


@pytest.mark.parametrize("shape", Z.SHAPES, ids=str)
def test_oracle_and_restatement_agree_on_every_row(shape):
    for r in Z.rows(shape):
        for vecs, mask, expect, nonfinite in ((r['fa'], r['ma'], r['expect_a'], r['nonfinite_a']), (r['fb'], r['mb'], r['expect_b'], r['nonfinite_b'])):
            m = mask != 0
            flow = [not O.is_zero_flow(vecs[m][None], False), not O.is_zero_flow(vecs[m][None], True),
                    not O.is_zero_flow(vecs, False), not O.is_zero_flow(vecs, True)]
            raw = [not O.is_zero_raw(vecs, mask, False), not O.is_zero_raw(vecs, mask, True),
                   not O.is_zero_raw(vecs, None, False), not O.is_zero_raw(vecs, None, True)]
            word = S.stats_word(vecs, mask)                         # (asserts its own cross-check with the oracle, non-finite rows too)
            assert expect == raw == flow == [bool(word & b) for b in BITS], r['name']
            assert bool(word & S.NONFINITE) == nonfinite, r['name']


@pytest.mark.parametrize("shape", Z.SHAPES, ids=str)
def test_rows_reach_what_they_claim(shape):
    H, W = shape
    rows = Z.rows(shape)
    seen = set()
    for r in rows:
        seen.add((r['kind'], r['placement'], r['value'], r['under']))
        field, mask = (r['fa'], r['ma']) if r['kind'] == 'fa' else (r['fb'], r['mb'])
        bits = field.view(np.uint32)
        planted = np.zeros((H, W, 2), bool)
        planted[tuple(zip(*r['px']))] = True
        assert (bits[planted] == Z.VALUES[r['value']]).all(), r['name']               # the bit pattern arrived as it is
        assert (mask[planted.any(-1)] == r['under']).all(), r['name']
        nan_value, special = r['value'] in Z.NAN_VALUES, r['value'] != 'negzero'
        if r['kind'] in ('fb', 'fa'):
            # the value is the ONLY thing in the field: everything else is exactly +0.0
            assert (bits[~planted] == 0).all(), r['name']
            expect = r['expect_a'] if r['kind'] == 'fa' else r['expect_b']
            if r['under'] == 0:
                assert expect[:2] == [False, False], r['name']                        # value only under mask 0: the masked words stay clear
            if nan_value or r['value'] in ('pinf', 'ninf', 'th', 'above_th'):
                assert expect == [bool(r['under']), bool(r['under']), True, True], r['name']
            elif special:                                                             # below the threshold, but not zero
                assert expect == [bool(r['under']), False, True, False], r['name']
            else:
                assert expect == [False] * 4, r['name']
        if r['kind'] == 'fa':
            assert r['expect_b'] == ([True] * 4 if r['shift'] else [False] * 4) or not r['mb'].any(), r['name']
        if r['kind'] == 'rot':
            # "masked value only": no other non-zero component under mb == 1; the rotation sits under mb == 0 and sets 6/7
            other = (r['mb'] != 0)[..., None] & ~planted
            assert (bits[other] == 0).all() and r['expect_b'][2:] == [True, True], r['name']
            want = (special and bool(r['under']))
            assert r['expect_b'][0] == want, r['name']
            # the condition by which compose3_xpose_kernel picks the transposed layout, for EVERY tile: the vertical flow at the
            # two ends of a tile's first row differs by more than kXposeRows rows per 128 px
            stream, xposed = Z.layouts(r)
            assert stream == 0 and xposed == -(-H // N.TILE_H) * -(-W // N.TILE_W), r['name']
            for y, x, _ in r['px']:
                assert not N.decision_pixels(r['fb'])[y, x], r['name']
        elif Z.is_tiled(shape) and r['kind'] == 'fb' and r['value'] not in ('pinf', 'ninf'):
            assert Z.layouts(r)[1] == 0, r['name']                                    # streaming layout (NaN compares false)
        if r['placement'] in ('odd_x', 'ragged'):
            assert all(x % 2 == 1 for _, x, _ in r['px']), r['name']                  # the second pixel of a streamed pair
        if r['placement'] == 'ragged':
            assert all(x >= W - W % N.TILE_W and y >= H - H % N.TILE_H for y, x, _ in r['px']), r['name']
        if r['placement'] == 'wave_rows' and r['kind'] != 'rot':
            strips = {(y // 2, x // N.TILE_W) for y, x, _ in r['px']}
            assert strips == {(k, i) for k in range(H // 2) for i in range(-(-W // N.TILE_W))}, r['name']
            assert {c for _, _, c in r['px']} == {0, 1}, r['name']
    # every value meets every placement under both mask bytes as the streamed field, and the transposed layout and the sampled
    # field where the table says so
    for value in Z.VALUES:
        for under in (0, 1):
            for p in Z.PLACEMENTS:
                if Z.pixels(p, shape) is not None:
                    assert ('fb', p, value, under) in seen
            if Z.is_tiled(shape):
                assert {('rot', p, value, under) for p in ('u_first', 'v_last', 'wave_rows')} <= seen
            assert ('fa', 'odd_x', value, under) in seen and ('fa', 'wave_rows', value, under) in seen
    assert (Z.pixels('ragged', shape) is not None) == (shape == (50, 258))


def test_first_and_last_pixels():
    for shape in Z.SHAPES:
        assert Z.pixels('u_first', shape) == [(0, 0, 0)] and Z.pixels('v_last', shape) == [(shape[0] - 1, shape[1] - 1, 1)]
    assert [Z.is_tiled(s) for s in Z.SHAPES] == [True, True, False]


@pytest.mark.parametrize("shape", Z.SHAPES, ids=str)
def test_oracle_takes_no_early_exit_on_a_nan_only_operand(shape):
    """The end-to-end answers of test_gpu_zero_predicates.py, computed here once.  An operand that is non-zero only through
    NaN under its mask is NOT zero for the oracle, in either role, reference and threshold setting: combine_with computes a field.
    The same value under mask 0 only, and -0.0, make the operand zero: the oracle hands back the partner."""
    n_nan = 0
    for index, r in Z.consumer_rows(shape):
        for ref in ('t', 's'):
            for thresholded in (False, True):
                for first in (True, False):
                    how, vecs, mask = Z.oracle_combine(shape, index, ref, thresholded, first)
                    tag = (r['name'], ref, thresholded, first)
                    if r['value'] in Z.NAN_VALUES and r['under'] == 1:
                        n_nan += 1
                        assert how == 'computed' and np.isnan(vecs).any(), tag
                        assert mask.any() and not np.isnan(vecs[mask]).all(), tag   # a field with valid, finite vectors beside the NaN
                    zero = r['expect_b'][1 if thresholded else 0] is False
                    if zero:
                        assert how == ('flow' if first else 'self'), tag             # the operand is zero: the partner comes back
                    else:
                        assert how == 'computed', tag
    assert n_nan == len(Z.NAN_VALUES) * len(Z.CONSUMER_PLACEMENTS) * 8
