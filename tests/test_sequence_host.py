"""CPU half of K25 (sequence accumulation): the NumPy restatement of tests/sequence_ref.py checks itself against the
oracle's fused composition and against a known answer, the generated inputs exercise what they are meant to, and
of.combine_flow_sequence raises its argument errors before a device is needed."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import args
from oracle import np_oracle as O
import sequence_ref as R


@pytest.mark.parametrize("shape", R.SHAPES)
def test_length_one_is_the_identity_and_length_two_is_the_composition(shape):
    for sign, quant in itertools.product(R.SIGNS, R.QUANTS):
        (vecs, masks), (out, mout, pv, pm, lost_at) = R.case(shape, 1, sign, quant)
        assert R._same_floats(out, vecs[0]) and np.array_equal(mout, masks[0])
        assert R._same_floats(pv, vecs) and np.array_equal(pm, masks)
        np.testing.assert_array_equal(lost_at, np.where(masks[0], -1, 0))
        (vecs, masks), (out, mout, pv, pm, lost_at) = R.case(shape, 2, sign, quant)
        first, second = (0, 1) if sign > 0 else (1, 0)
        c_out, c_mout = O.compose3_raw(vecs[second], masks[second], vecs[first], masks[first], sign, quant)
        assert R._same_floats(out, c_out) and np.array_equal(mout, c_mout)
        assert R._same_floats(pv[first], vecs[first]) and R._same_floats(pv[second], c_out)
        np.testing.assert_array_equal(pm[second], c_mout)
        np.testing.assert_array_equal(lost_at, np.where(~masks[first], first, np.where(~c_mout, second, -1)))


def test_the_fold_is_the_oracle_flow_chain_in_the_stated_association():
    """'s': F <- F.combine_with(f_k, 3); 't': G <- f_k.combine_with(G, 3) -- on fields that take no early exit"""
    shape, length = (19, 70), 5
    for ref, sign in (('s', 1), ('t', -1)):
        (vecs, masks), (out, mout, pv, pm, _) = R.case(shape, length, sign, O.QUANT_OPENCV)
        flows = [O.OFlow(vecs[k], ref, masks[k]) for k in range(length)]
        if ref == 's':
            acc = flows[0]
            for k in range(1, length):
                acc = acc.combine_with(flows[k], 3)
                assert R._same_floats(pv[k], acc.vecs) and np.array_equal(pm[k], acc.mask)
        else:
            acc = flows[-1]
            for k in range(length - 2, -1, -1):
                acc = flows[k].combine_with(acc, 3)
                assert R._same_floats(pv[k], acc.vecs) and np.array_equal(pm[k], acc.mask)
        assert R._same_floats(out, acc.vecs) and np.array_equal(mout, acc.mask)


@pytest.mark.parametrize("sign", R.SIGNS)
def test_integer_translations_sum_and_lose_pixels_where_the_walk_leaves_the_frame(sign):
    shape, steps = (19, 70), ((3, -2), (1, 4), (-2, 1), (4, 2))
    vecs, masks = R.translations(shape, steps)
    total, inside, lost = R.translations_answer(shape, steps, sign)
    for quant in R.QUANTS:
        out, mout, pv, pm, lost_at = R.fold(vecs, masks, sign, quant)
        np.testing.assert_array_equal(mout, inside)
        np.testing.assert_array_equal(lost_at, lost)
        assert (out[mout] == total).all() and 0 < mout.sum() < mout.size
        np.testing.assert_array_equal(pm[R.walk(len(steps), sign)[-1]], mout)
    np.testing.assert_array_equal(total, np.sum(np.array(steps, np.float32), axis=0))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_generated_inputs_lose_pixels_at_every_step_and_keep_enough(shape):
    """case() asserts the conditions itself (check_conditions); here they are read back in figures"""
    shares = []
    for length, sign, quant in itertools.product(R.LENGTHS, R.SIGNS, R.QUANTS):
        (vecs, masks), (_, mout, _, pm, lost_at) = R.case(shape, length, sign, quant)
        assert masks[0::2].all() and not masks[1::2, shape[0] // 4, shape[1] // 8].any()
        assert lost_at.min() >= -1 and lost_at.max() < length
        np.testing.assert_array_equal(lost_at < 0, mout)
        if length >= 2:
            shares.append(float(mout.mean()))
            if shape != (5, 7):
                assert set(R.walk(length, sign)[1:]) <= set(np.unique(lost_at).tolist())
    assert min(shares) > 0 if shape == (5, 7) else min(shares) >= 0.25


def test_sequence_args():
    assert args.sequence_args(6) == (6, 1, 0, False, False)
    assert args.sequence_args(6, 3, 1, True, None) == (3, 2, 1, True, False)
    assert args.sequence_args(6, np.int64(6)) == (6, 1, 0, False, False)
    for bad in (0, -3, 4, 7):
        with pytest.raises(ValueError, match="Error combining flow sequence: Length"):
            args.sequence_args(6, bad)
    for bad in (2.0, True, '3'):
        with pytest.raises(TypeError, match="Error combining flow sequence: Length"):
            args.sequence_args(6, bad)
    with pytest.raises(ValueError, match="Quant"):
        args.sequence_args(6, None, 2)
    with pytest.raises(TypeError, match="Quant"):
        args.sequence_args(6, None, None)
    with pytest.raises(TypeError, match="Return_partials"):
        args.sequence_args(6, None, 0, 1)
    with pytest.raises(TypeError, match="Return_lost_at"):
        args.sequence_args(6, None, 0, False, 'yes')


def test_combine_flow_sequence_argument_errors_need_no_device():
    assert 'combine_flow_sequence' in of.flow_operations.__all__ and of.combine_flow_sequence is of.flow_operations.combine_flow_sequence
    f = of.Flow.zero((6, 9), 't')
    prefix = "Error combining flow sequence: "
    with pytest.raises(ValueError, match=prefix + "Flows need to hold at least one flow"):
        of.combine_flow_sequence([])
    with pytest.raises(TypeError, match=prefix):
        of.combine_flow_sequence(f)
    with pytest.raises(TypeError, match=prefix):
        of.combine_flow_sequence([f, f.vecs])
    with pytest.raises(ValueError, match=prefix + "Flow fields need to have the same shape"):
        of.combine_flow_sequence([f, of.Flow.zero((6, 10), 't')])
    with pytest.raises(ValueError, match=prefix + "Flow fields need to have the same reference"):
        of.combine_flow_sequence([f, of.Flow.zero((6, 9), 's')])
    with pytest.raises(ValueError, match=prefix + "Masks go with"):
        of.combine_flow_sequence([f, f], masks=np.ones((2, 6, 9), bool))
    with pytest.raises(ValueError, match=prefix + "Flows need to be a numpy array of shape"):
        of.combine_flow_sequence(np.zeros((6, 9, 2), np.float32), 't')
    with pytest.raises(ValueError, match=prefix + "Flows need to be a numpy array of shape"):
        of.combine_flow_sequence(np.zeros((0, 6, 9, 2), np.float32), 't')
    with pytest.raises(TypeError, match=prefix + "Masks"):
        of.combine_flow_sequence(np.zeros((2, 6, 9, 2), np.float32), 't', masks=[1])
    with pytest.raises(ValueError, match=prefix + "Masks need to have shape"):
        of.combine_flow_sequence(np.zeros((2, 6, 9, 2), np.float32), 't', masks=np.ones((2, 6, 8), bool))
    with pytest.raises(ValueError):                                   # Flow's own check of the reference
        of.combine_flow_sequence(np.zeros((2, 6, 9, 2), np.float32), 'x')
    with pytest.raises(ValueError):                                   # and of the vectors
        of.combine_flow_sequence(np.full((2, 6, 9, 2), np.nan, np.float32), 't')
    with pytest.raises(TypeError, match=prefix + "Return_partials"):
        of.combine_flow_sequence([f, f], return_partials=1)
    with pytest.raises(TypeError, match=prefix + "Return_lost_at"):
        of.combine_flow_sequence([f, f], return_lost_at='no')
    with pytest.raises(ValueError, match=prefix + "Quant"):
        of.combine_flow_sequence([f, f], quant=5)
