"""CPU suite: the host half of the forward-backward check (K13) -- args.consistency_args -- and the NumPy restatement
tests/consistency_ref.py: its known answers, and the reach of the generated cases that test_gpu_consistency.py compares the
kernel with (every class of pixel populated, pixels near the threshold present), shown from the restatement alone."""
import numpy as np
import pytest

from oflibnumpy_amd import args
from oracle import np_oracle as O
import consistency_ref as C


# ---------------------------------------------------------------------------------------------- consistency_args
def test_consistency_args_defaults_and_values():
    a, b = args.consistency_args()
    assert (a, b) == (np.float32(0.01), np.float32(0.5)) and a.dtype == b.dtype == np.float32
    assert args.consistency_args(None, None) == (a, b)
    assert args.consistency_args(0, 0) == (0.0, 0.0)
    assert args.consistency_args(0.05, 2) == (np.float32(0.05), np.float32(2.0))
    assert args.consistency_args(np.float32(0.25), np.int64(3)) == (np.float32(0.25), np.float32(3.0))
    assert args.consistency_args(alpha=1.0)[1] == np.float32(0.5) and args.consistency_args(beta=1.0)[0] == np.float32(0.01)


@pytest.mark.parametrize("bad", [True, False, np.True_, "0.1", [0.1], (0.1,), np.array([0.1]), 1j, object()])
def test_consistency_args_type_errors(bad):
    with pytest.raises(TypeError):
        args.consistency_args(alpha=bad)
    with pytest.raises(TypeError):
        args.consistency_args(beta=bad)


@pytest.mark.parametrize("bad", [-1, -1e-9, -0.5, float('nan'), float('inf'), -float('inf'), np.float32('nan'), 1e39, 10 ** 400])
def test_consistency_args_value_errors(bad):
    with pytest.raises(ValueError):
        args.consistency_args(alpha=bad)
    with pytest.raises(ValueError):
        args.consistency_args(beta=bad)


def test_host_entry_points_check_arguments_before_the_device():
    """Flow.consistency and flow_consistency raise for bad arguments without a device (this suite has none)"""
    import oflibnumpy_amd as of
    f = of.Flow.zero((4, 6), 't')
    with pytest.raises(TypeError):
        f.consistency(np.zeros((4, 6, 2)))
    with pytest.raises(TypeError):
        f.consistency(f, alpha=True)
    with pytest.raises(TypeError):
        f.consistency(f, return_residual=1)
    with pytest.raises(ValueError):
        f.consistency(f, alpha=-1)
    with pytest.raises(ValueError):
        f.consistency(f, beta=float('nan'))
    with pytest.raises(ValueError, match="4, 6.*5, 6"):
        f.consistency(of.Flow.zero((5, 6), 't'))
    with pytest.raises(ValueError, match="'t'.*'s'"):
        f.consistency(of.Flow.zero((4, 6), 's'))
    with pytest.raises(ValueError):
        of.flow_consistency(np.zeros((4, 6, 2)), np.zeros((4, 6, 2)), 't', beta=-1)
    assert 'flow_consistency' in of.flow_operations.__all__


# ---------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("quant", C.QUANTS)
@pytest.mark.parametrize("alpha_beta", [(C.ALPHA, C.BETA), (0.0, 0.0)])
def test_integer_translation(oracle, quant, alpha_beta):
    """f = (3, -2), b = -f, 's', at (37, 131): the sample is exact, so the sum is exactly zero on the (37 - 2) x (131 - 3)
    pixels whose sample stays in the frame -- consistent also with alpha = beta = 0, which pins `<=`"""
    f, fm, b, bm = C.translation()
    consistent, covered, residual, counts = C.consistency(f, fm, b, bm, +1, *alpha_beta, quant=quant)
    assert np.array_equal(consistent, covered)
    assert counts == (4480, 4480) and covered[2:, :128].all() and not covered[:2].any() and not covered[:, 128:].any()
    assert not residual.any()


@pytest.mark.parametrize("quant, bound", [(O.QUANT_OPENCV, 0.05), (O.QUANT_EXACT, 0.05)])
@pytest.mark.parametrize("ref", ['s', 't'])
def test_rotation_and_its_inverse(oracle, ref, quant, bound):
    f, fm, b, bm = C.rotation(ref)
    consistent, covered, residual, counts = C.consistency(f, fm, b, bm, 1 if ref == 's' else -1, quant=quant)
    print("rotation", ref, quant, "covered", counts[0], "largest residual", residual.max())
    assert counts[0] > 1000 and np.array_equal(consistent, covered)
    assert residual.max() < bound


# ---------------------------------------------------------------------------------------------- the generator's reach
@pytest.mark.parametrize("shape", C.SHAPES[1:])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_generated_cases_populate_every_class(oracle, seed, shape):
    """not covered / covered and consistent / covered and inconsistent each hold at least 10 % of the pixels, and at least 5
    covered pixels lie within 5 % of the bound: a kernel that got the comparison, the bound or a mask wrong cannot pass"""
    n = shape[0] * shape[1]
    for sign in C.SIGNS:
        for quant in C.QUANTS:
            inputs, (consistent, covered, residual, counts) = C.case(seed, shape, sign, quant)
            shares = [(n - counts[0]) / n, counts[1] / n, (counts[0] - counts[1]) / n]
            near = C.near_threshold(*inputs, sign, quant=quant)
            print(seed, shape, sign, quant, "shares", [round(s, 3) for s in shares], "near", near)
            assert min(shares) >= 0.10, (seed, shape, sign, quant, shares)
            assert near >= 5, (seed, shape, sign, quant, near)
            assert not residual[~covered].any() and (residual[covered] >= 0).all()


def test_smallest_shape_runs(oracle):
    """(5, 7) is there for the index arithmetic only: it is exempt from the shares"""
    for sign in C.SIGNS:
        for quant in C.QUANTS:
            inputs, (consistent, covered, residual, counts) = C.case(1, (5, 7), sign, quant)
            assert consistent.shape == covered.shape == residual.shape == (5, 7) and counts[1] <= counts[0] <= 35
