"""CPU suite: the host half of the convex upsampling (K17) -- args.upsample_args, the ctypes table, the argument checks of
Flow.upsample_convex and upsample_flow_convex -- and the NumPy restatement tests/upsample_ref.py that test_gpu_upsample.py
compares the kernel with, byte for byte: the error of its exp32 against np.exp in float64, its distance from the float64
definition against the bound derived in upsample_ref.py, known answers that are exact, the float64 definition against the
textbook unfold / softmax / sum / permute / reshape formulation, and the mask rule."""
import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import args
import upsample_ref as U

HOST_SPREADS = (1.0, 8.0, 32.0, 80.0)


# ---------------------------------------------------------------------------------------------- exp32
@pytest.fixture(scope="module")
def exp_error():
    """E: the largest relative error of exp32 against float64 np.exp, in units of 2^-24, over a fixed dense sweep of
    [-87, 0] and the float32 neighbours of the reduction's breakpoints"""
    sweep = np.linspace(-87.0, 0.0, 2_000_001).astype(np.float32)
    br = U.BREAKPOINTS[(U.BREAKPOINTS >= -87.0) & (U.BREAKPOINTS <= 0.0)].astype(np.float32)
    near = [br]
    for _ in range(3):
        near.append(np.nextafter(near[-1], np.float32(0.0)))
    for _ in range(3):
        near.insert(0, np.nextafter(near[0], np.float32(-100.0)))
    t = np.concatenate([sweep] + near + [np.array([-87.0, 0.0, -0.0], np.float32)])
    t = t[(t >= -87.0) & (t <= 0.0)]
    exact = np.exp(t.astype(np.float64))
    return float(np.max(np.abs(U.exp32(t).astype(np.float64) - exact) / exact) / U.EPS)


def test_exp32_error_and_exact_one(exp_error):
    print("E = {:.3f} * 2^-24".format(exp_error))
    assert exp_error <= 2.0
    assert U.exp32(np.float32(0.0)).tobytes() == np.float32(1.0).tobytes()
    assert U.exp32(np.float32(-0.0)).tobytes() == np.float32(1.0).tobytes()
    assert U.exp32(np.float32(-87.0)) > np.finfo(np.float32).tiny                  # the exponent field stays positive


@pytest.mark.parametrize("f", U.FACTORS)
def test_restatement_is_within_the_derived_bound_of_float64(f, exp_error):
    shape = (9, 11)
    v = U.vectors(shape)
    umax = U.window_max(v, f)
    assert (umax > 0).all()
    bound = (24.0 + 2.0 * exp_error) * U.EPS * umax
    worst = 0.0
    for spread in HOST_SPREADS:
        for elem in ("float32", "float16", "bfloat16"):
            x, bf = U.stored(U.logits(shape, f, spread), elem)
            got = U.upsample(v, np.ones(shape, np.uint8), x, f, bf)[0].astype(np.float64)
            err = np.abs(got - U.upsample64(v, x, f, bf))
            worst = max(worst, float((err.max(-1) / (U.EPS * umax)).max()))
            assert (err.max(-1) <= bound).all(), (f, spread, elem)
    print("f = {}: worst error {:.2f} * 2^-24 * U".format(f, worst))


# ---------------------------------------------------------------------------------------------- known answers, exact
@pytest.mark.parametrize("f", U.FACTORS)
def test_uniform_logits_give_the_mean_summed_in_order(f):
    shape = (4, 5)
    v = U.vectors(shape)
    for value in (0.0, -3.5):
        got = U.upsample(v, np.ones(shape, np.uint8), np.full((9 * f * f,) + shape, value, np.float32), f)[0]
        taps = U._taps(v, f, np.float32)
        acc = taps[0].copy()
        for k in range(1, 9):
            acc = acc + taps[k]
        want = acc / np.float32(9.0)
        assert got.tobytes() == np.ascontiguousarray(np.repeat(np.repeat(want, f, 0), f, 1)).tobytes()


@pytest.mark.parametrize("f", U.FACTORS)
@pytest.mark.parametrize("elem,low", [("float32", -1e4), ("bfloat16", -1e4), ("float16", -6e4)])
def test_one_hot_logits_give_exactly_the_neighbour(f, elem, low):
    shape = (4, 5)
    v = U.vectors(shape)
    v[v == 0] = 1.5                                                # a zero neighbour would not tell a tap from padding
    for k in range(9):
        x = np.full((9, f, f) + shape, low, np.float32)
        x[k] = 0.0
        x, bf = U.stored(x.reshape((9 * f * f,) + shape), elem)
        got = U.upsample(v, np.ones(shape, np.uint8), x, f, bf)[0]
        dy, dx = k // 3 - 1, k % 3 - 1
        for y, xx in ((0, 0), (0, 2), (2, 2), (3, 4), (2, 0)):     # corners, an edge, the interior
            inside = 0 <= y + dy < shape[0] and 0 <= xx + dx < shape[1]
            want = v[y + dy, xx + dx] * np.float32(f) if inside else np.zeros(2, np.float32)
            block = got[f * y:f * y + f, f * xx:f * xx + f]
            assert block.tobytes() == np.broadcast_to(want, (f, f, 2)).astype(np.float32).tobytes(), (k, y, xx)


# ---------------------------------------------------------------------------------------------- channel and pixel order, mask
@pytest.mark.parametrize("f", U.FACTORS)
def test_float64_definition_equals_the_unfold_formulation(f):
    shape = (5, 7)
    v = U.vectors(shape)
    x = U.logits(shape, f, 8.0)
    a, b = U.upsample64(v, x, f), U.upsample_unfold(v, x, f)
    assert a.shape == b.shape == (f * shape[0], f * shape[1], 2)
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * f * np.abs(v).max())
    # and a permuted channel order or pixel order does not pass
    assert np.abs(a - U.upsample_unfold(v, x.reshape(9, f, f, *shape).transpose(0, 2, 1, 3, 4).reshape(x.shape), f)).max() > 1e-3


def test_mask_rule():
    m = np.ones((4, 5), np.uint8)
    m[1, 2] = 0
    got = U.out_mask(m, 2)
    want = np.ones((4, 5), np.uint8)
    want[0:3, 1:4] = 0                                             # every coarse pixel whose window holds (1, 2)
    assert got.dtype == np.uint8 and np.array_equal(got, np.repeat(np.repeat(want, 2, 0), 2, 1))
    assert U.out_mask(np.ones((1, 1), np.uint8), 8).all()          # taps outside the frame do not count
    assert not U.out_mask(np.zeros((1, 1), np.uint8), 4).any()
    v = U.vectors((4, 5))
    x = U.logits((4, 5), 2, 8.0)
    assert U.upsample(v, m, x, 2)[0].tobytes() == U.upsample(v, np.ones_like(m), x, 2)[0].tobytes()      # the vector is computed regardless


# ---------------------------------------------------------------------------------------------- args
def test_upsample_args_values():
    assert args.upsample_args(8, (576, 3, 4), (3, 4)) == 8
    assert args.upsample_args(np.int64(2), (5, 36, 3, 4), (3, 4)) == 2
    assert isinstance(args.upsample_args(np.int32(4), (144, 1, 1), (1, 1)), int)


@pytest.mark.parametrize("bad", [True, np.bool_(False), 8.0, "8", None, (8,)])
def test_upsample_args_type_errors(bad):
    with pytest.raises(TypeError, match="Error upsampling flow: factor"):
        args.upsample_args(bad, (576, 3, 4), (3, 4))


@pytest.mark.parametrize("factor,wshape,cshape,what", [
    (3, (81, 3, 4), (3, 4), "factor must be 2, 4 or 8"),
    (16, (2304, 3, 4), (3, 4), "factor must be 2, 4 or 8"),
    (0, (0, 3, 4), (3, 4), "factor must be 2, 4 or 8"),
    (8, (575, 3, 4), (3, 4), "576 weight channels, got 575"),
    (8, (577, 3, 4), (3, 4), "576 weight channels, got 577"),
    (4, (576, 3, 4), (3, 4), "144 weight channels"),
    (2, (36, 3, 5), (3, 4), "same height and width"),
    (2, (36, 4, 4), (3, 4), "same height and width"),
    (2, (2, 36, 4, 3), (3, 4), "same height and width"),
    (2, (36, 4), (3, 4), "not \\(C, h, w\\)"),
    (2, (36, 1, 16384), (1, 16384), "beyond"),
    (8, (576, 4096, 2), (4096, 2), "beyond"),
])
def test_upsample_args_value_errors(factor, wshape, cshape, what):
    with pytest.raises(ValueError, match="Error upsampling flow: .*" + what):
        args.upsample_args(factor, wshape, cshape)


# ---------------------------------------------------------------------------------------------- the host forms
def test_host_forms_check_arguments_before_the_device():
    f = of.Flow.zero((3, 4), 't')
    good = np.zeros((36, 3, 4), np.float32)
    with pytest.raises(TypeError, match="numpy array"):
        f.upsample_convex(good.tolist(), 2)
    with pytest.raises(TypeError, match="float32 or float16"):
        f.upsample_convex(good.astype(np.float64), 2)
    with pytest.raises(TypeError, match="factor"):
        f.upsample_convex(good, 2.0)
    with pytest.raises(ValueError, match="576 weight channels"):
        f.upsample_convex(good)                                    # the default factor is 8
    with pytest.raises(ValueError, match="same height and width"):
        f.upsample_convex(np.zeros((36, 4, 3), np.float16), 2)
    with pytest.raises(ValueError, match=r"\(C, h, w\)"):
        f.upsample_convex(good[None], 2)
    vecs, mask = np.zeros((3, 4, 2), np.float32), np.ones((3, 4), bool)
    with pytest.raises(ValueError, match="factor must be"):
        of.upsample_flow_convex(vecs, mask, good, 3)
    with pytest.raises(TypeError):
        of.upsample_flow_convex(vecs, mask, good.astype(np.int16), 2)
    assert 'upsample_flow_convex' in of.flow_operations.__all__ and of.upsample_flow_convex is of.flow_operations.upsample_flow_convex
