"""NumPy statement of K25 (oflibnumpy_amd/csrc/ofl_sequence.hip, include/ofl.h) on top of the oracle -- a helper of
test_sequence_host.py and test_gpu_sequence.py, not a test.

A sequence of L fields of one reference is accumulated by folding the oracle's fused mode-3 composition, compose3_raw with
fb = the accumulated field and fa = the next field, in the walk order of the definition: k = 0, 1, ..., L - 1 for sign +1
('s'), k = L - 1, ..., 0 for sign -1 ('t').  The partial results are the accumulated field after each step, stored at the
index of the field taken last; lost_at is the index of the field at which a pixel's mask first became 0 (the first-walked
index for a pixel unset there), -1 for a pixel still set at the end.  Floats are compared with consistency_ref._same_floats,
which leaves NaN payloads free; masks and lost_at with array_equal."""
import functools

import numpy as np

from oracle import np_oracle as O
from consistency_ref import _same_floats, smooth, SHAPES, SIGNS, QUANTS          # noqa: F401 (re-exported to the tests)

F32 = np.float32
LENGTHS = [1, 2, 3, 5, 8]
LARGER = [s for s in SHAPES if s != (5, 7)]
SEED = 7


def walk(length, sign):
    """the batch indices in the order the fields are taken"""
    return list(range(length)) if sign > 0 else list(range(length - 1, -1, -1))


def fold(vecs, masks, sign, quant=O.QUANT_OPENCV):
    """vecs (L, H, W, 2), masks (L, H, W) -> (out float32 (H, W, 2), mout bool (H, W), part_vecs float32 (L, H, W, 2),
    part_masks bool (L, H, W), lost_at int32 (H, W))"""
    vecs = np.ascontiguousarray(vecs, F32)
    masks = np.asarray(masks).astype(bool)
    order = walk(len(vecs), sign)
    acc, m = vecs[order[0]].copy(), masks[order[0]].copy()
    part_vecs, part_masks = np.empty_like(vecs), np.empty_like(masks)
    part_vecs[order[0]], part_masks[order[0]] = acc, m
    lost_at = np.where(m, -1, order[0]).astype(np.int32)
    for k in order[1:]:
        acc, m = O.compose3_raw(vecs[k], masks[k], acc, m, sign, quant)
        part_vecs[k], part_masks[k] = acc, m
        lost_at[(lost_at < 0) & ~m] = k
    return acc, m, part_vecs, part_masks, lost_at


# ------------------------------------------------------------------------------------------------- the input generator
def sequence(shape, length, seed=SEED):
    """(vecs (L, H, W, 2) float32, masks (L, H, W) bool): smooth fields plus a constant drift -- 3 px and (1.5, -1.0) at the
    larger shapes, 1 px and 0.3 of the drift at (5, 7), which is there for the index arithmetic --, every odd-indexed field
    with a mask hole"""
    h, w = shape
    small = shape == (5, 7)
    rng = np.random.default_rng(seed)
    drift = np.array([1.5, -1.0], F32) * F32(0.3 if small else 1.0)
    vecs = np.stack([smooth(rng, h, w, 1.0 if small else 3.0) + drift for _ in range(length)]).astype(F32)
    masks = np.ones((length, h, w), bool)
    masks[1::2, h // 4:h // 2, w // 8:w // 3] = False
    return vecs, masks


def check_conditions(shape, length, sign, want):
    """what the generated inputs must exercise (they were folded through the oracle when the generator was chosen: at the
    larger shapes every index that can lose a pixel by stepping occurs in lost_at and the final valid share lies between
    0.34 and 0.91; at (5, 7) the smallest valid share is 0.11).  L = 1 cannot lose a pixel by stepping."""
    if length < 2:
        return
    _, mout, _, _, lost_at = want
    share = float(mout.mean())
    if shape == (5, 7):
        assert share > 0, (shape, length, sign, share)
        return
    assert share >= 0.25, (shape, length, sign, share)
    seen = set(np.unique(lost_at).tolist())
    assert set(walk(length, sign)[1:]) <= seen, (shape, length, sign, sorted(seen))


@functools.lru_cache(maxsize=None)
def case(shape, length, sign, quant, seed=SEED):
    """(inputs, expected) of one generated case, computed once and shared; read-only"""
    inputs = sequence(shape, length, seed)
    want = fold(*inputs, sign, quant)
    if seed == SEED:
        check_conditions(shape, length, sign, want)
    for a in inputs + want:
        a.flags.writeable = False
    return inputs, want


# ------------------------------------------------------------------------------------------------- the known answer
def translations(shape=(19, 70), steps=((3, -2), (1, 4), (-2, 1), (4, 2))):
    """L integer translations on all-valid masks -> (vecs, masks)"""
    vecs = np.stack([np.broadcast_to(np.array(v, F32), shape + (2,)) for v in steps]).astype(F32)
    return vecs, np.ones((len(steps),) + shape, bool)


def translations_answer(shape, steps, sign):
    """(sum, mask, lost_at) of the walk through integer translations, analytically: the sample position before taking
    field k is x + sign * (the sum of the fields walked so far); the pixel is lost at the first k whose position is outside"""
    h, w = shape
    ys, xs = np.mgrid[:h, :w]
    order = walk(len(steps), sign)
    lost_at = np.full(shape, -1, np.int32)
    total = np.array(steps[order[0]], np.int64)
    for k in order[1:]:
        px, py = xs + sign * total[0], ys + sign * total[1]
        outside = (px < 0) | (px > w - 1) | (py < 0) | (py > h - 1)
        lost_at[(lost_at < 0) & outside] = k
        total = total + np.array(steps[k], np.int64)
    return total.astype(F32), lost_at < 0, lost_at
