"""GPU suite: every producer and consumer of the four zero-flow predicates against the one case table of tests/zero_cases.py,
word for word and without a tolerance.

Producers: K4 (ofl_flow_stats_dev); ofl_compose3_dev with flag words -- both quantisations (the store-only flush and
c3_flush_stats_late), both signs, a batch of one and of three different rows, zeroed and pre-set rows; ofl_compose3_bits_dev
on the even widths; the generic kernel at (9, 37).  The contract of a launch into the row `before`:
    words 4..7   == before | oracle(fb, mb): a NaN component counts as non-zero and as >= threshold, as in the reference;
    words 0/1    certificates for fa: never set unless the oracle predicate of (fa, ma) holds, and SET when a finite masked
                 vector that fulfils it is gathered as a top-left tap (zero_cases.observed); exact in the generic kernel;
    words 2/3    keep their value (tiled) / exact (generic);
    outputs      equal to O.compose3_raw, NaN for NaN and bytes elsewhere, between intact guard bytes.
Consumers: DeviceFlow.combine_with(mode=3) on fresh objects, after stats() on both operands, and a second time on the objects
of the first call (whose cached word then comes from the fused launch) agree with each other and with O.OFlow.combine_with --
the same operand handed back, or the same computed field -- and so do DeviceFlowBatch.compose3 and combine_flows_batch.

Before C3Stat kept bit patterns, the tiled kernels failed here on every row whose field is non-zero only through NaN under the
mask (words 4/5, and 6/7 where nothing else sets them; combine_with handed back the partner).  Values only: nothing can fault."""
import numpy as np
import pytest

import devmem as D
import nonfinite_cases as N
import stream_ref as S
import zero_cases as Z
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64
QUANTS = [O.QUANT_OPENCV, O.QUANT_EXACT]
SIGNS = [-1, 1]
SHAPE_PLACEMENTS = [(s, p) for s in Z.SHAPES for p in Z.PLACEMENTS if Z.pixels(p, s) is not None]
SP_IDS = ["{}x{}-{}".format(*s, p) for s, p in SHAPE_PLACEMENTS]
EVEN = [s for s in Z.SHAPES if Z.is_tiled(s)]


def _indexed(shape, placement=None):
    return [(i, r) for i, r in enumerate(Z.rows(shape)) if placement is None or r['placement'] == placement]


def _upload(*arrays):
    return [D.place(np.ascontiguousarray(a)) for a in arrays]


def _unchanged(bufs, arrays, tag):
    for (buf, _), a in zip(bufs, arrays):
        a = np.ascontiguousarray(a)
        assert np.array_equal(buf.to_host((a.nbytes,), np.uint8), a.reshape(-1).view(np.uint8)), ("input changed", tag)


def _read(buf, want):
    return D.read_guarded(buf, 0, want.nbytes, GUARD, want.dtype, want.shape)


def _preset(index):
    """a flag row with some words already set, different from row to row"""
    return np.array([((11 * index + 5) >> k) & 1 for k in range(8)], np.uint32)


def check_words(got, before, r, sign, quant, tag):
    print(tag, "before", before.tolist(), "after", got.tolist(), "fb", r['expect_b'], "fa", r['expect_a'])
    assert set(got.tolist()) <= {0, 1}, (tag, got)
    for k in range(4):
        assert bool(got[4 + k]) == (r['expect_b'][k] or bool(before[4 + k])), (tag, "word", 4 + k, got, r['expect_b'])
    if not Z.is_tiled(r['shape']):                # the generic kernel: all eight words exact
        for k in range(4):
            assert bool(got[k]) == (r['expect_a'][k] or bool(before[k])), (tag, "word", k, got, r['expect_a'])
        return
    assert got[2] == before[2] and got[3] == before[3], (tag, got)
    must = Z.observed(r, sign, quant)
    for k in (0, 1):
        if before[k]:
            assert got[k] == 1, (tag, "word", k, got)
            continue
        if got[k]:
            assert r['expect_a'][k], (tag, "word", k, "set although the oracle predicate of fa is false", got)
        if must[k]:
            assert got[k] == 1, (tag, "word", k, "a gathered finite vector did not set it", got)


def check_outputs(out, mout, want, tag):
    w_out, w_m = want
    np.testing.assert_array_equal(_read(mout, w_m), w_m, err_msg=str(tag))
    assert N.same_floats(_read(out, w_out), w_out), tag


# ================================================================================================ K4
@pytest.mark.parametrize("shape", Z.SHAPES, ids=str)
def test_flow_stats_word(gpu, shape):
    """bits 0..3 are the oracle's predicates, NONFINITE exactly when the field holds a non-finite component, MASK_HAS_ZERO by
    the mask: the whole word equals the restatement"""
    nat, lib = gpu.native, gpu.native.load()
    n = shape[0] * shape[1]
    for r in Z.rows(shape):
        fields = [('fb', r['fb'], r['mb'], r['expect_b'], r['nonfinite_b'])]
        if r['kind'] == 'fa':
            fields.append(('fa', r['fa'], r['ma'], r['expect_a'], r['nonfinite_a']))
        for which, vecs, mask, expect, nonfinite in fields:
            (dv, pv), (dm, pm) = _upload(vecs, mask)
            word = D.guarded(4, GUARD)
            nat.check(lib.ofl_flow_stats_dev(pv, pm, n, S.TH, word.ptr, None))
            got = int(D.read_guarded(word, 0, 4, GUARD, np.uint32, (1,))[0])
            assert [bool(got & (1 << k)) for k in range(4)] == expect, (r['name'], which, got)
            assert bool(got & S.NONFINITE) == nonfinite, (r['name'], which, got)
            assert got == S.stats_word(vecs, mask), (r['name'], which, got)


# ================================================================================================ K2, one field per launch
@pytest.mark.parametrize("shape,placement", SHAPE_PLACEMENTS, ids=SP_IDS)
def test_compose3_flag_words(gpu, shape, placement):
    from oflibnumpy_amd import device as dev
    nat, lib = gpu.native, gpu.native.load()
    H, W = shape
    for index, r in _indexed(shape, placement):
        arrays = (r['fa'], r['ma'], r['fb'], r['mb'])
        bufs = _upload(*arrays)
        (_, fa), (_, ma), (_, fb), (_, mb) = bufs
        for sign in SIGNS:
            for quant in QUANTS:
                want = Z.want(shape, index, sign, quant)
                for before in (np.zeros(8, np.uint32), _preset(index)):
                    out, mout = D.guarded(want[0].nbytes, GUARD), D.guarded(want[1].nbytes, GUARD)
                    words = dev.DeviceBuffer.from_host(before)
                    nat.check(lib.ofl_compose3_dev(fa, ma, fb, mb, sign, H, W, 1, out.ptr, mout.ptr, words.ptr, quant, None))
                    tag = (r['name'], 'sign', sign, 'quant', quant)
                    check_words(words.to_host((8,), np.uint32), before, r, sign, quant, tag)
                    check_outputs(out, mout, want, tag)
            if Z.is_tiled(shape):
                want = Z.want(shape, index, sign, O.QUANT_OPENCV)
                ba, bb = dev.mask_pack(bufs[1][0], H, W, 1), dev.mask_pack(bufs[3][0], H, W, 1)
                for before in (np.zeros(8, np.uint32), _preset(index + 1)):
                    out, bo = D.guarded(want[0].nbytes, GUARD), dev.DeviceBuffer.zeros(dev.mask_bits_bytes(H, W, 1))
                    words = dev.DeviceBuffer.from_host(before)
                    dev.compose3_bits_launch(bufs[0][0], ba, bufs[2][0], bb, sign, (H, W), out, bo, words, batch=1)
                    tag = (r['name'], 'sign', sign, 'bits')
                    check_words(words.to_host((8,), np.uint32), before, r, sign, O.QUANT_OPENCV, tag)
                    np.testing.assert_array_equal(dev.mask_unpack(bo, H, W, 1).to_host((H, W), np.uint8), want[1], err_msg=str(tag))
                    assert N.same_floats(_read(out, want[0]), want[0]), tag
        _unchanged(bufs, arrays, r['name'])


# ================================================================================================ K2, three different rows per launch
@pytest.mark.parametrize("shape", Z.SHAPES, ids=str)
def test_compose3_flag_words_batch_of_three(gpu, shape):
    """A different row of the table per field: a row takes nothing from its neighbours.  Every row of the shape is in one triple."""
    from oflibnumpy_amd import device as dev
    nat, lib = gpu.native, gpu.native.load()
    H, W = shape
    rows = _indexed(shape)
    third = len(rows) // 3
    assert third * 3 == len(rows)
    for k in range(third):
        trio = [rows[k], rows[k + third], rows[k + 2 * third]]
        arrays = [np.stack([r[key] for _, r in trio]) for key in ('fa', 'ma', 'fb', 'mb')]
        bufs = _upload(*arrays)
        (_, fa), (_, ma), (_, fb), (_, mb) = bufs
        sign, quant = SIGNS[k % 2], QUANTS[(k // 2) % 2]
        wants = [Z.want(shape, i, sign, quant) for i, _ in trio]
        want = (np.stack([w[0] for w in wants]), np.stack([w[1] for w in wants]))
        before = np.zeros((3, 8), np.uint32)
        out, mout = D.guarded(want[0].nbytes, GUARD), D.guarded(want[1].nbytes, GUARD)
        words = dev.DeviceBuffer.from_host(before)
        nat.check(lib.ofl_compose3_dev(fa, ma, fb, mb, sign, H, W, 3, out.ptr, mout.ptr, words.ptr, quant, None))
        got = words.to_host((3, 8), np.uint32)
        for b, (_, r) in enumerate(trio):
            check_words(got[b], before[b], r, sign, quant, ('batch', k, b, r['name'], sign, quant))
        check_outputs(out, mout, want, ('batch', k))
        if Z.is_tiled(shape) and quant == O.QUANT_OPENCV:
            ba, bb = dev.mask_pack(bufs[1][0], H, W, 3), dev.mask_pack(bufs[3][0], H, W, 3)
            out, bo = D.guarded(want[0].nbytes, GUARD), dev.DeviceBuffer.zeros(dev.mask_bits_bytes(H, W, 3))
            words = dev.DeviceBuffer.from_host(before)
            dev.compose3_bits_launch(bufs[0][0], ba, bufs[2][0], bb, sign, (H, W), out, bo, words, batch=3)
            got = words.to_host((3, 8), np.uint32)
            for b, (_, r) in enumerate(trio):
                check_words(got[b], before[b], r, sign, quant, ('batch bits', k, b, r['name'], sign))
            np.testing.assert_array_equal(dev.mask_unpack(bo, H, W, 3).to_host((3, H, W), np.uint8), want[1], err_msg=str(('batch bits', k)))
            assert N.same_floats(_read(out, want[0]), want[0]), ('batch bits', k)


# ================================================================================================ consumers
def _operands(dev, r, ref, first):
    op = dev.DeviceFlow.from_host(r['fb'], ref, r['mb'])
    pa = dev.DeviceFlow.from_host(Z.partner(r['shape']), ref)
    return (op, pa, op) if first else (pa, op, op)


def _same_answer(res, a, b, oracle, tag):
    how, vecs, mask = oracle
    if how == 'self':
        assert res is a, (tag, "the oracle hands back self")
    elif how == 'flow':
        assert res is b, (tag, "the oracle hands back flow")
    else:
        assert res is not a and res is not b, (tag, "an early exit where the oracle computes a field")
        got_v, got_m = res.to_host()
        np.testing.assert_array_equal(got_m, mask, err_msg=str(tag))
        assert N.same_floats(got_v, vecs), tag


@pytest.mark.parametrize("ref", ['t', 's'])
@pytest.mark.parametrize("shape", Z.SHAPES, ids=str)
def test_combine_with_does_not_depend_on_what_ran_before(gpu, shape, ref):
    from oflibnumpy_amd import device as dev
    for index, r in Z.consumer_rows(shape):
        fresh = dev.DeviceFlow.from_host(r['fb'], ref, r['mb'])
        zero = {(t, m): fresh.is_zero(t, m) for t in (False, True) for m in (False, True)}              # K4
        assert [not zero[(False, True)], not zero[(True, True)], not zero[(False, False)], not zero[(True, False)]] == r['expect_b'], r['name']
        for thresholded in (False, True):
            for first in (True, False):
                oracle = Z.oracle_combine(shape, index, ref, thresholded, first)
                tag = (r['name'], ref, 'thresholded', thresholded, 'operand first', first, 'oracle', oracle[0])
                a, b, op = _operands(dev, r, ref, first)                                               # (a) fresh objects
                _same_answer(a.combine_with(b, 3, thresholded), a, b, oracle, tag + ('fresh',))
                for (t, m), z in zero.items():
                    assert op.is_zero(t, m) == z, (tag, "is_zero after the fused launch", t, m)
                _same_answer(a.combine_with(b, 3, thresholded), a, b, oracle, tag + ('second call',))  # (c) the same objects again
                a, b, op = _operands(dev, r, ref, first)                                               # (b) after stats() on both
                a.stats(), b.stats()
                _same_answer(a.combine_with(b, 3, thresholded), a, b, oracle, tag + ('after stats',))


@pytest.mark.parametrize("ref", ['t', 's'])
@pytest.mark.parametrize("shape", Z.SHAPES, ids=str)
def test_batch_compose3_and_per_pair_exits(gpu, shape, ref):
    """DeviceFlowBatch.compose3 over all consumer rows at once (byte masks, and bit planes on the even widths): fields equal to
    O.compose3_raw, words 4..7 the operand's predicates, and the per-pair exits that combine_flows_batch derives from the words
    equal to the oracle's.  combine_flows_batch itself takes Flow objects, which refuse NaN and Inf as the reference does: it
    is run on the finite rows and must raise on the others."""
    of = gpu
    from oflibnumpy_amd import device as dev
    from oflibnumpy_amd.batch import DeviceFlowBatch
    H, W = shape
    rows = Z.consumer_rows(shape)
    n = len(rows)
    op_v, op_m = np.stack([r['fb'] for _, r in rows]), np.stack([r['mb'] for _, r in rows])
    pa_v, pa_m = np.stack([Z.partner(shape)] * n), np.ones((n, H, W), np.uint8)
    wrap = lambda v, m: DeviceFlowBatch.wrap(n, shape, ref, dev.DeviceBuffer.from_host(np.ascontiguousarray(v)), dev.DeviceBuffer.from_host(np.ascontiguousarray(m)))
    # the operand is the STREAMED field fb: `flow` for 't' (self = partner), `self` for 's' (flow = partner)
    b_self, b_flow = (wrap(pa_v, pa_m), wrap(op_v, op_m)) if ref == 't' else (wrap(op_v, op_m), wrap(pa_v, pa_m))
    sign = -1 if ref == 't' else 1
    for packed in ((False, True) if Z.is_tiled(shape) else (False,)):
        out, words, _ = (b_self.pack() if packed else b_self).compose3(b_flow.pack() if packed else b_flow)
        got_v, got_m = out.vecs.to_host((n, H, W, 2), np.float32), out.mask.to_host((n, H, W), np.uint8)
        for k, (index, r) in enumerate(rows):
            tag = (r['name'], ref, 'packed', packed)
            assert [bool(x) for x in words[k][4:8]] == r['expect_b'], (tag, words[k])
            # the partner is gathered: certificates set; words 2/3 untouched by the tiled kernel, exact in the generic one
            assert words[k][:4].tolist() == ([1, 1, 0, 0] if Z.is_tiled(shape) else [1, 1, 1, 1]), (tag, words[k])
            w_v, w_m = O.compose3_raw(Z.partner(shape), np.ones((H, W), np.uint8), r['fb'], r['mb'], sign, O.QUANT_OPENCV)
            np.testing.assert_array_equal(got_m[k], w_m.astype(np.uint8), err_msg=str(tag))
            assert N.same_floats(got_v[k], w_v), tag
            for thresholded in (False, True):
                # combine_flows_batch's reading of the words (batch.py): fb zero <=> word 4 + bit clear
                fb_zero = not words[k][4 + (1 if thresholded else 0)]
                how = Z.oracle_combine(shape, index, ref, thresholded, ref == 's')[0]
                assert fb_zero == (how != 'computed'), (tag, thresholded, how, words[k])
    for k, (index, r) in enumerate(rows):
        f_op = lambda: of.Flow(r['fb'], ref, r['mb'].astype(bool))
        if r['value'] in Z.NONFINITE_VALUES:
            with pytest.raises(ValueError):
                f_op()
            continue
        op, pa = f_op(), of.Flow(Z.partner(shape), ref)
        for thresholded in (False, True):
            for first in (True, False):
                a, b = (op, pa) if first else (pa, op)
                (_, res), = of.combine_flows_batch([a], [b], thresholded=thresholded)
                how, vecs, mask = Z.oracle_combine(shape, index, ref, thresholded, first)
                tag = (r['name'], ref, thresholded, first, how)
                if how == 'computed':
                    assert res is not a and res is not b, tag
                    np.testing.assert_array_equal(res.mask, mask, err_msg=str(tag))
                    assert N.same_floats(np.ascontiguousarray(res.vecs), vecs), tag
                else:
                    assert res is (a if how == 'self' else b), tag
