"""K25 (ofl_sequence.hip): a sequence of fields accumulated into one on the device, bit for bit against
tests/sequence_ref.py (the oracle's fused composition folded in the walk order), against the chain of compose-kernel launches
it replaces on the device itself, and through every layer: the raw ABI, the host entry, DeviceFlowBatch.combine_sequence and
of.combine_flow_sequence.  Nothing here has a tolerance: vectors are compared bit for bit (a NaN may carry any payload),
masks and lost_at with array_equal."""
import itertools

import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import devmem
import sequence_ref as R

pytestmark = pytest.mark.gpu
nat = of.native
GUARD = 256


def same(got, want, what):
    assert got.shape == want.shape and R._same_floats(np.ascontiguousarray(got), np.ascontiguousarray(want)), what


def raw_call(flows_ptr, masks_ptr, sign, shape, length, n_seq=1, quant=nat.QUANT_OPENCV, partials=True, lost_at=True):
    """ofl_compose_sequence_dev with every output between guard bands -> (out, mout, part_vecs | None, part_masks | None,
    lost_at | None) on the host; the guards of every buffer, the ones not handed to the call included, are checked"""
    h, w = shape
    px, n = n_seq * h * w, n_seq * length * h * w
    sizes = {"out": px * 8, "mout": px, "pv": n * 8, "pm": n, "lost": px * 4}
    bufs = {k: devmem.guarded(v, GUARD, GUARD) for k, v in sizes.items()}
    given = {"out": True, "mout": True, "pv": partials, "pm": partials, "lost": lost_at}
    ptr = lambda k: bufs[k].ptr + GUARD if given[k] else None
    nat.check(nat.load().ofl_compose_sequence_dev(flows_ptr, masks_ptr, sign, h, w, length, n_seq, ptr("out"), ptr("mout"),
                                                  ptr("pv"), ptr("pm"), ptr("lost"), quant, None))
    dev.sync()
    lead = (n_seq,) if n_seq > 1 else ()
    many = (n_seq, length) if n_seq > 1 else (length,)
    read = lambda k, dtype, shp: devmem.read_guarded(bufs[k], GUARD, sizes[k], GUARD, dtype, shp)
    res = (read("out", np.float32, lead + (h, w, 2)), read("mout", np.uint8, lead + (h, w)),
           read("pv", np.float32, many + (h, w, 2)), read("pm", np.uint8, many + (h, w)), read("lost", np.int32, lead + (h, w)))
    for k, i in (("pv", 2), ("pm", 3), ("lost", 4)):
        if not given[k]:                                    # an output the call was not given is never written
            assert (res[i].view(np.uint8) == 0xA5).all(), k
    return tuple(r if given[k] else None for r, k in zip(res, ("out", "mout", "pv", "pm", "lost")))


def check(got, want, what, partials=True, lost_at=True):
    out, mout, pv, pm, lost = want
    same(got[0], out, what + " out")
    np.testing.assert_array_equal(got[1], mout.astype(np.uint8), err_msg=what + " mout")
    if partials:
        same(got[2], pv, what + " partial vectors")
        np.testing.assert_array_equal(got[3], pm.astype(np.uint8), err_msg=what + " partial masks")
    else:
        assert got[2] is None and got[3] is None
    if lost_at:
        np.testing.assert_array_equal(got[4], lost, err_msg=what + " lost_at")
    else:
        assert got[4] is None


# ---------------------------------------------------------------------------------------------- 1: the raw ABI against the restatement
@pytest.mark.parametrize("shape", R.SHAPES)
def test_raw_entry_against_the_reference(gpu, shape):
    for length, sign, quant in itertools.product(R.LENGTHS, R.SIGNS, R.QUANTS):
        (vecs, masks), want = R.case(shape, length, sign, quant)
        (fbuf, fptr), (mbuf, mptr) = devmem.place(vecs), devmem.place(masks.view(np.uint8), shift=3)
        for partials, lost_at in ((True, True), (False, False), (True, False), (False, True)):
            what = "{} L {} sign {} quant {} partials {} lost_at {}".format(shape, length, sign, quant, partials, lost_at)
            got = raw_call(fptr, mptr, sign, shape, length, quant=quant, partials=partials, lost_at=lost_at)
            check(got, want, what, partials, lost_at)
        # the inputs are unchanged
        np.testing.assert_array_equal(fbuf.to_host(vecs.shape, np.float32).view(np.uint32), vecs.view(np.uint32))
        np.testing.assert_array_equal(mbuf.to_host((masks.size + 3,), np.uint8)[3:], masks.view(np.uint8).ravel())


@pytest.mark.parametrize("shape,length", [((5, 7), 2), ((19, 70), 3), ((37, 131), 5)])
def test_three_sequences_in_one_launch(gpu, shape, length):
    for sign, quant in itertools.product(R.SIGNS, R.QUANTS):
        cases = [R.case(shape, length, sign, quant, seed) for seed in (R.SEED, R.SEED + 1, R.SEED + 2)]
        (_, fptr), (_, mptr) = (devmem.place(np.stack([c[0][0] for c in cases])),
                                devmem.place(np.stack([c[0][1] for c in cases]).view(np.uint8)))
        assert not np.array_equal(cases[0][0][0], cases[1][0][0])
        for partials, lost_at in ((True, True), (False, False)):
            got = raw_call(fptr, mptr, sign, shape, length, n_seq=3, quant=quant, partials=partials, lost_at=lost_at)
            for i, (_, want) in enumerate(cases):
                check(tuple(None if g is None else g[i] for g in got), want, "{} sequence {} sign {} quant {}".format(shape, i, sign, quant),
                      partials, lost_at)


# ---------------------------------------------------------------------------------------------- 2: against the compose kernel
def make_batch(vecs, masks, ref):
    n, h, w = masks.shape
    b = DeviceFlowBatch(n, (h, w), ref)
    v, m = np.ascontiguousarray(vecs, np.float32), np.ascontiguousarray(masks).view(np.uint8)
    nat.check(nat.load().ofl_upload(b.vecs.ptr, v.ctypes.data, v.nbytes, None))
    nat.check(nat.load().ofl_upload(b.mask.ptr, m.ctypes.data, m.nbytes, None))
    dev.sync()
    return b


@pytest.mark.parametrize("shape", R.LARGER)
def test_fused_launch_equals_the_chain_of_compose_launches(gpu, shape):
    """(19, 70) and (64, 256) take K2's tiled path, (37, 131) its generic one: the plain gather is pinned against both"""
    for length, (ref, sign), quant in itertools.product(R.LENGTHS, (('s', 1), ('t', -1)), R.QUANTS):
        (vecs, masks), _ = R.case(shape, length, sign, quant)
        batch = make_batch(vecs, masks, ref)
        order = R.walk(length, sign)
        acc = batch.field(order[0])
        for k in order[1:]:
            nxt = dev.DeviceFlow.empty(shape, ref)
            dev.compose3_launch(batch.field(k), acc, sign, nxt, quant=quant)
            acc = nxt
        fused = batch.combine_sequence(quant=quant)
        assert isinstance(fused, dev.DeviceFlow) and fused.ref == ref and fused.shape == shape
        (fv, fm), (cv, cm) = fused.to_host(), acc.to_host()
        what = "{} L {} ref {} quant {}".format(shape, length, ref, quant)
        np.testing.assert_array_equal(fv.view(np.uint32), cv.view(np.uint32), err_msg=what)
        np.testing.assert_array_equal(fm, cm, err_msg=what)


# ---------------------------------------------------------------------------------------------- 3: through every layer
def method_chain(fields, ref):
    """the DeviceFlow.combine_with(..., 3) chain in the stated association; no operand may take a zero-flow early exit"""
    def live(f):
        assert not any(f.is_zero(thresholded=t, masked=m) for t in (False, True) for m in (False, True))
        return f
    steps = {}
    if ref == 's':
        acc = live(fields[0])
        steps[0] = acc
        for k in range(1, len(fields)):
            acc = live(acc).combine_with(live(fields[k]), 3)
            steps[k] = acc
    else:
        acc = live(fields[-1])
        steps[len(fields) - 1] = acc
        for k in range(len(fields) - 2, -1, -1):
            acc = live(fields[k]).combine_with(live(acc), 3)
            steps[k] = acc
    return acc, steps


@pytest.mark.parametrize("ref", ['s', 't'])
def test_batch_method_splits_six_fields_into_two_sequences(gpu, ref):
    shape, sign = (19, 70), (1 if ref == 's' else -1)
    cases = [R.case(shape, 3, sign, nat.QUANT_OPENCV, seed) for seed in (R.SEED, R.SEED + 1)]
    vecs, masks = np.concatenate([c[0][0] for c in cases]), np.concatenate([c[0][1] for c in cases])
    batch = make_batch(vecs, masks, ref)
    chains = [method_chain([batch.field(3 * s + k) for k in range(3)], ref) for s in range(2)]
    for b in (batch, batch.pack()):
        if b.packed:                    # a packed batch must answer from its bit planes
            b._mask = None
        res, parts, lost = b.combine_sequence(length=3, return_partials=True, return_lost_at=True)
        assert isinstance(res, DeviceFlowBatch) and (res.n, res.shape, res.ref, res.packed) == (2, shape, ref, False)
        assert isinstance(parts, DeviceFlowBatch) and (parts.n, parts.shape, parts.ref) == (6, shape, ref)
        lost = lost.to_host((2,) + shape, np.int32)
        for s, ((_, (out, mout, pv, pm, lost_at)), (end, steps)) in enumerate(zip(cases, chains)):
            v, m = res.field(s).to_host()
            same(v, out, "sequence {}".format(s))
            np.testing.assert_array_equal(m, mout)
            np.testing.assert_array_equal(lost[s], lost_at)
            cv, cm = end.to_host()
            np.testing.assert_array_equal(v.view(np.uint32), cv.view(np.uint32))
            np.testing.assert_array_equal(m, cm)
            for k in range(3):
                v, m = parts.field(3 * s + k).to_host()
                same(v, pv[k], "partial {} of sequence {}".format(k, s))
                np.testing.assert_array_equal(m, pm[k])
                cv, cm = steps[k].to_host()
                np.testing.assert_array_equal(v.view(np.uint32), cv.view(np.uint32))
                np.testing.assert_array_equal(m, cm)
        # the other shapes of the answer
        assert isinstance(b.combine_sequence(length=3), DeviceFlowBatch)
        whole = b.combine_sequence()
        assert isinstance(whole, dev.DeviceFlow) and whole.shape == shape
        one, lost1 = b.combine_sequence(length=6, return_lost_at=True)
        assert isinstance(one, DeviceFlowBatch) and one.n == 1 and lost1.nbytes >= shape[0] * shape[1] * 4
        np.testing.assert_array_equal(one.field(0).to_host()[0].view(np.uint32), whole.to_host()[0].view(np.uint32))
        each = b.combine_sequence(length=1)                   # L = 1 copies the fields
        np.testing.assert_array_equal(each.vecs.to_host(vecs.shape, np.float32).view(np.uint32), vecs.view(np.uint32))
        np.testing.assert_array_equal(each.mask.to_host(masks.shape, np.uint8), masks.view(np.uint8))
    with pytest.raises(ValueError, match="Length"):
        batch.combine_sequence(length=4)
    with pytest.raises(TypeError, match="Return_partials"):
        batch.combine_sequence(return_partials=1)
    # the inputs are unchanged
    np.testing.assert_array_equal(batch.vecs.to_host(vecs.shape, np.float32).view(np.uint32), vecs.view(np.uint32))
    np.testing.assert_array_equal(batch.mask.to_host(masks.shape, np.uint8), masks.view(np.uint8))


@pytest.mark.parametrize("ref", ['s', 't'])
def test_host_function_with_flows_and_with_arrays(gpu, ref):
    shape, length, sign = (37, 131), 5, (1 if ref == 's' else -1)
    for quant in R.QUANTS:
        (vecs, masks), (out, mout, pv, pm, lost_at) = R.case(shape, length, sign, quant)
        flows = [of.Flow(vecs[k], ref, masks[k]) for k in range(length)]
        res, parts, lost = of.combine_flow_sequence(flows, quant=quant, return_partials=True, return_lost_at=True)
        assert isinstance(res, of.Flow) and res.ref == ref and isinstance(parts, list) and len(parts) == length
        assert lost.dtype == np.int32 and lost.shape == shape
        same(res.vecs, out, "flows")
        np.testing.assert_array_equal(res.mask, mout)
        np.testing.assert_array_equal(lost, lost_at)
        for k in range(length):
            assert isinstance(parts[k], of.Flow) and parts[k].ref == ref
            same(parts[k].vecs, pv[k], "partial {}".format(k))
            np.testing.assert_array_equal(parts[k].mask, pm[k])
        a_res, a_lost = of.combine_flow_sequence(vecs, ref, masks, quant=quant, return_lost_at=True)
        same(a_res.vecs, out, "arrays")
        np.testing.assert_array_equal(a_res.mask, mout)
        np.testing.assert_array_equal(a_lost, lost_at)
        plain = of.combine_flow_sequence(flows, quant=quant)
        assert isinstance(plain, of.Flow)
        same(plain.vecs, out, "no extras")
        # arrays without masks: all valid
        free = of.combine_flow_sequence(vecs, ref, quant=quant)
        f_out, f_mout, _, _, _ = R.fold(vecs, np.ones_like(masks), sign, quant)
        same(free.vecs, f_out, "arrays, no masks")
        np.testing.assert_array_equal(free.mask, f_mout)
    # the chain of Flow.combine_with calls it replaces, in the stated association
    (vecs, masks), _ = R.case(shape, length, sign, nat.QUANT_OPENCV)
    end, _ = method_chain([dev.DeviceFlow.from_host(vecs[k], ref, masks[k]) for k in range(length)], ref)
    res = of.combine_flow_sequence(vecs, ref, masks)
    cv, cm = end.to_host()
    np.testing.assert_array_equal(res.vecs.view(np.uint32), cv.view(np.uint32))
    np.testing.assert_array_equal(res.mask, cm)


def test_host_entry_with_two_sequences(gpu):
    shape, length, sign, quant = (19, 70), 3, -1, nat.QUANT_EXACT
    cases = [R.case(shape, length, sign, quant, seed) for seed in (R.SEED, R.SEED + 1)]
    vecs = np.ascontiguousarray(np.stack([c[0][0] for c in cases]))
    masks = np.ascontiguousarray(np.stack([c[0][1] for c in cases])).view(np.uint8)
    out, mout = np.empty((2,) + shape + (2,), np.float32), np.empty((2,) + shape, np.uint8)
    pv, pm = np.empty((2, length) + shape + (2,), np.float32), np.empty((2, length) + shape, np.uint8)
    lost = np.empty((2,) + shape, np.int32)
    lib = nat.load()
    nat.check(lib.ofl_compose_sequence(vecs.ctypes.data, masks.ctypes.data, sign, shape[0], shape[1], length, 2, out.ctypes.data,
                                       mout.ctypes.data, pv.ctypes.data, pm.ctypes.data, lost.ctypes.data, quant))
    for i, (_, want) in enumerate(cases):
        check((out[i], mout[i], pv[i], pm[i], lost[i]), want, "host entry, sequence {}".format(i))
    out2, mout2 = np.full_like(out, 7), np.full_like(mout, 7)
    nat.check(lib.ofl_compose_sequence(vecs.ctypes.data, masks.ctypes.data, sign, shape[0], shape[1], length, 2, out2.ctypes.data,
                                       mout2.ctypes.data, None, None, None, quant))
    np.testing.assert_array_equal(out2.view(np.uint32), out.view(np.uint32))
    np.testing.assert_array_equal(mout2, mout)
    assert lib.ofl_compose_sequence(vecs.ctypes.data, masks.ctypes.data, sign, shape[0], shape[1], length, 2, out2.ctypes.data,
                                    mout2.ctypes.data, pv.ctypes.data, None, None, quant) == nat.E_INVALID
    assert "ofl_compose_sequence" in nat.last_error()


# ---------------------------------------------------------------------------------------------- 4: non-finite vectors
@pytest.mark.parametrize("quant", R.QUANTS)
@pytest.mark.parametrize("sign", R.SIGNS)
def test_non_finite_vectors_follow_the_rules_of_the_header(gpu, sign, quant):
    """NaN / +-Inf vectors in the first-walked field and in a middle field: the result is the restatement's; once a pixel's
    accumulated vector is not finite it samples nothing, so it is invalid from the next step on"""
    shape, length = (19, 70), 5
    (vecs, masks), _ = R.case(shape, length, sign, quant)
    vecs = vecs.copy()
    order = R.walk(length, sign)
    nan, inf = np.float32('nan'), np.float32('inf')
    bad = [(nan, 1.0), (0.5, nan), (nan, nan), (inf, 0.0), (0.0, -inf), (-inf, inf), (inf, nan)]
    spots = {order[0]: [(2, 3), (9, 35), (18, 69), (0, 0), (12, 64), (7, 63), (15, 20)],
             order[2]: [(3, 5), (10, 30), (17, 68), (0, 1), (13, 63), (6, 64), (14, 40)]}
    for k, where in spots.items():
        for (y, x), v in zip(where, bad):
            vecs[k, y, x] = v
    want = R.fold(vecs, masks, sign, quant)
    pv, pm = want[2], want[3]
    assert not np.isfinite(want[0]).all()
    for i, k in enumerate(order[:-1]):
        gone = ~np.isfinite(pv[k]).all(axis=-1)
        assert gone.any()
        for later in order[i + 1:]:
            assert not pm[later][gone].any() and not np.isfinite(pv[later][gone]).all(axis=-1).any()
    # a neighbour that samples the non-finite tap of the middle field carries it on, a tap of weight 0 included
    assert (~np.isfinite(pv[order[2]]).all(axis=-1)).sum() > (~np.isfinite(pv[order[1]]).all(axis=-1)).sum()
    (_, fptr), (_, mptr) = devmem.place(vecs), devmem.place(masks.view(np.uint8))
    check(raw_call(fptr, mptr, sign, shape, length, quant=quant), want, "non-finite sign {} quant {}".format(sign, quant))


# ---------------------------------------------------------------------------------------------- 5: refusals
def test_raw_entry_refuses_bad_arguments_without_launching(gpu):
    lib = nat.load()
    h, w, length = 6, 9, 3
    px = h * w
    flows, masks = dev.DeviceBuffer.zeros(length * px * 8 + 8), dev.DeviceBuffer.zeros(length * px)
    out, mout = dev.DeviceBuffer(px * 8 + 8), dev.DeviceBuffer(px)
    pv, pm, lost = dev.DeviceBuffer(length * px * 8 + 8), dev.DeviceBuffer(length * px), dev.DeviceBuffer(px * 4 + 4)
    for b in (out, mout, pv, pm, lost):
        nat.check(lib.ofl_memset(b.ptr, 7, b.nbytes, None))

    def call(sign=1, L=length, S=1, hh=h, ww=w, quant=nat.QUANT_OPENCV, f_ptr=flows.ptr, m_ptr=masks.ptr, out_ptr=out.ptr,
             mout_ptr=mout.ptr, pv_ptr=pv.ptr, pm_ptr=pm.ptr, lost_ptr=lost.ptr):
        return lib.ofl_compose_sequence_dev(f_ptr, m_ptr, sign, hh, ww, L, S, out_ptr, mout_ptr, pv_ptr, pm_ptr, lost_ptr, quant, None)

    for kw in (dict(sign=0), dict(sign=2), dict(L=0), dict(L=-1), dict(S=0), dict(S=65536), dict(hh=0), dict(ww=-1), dict(ww=32767),
               dict(quant=7), dict(f_ptr=None), dict(m_ptr=None), dict(out_ptr=None), dict(mout_ptr=None),
               dict(f_ptr=flows.ptr + 4), dict(out_ptr=out.ptr + 4), dict(pv_ptr=pv.ptr + 4), dict(lost_ptr=lost.ptr + 2),
               dict(pv_ptr=None), dict(pm_ptr=None),
               dict(out_ptr=flows.ptr), dict(mout_ptr=masks.ptr + px), dict(pv_ptr=flows.ptr), dict(pm_ptr=masks.ptr),
               dict(lost_ptr=flows.ptr + 8), dict(mout_ptr=out.ptr), dict(pm_ptr=pv.ptr + 16)):
        assert call(**kw) == nat.E_INVALID, kw
        assert "ofl_compose_sequence" in nat.last_error(), kw
    dev.sync()
    for b in (out, mout, pv, pm, lost):
        assert (b.to_host((b.nbytes,), np.uint8) == 7).all()          # nothing was launched
    assert call() == nat.OK
    assert call(pv_ptr=None, pm_ptr=None, lost_ptr=None) == nat.OK
    dev.sync()
    assert not out.to_host((px * 8,), np.uint8).any() and not mout.to_host((px,), np.uint8).any()   # zero fields, empty masks
    np.testing.assert_array_equal(lost.to_host((px,), np.int32), 0)     # every pixel is unset in the first-walked field, k0 = 0
