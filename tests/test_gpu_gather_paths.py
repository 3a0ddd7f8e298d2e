"""The image-gather kernels (K1: gather2_kernel / gather_kernel, ofl_gather.hip) on every branch they take, bit-exact against the
C oracle.  The cases come from tests/gather_cases.py; tests/test_gather_census_host.py proves on the CPU which branch each of
them reaches (flow load, transposed form, all outside / all inside / border, the read-ahead fallback, joined and per-pair stores),
a test's name is its case's, and every failure message adds the classes that the census finds in it.

Every destination buffer is filled with 0xA5 and has 64 guard bytes behind its end: every byte inside must be the oracle's,
every guard byte must still be 0xA5 -- a joined store that writes a lane too far, or skips one, shows either way."""
import numpy as np
import pytest

import gather_cases as G
import gather_census as gc

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5


def _classes(c, a):
    """the classes the census finds in a built case: part of every failure message"""
    seen, routes = set(), set()
    for b in range(c['batch']):
        r, tokens, _ = G.census_of(c, a, b)
        routes.add(r)
        seen.update(tokens)
    return gc.summary({k: 1 for k in seen}) if routes == {'paired'} else '+'.join(sorted(routes))


def _guarded(dev, nbytes):
    return dev.DeviceBuffer.from_host(np.full(nbytes + GUARD, FILL, np.uint8))


def _check(buf, want, what, tag):
    """all of `buf`: the bytes of `want`, then the untouched guard"""
    got = buf.to_host((want.nbytes + GUARD,), np.uint8)
    np.testing.assert_array_equal(got[:want.nbytes].view(want.dtype).reshape(want.shape), want, err_msg="{}: {}".format(what, tag))
    assert np.array_equal(got[:want.nbytes], np.ascontiguousarray(want).reshape(-1).view(np.uint8)), "{} bytes: {}".format(what, tag)
    assert (got[want.nbytes:] == FILL).all(), "{}: guard bytes overwritten: {}".format(what, tag)


@pytest.mark.parametrize("case", G.CASES, ids=[c['id'] for c in G.CASES])
def test_gather_paths_bit_exact(gpu, oracle, case):
    from oflibnumpy_amd import device as dev
    nat, lib = gpu.native, gpu.native.load()
    c = case
    a = G.build(c)
    want_img, want_val = G.expected(c, a, oracle)
    tag = "{} [{}]".format(c['id'], _classes(c, a))
    code = {gc.U8: nat.U8, gc.I16: nat.I16, gc.U16: nat.U16, gc.F32: nat.F32, gc.F64: nat.F64}[c['dtype']]
    up = lambda x: None if x is None else dev.DeviceBuffer.from_host(x)
    ptr = lambda b: None if b is None else b.ptr
    src, flow, smask, fmask = up(a['src']), up(a['flow']), up(a['smask']), up(a['fmask'])
    dst = _guarded(dev, want_img.nbytes)
    valid = _guarded(dev, want_val.nbytes) if c['valid'] else None
    if c['entry'] == 'single':
        nat.check(lib.ofl_gather_bilinear_dev(src.ptr, code, c['C'], c['H'], c['W'], flow.ptr, c['fH'], c['fW'], c['pad_top'],
                                              c['pad_left'], c['sign'], ptr(smask), ptr(fmask), dst.ptr, ptr(valid),
                                              c['quant'], c['arith'], c['rule'], None))
    elif c['entry'] == 'rows':
        nat.check(lib.ofl_gather_rows_dev(src.ptr, code, c['C'], c['H'], c['W'], c['row0'], c['rows'], flow.ptr, c['sign'],
                                          ptr(smask), ptr(fmask), dst.ptr, ptr(valid), c['quant'], c['arith'], c['rule'], None))
    else:
        nat.check(lib.ofl_gather_bilinear_batch_dev(src.ptr, int(c['shared']), code, c['C'], c['H'], c['W'], c['batch'], flow.ptr,
                                                    c['fH'], c['fW'], c['pad_top'], c['pad_left'], c['sign'], ptr(smask),
                                                    int(c['shared']), ptr(fmask), dst.ptr, ptr(valid), c['quant'], c['arith'],
                                                    c['rule'], None))
    _check(dst, want_img, "image", tag)
    if c['valid']:
        _check(valid, want_val, "validity", tag)
