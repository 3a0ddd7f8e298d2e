"""The argument checks the image-pair families K21 ... K24 and K26 share, at the ten native entries: ofl_photometric, ofl_census,
ofl_ssim, ofl_refine, ofl_inverse_search and their _dev forms.  One argument of the shared set is invalid at a time, every call
fails validation -- no kernel is launched -- and the return code and the exact ofl_last_error text are pinned."""
import numpy as np
import pytest

from oflibnumpy_amd import _native as nat
from oflibnumpy_amd import device as dev

pytestmark = pytest.mark.gpu

F32, U8 = np.float32, np.uint8
H = W = 8
PX = H * W
MAX_C = {'photometric': 65535, 'census': 4, 'ssim': 4, 'refine': 4, 'inverse_search': 4}
FAMILIES = sorted(MAX_C)
TAPS = np.ones(3, F32)                          # K26's window, a host array in both forms

# the shared arguments of a good call: 8 x 8, three channels of float32
GOOD = dict(elem=nat.EL_F32, layout=nat.TENSOR_NCHW, N=1, C=3, H=H, W=W, sign=1, quant=nat.QUANT_OPENCV)


def _messages(family):
    who, max_c = "ofl_" + family, MAX_C[family]
    return [
        (dict(elem=7), who + ": elem must be OFL_EL_F16, OFL_EL_BF16 or OFL_EL_F32, got 7"),
        (dict(layout=5), who + ": bad layout 5"),
        (dict(N=0), who + ": N must be in [1, 65535], got 0"),
        (dict(C=0), who + ": C must be in [1, {}], got 0".format(max_c)),
        (dict(C=max_c + 1), who + ": C must be in [1, {}], got {}".format(max_c, max_c + 1)),
        (dict(H=0), who + ": H, W must be in [1, 32766] (got 0 x 8)"),
        (dict(sign=0), who + ": sign must be +1 or -1"),
        (dict(quant=2), who + ": bad quant"),
    ]


class _Device:
    """pointers into device buffers: every entry's `_dev` form"""
    def __init__(self):
        self.keep = [dev.DeviceBuffer.zeros(n) for n in (PX * 3 * 4 + 8, PX * 8, PX, PX * 8, PX, PX, 64 * PX)]
        self.t, self.flow, self.fmask, self.out, self.o1, self.o2, self.work = (b.ptr for b in self.keep)
        self.work_bytes = 64 * PX
        self.tail = (None,)                     # the stream


class _Host:
    """pointers into NumPy arrays: every entry's host form"""
    def __init__(self):
        self.keep = [np.zeros(n, U8) for n in (PX * 3 * 4 + 8, PX * 8, PX, PX * 8, PX, PX)]
        self.t, self.flow, self.fmask, self.out, self.o1, self.o2 = (a.ctypes.data for a in self.keep)
        self.tail = ()


def _call(family, m, near=None, **change):
    """the entry of `family` in the form of `m` with the shared arguments of GOOD, `change` applied"""
    a = dict(GOOD, **change)
    lib, on_device = nat.load(), isinstance(m, _Device)
    fn = getattr(lib, "ofl_" + family + ("_dev" if on_device else ""))
    head = (m.t if near is None else near, m.t, a['elem'], a['layout'], a['N'], a['C'], a['H'], a['W'], m.flow, m.fmask)
    work = (m.work, m.work_bytes) if on_device else ()
    if family == 'photometric':
        return fn(*head, 1, a['sign'], None, None, nat.PHOTO_L1, F32(0), F32(0), m.out, m.o1, None, None, a['quant'], *m.tail)
    if family == 'census':
        return fn(*head, 1, a['sign'], None, None, 3, nat.CENSUS_HARD, F32(0), F32(0), 8, F32(0), m.out, m.o1, None, None,
                  a['quant'], *m.tail)
    if family == 'ssim':
        return fn(*head, 1, a['sign'], None, None, 3, TAPS.ctypes.data, F32(1), F32(1), 9, F32(0), m.out, m.o1, None, None,
                  a['quant'], *m.tail)
    if family == 'refine':
        return fn(*head, a['sign'], None, None, None, F32(20), F32(5), F32(0.1), F32(0.1), 1, 1, F32(1.6), *work, m.out, m.o1,
                  a['quant'], *m.tail)
    return fn(*head, a['sign'], 8, 4, 1, 1, F32(1), *work, m.out, m.o1, None, None, a['quant'], *m.tail)


@pytest.fixture(scope="module")
def memory(gpu):
    return {'dev': _Device(), 'host': _Host()}


@pytest.mark.parametrize("form", ['dev', 'host'])
@pytest.mark.parametrize("family", FAMILIES)
def test_one_invalid_shared_argument_at_a_time(memory, family, form):
    m = memory[form]
    for change, text in _messages(family):
        assert _call(family, m, **change) == nat.E_INVALID, (family, form, change)
        assert nat.last_error() == text, (family, form, change)


@pytest.mark.parametrize("family", FAMILIES)
def test_misaligned_near_at_the_device_entry(memory, family):
    m = memory['dev']
    assert _call(family, m, near=m.t + 1) == nat.E_INVALID
    assert nat.last_error() == "ofl_{}: near and far must be aligned to the element size".format(family)
