"""The frame the three error-map entries K21, K22 and K26 share on the output side, at the six native entries: ofl_photometric,
ofl_census, ofl_ssim and their _dev forms.  Every call fails validation -- no kernel is launched -- and the return code and the
exact ofl_last_error text are pinned: one invalid argument at a time, and three pairs of invalid arguments that pin the order
of the checks (the NULL line, the shared arguments, the family's settings, err / within, tau).  The shared input side is
test_gpu_pair_args.py's."""
import numpy as np
import pytest

from oflibnumpy_amd import _native as nat
from oflibnumpy_amd import device as dev

pytestmark = pytest.mark.gpu

F32, U8 = np.float32, np.uint8
H = W = 8
PX = H * W
FAMILIES = ['census', 'photometric', 'ssim']
TAPS = np.ones(3, F32)                          # K26's window, a host array in both forms
# a family's own setting, invalid, and the message that names it
BAD_SETTING = {'photometric': (9, "ofl_photometric: bad metric 9"),
               'census': (4, "ofl_census: window must be 3, 5 or 7, got 4"),
               'ssim': (4, "ofl_ssim: window must be 3, 5, 7 or 11, got 4")}
GOOD_SETTING = {'photometric': nat.PHOTO_L1, 'census': 3, 'ssim': 3}

NULL_LINE = "ofl_{}: NULL pointer (near, far, flow and fmask are required)"
OUTPUTS = "ofl_{}: one of err and within is required"
TAU = "ofl_{}: tau must be finite and not negative (got {})"


class _Device:
    """pointers into device buffers: every entry's `_dev` form"""
    def __init__(self):
        self.keep = [dev.DeviceBuffer.zeros(n) for n in (PX * 3 * 4, PX * 8 + 8, PX, PX * 4 + 8, PX, PX, 16)]
        self.t, self.flow, self.fmask, self.err, self.covered, self.within, self.counts = (b.ptr for b in self.keep)
        self.tail = (None,)                     # the stream


class _Host:
    """pointers into NumPy arrays: every entry's host form"""
    def __init__(self):
        self.keep = [np.zeros(n, U8) for n in (PX * 3 * 4, PX * 8 + 8, PX, PX * 4 + 8, PX, PX, 16)]
        self.t, self.flow, self.fmask, self.err, self.covered, self.within, self.counts = (a.ctypes.data for a in self.keep)
        self.tail = ()


def _call(family, m, **change):
    """the entry of `family` in the form of `m`: a good call of 8 x 8, three channels of float32, err and covered given, with
    `change` applied (a pointer None: NULL; `setting`: the metric or the window)"""
    a = dict(near=m.t, far=m.t, flow=m.flow, fmask=m.fmask, err=m.err, covered=m.covered, within=None, counts=None,
             C=3, quant=nat.QUANT_OPENCV, tau=F32(0), setting=GOOD_SETTING[family])
    a.update(change)
    fn = getattr(nat.load(), "ofl_" + family + ("_dev" if isinstance(m, _Device) else ""))
    head = (a['near'], a['far'], nat.EL_F32, nat.TENSOR_NCHW, 1, a['C'], H, W, a['flow'], a['fmask'], 1, 1, None, None)
    tail = (F32(a['tau']), a['err'], a['covered'], a['within'], a['counts'], a['quant'], *m.tail)
    if family == 'photometric':
        return fn(*head, a['setting'], F32(0), *tail)
    if family == 'census':
        return fn(*head, a['setting'], nat.CENSUS_HARD, F32(0), F32(0), 8, *tail)
    return fn(*head, a['setting'], TAPS.ctypes.data, F32(1), F32(1), 9, *tail)


def _refused(family, m, text, **change):
    assert _call(family, m, **change) == nat.E_INVALID, (family, change)
    assert nat.last_error() == text, (family, change)


@pytest.fixture(scope="module")
def memory(gpu):
    return {'dev': _Device(), 'host': _Host()}


@pytest.mark.parametrize("form", ['dev', 'host'])
@pytest.mark.parametrize("family", FAMILIES)
def test_one_invalid_output_side_argument_at_a_time(memory, family, form):
    m = memory[form]
    for name in ('near', 'far', 'flow', 'fmask'):
        _refused(family, m, NULL_LINE.format(family), **{name: None})
    _refused(family, m, OUTPUTS.format(family), err=None, within=None)
    for tau, shown in ((-1.0, "-1"), (np.nan, "nan"), (np.inf, "inf")):
        _refused(family, m, TAU.format(family, shown), within=m.within, tau=tau)
        _refused(family, m, TAU.format(family, shown), err=None, within=m.within, tau=tau)


@pytest.mark.parametrize("family", FAMILIES)
def test_tau_is_not_looked_at_without_within(memory, family):
    """the rule is `within given`: with err alone a NaN tau passes the checks, and the next one names the alignment"""
    m = memory['dev']
    _refused(family, m, "ofl_{}: flow must be 8-byte aligned".format(family), tau=np.nan, flow=m.flow + 4)


@pytest.mark.parametrize("family", FAMILIES)
def test_misaligned_pointers_at_the_device_entry(memory, family):
    m = memory['dev']
    _refused(family, m, "ofl_{}: flow must be 8-byte aligned".format(family), flow=m.flow + 4)
    _refused(family, m, "ofl_{}: err and counts must be 4-byte aligned".format(family), err=m.err + 1)
    _refused(family, m, "ofl_{}: err and counts must be 4-byte aligned".format(family), counts=m.counts + 2)


@pytest.mark.parametrize("form", ['dev', 'host'])
@pytest.mark.parametrize("family", FAMILIES)
def test_the_order_of_the_checks(memory, family, form):
    m = memory[form]
    bad, names_it = BAD_SETTING[family]
    _refused(family, m, NULL_LINE.format(family), near=None, C=0)
    _refused(family, m, "ofl_{}: bad quant".format(family), quant=2, setting=bad)
    _refused(family, m, names_it, setting=bad, err=None, within=None)
