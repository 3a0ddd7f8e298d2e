"""Register budget of the photometric kernels (CPU only: a gfx950 compile with the build's flags).

Every instantiation of csrc/ofl_photometric.hip -- photo_nchw_kernel<E, QUANT, CN>, 3 element types x 2 quantisations x the
five channel-count variants (1 to 4, and 0 for any), and photo_nhwc_kernel<E, QUANT, WIDE>, 3 x 2 x the two load shapes --
must use no scratch and spill nothing.  The planar
kernel keeps 16 partial sums in a register array that only unrolled loops with constant indices touch; a change that
indexes it with the channel gets scratch and fails here before it reaches the hardware."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

SOURCE = os.path.join(bn.CSRC, "ofl_photometric.hip")
NCHW = re.compile(r"photo_nchw_kernelILi(\d)ELi(\d)ELi(\d)EE")
NHWC = re.compile(r"photo_nhwc_kernelILi(\d)ELi(\d)ELb([01])EE")


def _key(name):
    k = NCHW.search(name)
    if k:
        return ("nchw", int(k.group(1)), int(k.group(2)), int(k.group(3)))
    k = NHWC.search(name)
    assert k or "photo" not in name, "a photometric kernel this test does not know: " + name
    return ("nhwc", int(k.group(1)), int(k.group(2)), bool(int(k.group(3)))) if k else None


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(SOURCE, _key)


def test_every_instantiation_is_found(usage):
    want = {("nchw", e, q, cn) for e in (0, 1, 2) for q in (0, 1) for cn in range(5)}
    want |= {("nhwc", e, q, wide) for e in (0, 1, 2) for q in (0, 1) for wide in (False, True)}
    assert set(usage) == want and len(want) == 42


def test_no_scratch_and_no_spills(usage):
    assert usage
    for inst, u in sorted(usage.items(), key=str):
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["vgprs"] <= 128 and u["occupancy"] >= 4, (inst, u)      # four waves per SIMD at least
        if inst[0] == "nhwc" or inst[3] > 0:                              # the streaming variants stay at full residency
            assert u["vgprs"] <= 64 and u["occupancy"] >= 8, (inst, u)
        assert u["lds"] <= 64, (inst, u)                                  # the eight words of the counts, nothing else
