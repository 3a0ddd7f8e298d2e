"""Register budget of the median filter kernel (CPU only: a gfx950 compile with the build's flags).

Every instantiation median_kernel<K, VALID, ONLY, MASK> of csrc/ofl_median.hip -- 3 window sizes x 8 combinations of optional
pointers -- must use no scratch, spill nothing, and fit the waves per SIMD its __launch_bounds__ names (med_waves(K)).  The
window lives in a register array that only a sorting network with constant indices touches; a change that indexes it
dynamically gets scratch and fails here before it reaches the hardware."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

MEDIAN = os.path.join(bn.CSRC, "ofl_median.hip")
KERNEL = re.compile(r"median_kernelILi(\d)ELb([01])ELb([01])ELb([01])E")


def _waves(ksize):
    m = re.search(r"^constexpr int med_waves\(int k\) \{ return k == 7 \? (\d+) : (\d+); \}", open(MEDIAN).read(), re.M)
    assert m, "med_waves not found in ofl_median.hip"
    return int(m.group(1)) if ksize == 7 else int(m.group(2))


def _key(name):
    k = KERNEL.search(name)
    assert k or "median" not in name, "a median kernel this test does not know: " + name
    return (int(k.group(1)),) + tuple(bool(int(k.group(i))) for i in (2, 3, 4)) if k else None


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(MEDIAN, _key)


def test_every_instantiation_is_found(usage):
    want = {(k, v, o, m) for k in (3, 5, 7) for v in (False, True) for o in (False, True) for m in (False, True)}
    assert set(usage) == want


def test_no_scratch_no_spills_and_the_named_residency(usage):
    assert usage
    for inst, u in sorted(usage.items()):
        assert len(u) == len(FIELDS), (inst, u)
        waves = _waves(inst[0])
        assert 1 <= waves <= 8
        vgpr_cap = (512 // waves) // 8 * 8                  # VGPRs allocate in granules of 8 of the SIMD's 512 per lane
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["vgprs"] <= vgpr_cap and u["occupancy"] >= waves, (inst, u)
        assert u["lds"] <= 160 * 1024 // 8, (inst, u)        # eight workgroups of four waves per CU: LDS never limits residency
