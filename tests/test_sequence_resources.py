"""Register and LDS budget of the sequence-accumulation kernel (CPU only: a gfx950 compile with the build's flags).

sequence_kernel<QUANT> of csrc/ofl_sequence.hip, 2 quantisations (the partial results and lost_at are uniform run-time
branches), must use no scratch, spill nothing and have no LDS: the accumulated vector, the mask bit and the lost index stay in
registers over the walk.  Each lane makes L - 1 dependent gathers, so occupancy is what hides their latency.

Reached by this build: 34 VGPRs and 8 waves per SIMD in both instantiations (52 - 54 SGPRs); the floor K21 - K24 assert
(128 VGPRs, 4 waves) is asserted here too."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

SOURCE = os.path.join(bn.CSRC, "ofl_sequence.hip")
KERNEL = re.compile(r"sequence_kernelILi(\d)EE")


def _key(name):
    m = KERNEL.search(name)
    if m:
        return int(m.group(1))
    assert "sequence" not in name, "a sequence kernel this test does not know: " + name
    return None


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(SOURCE, _key)


def test_both_instantiations_are_found(usage):
    assert set(usage) == {0, 1}


def test_no_scratch_no_spills_no_lds_and_four_waves(usage):
    assert usage
    for inst, u in sorted(usage.items()):
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["lds"] == 0, (inst, u)
        assert u["vgprs"] <= 128 and u["occupancy"] >= 4, (inst, u)      # K21's floor for its general kernel
