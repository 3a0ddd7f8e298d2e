"""Register and LDS budget of the inverse-search kernels (CPU only: a gfx950 compile with the build's flags).

Every kernel of csrc/ofl_inverse_search.hip -- isearch_setup_kernel<E>: 3 element types (the layout and the channel count are
run-time strides and a uniform loop bound); isearch_search_kernel<P, QUANT>: 2 patch sizes x 2 quantisations;
isearch_densify_kernel<QUANT>: 2 quantisations -- must use no scratch and spill nothing, and none has LDS: the sums of a patch
cross the lanes of its wave, T, gx and gy of a pixel stay in registers over the iterations.

Reached by this build: setup 10 VGPRs, search 47 - 50, densify 37 - 39; 8 waves per SIMD in all nine, so the floor K21 - K23
assert (128 VGPRs, 4 waves) is asserted here too."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

SOURCE = os.path.join(bn.CSRC, "ofl_inverse_search.hip")
SETUP = re.compile(r"isearch_setup_kernelILi(\d)EE")
SEARCH = re.compile(r"isearch_search_kernelILi(\d)ELi(\d)EE")
DENSIFY = re.compile(r"isearch_densify_kernelILi(\d)EE")


def _key(name):
    for kind, rx in (("setup", SETUP), ("search", SEARCH), ("densify", DENSIFY)):
        m = rx.search(name)
        if m:
            return (kind,) + tuple(int(g) for g in m.groups())
    assert "isearch" not in name, "an inverse-search kernel this test does not know: " + name
    return None


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(SOURCE, _key)


def test_every_kernel_is_found(usage):
    want = ({("setup", e) for e in (0, 1, 2)} | {("search", p, q) for p in (4, 8) for q in (0, 1)} |
            {("densify", q) for q in (0, 1)})
    assert set(usage) == want and len(want) == 9


def test_no_scratch_no_spills_no_lds_and_four_waves(usage):
    assert usage
    for inst, u in sorted(usage.items()):
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["lds"] == 0, (inst, u)
        assert u["vgprs"] <= 128 and u["occupancy"] >= 4, (inst, u)      # K21's floor for its general kernel
