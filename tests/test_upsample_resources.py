"""Register and LDS budget of the convex upsampling kernel (CPU only: a gfx950 compile with the build's flags).

Every instantiation upsample_kernel<F, E, LAYOUT> of csrc/ofl_upsample.hip -- 3 factors x 3 element types x 2 layouts -- must
use no scratch, spill nothing, fit the waves per SIMD its __launch_bounds__ names (kWaves) in registers, and keep its LDS -- the
staged coarse neighbourhood plus the band of fine rows -- small enough that LDS does not limit that residency either."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

UPSAMPLE = os.path.join(bn.CSRC, "ofl_upsample.hip")
KERNEL = re.compile(r"upsample_kernelILi(\d)ELi(\d)ELi(\d)EE")
LDS_PER_CU = 160 * 1024
NCHW = 0


def _waves():
    m = re.search(r"^constexpr int kWaves = (\d+);", open(UPSAMPLE).read(), re.M)
    assert m, "kWaves not found in ofl_upsample.hip"
    return int(m.group(1))


def _block_waves(factor, layout):
    """waves per workgroup: a planar block has one wave per sub-row, four at most; a channels-last block has four"""
    return min(factor, 4) if layout == NCHW else 4


def _key(name):
    k = KERNEL.search(name)
    assert k or "upsample" not in name, "an upsample kernel this test does not know: " + name
    return tuple(int(k.group(i)) for i in (1, 2, 3)) if k else None


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(UPSAMPLE, _key)


def test_every_instantiation_is_found(usage):
    # (factor, OFL_EL_F16 / BF16 / F32 = 0 / 1 / 2, OFL_TENSOR_NCHW / NHWC = 0 / 1)
    assert set(usage) == {(f, e, l) for f in (2, 4, 8) for e in (0, 1, 2) for l in (0, 1)}


def test_no_scratch_no_spills_and_the_named_residency(usage):
    assert len(usage) == 18
    waves = _waves()
    assert 1 <= waves <= 8
    vgpr_cap = (512 // waves) // 8 * 8                      # VGPRs allocate in granules of 8 of the SIMD's 512 per lane
    for inst, u in sorted(usage.items()):
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["vgprs"] <= vgpr_cap and u["occupancy"] >= waves, (inst, u)
        blocks_per_cu = 4 * waves // _block_waves(inst[0], inst[2])      # what kWaves waves on each of the four SIMDs hold
        assert u["lds"] * blocks_per_cu <= LDS_PER_CU, (inst, u)
