"""Register and LDS budget of the correlation lookup kernel (CPU only: a gfx950 compile with the build's flags).

Every instantiation corr_kernel<E1, E2, K> of csrc/ofl_correlation.hip -- 3 x 3 element types x 4 channel routes (K = 2, 4: the
pixel's f1 channels in registers for C <= 128, 256; K = 0: any C; K = -1: element by element) -- and the three avgpool kernels
must use no scratch, spill nothing, fit the waves per SIMD the __launch_bounds__ of corr_kernel names (kWaves) in registers,
and keep the LDS of a workgroup -- the dots of 32 pixels and their weights -- small enough that LDS does not limit that
residency either."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

SOURCE = os.path.join(bn.CSRC, "ofl_correlation.hip")
CORR = re.compile(r"corr_kernelILi(\d)ELi(\d)ELi(n?\d)EE")
POOL = re.compile(r"avgpool_kernelILi(\d)EE")
LDS_PER_CU = 160 * 1024
BLOCK_WAVES = 4


def _waves():
    m = re.search(r"^constexpr int kWaves  = (\d+);", open(SOURCE).read(), re.M)
    assert m, "kWaves not found in ofl_correlation.hip"
    return int(m.group(1))


def _key(name):
    k, p = CORR.search(name), POOL.search(name)
    assert k or p, "a kernel this test does not know: " + name
    return ("corr",) + tuple(int(k.group(i).replace("n", "-")) for i in (1, 2, 3)) if k else ("pool", int(p.group(1)))


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(SOURCE, _key)


def test_every_instantiation_is_found(usage):
    # (OFL_EL_F16 / BF16 / F32 = 0 / 1 / 2 of f1 and of f2, K)
    want = {("corr", e1, e2, k) for e1 in (0, 1, 2) for e2 in (0, 1, 2) for k in (2, 4, 0, -1)} | {("pool", e) for e in (0, 1, 2)}
    assert set(usage) == want


def test_no_scratch_no_spills_and_the_named_residency(usage):
    assert len(usage) == 39
    waves = _waves()
    assert 1 <= waves <= 8
    vgpr_cap = (512 // waves) // 8 * 8                      # VGPRs allocate in granules of 8 of the SIMD's 512 per lane
    for inst, u in sorted(usage.items()):
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["vgprs"] <= vgpr_cap and u["occupancy"] >= waves, (inst, u)
        if inst[0] == "corr":
            blocks_per_cu = 4 * u["occupancy"] // BLOCK_WAVES      # what the reported residency on each of the four SIMDs holds
            assert 0 < u["lds"] and u["lds"] * blocks_per_cu <= LDS_PER_CU, (inst, u)
        else:
            assert u["lds"] == 0, (inst, u)
