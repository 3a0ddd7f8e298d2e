"""Register and LDS budget of the global matching kernel (CPU only: a gfx950 compile with the build's flags).

Every instantiation match_kernel<E, MODE, B> of csrc/ofl_match.hip -- 3 element types x 3 routes (MODE 0: the queries' operands
in registers, 1: aligned tensors of any C, 2: element by element) x B = 1 or 2 query blocks a wave -- must use no scratch,
spill nothing, fit the waves per SIMD its __launch_bounds__ names (kWavesOf[B]) in registers, and keep the LDS of a
workgroup -- the maxima and the sums of 32 B queries from four waves -- far below what would limit that residency.

Recorded with the build's compiler (16-bit / float32 vector registers, waves per SIMD): MODE 0 B = 1 132 / 132, 3; B = 2
176 / 184, 2; MODE 1 88 / 84, 5 and 110 / 106, 4; MODE 2 86 / 84, 5 and 108 / 106, 4; 2560 B bytes of LDS a workgroup."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

SOURCE = os.path.join(bn.CSRC, "ofl_match.hip")
MATCH = re.compile(r"match_kernelILi(\d)ELi(\d)ELi(\d)EE")
LDS_PER_CU = 160 * 1024
BLOCK_WAVES = 4


def _waves():
    """{B: waves per SIMD its __launch_bounds__ names}"""
    m = re.search(r"^constexpr int kWavesOf\[3\] = \{ 0, (\d+), (\d+) \};", open(SOURCE).read(), re.M)
    assert m, "kWavesOf not found in ofl_match.hip"
    return {1: int(m.group(1)), 2: int(m.group(2))}


def _key(name):
    k = MATCH.search(name)
    assert k, "a kernel this test does not know: " + name
    return int(k.group(1)), int(k.group(2)), int(k.group(3))


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(SOURCE, _key)


def test_every_instantiation_is_found(usage):
    assert set(usage) == {(e, mode, b) for e in (0, 1, 2) for mode in (0, 1, 2) for b in (1, 2)}      # OFL_EL_F16 / BF16 / F32 = 0 / 1 / 2


def test_no_scratch_no_spills_and_the_named_residency(usage):
    for inst, u in sorted(usage.items()):
        waves = _waves()[inst[2]]
        assert 1 <= waves <= 8
        vgpr_cap = (512 // waves) // 8 * 8                  # VGPRs allocate in granules of 8 of the SIMD's 512 per lane
        print(inst, u)
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["vgprs"] <= vgpr_cap and u["occupancy"] >= waves, (inst, u)
        blocks_per_cu = 4 * u["occupancy"] // BLOCK_WAVES
        assert 0 < u["lds"] and u["lds"] * blocks_per_cu <= LDS_PER_CU, (inst, u)


def test_the_kernel_runs_on_the_matrix_cores():
    """the three builtins of the definition are what the source calls, one per element type"""
    text = open(SOURCE).read()
    for name in ("__builtin_amdgcn_mfma_f32_32x32x16_f16", "__builtin_amdgcn_mfma_f32_32x32x16_bf16", "__builtin_amdgcn_mfma_f32_32x32x2f32"):
        assert name in text, name
