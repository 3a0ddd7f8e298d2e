"""Register budget of the splat kernels (CPU only: a gfx950 compile with the build's flags).

Every instantiation of csrc/ofl_splat.hip -- accum_kernel<E, LAYOUT, SOFTMAX> over 3 element types x 2 layouts x {softmax,
not}, finish_kernel<E, LAYOUT> over 3 x 2, and the one max_kernel -- must be found, use no scratch and spill nothing."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

SPLAT = os.path.join(bn.CSRC, "ofl_splat.hip")
ACCUM = re.compile(r"accum_kernelILi(\d)ELi(\d)ELb([01])EE")
FINISH = re.compile(r"finish_kernelILi(\d)ELi(\d)EE")


def _key(name):
    a, f = ACCUM.search(name), FINISH.search(name)
    if a:
        return ("accum",) + tuple(int(a.group(i)) for i in (1, 2, 3))
    if f:
        return ("finish",) + tuple(int(f.group(i)) for i in (1, 2))
    if "max_kernel" in name:
        return ("max",)
    assert "kernel" not in name, "a splat kernel this test does not know: " + name
    return None


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(SPLAT, _key)


def test_every_splat_instantiation_is_found(usage):
    # OFL_EL_F16 / BF16 / F32 = 0 / 1 / 2, OFL_TENSOR_NCHW / NHWC = 0 / 1
    want = {("accum", e, l, s) for e in (0, 1, 2) for l in (0, 1) for s in (0, 1)}
    want |= {("finish", e, l) for e in (0, 1, 2) for l in (0, 1)} | {("max",)}
    assert set(usage) == want


def test_splat_kernels_use_no_scratch_and_spill_nothing(usage):
    assert len(usage) == 19
    for inst, u in sorted(usage.items()):
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
