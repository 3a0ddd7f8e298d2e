"""Register and LDS budget of the SSIM kernel (CPU only: a gfx950 compile with the build's flags).

Every instantiation of csrc/ofl_ssim.hip -- ssim_kernel<E, QUANT, K>: 3 element types x 2 quantisations x the windows 3, 5,
7, 11; the layout and the channel count are run-time strides and a uniform loop bound -- must use no scratch and spill
nothing: the window phase keeps the six row sums and the six sums of each of a thread's four centres in register arrays that
only unrolled loops with constant indices touch, and the taps are read from the kernel arguments at constant offsets; a
change that indexes either with a run-time row counter gets scratch and fails here before it reaches the hardware.

LDS, as the kernel's header comment states it: only the staged tile -- (64 + 2r) x (16 + 2r) entries of two float planes and
one byte plane, 9 bytes an entry -- and, on the next 16-byte boundary, the eight words of the counts (K21's scheme)."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

SOURCE = os.path.join(bn.CSRC, "ofl_ssim.hip")
KERNEL = re.compile(r"ssim_kernelILi(\d)ELi(\d)ELi(\d+)EE")


def _key(name):
    k = KERNEL.search(name)
    assert k or "ssim" not in name, "an SSIM kernel this test does not know: " + name
    return tuple(int(k.group(i)) for i in range(1, 4)) if k else None


def lds_bytes(K):
    r = K // 2
    entries = (64 + 2 * r) * (16 + 2 * r)
    return (9 * entries + 15) // 16 * 16 + 4 * 2 * 4


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(SOURCE, _key)


def test_every_instantiation_is_found(usage):
    want = {(e, q, K) for e in (0, 1, 2) for q in (0, 1) for K in (3, 5, 7, 11)}
    assert set(usage) == want and len(want) == 24


def test_no_scratch_no_spills_and_four_waves(usage):
    assert usage
    for inst, u in sorted(usage.items()):
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["vgprs"] <= 128 and u["occupancy"] >= 4, (inst, u)


def test_lds_is_the_tile_formula(usage):
    assert [lds_bytes(K) for K in (3, 5, 7, 11)] == [10736, 12272, 13904, 17360]
    for inst, u in sorted(usage.items()):
        assert u["lds"] == lds_bytes(inst[2]), (inst, u)
