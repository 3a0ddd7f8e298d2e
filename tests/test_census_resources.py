"""Register and LDS budget of the census kernel (CPU only: a gfx950 compile with the build's flags).

Every instantiation of csrc/ofl_census.hip -- census_kernel<E, QUANT, K, MODE>: 3 element types x 2 quantisations x the
windows 3, 5, 7 x hard / soft; the layout and the channel count are run-time strides and a uniform loop bound -- must use no
scratch and spill nothing: the window phase keeps the K values of a tile row and the four centres of a thread in register
arrays that only unrolled loops with constant indices touch, and a change that indexes one with the row counter gets scratch
and fails here before it reaches the hardware.

LDS: the tile of 64 x 16 pixels with a halo of r = K / 2 is (64 + 2r) x (16 + 2r) entries of two float planes and one byte
plane, 9 bytes an entry; the eight words of the counts (K21's scheme) follow on the next 16-byte boundary."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

SOURCE = os.path.join(bn.CSRC, "ofl_census.hip")
KERNEL = re.compile(r"census_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)EE")


def _key(name):
    k = KERNEL.search(name)
    assert k or "census" not in name, "a census kernel this test does not know: " + name
    return tuple(int(k.group(i)) for i in range(1, 5)) if k else None


def lds_bytes(K):
    r = K // 2
    entries = (64 + 2 * r) * (16 + 2 * r)
    return (9 * entries + 15) // 16 * 16 + 4 * 2 * 4


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(SOURCE, _key)


def test_every_instantiation_is_found(usage):
    want = {(e, q, K, mode) for e in (0, 1, 2) for q in (0, 1) for K in (3, 5, 7) for mode in (0, 1)}
    assert set(usage) == want and len(want) == 36


def test_no_scratch_no_spills_and_four_waves(usage):
    assert usage
    for inst, u in sorted(usage.items()):
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["vgprs"] <= 128 and u["occupancy"] >= 4, (inst, u)      # K21's floor for its general kernel


def test_lds_is_the_tile_formula(usage):
    assert [lds_bytes(K) for K in (3, 5, 7)] == [10736, 12272, 13904]
    for inst, u in sorted(usage.items()):
        assert u["lds"] == lds_bytes(inst[2]), (inst, u)
