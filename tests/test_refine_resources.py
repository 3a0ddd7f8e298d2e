"""Register and LDS budget of the refinement kernels (CPU only: a gfx950 compile with the build's flags).

Every kernel of csrc/ofl_refine.hip -- refine_setup_kernel<E, QUANT>: 3 element types x 2 quantisations (the layout and the
channel count are run-time strides and a uniform loop bound), and the weights, sweep and finish kernels, which have no
template arguments -- must use no scratch and spill nothing: the solver kernels keep the four neighbours of a pixel in
register arrays that only unrolled loops with constant indices touch.

LDS: only the setup kernel has any.  The tile of 64 x 16 pixels with a halo of 1 is 66 x 18 entries of two float planes and
one byte plane (K22's staging), 9 bytes an entry; there are no counts, so nothing follows."""
import os
import re

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

SOURCE = os.path.join(bn.CSRC, "ofl_refine.hip")
SETUP = re.compile(r"refine_setup_kernelILi(\d)ELi(\d)EE")
PLAIN = re.compile(r"refine_(weights|sweep|finish)_kernel")


def _key(name):
    k, p = SETUP.search(name), PLAIN.search(name)
    assert k or p or "refine" not in name, "a refinement kernel this test does not know: " + name
    return ("setup", int(k.group(1)), int(k.group(2))) if k else ((p.group(1),) if p else None)


def lds_bytes():
    return 9 * (64 + 2) * (16 + 2)


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(SOURCE, _key)


def test_every_kernel_is_found(usage):
    want = {("setup", e, q) for e in (0, 1, 2) for q in (0, 1)} | {("weights",), ("sweep",), ("finish",)}
    assert set(usage) == want and len(want) == 9


def test_no_scratch_no_spills_and_four_waves(usage):
    assert usage
    for inst, u in sorted(usage.items()):
        assert len(u) == len(FIELDS), (inst, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (inst, u)
        assert u["vgprs"] <= 128 and u["occupancy"] >= 4, (inst, u)      # K21's floor for its general kernel


def test_lds_is_the_tile_formula(usage):
    assert lds_bytes() == 10692
    for inst, u in sorted(usage.items()):
        assert u["lds"] == (lds_bytes() if inst[0] == "setup" else 0), (inst, u)
