"""Register budget of the fused mode-3 compose kernel (CPU only: a gfx950 compile with the build's flags).

compose3_xpose_kernel<Q, S, false> must fit the waves per SIMD its __launch_bounds__ asks for (kC3Waves) with no spills and
no scratch, and with TotalSGPRs <= 80, the count at which eight 256-thread workgroups are admitted per CU.  A small change
that quietly spills, or that drops residency back, fails here before it reaches the hardware.  The host-side routing of
fields too large for the kernel's 32-bit offsets is checked on a compiled copy of its header."""
import os
import re
import subprocess
import tempfile

import pytest

from oflibnumpy_amd import build_native as bn
import kernel_resources
from kernel_resources import FIELDS

COMPOSE3 = os.path.join(bn.CSRC, "ofl_compose3.hip")
KERNEL = re.compile(r"compose3_xpose_kernelILi([01])ELb([01])ELb0E")


def _waves():
    m = re.search(r"^constexpr int kC3Waves = (\d+);", open(COMPOSE3).read(), re.M)
    assert m, "kC3Waves not found in ofl_compose3.hip"
    return int(m.group(1))


def _key(name):
    k = KERNEL.search(name)
    return (int(k.group(1)), bool(int(k.group(2)))) if k else None


@pytest.fixture(scope="module")
def usage():
    return kernel_resources.usage(COMPOSE3, _key)


@pytest.mark.parametrize("quant", [0, 1])
@pytest.mark.parametrize("stats", [True, False])
def test_compose3_xpose_register_budget(usage, quant, stats):
    u = usage.get((quant, stats))
    assert u and len(u) == len(FIELDS), f"no resource remarks for compose3_xpose_kernel<{quant}, {stats}, false>"
    waves = _waves()
    assert waves >= 6, "kC3Waves below the 6 waves per SIMD the kernel has reached: residency given back"
    vgpr_cap = (512 // waves) // 8 * 8                      # VGPRs allocate in granules of 8 of the SIMD's 512 per lane
    assert u["vgprs"] <= vgpr_cap, u
    assert u["sgprs"] <= 80, u                              # <= 80: eight 256-thread workgroups per CU
    assert u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0, u
    assert u["lds"] <= 9728, u


def test_compose3_route_threshold():
    """Fields whose float2 vector plane reaches 4 GiB (and odd widths) leave the tiled kernel for the generic one."""
    src = r'''
#include "ofl_compose3_route.h"
#include <stdio.h>
int main() {
    using ofl::c3_tiled_fits;
    static_assert(c3_tiled_fits(2160, 3840) && c3_tiled_fits(4320, 7680), "benchmark sizes stay tiled");
    static_assert(!c3_tiled_fits(2160, 3841), "odd widths go to the generic kernel");
    static_assert(c3_tiled_fits(16384, 32766) && c3_tiled_fits(32766, 16384), "2^29 - 2^15 px: tiled");
    static_assert(!c3_tiled_fits(23170, 23172) && c3_tiled_fits(23170, 23170), "threshold at H * W = 2^29");
    static_assert(!c3_tiled_fits(32766, 32766), "largest admissible field: generic kernel");
    puts("ok");
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "route.cpp")
        open(c, "w").write(src)
        exe = os.path.join(d, "route")
        r = subprocess.run(["c++", "-std=c++17", "-I", bn.CSRC, c, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([exe], capture_output=True, text=True).stdout.strip() == "ok"
