"""Register and LDS budget of the correlation lookup kernel (CPU only: a gfx950 compile with the build's flags).

Every instantiation corr_kernel<E1, E2, K> of csrc/ofl_correlation.hip -- 3 x 3 element types x 4 channel routes (K = 2, 4: the
pixel's f1 channels in registers for C <= 128, 256; K = 0: any C; K = -1: element by element) -- and the three avgpool kernels
must use no scratch, spill nothing, fit the waves per SIMD the __launch_bounds__ of corr_kernel names (kWaves) in registers,
and keep the LDS of a workgroup -- the dots of 32 pixels and their weights -- small enough that LDS does not limit that
residency either."""
import os
import re
import subprocess
import tempfile

import pytest

from oflibnumpy_amd import build_native as bn

SOURCE = os.path.join(bn.CSRC, "ofl_correlation.hip")
CORR = re.compile(r"corr_kernelILi(\d)ELi(\d)ELi(n?\d)EE")
POOL = re.compile(r"avgpool_kernelILi(\d)EE")
FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "SGPRs Spill": "sgpr_spill",
          "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}
LDS_PER_CU = 160 * 1024
BLOCK_WAVES = 4


def _waves():
    m = re.search(r"^constexpr int kWaves  = (\d+);", open(SOURCE).read(), re.M)
    assert m, "kWaves not found in ofl_correlation.hip"
    return int(m.group(1))


@pytest.fixture(scope="module")
def usage():
    with tempfile.TemporaryDirectory() as d:
        cmd = [bn._hipcc()] + bn.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                         "-c", SOURCE, "-o", os.path.join(d, "c.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k, p = CORR.search(m.group(1)), POOL.search(m.group(1))
            assert k or p, "a kernel this test does not know: " + m.group(1)
            cur = ("corr",) + tuple(int(k.group(i).replace("n", "-")) for i in (1, 2, 3)) if k else ("pool", int(p.group(1)))
            out[cur] = {}
            continue
        if cur:
            m = re.search(r"remark:\s+(.+?): (\d+) \[", line)
            if m and m.group(1).split(":")[-1].strip() in FIELDS:
                out[cur][FIELDS[m.group(1).split(":")[-1].strip()]] = int(m.group(2))
    return out


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
