"""What the compiler reports a source file's kernels to use (CPU only: a gfx950 device compile with the build's flags and
-Rpass-analysis=kernel-resource-usage).  The register-budget tests share the compile and the walk over the remarks; which
kernels they look at, and what they ask of them, is theirs."""
import os
import re
import subprocess
import tempfile

from oflibnumpy_amd import build_native as bn

FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "SGPRs Spill": "sgpr_spill",
          "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}


def usage(source, key):
    """{key(mangled kernel name): {sgprs, vgprs, scratch, sgpr_spill, vgpr_spill, lds, occupancy}} of every kernel of
    `source`; a kernel for which `key` returns None is left out (`key` may also refuse a name it does not know)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = [bn._hipcc()] + bn.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                         "-c", source, "-o", os.path.join(d, "k.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = key(m.group(1))
            if cur is not None:
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[", line)
        if m and cur is not None and m.group(1).split(":")[-1].strip() in FIELDS:
            out[cur][FIELDS[m.group(1).split(":")[-1].strip()]] = int(m.group(2))
    return out
