"""CPU suite: where the parts of the exact path's workspace lie (oflibnumpy_amd/csrc/ofl_delaunay_ws.h: carve_exact),
compiled for the host as a stand-alone program under AddressSanitizer and UBSan and run over shapes from 1 x 1 to 4320 x 7680:
every part on a 256-byte boundary, parts disjoint and in declaration order, the last one -- the owner map, H * W words --
ending at the reported total, and that total equal to what ofl_scatter_workspace_bytes promised before the layout became a
table."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_layout_rules_hold_and_totals_are_the_recorded_ones(tmp_path):
    exe = tmp_path / "dl_layout_cpu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "dl_layout_cpu.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().endswith("layouts ok"), run.stdout
