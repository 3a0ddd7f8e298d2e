"""CPU suite: the layout arithmetic behind the host-array entry points (oflibnumpy_amd/csrc/ofl_stage_layout.h, the header
ofl_host_stage.h builds on), compiled for the host as a stand-alone program under AddressSanitizer and UBSan and run over the
part lists of the eight entries: every subset of optional parts absent, pixel counts that leave every element size off the
16-byte grid, zero-byte parts."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_layout_rules_hold_for_every_entry(tmp_path):
    exe = tmp_path / "host_stage_cpu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "host_stage_cpu.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().endswith("layouts ok"), run.stdout
