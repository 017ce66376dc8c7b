"""The 16-bit column ids of the team step's leading all-low turns (csrc/plan_host.cpp plan_team_ids16,
DESIGN.md 4.1 "Round 10"), checked on the CPU: the planner built without the HIP runtime under
AddressSanitizer + UndefinedBehaviorSanitizer together with its stand-alone checker
(tests/c/ids16_check.cpp), which decodes the 16-bit array the way the kernel does, compares it slot for
slot with the 32-bit ids and every wave's count of converted turns with a brute-force count: random
graphs, every id low, every id high, the first high id in each of the eight slots of a turn, the columns
65534 (low) and 65535 (high: the pad value stands for no column), odd and even chunk counts, 1, 10 and 16
lanes per row."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_ids16_planner_under_asan_ubsan(tmp_path):
    csrc = os.path.join(REPO, "efficient-gnn_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "ids16_check_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I",
                    os.path.join(rocm, "include"), "-I", os.path.join(REPO, "include"), "-I", csrc,
                    os.path.join(REPO, "tests", "c", "ids16_check.cpp"), os.path.join(csrc, "plan_host.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert out.stdout.startswith("ok")
