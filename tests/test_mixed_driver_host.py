"""The reliable-update driver's decisions (csrc/sm_cg_host.h), run as a
stand-alone program under the host sanitizers with scripted operations:
tools/mixed_driver_check.cpp, built with the line its header states (no GPU)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_mixed_driver_check(tmp_path):
    exe = str(tmp_path / "mixed_driver_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{os.path.join(REPO, 'include')}", os.path.join(REPO, "tools", "mixed_driver_check.cpp"),
                    "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "mixed_driver_check ok"
