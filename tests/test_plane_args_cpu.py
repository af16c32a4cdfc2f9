"""groundgrid_amd/csrc/plane_args.h, the argument frame of the plane calls, alone: tests/cpp/test_plane_args.cpp built for the host with
AddressSanitizer + UndefinedBehaviourSanitizer (a program of its own: nothing is preloaded) and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")


@pytest.mark.skipif(not GXX, reason="no g++")
def test_plane_args_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "test_plane_args")
    subprocess.check_call([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "groundgrid_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_plane_args.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert "plane args OK" in p.stdout
