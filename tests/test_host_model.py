"""csrc/gpd_host_model.h, the HIP-free host model of libgpd.so, builds with a plain C++ compiler and
runs clean under AddressSanitizer + UBSan (tests/host_model_driver.cpp: pose_tables, the gimbal branch
of pose_template, the truncation counter against brute force, check_env_rows' refusal).

A stand-alone program, as oracle/asan_driver.c is for the C oracle: nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_model_under_asan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "host_model_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "host_model_driver.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "OK" in r.stdout and "FAIL" not in out and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
