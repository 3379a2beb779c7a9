"""The index math of dgrad_s2 (csrc/dgrad_s2_geom.h), exhausted on the CPU:
tests/dgrad_s2_geom_check.cpp is compiled with the host compiler under
AddressSanitizer + UBSan and run as its own program -- the fence against an
out-of-bounds halo read before the kernel runs on a card.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "semanticsegmentation_tensorflow_amd", "csrc")


def test_geometry_exhaustive_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is required"
    exe = str(tmp_path / "dgrad_s2_geom_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "dgrad_s2_geom_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().startswith("ok:"), r.stdout
