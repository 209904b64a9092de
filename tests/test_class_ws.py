"""The class workspace layout (capnp-zig_amd/csrc/class_ws.h) on the CPU:
tests/host/class_ws_test.cpp includes only that header and checks every region offset against
the formulas written out again, the regions' order, overlap and alignment, long_list_slot's walk
and the recorded totals. Built here with the host compiler and run once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_against_recorded_formulas(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "class_ws_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "capnp-zig_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "class_ws_test.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("class_ws ok"), run.stdout
