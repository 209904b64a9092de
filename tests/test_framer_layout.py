"""The framer session's region planner (capnp-zig_amd/csrc/framer_layout.h) on
the CPU: tests/host/framer_layout_test.cpp includes only that header, keeps a byte-array model of
the arena and the staging buffer, applies every plan's copy jobs launch by launch and checks the
model after every read (bytes held = bytes fed minus bytes popped, regions disjoint and inside
the arena, m0 <= len <= cap, moved_bytes, no copy overlapping another of its launch). Built here
with the host compiler and run once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_against_byte_model(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "framer_layout_test")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "capnp-zig_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "framer_layout_test.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("framer_layout ok"), run.stdout
