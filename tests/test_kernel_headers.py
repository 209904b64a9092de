"""Every kernel header (capnp-zig_amd/csrc/kernels/*.h) compiles on its own: it includes what it
uses, so the dependencies each header names in its opening comment are the ones the compiler
sees. Runs the Makefile's check-headers command (hipcc -fsyntax-only for gfx950, no GPU needed)
on one header per case.

The order contract, from the text alone: packed_kernels.hip includes every header of that
directory directly, exactly once, so the order of functions in the object is read from that one
file and no header enters the translation unit only through another header."""
import collections
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "capnp-zig_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEADERS = sorted(os.path.basename(h) for h in glob.glob(os.path.join(PKG, "csrc", "kernels", "*.h")))


def test_headers_found():
    assert HEADERS, "no header under capnp-zig_amd/csrc/kernels/"


def test_kernel_file_includes_every_header_once():
    with open(os.path.join(PKG, "csrc", "packed_kernels.hip")) as f:
        included = collections.Counter(re.findall(r'^\s*#\s*include\s+"kernels/([^"/]+\.h)"', f.read(), re.M))
    assert set(included) == set(HEADERS), sorted(set(included) ^ set(HEADERS))
    assert all(n == 1 for n in included.values()), {h: n for h, n in included.items() if n != 1}


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header):
    if shutil.which(HIPCC) is None:
        pytest.skip("no hipcc on this machine")
    run = subprocess.run(["make", "-s", "-C", PKG, "check-headers", "HIPCC=" + HIPCC,
                          "KHDRS=csrc/kernels/" + header], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
