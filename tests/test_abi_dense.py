"""The dense batch encode's entry points (capnp_packed_encode_dense_batch, the batch form of
writePackedTo): exported, bound, declared in the Zig binding, and their argument checks, all
of which answer before any device work (no GPU needed)."""
import ctypes
import os
import re

import pytest

import capnp_packed as cp

NEW = ("capnp_packed_encode_dense_workspace_bytes", "capnp_packed_encode_dense_batch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dense(n=0, d_in=0, in_off=0, in_len=0, d_out=0, base=0, cap=0, out_off=0, out_len=0, status=0, dialect=0,
          ws=0, ws_bytes=0):
    return cp.lib().capnp_packed_encode_dense_batch(d_in, in_off, in_len, n, d_out, base, cap, out_off, out_len,
                                                    status, dialect, ws, ws_bytes, 0)


def test_symbols_exported_bound_and_declared():
    L = cp.lib()
    with open(cp.HEADER_PATH) as f:
        h = f.read()
    with open(os.path.join(ROOT, "zig", "packed_ffi.zig")) as f:
        z = f.read()
    for name in NEW:
        assert name in cp.SIGNATURES
        assert hasattr(L, name)
        assert re.search(r"\b" + name + r"\(", h)
        assert re.search(r'extern "capnp_packed" fn ' + name + r"\(", z)


def test_abi_version_is_still_2():
    assert hasattr(cp.lib(), NEW[1])
    assert cp.lib().capnp_packed_abi_version() == 2


def test_unknown_dialect_is_invalid_argument():
    assert dense(dialect=7) == cp.INVALID_ARGUMENT
    assert dense(dialect=2, n=1) == cp.INVALID_ARGUMENT


def test_empty_batch_with_null_arrays_is_ok():
    for d in (0, 1):
        assert dense(n=0, dialect=d) == cp.OK


# host addresses stand in for the device arrays: the checks must answer before anything is read
def _arrays():
    buf = ctypes.create_string_buffer(4096 + 512)
    a = (ctypes.addressof(buf) + 255) & ~255  # 256-B aligned
    return buf, a


def test_workspace_checks():
    buf, a = _arrays()
    need = cp.lib().capnp_packed_encode_dense_workspace_bytes(100)
    assert 0 < need <= 2048
    arrays = dict(n=100, in_off=a + 2048, in_len=a + 2048, out_off=a + 2048, out_len=a + 2048, status=a + 2048)
    assert dense(ws=0, ws_bytes=0, **arrays) == cp.INVALID_ARGUMENT          # NULL
    assert dense(ws=a, ws_bytes=need - 1, **arrays) == cp.INVALID_ARGUMENT   # short
    assert dense(ws=a, ws_bytes=0, **arrays) == cp.INVALID_ARGUMENT
    assert dense(ws=a + 8, ws_bytes=need, **arrays) == cp.INVALID_ARGUMENT   # 8- but not 256-aligned
    assert "256" in cp.last_error()
    del buf


@pytest.mark.parametrize("missing", ["out_off", "out_len", "status"])
def test_null_result_arrays_are_invalid_argument(missing):
    buf, a = _arrays()
    need = cp.lib().capnp_packed_encode_dense_workspace_bytes(4)
    arrays = dict(n=4, in_off=a + 2048, in_len=a + 2048, out_off=a + 2048, out_len=a + 2048, status=a + 2048,
                  ws=a, ws_bytes=need)
    arrays[missing] = 0
    assert dense(**arrays) == cp.INVALID_ARGUMENT
    del buf


def test_workspace_bytes_grows_with_n_in_16_byte_steps():
    L = cp.lib()
    ns = list(range(0, 70)) + [255, 256, 257, 1000, 4095, 4096, 4097, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 28,
                               (1 << 32) - 1]
    sizes = [L.capnp_packed_encode_dense_workspace_bytes(n) for n in ns]
    assert all(s % 16 == 0 and s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] > sizes[0]


def test_python_rejects_other_dialects():
    for bad in ("c++", "", None, 1):
        with pytest.raises(cp.InvalidArgument):
            cp.encode_dense_batch(None, None, None, None, None, None, None, dialect=bad)
