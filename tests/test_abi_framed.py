"""The framed-message encoders' entry points (capnp_packed_encode_framed, _framed_batch,
_framed_dense_batch, _framed_workspace_bytes): exported, bound, declared in
the header and the Zig binding, and their argument checks, all of which answer before any
device work (no GPU needed)."""
import ctypes
import os
import re

import pytest

import capnp_packed as cp

NEW = ("capnp_packed_encode_framed", "capnp_packed_encode_framed_workspace_bytes",
       "capnp_packed_encode_framed_batch", "capnp_packed_encode_framed_dense_batch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch(n=0, d_in=0, in_off=0, in_len=0, d_out=0, out_off=0, out_cap=0, out_len=0, status=0, dialect=0, ws=0,
          ws_bytes=0):
    return cp.lib().capnp_packed_encode_framed_batch(d_in, in_off, in_len, n, d_out, out_off, out_cap, out_len,
                                                     status, dialect, ws, ws_bytes, 0)


def dense(n=0, d_in=0, in_off=0, in_len=0, d_out=0, base=0, cap=0, out_off=0, out_len=0, status=0, dialect=0,
          ws=0, ws_bytes=0):
    return cp.lib().capnp_packed_encode_framed_dense_batch(d_in, in_off, in_len, n, d_out, base, cap, out_off,
                                                           out_len, status, dialect, ws, ws_bytes, 0)


def host(data=b"", dialect=0):
    out = ctypes.create_string_buffer(64)
    n = ctypes.c_size_t(77)
    st = cp.lib().capnp_packed_encode_framed(ctypes.create_string_buffer(data, max(1, len(data))), len(data), out,
                                             64, ctypes.byref(n), dialect)
    return st, n.value


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
    assert "pub fn packMessage(" in z
    assert re.search(r"2, additions only: capnp_packed_encode_framed\b", h)


def test_signatures_mirror_the_unframed_calls():
    S = cp.SIGNATURES
    assert S["capnp_packed_encode_framed"] == S["capnp_packed_encode_dialect"]
    assert S["capnp_packed_encode_framed_batch"] == S["capnp_packed_encode_batch_dialect"]
    assert S["capnp_packed_encode_framed_dense_batch"] == S["capnp_packed_encode_dense_batch"]
    assert S["capnp_packed_encode_framed_workspace_bytes"] == S["capnp_packed_encode_dense_workspace_bytes"]


def test_abi_version_is_still_2_and_statuses_still_23():
    assert cp.lib().capnp_packed_abi_version() == 2
    with open(cp.HEADER_PATH) as f:
        h = f.read()
    assert re.search(r"#define CAPNP_PACKED_ABI_VERSION 2u", h)
    names = [cp.lib().capnp_packed_status_name(s).decode() for s in range(64)]
    assert sum(1 for x in names if x != "Unknown") == 23
    assert names[23] == "Unknown"
    assert cp.DIALECTS == {"zig": 0, "cxx": 1}


def test_unknown_dialect_is_invalid_argument():
    for call in (batch, dense):
        assert call(dialect=7) == cp.INVALID_ARGUMENT
        assert call(dialect=2, n=1) == cp.INVALID_ARGUMENT
    assert host(bytes(8), dialect=2) == (cp.INVALID_ARGUMENT, 77)  # before out_len is touched
    assert host(bytes(8), dialect=7)[0] == cp.INVALID_ARGUMENT


def test_empty_batch_with_null_arrays_is_ok():
    for d in (0, 1):
        assert batch(n=0, dialect=d) == cp.OK
        assert dense(n=0, dialect=d) == cp.OK


# host addresses stand in for the device arrays: the checks must answer before anything is read
def _arrays():
    buf = ctypes.create_string_buffer(65536 + 512)
    a = (ctypes.addressof(buf) + 255) & ~255  # 256-B aligned
    return buf, a


def test_workspace_checks():
    buf, a = _arrays()
    L = cp.lib()
    for call, need, extra in (
            (batch, L.capnp_packed_encode_framed_workspace_bytes(100), dict(out_cap=a + 32768)),
            (dense, L.capnp_packed_encode_dense_workspace_bytes(100), {})):
        assert need > 0  # (the checks answer from the pointer and the size alone: nothing is read)
        arrays = dict(n=100, in_off=a + 32768, in_len=a + 32768, d_out=a + 32768, out_off=a + 32768,
                      out_len=a + 32768, status=a + 32768, **extra)
        for d in (0, 1):
            assert call(ws=0, ws_bytes=0, dialect=d, **arrays) == cp.INVALID_ARGUMENT          # NULL
            assert call(ws=a, ws_bytes=need - 1, dialect=d, **arrays) == cp.INVALID_ARGUMENT   # short
            assert call(ws=a, ws_bytes=0, dialect=d, **arrays) == cp.INVALID_ARGUMENT
            assert call(ws=a + 8, ws_bytes=need, dialect=d, **arrays) == cp.INVALID_ARGUMENT   # not 256-aligned
            assert "256" in cp.last_error()
    del buf


@pytest.mark.parametrize("missing", ["in_off", "in_len", "out_len", "status", "out_off", "out_cap"])
def test_batch_null_arrays_are_invalid_argument(missing):
    buf, a = _arrays()
    need = cp.lib().capnp_packed_encode_framed_workspace_bytes(4)
    arrays = dict(n=4, in_off=a + 32768, in_len=a + 32768, d_out=a + 32768, out_off=a + 32768, out_cap=a + 32768,
                  out_len=a + 32768, status=a + 32768, ws=a, ws_bytes=need)
    arrays[missing] = 0
    for d in (0, 1):
        assert batch(dialect=d, **arrays) == cp.INVALID_ARGUMENT
    del buf


@pytest.mark.parametrize("missing", ["in_off", "in_len", "out_off", "out_len", "status"])
def test_dense_null_arrays_are_invalid_argument(missing):
    buf, a = _arrays()
    need = cp.lib().capnp_packed_encode_dense_workspace_bytes(4)
    arrays = dict(n=4, in_off=a + 32768, in_len=a + 32768, out_off=a + 32768, out_len=a + 32768, status=a + 32768,
                  ws=a, ws_bytes=need)
    arrays[missing] = 0
    for d in (0, 1):
        assert dense(dialect=d, **arrays) == cp.INVALID_ARGUMENT
    del buf


def test_host_call_argument_checks():
    L = cp.lib()
    n = ctypes.c_size_t()
    buf = ctypes.create_string_buffer(64)
    assert L.capnp_packed_encode_framed(buf, 8, buf, 64, None, 1) == cp.INVALID_ARGUMENT       # out_len NULL
    assert L.capnp_packed_encode_framed(None, 8, buf, 64, ctypes.byref(n), 1) == cp.INVALID_ARGUMENT
    assert L.capnp_packed_encode_framed(buf, 8, None, 64, ctypes.byref(n), 0) == cp.INVALID_ARGUMENT
    # len % 8 answers before any device work in both dialects
    assert host(bytes(12), 0) == (cp.INVALID_MESSAGE_SIZE, 0)
    assert host(bytes(12), 1) == (cp.INVALID_MESSAGE_SIZE, 0)


def test_workspace_bytes_is_aligned_and_holds_the_batch_workspace():
    L = cp.lib()
    ns = list(range(0, 70)) + [255, 256, 257, 1000, 4096, 4097, 1 << 16, 1 << 20, (1 << 20) + 1, 1 << 28]
    sizes = [L.capnp_packed_encode_framed_workspace_bytes(n) for n in ns]
    assert all(s % 256 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    for n, s in zip(ns, sizes):  # launch_encode's own workspace, the lengths and the verdicts
        assert s >= L.capnp_packed_batch_workspace_bytes(n) + 12 * n


def test_python_rejects_other_dialects():
    for bad in ("c++", "", None, 1):
        with pytest.raises(cp.InvalidArgument):
            cp.encode_framed_batch(None, None, None, None, None, None, None, None, dialect=bad)
        with pytest.raises(cp.InvalidArgument):
            cp.encode_framed_dense_batch(None, None, None, None, None, None, None, dialect=bad)
        with pytest.raises(cp.InvalidArgument):
            cp.pack_message(bytes(8), dialect=bad)
        with pytest.raises(cp.InvalidArgument):
            cp.write_packed_messages([bytes(8)], dialect=bad)
