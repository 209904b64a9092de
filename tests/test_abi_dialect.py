"""The dialect entry points of the C-ABI: exported, bound, and their argument checks, all of
which answer before any device work (no GPU needed)."""
import ctypes
import os
import re

import capnp_packed as cp

NEW = ("capnp_packed_encode_dialect", "capnp_packed_encode_batch_dialect",
       "capnp_packed_encode_message_batch_dialect")


def test_symbols_exported_and_bound():
    L = cp.lib()
    for name in NEW:
        assert name in cp.SIGNATURES
        assert hasattr(L, name)


def test_header_constants():
    with open(cp.HEADER_PATH) as f:
        h = f.read()
    assert re.search(r"#define\s+CAPNP_PACKED_DIALECT_ZIG\s+0u", h)
    assert re.search(r"#define\s+CAPNP_PACKED_DIALECT_CXX\s+1u", h)
    assert cp.DIALECTS == {"zig": 0, "cxx": 1}
    assert cp.lib().capnp_packed_abi_version() == 2


def _encode(src, n, dialect, cap=64):
    out = ctypes.create_string_buffer(cap)
    ln = ctypes.c_size_t(123)
    st = cp.lib().capnp_packed_encode_dialect(src, n, out, cap, ctypes.byref(ln), dialect)
    return st, ln.value


def test_null_input_is_invalid_argument():
    for d in (0, 1):
        assert _encode(None, 8, d) == (cp.INVALID_ARGUMENT, 0)


def test_unknown_dialect_is_invalid_argument():
    src = ctypes.create_string_buffer(8)
    st, _ = _encode(src, 8, 7)
    assert st == cp.INVALID_ARGUMENT
    L = cp.lib()
    assert L.capnp_packed_encode_batch_dialect(0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 0, 0, 0) == cp.INVALID_ARGUMENT
    assert L.capnp_packed_encode_message_batch_dialect(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 0) == cp.INVALID_ARGUMENT


def test_seven_bytes_is_invalid_message_size():
    src = ctypes.create_string_buffer(8)
    for d in (0, 1):
        assert _encode(src, 7, d) == (cp.INVALID_MESSAGE_SIZE, 0)


def test_empty_batches_are_ok():
    L = cp.lib()
    for d in (0, 1):
        assert L.capnp_packed_encode_batch_dialect(0, 0, 0, 0, 0, 0, 0, 0, 0, d, 0, 0, 0) == cp.OK
        assert L.capnp_packed_encode_message_batch_dialect(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, d, 0) == cp.OK


def test_python_rejects_other_dialects():
    import pytest
    for bad in ("c++", "", None, 1):
        with pytest.raises(cp.InvalidArgument):
            cp.pack_packed(bytes(8), dialect=bad)
        with pytest.raises(cp.InvalidArgument):
            cp.MessageBuilder().to_packed_bytes(dialect=bad)


def test_zig_wrapper_declares_the_calls():
    zig = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zig", "packed_ffi.zig")
    with open(zig) as f:
        z = f.read()
    for name in NEW:
        assert re.search(r'extern "capnp_packed" fn ' + name + r"\(", z)
    assert "pub const dialect_cxx: u32 = 1;" in z and "pub fn packPackedCxx(" in z
