"""capnp_packed_read_fields_batch and capnp_packed_gather_batch at the C-ABI:
exported, bound, declared in the header and the Zig binding, and their host-side argument
checks, all of which answer before any device work (no GPU needed)."""
import ctypes
import os
import re

import pytest

import capnp_packed as cp

NEW = ("capnp_packed_read_fields_batch", "capnp_packed_gather_batch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# host addresses stand in for the device arrays: the checks must answer before anything is read
@pytest.fixture()
def arrays():
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    yield dict(d_in=a, in_off=a, in_len=a, value=a, length=a, count=a, status=a)
    del buf


def read_fields(fields, n=4, n_fields=None, null_fields=False, d_in=0, in_off=0, in_len=0, value=0, length=0,
                count=0, status=0):
    arr = (cp.CField * max(1, len(fields)))(*[f.c() for f in fields])
    return cp.lib().capnp_packed_read_fields_batch(d_in, in_off, in_len, n, None if null_fields else arr,
                                                   len(fields) if n_fields is None else n_fields, value, length,
                                                   count, status, 0)


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
    assert re.search(r"2, additions only: capnp_packed_read_fields_batch, capnp_packed_gather_batch\b", h)
    assert "pub const Field = extern struct" in z


def test_abi_version_is_still_2_and_statuses_still_23():
    assert cp.lib().capnp_packed_abi_version() == 2
    names = [cp.lib().capnp_packed_status_name(s).decode() for s in range(64)]
    assert sum(1 for x in names if x != "Unknown") == 23


def test_descriptor_is_32_bytes_and_matches_the_header():
    assert ctypes.sizeof(cp.CField) == 32
    assert [n for n, _ in cp.CField._fields_] == ["kind", "offset", "bit", "path_len", "path"]
    with open(cp.HEADER_PATH) as f:
        h = f.read()
    kinds = dict((k, int(v)) for k, v in re.findall(r"#define CAPNP_PACKED_FIELD_(\w+) (\d+)u", h))
    assert kinds == {"U8": cp.FIELD_U8, "U16": cp.FIELD_U16, "U32": cp.FIELD_U32, "U64": cp.FIELD_U64,
                     "BOOL": cp.FIELD_BOOL, "TEXT": cp.FIELD_TEXT, "DATA": cp.FIELD_DATA,
                     "LIST_BIT": cp.FIELD_LIST_BIT, "LIST_16": cp.FIELD_LIST_16, "LIST_32": cp.FIELD_LIST_32,
                     "LIST_64": cp.FIELD_LIST_64}
    assert sorted(kinds.values()) == list(range(11))
    assert re.search(r"#define CAPNP_PACKED_MAX_FIELDS 32u", h) and cp.MAX_FIELDS == 32
    assert re.search(r"#define CAPNP_PACKED_MAX_PATH 4u", h) and cp.MAX_PATH == 4
    with open(os.path.join(ROOT, "zig", "packed_ffi.zig")) as f:
        z = f.read()
    for k, v in kinds.items():
        assert re.search(rf"pub const field_{k.lower()}: u32 = {v};", z), k


def test_empty_batches_are_ok_with_null_arrays():
    assert read_fields([cp.Field(cp.FIELD_U8, 0)], n=0) == cp.OK
    assert read_fields([], n=4) == cp.OK
    assert read_fields([], n=0, null_fields=True) == cp.OK
    assert cp.lib().capnp_packed_gather_batch(0, 0, 0, 0, 0, 0, 0, 0, 0) == cp.OK


def test_more_than_32_fields(arrays):
    fields = [cp.Field(cp.FIELD_U8, 0)] * 33
    assert read_fields(fields, **arrays) == cp.INVALID_ARGUMENT
    assert read_fields(fields, n=0) == cp.INVALID_ARGUMENT
    assert read_fields(fields[:1], n_fields=0xFFFFFFFF, **arrays) == cp.INVALID_ARGUMENT


@pytest.mark.parametrize("field", [
    cp.Field(11, 0), cp.Field(0xFFFFFFFF, 0),                          # unknown kinds
    cp.Field(cp.FIELD_BOOL, 0, bit=8), cp.Field(cp.FIELD_BOOL, 0, bit=0xFFFFFFFF),
    cp.Field(cp.FIELD_U8, 0, bit=1), cp.Field(cp.FIELD_TEXT, 0, bit=7), cp.Field(cp.FIELD_LIST_64, 0, bit=1),
    cp.Field(cp.FIELD_U32, 0, path=(0, 0, 0, 0, 0)),                   # path_len 5
], ids=repr)
def test_bad_descriptors(arrays, field):
    good = cp.Field(cp.FIELD_U32, 4)
    for fields in ([field], [good, field], [good] * 31 + [field]):
        assert read_fields(fields, **arrays) == cp.INVALID_ARGUMENT
    assert cp.last_error()


def test_good_descriptors_pass_the_host_checks(arrays):
    """every kind, bit 0-7 on BOOL, paths of 0-4 steps, 32 fields: past the argument checks the
    call goes on to the device (and without one reports that, not INVALID_ARGUMENT)"""
    fields = [cp.Field(k, 3) for k in range(11)] + [cp.Field(cp.FIELD_BOOL, 0, bit=b) for b in range(8)]
    fields += [cp.Field(cp.FIELD_DATA, 1, path=(1,) * k) for k in range(5)]
    fields += [cp.Field(cp.FIELD_U64, 0xFFFFFFFF)] * (32 - len(fields))
    assert len(fields) == 32
    import torch
    if not torch.cuda.is_available():
        assert read_fields(fields, **arrays) == cp.NO_DEVICE
        return
    # with a device: one message of no bytes, which reads nothing (END_OF_STREAM for every field)
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.zeros(3 * 32, dtype=torch.int64, device="cuda")
    st = torch.full((32,), -1, dtype=torch.int32, device="cuda")
    cp.read_fields_batch(z.view(torch.uint8), z, z, fields, out[:32], out[32:64], st, out[64:])
    assert (st.cpu().numpy() == cp.END_OF_STREAM).all() and not out.cpu().numpy().any()


@pytest.mark.parametrize("missing", ["d_in", "in_off", "in_len", "value", "length", "status", "fields"])
def test_null_arrays_are_invalid_argument(arrays, missing):
    fields = [cp.Field(cp.FIELD_U8, 0)]
    if missing == "fields":
        assert read_fields(fields, null_fields=True, n_fields=1, **arrays) == cp.INVALID_ARGUMENT
    else:
        arrays[missing] = 0
        assert read_fields(fields, **arrays) == cp.INVALID_ARGUMENT


@pytest.mark.parametrize("missing", ["src_off", "src_len", "dst_off", "status", "d_in", "d_out"])
def test_gather_null_arrays_are_invalid_argument(arrays, missing):
    a = arrays["d_in"]
    args = dict(d_in=a, src_off=a, src_len=a, d_out=a, dst_off=a, status=a)
    args[missing] = 0
    assert cp.lib().capnp_packed_gather_batch(args["d_in"], args["src_off"], args["src_len"], 4, args["d_out"],
                                              args["dst_off"], 64, args["status"], 0) == cp.INVALID_ARGUMENT


def test_python_wrapper_checks_output_sizes():
    import torch
    off = torch.zeros(4, dtype=torch.int64)
    out = torch.zeros(7, dtype=torch.int64)
    with pytest.raises(cp.InvalidArgument):
        cp.read_fields_batch(None, off, off, [cp.Field(cp.FIELD_U8, 0)] * 2, out, out, torch.zeros(8, dtype=torch.int32))
