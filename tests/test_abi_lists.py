"""capnp_packed_list_heads_batch and capnp_packed_read_elements_batch at the C-ABI (DESIGN.md
§2.14): exported, bound, declared in the header and the Zig binding, the 32-byte head record,
and their host-side argument checks, all of which answer before any device work (no GPU needed)."""
import ctypes
import os
import re

import pytest

import capnp_packed as cp

NEW = ("capnp_packed_list_heads_batch", "capnp_packed_read_elements_batch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# host addresses stand in for the device arrays: the checks must answer before anything is read
@pytest.fixture()
def a():
    buf = ctypes.create_string_buffer(4096)
    yield ctypes.addressof(buf)
    del buf


def heads(n=4, path=(), path_len=None, null_path=False, pointer_index=0, kind=cp.LIST_STRUCT, d_in=0, in_off=0,
          in_len=0, head=0, count=0, status=0):
    arr = (ctypes.c_uint32 * max(1, len(path)))(*path)
    return cp.lib().capnp_packed_list_heads_batch(d_in, in_off, in_len, n, None if null_path else arr,
                                                  len(path) if path_len is None else path_len, pointer_index, kind,
                                                  head, count, status, 0)


def elements(fields, n=4, kind=cp.LIST_STRUCT, elem_cap=16, n_fields=None, null_fields=False, d_in=0, in_off=0,
             in_len=0, head=0, start=0, parent=0, index=0, value=0, length=0, count=0, status=0):
    arr = (cp.CField * max(1, len(fields)))(*[f.c() for f in fields])
    return cp.lib().capnp_packed_read_elements_batch(d_in, in_off, in_len, n, head, start, kind, elem_cap,
                                                     None if null_fields else arr,
                                                     len(fields) if n_fields is None else n_fields, parent, index,
                                                     value, length, count, status, 0)


def head_args(a):
    return dict(d_in=a, in_off=a, in_len=a, head=a, count=a, status=a)


def elem_args(a):
    return dict(d_in=a, in_off=a, in_len=a, head=a, start=a, parent=a, index=a, value=a, length=a, count=a, status=a)


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
    assert re.search(r"2, additions only: capnp_packed_list_heads_batch, capnp_packed_read_elements_batch\b", h)
    assert "pub const ListHead = extern struct" in z
    assert re.search(r"#define CAPNP_PACKED_LIST_STRUCT 0u", h) and cp.LIST_STRUCT == 0
    assert re.search(r"#define CAPNP_PACKED_LIST_POINTER 1u", h) and cp.LIST_POINTER == 1
    assert re.search(r"pub const list_struct: u32 = 0;", z) and re.search(r"pub const list_pointer: u32 = 1;", z)


def test_abi_version_is_still_2_and_statuses_still_23():
    assert cp.lib().capnp_packed_abi_version() == 2
    names = [cp.lib().capnp_packed_status_name(s).decode() for s in range(64)]
    assert sum(1 for x in names if x != "Unknown") == 23


def test_head_is_32_bytes_and_matches_the_header_and_the_zig_binding():
    assert ctypes.sizeof(cp.CListHead) == 32 and cp.LIST_HEAD_BYTES == 32 and cp.LIST_HEAD_DTYPE.itemsize == 32
    order = ["elems_off", "count", "segment", "seg_begin", "seg_bytes", "data_words", "pointer_words", "status"]
    assert [n for n, _ in cp.CListHead._fields_] == order
    assert list(cp.LIST_HEAD_DTYPE.names) == order
    assert [cp.LIST_HEAD_DTYPE.fields[n][1] for n in order] == [getattr(cp.CListHead, n).offset for n in order]
    with open(cp.HEADER_PATH) as f:
        h = f.read()
    body = re.search(r"typedef struct capnp_packed_list_head \{(.*?)\} capnp_packed_list_head;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            declared += [x.strip() for x in decl.split(None, 1)[1].split(",")]
    assert declared == order
    with open(os.path.join(ROOT, "zig", "packed_ffi.zig")) as f:
        z = f.read()
    zbody = re.search(r"pub const ListHead = extern struct \{(.*?)\};", z, re.S).group(1)
    assert re.findall(r"(\w+): [ui]\d+", zbody) == order


def test_empty_batches_are_ok_with_null_arrays():
    assert heads(n=0) == cp.OK
    assert heads(n=0, null_path=True, kind=cp.LIST_POINTER) == cp.OK
    assert elements([cp.Field(cp.FIELD_U8, 0)], n=0) == cp.OK
    assert elements([cp.Field(cp.FIELD_U8, 0)], n=4, elem_cap=0) == cp.OK
    assert elements([], n=0, null_fields=True) == cp.OK
    assert elements([], n=4) == cp.OK  # no fields and no numbering asked for: nothing to do


@pytest.mark.parametrize("kind", [2, 7, 0xFFFFFFFF])
def test_unknown_list_kind(a, kind):
    assert heads(kind=kind, **head_args(a)) == cp.INVALID_ARGUMENT
    assert heads(kind=kind, n=0) == cp.INVALID_ARGUMENT
    assert elements([cp.Field(cp.FIELD_U8, 0, path=(0,))], kind=kind, **elem_args(a)) == cp.INVALID_ARGUMENT
    assert cp.last_error()


def test_heads_path_longer_than_4(a):
    assert heads(path=(0, 0, 0, 0, 0), **head_args(a)) == cp.INVALID_ARGUMENT
    assert heads(path=(0,), path_len=0xFFFFFFFF, **head_args(a)) == cp.INVALID_ARGUMENT


@pytest.mark.parametrize("missing", ["d_in", "in_off", "in_len", "head", "count", "status", "path"])
def test_heads_null_arrays_are_invalid_argument(a, missing):
    args = head_args(a)
    if missing == "path":
        assert heads(path=(1,), null_path=True, path_len=1, **args) == cp.INVALID_ARGUMENT
    else:
        args[missing] = 0
        assert heads(**args) == cp.INVALID_ARGUMENT


def test_elem_cap_of_2_to_the_32_or_more(a):
    f = [cp.Field(cp.FIELD_U8, 0)]
    assert elements(f, elem_cap=1 << 32, **elem_args(a)) == cp.INVALID_ARGUMENT
    assert elements(f, elem_cap=(1 << 64) - 1, **elem_args(a)) == cp.INVALID_ARGUMENT


def test_more_than_32_fields(a):
    fields = [cp.Field(cp.FIELD_U8, 0)] * 33
    assert elements(fields, **elem_args(a)) == cp.INVALID_ARGUMENT
    assert elements(fields[:1], n_fields=0xFFFFFFFF, **elem_args(a)) == cp.INVALID_ARGUMENT


@pytest.mark.parametrize("field", [
    cp.Field(11, 0), cp.Field(0xFFFFFFFF, 0), cp.Field(cp.FIELD_BOOL, 0, bit=8), cp.Field(cp.FIELD_U8, 0, bit=1),
    cp.Field(cp.FIELD_TEXT, 0, bit=7), cp.Field(cp.FIELD_U32, 0, path=(0, 0, 0, 0, 0)),
], ids=repr)
@pytest.mark.parametrize("kind", [cp.LIST_STRUCT, cp.LIST_POINTER])
def test_bad_descriptors(a, field, kind):
    good = cp.Field(cp.FIELD_TEXT, 0)
    for fields in ([field], [good, field], [good] * 31 + [field]):
        assert elements(fields, kind=kind, **elem_args(a)) == cp.INVALID_ARGUMENT


@pytest.mark.parametrize("field", [
    cp.Field(cp.FIELD_U8, 0), cp.Field(cp.FIELD_U64, 0), cp.Field(cp.FIELD_BOOL, 0, bit=3),  # a data kind, no path
    cp.Field(cp.FIELD_TEXT, 1), cp.Field(cp.FIELD_LIST_64, 0xFFFFFFFF),                      # offset != 0, no path
    cp.Field(cp.FIELD_TEXT, 0, path=(1,)), cp.Field(cp.FIELD_U32, 0, path=(2, 0)),           # path[0] != 0
], ids=repr)
def test_pointer_list_descriptors(a, field):
    good = cp.Field(cp.FIELD_TEXT, 0)
    for fields in ([field], [good, field]):
        assert elements(fields, kind=cp.LIST_POINTER, **elem_args(a)) == cp.INVALID_ARGUMENT
    import torch
    if not torch.cuda.is_available():  # the same descriptor is fine on a struct list
        assert elements([field], kind=cp.LIST_STRUCT, **elem_args(a)) == cp.NO_DEVICE


@pytest.mark.parametrize("missing", ["d_in", "in_off", "in_len", "head", "start", "value", "length", "status", "fields"])
def test_elements_null_arrays_are_invalid_argument(a, missing):
    fields = [cp.Field(cp.FIELD_U8, 0)]
    args = elem_args(a)
    if missing == "fields":
        assert elements(fields, null_fields=True, n_fields=1, **args) == cp.INVALID_ARGUMENT
    else:
        args[missing] = 0
        assert elements(fields, **args) == cp.INVALID_ARGUMENT


def test_optional_arrays_and_the_numbering_only_call(a):
    """d_parent, d_index and d_count may be NULL; no fields with d_parent or d_index is the element
    numbering alone and needs the start array only. Past the argument checks the call goes on to
    the device (and without one reports that, not INVALID_ARGUMENT)."""
    import torch
    if torch.cuda.is_available():
        # with a device: one message of no bytes (END_OF_STREAM, no element), through the wrappers
        z = torch.zeros(2, dtype=torch.int64, device="cuda")
        head = torch.zeros(32, dtype=torch.uint8, device="cuda")
        st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        out = torch.full((4,), -7, dtype=torch.int64, device="cuda")
        num = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        cp.list_heads_batch(z.view(torch.uint8), z[:1], z[:1], cp.LIST_POINTER, 0, head, z[1:], st)
        cp.read_elements_batch(z.view(torch.uint8), z[:1], z[:1], head, z, cp.LIST_POINTER, 4,
                               [cp.Field(cp.FIELD_TEXT, 0)], out, out, num)
        cp.read_elements_batch(None, z[:1], z[:1], None, z, cp.LIST_POINTER, 4, [], None, None, None, parent=num)
        cp.read_elements_batch(None, z[:1], z[:1], None, z, cp.LIST_POINTER, 4, [], None, None, None, index=num)
        assert st.cpu().tolist() == [cp.END_OF_STREAM] and not head[:28].cpu().numpy().any()
        assert out.cpu().tolist() == [-7] * 4 and num.cpu().tolist() == [-7] * 4
        assert elements([], parent=a, index=a) == cp.INVALID_ARGUMENT  # no start array
        return
    args = elem_args(a)
    args.update(parent=0, index=0, count=0)
    assert elements([cp.Field(cp.FIELD_U8, 0)], **args) == cp.NO_DEVICE
    assert elements([], start=a, parent=a) == cp.NO_DEVICE
    assert elements([], start=a, index=a) == cp.NO_DEVICE
    assert elements([], parent=a, index=a) == cp.INVALID_ARGUMENT  # no start array
    assert heads(path=(), null_path=True, **head_args(a)) == cp.NO_DEVICE


def test_python_wrappers_check_output_sizes():
    import torch
    off = torch.zeros(4, dtype=torch.int64)
    out = torch.zeros(15, dtype=torch.int64)
    st = torch.zeros(16, dtype=torch.int32)
    head = torch.zeros(4 * 32, dtype=torch.uint8)
    start = torch.zeros(5, dtype=torch.int64)
    f = [cp.Field(cp.FIELD_U8, 0)] * 2
    with pytest.raises(cp.InvalidArgument):  # 2 fields x 8 elements need 16 entries
        cp.read_elements_batch(None, off, off, head, start, cp.LIST_STRUCT, 8, f, out, out, st)
    with pytest.raises(cp.InvalidArgument):
        cp.read_elements_batch(None, off, off, head[:-1], start, cp.LIST_STRUCT, 4, f, out, out, st)
    with pytest.raises(cp.InvalidArgument):
        cp.read_elements_batch(None, off, off, head, start[:4], cp.LIST_STRUCT, 4, f, out, out, st)
    with pytest.raises(cp.InvalidArgument):
        cp.read_elements_batch(None, off, off, head, start, cp.LIST_STRUCT, 4, f, out, out, st,
                               parent=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(cp.InvalidArgument):
        cp.list_heads_batch(None, off, off, cp.LIST_STRUCT, 0, head[:100], off, st)
    with pytest.raises(cp.InvalidArgument):
        cp.list_heads_batch(None, off, off, cp.LIST_STRUCT, 0, head, off[:3], st)
