"""capnp_packed_build_fields_batch at the C-ABI: exported, bound, declared in
the header and the Zig binding, and its host-side argument checks, all of which answer before
any device work (no GPU needed). The model's check_ops (tests/build_streams.py) must agree with
the library on every program tried here. Host addresses stand in for device arrays ONLY in calls
that are refused before device work, or when no device is present; a program the call accepts
is run, where a device is present, on real device tensors (accepted()).

test_abi_fields.py already pins the ABI version at 2 and the statuses at 23."""
import ctypes
import os
import random
import re

import pytest

import build_streams as bs
import capnp_packed as cp
from build_streams import Op

NAME = "capnp_packed_build_fields_batch"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = bs.STRUCT


# host addresses stand in for the device arrays: the checks must answer before anything is read
@pytest.fixture()
def arrays():
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    yield dict(pool=a, value=a, length=a, count=a, out=a, out_off=a, out_cap=a, out_len=a, status=a)
    del buf


def c_ops(ops):
    arr = (cp.CBuildOp * max(1, len(ops)))()
    for i, o in enumerate(ops):
        arr[i] = cp.CBuildOp(o.kind, o.target, o.offset, o.bit, o.dw, o.pw, (ctypes.c_uint32 * 3)(*o.reserved))
    return arr


def build(ops, n=4, n_ops=None, null_ops=False, pool=0, pool_len=64, value=0, length=0, count=0, out=0, out_off=0,
          out_cap=0, out_len=0, status=0):
    arr = c_ops(ops)
    return cp.lib().capnp_packed_build_fields_batch(pool, pool_len, n, None if null_ops else arr,
                                                    len(ops) if n_ops is None else n_ops, value, length, count, out,
                                                    out_off, out_cap, out_len, status, 0)


def accepted(ops, arrays, count=True, outputs=True, pool=True):
    """True when the call takes `ops` past its argument checks. Without a device the call then
    answers NO_DEVICE, and host addresses stand in for the arrays (nothing is read). With a
    device it would launch, so the arrays are real device tensors: one message, every column
    entry 0 (an empty slice at pool offset 0, a zero value), built into a slot of its own."""
    import torch
    if not torch.cuda.is_available():
        a = dict(arrays)
        if not count:
            a["count"] = 0
        if not outputs:
            a.update(out=0, out_off=0, out_cap=0)
        if not pool:
            a["pool"] = 0
        return build(ops, pool_len=64 if pool else 0, **a) == cp.NO_DEVICE
    n_ops = len(ops)
    col = torch.zeros(n_ops, dtype=torch.int64, device="cuda")
    d_pool = torch.zeros(64, dtype=torch.uint8, device="cuda") if pool else None
    out_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    bops = [cp.BuildOp(o.kind, o.offset, o.bit, o.target, o.dw, o.pw) for o in ops]
    cap = 8 * (2 + bs.MAX_WORDS + n_ops)  # table, root pointer, the structs, a word per empty Text
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda") if outputs else None
    off = torch.zeros(1, dtype=torch.int64, device="cuda") if outputs else None
    caps = torch.full((1,), cap, dtype=torch.int64, device="cuda") if outputs else None
    try:
        cp.build_fields_batch(d_pool, bops, col, col, d_out, off, caps, out_len, st, count=col if count else None,
                              pool_len=64 if pool else 0)
    except cp.InvalidArgument:
        return False
    torch.cuda.synchronize()
    want = bs.build_message(ops, [(0, 0, 0)] * n_ops, bytes(64 if pool else 0), cap=cap, sizes_only=not outputs)
    assert (int(st.item()), int(out_len.item())) == want[:2]
    return True


def test_symbol_exported_bound_and_declared():
    with open(cp.HEADER_PATH) as f:
        h = f.read()
    with open(os.path.join(ROOT, "zig", "packed_ffi.zig")) as f:
        z = f.read()
    assert NAME in cp.SIGNATURES and hasattr(cp.lib(), NAME)
    assert re.search(r"\b" + NAME + r"\(", h)
    assert re.search(r'extern "capnp_packed" fn ' + NAME + r"\(", z)
    assert re.search(r"2, additions only: capnp_packed_build_fields_batch\b", h)
    assert "pub const BuildOp = extern struct" in z
    assert len(cp.SIGNATURES[NAME][1]) == 14


def test_op_is_32_bytes_and_constants_match_the_header():
    assert ctypes.sizeof(cp.CBuildOp) == 32
    assert [n for n, _ in cp.CBuildOp._fields_] == ["kind", "target", "offset", "bit", "data_words", "pointer_words",
                                                    "reserved"]
    with open(cp.HEADER_PATH) as f:
        h = f.read()
    assert re.search(r"#define CAPNP_PACKED_BUILD_STRUCT 16u", h) and cp.BUILD_STRUCT == 16 == bs.STRUCT
    assert re.search(r"#define CAPNP_PACKED_BUILD_ABSENT UINT64_MAX", h) and cp.BUILD_ABSENT == 2 ** 64 - 1 == bs.ABSENT
    assert re.search(r"#define CAPNP_PACKED_MAX_BUILD_OPS 32u", h) and cp.MAX_BUILD_OPS == 32 == bs.MAX_OPS
    assert re.search(r"#define CAPNP_PACKED_MAX_BUILD_WORDS 64u", h) and cp.MAX_BUILD_WORDS == 64 == bs.MAX_WORDS
    with open(os.path.join(ROOT, "zig", "packed_ffi.zig")) as f:
        z = f.read()
    assert "pub const build_struct: u32 = 16;" in z and "pub const max_build_ops: u32 = 32;" in z


def test_empty_batch_is_ok_with_null_arrays():
    assert build([Op(S, dw=1)], n=0) == cp.OK
    assert build([], n=0, null_ops=True) == cp.OK
    assert build([Op(bs.U8)], n=0) == cp.OK  # the ops are not looked at


def test_more_than_32_ops(arrays):
    ops = [Op(S, dw=1)] + [Op(bs.U8, 0)] * 32
    assert build(ops, **arrays) == cp.INVALID_ARGUMENT
    assert build(ops, n=0) == cp.INVALID_ARGUMENT
    assert build(ops[:2], n_ops=0xFFFFFFFF, **arrays) == cp.INVALID_ARGUMENT
    assert accepted(ops[:32], arrays)


REFUSED = {
    "no ops": [],
    "op 0 not a struct": [Op(bs.U8, 0)],
    "kind 11": [Op(S, dw=1), Op(11, 0)],
    "kind 15": [Op(S, dw=1), Op(15, 0)],
    "kind 17": [Op(S, dw=1), Op(17, 0)],
    "kind 2^32 - 1": [Op(S, dw=1), Op(0xFFFFFFFF, 0)],
    "bit 8": [Op(S, dw=1), Op(bs.BOOL, 0, bit=8)],
    "bit off BOOL": [Op(S, dw=1), Op(bs.U8, 0, bit=1)],
    "bit on a struct": [Op(S, dw=1, pw=1), Op(S, 0, bit=1, dw=1)],
    "bit on a slice": [Op(S, pw=1), Op(bs.TEXT, 0, bit=7)],
    "reserved[0]": [Op(S, dw=1), Op(bs.U8, 0, reserved=(1, 0, 0))],
    "reserved[2] of op 0": [Op(S, dw=1, reserved=(0, 0, 5))],
    "target is the op itself": [Op(S, dw=1), Op(bs.U8, 0, target=1)],
    "target later": [Op(S, dw=1, pw=1), Op(bs.U8, 0, target=2), Op(S, 0, dw=1)],
    "target not a struct": [Op(S, dw=1), Op(bs.U8, 0), Op(bs.U8, 0, target=1)],
    "pointer index": [Op(S, pw=1), Op(bs.TEXT, 1)],
    "pointer index of a struct": [Op(S, pw=1), Op(S, 1, dw=1)],
    "pointer index in an empty struct": [Op(S, pw=1), Op(S, 0), Op(bs.DATA, 0, target=1)],
    "slot twice": [Op(S, pw=1), Op(bs.TEXT, 0), Op(bs.DATA, 0)],
    "slot twice, a struct": [Op(S, pw=1), Op(bs.TEXT, 0), Op(S, 0, dw=1)],
    "64 struct words": [Op(S, dw=32, pw=1), Op(S, 0, dw=31)],
    "64 struct words at once": [Op(S, dw=60, pw=4)],
    "65535 words": [Op(S, dw=0xFFFF, pw=0xFFFF)],
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_programs(arrays, name):
    ops = REFUSED[name]
    assert not bs.check_ops(ops)
    assert build(ops, **arrays) == cp.INVALID_ARGUMENT
    assert cp.last_error()
    good = [Op(S, dw=1, pw=4), Op(bs.U32, 4)]
    if ops and ops[0].kind == S and len(ops) <= 3 and ops[0].dw + ops[0].pw < 40:  # the same fault later in a program
        moved = good + [Op(o.kind, o.offset, o.bit, o.target + 2 if k else 0, o.dw, o.pw, o.reserved)
                        for k, o in enumerate(ops)]
        moved[2].offset = 3  # what was op 0 is now initStruct(3) of the new root
        assert not bs.check_ops(moved)
        assert build(moved, **arrays) == cp.INVALID_ARGUMENT


def test_accepted_programs(arrays):
    """63 struct words, every kind, bit 0-7 on BOOL, 32 ops, data writes past the data section
    (dropped, not refused), and generated programs: the model and the library agree"""
    progs = [
        [Op(S, dw=32, pw=1), Op(S, 0, dw=30)],
        [Op(S, dw=59, pw=4)],
        [Op(S)],
        [Op(S, dw=1, pw=6)] + [Op(k, k - bs.TEXT) for k in bs.SLICES] + [Op(bs.BOOL, 0, bit=b) for b in range(8)],
        [Op(S, dw=1)] + [Op(bs.U64, 0xFFFFFFFF)] * 31,
        [Op(S, pw=1), Op(S, 0), Op(bs.U8, 0, target=1)],
    ]
    rng = random.Random(11)
    progs += [bs.gen_program(rng, n) for n in range(1, 33)]
    for ops in progs:
        assert bs.check_ops(ops), ops
        assert accepted(ops, arrays), (ops, cp.last_error())


@pytest.mark.parametrize("missing", ["pool", "value", "length", "out_len", "status", "out_off", "out_cap", "ops"])
def test_null_arrays_are_invalid_argument(arrays, missing):
    ops = [Op(S, dw=1, pw=1), Op(bs.TEXT, 0)]
    if missing == "ops":
        assert build(ops, null_ops=True, **arrays) == cp.INVALID_ARGUMENT
    else:
        arrays[missing] = 0
        assert build(ops, **arrays) == cp.INVALID_ARGUMENT


def test_count_may_be_null_without_a_bit_list(arrays):
    assert accepted([Op(S, dw=1, pw=1), Op(bs.TEXT, 0)], arrays, count=False)
    arrays["count"] = 0
    assert build([Op(S, dw=1, pw=1), Op(bs.LIST_BIT, 0)], **arrays) == cp.INVALID_ARGUMENT


def test_sizes_only_needs_no_output_arrays(arrays):
    assert accepted([Op(S, dw=1, pw=1), Op(bs.TEXT, 0)], arrays, outputs=False)
    assert accepted([Op(S, dw=1, pw=1), Op(bs.TEXT, 0)], arrays, outputs=False, pool=False)


def test_python_wrapper_checks_column_sizes():
    import torch
    col = torch.zeros(7, dtype=torch.int64)
    n4 = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(cp.InvalidArgument):
        cp.build_fields_batch(None, [cp.BuildOp(cp.BUILD_STRUCT, 0, data_words=1), cp.BuildOp(cp.FIELD_U8, 0)], col,
                              col, None, None, None, n4, torch.zeros(4, dtype=torch.int32))
