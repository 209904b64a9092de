"""The model of capnp_packed_build_fields_batch (tests/build_streams.py), pinned three ways
without a Zig toolchain:
  (a) known-answer vectors derived by hand from the reference lines, word by word;
  (b) every corpus message read back by struct_streams.read_fields (the read model, itself pinned
      by the fixtures) with the mirrored descriptors: it returns what was written;
  (c) the coverage table: both ways of every check of the model, every status, the sizes-only path."""
import random

import pytest

import build_streams as bs
import struct_streams as ss
from build_streams import Op


def words(hex_text):
    return bytes.fromhex(hex_text.replace(" ", "").replace("\n", ""))


def build_one(ops, row, **kw):
    pool, cols = bs.columns(ops, [row])
    kw.setdefault("cap", 1 << 40)
    return bs.build_message(ops, cols[0], pool, **kw)


# (a) ---------------------------------------------------------------------------------------------
# Each vector: toBytes (message.zig:2147-2157) gives the table word 0 | segment words << 32;
# allocateStruct (:2076-2087) the root pointer dw << 32 | pw << 48 at offset 0.
VECTORS = {
    # data word: writeU32 little-endian (struct_builder.zig:379-383). Pointer 0 at byte 16, the text
    # at byte 24: offset (24 - 16 - 8) / 8 = 0, makeListPointer(0, 2, 3) = 1 | 2 << 32 | 3 << 35
    # (message.zig:1808-1812, :37-43); "hi", NUL, 5 bytes of padding (:1796-1804).
    "A": (bs.SEED_A, """00000000 04000000  00000000 01000100  44332211 00000000
                        01000000 1a000000  68690000 00000000"""),
    # pointers at bytes 8 and 16. initStruct(1, 1, 0) appends at byte 24: offset (24 - 16 - 8) / 8
    # = 0, makeStructPointer(0, 1, 0) (:1869-1877). writeU8(7) then writeBool(0, 3) on that struct.
    # writeData appends 9 bytes + 7 of padding at byte 32 (:1929-1940): offset (32 - 8 - 8) / 8 = 2,
    # makeListPointer(2, 2, 9) = 1 | 2 << 2 | 2 << 32 | 9 << 35.
    "B": (bs.SEED_B, """00000000 06000000  00000000 00000200  09000000 4a000000
                        00000000 01000000  08000000 000000ab  01020304 05060708
                        09000000 00000000"""),
    # an empty text is its NUL: 1 byte + 7 of padding, count 1 (:1796-1812)
    "C": (bs.SEED_C, "00000000 03000000  00000000 00000100  01000000 0a000000  00000000 00000000"),
    # empty Data: listContentBytes = 0, nothing appended, the pointer is not null: offset 0 (the end
    # of the segment), size 2, count 0 (:1934-1948)
    "D": (bs.SEED_D, "00000000 02000000  00000000 00000100  01000000 02000000"),
    # initStruct(0, 0, 0) writes a null pointer and allocates nothing (:1851-1860); writeU16(6);
    # a bit list of 11: 2 bytes, the 5 unused bits 0, makeListPointer(0, 1, 11) = 1 | 1 << 32 | 11 << 35
    "E": (bs.SEED_E, """00000000 05000000  00000000 01000200  00000000 0000efbe
                        00000000 00000000  01000000 59000000  ff070000 00000000"""),
}


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_known_answer(name):
    (ops, row), want = VECTORS[name]
    st, n, out = build_one(ops, row)
    assert st == bs.OK and out == words(want) and n == len(out)


# (b) ---------------------------------------------------------------------------------------------
def mirrored(ops):
    """the read descriptor of every op (a BUILD_STRUCT op: a placeholder that keeps the indices)"""
    return [ss.F(ss.U8, 0) if o.kind == bs.STRUCT else ss.F(o.kind, o.offset, o.bit, p)
            for o, p in zip(ops, bs.paths(ops))]


def overwritten(ops, k):
    """a later data op touches a byte of data op k (same struct)"""
    o = ops[k]
    w = 1 if o.kind == bs.BOOL else bs.WIDTH[o.kind]
    for l in ops[k + 1:]:
        if l.kind <= bs.BOOL and l.target == o.target:
            lw = 1 if l.kind == bs.BOOL else bs.WIDTH[l.kind]
            if l.offset < o.offset + w and o.offset < l.offset + lw:
                return True
    return False


def check_readback(ops, row, framed, pool, col):
    got = ss.read_fields(framed, mirrored(ops))
    for k, o in enumerate(ops):
        if o.kind == bs.STRUCT:
            continue
        st, value, length, count = got[k]
        t = ops[o.target]
        under_null = any(ops[a].kind == bs.STRUCT and a and ops[a].dw + ops[a].pw == 0 for a in ancestors(ops, k))
        if under_null:
            assert st == ss.INVALID_POINTER  # readStruct of the null pointer initStruct(0, 0) wrote
            continue
        if o.kind <= bs.BOOL:
            width = 1 if o.kind == bs.BOOL else bs.WIDTH[o.kind]
            assert st == ss.OK
            if o.offset + width > 8 * t.dw:
                assert (value, length) == (0, 0)  # dropped by the write, defaulted by the read
            elif row[k] is not None and not overwritten(ops, k):
                want = row[k] & 1 if o.kind == bs.BOOL else row[k] & ((1 << (8 * width)) - 1)
                assert value == want, (k, o)
        elif row[k] is None:  # absent: the pointer stays null
            assert (st, length) == ((ss.OK, 0) if o.kind == bs.TEXT else (ss.INVALID_POINTER, 0))
        else:
            data, n = row[k] if o.kind == bs.LIST_BIT else (row[k], None)
            assert st == ss.OK and length == len(data)
            content = bytearray(data)
            if o.kind == bs.LIST_BIT:
                assert count == n
                if n % 8:
                    content[-1] &= (1 << (n % 8)) - 1
            elif o.kind in (bs.LIST_16, bs.LIST_32, bs.LIST_64):
                assert count == len(data) >> (o.kind - bs.LIST_16 + 1)
            else:
                assert count == len(data)
            assert framed[value:value + length] == bytes(content)


def ancestors(ops, k):
    a, out = ops[k].target, []
    while True:
        out.append(a)
        if a == 0:
            return out
        a = ops[a].target


CORPUS = bs.corpus()


def test_corpus_reads_back():
    seen_ops = set()
    for ops, rows in CORPUS:
        assert bs.check_ops(ops)
        seen_ops.add(len(ops))
        pool, cols = bs.columns(ops, rows)
        for row, col in zip(rows, cols):
            st, n, framed = bs.build_message(ops, col, pool, cap=1 << 40)
            assert st == bs.OK and len(framed) == n and n % 8 == 0
            check_readback(ops, row, framed, pool, col)
    assert {1, 32} <= seen_ops


# (c) ---------------------------------------------------------------------------------------------
def test_coverage():
    bs.SEEN.clear()
    S = bs.STRUCT
    for ops, rows in CORPUS:
        bs.check_ops(ops)
        pool, cols = bs.columns(ops, rows)
        for col in cols:
            bs.build_message(ops, col, pool, cap=1 << 40)
    # the host-side refusals
    refused = {
        "too many": [Op(S, dw=1)] + [Op(bs.U8, 0)] * 32,
        "none": [],
        "op 0": [Op(bs.U8, 0)],
        "kind": [Op(S, dw=1), Op(11, 0)],
        "kind 17": [Op(S, dw=1), Op(17, 0)],
        "bit 8": [Op(S, dw=1), Op(bs.BOOL, 0, bit=8)],
        "bit off bool": [Op(S, dw=1), Op(bs.U8, 0, bit=1)],
        "reserved": [Op(S, dw=1), Op(bs.U8, 0, reserved=(0, 0, 1))],
        "target later": [Op(S, dw=1), Op(bs.U8, 0, target=1)],
        "target not struct": [Op(S, dw=1), Op(bs.U8, 0), Op(bs.U8, 0, target=1)],
        "pointer index": [Op(S, pw=1), Op(bs.TEXT, 1)],
        "struct pointer index": [Op(S, pw=1), Op(S, 1, dw=1)],
        "slot twice": [Op(S, pw=1), Op(bs.TEXT, 0), Op(bs.DATA, 0)],
        "64 words": [Op(S, dw=32, pw=1), Op(S, 0, dw=31)],
    }
    for name, ops in refused.items():
        assert not bs.check_ops(ops), name
    assert bs.check_ops([Op(S, dw=32, pw=1), Op(S, 0, dw=30)])  # 63 struct words + the root pointer
    # every status of the call
    ops = [Op(S, dw=1, pw=3), Op(bs.LIST_16, 0), Op(bs.LIST_BIT, 1), Op(bs.DATA, 2)]
    pool = bytes(64)
    good = [(0, 0, 0), (0, 4, 0), (4, 2, 9), (8, 5, 0)]

    def with_(k, entry):
        return good[:k] + [entry] + good[k + 1:]

    size = 8 * (1 + 1 + 4 + 1 + 1 + 1)
    assert bs.build_message(ops, good, pool, cap=size)[:2] == (bs.OK, size)
    assert bs.build_message(ops, good, pool, sizes_only=True) == (bs.OK, size, None)
    assert bs.build_message(ops, good, pool, sizes_only=True, out_addr=4)[0] == bs.OK
    assert bs.build_message(ops, good, pool, cap=size, out_addr=4) == (bs.INVALID_ARGUMENT, 0, None)
    assert bs.build_message(ops, good, pool, cap=size - 8) == (bs.OUT_OF_SPACE, size, None)
    assert bs.build_message(ops, with_(1, (0, 3, 0)), pool, cap=size)[0] == bs.INVALID_ARGUMENT
    assert bs.build_message(ops, with_(2, (4, 1, 9)), pool, cap=size)[0] == bs.INVALID_ARGUMENT
    assert bs.build_message(ops, with_(3, (0, 1 << 29, 0)), pool, cap=size)[0] == bs.LIST_TOO_LARGE
    assert bs.build_message(ops, with_(3, (60, 5, 0)), pool, cap=size)[0] == bs.OUT_OF_BOUNDS
    assert bs.build_message(ops, with_(3, (65, 0, 0)), pool, cap=size)[0] == bs.OUT_OF_BOUNDS
    assert bs.build_message(ops, with_(3, (64, 0, 0)), pool, cap=size)[0] == bs.OK
    # the first failing op wins, and within an op the table's order
    assert bs.build_message(ops, with_(1, (0, 3, 0))[:3] + [(0, 1 << 29, 0)], pool, cap=size)[0] == bs.INVALID_ARGUMENT
    assert bs.build_message(ops, with_(3, (1 << 40, 1 << 29, 0)), pool, cap=size)[0] == bs.LIST_TOO_LARGE
    # 8 Data slices of 2^29 - 1 bytes: 4 GiB framed
    big = [Op(S, pw=8)] + [Op(bs.DATA, p) for p in range(8)]
    cols = [(0, 0, 0)] + [(0, (1 << 29) - 1, 0)] * 8
    assert bs.build_message(big, cols, b"", pool_len=1 << 29, cap=0) == (bs.MESSAGE_TOO_LARGE, 0, None)
    missing = [(c, w) for c in bs.CHECKS for w in (False, True) if (c, w) not in bs.SEEN]
    assert not missing, missing
    assert {c for c, _ in bs.SEEN} <= set(bs.CHECKS)


def test_later_write_wins_and_bool_is_read_modify_write():
    ops = [Op(bs.STRUCT, dw=2), Op(bs.U64, 0), Op(bs.U16, 3), Op(bs.BOOL, 4, bit=0), Op(bs.BOOL, 3, bit=7),
           Op(bs.U32, 6)]
    st, n, out = build_one(ops, [None, 0x1111111111111111, 0xABCD, 0, 0, 0x99887766])
    assert st == bs.OK
    # U64, then U16 over bytes 3-4, bit 0 of byte 4 cleared (0xAB -> 0xAA), bit 7 of byte 3 cleared
    # (0xCD -> 0x4D), then a U32 straddling both words at bytes 6-9
    assert out[16:32] == bytes([0x11, 0x11, 0x11, 0x4D, 0xAA, 0x11, 0x66, 0x77, 0x88, 0x99, 0, 0, 0, 0, 0, 0])


def test_generator_is_deterministic():
    a = bs.gen_program(random.Random(3), 20)
    b = bs.gen_program(random.Random(3), 20)
    assert [repr(o) for o in a] == [repr(o) for o in b] and bs.check_ops(a)
