"""The framed encoders' model and generators (tests/framed_streams.py) on the CPU: the model
against the oracle's Message.init, the routes and statuses the generators reach, and the
identity the kernels' single-segment fast path rests on."""
import struct

import numpy as np
import pytest

import framed_streams as fs
import oracle
import pyref_cxx


def zig_pack(b):
    st, p = oracle.pack(b)
    assert st == oracle.OK
    return p


# oracle_message_init's return codes (oracle/packed_oracle.h)
ORACLE_TO_ABI = {0: fs.OK, -1: fs.END_OF_STREAM, -2: fs.INVALID_SEGMENT_COUNT, -3: fs.SEGMENT_COUNT_LIMIT_EXCEEDED,
                 -4: fs.TRUNCATED_MESSAGE, -5: fs.INVALID_MESSAGE_SIZE}


def all_units():
    rng = np.random.default_rng(0xF4A3ED01)
    units = {k: fs.frame(v) for k, v in fs.boundary_units().items()}
    units.update(fs.count_units(rng))
    units.update(fs.tile_edge_units(rng))
    units.update({k: u for k, (u, _) in fs.error_units().items()})
    for i in range(200):
        units[f"random_{i}"] = fs.random_frame(rng)
    return units


def test_model_agrees_with_the_oracles_message_init():
    for name, unit in all_units().items():
        if len(unit) % 8:
            continue
        st, segs = fs.message_init(unit)
        o = oracle.message_init(unit)
        assert ORACLE_TO_ABI[o[0]] == st, name
        if st == fs.OK:
            assert pyref_cxx.split_framed(unit) == segs, name
            assert fs.frame(segs)[:4 * (1 + len(segs))] == unit[:4 * (1 + len(segs))]


def test_error_units_get_their_statuses_in_order():
    for name, (unit, want) in fs.error_units().items():
        assert fs.verdict(unit)[0] == want, name
        # a misaligned word side comes first, whatever else is wrong
        assert fs.verdict(unit, address=4)[0] == fs.INVALID_ARGUMENT, name
    # len % 8 comes before the table parse, the table parse before the trailing-words rule
    assert fs.verdict(fs.count_field(0xFFFFFFFF, 12))[0] == fs.INVALID_MESSAGE_SIZE
    assert fs.verdict(fs.count_field(0xFFFFFFFF, 16))[0] == fs.INVALID_SEGMENT_COUNT
    assert fs.verdict(struct.pack("<II", 0, 5) + bytes(8))[0] == fs.TRUNCATED_MESSAGE
    # Message.init itself ignores trailing words; the framed calls must not
    unit = fs.error_units()["one_trailing_word"][0]
    assert fs.message_init(unit)[0] == fs.OK and fs.verdict(unit)[0] == fs.INVALID_ARGUMENT


def test_coverage_of_routes_and_statuses():
    units = all_units()
    seen = {(d, fs.route(u, d)) for u in units.values() for d in ("zig", "cxx")}
    assert seen == {(d, r) for d in ("zig", "cxx") for r in ("fail", "tile", "walk")}
    statuses = {fs.verdict(u)[0] for u in units.values()}
    assert statuses == {fs.OK, fs.INVALID_MESSAGE_SIZE, fs.INVALID_ARGUMENT, fs.END_OF_STREAM,
                        fs.INVALID_SEGMENT_COUNT, fs.SEGMENT_COUNT_LIMIT_EXCEEDED, fs.TRUNCATED_MESSAGE}
    ok = [u for u in units.values() if fs.verdict(u)[0] == fs.OK]
    counts = {len(fs.verdict(u)[1]) for u in ok}
    assert {1, 2, 3, 63, 64, 65, 511, 512} <= counts
    # multi-segment units of one tile (walked under the C++ rule only), single-segment units of
    # more than one tile (walked under both), first segments at 8 mod 16 (an odd table)
    assert any(fs.route(u, "cxx") == "walk" and fs.route(u, "zig") == "tile" for u in ok)
    assert any(len(fs.verdict(u)[1]) == 1 and fs.route(u, "zig") == "walk" for u in ok)
    assert any((len(fs.verdict(u)[1]) // 2 + 1) % 2 == 1 and len(fs.verdict(u)[1]) > 1 for u in ok)
    # pieces of more than one tile and of more than two
    assert any(max(len(s) for s in fs.verdict(u)[1]) > 8 * 1024 for u in ok)


def test_boundary_units_pack_as_the_rule_says():
    b = fs.boundary_units()
    table2 = pyref_cxx.pack_piece(pyref_cxx.segment_table([bytes(16), bytes(16)]))
    # Z Z | Z Z: the zero run restarts at the boundary
    assert pyref_cxx.pack_message(b["ZZ|ZZ"]) == table2 + bytes((0, 1, 0, 1))
    assert pyref_cxx.pack_buffer(b"".join(b["ZZ|ZZ"])) == bytes((0, 3))
    # A A | A A: two literal runs of one following word each
    got = pyref_cxx.pack_message(b["AA|AA"])
    assert got[len(table2):][0] == 0xFF and got[len(table2):][9] == 1 and len(got) == len(table2) + 2 * 18
    # A | B: the B is a tag record, not a literal word of the A's run
    got = pyref_cxx.pack_message(b["A|B"])
    tail = got[len(pyref_cxx.pack_piece(pyref_cxx.segment_table(b["A|B"]))):]
    assert tail[:10] == b"\xff" + b["A|B"][0] + b"\x00" and len(tail) == 10 + 1 + 7
    # (k, 0, 0): the table's last word is zero and segment 0 starts with zero words
    t = pyref_cxx.segment_table(b["k,0,0"])
    assert t[8:] == bytes(8) and b["k,0,0"][0][:24] == bytes(24)
    got = pyref_cxx.pack_message(b["k,0,0"])
    assert got[:len(pyref_cxx.pack_piece(t))].endswith(bytes((0, 0)))
    assert got[len(pyref_cxx.pack_piece(t)):][:2] == bytes((0, 2))
    for name, segs in b.items():
        st, p = fs.expected(fs.frame(segs), "cxx", zig_pack)
        assert st == fs.OK and p == pyref_cxx.pack_message(segs), name


SIZES = (0, 1, 2, 7, 8, 63, 64, 65, 255, 256, 257, 511, 512, 513)
PROBS = (0, 0.02, 0.5, 0.9, 1)


@pytest.mark.parametrize("p", PROBS)
def test_single_segment_identity(p):
    """pack_message([s]) == pack_buffer(framed): the table word (0, size) has at least four zero
    bytes, so it is never an A or B word and no literal run crosses it, and it is a Z word only
    when the segment is empty."""
    rng = np.random.default_rng(0xF4A3ED02)
    for words in SIZES:
        for rep in range(4):
            seg = fs.rand_words(rng, words, p)
            framed = fs.frame([seg])
            assert pyref_cxx.pack_message([seg]) == pyref_cxx.pack_buffer(framed), (words, p, rep)
            assert fs.route(framed, "cxx") == ("tile" if words + 1 <= fs.TILE_WORDS else "walk")
    # the identity fails for more than one segment (which is why those are walked)
    segs = fs.boundary_units()["ZZ|ZZ"]
    assert pyref_cxx.pack_message(segs) != pyref_cxx.pack_buffer(fs.frame(segs))


def test_zig_dialect_is_whole_buffer_packing():
    rng = np.random.default_rng(0xF4A3ED03)
    for _ in range(20):
        unit = fs.random_frame(rng, max_segs=8, max_words=200)
        assert fs.expected(unit, "zig", zig_pack) == (fs.OK, zig_pack(unit))
