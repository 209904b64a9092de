"""The C++-canonical packing rule as tests/pyref_cxx.py states it, pinned by
the four packed fixtures the C++ encoder and pycapnp wrote (tests/golden/fixtures). CPU only."""
import os

import numpy as np
import pytest

import oracle
import pyref_cxx as rx

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "fixtures")

PAIRS = [("binary", "packed"), ("segmented", "segmented-packed"),
         ("fixture_single.bin", "fixture_single_packed.bin"), ("fixture_far.bin", "fixture_far_packed.bin")]


def fixture(name: str) -> bytes:
    with open(os.path.join(FIX, name), "rb") as f:
        return f.read()


@pytest.mark.parametrize("raw,packed", PAIRS)
def test_per_piece_reproduces_fixture(raw, packed):
    framed = fixture(raw)
    segs = rx.split_framed(framed)
    assert rx.segment_table(segs) + b"".join(segs) == framed
    assert rx.pack_message(segs) == fixture(packed)


@pytest.mark.parametrize("raw,packed", PAIRS)
def test_whole_buffer_differs_only_on_segmented(raw, packed):
    whole = rx.pack_buffer(fixture(raw))
    if raw == "segmented":
        assert whole != fixture(packed)  # the restart at each of its 126 pieces changes the bytes
    else:
        assert whole == fixture(packed)


def test_piece_counts():
    counts = {raw: 1 + len(rx.split_framed(fixture(raw))) for raw, _ in PAIRS}
    assert counts == {"binary": 2, "segmented": 126, "fixture_single.bin": 2, "fixture_far.bin": 5}


KNOWN = [("B A B C", 33), ("A*257", 2060), ("A*256 B A", 2068), ("A*256 B B A B", 2084), ("A Z A", 22),
         ("Z*257", 4), ("", 0)]


@pytest.mark.parametrize("spec,size", KNOWN)
def test_known_answers(spec, size):
    data = rx.words(spec)
    p = rx.pack_piece(data)
    assert len(p) == size
    st, back = oracle.unpack(p)
    assert st == oracle.OK and back == data


def test_same_length_different_bytes():
    data = rx.words("B A B C")
    st, zig = oracle.pack(data)
    cxx = rx.pack_piece(data)
    assert st == oracle.OK and len(zig) == len(cxx) == 33 and zig != cxx
    w = [data[8 * i:8 * i + 8] for i in range(4)]
    nz = lambda x: bytes(b for b in x if b)
    tag = lambda x: bytes((sum(1 << k for k in range(8) if x[k]),))
    # the run's count byte is 01 and the second B is raw
    assert cxx == tag(w[0]) + nz(w[0]) + b"\xff" + w[1] + b"\x01" + w[2] + tag(w[3]) + nz(w[3])
    assert zig == tag(w[0]) + nz(w[0]) + b"\xff" + w[1] + b"\x00" + tag(w[2]) + nz(w[2]) + tag(w[3]) + nz(w[3])


def test_cap_edges():
    a, b = rx.word_a, rx.word_b
    p = rx.pack_piece(rx.words("A*256 B A"))
    assert p[0] == 0xFF and p[9] == 255           # the first run holds 256 words
    assert p[2050] == 0xFF ^ 0x01                 # the B after the cap is a tag record (byte 0 is its zero)
    assert p[2058] == 0xFF and p[2067] == 0       # and the next A opens a run of one
    p = rx.pack_piece(rx.words("Z*257"))
    assert p == bytes((0, 255, 0, 0))
    assert a(3).count(0) == 0 and b(3).count(0) == 1 and rx.word_c(3).count(0) == 2


def random_unit(rng, nwords, p):
    a = rng.integers(1, 256, size=8 * nwords, dtype=np.uint8)
    a[rng.random(8 * nwords) < p] = 0
    return a.tobytes()


@pytest.mark.parametrize("p", [0.02, 0.1, 0.5, 0.9])
def test_round_trip_and_never_larger(p):
    rng = np.random.default_rng(int(p * 1000) + 7)
    smaller = 0
    for _ in range(100):
        data = random_unit(rng, int(rng.integers(0, 700)), p)
        cxx = rx.pack_piece(data)
        st, back = oracle.unpack(cxx)
        assert st == oracle.OK and back == data
        st, zig = oracle.pack(data)
        assert st == oracle.OK and len(cxx) <= len(zig)
        smaller += len(cxx) < len(zig)
    if p in (0.02, 0.1):
        assert smaller > 0  # B words inside runs are common there
