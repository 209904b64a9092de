"""The reader-stream corpus (tests/reader_streams.py) against the oracle, on the CPU.

- read_message (the plain-Python reader) and oracle_read_packed_message agree on status, decoded
  bytes and consumed: every corpus stream of at most 2,048 bytes, every 8th longer one, and the
  reader.zig:304-386 known answers of tests/test_gpu_read_message.py::test_reader_kats.
- What the generator says of each stream it built (family, the record that reaches or passes the
  framed length, where that record ends) holds: by the oracle's status for every stream, by
  read_message's facts for the sampled ones.
- The coverage table: the cells the GPU fuzz (tests/test_gpu_read_message_fuzz.py) relies on are
  filled by this seed. The minima are conditions on the generator, not measurements.
"""
import collections
import hashlib
import struct

import pytest

import reader_streams as rs


@pytest.fixture(scope="module")
def cases():
    return rs.cases(rs.SEED)


def test_corpus_is_pinned():
    """corpus(SEED) byte for byte: the GPU fuzzes and the framer streams built on it
    (tests/framer_streams.py) stay the ones their coverage tables were checked on."""
    streams = rs.corpus(rs.SEED)
    digest = hashlib.sha256(b"".join(s.data for s in streams)).hexdigest()
    assert len(streams) == 5922
    assert digest == "d41d631c58bba6e8a398f184fcd5fb3b7c9bb74bc91170a18ae2dd03e4af1aa6"


def sampled(cases):
    longer = 0
    for c in cases:
        if len(c.data) <= 2048:
            yield c
        else:
            longer += 1
            if longer % 8 == 0:
                yield c


def test_python_reader_agrees_with_the_oracle(cases):
    n = 0
    for c in sampled(cases):
        got = rs.read_message(c.data)
        assert (got.status, got.framed, got.consumed) == (c.status, c.framed, c.consumed), \
            (c.family, len(c.data), got.status, c.status, got.consumed, c.consumed)
        # the header-only read every stream got says the same as the full one
        assert got.fw == c.fw, (c.family, got.fw, c.fw)
        if c.fw is not None:
            assert got.spans == c.spans
        # what the generator built is what a reader meets
        if c.family in ("zero_over", "lit_over", "lit_cut"):
            assert (got.kind, got.rend) == (c.kind, c.rend), (c.family, got.kind, got.rend, c.kind, c.rend)
        if c.family == "trunc":  # the last record of the message itself may be a literal run
            assert got.kind is None or (got.kind == "lit" and got.rend > len(c.data))
        n += 1
    assert n >= 3000


def test_python_reader_on_the_known_answers():
    """The streams of test_gpu_read_message.py::test_reader_kats (reader.zig:304-386)."""
    p = bytearray(10)
    p[0] = 0xFF
    p[1:9] = struct.pack("<Q", 0x00000000FFFFFFFF)
    bad_count = bytes(p)
    p[1:9] = struct.pack("<Q", (8 * 1024 * 1024 + 1) << 32)
    too_large = bytes(p)
    streams = [bad_count, too_large, b"\x00\x01", b"\x00", b"\xff", b"\x01", b"\x10\x01\x00\x00", b""]
    want = [rs.INVALID_SEGMENT_COUNT, rs.MESSAGE_TOO_LARGE, rs.INVALID_PACKED_MESSAGE, rs.END_OF_STREAM,
            rs.END_OF_STREAM, rs.END_OF_STREAM, rs.OK, rs.END_OF_STREAM]
    for s, w in zip(streams, want):
        got = rs.read_message(s)
        assert got.status == w
        assert (got.status, got.framed, got.consumed) == rs.oracle_read(s)
    got = rs.read_message(streams[6])
    assert (got.framed, got.consumed, got.fw, got.kind) == (bytes(4) + b"\x01" + bytes(11), 4, 2, "zero")


def test_families_read_as_built(cases):
    want = {"exact": rs.OK, "zero_over": rs.INVALID_PACKED_MESSAGE, "lit_over": rs.INVALID_PACKED_MESSAGE,
            "lit_cut": rs.END_OF_STREAM, "trunc": rs.END_OF_STREAM}
    for c in cases:
        if c.family in want:
            assert c.status == want[c.family], (c.family, len(c.data), c.status)
            assert c.fw is not None or c.family == "trunc"
        if c.family in ("zero_over", "lit_over"):
            assert c.consumed == c.rend and len(c.framed) > 8 * c.fw
        if c.family == "lit_cut":
            assert len(c.data) < c.rend
        if c.family == "exact":
            assert len(c.framed) == 8 * c.fw
    total = sum(len(c.data) for c in cases)
    assert 5000 <= len(cases) <= 7000 and total < 24 << 20, (len(cases), total)


def test_coverage_table(cases):
    cell = collections.Counter()
    for c in cases:
        if c.fw is None:
            continue
        route = "words" if c.fw <= rs.WORDS_ROUTE_MAX else "walk"
        cell[route, len(c.data) > 10 * c.fw, rs.outcome(c)] += 1
    for past in (False, True):
        for kind in rs.OUTCOMES:
            assert cell["words", past, kind] >= 32, (past, kind, cell["words", past, kind])
    assert cell["words", False, "eos_trunc"] >= 32
    for kind in rs.OUTCOMES:
        assert cell["walk", False, kind] + cell["walk", True, kind] >= 8, kind

    # a message takes at most 10 packed bytes per framed word, so a stream longer than that
    # cannot end before the framed length: the only EndOfStream there is a cut literal run
    for c in cases:
        if c.status == rs.END_OF_STREAM and c.fw is not None and len(c.data) > 10 * c.fw:
            if c.family == "random":
                got = rs.read_message(c.data)
                assert got.kind == "lit" and len(c.data) < got.rend
            else:
                assert c.family == "lit_cut", c.family
    assert cell["words", True, "eos_trunc"] == 0 and cell["walk", True, "eos_trunc"] == 0

    # one byte short of the overshooting literal run's end, and its end exactly, past 10 * fw
    past = [c for c in cases if c.kind == "lit" and c.fw <= rs.WORDS_ROUTE_MAX and len(c.data) > 10 * c.fw]
    assert any(len(c.data) == c.rend - 1 and c.status == rs.END_OF_STREAM for c in past)
    assert any(len(c.data) == c.rend and c.status == rs.INVALID_PACKED_MESSAGE for c in past)

    by_status = collections.Counter(c.status for c in cases)
    for st in (rs.INVALID_SEGMENT_COUNT, rs.SEGMENT_COUNT_LIMIT_EXCEEDED, rs.MESSAGE_TOO_LARGE):
        assert by_status[st] >= 4, st
    # a zero run of at least 16 words as the record that reaches or passes the framed length
    assert sum(1 for c in cases if c.kind == "zero" and c.data[c.rend - 1] + 1 >= 16) >= 32
    assert sum(1 for c in cases if c.spans) >= 32
    # both packing dialects' frames, every listed segment count, both routes' bounds
    fws = {c.fw for c in cases if c.family == "exact"}
    assert {1, 2} <= fws and set(range(1019, 1031)) <= fws and any(f > 2900 for f in fws)
    assert any(100 <= f <= 1000 for f in fws)
    counts = {struct.unpack_from("<I", c.framed)[0] + 1 for c in cases if c.family == "exact"}
    assert counts >= set(rs.SEGMENT_COUNTS)
