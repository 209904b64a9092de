"""Batch layouts and expectations for capnp_packed_split_streams: what tests/test_split_streams.py
checks on the CPU and tests/test_gpu_split_streams.py runs on the device. No GPU and no torch here.

The property. Stream s of a batch is what repeated Reader.readPackedMessage calls on one reader
consume (reader.zig:84-156); the call lists its whole messages, the bytes they take and the status
the loop stopped with, exactly as framer_streams.whole_stream states it with the C oracle.

The streams are framer_streams' (connection_streams, large_streams, window_exit_streams) and a few
built here from the same pools for shapes those do not hold: the empty stream, cuts inside a header
and inside a last record, a header across a window line, one stream of several hundred messages
(the framer stops a pass at 64) and one of two messages of more than 20 windows each. A batch lays
them out densely, stream after stream with no gap and in a shuffled order, so that an over-read or
an overrun into the neighbour changes a result instead of faulting, with distinct non-zero filler
in front of the first stream and behind the last.
"""
import collections
import functools

import numpy as np

import framer_streams as fs
import reader_streams as rs
from framer_streams import W, connection_streams, large_streams, whole_stream, window_exit_streams

SEED = 0x5B117001
FRONT, BACK = 0xC3, 0x5A  # filler bytes in front of the first stream / behind the last
FRONT_LEN, BACK_LEN = 32, 64
N_MANY = 300              # messages of the many-messages stream
BIG_WINDOWS = 20          # windows of each message of the two-large-messages stream

# name: where the stream comes from; data: its bytes; msgs: (start, packed bytes, framed bytes) per
# whole message; consumed: where the loop stopped; status: its final ABI status
Stream = collections.namedtuple("Stream", "name data msgs consumed status")


def _stream(name, data):
    msgs, left, status, _ = whole_stream(data)
    return Stream(name, bytes(data), tuple(msgs), len(data) - left, status)


def _small_pool():
    return [c.data[:c.consumed] for c in rs.cases(rs.SEED) if c.status == rs.OK and 0 < c.consumed <= 1200]


def _header_end(msg):
    return rs.read_message(msg, header_only=True).consumed


def _pads_to(rng, small, by_len, target):
    """Whole small messages whose lengths sum to target modulo W (two random ones, then two whose
    lengths bring the sum there, as framer_streams.window_exit_streams does)."""
    for _ in range(4096):
        pads = [small[int(rng.integers(0, len(small)))] for _ in range(2)]
        t = (target - sum(len(m) for m in pads)) % W
        pair = next(((a, t - a) for a in sorted(by_len) if (t - a) in by_len), None)
        if pair:
            return pads + [by_len[pair[0]], by_len[pair[1]]]
    raise AssertionError("no four messages bring the sum to the target")


def built_streams(seed=SEED):
    """The streams built here: [(name, data)]."""
    rng = np.random.default_rng(seed)
    small = _small_pool()
    pick = lambda: small[int(rng.integers(0, len(small)))]
    out = [("empty", b"")]
    # the bytes end inside a header (one byte short of the record that completes the segment
    # table), bare and behind two whole messages
    multi = max(small, key=_header_end)
    assert _header_end(multi) >= 3
    out.append(("cut_in_header", multi[:_header_end(multi) - 1]))
    out.append(("cut_in_header_after_2", pick() + pick() + multi[:_header_end(multi) - 1]))
    # the bytes end inside the last record, and exactly at a message's end
    tail = next(m for m in small if len(m) - rs._record_starts(m)[-1][0] >= 3 and _header_end(m) < len(m) - 3)
    out.append(("cut_in_last_record", pick() + tail[:-1]))
    out.append(("ends_at_message_end", pick() + pick() + tail))
    # a header across a window line: the message starts one byte before the line
    wide = [c.data[:c.consumed] for c in rs.cases(rs.SEED) if c.status == rs.OK and 0 < c.consumed < W]
    pads = _pads_to(rng, wide, {len(m): m for m in wide}, W - 1)
    out.append(("header_across_window_line", b"".join(pads) + multi + pick()))
    # one stream of N_MANY whole messages, and the same with an error behind them
    many = b"".join(pick() for _ in range(N_MANY))
    out.append(("many_messages", many))
    out.append(("many_messages_then_cut", many + tail[:-1]))
    # two messages of more than BIG_WINDOWS windows each, bare and behind a small one
    bigs = []
    for info, st in large_streams():
        if info.ending == "exact_next" and info.front is None and info.words >= 20000:
            start, used, framed = whole_stream(st.data)[0][0]
            if used > BIG_WINDOWS * W:
                bigs.append(st.data[start:start + used])
        if len(bigs) == 2:
            break
    assert len(bigs) == 2
    out.append(("two_large_messages", bigs[0] + bigs[1]))
    out.append(("small_then_two_large_then_cut", pick() + bigs[1] + bigs[0] + tail[:-1]))
    return out


@functools.lru_cache(maxsize=1)
def corpus():
    """Every stream once: [Stream]."""
    out = [_stream(f"conn{i}", cs.data) for i, cs in enumerate(connection_streams())]
    out += [_stream(f"large{i}_{info.ending}", cs.data) for i, (info, cs) in enumerate(large_streams())]
    out += [_stream(f"exit_{place}_{mode}", cs.data) for place, mode, cs in window_exit_streams()]
    out += [_stream(name, data) for name, data in built_streams()]
    return out


# buf: the batch's bytes (filler, the streams back to back, filler); off / length: per stream;
# order: order[s] = index into the streams given
Layout = collections.namedtuple("Layout", "buf off length order")


def layout(streams, seed=SEED, shift=0):
    """The streams laid out densely in a shuffled order behind FRONT_LEN + shift filler bytes."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(streams))
    lens = np.array([len(streams[i].data) for i in order], dtype=np.int64)
    off = FRONT_LEN + shift + np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    buf = np.full(FRONT_LEN + shift + int(lens.sum()) + BACK_LEN, BACK, dtype=np.uint8)
    buf[:FRONT_LEN + shift] = FRONT
    for o, i in zip(off, order):
        d = streams[i].data
        buf[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    return Layout(buf, off, lens, order)


# first: n + 1 message counts before each stream; off / length / framed / stream: the rows;
# consumed / status: per stream
Expect = collections.namedtuple("Expect", "first off length framed stream consumed status")


def expect(streams, lay):
    """What the call must write for `streams` laid out as `lay`."""
    first, off, length, framed, stream, consumed, status = [0], [], [], [], [], [], []
    for s, i in enumerate(lay.order):
        st = streams[i]
        for start, used, fr in st.msgs:
            off.append(int(lay.off[s]) + start)
            length.append(used)
            framed.append(fr)
            stream.append(s)
        first.append(len(off))
        consumed.append(st.consumed)
        status.append(st.status)
    i64 = lambda v: np.array(v, dtype=np.int64)
    return Expect(i64(first), i64(off), i64(length), i64(framed), np.array(stream, dtype=np.int32), i64(consumed),
                  np.array(status, dtype=np.int32))


def frames(stream):
    """The framed bytes of a stream's whole messages, by the oracle's reader at each start."""
    held = bytearray(stream.data)
    out = []
    for start, used, fr in stream.msgs:
        rc, framed, took = fs.oracle_read_at(held, start)
        assert rc == 0 and took == used and len(framed) == fr
        out.append(framed)
    return out
