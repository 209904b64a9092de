"""The framer session (capnp_packed_framer_*) against the oracle reader under
split reads: a real cp.FramerSession and framer_streams.ModelSession driven by the same schedule
(tests/framer_streams.py; its inputs are checked on the CPU in tests/test_framer_streams.py).

After every read and for every slot: the frames popped in that read equal the model's as bytes
and in order, and so do status, buffered() and expected(). At the end every fed byte was
uploaded once. The streams are hostile: every reader error, overshooting zero and literal runs,
cut literal runs, truncations and random bytes, in hand-built, Zig-rule and C++-dialect records,
behind 0-3 whole messages, so that errors are met after a resume, in a window reached by a table
lookup, and in the message after one that was cut.
"""
import ctypes

import numpy as np
import pytest

import capnp_packed as cp
import framer_streams as fs
import reader_streams as rs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MAX_REPORTED = 12


class Mismatches:
    """What differed, by (round, slot, stream index); a slot that differed is left unchecked until
    its next stream starts (both sessions reset there), so one run shows every stream that fails."""

    def __init__(self, name):
        self.name, self.items, self.bad, self.count = name, [], set(), 0

    def add(self, r, c, stream, what, got, want):
        self.bad.add(c)
        self.count += 1
        if len(self.items) < MAX_REPORTED:
            self.items.append(f"round {r} slot {c} stream {stream}: {what}: got {got!r}, want {want!r}")

    def check(self):
        assert not self.items, f"{self.name}: {self.count} mismatches, the first:\n" + "\n".join(self.items)


def compare_round(mis, r, n, cur, got, want, sess, model):
    got_frames, got_status = got
    want_frames, want_status = want
    for c in range(n):
        if c in mis.bad:
            continue
        i = cur.get(c)
        g = [bytes(f) for f in got_frames.get(c, [])]
        w = [bytes(f) for f in want_frames.get(c, [])]
        if g != w:
            first = next((k for k, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            mis.add(r, c, i, f"frames (first difference at frame {first})", [len(x) for x in g], [len(x) for x in w])
        elif int(got_status[c]) != int(want_status[c]):
            mis.add(r, c, i, "status", int(got_status[c]), int(want_status[c]))
        elif sess.buffered(c) != model.buffered(c):
            mis.add(r, c, i, "buffered", sess.buffered(c), model.buffered(c))
        elif sess.expected(c) != model.expected(c):
            mis.add(r, c, i, "expected", sess.expected(c), model.expected(c))


def run_schedule(sched, name, read=None):
    """The schedule through a FramerSession and the model; returns the session's stats() and
    walk_stats().
    read(sess, reads) -> (frames, status): how a round's read is made (default: sess.read)."""
    n = sched.n_slots
    sess, model = cp.FramerSession(n), fs.ModelSession(n)
    mis = Mismatches(name)
    cur = {}
    try:
        for r, (resets, starts, reads) in enumerate(sched.rounds):
            cur.update(starts)
            for c in set(resets) | (mis.bad & set(starts)):
                sess.reset(c)
                model.reset(c)
            mis.bad -= set(starts)
            want = model.read(reads)
            try:
                got = sess.read(reads) if read is None else read(sess, reads)
            except cp.PackedError as e:
                slots = {c: cur.get(c) for c in sorted(reads)}
                pytest.fail(f"{name}: round {r}: the session raised {e!r}; slots read (slot: stream): {slots}")
            compare_round(mis, r, n, cur, got, want, sess, model)
        mis.check()
        assert sess.stats()["uploaded_bytes"] == sched.fed == model.fed
        return {**sess.stats(), **sess.walk_stats()}
    finally:
        sess.close()


@pytest.mark.parametrize("policy", list(fs.SMALL_POLICIES))
def test_soak(policy):
    """A fifth of the connection streams per policy (the five cover them once) through 192 slots,
    reused as streams end, fail or are reset."""
    run_schedule(fs.small_schedule(policy), f"soak[{policy}]")


def test_soak_long_lived_connections():
    """Streams of 50-140 KB (30-60 whole messages, then a corpus terminal) in reads of up to 4 KiB
    through 64 slots: a connection passes the end of its 64-KiB region with part of a message
    held, so held bytes slide or move to a new region (moved_bytes > 0) between the reads of a
    message, before the error or the cut arrives; a slot goes on without a reset after a stream
    that was consumed whole."""
    stats = run_schedule(fs.long_lived_schedule(), "soak_long_lived")
    assert stats["moved_bytes"] > 0, stats


def tight_read(frames_cap, max_frames=3):
    """capnp_packed_framer_read itself with a frames buffer of `frames_cap` bytes and a table of
    `max_frames` entries, called again with no new bytes while it returns OUT_OF_SPACE: frames and
    statuses accumulated over the calls of one read."""
    L = cp.lib()

    def read(sess, reads):
        n = sess.n
        host, off, lens = sess.assemble(reads)
        total = int(lens.sum())
        buf = np.zeros(frames_cap, dtype=np.uint8)
        fo, fl = np.zeros(max_frames, dtype=np.uint64), np.zeros(max_frames, dtype=np.uint64)
        fc, stc = np.zeros(max_frames, dtype=np.uint32), np.zeros(n, dtype=np.int32)
        nf = ctypes.c_uint32(0)
        frames, status = {}, np.full(n, cp.END_OF_STREAM, dtype=np.int32)
        first = True
        while True:
            rc = L.capnp_packed_framer_read(sess.handle, host.ctypes.data if first else None, total if first else 0,
                                            off.ctypes.data if first else None, lens.ctypes.data if first else None,
                                            buf.ctypes.data, buf.size, fo.ctypes.data, fl.ctypes.data, fc.ctypes.data,
                                            max_frames, stc.ctypes.data, ctypes.byref(nf))
            first = False
            read.calls += 1
            read.out_of_space += rc == cp.OUT_OF_SPACE
            if rc not in (cp.OK, cp.OUT_OF_SPACE):
                cp._raise(rc, "framer_read")
            assert rc == cp.OK or nf.value > 0, "OUT_OF_SPACE without a frame: the largest frame fits the buffer"
            for k in range(nf.value):
                frames.setdefault(int(fc[k]), []).append(buf[int(fo[k]):int(fo[k]) + int(fl[k])].tobytes())
            err = stc != cp.END_OF_STREAM
            assert not (err & (status != cp.END_OF_STREAM)).any(), "an error reported twice"
            status[err] = stc[err]
            if rc == cp.OK:
                return frames, status
    read.calls = read.out_of_space = 0
    return read


def test_soak_tight_buffers():
    """The random policy over the streams of test_soak[whole] through capnp_packed_framer_read
    with a frames buffer of the largest frame + 64 B and a frame table of 3 entries: most reads
    need several calls, and a message found whole that did not fit is marked as walked and
    popped by the next call, with the connection's later messages and its error queued behind."""
    share = fs.small_share("whole")
    largest = max(st.max_frame for _, st in share)
    sched = fs.schedule(share, fs.cut_random, fs.SEED + 99)
    read = tight_read(largest + 64)
    run_schedule(sched, "soak_tight_buffers", read=read)
    # 3 frames a call at the most: the whole messages of the streams need this many calls
    whole = sum(st.n_msgs for _, st in share)
    assert read.calls >= whole // 3 and read.out_of_space >= whole // 3 - len(sched.rounds) > 300


@pytest.mark.parametrize("policy", list(fs.LARGE_POLICIES))
def test_large(policy):
    """Messages of 4-126 windows, a slot each. The table rules of framer_read_locked: `whole`
    over the 70,000-word literal streams alone is the rule for an undecoded header (held bytes
    over 64 windows); header_then_rest and reads_64k are the rule for a known header (over two
    windows of framed bytes left, the unwalked bytes over a window)."""
    stats = run_schedule(fs.large_schedule(policy), f"large[{policy}]")
    if policy in ("header_then_rest", "reads_64k"):
        assert stats["table_windows"] > 0, stats
    if policy == "whole":
        only = fs.large_schedule("whole", only=lambda info: info.words == 70000 and info.density == "literal")
        stats = run_schedule(only, "large[whole, 70,000-word literal]")
        assert stats["table_windows"] > 0, stats


def test_large_message_ends_at_a_window_edge():
    """A 70,000-word message behind four small ones, whole in a fresh slot's first read (tables
    are built: over 64 windows, no header decoded), laid so that it ends on a line of the walk's
    window grid or a byte past one, or that its last record starts a byte before a line or on it.
    At the window's exit a lookup's word count equals the words left: the walk must end the
    message there, not cross into the next one."""
    stats = run_schedule(fs.window_exit_schedule(), "window_exit")
    assert stats["table_windows"] > 0, stats


def test_many_small_messages_past_64_windows():
    """One read of about 320 KB of small whole messages and then an overshooting zero run: the
    held bytes span over 64 windows with no header decoded, so tables are built, but every
    message ends inside a window and almost no lookup is taken. The walk finds 64 messages a
    pass."""
    rng = np.random.default_rng(0x64E5)
    cases = rs.cases(rs.SEED)
    pool = [c.data[:c.consumed] for c in cases if c.status == rs.OK and 64 <= c.consumed <= 2048]
    bad = next(c for c in cases if c.family == "zero_over" and c.fw > 100)
    msgs, size = [], 0
    while size < 320_000:
        msgs.append(pool[int(rng.integers(0, len(pool)))])
        size += len(msgs[-1])
    data = b"".join(msgs) + bad.data
    assert len(data) > fs.HEADERLESS_TABLE_WINDOWS * fs.W
    frames, rest, code = fs.oracle_frames(data)
    assert len(frames) == len(msgs) and code == cp.INVALID_PACKED_MESSAGE
    sess = cp.FramerSession(2)
    try:
        got, status = sess.read({1: data})
        assert [bytes(f) for f in got.get(1, [])] == frames and 0 not in got
        assert [int(x) for x in status] == [cp.END_OF_STREAM, cp.INVALID_PACKED_MESSAGE]
        assert sess.buffered(1) == 0 and sess.expected(1) == 0
        stats = sess.walk_stats()
        assert stats["table_windows"] > 0 and stats["passes"] >= -(-len(msgs) // 64), (stats, len(msgs))
    finally:
        sess.close()
