"""The framer fuzz's inputs (tests/framer_streams.py) on the CPU, with no device.

- Model agreement: every schedule replayed through ModelSession gives, over all reads of a
  stream, the frames, final status and held bytes of the whole-stream loop (oracle_frames). An
  error comes in a stream's last read and in no earlier one. The whole-stream loop on
  reader_streams.read_message, message by message, gives the same on every stream of every
  family: two independent restatements of Reader.readPackedMessage.
- The coverage table: the cells tests/test_gpu_framer_fuzz.py relies on are filled by this seed.
  The minima are conditions on the inputs, not measurements.
"""
import collections

import numpy as np
import pytest

import capnp_packed as cp
import framer_streams as fs
import reader_streams as rs


OUTCOMES = ("ok", "invalid_zero", "invalid_lit", "eos_cut", "eos_trunc")
HEADER_ERRORS = (rs.INVALID_SEGMENT_COUNT, rs.SEGMENT_COUNT_LIMIT_EXCEEDED, rs.MESSAGE_TOO_LARGE)


def test_status_codes_are_the_bindings():
    assert fs.ABI_OK == cp.OK
    for name, code in fs.ABI.items():
        assert getattr(cp, name) == code, name


def test_corpus_modes_and_extra_header_errors():
    streams = fs.connection_streams()
    n_cases = len(rs.cases(rs.SEED))
    extra = streams[n_cases + 5 * 18:]
    assert len(extra) >= 150 and all(st.family == "lit_count0" and st.kind == "lit" for st in extra)
    assert {st.mode for st in extra} == set(fs.MODES)
    for st in extra:  # FF w 00 ends the message exactly: the reader stops at rend with OK
        msgs = fs.whole_stream(st.data)[0]
        assert len(msgs) > st.n_prefix and sum(msgs[st.n_prefix][:2]) == st.rend
        assert st.data[st.rend - 10] == 0xFF and st.data[st.rend - 1] == 0
    # every corpus case is a terminal once: its bytes end the stream, in corpus order
    for st, c in zip(streams, rs.cases(rs.SEED)):
        assert st.data[st.prefix_len:] == c.data and (st.family, st.kind, st.mode) == (c.family, c.kind, c.mode)
        assert 0 <= st.n_prefix <= 3
    assert {st.n_prefix for st in streams} == {0, 1, 2, 3}


def read_message_loop(data):
    """oracle_frames' loop on reader_streams.read_message."""
    frames, pos = [], 0
    while pos < len(data):
        got = rs.read_message(data[pos:])
        if got.status != rs.OK:
            return frames, len(data) - pos, fs.ABI[got.status]
        frames.append(got.framed)
        pos += got.consumed
    return frames, 0, fs.ABI_OK


class Collector:
    """Per stream of a schedule: the frames, statuses and final held bytes a session gave."""

    def __init__(self, sched, sess):
        self.sched, self.sess = sched, sess
        self.cur = {}      # slot -> stream index
        self.frames = {}   # stream index -> frames so far
        self.status = {}   # stream index -> statuses of its reads
        self.done = {}     # stream index -> (frames, statuses, held)

    def __call__(self, r, reads, results):
        frames, status = results[0]
        self.cur.update(self.sched.rounds[r][1])
        for c in frames:
            assert c in reads, (r, c)  # a slot that got no bytes pops nothing
        for c in reads:
            i = self.cur[c]
            self.frames.setdefault(i, []).extend(bytes(f) for f in frames.get(c, []))
            self.status.setdefault(i, []).append(int(status[c]))
            if self.sched.last[i] == (r, c):
                self.done[i] = (self.frames.pop(i), self.status.pop(i), self.sess.buffered(c))


def check_agreement(sched, streams):
    sess = fs.ModelSession(sched.n_slots)
    col = Collector(sched, sess)
    fs.replay(sched, [sess], col)
    assert sess.fed == sched.fed
    for i, st in streams:
        if not st.data:
            continue
        frames, statuses, held = col.done[i]
        want_frames, rest, code = fs.oracle_frames(st.data)
        assert code == st.status
        assert frames == want_frames, i
        final = code if code not in (fs.ABI_OK, fs.ABI_END_OF_STREAM) else fs.ABI_END_OF_STREAM
        assert statuses[-1] == final and set(statuses[:-1]) <= {fs.ABI_END_OF_STREAM}, (i, statuses, final)
        assert held == (len(rest) if code == fs.ABI_END_OF_STREAM else 0), i
        if code not in (fs.ABI_OK, fs.ABI_END_OF_STREAM):
            assert st.err_at is not None and st.stop_at == len(st.data) - len(rest)
    assert not col.frames and len(col.done) == sum(1 for _, st in streams if st.data)


@pytest.mark.parametrize("policy", list(fs.SMALL_POLICIES))
def test_model_agreement(policy):
    share = fs.small_share(policy)
    check_agreement(fs.small_schedule(policy), share)


@pytest.mark.parametrize("policy", list(fs.LARGE_POLICIES))
def test_model_agreement_large(policy):
    check_agreement(fs.large_schedule(policy), fs.large_share())


@pytest.mark.parametrize("family", ["connection", "large", "window_exit", "long_lived"])
def test_read_message_agrees_on_every_stream(family):
    """The second restatement: reader_streams.read_message message by message against the oracle's
    whole-stream loop, on every stream the schedules are made of."""
    streams = {"connection": fs.connection_streams, "large": lambda: [st for _, st in fs.large_streams()],
               "window_exit": lambda: [st for _, _, st in fs.window_exit_streams()],
               "long_lived": fs.long_lived_streams}[family]()
    for i, st in enumerate(streams):
        frames, rest, code = fs.oracle_frames(st.data)
        assert read_message_loop(st.data) == (frames, len(rest), code), (family, i)


def test_model_agreement_long_lived():
    streams = fs.long_lived_streams()
    assert len(streams) >= 200 and all(len(st.data) > 40_000 for st in streams)
    n = collections.Counter(st.outcome for st in streams)
    for kind in OUTCOMES:
        assert n[kind] >= 5, (kind, n)
    # slots are reused, and a slot goes on without a reset after a stream that was consumed whole
    sched = fs.long_lived_schedule()
    assert len(streams) >= 3 * sched.n_slots and sum(st.status == fs.ABI_OK for st in streams) >= 5
    check_agreement(sched, list(enumerate(streams)))


def test_model_agreement_window_exit():
    """The large messages laid against the window grid, and that they are: the message's end, or
    its last record's start, at the stated distance from a multiple of W from the stream's start."""
    streams = fs.window_exit_streams()
    assert {(p, m) for p, m, _ in streams} == {(p, m) for p in fs.WINDOW_EXIT_PLACES for m in fs.MODES}
    for place, mode, cs in streams:
        assert len(cs.data) > fs.HEADERLESS_TABLE_WINDOWS * fs.W
        msgs = fs.whole_stream(cs.data)[0]
        start, packed, framed = msgs[cs.n_prefix]
        assert start == cs.prefix_len and framed == 8 * 70000
        end = start + packed
        last_start = start + rs._record_starts(cs.data[start:end])[-1][0]
        at = {"ends_on_grid": end, "ends_1_past_grid": end - 1,
              "last_record_starts_1_before_grid": last_start + 1, "last_record_starts_on_grid": last_start}[place]
        assert at % fs.W == 0 and last_start < end, (place, mode)
    sched = fs.window_exit_schedule()
    assert len(sched.rounds) == 1
    check_agreement(sched, [(i, cs) for i, (_, _, cs) in enumerate(streams)])


# ---------------------------------------------------------------------------
# The coverage table
# ---------------------------------------------------------------------------


def test_coverage_outcomes_and_modes_under_every_policy():
    for policy in fs.SMALL_POLICIES:
        share = [st for _, st in fs.small_share(policy)]
        n = collections.Counter(st.outcome for st in share)
        for kind in OUTCOMES:
            assert n[kind] >= 20, (policy, kind, n[kind])
        for kind in HEADER_ERRORS:
            assert n[kind] >= 5, (policy, kind, n[kind])
        modes = collections.Counter(st.mode for st in share)
        for mode in fs.MODES:
            assert modes[mode] >= 100, (policy, mode, modes[mode])


def read_ends(reads):
    return np.cumsum([len(x) for x in reads]).tolist()


def test_coverage_last_record_arrival_shapes():
    """Under last_record a read ends 9, 8 and 1 bytes before the end of the record that reaches
    or passes the framed length and at its end, where that cut lies inside the record (00 c: 2
    bytes; FF w c L: 10 + 8 c). By the bytes of the record held when the read ends:
    - "tag": the tag alone (00 | c; FF | w 00 of the 10-byte literal record);
    - "tag_part_word": FF and 1-7 bytes of its word;
    - "tag_word": FF and its word, the count not there yet; for the 10-byte record this is
      "no_count", everything but the count;
    - "no_last_byte": a run of c >= 1 words short of its last byte; "run_cut9" / "run_cut8": short
      of its last 9 / 8 bytes;
    - "whole", with bytes after it in the stream ("whole_then_more") or as its last
      ("whole_at_end").
    The 10-byte record FF w 00 (lit_count0_streams) comes in all three modes."""
    shapes = collections.Counter()
    count0_modes = set()
    for i, st, reads in fs.stream_reads(fs.small_share("last_record"), fs.cut_last_record,
                                        fs.small_seed("last_record")):
        if st.kind not in ("zero", "lit") or st.family == "random":
            continue
        ends = set(read_ends(reads))
        term = st.data[st.prefix_len:]
        rel = st.rend - st.prefix_len
        if st.kind == "zero":
            rec_len = 2
        else:  # the count byte is 8 c + 1 bytes before the end: find c by its own value
            rec_len = next(10 + 8 * c for c in range(256)
                           if rel - 10 - 8 * c >= 0 and rel - 8 * c - 1 < len(term)
                           and term[rel - 10 - 8 * c] == 0xFF and term[rel - 8 * c - 1] == c)
        assert (rec_len == 10) == (st.family == "lit_count0") or st.kind == "zero", (i, st.family, rec_len)
        for d in fs.LAST_RECORD_CUTS:
            if d >= rec_len or st.rend - d not in ends:
                continue
            held = rec_len - d
            if d == 0:
                shapes[st.kind, "whole"] += 1
                shapes[st.kind, "whole_then_more" if st.rend < len(st.data) else "whole_at_end"] += 1
            elif held == 1:
                shapes[st.kind, "tag"] += 1
                if st.kind == "lit":
                    count0_modes.add(st.mode)
            elif held < 9:
                shapes["lit", "tag_part_word"] += 1
            elif held == 9:
                shapes["lit", "tag_word"] += 1
                shapes["lit", "no_count"] += rec_len == 10
            else:
                shapes["lit", {1: "no_last_byte", 8: "run_cut8", 9: "run_cut9"}[d]] += 1
    for cell in (("zero", "tag"), ("zero", "whole"), ("zero", "whole_then_more"), ("zero", "whole_at_end"),
                 ("lit", "tag"), ("lit", "tag_part_word"), ("lit", "tag_word"), ("lit", "no_count"),
                 ("lit", "no_last_byte"), ("lit", "run_cut8"), ("lit", "run_cut9"),
                 ("lit", "whole"), ("lit", "whole_then_more"), ("lit", "whole_at_end")):
        assert shapes[cell] >= 10, (cell, shapes)
    assert count0_modes == set(fs.MODES)


def test_coverage_bytewise_header_cuts_inside_the_table():
    inside = big = 0
    for i, st, reads in fs.stream_reads(fs.small_share("bytewise_header"), fs.cut_bytewise_header,
                                        fs.small_seed("bytewise_header")):
        if st.hdr_end is None or not any(0 < e < st.hdr_end for e in read_ends(reads)):
            continue
        inside += 1
        big += st.hdr_segs >= 64
    assert inside >= 100 and big >= 20, (inside, big)


def test_coverage_errors_after_a_resume():
    """Streams that end in an error met in a later read than the one that delivered the failing
    message's first byte, and those of them whose failing message is not the connection's first."""
    later = later_not_first = 0
    for policy, cut in fs.SMALL_POLICIES.items():
        for i, st, reads in fs.stream_reads(fs.small_share(policy), cut, fs.small_seed(policy)):
            if st.err_at is None:
                continue
            ends = read_ends(reads)
            assert ends[-1] >= st.err_at and (len(ends) == 1 or ends[-2] < st.err_at)
            first_byte_read = next(k for k, e in enumerate(ends) if e > st.stop_at)
            if first_byte_read < len(ends) - 1:
                later += 1
                later_not_first += st.stop_at > 0
    assert later >= 300 and later_not_first >= 300, (later, later_not_first)


def packed_words(held):
    """Words the whole records of `held` decode to (the walk counts complete records only)."""
    r, n, words = 0, len(held), 0
    while r < n:
        t = held[r]
        if t == 0:
            size, w = 2, 1 + (held[r + 1] if r + 1 < n else 0)
        elif t == 0xFF:
            size, w = 10 + 8 * (held[r + 9] if r + 9 < n else 0), 1 + (held[r + 9] if r + 9 < n else 0)
        else:
            size, w = 1 + bin(t).count("1"), 1
        if r + size > n:
            break
        words += w
        r += size
    return words


def test_coverage_large_family_table_rules():
    """framer_read_locked builds window tables for a connection whose header is not decoded when
    its held bytes span over 64 windows, and for one whose header is known when more than two
    windows of framed bytes are left and its unwalked bytes span over a window. Both from the
    model: a first read of a fresh slot over 64 W; a read of over W bytes onto held bytes (at most
    two windows of them, so that their words are cheap to count here) that decode the header and
    leave more than 2 W framed bytes."""
    infos = [info for info, _ in fs.large_streams()]
    assert len(infos) == 120
    for attr, want in (("words", fs.LARGE_WORDS), ("density", fs.LARGE_DENSITIES), ("mode", fs.MODES),
                       ("segs", fs.LARGE_SEGMENTS), ("ending", fs.LARGE_ENDINGS), ("front", (None, "small", "large"))):
        assert {getattr(i, attr) for i in infos} == set(want), attr
    # every mode meets every segment count, and an error terminal stands behind a large message
    assert {(i.mode, i.segs) for i in infos} == {(m, s) for m in fs.MODES for s in fs.LARGE_SEGMENTS}
    errors = [st for info, st in fs.large_streams() if info.front == "large" and st.err_at is not None]
    assert len(errors) >= 20

    headerless = 0
    for i, st, reads in fs.stream_reads(fs.large_share(), fs.cut_whole, fs.large_seed("whole")):
        headerless += len(reads) == 1 and len(reads[0]) > fs.HEADERLESS_TABLE_WINDOWS * fs.W
    assert headerless >= 6, headerless
    literal_70k = fs.large_share(lambda info: info.words == 70000 and info.density == "literal")
    assert len(literal_70k) == 15 and all(len(st.data) > 64 * fs.W for _, st in literal_70k)

    known = collections.Counter()
    for policy in fs.LARGE_POLICIES:
        sched = fs.large_schedule(policy)
        sess = fs.ModelSession(sched.n_slots)
        for resets, starts, reads in sched.rounds:
            for c in resets:
                sess.reset(c)
            for c, d in reads.items():
                held = sess.buf[c]
                if len(d) > fs.W and 0 < len(held) <= 2 * fs.W and sess.expected(c):
                    known[policy] += sess.expected(c) - 8 * packed_words(held) > 2 * fs.W
            sess.read(reads)
    assert sum(known.values()) >= 30 and known["header_then_rest"] >= 30, known
