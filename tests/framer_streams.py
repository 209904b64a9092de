"""Connection streams, cut policies and slot schedules for the framer-session fuzz: what
tests/test_framer_streams.py checks on the CPU and tests/test_gpu_framer_fuzz.py replays through
a real capnp_packed_framer beside the model. No GPU and no torch here.

The property. However a connection's stream is cut into reads, after every read the frames
popped, the status, the bytes held and expected_total equal what Reader.readPackedMessage
(reader.zig:84-156) gives on the bytes delivered so far, message after message, as
Connection.handleRead loops (connection.zig:153-203). ModelSession states that with the C oracle;
reader_streams.read_message states it a second time in the CPU test.

The streams are reader_streams' corpus around the framed-length cut (hand-built records, the
Zig-rule packer, the C++-dialect packer), each stream behind 0-3 whole messages, and a family of
messages of 4-126 walk windows built with the same base_endings.
"""
import collections
import ctypes
import functools

import numpy as np

import oracle
import reader_streams as rs

# include/capnp_packed.h's statuses (tests/test_framer_streams.py compares them with the binding's)
ABI_OK = 0
ABI = {rs.END_OF_STREAM: 8, rs.INVALID_SEGMENT_COUNT: 9, rs.SEGMENT_COUNT_LIMIT_EXCEEDED: 10,
       rs.MESSAGE_TOO_LARGE: 11, rs.INVALID_PACKED_MESSAGE: 12}
ABI_END_OF_STREAM = ABI[rs.END_OF_STREAM]
ORACLE_TO_ABI = {0: ABI_OK, -1: 8, -2: 9, -3: 10, -6: 11, -7: 12}

# The walk's window: kWvWin of csrc/kernels/decode_wave.h (64 chunks of 72 packed bytes), which the
# library reports as cpk::framer_window_bytes() and framer_read_locked compares spans with.
W = 4608
HEADERLESS_TABLE_WINDOWS = 64  # framer_read_locked: header not decoded, held bytes over 64 windows
N_SLOTS = 192
SKIP = 0.15
SEED = 0xF7A3E001

_OUT_CAP = 8 * (rs.MAX_TOTAL_WORDS + 520)


class _Out:
    """The oracle's output buffer, kept between calls (a fresh one is zero-filled every time)."""
    buf = None
    cap = 0

    @classmethod
    def get(cls, cap):
        if cls.cap < cap:
            cls.buf = ctypes.create_string_buffer(cap)
            cls.cap = cap
        return cls.buf


def oracle_read_at(held, pos=0):
    """oracle.read_packed_message on held[pos:] (a bytearray, read in place): (code, framed,
    consumed). The output buffer grows to the 8 Mi-word limit (framing.zig:5) when it must."""
    n = len(held) - pos
    if n <= 0:
        return -1, b"", 0
    src = (ctypes.c_ubyte * len(held)).from_buffer(held)
    try:
        cap = max(_Out.cap, 1 << 20)
        while True:
            dst = _Out.get(cap)
            ln, used = ctypes.c_size_t(), ctypes.c_size_t()
            rc = oracle.lib().oracle_read_packed_message(ctypes.addressof(src) + pos, n, dst, cap, ctypes.byref(ln),
                                                         ctypes.byref(used))
            if rc != -8 or cap >= _OUT_CAP:
                return rc, ctypes.string_at(dst, ln.value), used.value
            cap = min(_OUT_CAP, 8 * cap)
    finally:
        del src  # releases the bytearray for resizing


class ModelSession:
    """capnp_packed_framer_* restated on the oracle reader (include/capnp_packed.h's contract):
    read() appends and pops every whole message; an error is reported once, in the read that
    meets it, and drops the connection's bytes; END_OF_STREAM otherwise."""

    def __init__(self, n_conns):
        self.n = n_conns
        self.buf = [bytearray() for _ in range(n_conns)]
        self.calls = 0
        self.fed = 0  # bytes given to read()
        self._expected = [0] * n_conns

    def read(self, reads):
        self.calls += 1
        frames, status = {}, np.full(self.n, ABI_END_OF_STREAM, dtype=np.int32)
        for c, d in reads.items():
            if not len(d):
                continue  # nothing new: what is held stays short of a message
            held = self.buf[c]
            held += d
            self.fed += len(d)
            self._expected[c] = None
            pos = 0
            while pos < len(held):
                rc, framed, used = oracle_read_at(held, pos)
                rc = ORACLE_TO_ABI[rc]
                if rc == ABI_END_OF_STREAM:
                    break
                if rc != ABI_OK:
                    status[c] = rc
                    pos = len(held)  # the session drops a failed connection's bytes
                    break
                frames.setdefault(c, []).append(memoryview(framed))
                pos += used
            del held[:pos]
        return frames, status

    def buffered(self, c):
        return len(self.buf[c])

    def expected(self, c):
        """Framer.expected_total: 8 x the framed words once the held bytes decode the header."""
        if self._expected[c] is None:
            h = rs.read_message(self.buf[c], header_only=True)
            self._expected[c] = 8 * h.fw if h.status is None else 0
        return self._expected[c]

    def reset(self, c):
        self.buf[c] = bytearray()
        self._expected[c] = 0


def whole_stream(data):
    """The whole-stream loop over `data`: ((start, packed bytes, framed bytes) per whole message,
    bytes left, final ABI status (OK: every byte consumed), and for an error the stream byte at
    which the reader returned it: it reads in order, so it returns the error as soon as the bytes
    before that one are there, and EndOfStream on any shorter prefix of the message)."""
    held = bytearray(data)
    pos, msgs = 0, []
    while pos < len(held):
        rc, framed, used = oracle_read_at(held, pos)
        if rc != 0:
            return msgs, len(held) - pos, ORACLE_TO_ABI[rc], None if rc == -1 else pos + used
        msgs.append((pos, used, len(framed)))
        pos += used
    return msgs, 0, ABI_OK, None


def oracle_frames(data):
    """The same loop through oracle.read_packed_message on copies of the bytes left, as
    tests/test_gpu_framer.py states it: (frames, rest, ABI status, OK when nothing is left)."""
    frames = []
    while data:
        rc, framed, used = oracle.read_packed_message(data, cap=1 << 20)
        if rc == -8:
            rc, framed, used = oracle.read_packed_message(data, cap=_OUT_CAP)
        if rc != 0:
            return frames, data, ORACLE_TO_ABI[rc]
        frames.append(framed)
        data = data[used:]
    return frames, data, ABI_OK


# ---------------------------------------------------------------------------
# Connection streams
# ---------------------------------------------------------------------------

# data: the connection's bytes. n_prefix / prefix_len: the whole messages in front of the terminal
# corpus case. family / kind / mode: the terminal's; rend: its, shifted by prefix_len (a terminal
# the generator gave none: where the reader stopped in it). outcome: reader_streams.outcome or the
# header error's name. hdr_end / hdr_segs: the packed end of the record that completes the first
# message's segment table and its segment count (None: the stream never gets there).
# status: the final ABI status of the whole-stream loop (OK: all consumed), err_at: the stream
# byte whose arrival lets the reader reach its error (None: no error), n_msgs: whole messages,
# max_frame: the largest framed length among them, stop_at: where the message starts that the loop
# stopped in (the stream's length when all was consumed). forced: cuts every policy must make.
ConnStream = collections.namedtuple(
    "ConnStream", "data n_prefix prefix_len family kind mode rend outcome hdr_end hdr_segs status err_at n_msgs "
                  "max_frame stop_at forced")


def _conn_stream(prefix_msgs, term, forced=()):
    prefix = b"".join(prefix_msgs)
    data = prefix + term.data
    msgs, left, status, err_at = whole_stream(data)
    h = rs.read_message(data, header_only=True)
    hdr_end, hdr_segs = None, None
    if h.status is None:
        hdr_end = h.consumed
        hdr_segs = int.from_bytes(_first_word(data), "little") + 1
    rend = term.rend if term.rend is not None else term.consumed
    outcome = rs.outcome(term) or (term.status if term.status in (
        rs.INVALID_SEGMENT_COUNT, rs.SEGMENT_COUNT_LIMIT_EXCEEDED, rs.MESSAGE_TOO_LARGE) else None)
    return ConnStream(data, len(prefix_msgs), len(prefix), term.family, term.kind, term.mode, len(prefix) + rend,
                      outcome, hdr_end, hdr_segs, status, err_at, len(msgs),
                      max((m[2] for m in msgs), default=0), len(data) - left, tuple(len(prefix) + f for f in forced))


def _first_word(head):
    """The first four decoded bytes of a stream whose first record is whole."""
    out = bytearray()
    r = 0
    while len(out) < 4:
        t = head[r]
        r += 1
        if t == 0:
            out += bytes(8)
            r += 1
        elif t == 0xFF:
            out += head[r:r + 8]
            r += 9 + 8 * head[r + 8]
        else:
            w = bytearray(8)
            for k in range(8):
                if t >> k & 1:
                    w[k] = head[r]
                    r += 1
            out += w
    return bytes(out[:4])


MODES = ("hand", "zig", "cxx")


@functools.lru_cache(maxsize=1)
def connection_streams(seed=SEED):
    """Every corpus case once as the terminal of a connection, behind 0-3 whole messages
    (case.data[:case.consumed] of OK cases, the modes in turn). The corpus holds 6 streams per
    header error, one per policy: 5 more sets of reader_streams' header-error streams follow, so
    that each policy's fifth meets each of the three at least 5 times. Every literal run the
    corpus ends a message with has a count of at least 1: lit_count0_streams follow, whose last
    record is FF w 00."""
    rng = np.random.default_rng(seed)
    cases = rs.cases(rs.SEED)
    pool = {m: [c.data[:c.consumed] for c in cases if c.status == rs.OK and c.mode == m] for m in MODES}
    out = []
    for i, c in enumerate(cases):
        k = int(rng.integers(0, 4))
        prefix = []
        for j in range(k):
            msgs = pool[MODES[(i + j) % 3]]
            prefix.append(msgs[int(rng.integers(0, len(msgs)))])
        out.append(_conn_stream(prefix, c))
    nexts = rs._small_messages(rng)
    for _ in range(5):
        for s in rs._header_error_streams(rng, nexts):
            status, framed, used = rs.oracle_read(s.data)
            prefix = [pool[MODES[len(out) % 3]][int(rng.integers(0, 50))] for _ in range(int(rng.integers(0, 4)))]
            out.append(_conn_stream(prefix, rs.Case(s.data, s.family, s.kind, s.rend, status, framed, used, None,
                                                    False, s.mode)))
    for s in lit_count0_streams(rng, nexts):
        status, framed, used = rs.oracle_read(s.data)
        h = rs.read_message(s.data, header_only=True)
        prefix = [pool[MODES[len(out) % 3]][int(rng.integers(0, 50))] for _ in range(int(rng.integers(0, 4)))]
        out.append(_conn_stream(prefix, rs.Case(s.data, s.family, s.kind, s.rend, status, framed, used, h.fw,
                                                h.spans, s.mode)))
    return out


N_LIT_COUNT0 = 2  # passes over reader_streams' base specs


def lit_count0_streams(rng, nexts):
    """Messages whose last record is FF w 00, a literal word with an empty run, reaching the
    framed length exactly (family "lit_count0", kind "lit", rend at its end): the 10-byte record
    can arrive as its tag alone, tag and word without the count, and whole. A C++-dialect packer
    writes it for a word it would not start a run with; w holds zero bytes in two of three. Then
    nothing, the next message, or 1-7 bytes."""
    out = []
    for rep_ in range(N_LIT_COUNT0):
        for bi, (fw, nseg, density, mode) in enumerate(rs._base_specs(rng)):
            if fw - (nseg // 2 + 1) < 1:
                continue  # a table-only message: no body word to replace
            p = rs._build_base(rng, fw, nseg, density, mode)(1)
            w = bytearray(rs._nonzero(rng, 8))
            if bi % 3:
                w[int(rng.integers(0, 8))] = 0
                w[int(rng.integers(0, 8))] = 0
            tail = (b"", nexts[bi % len(nexts)], rs._rand(rng, 1 + bi % 7))[(bi + rep_) % 3]
            out.append(rs.Stream(p + b"\xff" + bytes(w) + b"\x00" + tail, "lit_count0", "lit", len(p) + 10, mode))
    return out


# ---------------------------------------------------------------------------
# Cut policies: the reads one stream arrives in
# ---------------------------------------------------------------------------

def _reads(st, cuts):
    """st.data cut at `cuts` and st.forced; reads past the one that meets the error are dropped
    (the session has dropped the connection's bytes, as Connection.handleRead closes it)."""
    n = len(st.data)
    edges = sorted({int(x) for x in cuts if 0 < x < n} | {f for f in st.forced if 0 < f < n})
    out = []
    prev = 0
    for e in edges + [n]:
        if e > prev:
            out.append(st.data[prev:e])
        prev = e
        if st.err_at is not None and e >= st.err_at:
            break
    return out


def cut_whole(st, rng):
    return _reads(st, [])


def cut_random(st, rng):
    return _reads(st, rng.integers(0, len(st.data) + 1, int(rng.integers(1, 13))))


def cut_bytewise_header(st, rng):
    """A byte per read to two bytes past the first message's header record, then 1-3 cuts."""
    n = len(st.data)
    upto = min(n, (st.hdr_end if st.hdr_end is not None else min(n, 24)) + 2)
    later = rng.integers(upto, n + 1, int(rng.integers(1, 4))) if n > upto else []
    return _reads(st, list(range(1, upto + 1)) + list(later))


LAST_RECORD_CUTS = (9, 8, 1, 0)  # bytes before rend


def cut_last_record(st, rng):
    """Cuts 9, 8 and 1 bytes before the end of the record that reaches or passes the framed length
    and at its end, and one cut before them."""
    cuts = [st.rend - d for d in LAST_RECORD_CUTS if 0 < st.rend - d < len(st.data)]
    first = min(cuts, default=len(st.data))
    if first > 1:
        cuts.append(int(rng.integers(1, first)))
    return _reads(st, cuts)


def cut_trickle(st, rng):
    """Reads of 1-7 bytes over the first 200 bytes, then of up to 1 KiB."""
    cuts, pos, n = [], 0, len(st.data)
    while pos < n:
        pos += int(rng.integers(1, 8)) if pos < 200 else int(rng.integers(1, 1025))
        cuts.append(pos)
    return _reads(st, cuts)


SMALL_POLICIES = {"whole": cut_whole, "random": cut_random, "bytewise_header": cut_bytewise_header,
                  "last_record": cut_last_record, "trickle": cut_trickle}


def cut_header_then_rest(st, rng):
    return _reads(st, [16])


def cut_reads_64k(st, rng):
    return _reads(st, range(65536, len(st.data), 65536))


def cut_reads_5k(st, rng):
    """Every read spans a window and a ninth."""
    return _reads(st, range(5120, len(st.data), 5120))


WINDOW_EDGE_DELTAS = (-10, -9, -1, 0, 1, 9, 10)


def cut_window_edges(st, rng):
    """Cuts at k W + d from the previous cut: tags, count bytes and literal words then straddle the
    walk's window grid, which starts where the previous read's walk stopped."""
    cuts, pos, i = [], 0, int(rng.integers(0, 7))
    while pos < len(st.data):
        pos += int(rng.integers(1, 4)) * W + WINDOW_EDGE_DELTAS[i % 7]
        cuts.append(pos)
        i += 1
    return _reads(st, cuts)


LARGE_POLICIES = {"whole": cut_whole, "header_then_rest": cut_header_then_rest, "reads_64k": cut_reads_64k,
                  "reads_5k": cut_reads_5k, "window_edges": cut_window_edges}


# ---------------------------------------------------------------------------
# Slot schedule
# ---------------------------------------------------------------------------

# rounds: per round (resets, starts, reads): the slots to reset first, {slot: stream index} for
# the streams that begin in this round, {slot: bytes} for the round's read. fed: the bytes of all
# reads. last: {stream index: (round, slot)} of each stream's last read.
Schedule = collections.namedtuple("Schedule", "n_slots rounds fed last")


def stream_reads(streams, policy, seed):
    """[(index, stream, reads)] of a list of (index, ConnStream) under a cut policy."""
    rng = np.random.default_rng(seed)
    return [(i, st, policy(st, rng)) for i, st in streams]


def schedule(streams, policy, seed, n_slots=N_SLOTS, skip=SKIP):
    """The streams (a list of (index, ConnStream)) through `n_slots` connections: every live slot
    gets its next read each round, a seeded `skip` of them sit the round out; a slot whose stream
    is used up or failed takes the next one in the following round, after a reset when the stream
    ended with bytes held. Streams with the most reads start first, so the last rounds are not
    one slot's."""
    rng = np.random.default_rng(seed ^ 0x5C4ED)
    queue = [q for q in stream_reads(streams, policy, seed) if q[2]]  # an empty stream has no reads
    queue.sort(key=lambda q: -len(q[2]))
    queue.reverse()  # pop() from the end
    live = [None] * n_slots  # [index, stream, reads, next read]
    dirty = [False] * n_slots
    rounds, fed, last = [], 0, {}
    while queue or any(live):
        resets, starts, reads = [], {}, {}
        for c in range(n_slots):
            if live[c] is None and queue:
                i, st, rd = queue.pop()
                live[c] = [i, st, rd, 0]
                starts[c] = i
                if dirty[c]:
                    resets.append(c)
                    dirty[c] = False
        skipped = rng.random(n_slots) < skip
        for c in range(n_slots):
            if live[c] is None or skipped[c]:
                continue
            i, st, rd, k = live[c]
            reads[c] = rd[k]
            fed += len(rd[k])
            live[c][3] = k + 1
            if k + 1 == len(rd):
                last[i] = (len(rounds), c)
                # held bytes stay behind unless the stream failed or was consumed whole
                dirty[c] = st.status == ABI_END_OF_STREAM
                live[c] = None
        rounds.append((resets, starts, reads))
    return Schedule(n_slots, rounds, fed, last)


def small_share(policy_name):
    """Every fifth connection stream, at the policy's own phase: the five policies cover the
    corpus once."""
    phase = list(SMALL_POLICIES).index(policy_name)
    return [(i, st) for i, st in enumerate(connection_streams()) if i % 5 == phase]


def small_seed(policy_name):
    return SEED + list(SMALL_POLICIES).index(policy_name)


def small_schedule(policy_name, share=None):
    share = small_share(policy_name) if share is None else share
    return schedule(share, SMALL_POLICIES[policy_name], small_seed(policy_name))


# ---------------------------------------------------------------------------
# Long-lived connections: a region used over and over before the terminal
# ---------------------------------------------------------------------------

LONG_LIVED_SLOTS = 64


@functools.lru_cache(maxsize=1)
def long_lived_streams(seed=SEED):
    """Every 20th corpus case behind 30-60 whole messages of at most 4 KiB (50-140 KB a stream): in
    reads of up to 4 KiB a connection passes the end of its 64-KiB region with part of a message
    held, so the held bytes slide to the region's start or move to a larger region before the
    terminal's error or cut arrives."""
    rng = np.random.default_rng(seed + 25)
    cases = rs.cases(rs.SEED)
    pool = [c.data[:c.consumed] for c in cases if c.status == rs.OK and c.mode in MODES and 256 <= c.consumed <= 4096]
    out = []
    for c in cases[3::20]:
        k = int(rng.integers(30, 61))
        out.append(_conn_stream([pool[int(rng.integers(0, len(pool)))] for _ in range(k)], c))
    return out


def cut_reads_4k(st, rng):
    cuts, pos = [], 0
    while pos < len(st.data):
        pos += int(rng.integers(1, 4097))
        cuts.append(pos)
    return _reads(st, cuts)


def long_lived_schedule():
    return schedule(list(enumerate(long_lived_streams())), cut_reads_4k, SEED + 50, n_slots=LONG_LIVED_SLOTS)


# ---------------------------------------------------------------------------
# The large family: messages of 4 to 126 windows
# ---------------------------------------------------------------------------

LARGE_WORDS = (2500, 6000, 20000, 70000)
LARGE_DENSITIES = ("literal", "mixed")
LARGE_SEGMENTS = (1, 3, 64)
LARGE_ENDINGS = ("exact_next", "zero_over", "lit_over", "lit_cut_completed", "trunc")

# words / density / mode / segs of the base, ending as LARGE_ENDINGS, front: None / "small" / "large"
LargeInfo = collections.namedtuple("LargeInfo", "words density mode segs ending front")


@functools.lru_cache(maxsize=1)
def large_streams(seed=SEED):
    """[(LargeInfo, ConnStream)]: per base (framed words x density x mode, the segment counts in
    turn) one stream per ending, picked from reader_streams.base_endings: the message exact with
    the next one behind it, a zero run and a literal run past the framed length, that literal run
    cut by a read boundary and completed by the next read, and the message one byte short. A third
    of them stand behind 3-8 small whole messages, and another third (error terminals among them)
    behind a large whole message."""
    rng = np.random.default_rng(seed)
    nexts = rs._small_messages(rng)
    small = [c.data[:c.consumed] for c in rs.cases(rs.SEED) if c.status == rs.OK and 0 < c.consumed <= 1200]

    def trailing(j, nbytes):
        return rs._rand(rng, nbytes) if nbytes > 0 else b""

    picked = []
    exacts = []
    bi = 0
    for fw in LARGE_WORDS:
        for density in LARGE_DENSITIES:
            for mode in MODES:
                nseg = LARGE_SEGMENTS[(bi + bi // 3) % 3]
                prefix = rs._build_base(rng, fw, nseg, density, mode)
                ends = rs.base_endings(rng, bi, fw, nseg, prefix, trailing, nexts, mode)
                by = collections.defaultdict(list)
                for s in ends:
                    by[s.family].append(s)
                exact_next = by["exact"][5]  # the message, the next message, 0-4 bytes
                exact_len = len(by["exact"][0].data)  # no trailing bytes
                exacts.append(by["exact"][0].data)
                lit_over = by["lit_over"][bi % len(by["lit_over"])]
                lit_cut = by["lit_cut"][(bi * 5) % len(by["lit_cut"])]
                chosen = {
                    "exact_next": (exact_next, ()),
                    "zero_over": (by["zero_over"][(bi * 7) % len(by["zero_over"])], ()),
                    "lit_over": (lit_over, ()),
                    # the run cut where the lit_cut stream ends, its rest in a later read
                    "lit_cut_completed": (by["lit_over"][-1], (len(lit_cut.data),)),
                    "trunc": (next(s for s in by["trunc"] if len(s.data) == exact_len - 1), ()),
                }
                for ending in LARGE_ENDINGS:
                    s, forced = chosen[ending]
                    picked.append((LargeInfo(fw, density, mode, nseg, ending, None), s, forced))
                bi += 1
    out = []
    for idx, (info, s, forced) in enumerate(picked):
        rc, framed, used = oracle_read_at(bytearray(s.data))
        status = rs.ORACLE_NAME[rc]
        h = rs.read_message(s.data, header_only=True)
        term = rs.Case(s.data, s.family, s.kind, s.rend, status, framed, used, h.fw, h.spans, s.mode)
        front, prefix = None, []
        if idx % 3 == 0:
            front = "small"
            prefix = [small[int(rng.integers(0, len(small)))] for _ in range(int(rng.integers(3, 9)))]
        elif idx % 3 == 1:  # three in five of them error terminals
            front = "large"
            prefix = [exacts[(idx * 5 + 1) % len(exacts)]]
        out.append((info._replace(front=front), _conn_stream(prefix, term, forced)))
    return out


WINDOW_EXIT_PLACES = ("ends_on_grid", "ends_1_past_grid", "last_record_starts_1_before_grid",
                      "last_record_starts_on_grid")


@functools.lru_cache(maxsize=1)
def window_exit_streams(seed=SEED):
    """[(place, mode, ConnStream)]: the 70,000-word literal messages (over 64 windows: a fresh
    slot that gets one whole builds tables) behind small whole messages whose lengths put the large
    message's last record against the walk's window grid, which starts at the connection's first
    held byte: the message ends on a grid line (the next one starts a window) or a byte past it,
    or its last record starts a byte before a grid line (it is the last record of its window: the
    message ends at the window's exit, where a lookup's word count equals the words left) or on
    it (the first record of the next window)."""
    rng = np.random.default_rng(seed + 7)
    small = [c.data[:c.consumed] for c in rs.cases(rs.SEED) if c.status == rs.OK and 0 < c.consumed < W]
    by_len = {len(m): m for m in small}
    out = []
    for info, st in large_streams(seed):
        if not (info.ending == "exact_next" and info.words == 70000 and info.density == "literal"):
            continue
        data = st.data[st.prefix_len:]
        end = whole_stream(data)[0][0][1]  # the large message's packed length
        last = end - rs._record_starts(data[:end])[-1][0]
        rc, framed, used = oracle_read_at(bytearray(data))
        term = rs.Case(data, "exact", None, None, rs.ORACLE_NAME[rc], framed, used, info.words, False, info.mode)
        for place, r in zip(WINDOW_EXIT_PLACES, (0, 1, last - 1, last)):
            while True:  # two random messages, then two whose lengths bring the end to the place
                pads = [small[int(rng.integers(0, len(small)))] for _ in range(2)]
                target = (r - end - sum(len(m) for m in pads)) % W
                pair = next(((a, target - a) for a in sorted(by_len) if (target - a) in by_len), None)
                if pair:
                    break
            pads += [by_len[pair[0]], by_len[pair[1]]]
            cs = _conn_stream(pads, term)
            assert (cs.prefix_len + end - r) % W == 0
            out.append((place, info.mode, cs))
    return out


def window_exit_schedule():
    """A slot per window_exit_streams stream, each delivered whole in one read."""
    streams = [(i, cs) for i, (place, mode, cs) in enumerate(window_exit_streams())]
    return schedule(streams, cut_whole, SEED + 40, n_slots=len(streams), skip=0.0)


def large_seed(policy_name):
    return SEED + 16 + list(LARGE_POLICIES).index(policy_name)


def large_share(only=None):
    return [(i, st) for i, (info, st) in enumerate(large_streams()) if only is None or only(info)]


def large_schedule(policy_name, only=None):
    """A slot per large stream (`only`: a filter on LargeInfo), no round skipped before a stream's
    first read, so `whole` delivers each stream in the session's first read of it."""
    streams = large_share(only)
    return schedule(streams, LARGE_POLICIES[policy_name], large_seed(policy_name),
                    n_slots=len(streams), skip=0.0 if policy_name == "whole" else SKIP)


# ---------------------------------------------------------------------------
# Replay
# ---------------------------------------------------------------------------

def replay(sched, sessions, check):
    """Drive every session of `sessions` with the schedule: check(round index, reads, results)
    after each round, results being each session's (frames, status) of the round's read."""
    for r, (resets, starts, reads) in enumerate(sched.rounds):
        for sess in sessions:
            for c in resets:
                sess.reset(c)
        check(r, reads, [sess.read(reads) for sess in sessions])
