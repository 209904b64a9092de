"""Adversarial and segment-edge inputs for the fused message encoders
(capnp_packed_encode_message_batch / _dialect: encode_message_kernel<WRITE, TILED> under the
default dialect, encode_message_cxx_kernel under the C++ one), with the
references' verdict on each message. CPU only: numpy, `oracle`, `pyref`, `pyref_cxx`;
tests/test_message_streams.py judges these inputs on the CPU and
tests/test_gpu_message_adversarial.py feeds them to the device.

References: the default dialect's bytes are oracle.pack(pyref.frame(segs or [b""]))
(message.zig:2123-2179), the C++ dialect's pyref_cxx.pack_message(segs). Nothing the library
computes appears on the expected side.

Words are encode_streams' (A no zero byte, B one, C two, Z all zero). A batch is laid out as the
device sees it:
- one segment pool, POOL_PAD poison bytes at both ends, its base 256-B aligned; a segment entry
  is (offset into the pool, bytes). Every byte of the pool that is no segment's is part of a
  POISON word: non-zero, present in no message, so that a read of it changes the output.
- an empty segment of an end-to-end placement stands where the next segment starts (as in a
  MessageBuilder's arena); in every other placement its address is that of a poison word of the
  front pad (8-aligned, inside the pool, never null), a different one than its neighbour's.
- the segment arrays start and end with NPOISON poison entries (16 poison bytes each): a message
  with seg_count == 0 has its seg_first at one of them.
- output slots as encode_streams': a chosen `address & 15`, FRONT sentinel bytes before each slot
  and BACK after its capacity. Capacities depend on the dialect (a message's need does), so a
  batch carries one set of slots per dialect.
"""
import collections
import functools
import struct

import numpy as np

import oracle
import pyref
import pyref_cxx
from encode_streams import SENT, FRONT, BACK, PATTERNS, encode_bound, letters, random_words, spell, words  # noqa: F401

DIALECTS = ("zig", "cxx")
TILE = 512           # framed words per tile
ONE_SEGS = 64        # segments the one-tile pass takes (kMsgOneSegs)
MAX_SEGS = 512       # Message.max_segment_count
POOL_PAD = 64        # poison bytes at both ends of the pool
NPOISON = 3          # poison entries at both ends of the segment arrays
POISON = bytes((0xEE, 0x11, 0xDD, 0x22, 0xCC, 0x33, 0xBB, 0x44))
SEED = 0x5E6E5
SLACK = (0, 1, 16, 41)
ROUTES = ("e2e", "gather", "tiled", "arg")
PLACEMENTS = ("e2e0", "e2e8", "shuffle", "reverse", "adj_rev", "last_broken", "dedup")

# segs: tuple of bytes (seg_count = len(segs)); place: a PLACEMENTS name or ("same", j): the
# entries of message j of the batch; bad: None, ("len", s) / ("ptr", s): segment s listed with
# 4 more bytes / 4 bytes further, or ("count",): more than MAX_SEGS segments
Msg = collections.namedtuple("Msg", "segs kind place bad")
Exp = collections.namedtuple("Exp", "st need ref")
Slots = collections.namedtuple("Slots", "caps out_off out_end")
Batch = collections.namedtuple("Batch", "msgs entries routes pool seg_off seg_len first count exp slots")


def msg(segs, kind, place="e2e0", bad=None):
    return Msg(tuple(bytes(s) for s in segs), kind, place, bad)


def header_words(count):
    """toBytes 2135-2137: words of the segment table of `count` >= 1 segments."""
    return (1 + count + (0 if count % 2 else 1)) // 2


def frame_of(m):
    return pyref.frame(list(m.segs) or [b""])


def framed_words(m):
    return header_words(max(len(m.segs), 1)) + sum(len(s) for s in m.segs) // 8


# ---- the references ---------------------------------------------------------------------------

_REF = {}


def reference(segs, dialect):
    """The packed bytes of a valid message."""
    key = (dialect, segs)
    p = _REF.get(key)
    if p is None:
        if dialect == "zig":
            st, p = oracle.pack(pyref.frame(list(segs) or [b""]))
            assert st == oracle.OK
        else:
            assert dialect == "cxx"
            p = pyref_cxx.pack_message(list(segs))
        _REF[key] = p
    return p


def piecewise_zig(segs):
    """The table and every segment packed on their own under the Zig rule, concatenated: what an
    encoder that restarts its runs at a piece edge would write."""
    segs = list(segs) or [b""]
    return b"".join(oracle.pack(p)[1] for p in [pyref_cxx.segment_table(segs)] + segs)


# ---- routing, restated from the kernel --------------------------------------------------------

def route_of(count_in, entries):
    """The route of a message listed as `entries` [(address or pool offset, bytes)] (the pool's
    base is 256-B aligned, so an offset's low bits are the address's): encode_message_kernel's
    first pass (encode_message_tile1_body) and what it leaves to the tiled pass."""
    count = max(count_in, 1)
    if count > MAX_SEGS:
        return "arg"
    ent = list(entries) if count_in else [(0, 0)]
    if any(ln % 8 or ad % 8 for ad, ln in ent):
        return "arg"
    hw = header_words(count)
    if count > ONE_SEGS or any(ln // 8 > TILE for _, ln in ent) or hw + sum(ln for _, ln in ent) // 8 > TILE:
        return "tiled"
    if all(ent[s][0] + ent[s][1] == ent[s + 1][0] for s in range(count - 1)):
        return "e2e"
    return "gather"


def route(m, placement=None):
    """route_of a message laid out on its own under `placement` (default: its own)."""
    pool = _Pool()
    return route_of(len(m.segs), _listed(m, _place(pool, m.segs, placement or m.place, 0)))


# ---- layout -----------------------------------------------------------------------------------

class _Pool:
    def __init__(self):
        self.parts = [POISON * (POOL_PAD // 8)]
        self.pos = POOL_PAD

    def gap(self, nwords=1):
        at = self.pos
        self.parts.append(POISON * nwords)
        self.pos += 8 * nwords
        return at

    def align(self, phase):
        while self.pos % 16 != phase:
            self.gap()

    def put(self, data):
        at = self.pos
        assert len(data) % 8 == 0
        self.parts.append(data)
        self.pos += len(data)
        return at

    def bytes(self):
        buf = np.frombuffer(b"".join(self.parts) + POISON * (POOL_PAD // 8), dtype=np.uint8).copy()
        assert buf.size == self.pos + POOL_PAD
        return buf


def _empty_at(k, s):
    """The address of empty segment s of message k outside the end-to-end placements: a poison
    word of the front pad, another one than segment s - 1's and s + 1's."""
    return 8 * (1 + (k + s) % 6)


def _place(pool, segs, placement, k):
    """Write the segments of message k into the pool; returns its entries [(offset, bytes)]."""
    n = len(segs)
    if placement in ("e2e0", "e2e8"):
        pool.align(8 if placement == "e2e8" else 0)
        ent = [(pool.put(s), len(s)) for s in segs]
        pool.gap()
        return ent
    if placement == "last_broken":  # end to end but for the last link
        pool.align(8 * (k % 2))
        ent = [(pool.put(s), len(s)) for s in segs[:-1]]
        pool.gap()
        if n:
            ent.append((pool.put(segs[-1]), len(segs[-1])) if segs[-1] else (_empty_at(k, n - 1), 0))
        pool.gap()
        return ent
    if placement == "shuffle":
        order = np.random.default_rng(SEED + 7919 * k + n).permutation(n)
    else:
        assert placement in ("reverse", "adj_rev", "dedup"), placement
        order = range(n) if placement == "dedup" else range(n - 1, -1, -1)
    ent = [None] * n
    seen = {}
    for s in order:
        s = int(s)
        if not segs[s]:
            ent[s] = (_empty_at(k, s), 0)
        elif placement == "dedup" and segs[s] in seen:  # the same bytes listed twice
            ent[s] = seen[segs[s]]
        else:
            ent[s] = seen[segs[s]] = (pool.put(segs[s]), len(segs[s]))
            if placement != "adj_rev":
                pool.gap()  # 8 bytes between neighbours
    pool.gap()
    return ent


def _listed(m, ent):
    """The entries as the arrays list them: with the message's flaw."""
    ent = list(ent)
    if m.bad and m.bad[0] == "len":
        s = m.bad[1]
        ent[s] = (ent[s][0], ent[s][1] + 4)
    elif m.bad and m.bad[0] == "ptr":
        s = m.bad[1]
        ent[s] = (ent[s][0] + 4, ent[s][1])
    return ent


def resolve_cap(spec, need, framed_bytes):
    if spec[0] == "need":
        return max(need + spec[1], 0)
    if spec[0] == "bound":
        return encode_bound(framed_bytes)
    assert spec[0] == "abs"
    return spec[1]


def make_batch(items):
    """items: (Msg, capacity spec, slot `address & 15`); a capacity is ("need", k): the dialect's
    need + k, ("bound",): encode_bound of the framed bytes, or ("abs", c)."""
    pool = _Pool()
    msgs, entries, entries_raw, routes = [], [], [], []
    for k, (m, _, _) in enumerate(items):
        if isinstance(m.place, tuple):
            assert m.place[0] == "same" and msgs[m.place[1]].segs == m.segs
            raw = entries_raw[m.place[1]]
        else:
            raw = _place(pool, m.segs, m.place, k)
        entries_raw.append(raw)
        ent = _listed(m, raw)
        msgs.append(m)
        entries.append(ent)
        routes.append(route_of(len(m.segs), ent))
        assert (routes[-1] == "arg") == (m.bad is not None), (k, m.kind)
    buf = pool.bytes()
    poison_entry = (8, 16)
    flat = [poison_entry] * NPOISON
    first, count = [], []
    for k, (m, ent) in enumerate(zip(msgs, entries)):
        if not m.segs:  # seg_first at a poison entry, the front ones by turns with the back ones
            first.append(k % NPOISON if k % 2 else -1 - k % NPOISON)
        else:
            first.append(len(flat))
            flat.extend(ent)
        count.append(len(m.segs))
    flat.extend([poison_entry] * NPOISON)
    first = [len(flat) + f if f < 0 else f for f in first]
    for ad, ln in flat:
        assert ad % 4 == 0 and 8 <= ad and ad + ln + 8 <= buf.size  # inside the pool, never null
    exp, slots = {}, {}
    for d in DIALECTS:
        ex = []
        for m, r in zip(msgs, routes):
            if r == "arg":
                ex.append(Exp(oracle.INVALID_ARGUMENT, 0, b""))
            else:
                p = reference(m.segs, d)
                ex.append(Exp(oracle.OK, len(p), p))
        caps = [resolve_cap(spec, e.need, 8 * framed_words(m)) for (m, spec, _), e in zip(items, ex)]
        out_off = np.zeros(len(items), dtype=np.int64)
        o = 0
        for i, (_, _, phase) in enumerate(items):
            o += FRONT
            o += (int(phase) - o) % 16
            out_off[i] = o
            o += caps[i] + BACK
        exp[d] = ex
        slots[d] = Slots(caps, out_off, o)
    return Batch(msgs, entries, routes, buf, np.array([a for a, _ in flat], dtype=np.int64),
                 np.array([ln for _, ln in flat], dtype=np.int64), np.array(first, dtype=np.int32),
                 np.array(count, dtype=np.int32), exp, slots)


def output_bytes(b, dialect):
    return b.slots[dialect].out_end + FRONT


def outcome(e, cap):
    if e.st != oracle.OK:
        return e.st, 0
    if e.need > cap:
        return oracle.OUT_OF_SPACE, e.need
    return oracle.OK, e.need


def statuses(b, dialect):
    return {int(outcome(e, c)[0]) for e, c in zip(b.exp[dialect], b.slots[dialect].caps)}


def describe(b, i, dialect):
    m, sl = b.msgs[i], b.slots[dialect]
    return dict(msg=i, kind=m.kind, place=m.place, route=b.routes[i], segs=len(m.segs), framed_words=framed_words(m),
                cap=sl.caps[i], need=b.exp[dialect][i].need, slot_phase=int(sl.out_off[i]) & 15, dialect=dialect)


def check(b, out, out_len, status, dialect):
    """The contract of capnp_packed_encode_message_batch ("Output as in capnp_packed_encode_batch",
    include/capnp_packed.h) for one call (out: the output buffer after it, SENT before it; out None:
    the sizes-only call, which knows no slot: a valid message is OK with the reference's length).
      valid and fits     OK, the reference's length and bytes, [out_len, cap) still SENT;
      valid, too small   OUT_OF_SPACE, the reference's length, the slot's content unspecified;
      an arg message     INVALID_ARGUMENT, length 0, the slot untouched;
      always             nothing outside [slot, slot + cap) changes, and every status and out_len
                         entry has been written (whatever the arrays held: the expected values are
                         never negative and never the first pass's mark).
    Returns the set of statuses expected (and met)."""
    n = len(b.msgs)
    ex, sl = b.exp[dialect], b.slots[dialect]
    assert len(out_len) == n and len(status) == n
    want = [outcome(e, c) if out is not None else (e.st, e.need) for e, c in zip(ex, sl.caps)]
    wst = np.array([w[0] for w in want], dtype=np.int64)
    wln = np.array([w[1] for w in want], dtype=np.int64)
    st, ol = np.asarray(status).astype(np.int64), np.asarray(out_len).astype(np.int64)
    bad = np.flatnonzero(st != wst)
    assert bad.size == 0, ("status", int(bad.size), describe(b, int(bad[0]), dialect), int(st[bad[0]]),
                           int(wst[bad[0]]))
    bad = np.flatnonzero(ol != wln)
    assert bad.size == 0, ("out_len", int(bad.size), describe(b, int(bad[0]), dialect), int(ol[bad[0]]),
                           int(wln[bad[0]]))
    if out is not None:
        assert out.size == output_bytes(b, dialect)
        image = np.full(out.size, SENT, dtype=np.uint8)
        care = np.ones(out.size, dtype=bool)
        for i, (s, ln) in enumerate(want):
            o = int(sl.out_off[i])
            if s == oracle.OK:
                image[o:o + ln] = np.frombuffer(ex[i].ref, dtype=np.uint8)
            elif s == oracle.OUT_OF_SPACE:
                care[o:o + sl.caps[i]] = False
        wrong = np.flatnonzero((out != image) & care)
        if wrong.size:
            at = int(wrong[0])
            i = max(int(np.searchsorted(sl.out_off, at + FRONT, side="right")) - 1, 0)
            o = int(sl.out_off[i])
            where = ("before the slot" if at < o else "past cap" if at >= o + sl.caps[i] else
                     "in the packed bytes" if at < o + wln[i] else "in [out_len, cap)")
            raise AssertionError(("byte", int(wrong.size), describe(b, i, dialect), where, "slot offset", at - o,
                                  "got", int(out[at]), "want", int(image[at])))
    return {int(s) for s in wst}


def segment_table_of(b, i):
    """[(offset in the framed bytes, bytes)] of message i's segments: what Message.init finds."""
    m = b.msgs[i]
    segs = list(m.segs) or [b""]
    o = 8 * header_words(len(segs))
    tab = []
    for s in segs:
        tab.append((o, len(s)))
        o += len(s)
    return tab


# ---- builders -----------------------------------------------------------------------------------

def split(data, sizes):
    """The segments of `sizes` words each, cut from data."""
    assert 8 * sum(sizes) == len(data)
    out, o = [], 0
    for w in sizes:
        out.append(data[o:o + 8 * w])
        o += 8 * w
    return out


def _caps_turns(i):
    return ("bound",) if i % 5 == 4 else ("need", SLACK[i % 4])


def _items(msgs):
    return [(m, ("bound",) if m.bad else _caps_turns(i), (5 * i + 3) % 16) for i, m in enumerate(msgs)]


COUNTS = [0] + list(range(1, 67)) + [127, 128, 129, 255, 256, 257, 511, 512]
SIZE_CYCLES = ((1, 0, 2, 3), (0, 1, 1, 2), (3, 2, 0, 1), (2, 0, 0, 1))
LATTICE_PATTERNS = ("A", "B", "C", "Z", "ZA", "CAAAB", "AAZZ", "ZZZC")
LATTICE_PLACES = ("e2e0", "e2e8", "shuffle")


def lattice_messages():
    out = []
    for c in COUNTS:
        for v, cyc in enumerate(SIZE_CYCLES):
            sizes = [cyc[(k + c) % 4] for k in range(c)]
            name = LATTICE_PATTERNS[(c + 3 * v) % 8]
            segs = split(letters(PATTERNS[name](sum(sizes)), c + v), sizes)
            for place in LATTICE_PLACES:
                out.append(msg(segs, f"{c} segments sizes {v} {name}", place))
    return out


@functools.lru_cache(maxsize=None)
def count_lattice():
    """Counts 0 (seg_count 0), 1 .. 66, 127 .. 129, 255 .. 257, 511, 512, segments of 0 .. 3 words in
    four size cycles and eight A/B/C/Z patterns, each end to end at both base phases and gathered:
    every hw parity, every header-pair position, the 64-segment switch and the 512-segment limit
    (a table of 257 words)."""
    return make_batch(_items(lattice_messages()))


def empty_shapes(c):
    """(name, sizes) of c >= 2 segments with empty ones first, last, in a row, all, all but one."""
    base = [1 + k % 3 for k in range(c)]

    def zero(idx):
        return [0 if k in idx else w for k, w in enumerate(base)]

    mid = c // 2
    one = [0] * c
    one[(0, mid, c - 1)[c % 3]] = 2
    out = [("first", zero({0})), ("last", zero({c - 1})), ("all", [0] * c), ("all but one", one)]
    if c >= 3:
        out += [("two in a row", zero({mid - 1, mid})), ("first and last", zero({0, c - 1}))]
    if c >= 4:
        out += [("three first", zero({0, 1, 2})), ("three last", zero({c - 3, c - 2, c - 1}))]
    return out


EMPTY_TILED_COUNTS = (2, 3, 5, 8, 33, 63, 64)
EMPTY_MANY_COUNTS = (65, 66, 100)


@functools.lru_cache(maxsize=None)
def empty_edges():
    """Counts 2 .. 64 in the gathered route with empty segments first, last, two and more in a row,
    all empty (payload 0) and all empty but one; then such messages in the tiled route, reached by
    one more segment of 513 words or by 65 and more segments."""
    out = []
    for c in range(2, ONE_SEGS + 1):
        for j, (name, sizes) in enumerate(empty_shapes(c)):
            pat = LATTICE_PATTERNS[(c + j) % 8]
            segs = split(letters(PATTERNS[pat](sum(sizes)), c), sizes)
            out.append(msg(segs, f"{c} segments, empty {name}, {pat}", "shuffle"))
            if c in EMPTY_TILED_COUNTS:
                out.append(msg(segs + [letters("C" * 513, j)], f"{c} segments, empty {name}, {pat}, + 513 words",
                               "shuffle"))
    for c in EMPTY_MANY_COUNTS:
        for j, (name, sizes) in enumerate(empty_shapes(c)):
            pat = LATTICE_PATTERNS[(c + j) % 8]
            segs = split(letters(PATTERNS[pat](sum(sizes)), c), sizes)
            for place in ("shuffle", "e2e8"):
                out.append(msg(segs, f"{c} segments, empty {name}, {pat}", place))
    return make_batch(_items(out))


LIMIT_WORDS = (510, 511, 512, 513, 514)
LIMIT_COUNTS = (1, 2, 3, 63, 64)


@functools.lru_cache(maxsize=None)
def tile_limit():
    """hw + payload of 510 .. 514 words for 1, 2, 3, 63 and 64 segments in both placements; one
    segment of exactly 512 and of 513 words; framed lengths of exactly 1024 and 1536 words with a
    segment edge on, one before and one after each tile end."""
    out = []
    for c in LIMIT_COUNTS:
        for total in LIMIT_WORDS:
            room = total - header_words(c)
            for big in sorted({0, c - 1}):  # which segment takes what the one-word segments leave
                sizes = [1] * c
                sizes[big] = room - (c - 1)
                segs = split(letters(PATTERNS["CAAAB"](room), total), sizes)
                for place in ("e2e0", "e2e8", "shuffle"):
                    out.append(msg(segs, f"{c} segments, {total} framed words, big {big}", place))
    for w in (512, 513):
        big = letters(PATTERNS["AC"](w), w)
        for sizes_name, segs in (("alone", [big]), ("after a word", [letters("B"), big]),
                                 ("before an empty one", [big, b""]), ("between words", [letters("A"), big, letters("C")])):
            for place in ("e2e8", "shuffle"):
                out.append(msg(segs, f"a segment of {w} words {sizes_name}", place))
    for total in (1024, 1536):
        for end in range(TILE, total, TILE):
            for d in (-1, 0, 1):
                a = end + d - 2  # 3 segments: 2 table words
                sizes = [a, 7, total - 2 - a - 7]
                segs = split(letters(PATTERNS["CAAAB"](total - 2), total + d), sizes)
                for place in ("e2e0", "shuffle"):
                    out.append(msg(segs, f"{total} framed words, a segment edge at {end}{d:+d}", place))
    return make_batch(_items(out))


RUNS = (255, 256, 257)


def run_edge_messages():
    """(edge kind, Msg): "hdr" header -> segment 0, "seg" segment -> segment in a one-tile route,
    "tile" a tile end with a segment edge or an empty segment inside the look-ahead, "tail" the
    message's end less than 256 words after a tile end. A literal run cannot start in the table
    (a table word without a zero byte needs sizes of 2^24 words), so "hdr" runs are zero runs."""
    out = []

    def add(edge, s, sizes, kind, places):
        segs = split(letters(s, len(out)), sizes)
        for p in places:
            out.append((edge, msg(segs, kind, p)))

    for N in RUNS:
        for br in "ABCZ":
            # count 3, sizes (k, 0, 0): the second table word is zero and segment 0 opens with Z
            s = "Z" * (N - 1) + br + "C"
            add("hdr", s, [len(s), 0, 0], f"hdr 3 segments Z*{N} {br}", ("e2e0", "e2e8", "shuffle"))
            s = "Z" * (N - 2) + br + "C"
            add("hdr", s, [len(s), 0, 0, 0, 0], f"hdr 5 segments Z*{N} {br}", ("e2e8", "shuffle"))
            for L in "ZA":
                s = "C" + L * N + br + "C"
                for a in (1, 128, N - 1):
                    add("seg", s, [1 + a, len(s) - 1 - a], f"seg {L}*{N} cut at {a} {br}", ("e2e0", "e2e8", "shuffle"))
                add("seg", s, [129, 0, len(s) - 129], f"seg {L}*{N} empty at 128 {br}", ("e2e8", "shuffle", "last_broken"))
                # 2 table words; the run starts x words before the tile end, the edge is y past it
                for x in (1, 200):
                    for y in (1, 50, 255):
                        s = "C" * (TILE - x - 2) + L * N + br + "C"
                        cut = TILE + y - 2
                        if cut >= len(s):
                            continue
                        add("tile", s, [cut, len(s) - cut], f"tile {L}*{N} from -{x} edge +{y} {br}", ("e2e0", "shuffle"))
                        add("tile", s, [cut, 0, len(s) - cut], f"tile {L}*{N} from -{x} empty +{y} {br}", ("shuffle",))
                for t in (1, 100, 255):
                    h = TILE + t - 1 - N - 2
                    s = "C" * h + L * N + br + "C"
                    add("tail", s, [len(s)], f"tail {L}*{N} end +{t} {br}", ("e2e8",))
                    add("tail", s, [h + N // 2, len(s) - h - N // 2], f"tail {L}*{N} end +{t} {br} cut", ("shuffle",))
    for L in "ZA":
        for t in (1, 100, 255):  # the run goes on to the message's end
            s = "C" * (TILE - 3 - 1) + L * (3 + t)
            out.append(("tail", msg([letters(s, t)], f"tail {L} to the end +{t}", "e2e0")))
    return out


@functools.lru_cache(maxsize=None)
def run_edges():
    """Z and A runs of 255, 256 and 257 words across the edges of run_edge_messages, every breaker
    after the run."""
    return make_batch(_items([m for _, m in run_edge_messages()]))


PAIR_COUNTS = (2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 62, 63, 64)
PAIR_PLACES = ("e2e0", "e2e8", "shuffle", "reverse", "adj_rev", "last_broken", "dedup")


@functools.lru_cache(maxsize=None)
def pairs():
    """One-word segments throughout (every pair of the gathered route straddles two segments), and
    alternating 1- and 2-word segments at both header parities, in every placement."""
    out = []
    for c in PAIR_COUNTS:
        for j, (name, sizes) in enumerate((("ones", [1] * c), ("1 2", [1 + k % 2 for k in range(c)]),
                                           ("2 1", [2 - k % 2 for k in range(c)]))):
            pat = LATTICE_PATTERNS[(c + j) % 8]
            # "dedup" lists the same bytes twice: segments repeat with period 4
            for place in PAIR_PLACES:
                if place == "dedup":
                    unit = split(letters(PATTERNS[pat](sum(sizes[:4])), c), sizes[:4])
                    segs = [unit[k % 4] for k in range(c)]
                else:
                    segs = split(letters(PATTERNS[pat](sum(sizes)), c), sizes)
                out.append(msg(segs, f"{c} segments {name} {pat}", place))
    n = len(out)
    for j in range(0, n, 9):  # the same pool bytes shared by two messages
        out.append(out[j]._replace(place=("same", j), kind=out[j].kind + " shared"))
    return make_batch(_items(out))


def _route_samples():
    """One small message per route."""
    a = letters("CAZAB")
    return {
        "e2e": msg(split(a, [2, 3]), "e2e sample", "e2e8"),
        "gather": msg(split(a, [1, 0, 4]), "gather sample", "shuffle"),
        "tiled": msg([letters("C")] * 65, "tiled sample", "e2e0"),
        "arg": msg(split(a, [3, 2]), "arg sample", "e2e0", ("len", 1)),
    }


WAVE_NS = (1, 2, 3, 7, 8, 9, 15, 16, 17)


@functools.lru_cache(maxsize=None)
def wave_pairs():
    """Batches whose (m0, m1), the two messages of a wave of the first pass, take every ordered
    pair of routes (the first batch: all 16), and batches of 1, 2, 3 and of odd and even n around
    8 and 16 (a block is 4 waves of 2 messages) that walk through the pairs."""
    sm = _route_samples()
    order = [(r0, r1) for r0 in ROUTES for r1 in ROUTES]
    seq = [sm[r] for pr in order for r in pr]
    batches = [make_batch(_items(seq))]
    at = 0
    for n in WAVE_NS:
        for rep in range(4):
            batches.append(make_batch(_items([seq[(at + j) % len(seq)] for j in range(n)])))
            at += 2 * (n // 2) + 2 + 2 * rep
    return batches


def wave_pair_routes(b):
    return [(b.routes[i], b.routes[i + 1]) for i in range(0, len(b.msgs) - 1, 2)]


def cap_walk_messages():
    c513 = letters("C" * 513)
    return [
        msg([], "no segment"),
        msg([letters("A")], "one A word"),
        msg(split(letters("AB"), [1, 1]), "2 x 1 word", "e2e8"),
        msg(split(letters("CAZ"), [2, 0, 1]), "3 segments gathered", "shuffle"),
        msg(split(letters("ZAZA"), [1, 1, 1, 1]), "4 x 1 word ZA", "reverse"),
        msg([letters("B")], "one B word", "e2e8"),
        msg(split(letters("AAAZZ"), [3, 2]), "A run then Z run", "last_broken"),
        msg([b"", b"", b""], "3 empty segments", "shuffle"),
        msg([letters(PATTERNS["CAAAB"](300))], "300 words end to end", "e2e8"),
        msg(split(letters(PATTERNS["AAZZ"](300)), [100, 100, 100]), "3 x 100 words gathered", "shuffle"),
        msg(split(letters(PATTERNS["AC"](64)), [1] * 64), "64 x 1 word", "shuffle"),
        msg(split(letters(PATTERNS["ZZZC"](200)), [50, 150]), "ZZZC end to end", "e2e0"),
        msg(split(letters("C" * 1100), [600, 500]), "600 + 500 C words", "e2e0"),
        msg(split(letters(PATTERNS["CAAAB"](130)), [2] * 65), "65 x 2 words", "shuffle"),
        msg(split(letters("C" * 400 + "Z" * 300 + "C" * 834), [700, 834]), "a Z run over the tile end", "shuffle"),
        msg(split(letters("C" * 400 + "A" * 300 + "C" * 500), [450, 0, 750]), "an A run over the tile end", "e2e8"),
        msg([letters(PATTERNS["CAAAB"](1200))], "one segment of 1200 words", "e2e0"),
        msg([c513, b""], "513 words and an empty segment", "shuffle"),
        msg(split(letters("AB" * 8), [8, 8]), "bad length", "e2e0", ("len", 0)),
    ]


@functools.lru_cache(maxsize=None)
def cap_walk():
    """Capacities around the need of messages of all four routes: every capacity 0 .. need + 1 for
    a need of at most 64, else need - 9 .. need + 1, one below, on and one above each tile's packed
    end (the Zig bytes of the first 512 k framed words) and, for the C++ dialect, the end of each
    piece (the table, then each segment). The capacities of both dialects are walked under both."""
    items = []
    for j, m in enumerate(cap_walk_messages()):
        if m.bad:
            caps = {0, 1, 40}
        else:
            caps = set()
            for d in DIALECTS:
                need = len(reference(m.segs, d))
                caps |= set(range(0, need + 2)) if need <= 64 else set(range(need - 9, need + 2))
            f = frame_of(m)
            for end in range(8 * TILE, len(f), 8 * TILE):
                e = len(oracle.pack(f[:end])[1])
                caps |= {e - 1, e, e + 1}
            segs = list(m.segs) or [b""]
            e = 0
            for piece in [pyref_cxx.segment_table(segs)] + segs:
                e += len(pyref_cxx.pack_piece(piece))
                caps |= {max(e - 1, 0), e, e + 1}
        for c in sorted(caps):
            items.append((m, ("abs", c), (3 * len(items) + j) % 16))
    return make_batch(items)


ERROR_SPOTS = ((1, 0), (64, 0), (64, 63), (65, 0), (65, 64), (300, 0), (300, 64), (300, 299))


@functools.lru_cache(maxsize=None)
def errors():
    """len % 8 != 0 and ptr % 8 != 0 on segment 0, 63, 64 and the last of 300 segments, and 513
    segments; each as m0 beside a good m1 and as m1 beside a good m0, between valid neighbours of
    every route."""
    sm = _route_samples()
    good = [sm["e2e"], sm["gather"], sm["tiled"]]
    bads = []
    for c, s in ERROR_SPOTS:
        segs = split(letters(PATTERNS["CAAAB"](c), c + s), [1] * c)
        for what in ("len", "ptr"):
            for place in ("e2e0", "shuffle"):
                bads.append(msg(segs, f"{c} segments, bad {what} at {s}", place, (what, s)))
    bads.append(msg([letters("C")] * 513, "513 segments", "e2e0", ("count",)))
    bads.append(msg([b""] * 513, "513 empty segments", "shuffle", ("count",)))
    out, g = [], 0
    for bad in bads:
        for parity in (0, 1):  # the bad message as m0 and as m1
            for _ in range(2 if len(out) % 2 == parity else 1):  # one or two good ones first
                out.append(good[g % 3])
                g += 1
            assert len(out) % 2 == parity
            out.append(bad)
    out.append(good[g % 3])
    return make_batch(_items(out))


@functools.lru_cache(maxsize=None)
def random_mixed(seed=SEED + 1, n=2000):
    """test_encode_message_batch_stress's mix of shapes under every placement and slot phase, with
    capacities exact, encode_bound and (3%) too small."""
    rng = np.random.default_rng(seed)
    pat = np.frombuffer(random_words(rng, 4096, 0.5), dtype=np.uint8)

    def seg(w):
        if w == 0:
            return b""
        kind = int(rng.integers(0, 4))
        if kind == 0:
            return bytes(8 * w)
        if kind == 1:
            return random_words(rng, w, 0.0)
        o = 8 * int(rng.integers(0, pat.size // 8 - w))
        return pat[o:o + 8 * w].tobytes()

    items = []
    for i in range(n):
        r = rng.random()
        if r < 0.35:    # the bench's framing shape
            segs = [seg(127) for _ in range(4)]
        elif r < 0.80:  # one tile, a few segments, some empty
            segs = [seg(int(rng.choice([0, 1, 2, 17, 60, 120]))) for _ in range(int(rng.integers(0, 9)))]
        elif r < 0.90:  # around the one-tile segment limit
            segs = [seg(int(rng.integers(0, 5))) for _ in range(int(rng.choice([62, 63, 64, 65, 66, 100])))]
        elif r < 0.97:  # around a tile of framed words
            w = int(rng.choice([505, 508, 509, 510, 511, 512, 513, 600]))
            k = int(rng.integers(1, 4))
            segs = [seg(w // k) for _ in range(k - 1)] + [seg(w - (k - 1) * (w // k))]
        else:           # several tiles (at most 4)
            segs = [seg(int(rng.integers(300, 680))) for _ in range(int(rng.integers(1, 4)))]
        place = PLACEMENTS[int(rng.integers(0, len(PLACEMENTS)))]
        c = rng.random()
        cap = ("need", 0) if c < 0.45 else ("need", -int(rng.integers(1, 20))) if c < 0.48 else ("bound",)
        items.append((msg(segs, f"random {i}", place), cap, int(rng.integers(0, 16))))
    return make_batch(items)


BUILDERS = collections.OrderedDict([
    ("count_lattice", count_lattice), ("empty_edges", empty_edges), ("tile_limit", tile_limit),
    ("run_edges", run_edges), ("pairs", pairs), ("cap_walk", cap_walk), ("errors", errors),
    ("random_mixed", random_mixed)])
# the statuses each builder's messages must end with, under either dialect
_OK = {oracle.OK}
STATUSES = {
    "count_lattice": _OK, "empty_edges": _OK, "tile_limit": _OK, "run_edges": _OK, "pairs": _OK,
    "wave_pairs": {oracle.OK, oracle.INVALID_ARGUMENT},
    "cap_walk": {oracle.OK, oracle.OUT_OF_SPACE, oracle.INVALID_ARGUMENT},
    "errors": {oracle.OK, oracle.INVALID_ARGUMENT},
    "random_mixed": {oracle.OK, oracle.OUT_OF_SPACE},
}
# the routes each builder is aimed at
AIMED = {
    "count_lattice": {"e2e", "gather", "tiled"}, "empty_edges": {"gather", "tiled"},
    "tile_limit": {"e2e", "gather", "tiled"}, "run_edges": {"e2e", "gather", "tiled"},
    "pairs": {"e2e", "gather"}, "cap_walk": set(ROUTES), "errors": set(ROUTES),
    "random_mixed": {"e2e", "gather", "tiled"},
}


# ---- Message.init: the frames of tests/test_gpu_message_adversarial.py ------------------------------

INIT_CODES = {0: oracle.OK, -1: 8, -2: 9, -3: 10, -4: 13}  # oracle.message_init's codes -> capnp_packed.h's
INIT_TRUNCATED = 12  # lattice frames cut at every length


@functools.lru_cache(maxsize=None)
def init_frames():
    """The frames of count_lattice (one per message shape), every truncation length of a dozen of
    them, and the header error vectors of test_message_init_batch_matches_message_init."""
    seen, frames = set(), []
    for m in lattice_messages():
        f = frame_of(m)
        if f not in seen:
            seen.add(f)
            frames.append(f)
    small = [f for f in frames if 16 < len(f) <= 120]
    for f in small[::max(len(small) // INIT_TRUNCATED, 1)][:INIT_TRUNCATED]:
        frames += [f[:k] for k in range(len(f))]
        frames.append(f + POISON)  # trailing bytes are ignored
    u32 = lambda v: struct.pack("<I", v)  # noqa: E731
    frames += [b"", b"\x00\x00", b"\xff\xff\xff\xff" + bytes(12), u32(512) + bytes(4 * 514 + 8),
               u32(511) + bytes(4 * 513), u32(511) + bytes(4 * 512)]
    return frames


def header_entries(f):
    """[(offset, bytes)] of the segments a frame's table lists, whether or not the frame holds
    them; [] where the table itself is cut or its count is refused (message.zig:341-353)."""
    if len(f) < 4:
        return []
    count = struct.unpack_from("<I", f)[0] + 1
    header = 4 * (1 + count + (0 if count % 2 else 1))
    if count > MAX_SEGS or header > len(f):
        return []
    out, o = [], header
    for w in struct.unpack_from(f"<{count}I", f, 4):
        out.append((o, 8 * w))
        o += 8 * w
    return out
