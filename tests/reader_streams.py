"""Reader streams for Reader.readPackedMessage (reader.zig:84-156): an independent reader, a
seeded corpus around the framed-length cut, and the batch layout / comparison the GPU tests and
scripts/dev/fuzz_batches.py --read share. No GPU and no torch here.

read_message is written from the rule's statement (SURVEY.md Appendix A for the records,
DESIGN.md §2.4 for the stop at the framed length), not from oracle/packed_oracle.c, the way
pyref.py relates to the C oracle: the two restatements check each other in
tests/test_reader_streams.py.

The rule. Records are decoded one after another: 00 c -> c + 1 zero words; FF w c L -> the word
w, then c more words L; any other tag -> one word, bit k set <=> byte k is the next stream byte.
A byte the stream does not hold is EndOfStream. After every record, until the framed length is
known: the first four decoded bytes are the segment count minus one (FFFFFFFF:
InvalidSegmentCount; a count over 512: SegmentCountLimitExceeded); once the whole segment table
(4 * (1 + count) bytes, padded to a word) is decoded, the sizes' sum over 8 Mi words is
MessageTooLarge, else the framed length is the table plus 8 bytes per word. Reading stops at
the first record boundary at or past the framed length; past it is InvalidPackedMessage.
"""
import collections
import functools
import struct

import numpy as np

import pyref
import pyref_cxx

OK = "OK"
END_OF_STREAM = "END_OF_STREAM"
INVALID_SEGMENT_COUNT = "INVALID_SEGMENT_COUNT"
SEGMENT_COUNT_LIMIT_EXCEEDED = "SEGMENT_COUNT_LIMIT_EXCEEDED"
MESSAGE_TOO_LARGE = "MESSAGE_TOO_LARGE"
INVALID_PACKED_MESSAGE = "INVALID_PACKED_MESSAGE"
# oracle_read_packed_message's return codes
ORACLE_NAME = {0: OK, -1: END_OF_STREAM, -2: INVALID_SEGMENT_COUNT, -3: SEGMENT_COUNT_LIMIT_EXCEEDED,
               -6: MESSAGE_TOO_LARGE, -7: INVALID_PACKED_MESSAGE}

MAX_SEGMENTS = 512
MAX_TOTAL_WORDS = 8 * 1024 * 1024
WORDS_ROUTE_MAX = 1024  # framed words the words decoder takes (kRdWordsMax); longer: the walk passes

# status, framed: the decoded bytes (OK; InvalidPackedMessage: with the words past the framed
# length), consumed: the stream bytes the reader took. Facts for the coverage table: fw = framed
# words (None: never known), kind / rend = the record that reached or passed the framed length
# ("tag" / "zero" / "lit") and where it ends in the stream (a cut literal run: where it would),
# spans = the record that completed the segment table also decoded words after it.
Read = collections.namedtuple("Read", "status framed consumed fw kind rend spans")

_TAG_POS = [[k for k in range(8) if t >> k & 1] for t in range(256)]


def _framed_length(out):
    """(error status or None, framed length or None if the segment table is not whole yet)."""
    (minus_one,) = struct.unpack_from("<I", out, 0)
    if minus_one == 0xFFFFFFFF:
        return INVALID_SEGMENT_COUNT, None
    count = minus_one + 1
    if count > MAX_SEGMENTS:
        return SEGMENT_COUNT_LIMIT_EXCEEDED, None
    header = 4 * (1 + count + (1 - count % 2))
    if len(out) < header:
        return None, None
    total = sum(struct.unpack_from(f"<{count}I", out, 4))
    if total > MAX_TOTAL_WORDS:
        return MESSAGE_TOO_LARGE, None
    return None, header + 8 * total


def read_message(stream, header_only=False):
    """One message from the front of `stream`. header_only: stop once the framed length is known
    (status None) or the stream fails before that; fw and spans are then final, the rest is not."""
    s = bytes(stream)
    n = len(s)
    out = bytearray()
    r = 0
    needed = None
    spans = False
    kind = None
    while needed is None or len(out) < needed:
        if r >= n:
            return Read(END_OF_STREAM, b"", n, needed and needed // 8, None, None, spans)
        tag = s[r]
        r += 1
        if tag == 0x00:
            if r >= n:
                return Read(END_OF_STREAM, b"", n, needed and needed // 8, None, None, spans)
            out += bytes(8 * (s[r] + 1))
            r += 1
            kind = "zero"
        elif tag == 0xFF:
            if r + 9 > n:  # the word or the count is cut
                return Read(END_OF_STREAM, b"", n, needed and needed // 8, None, None, spans)
            out += s[r:r + 8]
            c = s[r + 8]
            r += 9
            if r + 8 * c > n:
                # a cut literal run; the reference fails here, before it looks at the header again
                cut_needed = needed
                if cut_needed is None:
                    err, cut_needed = _framed_length(out)
                if cut_needed is not None and len(out) + 8 * c >= cut_needed:
                    return Read(END_OF_STREAM, b"", n, cut_needed // 8, "lit", r + 8 * c, spans)
                return Read(END_OF_STREAM, b"", n, cut_needed and cut_needed // 8, None, None, spans)
            out += s[r:r + 8 * c]
            r += 8 * c
            kind = "lit"
        else:
            pos = _TAG_POS[tag]
            if r + len(pos) > n:
                return Read(END_OF_STREAM, b"", n, needed and needed // 8, None, None, spans)
            w = bytearray(8)
            for i, k in enumerate(pos):
                w[k] = s[r + i]
            out += w
            r += len(pos)
            kind = "tag"
        if needed is None:
            err, needed = _framed_length(out)
            if err is not None:
                return Read(err, b"", r, None, None, None, False)
            if needed is not None:
                count = struct.unpack_from("<I", out, 0)[0] + 1
                spans = len(out) > 4 * (1 + count + (1 - count % 2))
                if header_only:
                    return Read(None, b"", r, needed // 8, None, None, spans)
    status = OK if len(out) == needed else INVALID_PACKED_MESSAGE
    return Read(status, bytes(out), r, needed // 8, kind, r, spans)


def oracle_read(stream):
    """(status name, decoded bytes, consumed) from oracle/packed_oracle.c."""
    import oracle
    rc, framed, used = oracle.read_packed_message(stream, cap=1 << 20)
    return ORACLE_NAME[rc], framed, used


# ---------------------------------------------------------------------------
# The corpus
# ---------------------------------------------------------------------------

# family: exact / zero_over / lit_over / lit_cut / trunc / header / random. kind and rend as the
# generator built them (None where it did not build the last record): checked against read_message
# on the sampled streams. mode: how the base message was written (hand / zig / cxx; None: not a
# base's stream).
Stream = collections.namedtuple("Stream", "data family kind rend mode", defaults=(None,))

DENSITIES = ("literal", "mixed", "zero", "chain")
SEGMENT_COUNTS = (1, 2, 3, 8, 64, 511, 512)


def _rand(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def _nonzero(rng, n):
    return rng.integers(1, 256, int(n), dtype=np.uint8).tobytes()


def _segment_sizes(rng, nseg, body_words, front):
    """body_words over nseg segments, many of them empty; front: only the first half holds words
    (the last table word is then zero for nseg >= 2, and a zero run can span into the body)."""
    sizes = [0] * nseg
    holders = max(1, nseg // 2) if front else nseg
    live = sorted(set(int(x) for x in rng.integers(0, holders, min(holders, 6)))) if nseg > 1 else [0]
    cuts = sorted(int(x) for x in rng.integers(0, body_words + 1, len(live) - 1))
    prev = 0
    for seg, cut in zip(live, cuts + [body_words]):
        sizes[seg] = cut - prev
        prev = cut
    return sizes


def _body_bytes(rng, words, density):
    """Body words for a frame packed in one piece."""
    if words == 0:
        return b""
    if density == "chain":
        return bytes(8 * words)
    if density == "literal":
        a = rng.integers(1, 256, 8 * words, dtype=np.uint8)
        a[rng.random(8 * words) < 0.03] = 0
        return a.tobytes()
    if density == "mixed":
        a = rng.integers(1, 256, 8 * words, dtype=np.uint8)
        a[rng.random(8 * words) < 0.5] = 0
        return a.tobytes()
    a = np.zeros((words, 8), dtype=np.uint8)  # zero: runs of 64-256 zero words between a few others
    pos = int(rng.integers(0, 2)) * int(rng.integers(1, 100))  # half of them start with zero words
    while pos < words:
        k = min(int(rng.integers(1, 4)), words - pos)
        a[pos:pos + k] = rng.integers(0, 256, (k, 8), dtype=np.uint8)
        pos += k + int(rng.integers(64, 257))
    return a.tobytes()


def _hand_records(rng, words, density):
    """Records that decode to exactly `words` words."""
    out = bytearray()
    left = words
    while left > 0:
        x = rng.random()
        if density == "chain":
            run = min(left, 256)
        elif density == "zero":
            run = min(left, int(rng.integers(64, 257))) if x < 0.7 else 0
        elif density == "mixed":
            run = min(left, int(rng.integers(1, 20))) if x < 0.25 else 0
        else:
            run = min(left, 1) if x < 0.02 else 0
        if run:
            out += bytes((0, run - 1))
            left -= run
            continue
        if x > (0.7 if density == "literal" else 0.9):
            c = min(left - 1, int(rng.integers(0, 4)) if rng.random() < 0.7 else int(rng.integers(4, 40)))
            out += b"\xff" + _rand(rng, 8) + bytes((c,)) + _rand(rng, 8 * c)
            left -= 1 + c
        else:
            t = int(rng.integers(1, 255)) if density != "literal" else int(rng.integers(1, 255)) | 0x5A
            if t == 0xFF:
                t = 0x7F
            out += bytes((t,)) + _nonzero(rng, bin(t).count("1"))
            left -= 1
    return bytes(out)


def _record_starts(p):
    """(position, tag) of every record of a well-formed record string."""
    i, n, out = 0, len(p), []
    while i < n:
        t = p[i]
        out.append((i, t))
        if t == 0:
            i += 2
        elif t == 0xFF:
            i += 10 + 8 * p[i + 9]
        else:
            i += 1 + len(_TAG_POS[t])
    return out


def _small_messages(rng):
    """Packed messages for the bytes after a message (the next message on the connection)."""
    msgs = []
    for words in (0, 1, 3, 9, 40, 120):
        for p_zero in (0.1, 0.6):
            a = rng.integers(1, 256, 8 * words, dtype=np.uint8)
            a[rng.random(8 * words) < p_zero] = 0
            msgs.append(pyref.to_packed_bytes([a.tobytes()]))
    msgs.append(pyref.to_packed_bytes([bytes(8 * 700), bytes(range(1, 9))]))
    return msgs


def _base_specs(rng):
    """(framed words, segments, density, mode) per base message."""
    specs = []
    fws = [1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 4, 5, 5, 7, 9, 9, 12, 17, 17, 25, 33, 33, 41, 50, 64]
    fws += [int(x) for x in rng.integers(100, 1001, 34)]
    fws += list(range(1019, 1031)) * 2
    fws += [2990, 3001, 3007, 3012]
    for i, fw in enumerate(fws):
        nseg = SEGMENT_COUNTS[(i * 3 + i // 7) % len(SEGMENT_COUNTS)]
        while nseg // 2 + 1 > fw:  # the table alone must fit the framed words
            nseg = SEGMENT_COUNTS[SEGMENT_COUNTS.index(nseg) - 1]
        if fw == 2:
            nseg = (1, 2, 3)[i % 3]
        density = DENSITIES[(i + i // 4) % 4]
        if fw > 2000:
            density = ("zero", "chain", "mixed", "zero")[i % 4]
        mode = ("hand", "zig", "hand", "hand", "cxx", "hand")[i % 6]  # a third packed in one piece
        specs.append((fw, nseg, density, mode))
    return specs


def _build_base(rng, fw, nseg, density, mode):
    """prefix(k): record bytes decoding to the first fw - k framed words exactly."""
    hw = nseg // 2 + 1
    bw = fw - hw
    sizes = _segment_sizes(rng, nseg, bw, front=mode != "hand" and density in ("zero", "chain"))
    header = pyref.frame([bytes(8 * z) for z in sizes])[:8 * hw]
    if mode == "hand":
        body = _hand_records(rng, bw, density)
        starts = [p for p, _ in _record_starts(body)] + [len(body)]
        words_at = []  # framed body words decoded before each record start
        w = 0
        for p, t in _record_starts(body):
            words_at.append(w)
            w += 1 + (body[p + 1] if t == 0 else body[p + 9] if t == 0xFF else 0)
        words_at.append(w)
        head = pyref.pack(header)

        def prefix(k):
            # the longest whole-record prefix within bw - k words, topped up with tag words
            want = bw - k
            if want < 0:  # a table-only message: the record stands for the table's last word
                return pyref.pack(header[:8 * (hw + want)])
            j = max(i for i, x in enumerate(words_at) if x <= want)
            extra = want - words_at[j]
            return head + body[:starts[j]] + b"".join(b"\x81" + _nonzero(rng, 2) for _ in range(extra))
        return prefix
    frame = header + _body_bytes(rng, bw, density)
    packer = pyref.pack if mode == "zig" else pyref_cxx.pack_buffer

    def prefix(k):
        return packer(frame[:8 * (fw - k)])
    return prefix


def _header_error_streams(rng, tails):
    out = []
    for j in range(6):
        tail = tails[j % len(tails)][:j * 5]
        bad = struct.pack("<II", 0xFFFFFFFF, j)
        out.append(pyref.pack(bad) + tail)
        count = (513, 514, 1000, 1 << 16, 1 << 31, 0xFFFFFFFE)[j]
        over = struct.pack("<II", count - 1, 1 + j)
        out.append(pyref.pack(over) + tail + _rand(rng, 8 * j))
        nseg = (1, 2, 3, 64, 511, 512)[j]
        sizes = [MAX_TOTAL_WORDS // nseg + 1] * nseg
        table = struct.pack(f"<{1 + nseg}I", nseg - 1, *sizes) + bytes(4 * (1 - nseg % 2))
        out.append((pyref.pack if j % 2 else pyref_cxx.pack_buffer)(table) + tail)
    return [Stream(s, "header", None, None) for s in out]


def base_endings(rng, bi, fw, nseg, prefix, trailing, nexts, mode=None):
    """The streams around one base message's framed-length cut (prefix: _build_base's): exact
    with trailing bytes, a zero run or a literal run that passes the framed length, that literal
    run cut, and the stream truncated before the framed length."""
    streams = []
    S = functools.partial(Stream, mode=mode)
    bw = fw - (nseg // 2 + 1)
    exact = prefix(0)
    long_tail = 10 * fw + 40 - len(exact)
    for j, t in enumerate((0, 1, 7, 24, long_tail)):
        streams.append(S(exact + trailing(bi + j, t), "exact", None, None))
    nxt = nexts[bi % len(nexts)]
    streams.append(S(exact + nxt + _rand(rng, bi % 5), "exact", None, None))

    # the last record replaces the last k words (all of them in the body; a table-only
    # message ends in a zero word, which a zero run or a literal word can stand for)
    kmax = max(1, min(bw, 255))
    for j, over in enumerate((1, 16, 255) if bi % 2 else (2, 15, 100)):
        k = min(kmax, 256 - over, (1, 3, 40)[j])
        p = prefix(k)
        rec = bytes((0, k + over - 1))
        for jj, t in enumerate((0, 1, 7, 24, 10 * fw + 40 - len(p) - 2)):
            if j and jj in (1, 2):
                continue
            streams.append(S(p + rec + trailing(bi + jj, t), "zero_over", "zero", len(p) + 2))

    k = min(kmax, int(rng.integers(1, 9)))
    p = prefix(k)
    c = k + int(rng.integers(0, 30))
    reach = -(-(10 * fw + 14 - len(p) - 10) // 8)  # the run's end passes 10 * fw + 12
    if bi % 2 == 0 and reach <= 255:
        c = max(c, reach)
    c = min(c, 255)
    first = bytes(8) if bw == 0 else _rand(rng, 8)
    rec = b"\xff" + first + bytes((c,)) + _rand(rng, 8 * c)
    rend = len(p) + len(rec)
    ends = {rend - 9, rend - 8, rend - 1, rend, rend + 1, rend + 1500}
    ends |= {10 * fw + d for d in range(-12, 13) if 10 * fw + d > len(p)}
    full = p + rec
    for j, e in enumerate(sorted(ends)):
        if e < len(p) + 10:  # inside the record's first 9 bytes: no count byte, no run yet
            streams.append(S(full[:e], "trunc", None, None))
        elif e < rend:
            streams.append(S(full[:e], "lit_cut", "lit", rend))
        else:
            streams.append(S(full + trailing(bi + j, e - rend), "lit_over", "lit", rend))

    # the stream ends before the framed length: inside a tag's bytes, after a 00, inside an
    # FF record's first 9 bytes (first and last such record), and one byte short
    recs = _record_starts(exact)
    cuts = {len(exact) - 1, len(exact) // 2, 1} | ({0} if bi % 16 == 0 else set())
    for sel in (recs, recs[::-1]):
        tagged = next((q for q, t in sel if t not in (0, 0xFF) and len(_TAG_POS[t]) >= 2), None)
        zero = next((q for q, t in sel if t == 0), None)
        lit = next((q for q, t in sel if t == 0xFF), None)
        if tagged is not None:
            cuts.add(tagged + 2)
        if zero is not None:
            cuts.add(zero + 1)
        if lit is not None:
            cuts |= {lit + 1, lit + 5, lit + 9}
    for e in sorted(x for x in cuts if 0 <= x < len(exact)):
        streams.append(S(exact[:e], "trunc", None, None))
    return streams


def corpus(seed):
    """The list of Stream for this seed (about 6,000 streams, under 24 MB)."""
    rng = np.random.default_rng(seed)
    nexts = _small_messages(rng)
    streams = []

    def trailing(j, nbytes):
        """nbytes after a message: the next message's bytes (then noise), or noise alone."""
        if nbytes <= 0:
            return b""
        if j % 2:
            return _rand(rng, nbytes)
        return (nexts[j % len(nexts)] + _rand(rng, max(0, nbytes - len(nexts[j % len(nexts)]))))[:nbytes]

    for bi, (fw, nseg, density, mode) in enumerate(_base_specs(rng)):
        prefix = _build_base(rng, fw, nseg, density, mode)
        streams += base_endings(rng, bi, fw, nseg, prefix, trailing, nexts, mode)

    streams += _header_error_streams(rng, nexts)

    # message_test.zig:1076-1093 style random buffers, read as streams
    for i in range(1000):
        n = int(rng.integers(0, 161)) if i % 10 < 7 else int(rng.integers(513, 5121))
        b = bytearray(_rand(rng, n))
        if n and rng.random() < 0.5:
            b[0] = (0x00, 0xFF, 0x10, 0x01)[int(rng.integers(0, 4))]
        streams.append(Stream(bytes(b), "random", None, None))
    return streams


SEED = 0x5EED0007

# One corpus stream with everything the tests derive from the references: the oracle's result
# and read_message's header facts (fw, spans).
Case = collections.namedtuple("Case", "data family kind rend status framed consumed fw spans mode", defaults=(None,))


@functools.lru_cache(maxsize=2)
def cases(seed=SEED):
    out = []
    for s in corpus(seed):
        status, framed, used = oracle_read(s.data)
        h = read_message(s.data, header_only=True)
        out.append(Case(s.data, s.family, s.kind, s.rend, status, framed, used, h.fw, h.spans, s.mode))
    return out


def outcome(c):
    """The coverage table's outcome kinds (None: none of them)."""
    if c.status == OK:
        return "ok"
    if c.status == INVALID_PACKED_MESSAGE and c.kind in ("zero", "lit"):
        return "invalid_" + c.kind
    if c.status == END_OF_STREAM:
        return {"lit_cut": "eos_cut", "trunc": "eos_trunc"}.get(c.family)
    return None


OUTCOMES = ("ok", "invalid_zero", "invalid_lit", "eos_cut")


# ---------------------------------------------------------------------------
# Batch layout and comparison (numpy only; the GPU launch is the caller's)
# ---------------------------------------------------------------------------

SENT = 0xA5
FRONT = 64  # canary bytes before each slot
BACK = 64   # canary bytes after each slot's capacity


def choose_caps(cs, first=0):
    """Slot capacities, cycling per stream: the exact framed length, + 24, 9000 (walk route:
    framed + 4096), and for streams the oracle reads OK 8 bytes short of it."""
    caps = []
    for i, c in enumerate(cs):
        framed = 8 * (c.fw or 0)
        if c.status != OK:  # a random table may declare megabytes its stream cannot hold
            framed = min(framed, 1 << 16)
        big = 9000 if (c.fw or 0) <= WORDS_ROUTE_MAX else framed + 4096
        k = (i + first) % 4
        caps.append([framed, framed + 24, big, framed - 8 if c.status == OK else framed][k])
    return caps


def layout(rng, cs, caps):
    """Streams laid densely with 0-15 B gaps; 8-B aligned slots at every phase of a 128-B line,
    64 canary bytes before each and after each one's capacity."""
    n = len(cs)
    in_off = np.zeros(n, dtype=np.int64)
    pos = 0
    for i, c in enumerate(cs):
        pos += int(rng.integers(0, 16))
        in_off[i] = pos
        pos += len(c.data)
    buf = np.zeros(pos + 64, dtype=np.uint8)
    for c, o in zip(cs, in_off):
        buf[o:o + len(c.data)] = np.frombuffer(c.data, dtype=np.uint8)
    out_off = np.zeros(n, dtype=np.int64)
    o = 0
    for i, cap in enumerate(caps):
        o += FRONT + 8 * int(rng.integers(0, 16))
        out_off[i] = o
        o += (cap + 7) // 8 * 8 + BACK
    return buf, in_off, out_off, o + BACK


def compare(cs, caps, out_off, out, out_len, consumed, status, codes):
    """Every unit against the oracle's result; codes maps a status name to the library's code,
    with OUT_OF_SPACE. Returns the mismatches as (unit, what, got, want)."""
    bad = []
    for i, c in enumerate(cs):
        o, cap = int(out_off[i]), caps[i]
        st, ol, used = int(status[i]), int(out_len[i]), int(consumed[i])
        short = c.status == OK and len(c.framed) > cap
        want = codes["OUT_OF_SPACE"] if short else codes[c.status]
        if st != want:
            bad.append((i, "status", st, want))
            continue
        if c.status == OK:
            if (ol, used) != (len(c.framed), c.consumed):
                bad.append((i, "out_len, consumed", (ol, used), (len(c.framed), c.consumed)))
            elif not short and out[o:o + ol].tobytes() != c.framed:
                bad.append((i, "framed bytes differ from the oracle", None, None))
        elif (ol, used) != (0, 0):
            bad.append((i, "an error left out_len, consumed", (ol, used), (0, 0)))
        if not (out[o - FRONT:o] == SENT).all():
            bad.append((i, "bytes before the slot written", c.status, None))
        end = (cap + 7) // 8 * 8 + BACK
        lo = ol if c.status == OK and not short else cap
        if not (out[o + lo:o + end] == SENT).all():
            bad.append((i, "bytes past out_len (OK) / out_cap written", c.status, int(lo)))
    return bad
