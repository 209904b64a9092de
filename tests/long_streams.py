"""Adversarial and window-edge inputs for the long-unit decoders, with the
oracle's verdict on each. CPU only: plain numpy, `oracle` (message.zig:88-191) and the record
helpers of `small_streams`; tests/test_long_streams.py judges these inputs on the CPU and
tests/test_gpu_long_adversarial.py feeds them to the device.

A decode unit is long when it spans more than 320 16-B pieces counted from its 16-B aligned base
and its slot is 8-B aligned (huge: more than 64 KiB packed). Its packed bytes are cut into windows
of 4608 B at X_j = 4608 j; long_windows_kernel / window_spec_kernel / window_resolve_kernel /
window_fill_kernel take the units the window table holds, decode_wave_kernel<kWvLong> the others;
both run csrc/kernels/decode_wave.h. The families (every unit but the `edge` ones is long at any
alignment: 5121 packed bytes or more):
  random  random bytes;
  closed  random bytes cut at the last record boundary of the reference's walk (always OK);
  flip    a valid record stream with one tag, one 00 count or one FF count replaced, in the
          first, a middle and the last window;
  cut     a valid stream ending in a lone 00, in FF + 8 bytes without the count, inside a literal
          word, or 1 .. 10 bytes short: in the first and the last window of a short unit, and in
          windows 31, 32 and 33 of a longer one;
  phase   constant bytes and short periodic patterns in which every byte is a tag whose chain
          stays on its own phase, bare and after a 3-byte and a 4-byte record: chains from
          different entries never meet; and runs of 10 .. 200 bytes of one such pattern after
          another, on which lanes re-walk until their mark ids run out;
  entry   a record that ends exactly d bytes past a window boundary, d = 0 .. 72, at X_1 and X_2
          (a unit per tail) and at X_31, X_32 and X_33 (the resolve pass's batch edge), followed
          by a closed, a phase or a 00 FF-heavy tail;
  tail    units of 4608 k + r bytes, and units whose last window holds no record start;
  expand  zero and literal runs across a 1024-word output multiple, FF counts 3 and 4, two long
          literal runs starting in one lane chunk, FF 255 starting in a window's last 9 bytes,
          windows that begin with 144 bytes of 00 FF records;
  edge    valid streams of 5100 .. 5124 packed bytes at each of the 16 input alignments: both
          sides of ((address & 15) + P + 15) >> 4 > 320; and one long unit on a slot at 4 mod 8.
Every builder is deterministic in its seed and cached; nothing here is modified after it is
built. The window model at the end restates wv_resolve (walk A, walk B, the verification rounds)
lane by lane in plain Python."""
import bisect
import collections
import functools

import numpy as np

import oracle
import small_streams as ss

SENT, FRONT, BACK = ss.SENT, ss.FRONT, ss.BACK
WIN = 4608            # kWvWin
LONG_PIECES = 320     # kFlPieces
HUGE_BYTES = 65536    # kQHuge
WIN_BATCH = 32        # kWinBatch
WIN_D = 64            # kWinD
WIN_EXTRA = 32768     # the window table holds n / 8 + WIN_EXTRA windows
CMIN, SLACK, WAVE = 32, 16, 64  # kWvCmin, kWvSlack, lanes
EOFX = 0xFFFFFFFF     # kEOFX
NEVER = -1
LONG_MIN = 16 * LONG_PIECES + 1  # a unit of this many bytes is long at every alignment
SEED = 0x10C5EED5
FAMILIES = ("random", "closed", "flip", "cut", "phase", "entry", "tail", "expand", "edge")
PHASE_PATTERNS = (b"\x01", b"\x00", b"\x07", b"\x55", b"\x01\x07", b"\x00\x07", b"\x00\x01", b"\x03\x1f\x1f")
TAIL_R = (0, 1, 2, 9, 10, 31, 32, 33, 63, 64, 65, 72, 73, 4607)

# data: packed bytes; kind: family and detail; s: forced `address & 15` or None; mis: slot offset
# from its 8-B boundary; cap: forced capacity or None
Unit = collections.namedtuple("Unit", "data kind s mis cap")
Unit.__new__.__defaults__ = (None, 0, None)
Batch = collections.namedtuple("Batch", "units kinds cls exp caps mis in_off in_end out_off out_end")

_rand = ss._rand
expected = ss.expected


def pieces(P, s):
    return (s + P + 15) >> 4 if P else 0


def unit_class(P, s, mis=0):
    """'long' / 'huge' as launch_decode classes a unit of P bytes at `address & 15 == s`, else
    'other' (a misaligned slot keeps a unit off the long list: decode_long_unit)."""
    if mis or pieces(P, s) <= LONG_PIECES:
        return "other"
    return "huge" if P > HUGE_BYTES else "long"


# ---- record chains -----------------------------------------------------------------------------

_POP = np.array([bin(t).count("1") for t in range(256)], dtype=np.int64)
_TAB = {}


def tables(u):
    """(nx, wd): for every byte r of u read as a tag, the start of the next record (EOFX when the
    record runs past the end: wv_walk's rule) and the record's output words (wv_count)."""
    t = _TAB.get(u)
    if t is None:
        a = np.frombuffer(u, dtype=np.uint8).astype(np.int64)
        P = a.size
        c9 = np.zeros(P, dtype=np.int64)
        c9[:max(P - 9, 0)] = a[9:]
        b1 = np.zeros(P, dtype=np.int64)
        b1[:max(P - 1, 0)] = a[1:]
        ff, z = a == 0xFF, a == 0
        nx = np.arange(P) + 1 + _POP[a] + (ff | z) + ff * 8 * c9
        nx[nx > P] = EOFX
        wd = 1 + z * b1 + ff * c9
        t = _TAB[u] = (nx.tolist(), wd.tolist())
    return t


def chain(u):
    """(starts, eof): the record starts of u's true chain; eof is the start of the record that
    runs past the end, or None."""
    nx, _ = tables(u)
    r, P, out = 0, len(u), []
    while r < P:
        out.append(r)
        r = nx[r]
    return out, (out[-1] if r == EOFX else None)


def boundaries(p):
    """Record boundaries of a valid stream p (its end included)."""
    starts, eof = chain(p)
    assert eof is None
    return starts + [len(p)]


def fit(rng, p, L, bounds=None):
    """A valid stream of exactly L bytes: the longest prefix of the valid stream p that ends on a
    record boundary at L or at most L - 2, then short records (no record is one byte long)."""
    b = bounds if bounds is not None else boundaries(p)
    i = bisect.bisect_right(b, L) - 1
    while L - b[i] == 1:
        i -= 1
    out = bytearray(p[:b[i]])
    while len(out) < L:
        g = L - len(out)
        ok = [x for x in range(2, min(8, g) + 1) if g - x != 1]
        out += ss._filler(rng, ok[int(rng.integers(0, len(ok)))])
    return bytes(out)


def valid(rng, n):
    """A valid record stream of about n bytes: all record kinds, most 00 counts small."""
    return ss.records(rng, n, 0.1, 0.15, 0.1, 30)


def closed(rng, n):
    """n random bytes cut at the last record boundary of the reference's walk: always OK."""
    p = _rand(rng, n)
    _, eof = chain(p)
    return p if eof is None else p[:eof]


def ff_record(rng, c):
    return b"\xff" + _rand(rng, 8) + bytes([c]) + _rand(rng, 8 * c)


def straddler(rng, d):
    """A record for the end of which to land d bytes past a window boundary (it starts before
    the boundary): any record for d = 0, 00 c for d = 1 (the count is the window's first byte),
    a mixed record for d <= 7, an FF record of 10 + 8c > d bytes beyond (no other record is
    longer than 8 bytes)."""
    if d == 0:
        return ss._filler(rng, int(rng.integers(2, 9)))
    if d == 1:
        return bytes([0, int(rng.integers(0, 4))])
    if d <= 7:
        return ss._filler(rng, int(rng.integers(d + 1, 9)))
    return ff_record(rng, max(0, (d - 2) // 8) + int(rng.integers(0, 3)))


def phase_body(pat, n):
    return (pat * (n // len(pat) + 1))[:n]


def zero_heavy(rng, n):
    """About n bytes: 144 bytes of 00 FF records (256 zero words per 2 bytes), then short records
    with a 00 FF pair now and then."""
    out = bytearray(b"\x00\xff" * 72)
    while len(out) < n:
        out += b"\x00\xff" * int(rng.integers(1, 3)) if rng.random() < 0.06 else ss._filler(rng, int(rng.integers(2, 9)))
    return bytes(out)


def tail_stream(rng, kind, n, k=0):
    """A valid stream of about n bytes (at least n - 2100) of one of the entry family's tails."""
    if kind == "closed":
        return closed(rng, n + 2100)
    if kind == "phase":
        p = phase_body(PHASE_PATTERNS[k % len(PHASE_PATTERNS)], n + 16)
        return p[:boundaries_before(p, n + 8)]
    return zero_heavy(rng, n)


def boundaries_before(p, L):
    """The last record boundary of p's chain at or before L (p may end inside a record)."""
    nx, _ = tables(p)
    r = 0
    while r < len(p) and nx[r] != EOFX and nx[r] <= L:
        r = nx[r]
    return r


# ---- the families --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def big_base(seed=SEED + 100):
    """A valid stream of 36 windows and its boundaries, the shared head of the units that reach
    windows 31 .. 33."""
    rng = np.random.default_rng(seed)
    p = valid(rng, 36 * WIN)
    return p, boundaries(p)


@functools.lru_cache(maxsize=None)
def family(name, seed=SEED):
    """The Units of one family."""
    rng = np.random.default_rng(seed + FAMILIES.index(name))
    return tuple(globals()["_" + name](rng))


def _random(rng):
    return [Unit(_rand(rng, rng.integers(LONG_MIN, 20000)), "random") for _ in range(220)]


def _closed(rng):
    out = [Unit(closed(rng, int(rng.integers(7400, 36000))), "closed") for _ in range(38)]
    out += [Unit(closed(rng, 40 * WIN + 1000), "closed 40w"), Unit(closed(rng, 70 * WIN + 77), "closed 70w")]
    assert all(len(u.data) >= LONG_MIN for u in out)
    return out


def flip_in(rng, p, what, lo, hi):
    """p with one tag (what 0), one 00 count (1) or one FF count (2) of a record that starts in
    [lo, hi) replaced by another byte."""
    starts, _ = chain(p)
    want = {0: None, 1: 0, 2: 0xFF}[what]
    cand = [r for r in starts if lo <= r < hi and (want is None or p[r] == want) and r + 9 < len(p)]
    r = cand[int(rng.integers(0, len(cand)))] + (0, 1, 9)[what]
    q = bytearray(p)
    q[r] = (q[r] + int(rng.integers(1, 256))) & 0xFF
    return bytes(q)


def _flip(rng):
    out = []
    for i in range(36):
        p = fit(rng, valid(rng, 3 * WIN - 200), 3 * WIN - int(rng.integers(100, 1500)))
        w, what = i % 3, (i // 3) % 3
        out.append(Unit(flip_in(rng, p, what, w * WIN, min((w + 1) * WIN, len(p) - 20)),
                        "flip %s window %d" % (("tag", "00 count", "FF count")[what], w)))
    return out


def cut_end(rng, how, body):
    """The valid stream `body` ending one of four ways (small_streams.cut_one's)."""
    if how == 0:
        return body[:len(body) - int(rng.integers(1, 11))]
    if how == 1:
        return body + b"\x00"
    if how == 2:
        return body + b"\xff" + _rand(rng, 8)
    c = int(rng.integers(1, 6))
    return body + b"\xff" + _rand(rng, 8) + bytes([c]) + _rand(rng, 8 * c - int(rng.integers(1, 8)))


def _cut(rng):
    out = []
    base, bb = big_base()
    for how in range(4):
        for rep in range(3):  # the last window of a unit of 2 .. 4 windows
            w = 1 + rep
            body = fit(rng, valid(rng, (w + 1) * WIN), w * WIN + int(rng.integers(600 if w == 1 else 40, 4400)))
            out.append(Unit(cut_end(rng, how, body), "cut how %d last window %d" % (how, w)))
        for w in (31, 32, 33):
            body = fit(rng, base, w * WIN + int(rng.integers(40, 4400)), bb)
            out.append(Unit(cut_end(rng, how, body), "cut how %d window %d" % (how, w)))
    for rep in range(6):  # the first window: an FF run that starts there and is cut in the second
        t0 = int(rng.integers(3100, 4590))
        body = fit(rng, valid(rng, WIN), t0)
        P = int(rng.integers(LONG_MIN, min(t0 + 2049, 6600)))
        out.append(Unit(body + b"\xff" + _rand(rng, 8) + b"\xff" + _rand(rng, P - t0 - 10), "cut literal window 0"))
    assert all(len(u.data) >= LONG_MIN for u in out)
    return out


def _phase(rng):
    out = []
    for k, pat in enumerate(PHASE_PATTERNS):
        for pre in (0, 3, 4):
            n = int(rng.integers(2, 5)) * WIN + int(rng.integers(0, 4000)) + 600
            p = (ss._filler(rng, pre) if pre else b"") + phase_body(pat, n)
            if (k + pre) % 3:  # two units in three end on a record boundary
                p = p[:boundaries_before(p, len(p))]
            out.append(Unit(p, "phase %s prefix %d" % (pat.hex(), pre)))
    # the long ones: every lane of every window disagrees with its left neighbour
    p = ss._filler(rng, 3) + phase_body(b"\x01", 34 * WIN + 100)
    out.append(Unit(p[:boundaries_before(p, len(p))], "phase 01 prefix 3, 35 windows"))
    p = ss._filler(rng, 4) + phase_body(b"\x55", 40 * WIN + 7)
    out.append(Unit(p[:boundaries_before(p, len(p))], "phase 55 prefix 4, 41 windows"))
    # runs of 10 .. 200 bytes of one pattern after another: chains change phase from lane to lane,
    # lanes re-walk round after round and run out of mark ids (a seventh walk goes unmarked)
    pats = PHASE_PATTERNS + (b"\x1f", b"\x0f", b"\x7f", b"\x3f")
    for i in range(10):
        q = bytearray(ss._filler(rng, 2 + i % 7) if i % 2 else b"")
        n = int(rng.integers(2, 4)) * WIN + int(rng.integers(600, 4000))
        while len(q) < n:
            q += phase_body(pats[int(rng.integers(0, len(pats)))], int(rng.integers(10, 200)))
        p = bytes(q)
        out.append(Unit(p[:boundaries_before(p, len(p))], "phase runs"))
    assert all(len(u.data) >= LONG_MIN for u in out)
    return out


ENTRY_TAILS = ("closed", "phase", "zero")


def entry_unit(rng, d, windows, tail, k=0, head=None, head_bounds=None, end=None):
    """A unit in which a record ends exactly d bytes past X_j for every j of `windows`
    (consecutive), each followed by a `tail` stream."""
    out = bytearray()
    for j in windows:
        rec = straddler(rng, d)
        L = j * WIN + d - len(rec) - len(out)
        if not out and head is not None:
            out += fit(rng, head, L, head_bounds)
        else:
            out += fit(rng, tail_stream(rng, tail, L, k), L)
        out += rec
        assert len(out) == j * WIN + d
    L = int(rng.integers(600, 1500)) if end is None else end
    out += fit(rng, tail_stream(rng, tail, L, k), L)
    return bytes(out)


def _entry(rng):
    out = []
    base, bb = big_base()
    for d in range(73):
        for k, tail in enumerate(ENTRY_TAILS):
            out.append(Unit(entry_unit(rng, d, (1, 2), tail, d + k, valid(rng, WIN + 100)),
                            "entry d=%d X_1 X_2 %s" % (d, tail)))
            out.append(Unit(entry_unit(rng, d, (31, 32, 33), tail, d + k, base, bb),
                            "entry d=%d X_31..33 %s" % (d, tail)))
    return out


def _tail(rng):
    out = []
    for r in TAIL_R:
        for k in ((1, 2) if r >= 600 else (2, 3)):
            P = WIN * k + r
            out.append(Unit(fit(rng, valid(rng, P + 300), P), "tail k=%d r=%d" % (k, r)))
    # no record start in the last window: an FF run begun before X_k ends exactly at P = X_k + r
    for r in (1, 8, 9, 73, 500, 1500, 2039):
        k = int(rng.integers(2, 4))
        c = min(255, (r + 7) // 8 + int(rng.integers(0, 3)))
        L = WIN * k + r - 10 - 8 * c
        out.append(Unit(fit(rng, valid(rng, L + 300), L) + ff_record(rng, c), "tail run ends at P, r=%d" % r))
    return out


def _expand(rng):
    one = lambda n: b"".join(bytes([1, int(x)]) for x in rng.integers(1, 256, n))  # n one-word records
    pad = lambda p: p + fit(rng, valid(rng, 3000), max(LONG_MIN + 40 - len(p), 40))
    out = []
    # a zero run over output word 1024 and a literal run over word 2048 of window 0
    out.append(Unit(pad(one(1000) + b"\x00\x60" + one(932) + ff_record(rng, 40)), "expand runs over 1024 k"))
    # the same in window 1, entered 5 bytes in
    head = fit(rng, valid(rng, WIN), WIN - 3) + ss._filler(rng, 8)
    out.append(Unit(pad(head + one(1000) + b"\x00\xf0" + one(700) + ff_record(rng, 200)), "expand runs over 1024 k, window 1"))
    out.append(Unit(ss.records(rng, 3 * WIN, 0.2, 0.2, 1.0, 255), "expand long runs"))
    out.append(Unit(ss.records(rng, 4 * WIN, 0.05, 0.4, 1.0, 255), "expand long runs"))
    # FF counts 3 and 4: the last run a lane lists itself, the first it hands to the wave
    rec = lambda: b"\x00\x03" + ff_record(rng, 3) + ff_record(rng, 4) + ss._filler(rng, 5)
    out.append(Unit(b"".join(rec() for _ in range(120)), "expand FF 3 and 4"))
    # two FF records of count >= 4 that start in one 72-B lane chunk (period 144: bytes 0 and 42)
    two = lambda: ff_record(rng, 4) + ff_record(rng, 5) + fit(rng, b"", 52)
    out.append(Unit(b"".join(two() for _ in range(40)), "expand two runs a chunk"))
    for off in range(1, 10):  # FF 255 starting in the last 9 bytes of a window
        p = fit(rng, valid(rng, WIN), WIN - off) + ff_record(rng, 255) + fit(rng, valid(rng, 1200), 900)
        out.append(Unit(p, "expand FF 255 at X_1 - %d" % off))
    # windows whose first 144 bytes are 00 FF records; one window of more than 32767 words
    out.append(Unit(b"\x00\xff" * 72 + fit(rng, valid(rng, 5300), 5100), "expand 00 FF x 72, window 0"))
    out.append(Unit(fit(rng, valid(rng, WIN + 100), WIN) + b"\x00\xff" * 72 + fit(rng, valid(rng, 1500), 1200),
                    "expand 00 FF x 72, window 1"))
    out.append(Unit(b"\x00\xff" * 200 + fit(rng, valid(rng, 5300), 5000), "expand 00 FF x 200"))
    assert all(len(u.data) >= LONG_MIN for u in out)
    return out


def _edge(rng):
    out = []
    base = valid(rng, 5400)
    bb = boundaries(base)
    for s in range(16):
        for P in range(5100, 5125):
            if (P + s) % 5 == 0:  # an FF tag 3 bytes before the end: UNEXPECTED_EOF
                p = fit(rng, base, P - 3, bb) + b"\xff" + _rand(rng, 2)
            else:
                p = fit(rng, base, P, bb)
            out.append(Unit(p, "edge P=%d s=%d" % (P, s), s))
    # a long unit on a slot at 4 mod 8: INVALID_ARGUMENT, nothing written
    out.append(Unit(fit(rng, valid(rng, 7000), 6800), "edge misaligned slot", None, 4, 512))
    return out


# ---- layout and the per-unit contract ----------------------------------------------------------

def outcome(e, cap, mis=0):
    """(status, out_len) the decode batch owes for a non-empty unit."""
    if mis:
        return oracle.INVALID_ARGUMENT, 0
    if e.st != oracle.OK:
        return e.st, 0
    if len(e.ref) > cap:
        return oracle.OUT_OF_SPACE, len(e.ref)
    return oracle.OK, len(e.ref)


def make_batch(rng, units):
    """A batch of Units: the packed units form a dense stream with gaps of 0 .. 15 bytes (or at
    the unit's forced alignment), slot i is 8-B aligned (plus mis) with FRONT sentinel bytes
    before it and BACK after its capacity. An OK unit's capacity cycles through its exact size,
    8 B short (OUT_OF_SPACE), 24 B over and 0; a failing unit gets a random multiple of 512."""
    units = list(units)
    exp = expected([u.data for u in units])
    n = len(units)
    in_off, out_off = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    caps, cls = [], []
    pos, o, turn = 0, 0, 0
    for i, (u, e) in enumerate(zip(units, exp)):
        pos += int(rng.integers(0, 16)) if u.s is None else (u.s - pos) % 16
        in_off[i] = pos
        pos += len(u.data)
        if u.cap is not None:
            cap = u.cap
        elif e.st == oracle.OK:
            size = len(e.ref)
            cap = (size, max(size - 8, 0), size + 24, 0)[turn % 4]
            turn += 1
        else:
            cap = 512 * int(rng.integers(0, 9))
        caps.append(cap)
        cls.append(unit_class(len(u.data), int(in_off[i]) & 15, u.mis))
        o += FRONT
        out_off[i] = o + u.mis
        o += (cap + u.mis + 7) // 8 * 8 + BACK
    return Batch([u.data for u in units], [u.kind for u in units], cls, exp, caps, [u.mis for u in units],
                 in_off, pos, out_off, o)


def packed_stream(b):
    return ss.packed_stream(b.units, b.in_off, b.in_end)


def ideal(b):
    """What a correct device leaves: (status, out_len, output image)."""
    out = np.full(b.out_end, SENT, dtype=np.uint8)
    st, ol = np.zeros(len(b.units), dtype=np.int32), np.zeros(len(b.units), dtype=np.int64)
    for i, e in enumerate(b.exp):
        st[i], ol[i] = outcome(e, b.caps[i], b.mis[i])
        if st[i] == oracle.OK:
            o = int(b.out_off[i])
            out[o:o + len(e.ref)] = np.frombuffer(e.ref, dtype=np.uint8)
    return st, ol, out


def check(b, st, out_len, out_image):
    """The per-unit contract of a decoded batch b (out_image: the whole output buffer after the
    decode, SENT before it). A long unit is all-or-nothing (include/capnp_packed.h); the inside
    of a failed slot of any other unit is unspecified. Returns the statuses met, counted."""
    assert out_image.size == b.out_end
    seen = collections.Counter()
    for i, e in enumerate(b.exp):
        c, o, m = b.caps[i], int(b.out_off[i]), b.mis[i]
        want, wlen = outcome(e, c, m)
        seen[int(want)] += 1
        tag = (i, b.kinds[i], b.cls[i], len(b.units[i]), c)
        assert int(st[i]) == want, ("status",) + tag + (int(st[i]), int(want))
        assert int(out_len[i]) == wlen, ("out_len",) + tag + (int(out_len[i]), wlen)
        assert (out_image[o - m - FRONT:o] == SENT).all(), ("written before the slot",) + tag
        end = o + c
        back = o - m + (c + m + 7) // 8 * 8 + BACK
        assert (out_image[end:back] == SENT).all(), ("written past the capacity",) + tag
        if want == oracle.OK:
            got = out_image[o:o + wlen]
            if got.tobytes() != e.ref:
                at = int(np.flatnonzero(got != np.frombuffer(e.ref, dtype=np.uint8))[0])
                raise AssertionError(("decoded bytes differ from the oracle",) + tag + (at, at // 8))
            assert (out_image[o + wlen:end] == SENT).all(), ("written past out_len",) + tag
        elif b.cls[i] != "other" or m:
            assert (out_image[o:end] == SENT).all(), ("failed unit wrote into its slot",) + tag + (int(want),)
    return seen


def check_sizes(b, sz_len, sz_st):
    """decoded_size_batch against oracle.decoded_size (estimateUnpackedSize, message.zig:152-191)."""
    for i, e in enumerate(b.exp):
        want = (e.size_st, e.size if e.size_st == oracle.OK else 0)
        assert (int(sz_st[i]), int(sz_len[i])) == want, ("size", i, b.kinds[i], int(sz_st[i]), int(sz_len[i]), want)


# ---- the batches of tests/test_gpu_long_adversarial.py -----------------------------------------

@functools.lru_cache(maxsize=None)
def family_batch(name, seed=SEED + 1000):
    rng = np.random.default_rng(seed + FAMILIES.index(name))
    return make_batch(rng, family(name))


def encoder_units(rng, n):
    """n small and mid units of encoder output (8 .. 3000 B unpacked at three zero densities)."""
    out = []
    for i in range(n):
        size = 8 * int(rng.integers(1, 376))
        data = oracle.generate(1, size, seed=int(rng.integers(1 << 30)), zero_thresh=(26, 128, 230)[i % 3])
        st, p = oracle.pack(data.tobytes())
        assert st == oracle.OK
        out.append(Unit(p, "encoder output"))
    return out


@functools.lru_cache(maxsize=None)
def all_families(seed=SEED + 2000):
    """Every unit of every family and 300 small and mid encoder-output units, shuffled."""
    rng = np.random.default_rng(seed)
    units = [u for name in FAMILIES for u in family(name)] + encoder_units(rng, 300)
    order = rng.permutation(len(units))
    return make_batch(rng, [units[i] for i in order])


# The serial decoder: the window table holds n / 8 + WIN_EXTRA windows a batch, and inputs are
# read-only, so the same device-resident units are listed many times (equal in_off, a slot each)
# until the batch's windows exceed the table. Which units then take the serial list is decided
# by the order the waves of long_windows_kernel reserve in, so every alias is checked.
Serial = collections.namedtuple("Serial", "units kinds exp in_off in_end alias caps out_off out_end windows")
SERIAL_ALIASES = (("closed", 90, 0), ("closed", 60, -8), ("phase", 150, 0), ("entry", 150, 0), ("cut", 260, None))


@functools.lru_cache(maxsize=None)
def serial_batch(seed=SEED + 3000):
    rng = np.random.default_rng(seed)
    base, bb = big_base()
    p07 = ss._filler(rng, 3) + phase_body(b"\x07", 100000)
    units = {
        "closed": closed(rng, 300000),
        "phase": p07[:boundaries_before(p07, len(p07))],
        "entry": entry_unit(rng, 70, tuple(range(1, 13)), "closed", 0, valid(rng, WIN + 100)),
        "cut": fit(rng, base * 3, 400000, bb[:-1] + [len(base) + x for x in bb[:-1]] + [2 * len(base) + x for x in bb])
        + b"\xff" + _rand(rng, 8) + b"\x05" + _rand(rng, 33),
    }
    names = list(units)
    data = [units[k] for k in names]
    exp = expected(data)
    in_off, pos = [], 0
    for u in data:
        pos += int(rng.integers(0, 16))
        in_off.append(pos)
        pos += len(u)
    alias, caps = [], []
    for name, count, dcap in SERIAL_ALIASES:
        j = names.index(name)
        for _ in range(count):
            alias.append(j)
            caps.append(len(exp[j].ref) + dcap if dcap is not None else 512 * int(rng.integers(0, 9)))
    order = rng.permutation(len(alias))
    alias, caps = [alias[i] for i in order], [caps[i] for i in order]
    out_off, o = [], 0
    for c in caps:
        o += FRONT
        out_off.append(o)
        o += (c + 7) // 8 * 8 + BACK
    windows = sum((len(data[j]) + WIN - 1) // WIN for j in alias)
    return Serial(data, names, exp, np.array(in_off, dtype=np.int64), pos, np.array(alias, dtype=np.int64),
                  np.array(caps, dtype=np.int64), np.array(out_off, dtype=np.int64), o, windows)


def win_cap(n):
    return n // 8 + WIN_EXTRA


# ---- the window model ----------------------------------------------------------------------------
# wv_resolve of csrc/kernels/decode_wave.h, lane by lane. A lane's walks read and write marks in
# its own chunk only (a walk starts at or past its chunk's start and stops at the first tag at or
# past its end), so running the lanes of a step one after another is what the wave does at once.

Resolve = collections.namedtuple("Resolve", "exit rounds exhausted rewalks ents")
_RES = {}


def resolve(u, X, d0):
    """wv_resolve on the window of unit u at X entered at window byte d0: the exit (window-
    relative, EOFX), the verification rounds that re-walk a lane, whether a lane ran out of mark
    ids (a seventh walk: id 0), the most re-walks of one lane, and every lane's verified entry."""
    P = len(u)
    rem = P - X
    Pw = min(rem, WIN)
    key = (u[X:X + Pw + 10], min(rem, Pw + 2100), d0)
    got = _RES.get(key)
    if got is not None:
        return got
    nx, _ = tables(u)
    C = max(CMIN, (Pw + 63) >> 6)
    cs = [min(l * C, Pw) for l in range(WAVE)]
    ce = [min(c + C, Pw) for c in cs]
    mk = {}

    def walk(r, cend, ident):  # wv_walk: (exit, hit)
        while r < cend:
            m = mk.get(r, 0)
            if m:
                return r, m
            if ident:
                mk[r] = ident
            n = nx[X + r]
            r = EOFX if n == EOFX else n - X
        return r, 0

    e = [[0] * 8 for _ in range(WAVE)]  # e[lane][id]: the exit of the lane's walk id
    a0 = [d0] + cs[1:]
    ex = []
    for l in range(WAVE):  # walk A
        x, _ = walk(a0[l], ce[l], 1)
        e[l][1] = x
        ex.append(x)
    exa = list(ex)
    ent = [d0] + [cs[l] if exa[l - 1] > cs[l] + SLACK else exa[l - 1] for l in range(1, WAVE)]
    for l in range(WAVE):  # walk B
        if ent[l] != a0[l]:
            x, hit = walk(ent[l], ce[l], 2)
            if hit:
                x = e[l][min(hit, 7)]
            e[l][2] = x
            ex[l] = x
    nid = [3] * WAVE
    rounds, exhausted = 0, False
    while True:
        prev = [d0] + ex[:-1]
        bad = [ent[l] != prev[l] for l in range(WAVE)]
        if not any(bad):
            break
        rounds += 1
        assert rounds <= 2 * WAVE, "the rounds do not end"
        f = bad.index(True)
        new = list(ex)
        for l in range(1, WAVE):
            if bad[l] and (l == f or (not bad[l - 1] and prev[l] <= cs[l] + SLACK)):
                ent[l] = prev[l]
                ident = nid[l] if nid[l] <= 7 else 0
                exhausted = exhausted or ident == 0
                x, hit = walk(ent[l], ce[l], ident)
                if hit:
                    x = e[l][min(hit, 7)]
                if ident:
                    e[l][ident] = x
                new[l] = x
                nid[l] += 1
        ex = new
    got = _RES[key] = Resolve(ex[WAVE - 1], rounds, exhausted, max(nid) - 3, tuple(ent))
    return got


# per window j of a unit: depth the true entry (bytes past X_j; None: the chain does not enter),
# meet the bytes past X_j at which the chain guessed from X_j first joins the true one (NEVER),
# spec / entered the Resolve from entry 0 (the spec pass) and from the true entry (the resolve
# pass's re-stage and the fill pass), words the output words of the records that start in the
# window, starts their number, eof whether the record that runs past the end starts here
Window = collections.namedtuple("Window", "j depth meet spec entered words starts eof")
_WIN = {}


def windows(u):
    """The window model of unit u: a Window per 4608-B window."""
    got = _WIN.get(u)
    if got is not None:
        return got
    P = len(u)
    nx, wd = tables(u)
    starts, eof = chain(u)
    on = bytearray(P + 1)
    for r in starts:
        on[r] = 1
    k = (P + WIN - 1) // WIN
    seen = {}    # position -> the guessed walk that passed it
    result = {}  # guessed walk -> where it joined the true chain (absolute) or NEVER
    out, si = [], 0
    for j in range(k):
        X = j * WIN
        while si < len(starts) and starts[si] < X:
            si += 1
        s0 = si
        while si < len(starts) and starts[si] < X + WIN:
            si += 1
        mine = starts[s0:si]
        # the chain enters window j where the last record that starts before X_j ends; it does
        # not when that record runs past the unit's end (EOF) or ends it
        depth = 0
        if j:
            n = nx[starts[s0 - 1]]
            depth = None if n == EOFX or n >= P else n - X
        meet = None
        if depth is not None:
            r, path = X, []
            while True:
                if r == EOFX or r >= P:
                    res = NEVER
                    break
                if on[r]:
                    res = r
                    break
                if r in seen:
                    res = result[seen[r]]
                    break
                path.append(r)
                r = nx[r]
            for q in path:
                seen[q] = j
            result[j] = res
            meet = NEVER if res == NEVER else res - X
        spec = resolve(u, X, 0)
        entered = resolve(u, X, depth) if depth else (spec if depth == 0 else None)
        out.append(Window(j, depth, meet, spec, entered, sum(wd[r] for r in mine), len(mine),
                          eof is not None and X <= eof < X + WIN))
    _WIN[u] = out
    return out
