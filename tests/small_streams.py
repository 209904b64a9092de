"""Adversarial and class-edge inputs for the small-unit decoders (decode_small_kernel and
decode_small_group_kernel), with the oracle's verdict on each. CPU only: plain
numpy, `oracle` (message.zig:88-191) and `pyref_cxx`; tests/test_small_streams.py judges these
inputs on the CPU and tests/test_gpu_small_adversarial.py feeds them to the device.

A decode unit is small when it has at most 512 packed bytes and a slot of at most 8 KiB
(SMALL_LEN, SMALL_CAP). The kinds of unit (every one at most 512 packed bytes):
  random   random bytes, 161 .. 512 of them;
  records  valid record streams (00 c, FF w c + 8c, other tags) with 00 counts from all of
           0 .. 255 (one unit decodes to 8 KiB and beyond) and literal words of random bytes;
  cxx      C++-dialect streams (pyref_cxx) of random words at several zero densities;
  flip     a valid stream with one tag, one 00 count or one FF count replaced;
  cut      a valid stream shortened by 1 .. 10 bytes, or ending in a lone 00, in FF + 8 bytes
           without the count, or inside a literal word;
  chain    00 FF repeated 1 .. 5 times (2 KiB .. 10 KiB);
  tiny     streams of 0 .. 12 bytes (the refill batch's filler).
Every builder is deterministic in its seed and cached; nothing here is ever modified after it
is built.
"""
import collections
import functools

import numpy as np

import oracle
import pyref_cxx

SENT = 0xA5
FRONT = 64  # canary bytes before each slot
BACK = 64   # canary bytes after each slot's capacity
SMALL_LEN = 512
SMALL_CAP = 8192
MID_EDGES = (768, 1024, 1280, 1536, 2048, 2560, 3072)  # the mid bins' packed-length edges
LONG_PIECES = 320  # a unit of more 16-B pieces (from its 16-B aligned base) is long
KINDS = ("00 tag", "00 count", "FF tag", "FF count", "literal", "other tag")
SEED = 0x5A11AD5E

Exp = collections.namedtuple("Exp", "st ref size_st size")
# units / exp / caps / mis per unit; in_off / out_off relative to 256-B aligned device bases
Batch = collections.namedtuple("Batch", "units kinds exp caps mis in_off in_end out_off out_end")


def _rand(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


# ---- generators ---------------------------------------------------------------------------

def records(rng, target, p00=0.15, pff=0.15, wide=0.5, lit_max=12):
    """A valid packed stream of at most `target` bytes (the first record that would not fit
    ends it): shares p00 of 00 c, pff of FF w c + 8c, the rest other tags. A 00 count comes from
    0 .. 255 with probability `wide`, else from 0 .. 3; literal words are random bytes."""
    out = bytearray()
    while True:
        r = rng.random()
        if r < p00:
            c = int(rng.integers(0, 256)) if rng.random() < wide else int(rng.integers(0, 4))
            rec = bytes([0, c])
        elif r < p00 + pff:
            c = int(rng.integers(0, lit_max + 1)) if rng.random() < 0.5 else int(rng.integers(0, 3))
            rec = b"\xff" + _rand(rng, 8) + bytes([c]) + _rand(rng, 8 * c)
        else:
            t = int(rng.integers(1, 255))
            rec = bytes([t]) + _rand(rng, bin(t).count("1"))
        if len(out) + len(rec) > target:
            return bytes(out)
        out += rec


def record_starts(p):
    """(position, tag) of every record of a stream, as unpackPacked walks it (message.zig:101-141)."""
    i, n, out = 0, len(p), []
    while i < n:
        t = p[i]
        out.append((i, t))
        if t == 0:
            i += 2
        elif t == 0xFF:
            c = p[i + 9] if i + 9 < n else 0
            i += 10 + 8 * c
        else:
            i += 1 + bin(t).count("1")
    return out


def flip_one(rng, p):
    """Replace one tag, one 00 count or one FF count of a valid stream with a random byte."""
    starts = record_starts(p)
    pos, t = starts[int(rng.integers(0, len(starts)))]
    q = bytearray(p)
    if t == 0 and rng.random() < 0.5:
        pos += 1
    elif t == 0xFF and rng.random() < 0.5:
        pos += 9
    q[pos] = int(rng.integers(0, 256))
    return bytes(q)


def cut_one(rng, i, target):
    """A valid stream cut short: by 1 .. 10 bytes, or (i % 4 = 1, 2, 3) ending in a lone 00, in
    FF + 8 bytes with the count missing, or inside a literal word."""
    how = i % 4
    if how == 0:
        p = records(rng, target, 0.15, 0.2)
        return p[:max(1, len(p) - int(rng.integers(1, 11)))]
    if how == 1:
        return records(rng, target - 1, 0.15, 0.15) + b"\x00"
    if how == 2:
        return records(rng, target - 9, 0.15, 0.15) + b"\xff" + _rand(rng, 8)
    c = int(rng.integers(1, 6))
    p = records(rng, target - 10 - 8 * c, 0.15, 0.15)
    return p + b"\xff" + _rand(rng, 8) + bytes([c]) + _rand(rng, 8 * c - int(rng.integers(1, 8)))


def cxx_one(rng, i):
    """A C++-dialect stream (pyref_cxx) of random words: whole-word and per-byte zero densities
    by turns, shortened until it packs into SMALL_LEN bytes."""
    pz = (0.0, 0.3, 0.9, 0.97)[i % 4]          # whole zero words
    pb = (0.0, 0.05, 0.3, 0.7)[(i // 4) % 4]   # zero bytes within the other words
    nw = int(rng.integers(1, 1025 if pz >= 0.9 else 120))
    w = rng.integers(1, 256, (nw, 8), dtype=np.uint8)
    w[rng.random((nw, 8)) < pb] = 0
    w[rng.random(nw) < pz] = 0
    data = w.tobytes()
    p = pyref_cxx.pack_buffer(data)
    while len(p) > SMALL_LEN:
        data = data[:len(data) * 3 // 4 // 8 * 8]
        p = pyref_cxx.pack_buffer(data)
    return p


def chain(k):
    """00 FF, k times: 256 k zero words."""
    return bytes([0, 0xFF]) * k


def tiny_one(rng, i):
    """Streams of 0 .. 12 bytes: one or two short records, now and then failing or empty."""
    how = i % 16
    if how == 0:
        return b""
    if how == 1:
        return b"\x00"                       # a lone 00: UNEXPECTED_EOF
    if how == 2:
        return b"\xff" + _rand(rng, 8)       # the count is missing: UNEXPECTED_EOF
    if how == 3:
        t = int(rng.integers(1, 255)) | 3
        return bytes([t]) + _rand(rng, bin(t).count("1") - 1)  # a byte short: UNEXPECTED_EOF
    if how < 10:
        return bytes([0, int(rng.integers(0, 3))])
    if how < 14:
        return _filler(rng, 2)
    return records(rng, 12, 0.3, 0.1, wide=0.0, lit_max=0) or _filler(rng, 2)


def _filler(rng, nbytes):
    """One valid record of exactly nbytes bytes, 2 <= nbytes <= 8."""
    if nbytes == 2 and rng.random() < 0.3:
        return bytes([0, int(rng.integers(0, 3))])
    t = sum(1 << int(b) for b in rng.choice(8, nbytes - 1, replace=False))
    return bytes([t]) + _rand(rng, nbytes - 1)


def exact_len(rng, p, P):
    """The valid stream p brought to exactly P packed bytes with short valid records (no record
    is one byte long, so p first loses its last records while it is over P or one byte short)."""
    assert P >= 2
    starts = [pos for pos, _ in record_starts(p)]
    end = len(p)
    while end > P or P - end == 1:
        end = starts.pop()
    out = bytearray(p[:end])
    while len(out) < P:
        g = P - len(out)
        ok = [x for x in range(2, min(8, g) + 1) if g - x != 1]
        out += _filler(rng, ok[int(rng.integers(0, len(ok)))])
    return bytes(out)


def corpus_units(rng, n_random=600, n_records=1500, n_cxx=500, n_flip=600, n_cut=700, n_chain=100):
    """(units, kinds) of the main corpus."""
    units, kinds = [], []

    def add(kind, u):
        assert len(u) <= SMALL_LEN
        units.append(u)
        kinds.append(kind)

    for _ in range(n_random):
        add("random", _rand(rng, rng.integers(161, SMALL_LEN + 1)))
    for i in range(n_records):
        p00, pff, wide = ((0.15, 0.15, 0.5), (0.05, 0.3, 0.7), (0.3, 0.05, 0.3), (0.1, 0.1, 1.0))[i % 4]
        add("records", records(rng, int(rng.integers(161, SMALL_LEN + 1)), p00, pff, wide))
    for i in range(n_cxx):
        add("cxx", cxx_one(rng, i))
    for i in range(n_flip):
        add("flip", flip_one(rng, records(rng, int(rng.integers(161, SMALL_LEN + 1)), 0.1, 0.15, 0.3)))
    for i in range(n_cut):
        add("cut", cut_one(rng, i, int(rng.integers(161, SMALL_LEN + 1))))
    for i in range(n_chain):
        add("chain", chain(1 + i % 5))
    return units, kinds


# ---- the reference's verdict ----------------------------------------------------------------

_EXP = {}


def expected(units):
    """Exp per unit: oracle.unpack's status and bytes, oracle.decoded_size's status and size."""
    out = []
    for u in units:
        e = _EXP.get(u)
        if e is None:
            st, ref = oracle.unpack(u)
            sst, size = oracle.decoded_size(u)
            e = _EXP[u] = Exp(st, ref, sst, size)
        out.append(e)
    return out


def outcome(e, cap, ulen, mis=0):
    """(status, out_len) the decode batch owes for a unit of ulen packed bytes whose reference
    result is e, in a slot of cap bytes that starts `mis` bytes off an 8-B boundary."""
    if ulen == 0:
        return oracle.OK, 0  # an empty unit writes nothing: any slot will do
    if mis:
        return oracle.INVALID_ARGUMENT, 0
    if e.st != oracle.OK:
        return e.st, 0
    if len(e.ref) > cap:
        return oracle.OUT_OF_SPACE, len(e.ref)
    return oracle.OK, len(e.ref)


def choose_caps(rng, exp, small=True):
    """A slot capacity per unit. A unit that decodes OK: its exact size, size - 8, size + 1,
    size - 1, size + 24, or 8192 when the size fits. A unit that fails (or, with `small`,
    decodes past 8 KiB): any capacity in 0 .. 8192, not forced to a multiple of 8. With `small`
    every capacity is at most SMALL_CAP."""
    caps = []
    for e in exp:
        size = len(e.ref)
        if e.st == oracle.OK and not (small and size > SMALL_CAP):
            opts = [size, size - 8, size + 1, size - 1, size + 24] + ([SMALL_CAP] if size <= SMALL_CAP else [])
            opts = [c for c in opts if c >= 0 and not (small and c > SMALL_CAP)]
            caps.append(opts[int(rng.integers(0, len(opts)))])
        else:
            caps.append(int(rng.integers(0, SMALL_CAP + 1)))
    return caps


# ---- layout and the per-unit contract -------------------------------------------------------

def layout(units, caps, s, phase, mis=None, in_base=0, out_base=0):
    """Offsets of a batch, relative to the 256-B aligned bases of the device tensors. The packed
    units form a dense stream, unit i at the next address with `address & 15 == s[i]`; slot i
    starts at the next 8-B phase `phase[i]` (0 .. 7) of a 64-B chunk, plus mis[i] bytes, with FRONT
    canary bytes before it and BACK after its capacity. Returns in_off, in_end, out_off, out_end."""
    n = len(units)
    in_off = np.zeros(n, dtype=np.int64)
    out_off = np.zeros(n, dtype=np.int64)
    pos, o = in_base, out_base
    for i, u in enumerate(units):
        pos += (int(s[i]) - pos) % 16
        in_off[i] = pos
        pos += len(u)
        o += FRONT
        o += 8 * ((int(phase[i]) - (o >> 3)) % 8)
        m = int(mis[i]) if mis is not None else 0
        out_off[i] = o + m
        o += (caps[i] + m + 7) // 8 * 8 + BACK
    return in_off, pos, out_off, o


def packed_stream(units, in_off, in_end, in_base=0):
    """The packed bytes of a batch as laid out (gaps and 64 B of tail hold FF, the tag that would
    read furthest)."""
    buf = np.full(in_end - in_base + 64, 0xFF, dtype=np.uint8)
    for u, o in zip(units, in_off):
        buf[o - in_base:o - in_base + len(u)] = np.frombuffer(u, dtype=np.uint8)
    return buf


def make_batch(rng, units, kinds=None, caps=None, mis=None, s=None, phase=None, small=True):
    n = len(units)
    exp = expected(units)
    caps = list(caps) if caps is not None else choose_caps(rng, exp, small)
    mis = list(mis) if mis is not None else [0] * n
    s = s if s is not None else rng.integers(0, 16, n)
    phase = phase if phase is not None else rng.integers(0, 8, n)
    in_off, in_end, out_off, out_end = layout(units, caps, s, phase, mis)
    return Batch(list(units), list(kinds) if kinds is not None else [""] * n, exp, caps, mis, in_off, in_end,
                 out_off, out_end)


def is_small(b, i):
    return len(b.units[i]) <= SMALL_LEN and b.caps[i] <= SMALL_CAP


def check(b, out, st, ol, strict):
    """The per-unit contract of a decoded batch b (out: the output buffer after the decode, SENT
    before it). strict (one bool, or one per unit): a failed unit leaves its whole slot untouched.
    Returns the set of statuses met."""
    seen = set()
    for i, e in enumerate(b.exp):
        u, c, o, m = b.units[i], b.caps[i], int(b.out_off[i]), b.mis[i]
        want, wlen = outcome(e, c, len(u), m)
        seen.add(int(want))
        assert int(st[i]) == want, (i, b.kinds[i], len(u), c, int(st[i]), int(want))
        assert int(ol[i]) == wlen, (i, b.kinds[i], len(u), c, int(want), int(ol[i]), wlen)
        assert (out[o - FRONT:o] == SENT).all(), (i, b.kinds[i], "bytes before the slot written")
        if want == oracle.OK:
            assert out[o:o + wlen].tobytes() == e.ref[:wlen], (i, b.kinds[i], "decoded bytes differ from the oracle")
            assert (out[o + wlen:o + c + BACK] == SENT).all(), (i, b.kinds[i], "bytes past out_len written")
        else:
            whole = strict if isinstance(strict, (bool, np.bool_)) else strict[i]
            lo = o if (whole or m) else o + c
            assert (out[lo:o + c + BACK] == SENT).all(), (i, b.kinds[i], int(want), "failed unit wrote where it may not")
    return seen


def check_sizes(b, sz_len, sz_st):
    """decoded_size_batch against oracle.decoded_size (estimateUnpackedSize, message.zig:152-191)."""
    for i, e in enumerate(b.exp):
        want = (e.size_st, e.size if e.size_st == oracle.OK else 0)
        assert (int(sz_st[i]), int(sz_len[i])) == want, ("size", i, b.kinds[i], int(sz_st[i]), int(sz_len[i]), want)


def coverage(units, in_off):
    """Every (kind, (s + pos) mod 64) the batch holds, s = in_off & 15 and pos the byte's place
    in its unit: where in a lane's 64-B ring (16-B aligned space) each 00 tag, 00 count, FF tag,
    FF count, literal word start and other tag falls."""
    cov = set()
    for u, off in zip(units, in_off):
        s, n = int(off) & 15, len(u)
        for pos, t in record_starts(u):
            if t == 0:
                cov.add(("00 tag", (s + pos) % 64))
                if pos + 1 < n:
                    cov.add(("00 count", (s + pos + 1) % 64))
            elif t == 0xFF:
                cov.add(("FF tag", (s + pos) % 64))
                if pos + 9 < n:
                    cov.add(("FF count", (s + pos + 9) % 64))
                    for j in range(u[pos + 9]):
                        if pos + 10 + 8 * j < n:
                            cov.add(("literal", (s + pos + 10 + 8 * j) % 64))
            else:
                cov.add(("other tag", (s + pos) % 64))
    return cov


# ---- the batches of tests/test_gpu_small_adversarial.py -------------------------------------

@functools.lru_cache(maxsize=None)
def main_corpus(seed=SEED):
    """About 4000 small units of every kind at random alignments and slot phases."""
    rng = np.random.default_rng(seed)
    units, kinds = corpus_units(rng)
    return make_batch(rng, units, kinds)


@functools.lru_cache(maxsize=None)
def mixed_corpus(seed=SEED + 1):
    """The main corpus's units (fresh slots) with a mid unit (600 .. 3000 packed bytes: records,
    flipped, cut, random) after every second one, and six long units: the small list is not the
    identity. Slots of the others are not bound to 8 KiB."""
    rng = np.random.default_rng(seed)
    src = main_corpus()
    units, kinds, caps = [], [], []
    nlong = 0
    for i, (u, k, c) in enumerate(zip(src.units, src.kinds, src.caps)):
        units.append(u)
        kinds.append(k)
        caps.append(c)
        if i % 2:
            how = (i // 2) % 8
            target = int(rng.integers(900, 3001))  # a stream ends within 250 B of its target
            if how == 0 and nlong < 6:
                m, kd = records(rng, int(rng.integers(6000, 20000)), 0.1, 0.15, 0.0, 30), "long"
                nlong += 1
            elif how < 4:
                m, kd = records(rng, target, 0.15, 0.15, 0.1, 30), "mid records"
            elif how < 6:
                m, kd = flip_one(rng, records(rng, target, 0.1, 0.15, 0.1, 30)), "mid flip"
            elif how == 6:
                m, kd = cut_one(rng, i // 16, target), "mid cut"
            else:
                m, kd = _rand(rng, rng.integers(600, 3001)), "mid random"
            assert len(m) >= 600
            units.append(m)
            kinds.append(kd)
            caps.append(choose_caps(rng, expected([m]), small=False)[0])
    return make_batch(rng, units, kinds, caps)


@functools.lru_cache(maxsize=None)
def partial_wave(n, seed=SEED + 2):
    """n units drawn from the main corpus; from 3 units up, the second is an empty unit on a
    misaligned slot and the third a non-empty unit on a misaligned slot."""
    rng = np.random.default_rng(seed + n)
    src = main_corpus()
    pick = rng.choice(len(src.units), n, replace=False)
    units = [src.units[j] for j in pick]
    kinds = [src.kinds[j] for j in pick]
    caps = [src.caps[j] for j in pick]
    mis = [0] * n
    if n >= 3:
        units[1], kinds[1], caps[1], mis[1] = b"", "empty misaligned", 40, 3
        kinds[2], mis[2] = kinds[2] + " misaligned", 4
    return make_batch(rng, units, kinds, caps, mis)


@functools.lru_cache(maxsize=None)
def single_units(seed=SEED + 3):
    """One-unit batches: a corpus unit, an empty unit on a misaligned slot, a non-empty one on a
    misaligned slot."""
    rng = np.random.default_rng(seed)
    src = main_corpus()
    j = next(i for i, e in enumerate(src.exp) if outcome(e, src.caps[i], len(src.units[i]))[0] == oracle.OK)
    return (make_batch(rng, [src.units[j]], [src.kinds[j]], [src.caps[j]]),
            make_batch(rng, [b""], ["empty misaligned"], [24], [5]),
            make_batch(rng, [src.units[j]], [src.kinds[j] + " misaligned"], [src.caps[j]], [1]))


@functools.lru_cache(maxsize=None)
def lattice(seed=SEED + 4):
    """(batch, claimed packed lengths): valid streams of exact packed length on the class edges
    (511, 512, 513; each mid bin edge and the byte after it; the last length of 320 pieces and
    the first of 321), each at all 16 values of s, each in slots of its exact size, 8 short, 1
    over, 1 short, and 8184 / 8192 / 8200 B where the decoded size fits. And 00 FF x 4 into
    8192 B (small) and 00 FF x 4, 00 00 into 8200 B (mid)."""
    rng = np.random.default_rng(seed)
    units, kinds, caps, s_of, claims = [], [], [], [], []
    fixed = [511, 512, 513] + [B + d for B in MID_EDGES for d in (0, 1)]
    for s in range(16):
        # (s + P + 15) >> 4 == 320 for the last time at P = 5120 - s, 321 first at 5121 - s
        for P in fixed + [16 * LONG_PIECES - s, 16 * LONG_PIECES - s + 1]:
            p = exact_len(rng, records(rng, P - 12, 0.06, 0.15, 0.0, 20), P)
            size = len(expected([p])[0].ref)
            for c in [size, size - 8, size + 1, size - 1] + [x for x in (8184, 8192, 8200) if size <= x]:
                if c >= 0:
                    units.append(p)
                    kinds.append(f"P={P} s={s}")
                    caps.append(c)
                    s_of.append(s)
                    claims.append(P)
        for p, c in ((chain(4), 8192), (chain(4) + b"\x00\x00", 8200)):
            units.append(p)
            kinds.append(f"tiny s={s}")
            caps.append(c)
            s_of.append(s)
            claims.append(len(p))
    return make_batch(rng, units, kinds, caps, s=s_of), claims


# The group kernel (decode_small_group_kernel) gives each wave a contiguous range of
# ceil(count / waves) entries of the small list, 4 waves a block, one block per 256 units; a wave
# takes, from its cursor, the longest run of up to 64 entries whose 16-B pieces sum to at most
# GROUP_PIECES and whose capacity words (cap >> 3) sum to at most GROUP_WORDS.
GROUP_PIECES = 4096 // 16
GROUP_WORDS = 1024
GROUP_SEG = 16  # entries per wave in group_batches(): 64 units a batch, 4 waves


def pieces(u, s):
    return (s + len(u) + 15) >> 4 if len(u) else 0


def group_sizes(np_list, capw_list):
    """The sizes of the groups a wave makes of its range (the rule above; a group has at least
    one unit)."""
    out, i, n = [], 0, len(np_list)
    while i < n:
        g, sp, sw = 0, 0, 0
        while i + g < n and g < 64 and sp + np_list[i + g] <= GROUP_PIECES and sw + capw_list[i + g] <= GROUP_WORDS:
            sp += np_list[i + g]
            sw += capw_list[i + g]
            g += 1
        g = max(g, 1)
        out.append(g)
        i += g
    return out


@functools.lru_cache(maxsize=None)
def group_batches(seed=SEED + 5):
    """([batch, ...], {scenario: (batch index, first entry, s per entry)}): batches of 64 units, 4
    wave ranges of GROUP_SEG entries each; a range starts with a hand-built sequence and ends with
    tiny OK units in exact slots. Scenarios:
      pieces      eight units of 512 B at s = 15 (33 pieces each): the group cuts after seven;
      words=1024  caps 4096 + 4096: exactly 1024 capacity words, one group with what follows of cap 0;
      words>1024  caps 4096 + 4104: the second unit starts a new group;
      lone        a cap of 8192 (00 FF x 4): a group of its own once a unit with capacity follows;
      odd         cap-0 units, empty units and one misaligned slot inside a group;
      first / middle / last   a failing unit at entry 0 / 7 / 15 of a 16-unit group."""
    rng = np.random.default_rng(seed)
    ok2 = lambda: bytes([0, int(rng.integers(0, 3))]) if rng.random() < 0.5 else _filler(rng, int(rng.integers(2, 9)))
    EXACT = -1

    def seg(head):
        """head: [(unit, cap or EXACT, s or None, mis)]; padded to GROUP_SEG with tiny OK units."""
        rows = list(head)
        while len(rows) < GROUP_SEG:
            rows.append((ok2(), EXACT, None, 0))
        assert len(rows) == GROUP_SEG
        return rows

    full = lambda: exact_len(rng, records(rng, 500, 0.05, 0.2, 0.0, 20), 512)
    eof = lambda: cut_one(rng, int(rng.integers(1, 4)), 40)
    segs = {
        "pieces": seg([(full(), EXACT, 15, 0) for _ in range(8)]),
        "words=1024": seg([(chain(2), 4096, None, 0), (chain(2), 4096, None, 0)] +
                          [(ok2(), 0, None, 0) for _ in range(3)]),
        "words>1024": seg([(chain(2), 4096, None, 0), (chain(2) + b"\x00\x00", 4104, None, 0)]),
        "lone": seg([(ok2(), EXACT, None, 0), (chain(4), 8192, None, 0), (ok2(), EXACT, None, 0)]),
        "odd": seg([(ok2(), 0, None, 0), (b"", 0, None, 0), (ok2(), EXACT, None, 0), (b"", 64, None, 0),
                    (ok2(), EXACT, None, 3), (b"", 16, None, 5), (records(rng, 60, 0.1, 0.2), 0, None, 0),
                    (ok2(), 7, None, 0)]),
        "first": seg([(eof(), 64, None, 0)]),
        "middle": seg([(ok2(), EXACT, None, 0) for _ in range(7)] + [(chain(5), 8192 - 7 * 64, None, 0)]),
        "last": seg([(ok2(), EXACT, None, 0) for _ in range(15)] + [(eof(), 33, None, 0)]),
    }
    names = list(segs)
    batches, where = [], {}
    for b0 in range(0, len(names), 4):
        units, kinds, caps, mis, s_of = [], [], [], [], []
        for k, name in enumerate(names[b0:b0 + 4]):
            for u, c, s, m in segs[name]:
                units.append(u)
                kinds.append(name)
                caps.append(len(expected([u])[0].ref) if c == EXACT else c)
                mis.append(m)
                s_of.append(int(rng.integers(0, 16)) if s is None else s)
            where[name] = (len(batches), k * GROUP_SEG, s_of[k * GROUP_SEG:(k + 1) * GROUP_SEG])
        assert len(units) == 4 * GROUP_SEG
        batches.append(make_batch(rng, units, kinds, caps, mis, s=s_of))
    return batches, where


REFILL_TILE = 4096   # distinct units of the refill batch
REFILL_HEAVY = 64    # of them, the expanders: one per 64 consecutive list entries
Refill = collections.namedtuple("Refill", "tile stride n in_off out_off caps order image care_strict care_prefix")


@functools.lru_cache(maxsize=None)
def refill(n=1 << 20, seed=SEED + 6):
    """The lane-refill batch: n units, n / 4096 tiles of one 4096-unit batch `tile`. The tiles
    share the packed bytes; tile t's slots (and canaries) are the tile's, `stride` bytes further
    per tile. The tile holds 64 expanders (OK units of 4 KiB and more from the main corpus, 00 FF
    x 4 into 8192 B, 00 FF x 5 into 8192 B: OUT_OF_SPACE) and 4032 light units (tiny streams of
    0 .. 12 bytes, a third of them failing: UNEXPECTED_EOF, OUT_OF_SPACE, a misaligned slot; and
    corpus units in slots of at most 256 B). order[b] = 4096 t + j is the unit at batch position
    b: every 64 consecutive positions hold one expander at a random place among 63 light units
    of one tile, a fresh permutation per tile.
    image / care_*: the bytes one tile's output region must hold after the decode (SENT where
    nothing may be written) and the bytes that are pinned (all of them when failed units leave
    their slots untouched; all but the failed units' slots otherwise)."""
    assert n % REFILL_TILE == 0
    rng = np.random.default_rng(seed)
    src = main_corpus()
    verdict = [outcome(e, c, len(u)) for u, e, c in zip(src.units, src.exp, src.caps)]
    big = [i for i, (st, ln) in enumerate(verdict) if st == oracle.OK and ln >= 4096][:REFILL_HEAVY - 8]
    units = [src.units[i] for i in big] + [chain(4)] * 4 + [chain(5)] * 4
    kinds = ["expander"] * REFILL_HEAVY
    caps = [src.caps[i] for i in big] + [8192] * 4 + [8192, 8191, 8185, 8184]
    mis = [0] * REFILL_HEAVY
    assert len(units) == REFILL_HEAVY
    light = [i for i, c in enumerate(src.caps) if c <= 256]
    nlight = REFILL_TILE - REFILL_HEAVY
    for j in range(nlight):
        if j % 8 == 7:
            i = light[(j // 8) % len(light)]
            u, k, c, m = src.units[i], src.kinds[i], src.caps[i], 0
        else:
            u, k, m = tiny_one(rng, j), "tiny", 0
            size = len(expected([u])[0].ref)
            r = j % 5
            c = size if r < 3 else (max(size - int(rng.integers(1, 10)), 0) if r == 3 else size + int(rng.integers(0, 3)))
            if j % 41 == 13:
                m = int(rng.integers(1, 8))
        units.append(u)
        kinds.append(k)
        caps.append(c)
        mis.append(m)
    tile = make_batch(rng, units, kinds, caps, mis)
    stride = (tile.out_end + BACK + 255) // 256 * 256
    tiles = n // REFILL_TILE
    # batch order: per tile, 64 groups of (one expander + 63 light units), shuffled within the group
    heavy = rng.permuted(np.tile(np.arange(REFILL_HEAVY), (tiles, 1)), axis=1)
    lights = rng.permuted(np.tile(np.arange(REFILL_HEAVY, REFILL_TILE), (tiles, 1)), axis=1)
    groups = np.concatenate([heavy[:, :, None], lights.reshape(tiles, REFILL_HEAVY, 63)], axis=2)
    groups = rng.permuted(groups, axis=2)
    order = (groups.reshape(tiles, REFILL_TILE) + REFILL_TILE * np.arange(tiles)[:, None]).reshape(-1)
    j, t = order % REFILL_TILE, order // REFILL_TILE
    in_off = tile.in_off[j]
    out_off = tile.out_off[j] + stride * t
    caps_n = np.asarray(tile.caps, dtype=np.int64)[j]
    image = np.full(stride, SENT, dtype=np.uint8)
    care = np.ones(stride, dtype=bool)
    for i, e in enumerate(tile.exp):
        st, ln = outcome(e, tile.caps[i], len(tile.units[i]), tile.mis[i])
        o = int(tile.out_off[i])
        if st == oracle.OK:
            image[o:o + ln] = np.frombuffer(e.ref, dtype=np.uint8)[:ln]
        elif not tile.mis[i]:
            care[o:o + tile.caps[i]] = False  # a failed unit may leave a prefix of its words here
    return Refill(tile, stride, n, in_off, out_off, caps_n, order, image, np.ones(stride, dtype=bool), care)
