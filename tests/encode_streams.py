"""Adversarial and class-edge inputs for the default batch encoders (capnp_packed_encode_batch /
capnp_packed_encoded_size_batch under the Zig rule: encode_stream_kernel, encode_kernel,
long_tiles_kernel + tile_encode_kernel, behind class_scatter_kernel<4>), with
the oracle's verdict on each unit (oracle.pack, message.zig:200-271). CPU only: numpy and
`oracle`; tests/test_encode_streams.py judges these inputs on the CPU and
tests/test_gpu_encode_adversarial.py feeds them to the device.

Word language (pyref_cxx's, made with numpy here): A has no zero byte, B one, C two (six
non-zero bytes), Z is all zero. Under the Zig rule a zero run is Z words, a literal run is an A
word and the A words after it; both end after 256 words.

Every builder is deterministic and cached; nothing here is modified after it is built. A batch
is laid out as the device sees it: the units in one input buffer (IN_PAD bytes at both ends,
every unit at 0 or 8 mod 16 plus its misalignment, the gap after a unit filled so that it would
continue the unit's last word: zero bytes after a Z word, non-zero bytes otherwise), and a slot
per unit at a chosen `address & 15` with FRONT sentinel bytes before it and BACK after its
capacity.
"""
import collections
import functools

import numpy as np

import oracle

SENT = 0xA5
FRONT = 64    # sentinel bytes before each slot
BACK = 64     # sentinel bytes after each slot's capacity
IN_PAD = 64   # padding at both ends of the input buffer
FILL = 0x33   # a non-zero filler between units
TILE = 512            # words per tile: a valid unit of more is long
SMALL_WORDS = 64      # a valid unit of at most 64 words is small
BIN_TOPS = (8, 16, 32, 64)  # the small bins (unit_class<4>)
HUGE_BYTES = 65536    # a long unit of more input bytes is huge
CLASS_BLOCK = 1024    # units per class block (class_scatter_kernel)
SEED = 0xE5C0DE

# exp[i]: the unit's own verdict whatever its slot: status, packed length, packed bytes
Exp = collections.namedtuple("Exp", "st need ref")
# in_off / out_off are relative to the 256-B aligned bases of the device tensors
Batch = collections.namedtuple("Batch", "units kinds mis caps exp in_off in_end out_off out_end")


def encode_bound(n):
    """capnp_packed_encode_bound."""
    return 10 * (n // 8) + 16


# ---- words ---------------------------------------------------------------------------------

_KIND = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate("ABCZ"):
    _KIND[ord(_c)] = _i


def letters(s, k0=0):
    """One word per letter of s (A, B, C, Z); word k is pyref_cxx's word_a/b/c(k0 + k)."""
    n = len(s)
    if n == 0:
        return b""
    kind = _KIND[np.frombuffer(s.encode(), dtype=np.uint8)]
    k = np.arange(k0, k0 + n)
    w = (1 + (k[:, None] + np.arange(8)[None, :]) % 255).astype(np.uint8)
    rows = np.arange(n)
    bc = (kind == 1) | (kind == 2)
    w[rows[bc], k[bc] % 8] = 0
    c = kind == 2
    w[rows[c], (k[c] + 3) % 8] = 0
    w[kind == 3] = 0
    return w.tobytes()


def spell(spec):
    """'C*5 Z*256 A' -> 'CCCCCZZ...ZA'."""
    out = []
    for tok in spec.split():
        name, _, cnt = tok.partition("*")
        out.append(name * (int(cnt) if cnt else 1))
    return "".join(out)


def words(spec):
    return letters(spell(spec))


def rep(p, n):
    return (p * (n // len(p) + 1))[:n]


PATTERNS = collections.OrderedDict([
    ("A", lambda n: "A" * n),
    ("B", lambda n: "B" * n),
    ("C", lambda n: "C" * n),
    ("Z", lambda n: "Z" * n),
    ("ZA", lambda n: rep("ZA", n)),
    ("AC", lambda n: rep("AC", n)),
    ("CA*", lambda n: ("C" + "A" * n)[:n]),
    ("A*Z", lambda n: "A" * (n - 1) + "Z" if n else ""),
    ("Z*A", lambda n: "Z" * (n - 1) + "A" if n else ""),
    ("AAZZ", lambda n: rep("AAZZ", n)),
    ("CAAAB", lambda n: rep("CAAAB", n)),
    ("ZZZC", lambda n: rep("ZZZC", n)),
])


def random_words(rng, nw, density):
    """nw words of random non-zero bytes, each byte zero with probability `density`."""
    b = rng.integers(1, 256, nw * 8, dtype=np.uint8)
    if density >= 1:
        b[:] = 0
    elif density > 0:
        b[rng.random(nw * 8) < density] = 0
    return b.tobytes()


# ---- the reference's verdict ----------------------------------------------------------------

_PACK = {}


def verdict(u, mis=0):
    """Exp of a unit whose input starts `mis` bytes off an 8-B boundary: INVALID_ARGUMENT first
    (the batch contract's word-side alignment), else packPacked's result (message.zig:200-271:
    INVALID_MESSAGE_SIZE for a length that is no multiple of 8)."""
    if mis:
        return Exp(oracle.INVALID_ARGUMENT, 0, b"")
    e = _PACK.get(u)
    if e is None:
        st, p = oracle.pack(u)
        e = _PACK[u] = Exp(st, len(p), p)
    return e


def outcome(e, cap):
    """(status, out_len) the encode batch owes for a unit of verdict e in a slot of cap bytes."""
    if e.st != oracle.OK:
        return e.st, 0
    if e.need > cap:
        return oracle.OUT_OF_SPACE, e.need
    return oracle.OK, e.need


# ---- classes (unit_class<4>, class_scatter_kernel<4>) -------------------------------------------

def unit_class(u, mis=0):
    """'long' / 'huge' / 'mid', or the small bin 0 .. 3 (error units: bin 0)."""
    valid = not mis and len(u) % 8 == 0
    w = len(u) // 8
    if valid and w > TILE:
        return "huge" if len(u) > HUGE_BYTES else "long"
    if not valid:
        return 0
    if w > SMALL_WORDS:
        return "mid"
    return (w > 8) + (w > 16) + (w > 32)


def small_list(b):
    """The small list of a batch: its small units by (class block, length bin, batch order)."""
    rows = [(i // CLASS_BLOCK, c, i) for i, c in enumerate(unit_class(u, m) for u, m in zip(b.units, b.mis))
            if isinstance(c, int)]
    return [i for _, _, i in sorted(rows)]


# ---- layout and the per-unit contract -------------------------------------------------------

def make_batch(units, kinds, caps, in_phase, slot_phase, mis=None):
    """in_phase[i]: 0 or 8, the unit's `address & 15` before its misalignment mis[i] (0 .. 7);
    slot_phase[i]: the slot's `address & 15`."""
    n = len(units)
    mis = [0] * n if mis is None else list(mis)
    assert len(kinds) == len(caps) == len(in_phase) == len(slot_phase) == len(mis) == n
    in_off = np.zeros(n, dtype=np.int64)
    out_off = np.zeros(n, dtype=np.int64)
    pos, o = IN_PAD, 0
    for i, u in enumerate(units):
        pos += (int(in_phase[i]) + mis[i] - pos) % 16
        in_off[i] = pos
        pos += len(u)
        o += FRONT
        o += (int(slot_phase[i]) - o) % 16
        out_off[i] = o
        o += int(caps[i]) + BACK
    exp = [verdict(u, m) for u, m in zip(units, mis)]
    return Batch(list(units), list(kinds), mis, [int(c) for c in caps], exp, in_off, pos, out_off, o)


def input_buffer(b):
    """The input bytes of a batch as laid out; in_end + IN_PAD bytes."""
    buf = np.full(b.in_end + IN_PAD, FILL, dtype=np.uint8)
    n = len(b.units)
    for i, u in enumerate(b.units):
        o = int(b.in_off[i])
        buf[o:o + len(u)] = np.frombuffer(u, dtype=np.uint8)
        if len(u) >= 8 and not any(u[-8:]):
            buf[o + len(u):int(b.in_off[i + 1]) if i + 1 < n else buf.size] = 0
    return buf


def output_bytes(b):
    return b.out_end + FRONT


def in_bytes(b):
    return sum(len(u) for u in b.units)


def check(b, out, out_len, status):
    """The per-unit contract of an encoded batch (out: the output buffer after the call, SENT
    before it; out_len and status -1 before it). out None: the sizes-only call, which knows no
    slot: a valid unit is OK with the oracle's length.
      valid and fits     OK, the oracle's length and bytes, [out_len, cap) still SENT;
      valid, too small   OUT_OF_SPACE, the oracle's length, the slot's content unspecified;
      error units        their status, length 0, the slot untouched;
      always             nothing outside [slot, slot + cap) changes, and every status and out_len
                         entry has been written.
    Returns the set of statuses expected (and met)."""
    n = len(b.units)
    assert len(out_len) == n and len(status) == n
    want = [outcome(e, c) if out is not None else (e.st, e.need if e.st == oracle.OK else 0)
            for e, c in zip(b.exp, b.caps)]
    wst = np.array([w[0] for w in want], dtype=np.int64)
    wln = np.array([w[1] for w in want], dtype=np.int64)
    st, ol = np.asarray(status).astype(np.int64), np.asarray(out_len).astype(np.int64)
    bad = np.flatnonzero(st != wst)
    assert bad.size == 0, ("status", int(bad.size), describe(b, int(bad[0])), int(st[bad[0]]), int(wst[bad[0]]))
    bad = np.flatnonzero(ol != wln)
    assert bad.size == 0, ("out_len", int(bad.size), describe(b, int(bad[0])), int(ol[bad[0]]), int(wln[bad[0]]))
    if out is not None:
        assert out.size == output_bytes(b)
        image = np.full(out.size, SENT, dtype=np.uint8)
        care = np.ones(out.size, dtype=bool)
        for i, (s, ln) in enumerate(want):
            o = int(b.out_off[i])
            if s == oracle.OK:
                image[o:o + ln] = np.frombuffer(b.exp[i].ref, dtype=np.uint8)
            elif s == oracle.OUT_OF_SPACE:
                care[o:o + b.caps[i]] = False
        wrong = np.flatnonzero((out != image) & care)
        if wrong.size:
            at = int(wrong[0])
            i = max(int(np.searchsorted(b.out_off, at + FRONT, side="right")) - 1, 0)
            o = int(b.out_off[i])
            where = ("before the slot" if at < o else "in the packed bytes" if at < o + wln[i] else
                     "in [out_len, cap)" if at < o + b.caps[i] else "past cap")
            raise AssertionError(("byte", int(wrong.size), describe(b, i), where, "slot offset", at - o,
                                  "got", int(out[at]), "want", int(image[at])))
    return {int(s) for s in wst}


def describe(b, i):
    return dict(unit=i, kind=b.kinds[i], in_len=len(b.units[i]), mis=b.mis[i], cap=b.caps[i], need=b.exp[i].need,
                in_phase=int(b.in_off[i]) & 15, slot_phase=int(b.out_off[i]) & 15)


# ---- the packed bytes, walked ---------------------------------------------------------------

def record_starts(p):
    """(position, tag) of every record of a valid packed stream (small_streams.record_starts)."""
    i, n, out = 0, len(p), []
    while i < n:
        t = p[i]
        out.append((i, t))
        if t == 0:
            i += 2
        elif t == 0xFF:
            i += 10 + 8 * p[i + 9]
        else:
            i += 1 + bin(t).count("1")
    return out


def runs(p):
    """(zero runs, literal runs) of a packed stream, in words: a 00 record is count + 1 Z words, an
    FF record 1 + count A words, and a record that follows a full one (count 255) of its kind
    continues its run."""
    zr, lr = [], []
    prev = None  # (tag, count) of the previous record
    for pos, t in record_starts(p):
        if t == 0 or t == 0xFF:
            c = p[pos + 1] if t == 0 else p[pos + 9]
            into = zr if t == 0 else lr
            if prev == (t, 255):
                into[-1] += c + 1
            else:
                into.append(c + 1)
            prev = (t, c)
        else:
            prev = None
    return zr, lr


def literal_counts(p):
    """(cpos, end) of every FF record: the offset of its count byte and of the byte after its
    last literal word (where the output stands when encode_stream_kernel patches the count)."""
    return [(pos + 9, pos + 10 + 8 * p[pos + 9]) for pos, t in record_starts(p) if t == 0xFF]


def coverage(b):
    """Counter over the OK units of a batch, from the oracle's bytes and the slots' phases:
      ("tag", k)  a tag byte at chunk position k = (out_off + pos) & 15
      ("lit", k)  the first byte of a literal word (after an FF record's count) at k
      ("count", k) an FF record's count byte at k
      "same" / "later"  count bytes whose run ends in the same 16-B chunk / in a later one
      ("zrun", r) / ("lrun", r)  zero / literal runs of exactly r words, r in 1, 255, 256, 257."""
    cov = collections.Counter()
    per = {}
    for i, e in enumerate(b.exp):
        if e.st != oracle.OK or e.need > b.caps[i]:
            continue
        got = per.get(e.ref)
        if got is None:
            starts = record_starts(e.ref)
            tags = np.array([pos for pos, _ in starts], dtype=np.int64)
            lc = literal_counts(e.ref)
            lits = np.array([cp + 1 + 8 * j for cp, end in lc for j in range((end - cp - 1) // 8)], dtype=np.int64)
            zr, lr = runs(e.ref)
            rr = [("zrun", r) for r in zr if r in (1, 255, 256, 257)] + \
                 [("lrun", r) for r in lr if r in (1, 255, 256, 257)]
            got = per[e.ref] = (tags, lits, np.array(lc, dtype=np.int64).reshape(-1, 2), rr)
        tags, lits, lc, rr = got
        da = int(b.out_off[i]) & 15
        for name, arr in (("tag", tags), ("lit", lits), ("count", lc[:, 0])):
            for k, c in zip(*np.unique((da + arr) & 15, return_counts=True)):
                cov[(name, int(k))] += int(c)
        same = int((((da + lc[:, 0]) >> 4) == ((da + lc[:, 1]) >> 4)).sum())
        cov["same"] += same
        cov["later"] += len(lc) - same
        for r in rr:
            cov[r] += 1
    return cov


# ---- the batches of tests/test_gpu_encode_adversarial.py ----------------------------------------

SLACK = (0, 1, 16, 41)  # capacity over the need, by turns


@functools.lru_cache(maxsize=None)
def lattice_shapes():
    """(pattern name, words, bytes) for 0 .. 66 words of every pattern: 804 shapes."""
    return [(name, n, letters(f(n))) for n in range(SMALL_WORDS + 3) for name, f in PATTERNS.items()]


EXTREMES = 128  # units per (bin, input phase) of the lattice's all-A / all-Z stretches


@functools.lru_cache(maxsize=None)
def small_lattice():
    """Every lattice shape at both input phases and every slot phase, all fitting their slots
    (25.7k units); then, per small bin and input phase, EXTREMES units of the bin's top length
    that alternate all-A and all-Z: whole waves of encode_stream_kernel whose even lanes complete
    a chunk every second word and whose odd lanes complete none."""
    units, kinds, caps, ip, sp = [], [], [], [], []
    for inph in (0, 8):
        for slot in range(16):
            for name, n, u in lattice_shapes():
                units.append(u)
                kinds.append(f"{name} x{n}")
                caps.append(verdict(u).need + SLACK[len(units) % 4])
                ip.append(inph)
                sp.append(slot)
    for top in BIN_TOPS:
        a, z = letters("A" * top), letters("Z" * top)
        for inph in (0, 8):
            for j in range(EXTREMES):
                u = z if j % 2 else a
                units.append(u)
                kinds.append(("Z" if j % 2 else "A") + f" x{top} extreme")
                caps.append(verdict(u).need + SLACK[(j // 2) % 4])
                ip.append(inph)
                sp.append((j // 2 + j % 2 * 5) % 16)
    return make_batch(units, kinds, caps, ip, sp)


RUN_LENGTHS = (255, 256, 257, 511, 512, 513)
RUN_SIDES = (64, 256, 504, 512)


def run_heads(N):
    """Heads (C words before a run of N words) that put the run's start on every lane boundary
    of a 512-word tile (a lane owns 8 words), its end on every lane boundary, and its start and
    its end one before, on and one after 64, 256, 504 and 512 words."""
    heads = set(range(0, TILE + 1, 8))
    heads |= {(-N) % 8 + 8 * j for j in range(64)}
    for x in RUN_SIDES:
        for d in (-1, 0, 1):
            heads.add(x + d)
            if x + d - N >= 0:
                heads.add(x + d - N)
    return sorted(heads)


@functools.lru_cache(maxsize=None)
def run_edges():
    """C*head, a run of 255 .. 513 Z or A words, one breaker of each kind, one C word."""
    units, kinds, caps, ip, sp = [], [], [], [], []
    for N in RUN_LENGTHS:
        for L in "ZA":
            for h in run_heads(N):
                for br in "ABCZ":
                    u = letters("C" * h + L * N + br + "C")
                    units.append(u)
                    kinds.append(f"C*{h} {L}*{N} {br} C")
                    k = len(units)
                    caps.append(verdict(u).need + SLACK[k % 4] if k % 7 else encode_bound(len(u)))
                    ip.append(8 * (k // 4 % 2))
                    sp.append(k * 5 % 16)
    return make_batch(units, kinds, caps, ip, sp)


TILE_HEADS = (0, 1, 255, 256, 257, 504, 511, 512, 513)
TILE_RUNS = (1, 8, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1100)


def tile_unit(h, L, N, br):
    """C*h, L*N, the breaker, a tail of C words: 70 of them, or, where that leaves the unit
    under 600 words, as many as bring it to exactly two tiles (it ends on a tile end)."""
    body = h + N + 1
    tail = 70 if body + 70 >= 600 else 2 * TILE - body
    return "C" * h + L * N + br + "C" * tail


@functools.lru_cache(maxsize=None)
def tile_edges():
    """Long units of 2 to 4 tiles with a run placed against the tile bounds (864 units, 6.5 MB)."""
    units, kinds, caps, ip, sp = [], [], [], [], []
    for h in TILE_HEADS:
        for L in "ZA":
            for N in TILE_RUNS:
                for br in "ABCZ":
                    s = tile_unit(h, L, N, br)
                    u = letters(s)
                    units.append(u)
                    kinds.append(f"C*{h} {L}*{N} {br} C*{len(s) - h - N - 1}")
                    k = len(units)
                    caps.append(verdict(u).need + SLACK[k % 4] if k % 5 else encode_bound(len(u)))
                    ip.append(8 * (k // 2 % 2))
                    sp.append(k * 3 % 16)
    return make_batch(units, kinds, caps, ip, sp)


def run_spans(s):
    """(letter, start, end) of every maximal stretch of Z or of A letters of s."""
    out, i = [], 0
    while i < len(s):
        j = i
        while j < len(s) and s[j] == s[i]:
            j += 1
        if s[i] in "ZA":
            out.append((s[i], i, j))
        i = j
    return out


CLASS_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 503, 504, 505, 511, 512,
                 513, 520, 1023, 1024, 1025, 1536, 1537, 8191, 8192, 8193)
DENSITIES = (0.0, 0.1, 0.5, 0.9, 1.0)
ERROR_WORDS = (5, 200, 700)  # error units in the small, the mid and the long range


@functools.lru_cache(maxsize=None)
def class_edges(seed=SEED + 1):
    """Every class-edge length at both input phases and five zero densities; nine error units
    (a length that is no multiple of 8, a start that is no multiple of 8, both: each in the
    small, mid and long range) and an empty unit at a misaligned start."""
    rng = np.random.default_rng(seed)
    units, kinds, caps, ip, sp, mis = [], [], [], [], [], []

    def add(u, kind, cap, inph, m=0):
        units.append(u)
        kinds.append(kind)
        caps.append(cap)
        ip.append(inph)
        sp.append(int(rng.integers(0, 16)))
        mis.append(m)

    for nw in CLASS_LENGTHS:
        for inph in (0, 8):
            for d in DENSITIES:
                u = random_words(rng, nw, d)
                k = len(units)
                add(u, f"{nw} words p={d}", verdict(u).need + SLACK[k % 4] if k % 3 else encode_bound(len(u)), inph)
    for nw in ERROR_WORDS:
        u = random_words(rng, nw + 1, 0.1)
        add(u[:8 * nw + 4], f"{nw} words + 4 bytes", encode_bound(8 * nw + 8), 8)
        add(u[:8 * nw], f"{nw} words at 4 mod 8", encode_bound(8 * nw), 0, 4)
        add(u[:8 * nw + 5], f"{nw} words + 5 bytes at 3 mod 8", encode_bound(8 * nw + 8), 8, 3)
    add(b"", "empty at 5 mod 8", 16, 0, 5)
    return make_batch(units, kinds, caps, ip, sp, mis)


CUT_PHASES = (0, 1, 7, 8, 9, 15)
CUT_SMALL = [(name, n) for n in (1, 2, 3, 5, 8, 9, 16, 17) for name in ("A", "C", "ZA", "CA*", "A*Z")] + \
            [("A", 33), ("CAAAB", 40)]
CUT_MID = [(name, n) for n in (65, 100, 200, 257, 400, 512) for name in ("CAAAB", "AAZZ")]
CUT_C_TILES = (3583, 3584, 3585, 7167, 7168, 7169)  # around one and two all-C tiles of 3584 bytes
CUT_LONG_C = (1024, 1100, 1536)
CUT_LONG_RUN = ("C*400 A*300 C*400", "C*500 Z*100 A*600 C*100", "C*300 Z*700 A*40 C*200")


@functools.lru_cache(maxsize=None)
def cap_cuts():
    """Units in slots that cut them: small units at every capacity 0 .. need + 1 and six slot
    phases; mid units at 0, 1, need - 1, need, need + 1 and a stride of 97 between; all-C long
    units (a tile is 3584 packed bytes) around the tile ends and the need; long units with a
    run across a tile bound at a stride of 211."""
    units, kinds, caps, ip, sp = [], [], [], [], []

    def add(u, kind, cap_list, phases, inph):
        for ph in phases:
            for c in cap_list:
                units.append(u)
                kinds.append(kind)
                caps.append(c)
                ip.append(inph)
                sp.append(ph)

    for j, (name, n) in enumerate(CUT_SMALL):
        u = letters(PATTERNS[name](n))
        add(u, f"small {name} x{n}", range(0, verdict(u).need + 2), CUT_PHASES, 8 * (j % 2))
    for j, (name, n) in enumerate(CUT_MID):
        u = letters(PATTERNS[name](n))
        need = verdict(u).need
        add(u, f"mid {name} x{n}", sorted({0, 1, need - 1, need, need + 1} | set(range(97, need - 1, 97))),
            (CUT_PHASES[j % 6],), 8 * (j % 2))
    for j, n in enumerate(CUT_LONG_C):
        u = letters("C" * n)
        need = verdict(u).need
        assert need == 7 * n
        add(u, f"long C x{n}", sorted({0, 1, need - 1, need, need + 1} | {c for c in CUT_C_TILES if c <= need + 1}),
            (CUT_PHASES[j % 6], CUT_PHASES[(j + 3) % 6]), 8 * (j % 2))
    for j, spec in enumerate(CUT_LONG_RUN):
        u = words(spec)
        need = verdict(u).need
        add(u, f"long {spec}", sorted({need - 1, need} | set(range(0, need + 1, 211))), (CUT_PHASES[(j + 1) % 6],),
            8 * (j % 2))
    return make_batch(units, kinds, caps, ip, sp)


SMALL_ONLY = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
MIXED = SMALL_ONLY + ("minority", "blocks3")
# blocks3: the small bins that class block 0, 1 and 2 hold (an error unit is of bin 0)
BLOCKS3_BINS = ((1, 2, 3), (0, 3), (0, 1, 2))


def _small_unit(rng, shapes, i):
    """A lattice shape in a slot that fits (one in 16: a byte short), now and then an error unit."""
    name, n, u = shapes[int(rng.integers(0, len(shapes)))]
    mis = 0
    if i % 53 == 17:
        u, name, mis = (u + b"\x01\x02\x03\x04", name + " + 4 bytes", 0) if i % 2 else (u, name + " at 2 mod 8", 2)
    need = verdict(u, mis).need
    cap = need - 1 if (i % 16 == 5 and need) else need + int(rng.integers(0, 20))
    return u, f"{name} x{n}", cap, mis


@functools.lru_cache(maxsize=None)
def mixed_batch(key, seed=SEED + 2):
    """key n (SMALL_ONLY): n small units. "minority": every fifth unit small between mid units,
    some long units and one huge one, so no class list is the identity. "blocks3": three class
    blocks of small units (a mid unit now and then), each without some of the length bins."""
    rng = np.random.default_rng(seed + (key if isinstance(key, int) else len(key)))
    shapes = [s for s in lattice_shapes() if s[1] <= SMALL_WORDS]
    units, kinds, caps, ip, sp, mis = [], [], [], [], [], []

    def add(u, kind, cap, m=0):
        units.append(u)
        kinds.append(kind)
        caps.append(cap)
        ip.append(8 * int(rng.integers(0, 2)))
        sp.append(int(rng.integers(0, 16)))
        mis.append(m)

    def other(nw, kind, i):
        u = random_words(rng, nw, DENSITIES[i % 5])
        need = verdict(u).need
        add(u, f"{kind} {nw} words", need - 1 if i % 12 == 7 and need else need + int(rng.integers(0, 30)))

    if isinstance(key, int):
        for i in range(key):
            add(*_small_unit(rng, shapes, i))
    elif key == "minority":
        for i in range(640):
            if i % 5 == 2:
                add(*_small_unit(rng, shapes, i))
            elif i == 333:
                other(8200, "huge", i)
            elif i % 20 == 9:
                other(int(rng.integers(513, 3000)), "long", i)
            else:
                other(int(rng.integers(65, 513)), "mid", i)
    else:
        assert key == "blocks3"
        by_bin = [[s for s in shapes if unit_class(s[2]) == b] for b in range(4)]
        for blk, bins in enumerate(BLOCKS3_BINS):
            for j in range(CLASS_BLOCK):
                i = blk * CLASS_BLOCK + j
                if j % 97 == 41:
                    other(int(rng.integers(65, 300)), "mid", i)
                    continue
                pool = by_bin[bins[int(rng.integers(0, len(bins)))]]
                name, n, u = pool[int(rng.integers(0, len(pool)))]
                need = verdict(u).need
                add(u, f"{name} x{n}", need - 1 if (i % 16 == 5 and need) else need + int(rng.integers(0, 20)))
    return make_batch(units, kinds, caps, ip, sp, mis)


BUILDERS = collections.OrderedDict([
    ("small_lattice", small_lattice), ("run_edges", run_edges), ("tile_edges", tile_edges),
    ("class_edges", class_edges), ("cap_cuts", cap_cuts)])
# the statuses each builder's units must end with
STATUSES = {
    "small_lattice": {oracle.OK},
    "run_edges": {oracle.OK},
    "tile_edges": {oracle.OK},
    "class_edges": {oracle.OK, oracle.INVALID_MESSAGE_SIZE, oracle.INVALID_ARGUMENT},
    "cap_cuts": {oracle.OK, oracle.OUT_OF_SPACE},
    "mixed": {oracle.OK, oracle.OUT_OF_SPACE, oracle.INVALID_MESSAGE_SIZE, oracle.INVALID_ARGUMENT},
}


def statuses(b):
    return {int(outcome(e, c)[0]) for e, c in zip(b.exp, b.caps)}
