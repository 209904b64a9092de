"""Model, program generator and corpus for capnp_packed_build_fields_batch.

The model restates the reference's builder in plain Python, function for function:
MessageBuilder.init / allocateBytes / allocateStruct / writeTextPointer / writeStructPointer /
writeListPointer / toBytes (message.zig:1643-2170, makeStructPointer and makeListPointer :29-43,
listContentBytes :65-76) and StructBuilder's writeU8..writeU64, writeBool, writeText, initStruct,
writeData and the primitive list writes (message/struct_builder.zig:332-989). `build_message`
runs the call's own per-message checks first (the table of include/capnp_packed.h), then the
reference sequence. Every decision goes through `_chk(name, cond)`, which records which way it
went: the coverage table of test_build_streams.py is built from that record.

A program is a list of `Op`; a row is one message's values, one entry per op: an int (data
kinds), bytes (TEXT, DATA, LIST_16/32/64), (bytes, count) (LIST_BIT), None (a BUILD_STRUCT op, or
an absent op)."""
import random

# statuses (include/capnp_packed.h)
OK, OUT_OF_SPACE, INVALID_ARGUMENT, MESSAGE_TOO_LARGE, OUT_OF_BOUNDS, LIST_TOO_LARGE = 0, 4, 5, 11, 18, 22

# kinds
U8, U16, U32, U64, BOOL, TEXT, DATA, LIST_BIT, LIST_16, LIST_32, LIST_64 = range(11)
STRUCT = 16
ABSENT = 0xFFFFFFFFFFFFFFFF
MAX_OPS, MAX_WORDS = 32, 64
WIDTH = {U8: 1, U16: 2, U32: 4, U64: 8}
ELEMENT_SIZE = {TEXT: 2, DATA: 2, LIST_BIT: 1, LIST_16: 3, LIST_32: 4, LIST_64: 5}
SLICES = tuple(ELEMENT_SIZE)
M64 = (1 << 64) - 1


class Op:
    """capnp_packed_build_op"""

    def __init__(self, kind, offset=0, bit=0, target=0, dw=0, pw=0, reserved=(0, 0, 0)):
        self.kind, self.offset, self.bit, self.target, self.dw, self.pw = kind, offset, bit, target, dw, pw
        self.reserved = tuple(reserved)

    def __repr__(self):
        return f"Op({self.kind}, {self.offset}, bit={self.bit}, target={self.target}, dw={self.dw}, pw={self.pw})"


SEEN = set()  # (check name, which way it went)


def _chk(name, cond):
    cond = bool(cond)
    SEEN.add((name, cond))
    return cond


# every check of the model; the coverage test wants both ways of each
CHECKS = (
    "host.too_many_ops", "host.no_ops", "host.op0_not_struct", "host.unknown_kind", "host.bit", "host.reserved",
    "host.target", "host.pointer_index", "host.slot_taken", "host.words",
    "msg.misaligned", "op.absent", "list.width", "bit.length", "count.too_large", "slice.bounds",
    "msg.too_large", "msg.space", "msg.sizes_only",
    "data.dropped", "bool.dropped", "bool.value", "text.padding", "list.padding", "struct.empty",
)


# ---------------------------------------------------------------------------
# the reference builder, segment 0 only
# ---------------------------------------------------------------------------
def encode_offset_words(off):  # message.zig:20-27
    assert -(1 << 29) <= off < (1 << 29)
    return (1 << 30) + off if off < 0 else off


def make_struct_pointer(off, dw, pw):  # :29-35
    return (encode_offset_words(off) << 2) | (dw << 32) | (pw << 48)


def make_list_pointer(off, size, count):  # :37-43
    return 1 | (encode_offset_words(off) << 2) | (size << 32) | (count << 35)


def list_content_bytes(size, count):  # :65-76
    return {0: 0, 1: (count + 7) // 8, 2: count, 3: count * 2, 4: count * 4, 5: count * 8}[size]


class RefBuilder:
    """MessageBuilder with one segment."""

    def __init__(self):  # :1649-1654
        self.seg = bytearray()

    def _put64(self, pos, v):
        self.seg[pos:pos + 8] = v.to_bytes(8, "little")

    def allocate_bytes(self, n):  # :1701-1707
        off = len(self.seg)
        self.seg += bytes(n)
        return off

    def allocate_struct(self, dw, pw):  # :2061-2101, the first allocation
        assert len(self.seg) == 0
        self.allocate_bytes(8)
        self._put64(0, (dw << 32) | (pw << 48))  # :2076-2087
        return RefStruct(self, self.allocate_bytes(8 * (dw + pw)), dw, pw)

    def write_text_pointer(self, pointer_pos, text):  # :1780-1815
        padding = (8 - ((len(text) + 1) % 8)) % 8
        _chk("text.padding", padding != 0)
        text_offset = len(self.seg)
        self.seg += text + b"\0" + bytes(padding)
        rel = (text_offset - pointer_pos - 8) // 8
        self._put64(pointer_pos, make_list_pointer(rel, 2, len(text) + 1))

    def write_struct_pointer(self, pointer_pos, dw, pw):  # :1834-1886
        if _chk("struct.empty", dw == 0 and pw == 0):
            self._put64(pointer_pos, 0)
            return RefStruct(self, pointer_pos, 0, 0)
        off = self.allocate_bytes(8 * (dw + pw))
        self._put64(pointer_pos, make_struct_pointer((off - pointer_pos - 8) // 8, dw, pw))
        return RefStruct(self, off, dw, pw)

    def write_list_pointer(self, pointer_pos, size, count):  # :1909-1948
        assert len(self.seg) % 8 == 0
        total = list_content_bytes(size, count)
        off = self.allocate_bytes(total)
        padding = (8 - (total % 8)) % 8
        if _chk("list.padding", padding != 0):
            self.allocate_bytes(padding)
        self._put64(pointer_pos, make_list_pointer((off - pointer_pos - 8) // 8, size, count))
        return off

    def to_bytes(self):  # :2123-2170, one segment: count - 1 = 0, its words, no padding word
        return (0).to_bytes(4, "little") + (len(self.seg) // 8).to_bytes(4, "little") + bytes(self.seg)


class RefStruct:
    """StructBuilder (message/struct_builder.zig:332-989)."""

    def __init__(self, b, offset, dw, pw):
        self.b, self.offset, self.dw, self.pw = b, offset, dw, pw

    def write_uint(self, byte_offset, width, value):  # :356-430
        if _chk("data.dropped", byte_offset + width > 8 * self.dw):
            return
        p = self.offset + byte_offset
        self.b.seg[p:p + width] = (value & ((1 << (8 * width)) - 1)).to_bytes(width, "little")

    def write_bool(self, byte_offset, bit, value):  # :449-458
        if _chk("bool.dropped", byte_offset >= 8 * self.dw):
            return
        p = self.offset + byte_offset
        if _chk("bool.value", value):
            self.b.seg[p] |= 1 << bit
        else:
            self.b.seg[p] &= ~(1 << bit) & 0xFF

    def _pointer_pos(self, index):  # :489-493
        assert index < self.pw  # PointerIndexOutOfBounds: the call checks this on the host
        return self.offset + 8 * self.dw + 8 * index

    def write_text(self, index, text):  # :479-495
        self.b.write_text_pointer(self._pointer_pos(index), text)

    def init_struct(self, index, dw, pw):  # :497-518
        return self.b.write_struct_pointer(self._pointer_pos(index), dw, pw)

    def write_list(self, index, size, count, content):  # :534-570 and the typed list builders' sets
        off = self.b.write_list_pointer(self._pointer_pos(index), size, count)
        self.b.seg[off:off + len(content)] = content


# ---------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------
def check_ops(ops):
    """The host-side checks that concern the ops: True when the call accepts them."""
    if _chk("host.too_many_ops", len(ops) > MAX_OPS):
        return False
    if _chk("host.no_ops", len(ops) == 0):
        return False
    if _chk("host.op0_not_struct", ops[0].kind != STRUCT):
        return False
    words, slots = 1, set()
    for k, o in enumerate(ops):
        if _chk("host.unknown_kind", o.kind != STRUCT and o.kind > LIST_64):
            return False
        if _chk("host.bit", o.bit > (7 if o.kind == BOOL else 0)):
            return False
        if _chk("host.reserved", any(o.reserved)):
            return False
        if k and _chk("host.target", o.target >= k or ops[o.target].kind != STRUCT):
            return False
        if k and (o.kind == STRUCT or o.kind in SLICES):
            if _chk("host.pointer_index", o.offset >= ops[o.target].pw):
                return False
            if _chk("host.slot_taken", (o.target, o.offset) in slots):
                return False
            slots.add((o.target, o.offset))
        if o.kind == STRUCT:
            words += o.dw + o.pw
            if _chk("host.words", words > MAX_WORDS):
                return False
    return True


def slice_elements(kind, length, count):
    """(status, content bytes with Text's NUL, element count) of a slice entry."""
    if kind == TEXT:
        n = b = length + 1
    elif kind == LIST_BIT:
        if _chk("bit.length", length != (count + 7) // 8):
            return INVALID_ARGUMENT, 0, 0
        n, b = count, length
    elif kind in (LIST_16, LIST_32, LIST_64):
        w = 1 << (kind - LIST_16 + 1)
        if _chk("list.width", length % w != 0):
            return INVALID_ARGUMENT, 0, 0
        n, b = length // w, length
    else:
        n = b = length
    return OK, b, n


def build_message(ops, cols, pool, pool_len=None, out_addr=0, cap=None, sizes_only=False):
    """What the call answers for one message: (status, out_len, bytes or None). cols[k] is op k's
    (value, len, count); pool the bytes slices are taken from; out_addr the address d_out +
    d_out_off[i] (only its low bits matter); cap is d_out_cap[i]."""
    pool_len = len(pool) if pool_len is None else pool_len
    if not _chk("msg.sizes_only", sizes_only) and _chk("msg.misaligned", out_addr % 8 != 0):
        return INVALID_ARGUMENT, 0, None
    seg_words = 1
    for k, o in enumerate(ops):
        if o.kind == STRUCT:
            seg_words += o.dw + o.pw
        elif o.kind in SLICES:
            value, length, count = cols[k]
            if _chk("op.absent", length == ABSENT):
                continue
            st, nbytes, elems = slice_elements(o.kind, length, count)
            if st:
                return st, 0, None
            if _chk("count.too_large", elems >= 1 << 29):
                return LIST_TOO_LARGE, 0, None
            if _chk("slice.bounds", value > pool_len or length > pool_len - value):
                return OUT_OF_BOUNDS, 0, None
            seg_words += (nbytes + 7) // 8
    framed = 8 * (seg_words + 1)
    if _chk("msg.too_large", framed >= 1 << 32):
        return MESSAGE_TOO_LARGE, 0, None
    if not sizes_only and _chk("msg.space", framed > cap):
        return OUT_OF_SPACE, framed, None
    if sizes_only:
        return OK, framed, None
    # the reference sequence
    b = RefBuilder()
    structs = {0: b.allocate_struct(ops[0].dw, ops[0].pw)}
    for k, o in enumerate(ops):
        if k == 0:
            continue
        t = structs[o.target]
        if o.kind == STRUCT:
            structs[k] = t.init_struct(o.offset, o.dw, o.pw)
            continue
        value, length, count = cols[k]
        if length == ABSENT:
            continue
        if o.kind in WIDTH:
            t.write_uint(o.offset, WIDTH[o.kind], value)
        elif o.kind == BOOL:
            t.write_bool(o.offset, o.bit, value & 1)
        elif o.kind == TEXT:
            t.write_text(o.offset, bytes(pool[value:value + length]))
        else:
            _, nbytes, elems = slice_elements(o.kind, length, count)
            content = bytearray(pool[value:value + length])
            if o.kind == LIST_BIT and count % 8:  # BoolListBuilder.set of `count` elements: the rest stay 0
                content[-1] &= (1 << (count % 8)) - 1
            t.write_list(o.offset, ELEMENT_SIZE[o.kind], elems, bytes(content))
    out = b.to_bytes()
    assert len(out) == framed
    return OK, framed, out


# ---------------------------------------------------------------------------
# rows -> pool and columns
# ---------------------------------------------------------------------------
def columns(ops, rows, align=None, pool_pad=0):
    """(pool bytes, cols) for a batch: cols[i][k] = (value, len, count) of op k of message i.
    Slice j of the batch is placed at source alignment align[j % len(align)] mod 16 (default:
    cycling through 0..15), with filler bytes in between."""
    align = list(range(16)) if align is None else align
    pool, cols, j = bytearray(b"\xEE" * pool_pad), [], 0
    for row in rows:
        assert len(row) == len(ops)
        c = []
        for o, v in zip(ops, row):
            if o.kind == STRUCT:
                c.append((0, 0, 0))
            elif v is None:
                c.append((0, ABSENT, 0))
            elif o.kind in SLICES:
                data, count = v if o.kind == LIST_BIT else (v, 0)
                a = align[j % len(align)]
                j += 1
                while len(pool) % 16 != a:
                    pool.append(0xEE)
                c.append((len(pool), len(data), count))
                pool += data
            else:
                c.append((v & M64, 0, 0))
        cols.append(c)
    return bytes(pool), cols


# ---------------------------------------------------------------------------
# generated programs
# ---------------------------------------------------------------------------
def gen_program(rng, n_ops, max_words=MAX_WORDS, max_depth=4):
    """A valid program of n_ops ops: structs nested at most max_depth below the root (so that a
    read_fields path reaches every struct), unique pointer slots, at most max_words words."""
    while True:
        dw, pw = rng.randrange(0, 5), rng.randrange(0, 5)
        if n_ops == 1 or dw + pw:
            break
    ops = [Op(STRUCT, dw=dw, pw=pw)]
    depth = {0: 0}
    free = {0: list(range(pw))}
    words = 1 + dw + pw
    while len(ops) < n_ops:
        k = len(ops)
        targets = list(depth)
        t = rng.choice(targets)
        want_ptr = rng.random() < 0.5
        if want_ptr and free[t]:
            slot = free[t].pop(rng.randrange(len(free[t])))
            if rng.random() < 0.3 and depth[t] < max_depth:
                dw, pw = rng.randrange(0, 4), rng.randrange(0, 4)
                if words + dw + pw > max_words:
                    dw = pw = 0
                ops.append(Op(STRUCT, slot, target=t, dw=dw, pw=pw))
                words += dw + pw
                depth[k], free[k] = depth[t] + 1, list(range(pw))
            else:
                ops.append(Op(rng.choice(SLICES), slot, target=t))
        else:
            kind = rng.choice((U8, U16, U32, U64, BOOL))
            # mostly inside the data section, sometimes straddling a word or past the end
            offset = rng.randrange(0, 8 * ops[t].dw + 10)
            ops.append(Op(kind, offset, bit=rng.randrange(8) if kind == BOOL else 0, target=t))
    return ops


def gen_slice(rng, kind, length):
    """A slice of about `length` bytes for `kind` (rounded down to the element width)."""
    if kind == LIST_BIT:
        count = max(0, 8 * length - rng.randrange(8)) if length else 0
        return bytes(rng.randrange(256) for _ in range((count + 7) // 8)), count
    if kind in (LIST_16, LIST_32, LIST_64):
        length -= length % (1 << (kind - LIST_16 + 1))
    if kind == TEXT:
        return bytes(rng.randrange(1, 256) for _ in range(length))
    return bytes(rng.randrange(256) for _ in range(length))


def gen_row(rng, ops, lengths, absent=0.2):
    row = []
    for o in ops:
        if o.kind == STRUCT:
            row.append(None)
        elif rng.random() < absent:
            row.append(None)
        elif o.kind in SLICES:
            row.append(gen_slice(rng, o.kind, rng.choice(lengths)))
        else:
            row.append(rng.getrandbits(64))
    return row


def paths(ops):
    """per op: the pointer indices from the root to the struct it writes into (its target)."""
    own = {0: ()}
    out = []
    for k, o in enumerate(ops):
        if k and o.kind == STRUCT:
            own[k] = own[o.target] + (o.offset,)
        out.append(own[o.target] if k else ())
    return out


SHORT_LENGTHS = list(range(0, 42))
EDGE_LENGTHS = [255, 256, 257, 511, 512, 513, 4095, 4096, 4097]

# five seeds, with the bytes they must give (test_build_streams.py
# derives each word)
SEED_A = ([Op(STRUCT, dw=1, pw=1), Op(U32, 0), Op(TEXT, 0)], [None, 0x11223344, b"hi"])
SEED_B = ([Op(STRUCT, dw=0, pw=2), Op(STRUCT, 1, target=0, dw=1, pw=0), Op(U8, 7, target=1),
           Op(DATA, 0, target=0), Op(BOOL, 0, bit=3, target=1)],
          [None, None, 0xAB, bytes(range(1, 10)), 1])
SEED_C = ([Op(STRUCT, dw=0, pw=1), Op(TEXT, 0)], [None, b""])
SEED_D = ([Op(STRUCT, dw=0, pw=1), Op(DATA, 0)], [None, b""])
SEED_E = ([Op(STRUCT, dw=1, pw=2), Op(STRUCT, 0, target=0, dw=0, pw=0), Op(U16, 6), Op(LIST_BIT, 1)],
          [None, None, 0xBEEF, (b"\xFF\xFF", 11)])


def corpus(seed=0x5EED, programs=40, rows=6):
    """[(ops, rows)]: the seeds, then generated programs of 1..32 ops with rows over the short
    and the edge lengths."""
    rng = random.Random(seed)
    out = [(s[0], [s[1]]) for s in (SEED_A, SEED_B, SEED_C, SEED_D, SEED_E)]
    for i in range(programs):
        ops = gen_program(rng, 1 + (i * 31) // max(1, programs - 1))
        lengths = SHORT_LENGTHS + (EDGE_LENGTHS if i % 4 == 0 else [])
        out.append((ops, [gen_row(rng, ops, lengths) for _ in range(rows)]))
    return out
