"""Model and corpus for capnp_packed_read_fields_batch.

The model restates the reference's read path in plain Python, function for function:
Message.init (message.zig:341-394), getRootStruct (:973-985), resolvePointer /
resolveStructPointer / resolveListPointer (:451-561), StructReader's data reads (:1051-1158),
resolveListPointerAt, readStruct, the typed slice reads and readText (:1187-1443). Errors are
exceptions carrying the C-ABI status, raised where the reference raises them, so the first error
is the result. Every decision the model takes goes through `_chk(name, cond)`, which records
which way it went: the coverage table of test_struct_streams.py is built from that record.

The builder lays messages out by hand (near, single-far and double-far pointers, far chains,
any number of segments), and `corpus()` is the list of messages the CPU and GPU tests share."""
import os
import struct as _struct

# statuses (include/capnp_packed.h)
OK, INVALID_ARGUMENT = 0, 5
END_OF_STREAM, INVALID_SEGMENT_COUNT, SEGMENT_COUNT_LIMIT_EXCEEDED = 8, 9, 10
TRUNCATED_MESSAGE, EMPTY_MESSAGE, NESTING_LIMIT_EXCEEDED, INVALID_SEGMENT_ID = 13, 14, 15, 16
INVALID_POINTER, OUT_OF_BOUNDS, INVALID_FAR_POINTER = 17, 18, 20

# kinds
U8, U16, U32, U64, BOOL, TEXT, DATA, LIST_BIT, LIST_16, LIST_32, LIST_64 = range(11)
WIDTH = {U8: 1, U16: 2, U32: 4, U64: 8, BOOL: 1}
ELEMENT_SIZE = {TEXT: 2, DATA: 2, LIST_BIT: 1, LIST_16: 3, LIST_32: 4, LIST_64: 5}
MAX_SEGMENTS = 512


class F:
    """A field descriptor (capnp_packed_field)."""

    def __init__(self, kind, offset, bit=0, path=()):
        self.kind, self.offset, self.bit, self.path = kind, offset, bit, tuple(path)

    def __repr__(self):
        return f"F({self.kind}, {self.offset}, bit={self.bit}, path={self.path})"


class RefError(Exception):
    def __init__(self, status, name):
        super().__init__(name)
        self.status = status


SEEN = set()  # (check name, which way it went)


def _chk(name, cond):
    cond = bool(cond)
    SEEN.add((name, cond))
    return cond


# every check of the model; the coverage test wants both ways of each
CHECKS = (
    "init.short", "init.segcount", "init.seglimit", "init.header_truncated", "init.segment_truncated",
    "root.segment0_short",
    "resolve.depth0", "resolve.is_far", "far.segment_id", "far.pad_bounds", "far.is_double",
    "dfar.first_not_far", "dfar.first_is_double", "dfar.content_segment_id",
    "struct.null", "struct.not_struct", "struct.has_override", "struct.negative", "struct.truncated",
    "step.index", "step.null",
    "data.defaulted", "data.straddles_word",
    "slice.index", "slice.null", "list.null_resolved", "list.not_list", "list.has_override", "list.negative",
    "list.bounds", "slice.element_size", "text.index", "text.null", "text.element_size", "text.trailing_nul",
    "text.empty",
)


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class Msg:
    """Message.init's result: the segments and where each starts in the framed bytes."""

    def __init__(self, data):
        data = bytes(data)
        if _chk("init.short", len(data) < 4):
            raise RefError(END_OF_STREAM, "EndOfStream")
        (m1,) = _struct.unpack_from("<I", data, 0)
        if _chk("init.segcount", m1 == 0xFFFFFFFF):
            raise RefError(INVALID_SEGMENT_COUNT, "InvalidSegmentCount")
        count = m1 + 1
        if _chk("init.seglimit", count > MAX_SEGMENTS):
            raise RefError(SEGMENT_COUNT_LIMIT_EXCEEDED, "SegmentCountLimitExceeded")
        header = 4 * (1 + count + (1 if count % 2 == 0 else 0))
        if _chk("init.header_truncated", header > len(data)):
            raise RefError(TRUNCATED_MESSAGE, "TruncatedMessage")
        sizes = _struct.unpack_from(f"<{count}I", data, 4)
        self.segments, self.starts = [], []
        off = header
        for words in sizes:
            end = off + 8 * words
            if _chk("init.segment_truncated", end > len(data)):
                raise RefError(TRUNCATED_MESSAGE, "TruncatedMessage")
            self.segments.append(data[off:end])
            self.starts.append(off)
            off = end

    def word(self, seg, pos):
        return _struct.unpack_from("<Q", self.segments[seg], pos)[0]


def offset_words(word):  # decodeOffsetWords (:11-18)
    raw = (word >> 2) & 0x3FFFFFFF
    return raw - (1 << 30) if raw & 0x20000000 else raw


def resolve_pointer(m, seg, pos, word, depth):  # :451-490
    if _chk("resolve.depth0", depth == 0):
        raise RefError(NESTING_LIMIT_EXCEEDED, "PointerDepthLimit")
    if not _chk("resolve.is_far", word & 3 == 2):
        return seg, pos, word, None
    double, pad_words, far_seg = (word >> 2) & 1, (word >> 3) & 0x1FFFFFFF, word >> 32
    if _chk("far.segment_id", far_seg >= len(m.segments)):  # resolveFarLandingPad (:430-437)
        raise RefError(INVALID_SEGMENT_ID, "InvalidSegmentId")
    pad = pad_words * 8
    if _chk("far.pad_bounds", pad + (16 if double else 8) > len(m.segments[far_seg])):
        raise RefError(OUT_OF_BOUNDS, "OutOfBounds")
    if not _chk("far.is_double", double):
        return resolve_pointer(m, far_seg, pad, m.word(far_seg, pad), depth - 1)
    first, tag = m.word(far_seg, pad), m.word(far_seg, pad + 8)
    if _chk("dfar.first_not_far", first & 3 != 2):
        raise RefError(INVALID_FAR_POINTER, "InvalidFarPointer")
    if _chk("dfar.first_is_double", (first >> 2) & 1):
        raise RefError(INVALID_FAR_POINTER, "InvalidFarPointer")
    if _chk("dfar.content_segment_id", (first >> 32) >= len(m.segments)):
        raise RefError(INVALID_SEGMENT_ID, "InvalidSegmentId")
    return first >> 32, 0, tag, ((first >> 3) & 0x1FFFFFFF) * 8


class Struct:
    def __init__(self, seg, offset, data_words, pointers):
        self.seg, self.offset, self.data_words, self.pointers = seg, offset, data_words, pointers


def resolve_struct_pointer(m, seg, pos, word):  # :492-523
    seg, pos, word, override = resolve_pointer(m, seg, pos, word, 8)
    if _chk("struct.null", word == 0):
        raise RefError(INVALID_POINTER, "InvalidRootPointer")
    if _chk("struct.not_struct", word & 3 != 0):
        raise RefError(INVALID_POINTER, "InvalidRootPointer")
    data_words, pointers = (word >> 32) & 0xFFFF, (word >> 48) & 0xFFFF
    if _chk("struct.has_override", override is not None):
        offset = override
    else:
        offset = pos + 8 + offset_words(word) * 8
        if _chk("struct.negative", offset < 0):
            raise RefError(INVALID_POINTER, "InvalidRootPointer")
    if _chk("struct.truncated", offset + 8 * (data_words + pointers) > len(m.segments[seg])):
        raise RefError(TRUNCATED_MESSAGE, "TruncatedMessage")
    return Struct(seg, offset, data_words, pointers)


def resolve_list_pointer(m, seg, pos, word):  # :525-561 -> (segment, content offset, element size, count)
    seg, pos, word, override = resolve_pointer(m, seg, pos, word, 8)
    if _chk("list.null_resolved", word == 0):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    if _chk("list.not_list", word & 3 != 1):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    size, count = (word >> 32) & 7, word >> 35
    if _chk("list.has_override", override is not None):
        content = override
    else:
        content = pos + 8 + offset_words(word) * 8
        if _chk("list.negative", content < 0):  # computeContentOffset (:442-449)
            raise RefError(OUT_OF_BOUNDS, "OutOfBounds")
    nbytes = {0: 0, 1: (count + 7) // 8, 2: count, 3: 2 * count, 4: 4 * count, 5: 8 * count, 6: 8 * count,
              7: 8 * (count + 1)}[size]
    if _chk("list.bounds", content + nbytes > len(m.segments[seg])):
        raise RefError(OUT_OF_BOUNDS, "OutOfBounds")
    return seg, content, size, count


def get_root_struct(m):  # :973-985
    if len(m.segments) == 0:  # (Message.init always lists one: not reachable from framed bytes)
        raise RefError(EMPTY_MESSAGE, "EmptyMessage")
    if _chk("root.segment0_short", len(m.segments[0]) < 8):
        raise RefError(TRUNCATED_MESSAGE, "TruncatedMessage")
    return resolve_struct_pointer(m, 0, 0, m.word(0, 0))


def pointer_at(m, s, index):
    """the pointer section's entry: (position in the segment, word), or None past the section"""
    if 8 * index + 8 > 8 * s.pointers:
        return None
    pos = s.offset + 8 * s.data_words + 8 * index
    return pos, m.word(s.seg, pos)


def read_struct(m, s, index):  # :1224-1235
    p = pointer_at(m, s, index)
    if _chk("step.index", p is None):
        raise RefError(OUT_OF_BOUNDS, "OutOfBounds")
    if _chk("step.null", p[1] == 0):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    return resolve_struct_pointer(m, s.seg, p[0], p[1])


def read_data_kind(m, s, f):  # :1051-1158 -> (value, len, count)
    width = WIDTH[f.kind]
    data = m.segments[s.seg][s.offset:s.offset + 8 * s.data_words]
    if _chk("data.defaulted", f.offset + width > len(data)):
        return 0, 0, 0
    _chk("data.straddles_word", f.offset % 8 + width > 8)
    v = int.from_bytes(data[f.offset:f.offset + width], "little")
    if f.kind == BOOL:
        v = (v >> f.bit) & 1
    return v, width, 1


def read_slice_kind(m, s, f, base=0):  # :1187-1198 + the typed reads; readText :1417-1443 -> (value, len, count)
    p = pointer_at(m, s, f.offset)
    if f.kind == TEXT:
        if _chk("text.index", p is None):
            return 0, 0, 0
        if _chk("text.null", p[1] == 0):
            return 0, 0, 0
    else:
        if _chk("slice.index", p is None):
            raise RefError(OUT_OF_BOUNDS, "OutOfBounds")
        if _chk("slice.null", p[1] == 0):
            raise RefError(INVALID_POINTER, "InvalidPointer")
    seg, content, size, count = resolve_list_pointer(m, s.seg, p[0], p[1])
    if f.kind == TEXT:
        if _chk("text.element_size", size != 2):
            raise RefError(INVALID_POINTER, "InvalidTextPointer")
        nbytes = count
        if not _chk("text.empty", count == 0) and _chk("text.trailing_nul",
                                                       m.segments[seg][content + count - 1] == 0):
            nbytes -= 1
            count -= 1
    else:
        if _chk("slice.element_size", size != ELEMENT_SIZE[f.kind]):
            raise RefError(INVALID_POINTER, "InvalidPointer")
        nbytes = (count + 7) // 8 if size == 1 else count << (size - 2)
    return base + m.starts[seg] + content, nbytes, count


def read_fields(data, fields, base=0):
    """What capnp_packed_read_fields_batch answers for one message at offset `base` of the input
    buffer: a list of (status, value, len, count) per field; a slice's value is base + its offset
    in `data`."""
    try:
        m = Msg(data)
        root = get_root_struct(m)
    except RefError as e:
        return [(e.status, 0, 0, 0)] * len(fields)
    out = []
    for f in fields:
        try:
            s = root
            for index in f.path:
                s = read_struct(m, s, index)
            out.append((OK,) + (read_data_kind(m, s, f) if f.kind in WIDTH else read_slice_kind(m, s, f, base)))
        except RefError as e:
            out.append((e.status, 0, 0, 0))
    return out


# ---------------------------------------------------------------------------
# the builder
# ---------------------------------------------------------------------------
def struct_ptr(offset, data_words, pointers):
    return ((offset & 0x3FFFFFFF) << 2) | (data_words << 32) | (pointers << 48)


def list_ptr(offset, size, count):
    return 1 | ((offset & 0x3FFFFFFF) << 2) | (size << 32) | (count << 35)


def far_ptr(double, pad_words, seg):
    return 2 | (int(double) << 2) | (pad_words << 3) | (seg << 32)


def frame(segments):
    n = len(segments)
    head = _struct.pack(f"<{n + 1}I", n - 1, *(len(s) // 8 for s in segments))
    if n % 2 == 0:
        head += b"\0\0\0\0"
    return head + b"".join(bytes(s) for s in segments)


class Builder:
    """Segments of words; objects are appended, pointers are written by `point`."""

    def __init__(self, nseg):
        self.seg = [[] for _ in range(nseg)]

    def alloc(self, seg, words):
        """append words (ints) to a segment; returns the index of the first"""
        at = len(self.seg[seg])
        self.seg[seg].extend(words)
        return at

    def alloc_bytes(self, seg, raw):
        raw = bytes(raw) + b"\0" * (-len(raw) % 8)
        return self.alloc(seg, list(_struct.unpack(f"<{len(raw) // 8}Q", raw)))

    def point(self, at, to, make, via="near", pad_seg=None, hops=1):
        """write at (seg, word) a pointer to (seg, word). make(offset_words) is the struct / list
        word. via: "near" (same segment), "far" (`hops` single-far hops: the last landing pad holds
        the near pointer and so lies in the target's segment, the others in pad_seg), "dfar" (a
        double-far pad in pad_seg). pad_seg None: the target's segment."""
        (ps, pw), (ts, tw) = at, to
        if via == "near":
            assert ps == ts
            self.seg[ps][pw] = make(tw - pw - 1)
        elif via == "far":
            pad = self.alloc(ts, [0])
            self.seg[ts][pad] = make(tw - pad - 1)
            word = far_ptr(False, pad, ts)
            for h in range(hops - 1):  # further hops, each a far pointer to the one before
                hs = pad_seg if pad_seg is not None else ts
                pad = self.alloc(hs, [word])
                word = far_ptr(False, pad, hs)
            self.seg[ps][pw] = word
        elif via == "dfar":
            hs = pad_seg if pad_seg is not None else ts
            pad = self.alloc(hs, [far_ptr(False, tw, ts), make(0)])
            self.seg[ps][pw] = far_ptr(True, pad, hs)
        else:
            raise ValueError(via)

    def bytes(self):
        return frame([_struct.pack(f"<{len(s)}Q", *s) for s in self.seg])


# The corpus's one schema. Root: 3 data words, 8 pointers:
#   p0 Text, p1 Data, p2 child struct, p3 List(UInt16), p4 List(UInt32), p5 List(Bool), p6 List(UInt64), p7 null
# child (1 data word, 2 pointers): p0 Text, p1 grandchild (1, 1): p0 great-grandchild (1, 1): p0 Text
ROOT_DATA = bytes(range(0x11, 0x11 + 24))
FIELDS = [
    F(U8, 0), F(U8, 23), F(U8, 24), F(U16, 2), F(U16, 7), F(U16, 23), F(U32, 4), F(U32, 6),
    F(U32, 21), F(U64, 8), F(U64, 3), F(U64, 16), F(U64, 17), F(BOOL, 1, 0), F(BOOL, 1, 7), F(BOOL, 24, 3),
    F(TEXT, 0), F(DATA, 1), F(LIST_16, 3), F(LIST_32, 4), F(LIST_BIT, 5), F(LIST_64, 6), F(TEXT, 7), F(DATA, 7),
    F(TEXT, 8), F(DATA, 8), F(U32, 0, path=(2,)), F(TEXT, 0, path=(2,)), F(U16, 0, path=(2, 1)),
    F(U8, 7, path=(2, 1, 0)), F(TEXT, 0, path=(2, 1, 0)), F(DATA, 1, path=(9,)),
]
assert len(FIELDS) == 32


def standard(nseg=1, root="near", root_hops=1, ptrs="near", text=b"hello\0", data=b"\x01\x02\x03\x04\x05",
             home=None, pad_seg=None, edit=None, filler_words=3):
    """The schema above as a message of nseg segments. The root pointer is word 0 of segment 0;
    the root struct and everything it points to live in segment `home` (default: the last).
    root / ptrs: how the root pointer and the root's own pointers are written (near needs
    home == 0 for the root). edit(builder, where) may damage the message afterwards; `where`
    maps names to (segment, word)."""
    b = Builder(nseg)
    home = nseg - 1 if home is None else home
    b.alloc(0, [0])  # the root pointer
    for s in range(nseg):  # every segment holds something that is not zero
        b.alloc(s, [0xF1F1F1F1F1F1F1F1 + s] * filler_words)
    root_at = b.alloc_bytes(home, ROOT_DATA)
    rp = b.alloc(home, [0] * 8)
    where = {"root": (home, root_at), "root_ptrs": (home, rp)}
    b.point((0, 0), (home, root_at), lambda o: struct_ptr(o, 3, 8), via=root, pad_seg=pad_seg, hops=root_hops)

    def slice_(index, raw, size, count, name):
        at = b.alloc_bytes(home, raw)
        where[name] = (home, at)
        b.point((home, rp + index), (home, at), lambda o: list_ptr(o, size, count), via=ptrs, pad_seg=pad_seg)

    slice_(0, text, 2, len(text), "text")
    slice_(1, data, 2, len(data), "data")
    slice_(3, _struct.pack("<3H", 10, 20, 30), 3, 3, "l16")
    slice_(4, _struct.pack("<2I", 1000, 2000), 4, 2, "l32")
    slice_(5, b"\x15\x01", 1, 9, "bits")
    slice_(6, _struct.pack("<2Q", 123456789, 987654321), 5, 2, "l64")
    # child, grandchild, great-grandchild
    child = b.alloc(home, [0xC0FFEE0000000042, 0, 0])
    where["child"] = (home, child)
    b.point((home, rp + 2), (home, child), lambda o: struct_ptr(o, 1, 2), via=ptrs, pad_seg=pad_seg)
    t = b.alloc_bytes(home, b"child text")
    b.point((home, child + 1), (home, t), lambda o: list_ptr(o, 2, 10), via="near")
    grand = b.alloc(home, [0x1234, 0])
    b.point((home, child + 2), (home, grand), lambda o: struct_ptr(o, 1, 1), via="near")
    great = b.alloc(home, [0xAB00000000000000, 0])
    where["great"] = (home, great)
    b.point((home, grand + 1), (home, great), lambda o: struct_ptr(o, 1, 1), via="near")
    t = b.alloc_bytes(home, b"deep\0")
    b.point((home, great + 1), (home, t), lambda o: list_ptr(o, 2, 5), via="near")
    if edit:
        edit(b, where)
    return b.bytes()


def _set(name, index, make):
    """edit: overwrite root pointer `index` (or the word `name` + index) with make(builder, seg, word)"""
    def edit(b, where):
        s, w = where[name]
        b.seg[s][w + index] = make(b, s, w + index)
    return edit


def corpus():
    """[(name, framed bytes)]: every layout and every error unit of the call's contract."""
    out = []

    def add(name, data):
        out.append((name, bytes(data)))

    # ---- Message.init -----------------------------------------------------------------------
    add("empty", b"")
    add("three_bytes", b"\0\0\0")
    add("four_bytes_one_segment", _struct.pack("<I", 0))            # header 8 > 4: truncated
    add("four_bytes_segcount", _struct.pack("<I", 0xFFFFFFFF))
    add("seven_bytes_seglimit", _struct.pack("<I", 512) + b"\0\0\0")
    add("seglimit_513", _struct.pack("<I", 512) + bytes(4 * 513))
    add("header_truncated", _struct.pack("<III", 2, 1, 1) + bytes(4))  # 3 segments need 16 bytes
    add("segment_truncated", frame([bytes(8), bytes(16)])[:-8])
    add("second_segment_truncated_by_a_word", frame([struct_ptr(0, 0, 0).to_bytes(8, "little"), bytes(24)])[:-1])
    add("segment0_empty", frame([b""]))
    add("segment0_empty_of_two", frame([b"", bytes(16)]))
    good = standard()
    add("trailing_bytes_ignored", good + b"\xEE" * 24)
    # ---- layouts ----------------------------------------------------------------------------
    add("one_segment", good)
    for nseg in (2, 3, 5, 512):
        add(f"{nseg}_segments_far_root", standard(nseg, root="far"))
        add(f"{nseg}_segments_dfar_root", standard(nseg, root="dfar", pad_seg=nseg // 2))
    add("5_segments_far_pointers", standard(5, root="far", ptrs="far"))
    add("5_segments_dfar_pointers_pad_in_4", standard(5, root="far", ptrs="dfar", home=2, pad_seg=4))
    add("512_segments_dfar_pointers", standard(512, root="dfar", ptrs="dfar", home=300, pad_seg=511))
    add("2_segments_home_0_far_pointers", standard(2, root="near", ptrs="far", home=0))
    for hops in (1, 7, 8, 9):
        add(f"root_chain_{hops}_hops", standard(3, root="far", root_hops=hops, pad_seg=1))
    add("list_chain_7_hops", standard(2, root="far", edit=lambda b, w: b.point(
        (w["root_ptrs"][0], w["root_ptrs"][1] + 1), w["data"], lambda o: list_ptr(o, 2, 5), via="far", hops=7)))
    add("list_chain_8_hops", standard(2, root="far", edit=lambda b, w: b.point(
        (w["root_ptrs"][0], w["root_ptrs"][1] + 1), w["data"], lambda o: list_ptr(o, 2, 5), via="far", hops=8)))
    add("child_chain_8_hops", standard(2, root="far", edit=lambda b, w: b.point(
        (w["root_ptrs"][0], w["root_ptrs"][1] + 2), w["child"], lambda o: struct_ptr(o, 1, 2), via="far", hops=8)))
    # ---- the root pointer -------------------------------------------------------------------
    root0 = lambda make: standard(edit=lambda b, w: b.seg[0].__setitem__(0, make(b, w)))
    add("root_null", root0(lambda b, w: 0))
    add("root_is_list", root0(lambda b, w: list_ptr(0, 2, 1)))
    add("root_is_capability", root0(lambda b, w: 3))
    add("root_negative", root0(lambda b, w: struct_ptr(-2, 0, 0)))
    add("root_to_word_0", root0(lambda b, w: struct_ptr(-1, 1, 0)))  # the smallest offset that is not negative
    add("root_one_word_too_long", root0(lambda b, w: struct_ptr(w["root"][1] - 1, 3, len(b.seg[0]) - w["root"][1] - 2)))
    add("root_fills_segment", root0(lambda b, w: struct_ptr(w["root"][1] - 1, 3, len(b.seg[0]) - w["root"][1] - 3)))
    add("root_no_data_no_pointers", root0(lambda b, w: struct_ptr(0, 0, 0)))
    add("root_two_data_words", root0(lambda b, w: struct_ptr(w["root"][1] - 1, 2, 0)))
    # ---- far pointers -----------------------------------------------------------------------
    add("far_root_segment_id", root0(lambda b, w: far_ptr(False, 0, 1)))
    add("far_root_segment_id_big", standard(3, root="far", edit=lambda b, w: b.seg[0].__setitem__(
        0, far_ptr(False, 0, 0xFFFFFFFF))))
    add("far_root_pad_past_segment", standard(2, root="far", edit=lambda b, w: b.seg[0].__setitem__(
        0, far_ptr(False, len(b.seg[1]), 1))))
    add("far_root_pad_last_word", standard(2, root="far", edit=lambda b, w: (
        b.alloc(1, [0]), b.seg[0].__setitem__(0, far_ptr(False, len(b.seg[1]) - 1, 1)))))  # a null landing
    add("dfar_root_pad_one_word_left", standard(2, root="far", edit=lambda b, w: b.seg[0].__setitem__(
        0, far_ptr(True, len(b.seg[1]) - 1, 1))))
    add("dfar_root_pad_fits_exactly", standard(2, root="far", edit=lambda b, w: (
        b.alloc(1, [far_ptr(False, w["root"][1], 1), struct_ptr(0, 3, 8)]),
        b.seg[0].__setitem__(0, far_ptr(True, len(b.seg[1]) - 2, 1)))))

    def dfar_first(first):
        def edit(b, w):
            pad = b.alloc(1, [first(b, w), struct_ptr(0, 3, 8)])
            b.seg[0][0] = far_ptr(True, pad, 1)
        return standard(2, root="far", edit=edit)

    add("dfar_first_word_is_struct", dfar_first(lambda b, w: struct_ptr(0, 3, 8)))
    add("dfar_first_word_is_null", dfar_first(lambda b, w: 0))
    add("dfar_first_word_is_double_far", dfar_first(lambda b, w: far_ptr(True, w["root"][1], 1)))
    add("dfar_content_segment_id", dfar_first(lambda b, w: far_ptr(False, w["root"][1], 2)))
    add("dfar_content_past_segment", dfar_first(lambda b, w: far_ptr(False, len(b.seg[1]) + 5, 1)))
    add("dfar_tag_is_null", standard(2, root="far", edit=lambda b, w: b.seg[0].__setitem__(
        0, far_ptr(True, b.alloc(1, [far_ptr(False, w["root"][1], 1), 0]), 1))))
    add("dfar_tag_is_list", standard(2, root="far", edit=lambda b, w: b.seg[0].__setitem__(
        0, far_ptr(True, b.alloc(1, [far_ptr(False, w["root"][1], 1), list_ptr(0, 2, 3)]), 1))))
    # ---- path steps -------------------------------------------------------------------------
    add("child_null", standard(edit=_set("root_ptrs", 2, lambda b, s, i: 0)))
    add("child_is_list", standard(edit=_set("root_ptrs", 2, lambda b, s, i: list_ptr(0, 2, 0))))
    add("child_negative", standard(edit=_set("root_ptrs", 2, lambda b, s, i: struct_ptr(-i - 2, 1, 2))))
    add("child_truncated", standard(edit=_set("root_ptrs", 2, lambda b, s, i: struct_ptr(len(b.seg[s]) - i - 2, 1, 1))))
    add("child_far_segment_id", standard(edit=_set("root_ptrs", 2, lambda b, s, i: far_ptr(False, 0, 7))))
    add("great_grandchild_null", standard(edit=_set("great", -1, lambda b, s, i: 0)))
    add("great_grandchild_no_pointers", standard(edit=_set("great", -1, lambda b, s, i: struct_ptr(0, 1, 0))))
    # ---- slices -----------------------------------------------------------------------------
    for index, name in ((0, "text"), (1, "data"), (3, "l16"), (5, "bits")):
        def variant(tag, make, index=index, name=name):
            def edit(b, w):
                s, rp = w["root_ptrs"]
                b.seg[s][rp + index] = make(b, w, w[name][1] - (rp + index) - 1, rp + index)
            add(f"{name}_{tag}", standard(edit=edit))

        variant("null", lambda b, w, o, i: 0)
        variant("is_struct", lambda b, w, o, i: struct_ptr(o, 0, 0))
        variant("is_capability", lambda b, w, o, i: 3 | (5 << 32))
        variant("bytes_as_words", lambda b, w, o, i: list_ptr(o, 5, 1))
        variant("size_0", lambda b, w, o, i: list_ptr(o, 0, 1000))
        variant("size_6", lambda b, w, o, i: list_ptr(o, 6, 1))
        variant("size_7_fits", lambda b, w, o, i: list_ptr(o, 7, 0))
        variant("size_7_tag_past_end", lambda b, w, o, i: list_ptr(len(b.seg[0]) - i - 1, 7, 0))
        variant("negative", lambda b, w, o, i: list_ptr(-i - 2, 2, 0))
        variant("at_word_0", lambda b, w, o, i: list_ptr(-i - 1, {"text": 2, "data": 2, "l16": 3, "bits": 1}[name], 8))
        variant("ends_at_segment_end", lambda b, w, o, i: list_ptr(len(b.seg[0]) - i - 1, 2, 0))
        variant("starts_past_segment_end", lambda b, w, o, i: list_ptr(len(b.seg[0]) - i, 2, 0))
        variant("runs_one_byte_past", lambda b, w, o, i: list_ptr(o, 2, 8 * (len(b.seg[0]) - w[name][1]) + 1))
        variant("runs_to_the_end", lambda b, w, o, i: list_ptr(o, 2, 8 * (len(b.seg[0]) - w[name][1])))
        variant("wrong_size_and_past_end", lambda b, w, o, i: list_ptr(o, 5, len(b.seg[0])))
        variant("far_segment_id", lambda b, w, o, i: far_ptr(False, 0, 1))
        variant("far_pad_past_segment", lambda b, w, o, i: far_ptr(False, len(b.seg[0]), 0))
        variant("far_to_null", lambda b, w, o, i: far_ptr(False, w["root_ptrs"][1] + 7, 0))
        variant("dfar_first_not_far", lambda b, w, o, i: far_ptr(True, w["root"][1], 0))
    for count in range(0, 10):
        raw = bytes([0x41 + k for k in range(count)])
        add(f"text_{count}_bytes_no_nul", standard(text=raw))
        add(f"text_{count + 1}_bytes_nul", standard(text=raw + b"\0"))
    add("text_two_nuls", standard(text=b"ab\0\0"))
    add("data_empty", standard(data=b""))
    add("data_long", standard(data=bytes(range(256)) * 3))
    return out


def layout(messages, order, filler=0xA7):
    """The messages back to back in `order` (indices into messages), each at the next multiple
    of 8, between fillers of distinct nonzero bytes: (buffer, offsets, lengths)."""
    buf = bytearray()
    offs, lens = [], []
    for k, i in enumerate(order):
        buf += bytes([(filler + 3 * k + j) % 251 + 1 for j in range(8 + 8 * (k % 3))])
        buf += b"\x5C" * (-len(buf) % 8)
        offs.append(len(buf))
        lens.append(len(messages[i]))
        buf += messages[i]
    buf += bytes([0xE3] * 40)
    return bytes(buf), offs, lens


# ---------------------------------------------------------------------------
# the four interop fixtures and what the reference reads from them
# ---------------------------------------------------------------------------
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixtures")


def fixture(name):
    with open(os.path.join(FIXTURES, name), "rb") as f:
        return f.read()


def f32_bits(x):
    return _struct.unpack("<I", _struct.pack("<f", x))[0]


def f64_bits(x):
    return _struct.unpack("<Q", _struct.pack("<d", x))[0]


# (field, status, value or content bytes, len, count): what the reference reads from the fixtures
# Widget's pointers are the reference's own interop test's (tests/serialization/interop_test.zig:
# readData(3), readU16List(4) ... readF64List(9)); pointers 1, 2 and 10 are struct and pointer
# lists, which the call does not read.
WIDGET = [
    (F(U32, 0), OK, 123, 4, 1),
    (F(TEXT, 0), OK, b"widget", 6, 6),
    (F(DATA, 3), OK, bytes([1, 2, 3, 4, 5]), 5, 5),
    (F(LIST_16, 4), OK, _struct.pack("<3H", 10, 20, 30), 6, 3),
    (F(LIST_32, 5), OK, _struct.pack("<2I", 1000, 2000), 8, 2),
    (F(LIST_64, 6), OK, _struct.pack("<2Q", 123456789, 987654321), 16, 2),
    (F(LIST_BIT, 7), OK, b"\x15", 1, 5),
    (F(LIST_32, 8), OK, _struct.pack("<3f", 1.25, 2.5, -3.75), 12, 3),
    (F(LIST_64, 9), OK, _struct.pack("<2d", 1.125, -2.25), 16, 2),
    (F(DATA, 4), INVALID_POINTER, 0, 0, 0),   # a List(UInt16): element size 3
    (F(LIST_64, 10), INVALID_POINTER, 0, 0, 0),  # a pointer list: element size 6
    (F(DATA, 1), INVALID_POINTER, 0, 0, 0),   # a struct list: element size 7
    (F(TEXT, 11), OK, b"", 0, 0),  # past the 11 pointers
    (F(DATA, 11), OUT_OF_BOUNDS, 0, 0, 0),
]
ALL_TYPES = [
    (F(BOOL, 0, 0), OK, 1, 1, 1),
    (F(U8, 1), OK, 133, 1, 1),
    (F(U16, 2), OK, 53191, 2, 1),
    (F(U32, 4), OK, 4282621618, 4, 1),
    (F(U64, 8), OK, 18446620616920539271, 8, 1),
    (F(U8, 16), OK, 234, 1, 1),
    (F(U16, 18), OK, 45678, 2, 1),
    (F(U32, 20), OK, 3456789012, 4, 1),
    (F(U64, 24), OK, 12345678901234567890, 8, 1),
    (F(U32, 32), OK, f32_bits(1234.5), 4, 1),
    (F(U64, 40), OK, f64_bits(-123e45), 8, 1),
    (F(TEXT, 0), OK, b"foo", 3, 3),
    (F(DATA, 1), OK, b"bar", 3, 3),
    (F(LIST_16, 6), OK, None, 4, 2),
    (F(LIST_64, 8), OK, None, 16, 2),
    (F(U64, 48), OK, 0, 0, 0),
    (F(U64, 44), OK, 0, 0, 0),  # straddles the end of the data section
    (F(U8, 47), OK, 201, 1, 1),
    (F(U8, 1, path=(2,)), OK, 244, 1, 1),
    (F(U16, 2, path=(2,)), OK, 3456, 2, 1),
    (F(U64, 8, path=(2,)), OK, 56789012345678, 8, 1),
    (F(TEXT, 0, path=(2,)), OK, b"baz", 3, 3),
    (F(DATA, 1, path=(2,)), OK, b"qux", 3, 3),
    (F(TEXT, 0, path=(2, 2)), OK, b"nested", 6, 6),
    (F(TEXT, 0, path=(2, 2, 2)), OK, b"really nested", 13, 13),
    (F(TEXT, 0, path=(2, 2, 2, 2)), INVALID_POINTER, 0, 0, 0),
    (F(DATA, 19), INVALID_POINTER, 0, 0, 0),
    (F(LIST_16, 5), INVALID_POINTER, 0, 0, 0),
]
TABLES = {"fixture_single.bin": WIDGET, "fixture_far.bin": WIDGET, "binary": ALL_TYPES, "segmented": ALL_TYPES}


def check_table(data, table, got, base=0):
    """got[k] = (status, value, len, count) for table[k]; a slice's value - base is its offset in data"""
    for (field, status, want, length, count), (st, v, l, c) in zip(table, got):
        assert (st, l, c) == (status, length, count), field
        if isinstance(want, bytes):
            assert data[v - base:v - base + l] == want, field
        elif want is not None:
            assert v == want, field
