"""Model and corpus for capnp_packed_list_heads_batch and capnp_packed_read_elements_batch
(DESIGN.md §2.14), in the manner of struct_streams.py, whose model, builder and `_chk` record
this module reuses.

The model restates, function for function: resolveInlineCompositeList (message.zig:563-696),
readStructList (:1165-1185), readTextList / readPointerList (:1200-1222), StructListReader.get
(list_readers.zig:87-100), TextListReader.get (:113-133) and PointerListReader.getText / getData
/ readPrimitiveList / getStruct (:243-324). The device reads a pointer-list element as a struct
of no data words and one pointer; `element_fields` is that reading, and test_list_streams.py
asserts that it equals the restated list readers on every element of the corpus."""
import struct as _struct

import struct_streams as ss
from struct_streams import (DATA, F, INVALID_FAR_POINTER, INVALID_POINTER, INVALID_SEGMENT_ID, LIST_16, LIST_32,
                            LIST_64, LIST_BIT, OK, OUT_OF_BOUNDS, TEXT, U32, U64, BOOL, RefError, _chk, far_ptr,
                            list_ptr, struct_ptr)

INVALID_INLINE_COMPOSITE_POINTER = 21
LIST_STRUCT, LIST_POINTER = 0, 1

# every check of this module's model (struct_streams.CHECKS holds the ones it borrows)
CHECKS = (
    "slist.index", "slist.null", "icl.is_list", "icl.near_size", "icl.tag_negative", "icl.tag_bounds",
    "icl.tag_type", "icl.count_negative", "icl.count_words", "icl.bounds", "icl.not_far", "icl.far_segment_id",
    "icl.far_pad_bounds", "icl.far_is_double", "icl.landing_not_list", "icl.dfar_first_not_far",
    "icl.dfar_first_is_double", "icl.dfar_segment_id", "icl.second_is_struct", "icl.a_count_negative",
    "icl.a_bounds", "icl.second_is_list", "icl.b_size", "icl.b_tag_bounds", "icl.b_tag_type",
    "icl.b_count_negative", "icl.b_count_words", "icl.b_bounds",
    "plist.index", "plist.null", "plist.element_size",
    "tget.null", "tget.element_size", "tget.empty", "tget.trailing_nul",
    "pdata.null", "pdata.element_size", "pprim.null", "pprim.element_size", "pstruct.null",
)
# StructListReader.get's own bounds check is restated too, but it has one way only: after a
# resolved head it cannot fail (the head checked the whole list against the segment)
ONE_WAY = ("sget.bounds",)


def _icp():
    return RefError(INVALID_INLINE_COMPOSITE_POINTER, "InvalidInlineCompositePointer")


def _oob():
    return RefError(OUT_OF_BOUNDS, "OutOfBounds")


def _read_word(m, seg, pos, name):  # readWord (:420-425); the segment id was checked by every caller
    if _chk(name, pos + 8 > len(m.segments[seg])):
        raise _oob()
    return m.word(seg, pos)


def _tag(word):
    return ss.offset_words(word), (word >> 32) & 0xFFFF, (word >> 48) & 0xFFFF


def resolve_inline_composite_list(m, seg, pos, word):  # :563-696 -> (segment, elements offset, count, dw, pw)
    if word == 0:  # (readStructList checked this already: not reachable)
        raise RefError(INVALID_POINTER, "InvalidPointer")
    if _chk("icl.is_list", word & 3 == 1):
        if _chk("icl.near_size", (word >> 32) & 7 != 7):
            raise _icp()
        word_count = word >> 35
        tag_pos = pos + 8 + ss.offset_words(word) * 8
        if _chk("icl.tag_negative", tag_pos < 0):
            raise _oob()
        tag = _read_word(m, seg, tag_pos, "icl.tag_bounds")
        if _chk("icl.tag_type", tag & 3 != 0):
            raise _icp()
        count, dw, pw = _tag(tag)
        if _chk("icl.count_negative", count < 0):
            raise _icp()
        if _chk("icl.count_words", count * (dw + pw) > word_count):
            raise _icp()
        if _chk("icl.bounds", tag_pos + 8 + word_count * 8 > len(m.segments[seg])):
            raise _oob()
        return seg, tag_pos + 8, count, dw, pw
    if _chk("icl.not_far", word & 3 != 2):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    double, pad, far_seg = (word >> 2) & 1, ((word >> 3) & 0x1FFFFFFF) * 8, word >> 32
    if _chk("icl.far_segment_id", far_seg >= len(m.segments)):  # resolveFarLandingPad (:430-437)
        raise RefError(INVALID_SEGMENT_ID, "InvalidSegmentId")
    if _chk("icl.far_pad_bounds", pad + (16 if double else 8) > len(m.segments[far_seg])):
        raise _oob()
    if not _chk("icl.far_is_double", double):
        landing = m.word(far_seg, pad)
        if _chk("icl.landing_not_list", landing & 3 != 1):
            raise RefError(INVALID_POINTER, "InvalidPointer")
        return resolve_inline_composite_list(m, far_seg, pad, landing)
    first, second = m.word(far_seg, pad), m.word(far_seg, pad + 8)
    if _chk("icl.dfar_first_not_far", first & 3 != 2):
        raise RefError(INVALID_FAR_POINTER, "InvalidFarPointer")
    if _chk("icl.dfar_first_is_double", (first >> 2) & 1):
        raise RefError(INVALID_FAR_POINTER, "InvalidFarPointer")
    cseg, target = first >> 32, ((first >> 3) & 0x1FFFFFFF) * 8
    if _chk("icl.dfar_segment_id", cseg >= len(m.segments)):
        raise RefError(INVALID_SEGMENT_ID, "InvalidSegmentId")
    if _chk("icl.second_is_struct", second & 3 == 0):  # layout A
        count, dw, pw = _tag(second)
        if _chk("icl.a_count_negative", count < 0):
            raise _icp()
        # (:645's overflow guard: count < 2^29 and words < 2^17, so it cannot trip)
        if _chk("icl.a_bounds", target + count * (dw + pw) * 8 > len(m.segments[cseg])):
            raise _oob()
        return cseg, target, count, dw, pw
    if _chk("icl.second_is_list", second & 3 == 1):  # layout B
        if _chk("icl.b_size", (second >> 32) & 7 != 7):
            raise _icp()
        word_count = second >> 35
        tag = _read_word(m, cseg, target, "icl.b_tag_bounds")
        if _chk("icl.b_tag_type", tag & 3 != 0):
            raise _icp()
        count, dw, pw = _tag(tag)
        if _chk("icl.b_count_negative", count < 0):
            raise _icp()
        if _chk("icl.b_count_words", count * (dw + pw) > word_count):
            raise _icp()
        if _chk("icl.b_bounds", target + 8 + word_count * 8 > len(m.segments[cseg])):
            raise _oob()
        return cseg, target + 8, count, dw, pw
    raise _icp()


def read_struct_list(m, s, index):  # :1165-1185
    p = ss.pointer_at(m, s, index)
    if _chk("slist.index", p is None):
        raise _oob()
    if _chk("slist.null", p[1] == 0):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    return resolve_inline_composite_list(m, s.seg, p[0], p[1])


def read_pointer_list(m, s, index):  # readTextList / readPointerList (:1200-1222) -> (segment, offset, count, 0, 1)
    p = ss.pointer_at(m, s, index)
    if _chk("plist.index", p is None):  # resolveListPointerAt (:1187-1198)
        raise _oob()
    if _chk("plist.null", p[1] == 0):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    seg, content, size, count = ss.resolve_list_pointer(m, s.seg, p[0], p[1])
    if _chk("plist.element_size", size != 6):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    return seg, content, count, 0, 1


# ---- the list readers (list_readers.zig) --------------------------------------------------------
def struct_list_get(m, lst, k):  # StructListReader.get (:87-100); k < count is the caller's
    seg, eo, count, dw, pw = lst
    stride = 8 * (dw + pw)
    if _chk("sget.bounds", eo + k * stride + stride > len(m.segments[seg])):
        raise _oob()
    return ss.Struct(seg, eo + k * stride, dw, pw)


def _slot(m, lst, k):  # readPointer (:243-250)
    seg, eo = lst[0], lst[1]
    return seg, eo + 8 * k, m.word(seg, eo + 8 * k)


def _text_of(m, seg, content, count, base):
    nbytes = count
    if not _chk("tget.empty", count == 0) and _chk("tget.trailing_nul", m.segments[seg][content + count - 1] == 0):
        nbytes -= 1
    return base + m.starts[seg] + content, nbytes, nbytes


def text_list_get(m, lst, k, base=0):  # TextListReader.get (:113-133) = PointerListReader.getText (:258-272)
    seg, pos, word = _slot(m, lst, k)
    if _chk("tget.null", word == 0):
        return 0, 0, 0
    seg, content, size, count = ss.resolve_list_pointer(m, seg, pos, word)
    if _chk("tget.element_size", size != 2):
        raise RefError(INVALID_POINTER, "InvalidTextPointer")
    return _text_of(m, seg, content, count, base)


def pointer_list_get_data(m, lst, k, base=0):  # getData (:298-304)
    seg, pos, word = _slot(m, lst, k)
    if _chk("pdata.null", word == 0):  # readList (:252-256)
        raise RefError(INVALID_POINTER, "InvalidPointer")
    seg, content, size, count = ss.resolve_list_pointer(m, seg, pos, word)
    if _chk("pdata.element_size", size != 2):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    return base + m.starts[seg] + content, count, count


def pointer_list_read_primitive_list(m, lst, k, kind, base=0):  # readPrimitiveList (:308-324)
    seg, pos, word = _slot(m, lst, k)
    if _chk("pprim.null", word == 0):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    seg, content, size, count = ss.resolve_list_pointer(m, seg, pos, word)
    if _chk("pprim.element_size", size != ss.ELEMENT_SIZE[kind]):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    return base + m.starts[seg] + content, (count + 7) // 8 if size == 1 else count << (size - 2), count


def pointer_list_get_struct(m, lst, k):  # getStruct (:284-288)
    seg, pos, word = _slot(m, lst, k)
    if _chk("pstruct.null", word == 0):
        raise RefError(INVALID_POINTER, "InvalidPointer")
    return ss.resolve_struct_pointer(m, seg, pos, word)


def reader_field(m, lst, k, f, base=0):
    """Field f of element k of a POINTER list through the restated list readers:
    (status, value, len, count)."""
    try:
        if not f.path:
            assert f.offset == 0 and f.kind not in ss.WIDTH
            if f.kind == TEXT:
                return (OK,) + text_list_get(m, lst, k, base)
            if f.kind == DATA:
                return (OK,) + pointer_list_get_data(m, lst, k, base)
            return (OK,) + pointer_list_read_primitive_list(m, lst, k, f.kind, base)
        assert f.path[0] == 0
        s = pointer_list_get_struct(m, lst, k)
        for index in f.path[1:]:
            s = ss.read_struct(m, s, index)
        return (OK,) + (ss.read_data_kind(m, s, f) if f.kind in ss.WIDTH else ss.read_slice_kind(m, s, f, base))
    except RefError as e:
        return (e.status, 0, 0, 0)


def element_fields(m, kind, lst, k, fields, base=0):
    """What read_elements_batch answers for element k: the element as a struct reader (a
    pointer-list slot: no data words, one pointer), then read_fields_batch's field reads."""
    seg, eo, count, dw, pw = lst
    elem = struct_list_get(m, lst, k) if kind == LIST_STRUCT else ss.Struct(seg, eo + 8 * k, 0, 1)
    out = []
    for f in fields:
        try:
            s = elem
            for index in f.path:
                s = ss.read_struct(m, s, index)
            out.append((OK,) + (ss.read_data_kind(m, s, f) if f.kind in ss.WIDTH
                                else ss.read_slice_kind(m, s, f, base)))
        except RefError as e:
            out.append((e.status, 0, 0, 0))
    return out


class Head:
    """capnp_packed_list_head as the model gives it (all zero but the status when it failed)."""

    def __init__(self, status, elems_off=0, count=0, segment=0, seg_begin=0, seg_bytes=0, data_words=0,
                 pointer_words=0):
        self.status, self.elems_off, self.count, self.segment = status, elems_off, count, segment
        self.seg_begin, self.seg_bytes, self.data_words, self.pointer_words = seg_begin, seg_bytes, data_words, pointer_words

    def tuple(self):
        return (self.status, self.elems_off, self.count, self.segment, self.seg_begin, self.seg_bytes,
                self.data_words, self.pointer_words)


def read_list(data, kind, pointer_index, fields, path=(), base=0, limit=None):
    """(Head, [element k's [(status, value, len, count) per field]]) for one message at offset
    `base` of the input buffer; at most `limit` elements are read."""
    try:
        m = ss.Msg(data)
        s = ss.get_root_struct(m)
        for index in path:
            s = ss.read_struct(m, s, index)
        lst = (read_struct_list if kind == LIST_STRUCT else read_pointer_list)(m, s, pointer_index)
    except RefError as e:
        return Head(e.status), []
    seg, eo, count, dw, pw = lst
    head = Head(OK, base + m.starts[seg] + eo, count, seg, m.starts[seg], len(m.segments[seg]), dw, pw)
    rows = range(count if limit is None else min(count, limit))
    return head, [element_fields(m, kind, lst, k, fields, base) for k in rows]


# ---------------------------------------------------------------------------
# the builder
# ---------------------------------------------------------------------------
# The corpus's schema. Root: 1 data word, 4 pointers:
#   p0 List(Elem), p1 List(AnyPointer), p2 child (1 data word, 2 pointers: p0 List(Elem), p1 List(Text)), p3 null
# Elem (dw data words, pw pointers): U32@0 = 1000 * (k + 1), U32@4 = k, U64@8 = ~k; p0 Text, p1 Data,
# p2 a struct (1, 1): U32@0 = 77 + k, p0 Text
STRUCT_FIELDS = [
    F(U32, 0), F(U32, 4), F(U64, 8), F(U64, 16), F(BOOL, 1, 3), F(TEXT, 0), F(DATA, 1), F(U32, 0, path=(2,)),
    F(TEXT, 0, path=(2,)), F(TEXT, 5), F(DATA, 5), F(LIST_16, 0), F(U32, 6),
]
POINTER_FIELDS = [
    F(TEXT, 0), F(DATA, 0), F(LIST_16, 0), F(LIST_32, 0), F(LIST_64, 0), F(LIST_BIT, 0), F(U32, 0, path=(0,)),
    F(TEXT, 0, path=(0,)), F(DATA, 0, path=(0, 0)),
]


def _point_list(b, at, to, make, via, pad_seg):
    """the list pointer at `at`: near / far / dfar_b through Builder.point (dfar: a list pointer in
    the pad, layout B); dfar_a: the pad holds make_tag's word and the far word names element 0"""
    b.point(at, to, make, via={"dfar_b": "dfar"}.get(via, via), pad_seg=pad_seg)


def add_struct_list(b, at, seg, count, dw, pw, via="near", pad_seg=None, evia="near", eseg=None, where=None,
                    name="slist"):
    """a struct list of `count` elements in segment `seg`, its pointer written at `at`"""
    words = count * (dw + pw)
    tag = b.alloc(seg, [struct_ptr(count, dw, pw)])
    first = b.alloc(seg, [0] * words)
    eseg = seg if eseg is None else eseg
    for k in range(count):
        e = first + k * (dw + pw)
        data = [(1000 * (k + 1)) | (k << 32), ~k & 0xFFFFFFFFFFFFFFFF, 0x5151515151515151]
        for j in range(min(dw, 3)):
            b.seg[seg][e + j] = data[j]
        for j in range(3, dw):
            b.seg[seg][e + j] = 0x0707070707070707 + j
        if pw >= 1:
            raw = b"elem %d" % k + (b"\0" if k % 2 == 0 else b"")
            b.point((seg, e + dw), (eseg, b.alloc_bytes(eseg, raw)), lambda o, n=len(raw): list_ptr(o, 2, n),
                    via=evia, pad_seg=pad_seg)
        if pw >= 2:
            raw = bytes([k, k + 1, k + 2])
            b.point((seg, e + dw + 1), (eseg, b.alloc_bytes(eseg, raw)), lambda o: list_ptr(o, 2, 3), via=evia,
                    pad_seg=pad_seg)
        if pw >= 3:
            child = b.alloc(eseg, [77 + k, 0])
            b.point((seg, e + dw + 2), (eseg, child), lambda o: struct_ptr(o, 1, 1), via=evia, pad_seg=pad_seg)
            t = b.alloc_bytes(eseg, b"in %d" % k)
            b.point((eseg, child + 1), (eseg, t), lambda o, k=k: list_ptr(o, 2, len(b"in %d" % k)), via="near")
    if via == "dfar_a":
        hs = seg if pad_seg is None else pad_seg
        pad = b.alloc(hs, [far_ptr(False, first, seg), struct_ptr(count, dw, pw)])
        b.seg[at[0]][at[1]] = far_ptr(True, pad, hs)
    else:
        _point_list(b, at, (seg, tag), lambda o: list_ptr(o, 7, words), via, pad_seg)
    if where is not None:
        where[name + "_tag"], where[name + "_first"], where[name + "_words"] = (seg, tag), (seg, first), words


def add_pointer_list(b, at, seg, via="near", pad_seg=None, evia="near", eseg=None, texts_only=False, count=None,
                     where=None, name="plist"):
    """a pointer list in segment `seg`: a List(Text) (texts_only) or one slot of every sort"""
    eseg = seg if eseg is None else eseg
    if texts_only:
        slots = [("text", b"alpha\0"), ("text", b"beta\0"), ("null", None), ("text", b"no nul"), ("text", b""),
                 ("text", b"\0")]
    else:
        slots = [("text", b"alpha\0"), ("null", None), ("l16", _struct.pack("<2H", 7, 8)), ("struct", None),
                 ("data", bytes([9, 8, 7, 6, 5, 4, 3, 2, 1])), ("l64", _struct.pack("<2Q", 1 << 40, 3)),
                 ("l32", _struct.pack("<3I", 1, 2, 3)), ("bits", b"\x2D\x01"), ("text", b"tail"), ("cap", None)]
    if count is not None:
        slots = (slots * (count // len(slots) + 1))[:count]
    first = b.alloc(seg, [0] * len(slots))
    for k, (sort, raw) in enumerate(slots):
        slot = (seg, first + k)
        if sort == "null":
            continue
        if sort == "cap":
            b.seg[seg][first + k] = 3 | (k << 32)
        elif sort == "struct":
            child = b.alloc(eseg, [4242, 0])
            b.point(slot, (eseg, child), lambda o: struct_ptr(o, 1, 1), via=evia, pad_seg=pad_seg)
            inner = b.alloc(eseg, [0])  # a struct of no data and one pointer, to a Data
            b.point((eseg, child + 1), (eseg, inner), lambda o: struct_ptr(o, 0, 1), via="near")
            t = b.alloc_bytes(eseg, b"deep data")
            b.point((eseg, inner), (eseg, t), lambda o: list_ptr(o, 2, 9), via="near")
        else:
            size, n = {"text": (2, len(raw)), "data": (2, len(raw)), "l16": (3, len(raw) // 2),
                       "l32": (4, len(raw) // 4), "l64": (5, len(raw) // 8), "bits": (1, 9)}[sort]
            b.point(slot, (eseg, b.alloc_bytes(eseg, raw)), lambda o, size=size, n=n: list_ptr(o, size, n),
                    via=evia, pad_seg=pad_seg)
    _point_list(b, at, (seg, first), lambda o: list_ptr(o, 6, len(slots)), via.split("_")[0], pad_seg)
    if where is not None:
        where[name + "_first"], where[name + "_count"] = (seg, first), len(slots)


def message(nseg=1, via="near", count=3, dw=2, pw=3, evia="near", list_seg=None, eseg=None, pad_seg=None,
            pcount=None, edit=None):
    """The schema above. The root and the child struct lie in segment 0; the lists in `list_seg`
    (default: the last segment; `via` near needs segment 0), what elements point to in `eseg`."""
    b = ss.Builder(nseg)
    list_seg = nseg - 1 if list_seg is None else list_seg
    b.alloc(0, [0])
    for s in range(nseg):
        b.alloc(s, [0xF2F2F2F2F2F2F2F2 + s] * 2)
    root = b.alloc(0, [0xABCD, 0, 0, 0, 0])
    b.seg[0][0] = struct_ptr(root - 1, 1, 4)
    child = b.alloc(0, [0x1111, 0, 0])
    b.seg[0][root + 3] = struct_ptr(child - (root + 3) - 1, 1, 2)
    where = {"root": (0, root), "root_ptrs": (0, root + 1), "child_ptrs": (0, child + 1)}
    args = dict(via=via, pad_seg=pad_seg, evia=evia, eseg=eseg, where=where)
    add_struct_list(b, (0, root + 1), list_seg, count, dw, pw, **args)
    add_pointer_list(b, (0, root + 2), list_seg, count=pcount, **args)
    add_struct_list(b, (0, child + 1), list_seg, 2, 1, 1, name="child_slist", **args)
    add_pointer_list(b, (0, child + 2), list_seg, texts_only=True, name="child_plist", **args)
    if edit:
        edit(b, where)
    b.alloc(list_seg, [0xE0E0E0E0E0E0E0E0] * 2)  # the lists do not end their segment unless an edit says so
    return b.bytes()


# the (kind, pointer index, path) runs of the tests: each list read as what it is, as the other
# kind, and the null and the missing pointer
RUNS = [
    (LIST_STRUCT, 0, ()), (LIST_POINTER, 1, ()), (LIST_STRUCT, 0, (2,)), (LIST_POINTER, 1, (2,)),
    (LIST_STRUCT, 1, ()), (LIST_POINTER, 0, ()), (LIST_STRUCT, 3, ()), (LIST_POINTER, 3, ()), (LIST_STRUCT, 4, ()),
    (LIST_POINTER, 4, ()), (LIST_STRUCT, 0, (3,)),
]


def fields_of(kind):
    return STRUCT_FIELDS if kind == LIST_STRUCT else POINTER_FIELDS


def corpus():
    """[(name, framed bytes)]: every reaching arm, every error arm of the two calls' contract,
    and the element shapes."""
    out = []

    def add(name, data):
        out.append((name, bytes(data)))

    # ---- the message-level errors and layouts of read_fields_batch, borrowed ------------------
    borrowed = dict(ss.corpus())
    for name in ("empty", "three_bytes", "four_bytes_one_segment", "four_bytes_segcount", "seven_bytes_seglimit",
                 "header_truncated", "segment_truncated", "segment0_empty", "root_null", "root_chain_8_hops",
                 "dfar_first_word_is_struct", "far_root_segment_id", "root_one_word_too_long",
                 "far_root_pad_past_segment", "one_segment", "5_segments_far_pointers", "root_no_data_no_pointers"):
        add("fields_" + name, borrowed[name])
    # ---- the reaching arms ------------------------------------------------------------------------
    add("near", message())
    for nseg in (2, 3, 5):
        for via in ("far", "dfar_a", "dfar_b"):
            add(f"{via}_{nseg}_segments", message(nseg, via=via, pad_seg=nseg // 2))
    add("far_list_in_segment_0", message(2, via="far", list_seg=0))
    add("dfar_b_200_segments", message(200, via="dfar_b", list_seg=150, pad_seg=199))
    for evia in ("far", "dfar"):
        add(f"near_list_elements_{evia}", message(3, via="far", evia=evia, list_seg=1, eseg=2, pad_seg=2))
        add(f"dfar_a_list_elements_{evia}", message(6, via="dfar_a", evia=evia, list_seg=4, eseg=5, pad_seg=3))
    add("elements_far_same_segment", message(2, via="far", evia="far"))
    # ---- the element shapes -----------------------------------------------------------------------
    for count in (0, 1, 2, 17):
        add(f"count_{count}", message(count=count, pcount=count))
    add("zero_word_elements", message(count=1000, dw=0, pw=0))
    add("zero_word_elements_dfar_a", message(2, via="dfar_a", count=1000, dw=0, pw=0))
    add("no_pointers", message(count=4, dw=3, pw=0))
    add("no_data", message(count=4, dw=0, pw=2))
    add("one_data_word", message(count=5, dw=1, pw=1))
    add("wide", message(count=3, dw=5, pw=4))

    # ---- the error arms: edits of the list pointer, the tag and the pads -----------------------------
    def set_ptr(make, index=0, **kw):
        def edit(b, w):
            s, rp = w["root_ptrs"]
            b.seg[s][rp + index] = make(b, w, rp + index)
        return message(edit=edit, **kw)

    def near_word(b, w, i, size=7, words=None, off=None):
        tag = w["slist_tag"][1]
        return list_ptr(tag - i - 1 if off is None else off, size, w["slist_words"] if words is None else words)

    add("near_size_6", set_ptr(lambda b, w, i: near_word(b, w, i, size=6)))
    add("near_size_5_past_end", set_ptr(lambda b, w, i: near_word(b, w, i, size=5, words=1 << 20)))
    add("near_tag_negative", set_ptr(lambda b, w, i: near_word(b, w, i, off=-i - 2)))
    add("near_tag_at_word_0", set_ptr(lambda b, w, i: near_word(b, w, i, off=-i - 1, words=0)))
    add("near_tag_past_segment", set_ptr(lambda b, w, i: near_word(b, w, i, off=(1 << 20), words=0)))
    add("near_pointer_is_capability", set_ptr(lambda b, w, i: 3 | (7 << 32)))
    add("near_pointer_is_struct", set_ptr(lambda b, w, i: struct_ptr(0, 1, 1)))
    add("near_words_one_short", set_ptr(lambda b, w, i: near_word(b, w, i, words=w["slist_words"] - 1)))
    add("near_words_with_slack", set_ptr(lambda b, w, i: near_word(b, w, i, words=w["slist_words"] + 1)))
    add("near_words_past_segment", set_ptr(lambda b, w, i: near_word(b, w, i, words=1 << 15)))

    def set_tag(make):
        def edit(b, w):
            s, t = w["slist_tag"]
            b.seg[s][t] = make(b.seg[s][t])
        return edit

    for name, kw in (("near", {}), ("far", dict(nseg=2, via="far")), ("dfar_b", dict(nseg=3, via="dfar_b", pad_seg=1))):
        add(f"{name}_tag_is_list", message(edit=set_tag(lambda t: t | 1), **kw))
        add(f"{name}_tag_is_capability", message(edit=set_tag(lambda t: t | 3), **kw))
        add(f"{name}_tag_count_negative", message(edit=set_tag(lambda t: (t & ~0xFFFFFFFF) | (0x20000000 << 2)), **kw))
        add(f"{name}_tag_count_one_more", message(edit=set_tag(lambda t: t + 4), **kw))
        add(f"{name}_tag_wider_elements", message(edit=set_tag(lambda t: t + (1 << 48)), **kw))

    # ---- single far -------------------------------------------------------------------------------
    add("far_segment_id", set_ptr(lambda b, w, i: far_ptr(False, 0, 1)))
    add("far_segment_id_big", set_ptr(lambda b, w, i: far_ptr(False, 0, 0xFFFFFFFF), nseg=3, via="far"))
    add("far_pad_past_segment", set_ptr(lambda b, w, i: far_ptr(False, 1 << 20, 1), nseg=2, via="far"))
    add("far_pad_is_last_word", set_ptr(lambda b, w, i: far_ptr(False, b.alloc(1, [list_ptr(-4, 7, 0)]), 1), nseg=2,
                                        via="far"))
    add("far_lands_on_struct", set_ptr(lambda b, w, i: far_ptr(False, b.alloc(1, [struct_ptr(0, 1, 1)]), 1), nseg=2,
                                       via="far"))
    add("far_lands_on_null", set_ptr(lambda b, w, i: far_ptr(False, b.alloc(1, [0]), 1), nseg=2, via="far"))
    add("far_lands_on_far", set_ptr(lambda b, w, i: far_ptr(False, b.alloc(1, [b.seg[0][i]]), 1), nseg=2, via="far"))
    add("far_lands_on_capability", set_ptr(lambda b, w, i: far_ptr(False, b.alloc(1, [3]), 1), nseg=2, via="far"))
    add("far_lands_on_size_6", set_ptr(
        lambda b, w, i: far_ptr(False, b.alloc(1, [list_ptr(0, 6, 0)]), 1), nseg=2, via="far"))
    # ---- double far -------------------------------------------------------------------------------
    def dfar(first, second, nseg=3, **kw):
        def make(b, w, i):
            tag, start = w["slist_tag"], w["slist_first"]
            pad = b.alloc(1, [first(b, w, tag, start), second(b, w, tag, start)])
            return far_ptr(True, pad, 1)
        return set_ptr(make, nseg=nseg, via="far", **kw)

    to_first = lambda b, w, tag, start: far_ptr(False, start[1], start[0])
    to_tag = lambda b, w, tag, start: far_ptr(False, tag[1], tag[0])
    tag_of = lambda b, w, tag, start: b.seg[tag[0]][tag[1]]
    list_of = lambda b, w, tag, start: list_ptr(0, 7, w["slist_words"])
    add("dfar_pad_one_word_left", set_ptr(lambda b, w, i: far_ptr(True, b.alloc(1, [0]), 1), nseg=3, via="far"))
    add("dfar_pad_past_segment", set_ptr(lambda b, w, i: far_ptr(True, 1 << 20, 1), nseg=3, via="far"))
    add("dfar_segment_id", set_ptr(lambda b, w, i: far_ptr(True, 0, 3), nseg=3, via="far"))
    add("dfar_first_is_struct", dfar(lambda b, w, t, s: struct_ptr(0, 1, 1), tag_of))
    add("dfar_first_is_null", dfar(lambda b, w, t, s: 0, tag_of))
    add("dfar_first_is_double", dfar(lambda b, w, t, s: far_ptr(True, s[1], s[0]), tag_of))
    add("dfar_first_segment_id", dfar(lambda b, w, t, s: far_ptr(False, s[1], 3), tag_of))
    add("dfar_a_good", dfar(to_first, tag_of))
    add("dfar_a_count_negative", dfar(to_first, lambda b, w, t, s: (tag_of(b, w, t, s) & ~0xFFFFFFFF) | (0x3FFFFFFF << 2)))
    add("dfar_a_past_segment", dfar(to_first, lambda b, w, t, s: struct_ptr(1 << 12, 2, 3)))
    add("dfar_a_starts_past_segment", dfar(lambda b, w, t, s: far_ptr(False, 1 << 20, s[0]), tag_of))
    add("dfar_a_empty_at_segment_end", dfar(lambda b, w, t, s: far_ptr(False, len(b.seg[s[0]]) + 2, s[0]),
                                            lambda b, w, t, s: struct_ptr(0, 2, 3)))
    add("dfar_a_empty_past_segment_end", dfar(lambda b, w, t, s: far_ptr(False, len(b.seg[s[0]]) + 3, s[0]),
                                              lambda b, w, t, s: struct_ptr(0, 2, 3)))
    add("dfar_b_good", dfar(to_tag, list_of))
    add("dfar_b_size_6", dfar(to_tag, lambda b, w, t, s: list_ptr(0, 6, w["slist_words"])))
    add("dfar_b_tag_past_segment", dfar(lambda b, w, t, s: far_ptr(False, 1 << 20, t[0]), list_of))
    add("dfar_b_words_one_short", dfar(to_tag, lambda b, w, t, s: list_ptr(0, 7, w["slist_words"] - 1)))
    add("dfar_b_words_past_segment", dfar(to_tag, lambda b, w, t, s: list_ptr(0, 7, 1 << 15)))
    add("dfar_second_is_far", dfar(to_tag, lambda b, w, t, s: far_ptr(False, 0, 0)))
    add("dfar_second_is_capability", dfar(to_tag, lambda b, w, t, s: 3))
    # ---- the pointer list's pointer -----------------------------------------------------------------
    pl = lambda make, **kw: set_ptr(lambda b, w, i: make(b, w, i, w["plist_first"][1] - i - 1), index=1, **kw)
    add("plist_size_5", pl(lambda b, w, i, o: list_ptr(o, 5, w["plist_count"])))
    add("plist_size_7", pl(lambda b, w, i, o: list_ptr(o, 7, 1)))
    add("plist_size_5_past_end", pl(lambda b, w, i, o: list_ptr(o, 5, 1 << 20)))
    add("plist_past_end", pl(lambda b, w, i, o: list_ptr(o, 6, 1 << 20)))
    add("plist_negative", pl(lambda b, w, i, o: list_ptr(-i - 2, 6, 0)))
    add("plist_is_struct", pl(lambda b, w, i, o: struct_ptr(o, 0, 1)))
    add("plist_far_segment_id", pl(lambda b, w, i, o: far_ptr(False, 0, 9)))
    add("plist_dfar_first_not_far", pl(lambda b, w, i, o: far_ptr(True, w["root"][1], 0)))
    add("plist_chain_7_hops", message(2, via="far", edit=lambda b, w: b.point(
        (0, w["root_ptrs"][1] + 1), w["plist_first"], lambda o: list_ptr(o, 6, w["plist_count"]), via="far", hops=7)))
    add("plist_chain_8_hops", message(2, via="far", edit=lambda b, w: b.point(
        (0, w["root_ptrs"][1] + 1), w["plist_first"], lambda o: list_ptr(o, 6, w["plist_count"]), via="far", hops=8)))

    # ---- elements that fail ---------------------------------------------------------------------------
    def set_slot(k, make, name="plist", **kw):
        def edit(b, w):
            s, first = w[name + "_first"]
            b.seg[s][first + k] = make(b, w, first + k)
        return message(edit=edit, **kw)

    add("slot_far_segment_id", set_slot(0, lambda b, w, i: far_ptr(False, 0, 5)))
    add("slot_far_pad_past_segment", set_slot(0, lambda b, w, i: far_ptr(False, 1 << 20, 0)))
    add("slot_dfar_first_not_far", set_slot(2, lambda b, w, i: far_ptr(True, w["root"][1], 0)))
    add("slot_list_past_end", set_slot(2, lambda b, w, i: list_ptr(0, 3, 1 << 20)))
    add("slot_list_negative", set_slot(2, lambda b, w, i: list_ptr(-i - 2, 3, 0)))
    add("slot_struct_truncated", set_slot(3, lambda b, w, i: struct_ptr(0, 1 << 12, 1)))
    add("slot_struct_negative", set_slot(3, lambda b, w, i: struct_ptr(-i - 2, 1, 1)))
    add("slot_chain_8_hops", message(2, via="far", edit=lambda b, w: b.point(
        (w["plist_first"][0], w["plist_first"][1]), (0, w["root"][1]), lambda o: struct_ptr(o, 1, 4), via="far",
        hops=8, pad_seg=0)))

    def elem_ptr(k, index, make, **kw):
        def edit(b, w):
            s, first = w["slist_first"]
            b.seg[s][first + k * 5 + 2 + index] = make(b, w)
        return message(edit=edit, **kw)

    add("elem_text_is_words", elem_ptr(1, 0, lambda b, w: list_ptr(0, 5, 0)))
    add("elem_text_null", elem_ptr(1, 0, lambda b, w: 0))
    add("elem_data_null", elem_ptr(1, 1, lambda b, w: 0))
    add("elem_child_null", elem_ptr(2, 2, lambda b, w: 0))
    add("elem_child_is_list", elem_ptr(2, 2, lambda b, w: list_ptr(0, 2, 0)))
    add("elem_child_far_segment_id", elem_ptr(0, 2, lambda b, w: far_ptr(False, 0, 1)))
    add("elem_data_past_end", elem_ptr(0, 1, lambda b, w: list_ptr(0, 2, 1 << 20)))
    return out
