"""The model of capnp_packed_list_heads_batch / capnp_packed_read_elements_batch
(tests/list_streams.py) pinned by what the reference's own interop test asserts on the fixtures
(tests/serialization/interop_test.zig:15-33, 73-83), and the coverage of the corpus the GPU test
runs: every status the two calls can return from framed bytes and both ways of every check of
the model (no GPU needed)."""
import struct

import pytest

import list_streams as ls
import struct_streams as ss
from list_streams import LIST_POINTER, LIST_STRUCT
from struct_streams import DATA, F, LIST_16, OK, TEXT, U32, fixture


def content(data, row):
    st, v, l, c = row
    assert st == OK
    return data[v:v + l]


@pytest.mark.parametrize("name", ["fixture_single.bin", "fixture_far.bin"])
def test_model_reads_the_widget_lists(name):
    data = fixture(name)
    head, rows = ls.read_list(data, LIST_STRUCT, 1, [F(U32, 0), F(U32, 4)])
    assert (head.status, head.count) == (OK, 3)
    assert [[r[1] for r in row] for row in rows] == [[1, 10], [2, 20], [3, 30]]
    head, rows = ls.read_list(data, LIST_POINTER, 2, [F(TEXT, 0)])
    assert (head.status, head.count, head.data_words, head.pointer_words) == (OK, 2, 0, 1)
    assert [content(data, row[0]) for row in rows] == [b"alpha", b"beta"]
    head, rows = ls.read_list(data, LIST_POINTER, 10, [F(LIST_16, 0)])
    assert (head.status, head.count) == (OK, 2)
    assert [content(data, row[0]) for row in rows] == [struct.pack("<2H", 7, 8), struct.pack("<3H", 9, 10, 11)]
    assert [row[0][3] for row in rows] == [2, 3]


def test_the_far_fixture_reaches_its_lists_through_single_far_pointers():
    m = ss.Msg(fixture("fixture_far.bin"))
    root = ss.get_root_struct(m)
    segs = set()
    for index in (1, 2, 10):
        pos, word = ss.pointer_at(m, root, index)
        assert word & 7 == 2  # a single far pointer
        segs.add(word >> 32)
    assert segs == {2, 3}
    # each list read as the other kind is the reference's error, not a crash
    data = fixture("fixture_far.bin")
    assert ls.read_list(data, LIST_POINTER, 1, [])[0].status == ss.INVALID_POINTER
    assert ls.read_list(data, LIST_STRUCT, 2, [])[0].status == ls.INVALID_INLINE_COMPOSITE_POINTER


def test_all_types_lists_are_the_same_in_binary_and_segmented():
    """the reference pins no values for TestAllTypes' lists: the model must read identical content
    from the one-segment file and from the 125-segment one (double-far pads of layout B)"""
    one, many = fixture("binary"), fixture("segmented")
    m = ss.Msg(many)
    root = ss.get_root_struct(m)
    for index in (15, 16, 17):
        pos, word = ss.pointer_at(m, root, index)
        assert word & 7 == 6  # a double far pointer
        first, second = m.word(word >> 32, ((word >> 3) & 0x1FFFFFFF) * 8), m.word(word >> 32, ((word >> 3) & 0x1FFFFFFF) * 8 + 8)
        assert second & 3 == 1  # layout B: a list pointer in the pad

    def readable(data, kind, index, fields):
        head, rows = ls.read_list(data, kind, index, fields)
        assert head.status == OK
        return (head.count, head.data_words, head.pointer_words), [
            [(st, data[v:v + l] if f.kind not in ss.WIDTH else v, l, c) for f, (st, v, l, c) in zip(fields, row)]
            for row in rows]

    fields = [F(k, o) for k, o in ((ss.U64, 0), (ss.U64, 8), (ss.U32, 20), (ss.U64, 40), (ss.U8, 47))]
    fields += [F(TEXT, 0), F(DATA, 1), F(TEXT, 0, path=(2,)), F(LIST_16, 6), F(TEXT, 19)]
    a, b = readable(one, LIST_STRUCT, 17, fields), readable(many, LIST_STRUCT, 17, fields)
    assert a == b and a[0] == (3, 6, 20)
    assert any(l for row in a[1] for st, v, l, c in row)  # not all defaults
    for index in (15, 16):
        pf = [F(TEXT, 0), F(DATA, 0), F(LIST_16, 0), F(ss.LIST_32, 0), F(ss.LIST_64, 0), F(ss.LIST_BIT, 0),
              F(U32, 0, path=(0,))]
        a, b = readable(one, LIST_POINTER, index, pf), readable(many, LIST_POINTER, index, pf)
        assert a == b and a[0][0] > 0
        assert any(st == OK and l for row in a[1] for st, v, l, c in row)


def test_corpus_layouts():
    names = [n for n, _ in ls.corpus()]
    assert len(names) == len(set(names))
    assert len(names) <= 260
    for name, data in ls.corpus():
        assert len(data) < 16384, name  # small messages: the GPU batches hold hundreds of them


def test_corpus_reaches_every_status_and_both_ways_of_every_check():
    ss.SEEN.clear()
    head_statuses, element_statuses = set(), set()
    for name, data in ls.corpus():
        for kind, index, path in ls.RUNS:
            fields = ls.fields_of(kind)
            head, rows = ls.read_list(data, kind, index, fields, path)
            head_statuses.add(head.status)
            if head.status != OK:
                assert head.tuple()[1:] == (0,) * 7 and not rows, name
                continue
            m = ss.Msg(data)
            for k, row in enumerate(rows):
                for st, v, l, c in row:
                    element_statuses.add(st)
                    if st != OK:
                        assert (v, l, c) == (0, 0, 0), name
                if kind == LIST_POINTER:  # the struct-of-one-pointer reading is the list readers'
                    lst = (head.segment, head.elems_off - m.starts[head.segment], head.count, 0, 1)
                    assert row == [ls.reader_field(m, lst, k, f) for f in fields], (name, k)
    missing = [(c, way) for c in ls.CHECKS + ss.CHECKS for way in (False, True) if (c, way) not in ss.SEEN]
    assert not missing, missing
    assert {c for c, _ in ss.SEEN} == set(ls.CHECKS + ss.CHECKS + ls.ONE_WAY)
    assert ("sget.bounds", True) not in ss.SEEN
    # every status of the two calls but INVALID_ARGUMENT (the batch layout's, or a start array that
    # is not the heads') and EMPTY_MESSAGE (no table parse gives a message without segments)
    assert head_statuses == {OK, ss.END_OF_STREAM, ss.INVALID_SEGMENT_COUNT, ss.SEGMENT_COUNT_LIMIT_EXCEEDED,
                             ss.TRUNCATED_MESSAGE, ss.NESTING_LIMIT_EXCEEDED, ss.INVALID_SEGMENT_ID,
                             ss.INVALID_POINTER, ss.OUT_OF_BOUNDS, ss.INVALID_FAR_POINTER,
                             ls.INVALID_INLINE_COMPOSITE_POINTER}
    assert element_statuses == {OK, ss.TRUNCATED_MESSAGE, ss.NESTING_LIMIT_EXCEEDED, ss.INVALID_SEGMENT_ID,
                                ss.INVALID_POINTER, ss.OUT_OF_BOUNDS, ss.INVALID_FAR_POINTER}


def test_error_arms_of_the_struct_list():
    by_name = dict(ls.corpus())
    want = {
        "near_size_6": 21, "near_tag_negative": 18, "near_tag_past_segment": 18, "near_pointer_is_capability": 17,
        "near_pointer_is_struct": 17, "near_words_one_short": 21, "near_words_past_segment": 18,
        "near_tag_is_list": 21, "near_tag_count_negative": 21, "far_segment_id": 16, "far_pad_past_segment": 18,
        "far_lands_on_struct": 17, "far_lands_on_far": 17, "far_lands_on_null": 17, "dfar_pad_one_word_left": 18,
        "dfar_first_is_struct": 20, "dfar_first_is_double": 20, "dfar_first_segment_id": 16,
        "dfar_a_count_negative": 21, "dfar_a_past_segment": 18, "dfar_a_empty_past_segment_end": 18,
        "dfar_b_size_6": 21, "dfar_b_tag_past_segment": 18, "dfar_b_words_one_short": 21,
        "dfar_b_words_past_segment": 18, "dfar_b_tag_is_list": 21, "dfar_second_is_far": 21,
        "dfar_second_is_capability": 21, "near_words_with_slack": 0, "dfar_a_empty_at_segment_end": 0,
        "dfar_a_good": 0, "dfar_b_good": 0,
    }
    for name, status in want.items():
        assert ls.read_list(by_name[name], LIST_STRUCT, 0, [])[0].status == status, name
    # null and missing pointers
    assert ls.read_list(by_name["near"], LIST_STRUCT, 3, [])[0].status == ss.INVALID_POINTER
    assert ls.read_list(by_name["near"], LIST_STRUCT, 4, [])[0].status == ss.OUT_OF_BOUNDS
    assert ls.read_list(by_name["near"], LIST_POINTER, 3, [])[0].status == ss.INVALID_POINTER
    assert ls.read_list(by_name["near"], LIST_POINTER, 4, [])[0].status == ss.OUT_OF_BOUNDS


def test_pointer_list_bounds_come_before_the_element_size_and_depth_is_seven_hops():
    by_name = dict(ls.corpus())
    run = lambda name: ls.read_list(by_name[name], LIST_POINTER, 1, [])[0].status
    assert run("plist_size_5") == ss.INVALID_POINTER and run("plist_size_5_past_end") == ss.OUT_OF_BOUNDS
    assert run("plist_chain_7_hops") == OK and run("plist_chain_8_hops") == ss.NESTING_LIMIT_EXCEEDED


def test_zero_word_elements_read_as_defaults():
    data = dict(ls.corpus())["zero_word_elements"]
    head, rows = ls.read_list(data, LIST_STRUCT, 0, [F(U32, 0), F(TEXT, 0), F(DATA, 0)], limit=5)
    assert (head.count, head.data_words, head.pointer_words) == (1000, 0, 0)
    assert rows == [[(OK, 0, 0, 0), (OK, 0, 0, 0), (ss.OUT_OF_BOUNDS, 0, 0, 0)]] * 5
