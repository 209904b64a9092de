"""The model of capnp_packed_read_fields_batch (tests/struct_streams.py) pinned by the four
interop fixtures, and the coverage of the corpus the GPU test runs: every status the call can
return and both ways of every check of the model (no GPU needed)."""
import pytest

import struct_streams as ss
from struct_streams import DATA, F, TABLES, TEXT, U8, U32, check_table, fixture

@pytest.mark.parametrize("name", sorted(TABLES))
def test_model_reads_the_fixtures(name):
    data = fixture(name)
    check_table(data, TABLES[name], ss.read_fields(data, [row[0] for row in TABLES[name]]))


def test_fixture_shapes():
    for name, shape in (("fixture_single.bin", (1, 11)), ("fixture_far.bin", (1, 11)), ("binary", (6, 20)),
                        ("segmented", (6, 20))):
        m = ss.Msg(fixture(name))
        root = ss.get_root_struct(m)
        assert (root.data_words, root.pointers) == shape
    m = ss.Msg(fixture("segmented"))
    assert len(m.segments) == 125
    assert m.word(0, 0) & 7 == 6 and m.word(0, 0) >> 32 == 124  # a double-far root landing in segment 124
    assert ss.get_root_struct(m).seg == 1
    m = ss.Msg(fixture("fixture_far.bin"))
    assert m.word(0, 0) & 7 == 2 and ss.get_root_struct(m).seg == 1


def test_corpus_layouts():
    names = [n for n, _ in ss.corpus()]
    assert len(names) == len(set(names))
    assert len(names) <= 260  # two rounds of the 130-message GPU batch
    segs = set()
    for name, data in ss.corpus():
        try:
            segs.add(len(ss.Msg(data).segments))
        except ss.RefError:
            pass
    assert {1, 2, 3, 5, 512} <= segs


def test_corpus_reaches_every_status_and_both_ways_of_every_check():
    ss.SEEN.clear()
    statuses = set()
    for name, data in ss.corpus():
        for st, v, l, c in ss.read_fields(data, ss.FIELDS):
            statuses.add(st)
            if st != ss.OK:
                assert (v, l, c) == (0, 0, 0), name
    missing = [(c, way) for c in ss.CHECKS for way in (False, True) if (c, way) not in ss.SEEN]
    assert not missing, missing
    assert {c for c, _ in ss.SEEN} == set(ss.CHECKS)
    # every status of the call but the two no framed message can produce through the model:
    # INVALID_ARGUMENT belongs to the batch layout (a misaligned offset, a 4-GiB length) and
    # EMPTY_MESSAGE needs a message without segments, which Message.init never returns
    assert statuses == {ss.OK, ss.END_OF_STREAM, ss.INVALID_SEGMENT_COUNT, ss.SEGMENT_COUNT_LIMIT_EXCEEDED,
                        ss.TRUNCATED_MESSAGE, ss.NESTING_LIMIT_EXCEEDED, ss.INVALID_SEGMENT_ID,
                        ss.INVALID_POINTER, ss.OUT_OF_BOUNDS, ss.INVALID_FAR_POINTER}


def test_far_chain_depth_is_seven_hops():
    by_name = dict(ss.corpus())
    root = [F(U8, 0)]
    assert ss.read_fields(by_name["root_chain_7_hops"], root)[0][0] == ss.OK
    assert ss.read_fields(by_name["root_chain_8_hops"], root)[0][0] == ss.NESTING_LIMIT_EXCEEDED
    data = [F(DATA, 1)]
    assert ss.read_fields(by_name["list_chain_7_hops"], data)[0] == ss.read_fields(by_name["2_segments_far_root"], data)[0]
    assert ss.read_fields(by_name["list_chain_8_hops"], data)[0][0] == ss.NESTING_LIMIT_EXCEEDED
    assert ss.read_fields(by_name["child_chain_8_hops"], [F(U32, 0, path=(2,))])[0][0] == ss.NESTING_LIMIT_EXCEEDED


def test_bounds_error_comes_before_the_element_size_error():
    by_name = dict(ss.corpus())
    assert ss.read_fields(by_name["data_wrong_size_and_past_end"], [F(DATA, 1)])[0][0] == ss.OUT_OF_BOUNDS
    assert ss.read_fields(by_name["data_bytes_as_words"], [F(DATA, 1)])[0][0] == ss.INVALID_POINTER
    assert ss.read_fields(by_name["text_bytes_as_words"], [F(TEXT, 0)])[0][0] == ss.INVALID_POINTER


def test_layout_keeps_messages_aligned_and_apart():
    msgs = [d for _, d in ss.corpus()]
    buf, offs, lens = ss.layout(msgs, list(range(len(msgs))))
    end = 0
    for i, (o, l) in enumerate(zip(offs, lens)):
        assert o % 8 == 0 and o >= end + 8 and buf[o:o + l] == msgs[i]
        assert 0 not in buf[end:o]
        end = o + l
