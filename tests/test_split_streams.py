"""The split-streams corpus (tests/split_streams.py) really holds the shapes that
tests/test_gpu_split_streams.py relies on, and the new entry points are declared, exported and
bound (no GPU needed)."""
import os
import re

import numpy as np

import capnp_packed as cp
import framer_streams as fs
import reader_streams as rs
import split_streams as ss
from split_streams import W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capnp_packed_split_workspace_bytes", "capnp_packed_split_streams")
ERRORS = (cp.INVALID_SEGMENT_COUNT, cp.SEGMENT_COUNT_LIMIT_EXCEEDED, cp.MESSAGE_TOO_LARGE,
          cp.INVALID_PACKED_MESSAGE)


def by_name(name):
    return next(s for s in ss.corpus() if s.name == name)


def header_end(s, m):
    """Stream byte behind the record that completes message m's segment table."""
    start = s.msgs[m][0] if m < len(s.msgs) else s.consumed
    return start + rs.read_message(s.data[start:], header_only=True).consumed


# ---- the API ----

def test_symbols_declared_exported_and_bound():
    L = cp.lib()
    with open(cp.HEADER_PATH) as f:
        h = f.read()
    with open(os.path.join(ROOT, "zig", "packed_ffi.zig")) as f:
        z = f.read()
    for name in NEW:
        assert name in cp.SIGNATURES
        assert hasattr(L, name)
        assert re.search(r"\b" + name + r"\(", h)
        assert re.search(r'extern "capnp_packed" fn ' + name + r"\(", z)
    assert L.capnp_packed_abi_version() == 2
    for fn in ("split_workspace", "split_streams", "read_packed_messages"):
        assert callable(getattr(cp, fn))


def test_argument_checks_answer_before_any_device_work():
    import ctypes
    buf = ctypes.create_string_buffer(8192 + 512)
    a = (ctypes.addressof(buf) + 255) & ~255
    L = cp.lib()
    need = L.capnp_packed_split_workspace_bytes(4, 0)
    assert 0 < need <= 4096 and L.capnp_packed_split_workspace_bytes(0, 1 << 30) == 0
    assert L.capnp_packed_split_workspace_bytes(4, 100 * W) > need
    x = a + 4096  # stands in for every device array: nothing may be read

    def call(ws, ws_bytes, first=x, n=4):
        return L.capnp_packed_split_streams(x, x, x, n, 8, first, x, x, x, 0, x, x, ws, ws_bytes, 0)

    assert call(0, 0) == cp.INVALID_ARGUMENT               # NULL
    assert call(a, need - 1) == cp.INVALID_ARGUMENT        # short
    assert call(a + 8, need) == cp.INVALID_ARGUMENT        # 8- but not 256-aligned
    assert "256" in cp.last_error()
    assert call(a, need, first=0) == cp.INVALID_ARGUMENT   # no msg_first
    assert call(a, need, first=0, n=0) == cp.INVALID_ARGUMENT
    del buf


def test_workspace_bytes_grow_with_n_and_bound_up_to_the_table_limit():
    L = cp.lib()
    sizes = [L.capnp_packed_split_workspace_bytes(n, 0) for n in (1, 2, 63, 64, 65, 1000, 1 << 16, 1 << 20)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    by_bound = [L.capnp_packed_split_workspace_bytes(16, b) for b in (0, W - 1, W, 10 * W, 1 << 30, 1 << 40, 1 << 62)]
    assert by_bound[0] == by_bound[1] < by_bound[2] < by_bound[3] < by_bound[4]
    assert by_bound[4] <= by_bound[5] == by_bound[6]  # the table's limit (n / 8 + 32768 windows)


# ---- statuses and counts ----

def test_every_final_status_occurs():
    seen = {s.status for s in ss.corpus()}
    assert seen == {cp.OK, cp.END_OF_STREAM, *ERRORS}


def test_0_1_and_several_messages_in_front_of_every_error():
    for st in (cp.END_OF_STREAM, *ERRORS):
        counts = {min(len(s.msgs), 2) for s in ss.corpus() if s.status == st}
        assert counts == {0, 1, 2}, (st, counts)


def test_expectation_is_the_whole_stream_loop():
    for s in ss.corpus()[::7]:
        msgs, left, status, _ = fs.whole_stream(s.data)
        assert (tuple(msgs), len(s.data) - left, status) == (s.msgs, s.consumed, s.status)
        assert s.consumed == sum(m[1] for m in s.msgs)
        assert (s.status == cp.OK) == (s.consumed == len(s.data))


# ---- one-window shapes ----

def test_one_window_shapes():
    e = by_name("empty")
    assert (e.data, e.msgs, e.consumed, e.status) == (b"", (), 0, cp.OK)
    for name, n in (("cut_in_header", 0), ("cut_in_header_after_2", 2)):
        s = by_name(name)
        assert s.status == cp.END_OF_STREAM and len(s.msgs) == n and len(s.data) < W
        rest = s.data[s.consumed:]  # the framed length is never known
        assert len(rest) >= 2 and rs.read_message(rest, header_only=True).status == rs.END_OF_STREAM
    s = by_name("cut_in_last_record")
    assert s.status == cp.END_OF_STREAM and len(s.msgs) == 1 and len(s.data) < W
    rest = s.data[s.consumed:]
    assert rs.read_message(rest, header_only=True).status is None  # the header is whole
    whole = by_name("ends_at_message_end")
    assert whole.status == cp.OK and len(whole.msgs) == 3 and whole.consumed == len(whole.data) < W
    start, used, _ = whole.msgs[-1]
    msg = whole.data[start:]
    assert msg[:-1] == rest and rs._record_starts(msg)[-1][0] < len(rest)  # one byte short, inside the last record


# ---- window-grid shapes ----

def test_window_grid_shapes():
    ends = {(m[0] + m[1]) % W for s in ss.corpus() if len(s.data) > W for m in s.msgs if m[0] + m[1] > W}
    assert 0 in ends and 1 in ends
    places = {name.split("_", 1)[1].rsplit("_", 1)[0] for name in (s.name for s in ss.corpus())
              if name.startswith("exit_")}
    assert places == set(fs.WINDOW_EXIT_PLACES)
    # a last record across a window line: it starts a byte before the line and is longer than that
    s = next(s for s in ss.corpus() if s.name.startswith("exit_last_record_starts_1_before_grid"))
    big = max(s.msgs, key=lambda m: m[1])
    start = big[0] + rs._record_starts(s.data[big[0]:big[0] + big[1]])[-1][0]
    assert start % W == W - 1 and big[0] + big[1] > start + 1
    # a header across a window line
    s = by_name("header_across_window_line")
    m = next(i for i, msg in enumerate(s.msgs) if msg[0] % W == W - 1)
    assert s.msgs[m][0] > 0 and header_end(s, m) > s.msgs[m][0] + 1 and s.status == cp.OK


# ---- long streams ----

def test_long_streams():
    many = by_name("many_messages")
    assert len(many.msgs) == ss.N_MANY >= 200 and many.status == cp.OK
    cut = by_name("many_messages_then_cut")
    assert len(cut.msgs) == ss.N_MANY > 64 and cut.status == cp.END_OF_STREAM
    two = by_name("two_large_messages")
    assert len(two.msgs) == 2 and all(m[1] >= ss.BIG_WINDOWS * W for m in two.msgs) and two.status == cp.OK
    mixed = by_name("small_then_two_large_then_cut")
    assert len(mixed.msgs) == 3 and mixed.status == cp.END_OF_STREAM


# ---- the layout ----

def test_layout_is_dense_shuffled_and_fenced():
    streams = ss.corpus()
    for shift in (0, 1):
        lay = ss.layout(streams, shift=shift)
        assert sorted(lay.order) == list(range(len(streams))) and list(lay.order) != sorted(lay.order)
        assert lay.off[0] == ss.FRONT_LEN + shift and (lay.buf[:lay.off[0]] == ss.FRONT).all()
        assert (lay.off[1:] == lay.off[:-1] + lay.length[:-1]).all()  # no gap
        end = int(lay.off[-1] + lay.length[-1])
        assert len(lay.buf) == end + ss.BACK_LEN and (lay.buf[end:] == ss.BACK).all()
        for s in (0, len(streams) // 2, len(streams) - 1):
            d = streams[lay.order[s]].data
            assert lay.buf[lay.off[s]:lay.off[s] + len(d)].tobytes() == d
        exp = ss.expect(streams, lay)
        assert exp.first[-1] == len(exp.off) == sum(len(s.msgs) for s in streams)
        assert (np.diff(exp.first) == [len(streams[i].msgs) for i in lay.order]).all()
    assert ss.FRONT != ss.BACK and ss.FRONT and ss.BACK


def test_frames_are_the_oracles():
    s = by_name("ends_at_message_end")
    assert ss.frames(s) == fs.oracle_frames(s.data)[0]
