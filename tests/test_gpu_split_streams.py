"""capnp_packed_split_streams on the device: dense streams of packed messages split into their
messages, against the whole-stream loop of the C oracle (tests/split_streams.py).

Every table is filled with a canary first; rows the call must not write are checked for it."""
import numpy as np
import pytest

import capnp_packed as cp
import framer_streams as fs
import split_streams as ss

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = -0x5A5A5A5A5A5A5A5B
CANARY32 = -0x5A5A5A5B
SLACK = 37  # canary rows behind the last expected row


class Split:
    """One split_streams call over a device buffer and its results on the host."""

    def __init__(self, d_in, off, length, rows, bound=None, with_stream=True, ws="auto", stream=None):
        self.n = n = len(off)
        self.d_in = d_in
        self.off = torch.as_tensor(np.asarray(off, dtype=np.int64)).to(DEV)
        self.len = torch.as_tensor(np.asarray(length, dtype=np.int64)).to(DEV)
        self.first = torch.full((n + 1,), CANARY, dtype=torch.int64, device=DEV)
        self.tab = torch.full((3, rows + SLACK), CANARY, dtype=torch.int64, device=DEV)
        self.ms = torch.full((rows + SLACK,), CANARY32, dtype=torch.int32, device=DEV) if with_stream else None
        self.consumed = torch.full((n,), CANARY, dtype=torch.int64, device=DEV)
        self.status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        self.rows = rows
        if ws == "auto":
            ws = cp.split_workspace(n, int(np.sum(length)) if bound is None else bound, device=DEV) if n else None
        self.ws = ws
        self.stream = stream
        self.call()

    def call(self):
        r = self.rows
        cp.split_streams(self.d_in, self.off, self.len, self.first, self.tab[0][:r], self.tab[1][:r], self.tab[2][:r],
                         self.consumed, self.status, msg_stream=None if self.ms is None else self.ms[:r], ws=self.ws,
                         stream=self.stream)

    def check(self, exp):
        """first / consumed / status in full; the rows below self.rows; canaries from there on."""
        torch.cuda.synchronize()
        assert np.array_equal(self.first.cpu().numpy(), exp.first)
        assert np.array_equal(self.status.cpu().numpy(), exp.status)
        assert np.array_equal(self.consumed.cpu().numpy(), exp.consumed)
        k = min(self.rows, len(exp.off))
        tab = self.tab.cpu().numpy()
        for got, want, what in zip(tab, (exp.off, exp.length, exp.framed), ("off", "len", "framed")):
            bad = np.flatnonzero(got[:k] != want[:k])
            assert bad.size == 0, f"msg_{what}: row {bad[:1]} is {got[bad[:1]]}, not {want[bad[:1]]}"
            assert (got[k:] == CANARY).all(), f"msg_{what}: a row at or past {k} was written"
        if self.ms is not None:
            ms = self.ms.cpu().numpy()
            assert np.array_equal(ms[:k], exp.stream[:k]) and (ms[k:] == CANARY32).all()


@pytest.fixture(scope="module")
def batch():
    """The corpus laid out at shift 0 and 1, on the device, with its expectations."""
    streams = ss.corpus()
    out = {}
    for shift in (0, 1):
        lay = ss.layout(streams, shift=shift)
        out[shift] = (lay, ss.expect(streams, lay), torch.from_numpy(lay.buf).to(DEV))
    return streams, out


@pytest.mark.parametrize("shift", [0, 1])
def test_whole_corpus_in_one_call(batch, shift):
    streams, by_shift = batch
    lay, exp, d_in = by_shift[shift]
    Split(d_in, lay.off, lay.length, len(exp.off)).check(exp)


@pytest.mark.parametrize("part", ["half", "zero"])
def test_too_few_rows(batch, part):
    streams, by_shift = batch
    lay, exp, d_in = by_shift[0]
    rows = len(exp.off) // 2 if part == "half" else 0
    Split(d_in, lay.off, lay.length, rows).check(exp)


def test_without_msg_stream_and_counts_only(batch):
    streams, by_shift = batch
    lay, exp, d_in = by_shift[1]
    Split(d_in, lay.off, lay.length, len(exp.off), with_stream=False).check(exp)
    n = len(lay.off)
    first = torch.full((n + 1,), CANARY, dtype=torch.int64, device=DEV)
    consumed = torch.full((n,), CANARY, dtype=torch.int64, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.split_streams(d_in, torch.from_numpy(lay.off).to(DEV), torch.from_numpy(lay.length).to(DEV), first, None, None,
                     None, consumed, status)
    assert np.array_equal(first.cpu().numpy(), exp.first) and np.array_equal(status.cpu().numpy(), exp.status)


def test_window_tables_are_an_optimisation_only(batch):
    streams, by_shift = batch
    lay, exp, d_in = by_shift[0]
    L = cp.lib()
    n = len(lay.off)
    assert L.capnp_packed_split_workspace_bytes(n, 0) < L.capnp_packed_split_workspace_bytes(n, int(lay.length.sum()))
    assert (lay.length > ss.W).sum() > 100  # the multi-window streams
    Split(d_in, lay.off, lay.length, len(exp.off), bound=0).check(exp)
    # a table that holds a part of the windows only
    Split(d_in, lay.off, lay.length, len(exp.off), bound=int(lay.length.sum()) // 3).check(exp)


def test_rows_feed_lengths_to_offsets_and_decode_batch(batch):
    streams, by_shift = batch
    lay, exp, d_in = by_shift[1]
    total = len(exp.off)
    r = Split(d_in, lay.off, lay.length, total)
    framed = r.tab[2][:total]
    out_off = cp.lengths_to_offsets(framed)
    nbytes = int(out_off[total].item())
    assert nbytes == int(exp.framed.sum())
    d_out = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    out_len = torch.full((total,), -1, dtype=torch.int64, device=DEV)
    st = torch.full((total,), -1, dtype=torch.int32, device=DEV)
    cp.decode_batch(d_in, r.tab[0][:total], r.tab[1][:total], d_out, out_off, framed, out_len, st)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == cp.OK).all() and np.array_equal(out_len.cpu().numpy(), exp.framed)
    got = d_out.cpu().numpy()
    assert (got[nbytes:] == 0xA5).all()
    want = b"".join(b"".join(ss.frames(streams[i])) for i in lay.order)
    assert len(want) == nbytes and got[:nbytes].tobytes() == want


@pytest.mark.parametrize("dialect", ["zig", "cxx"])
def test_round_trip_with_the_dense_writer(dialect):
    rng = np.random.default_rng(0x5B117002)
    words = list(rng.integers(0, 200, 3000)) + [1, 40000] + list(rng.integers(0, 3000, 40))
    rng.shuffle(words)
    msgs = []
    for w in words:
        body = rng.integers(1, 256, 8 * int(w), dtype=np.uint8)
        body[rng.random(8 * int(w)) < (0.2, 0.5, 0.9)[int(w) % 3]] = 0
        msgs.append(cp.frame_segments([body.tobytes()]))
    sizes = {len(m) for m in msgs}
    assert {8, 16} <= sizes and max(sizes) == 8 + 8 * 40000  # an empty and a one-word segment, one of 320 KB
    n = len(msgs)
    in_len = np.array([len(m) for m in msgs], dtype=np.int64)
    in_off = np.concatenate(([0], np.cumsum(in_len)[:-1])).astype(np.int64)
    d_msgs = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()).to(DEV)
    base = 3
    d_pk = torch.full((base + int(in_len.sum()) * 5 // 4 + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    out_off = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
    out_len = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    est = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.encode_dense_batch(d_msgs, torch.from_numpy(in_off).to(DEV), torch.from_numpy(in_len).to(DEV), d_pk, out_off,
                          out_len, est, base=base, dialect=dialect)
    torch.cuda.synchronize()
    assert (est.cpu().numpy() == cp.OK).all()
    h_off = out_off.cpu().numpy()
    # the one stream, WITHOUT the writer's offsets
    r = Split(d_pk, [base], [int(h_off[n]) - base], n)
    torch.cuda.synchronize()
    assert r.first.cpu().tolist() == [0, n] and r.status.cpu().tolist() == [cp.OK]
    assert r.consumed.cpu().tolist() == [int(h_off[n]) - base]
    tab = r.tab.cpu().numpy()
    assert np.array_equal(tab[0][:n], h_off[:n]) and np.array_equal(tab[1][:n], out_len.cpu().numpy())
    assert np.array_equal(tab[2][:n], in_len) and (tab[:, n:] == CANARY).all()
    assert (r.ms.cpu().numpy()[:n] == 0).all()


def test_wide_batch():
    # 2^16 streams of one small message each: the grid-stride loops and a multi-block scan
    rng = np.random.default_rng(0x5B117003)
    small = [s.data[:s.consumed] for s in ss.corpus() if s.status == cp.OK and len(s.msgs) == 1 and len(s.data) < 600]
    assert len(small) >= 8
    n = 1 << 16
    pick = rng.integers(0, len(small), n)
    lens = np.array([len(small[i]) for i in pick], dtype=np.int64)
    off = 5 + np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    buf = np.frombuffer(bytes(5) + b"".join(small[i] for i in pick) + bytes(64), dtype=np.uint8).copy()
    framed = {i: next(s.msgs[0][2] for s in ss.corpus() if s.data[:s.consumed] == small[i] and len(s.msgs) == 1)
              for i in set(pick.tolist())}
    r = Split(torch.from_numpy(buf).to(DEV), off, lens, n)
    torch.cuda.synchronize()
    assert np.array_equal(r.first.cpu().numpy(), np.arange(n + 1)) and (r.status.cpu().numpy() == cp.OK).all()
    tab = r.tab.cpu().numpy()
    assert np.array_equal(tab[0][:n], off) and np.array_equal(tab[1][:n], lens) and (tab[:, n:] == CANARY).all()
    assert np.array_equal(tab[2][:n], np.array([framed[i] for i in pick.tolist()]))
    assert np.array_equal(r.ms.cpu().numpy()[:n], np.arange(n)) and np.array_equal(r.consumed.cpu().numpy(), lens)


def test_edges(batch):
    first = torch.full((3,), CANARY, dtype=torch.int64, device=DEV)
    none = torch.empty(0, dtype=torch.int64, device=DEV)
    cp.split_streams(None, none, none, first, None, None, None, none, torch.empty(0, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert first.cpu().tolist() == [0, CANARY, CANARY]  # n == 0
    # the workspace: NULL, misaligned, short
    streams, by_shift = batch
    lay, exp, d_in = by_shift[0]
    n, L = 4, cp.lib()
    need = L.capnp_packed_split_workspace_bytes(n, 0)
    ws = torch.empty(need // 8 + 64, dtype=torch.int64, device=DEV)
    r = Split(d_in, lay.off[:n], lay.length[:n], 64, ws=ws)
    p = lambda t: t.data_ptr()

    def raw(wsp, nbytes):
        return L.capnp_packed_split_streams(p(d_in), p(r.off), p(r.len), n, 64, p(r.first), p(r.tab[0]), p(r.tab[1]),
                                            p(r.tab[2]), 0, p(r.consumed), p(r.status), wsp, nbytes, 0)

    assert raw(0, 0) == cp.INVALID_ARGUMENT and raw(p(ws) + 8, need) == cp.INVALID_ARGUMENT
    assert raw(p(ws), need - 1) == cp.INVALID_ARGUMENT and raw(p(ws), need) == cp.OK
    # a stream longer than the header's limit: INVALID_ARGUMENT as its status, none of its bytes read
    length = lay.length[:n].copy()
    length[1] = (1 << 40) + 1
    r = Split(d_in, lay.off[:n], length, 64)
    torch.cuda.synchronize()
    st, fi = r.status.cpu().tolist(), r.first.cpu().tolist()
    assert st[1] == cp.INVALID_ARGUMENT and fi[2] == fi[1] and r.consumed.cpu().tolist()[1] == 0
    assert [st[0], st[2], st[3]] == [int(exp.status[i]) for i in (0, 2, 3)]


def test_offsets_above_4_gib():
    s = next(s for s in ss.corpus() if s.name == "ends_at_message_end")
    base = (1 << 32) + 12345
    d_in = torch.empty(base + len(s.data) + 4096, dtype=torch.uint8, device=DEV)
    d_in[base - 64:].fill_(0x5A)
    d_in[base:base + len(s.data)] = torch.from_numpy(np.frombuffer(s.data, dtype=np.uint8).copy()).to(DEV)
    r = Split(d_in, [base], [len(s.data)], 8)
    torch.cuda.synchronize()
    k = len(s.msgs)
    assert r.first.cpu().tolist() == [0, k] and r.status.cpu().tolist() == [cp.OK]
    tab = r.tab.cpu().numpy()
    assert tab[0][:k].tolist() == [base + m[0] for m in s.msgs] and tab[1][:k].tolist() == [m[1] for m in s.msgs]
    assert tab[2][:k].tolist() == [m[2] for m in s.msgs] and (tab[:, k:] == CANARY).all()


def test_graph_capture_replay(batch):
    streams, by_shift = batch
    lay, exp, d_in0 = by_shift[0]
    d_in = d_in0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r = Split(d_in, lay.off, lay.length, len(exp.off), stream=s)  # warm-up outside the capture
    s.synchronize()
    r.check(exp)
    r.stream = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.call()
    for _ in range(2):  # other work on the same buffers in between, then replay
        for t in (r.first, r.tab, r.consumed):
            t.fill_(CANARY)
        r.ms.fill_(CANARY32)
        r.status.fill_(-1)
        r.ws.fill_(-1)
        Split(by_shift[1][2], by_shift[1][0].off, by_shift[1][0].length, 16)
        g.replay()
        r.check(exp)


def test_read_packed_messages_on_the_host():
    by = {s.name: s for s in ss.corpus()}
    err = next(s for s in ss.corpus() if s.status == cp.INVALID_PACKED_MESSAGE and len(s.msgs) == 2)
    for s in (by["ends_at_message_end"], by["cut_in_last_record"], err):
        frames, rest, status = fs.oracle_frames(s.data)
        got, consumed, name = cp.read_packed_messages(s.data)
        assert got == frames and consumed == len(s.data) - len(rest) == s.consumed
        assert name == cp.lib().capnp_packed_status_name(status).decode() and status == s.status
    assert cp.read_packed_messages(b"") == ([], 0, cp.lib().capnp_packed_status_name(cp.OK).decode())
