"""capnp_packed_encode_framed / _framed_batch / _framed_dense_batch: the
encoders over framed messages. Under the C++ dialect a message's segment table and each of its
segments are packed as pieces of their own, which is what capnp convert binary:packed and
pycapnp write (tests/golden/fixtures); under the Zig dialect the bytes are packPacked's and the
framing only adds the per-unit checks.

Every unit is compared with the model of tests/framed_streams.py (expected bytes from
tests/pyref_cxx.py and oracle.pack, statuses from a plain-Python Message.init plus the
trailing-words rule). Slots and streams are filled with a canary first.
"""
import os

import numpy as np
import pytest

import capnp_packed as cp
import framed_streams as fs
import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "fixtures")
PAIRS = [("binary", "packed"), ("segmented", "segmented-packed"),
         ("fixture_single.bin", "fixture_single_packed.bin"), ("fixture_far.bin", "fixture_far_packed.bin")]
DEV = "cuda"
CANARY = 0xA5
DIALECTS = ("zig", "cxx")


def fixture(name: str) -> bytes:
    with open(os.path.join(FIX, name), "rb") as f:
        return f.read()


def zig_pack(b: bytes) -> bytes:
    st, p = oracle.pack(b)
    assert st == oracle.OK
    return p


def i64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)


class Layout:
    """Units laid out in one input buffer (256-B aligned on the device); pad[i] extra bytes go
    in front of unit i."""

    def __init__(self, units, pad=None):
        self.units = [bytes(u) for u in units]
        n = len(self.units)
        pad = [0] * n if pad is None else pad
        self.in_len = np.array([len(u) for u in self.units], dtype=np.int64)
        self.in_off = np.zeros(n, dtype=np.int64)
        pos = 0
        for i, u in enumerate(self.units):
            pos += pad[i]
            self.in_off[i] = pos
            pos += len(u)
        self.h_in = np.zeros(pos + 16, dtype=np.uint8)
        for i, u in enumerate(self.units):
            self.h_in[self.in_off[i]:self.in_off[i] + len(u)] = np.frombuffer(u, dtype=np.uint8)
        self.n = n
        self.d_in = torch.from_numpy(self.h_in).to(DEV)
        assert self.d_in.data_ptr() % 256 == 0
        self.d_off = i64(self.in_off)
        self.d_len = i64(self.in_len)

    def model(self, dialect):
        """(statuses, pieces) of every unit."""
        exp = [fs.expected(u, dialect, zig_pack, address=int(o)) for u, o in zip(self.units, self.in_off)]
        return np.array([e[0] for e in exp], dtype=np.int32), [e[1] for e in exp]


def words8(layout_units):
    """Pads that put every unit on a word boundary whatever its length."""
    pad, pos = [], 0
    for u in layout_units:
        p = (-pos) % 8
        pad.append(p)
        pos += p + len(u)
    return pad


class Slots:
    """One encode_framed_batch call into canary-filled slots (caps: per-unit capacities;
    default: room for any data of the unit's length)."""

    def __init__(self, lay, dialect, caps=None, sizes_only=False, ws=None):
        n = lay.n
        self.caps = np.array([cp.encode_bound(int(x) - int(x) % 8) + 16 for x in lay.in_len] if caps is None else caps,
                             dtype=np.int64)
        room = self.caps + 32  # canary after every slot
        self.off = np.concatenate(([16], 16 + np.cumsum(room)[:-1])).astype(np.int64)
        self.d_out = torch.full((int(16 + room.sum()),), CANARY, dtype=torch.uint8, device=DEV)
        self.len = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        self.st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        cp.encode_framed_batch(lay.d_in, lay.d_off, lay.d_len, None if sizes_only else self.d_out, i64(self.off),
                               i64(self.caps), self.len, self.st, ws=ws, dialect=dialect)
        torch.cuda.synchronize()
        self.h_out = self.d_out.cpu().numpy()
        self.h_len = self.len.cpu().numpy()
        self.h_st = self.st.cpu().numpy()

    def check(self, status, pieces):
        """Every unit's status, length and bytes; everything else is still the canary."""
        want_len = np.array([len(p) for p in pieces], dtype=np.int64)
        assert np.array_equal(self.h_st, status), np.flatnonzero(self.h_st != status)[:8]
        assert np.array_equal(self.h_len, want_len), np.flatnonzero(self.h_len != want_len)[:8]
        expect = np.full_like(self.h_out, CANARY)
        for o, p in zip(self.off, pieces):
            expect[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
        if not np.array_equal(self.h_out, expect):
            bad = int(np.flatnonzero(self.h_out != expect)[0])
            unit = int(np.searchsorted(self.off, bad, side="right")) - 1
            raise AssertionError(f"slots differ at byte {bad} (unit {unit}, byte {bad - int(self.off[unit])} of its slot)")


class Dense:
    """One encode_framed_dense_batch call on a canary-filled output."""

    def __init__(self, lay, dialect, out_bytes, base=0, cap=None, ws=None, stream=None, sizes_only=False):
        n = lay.n
        self.d_out = None if sizes_only else torch.full((out_bytes,), CANARY, dtype=torch.uint8, device=DEV)
        self.off = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
        self.len = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        self.st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        self.base = base
        self.args = dict(base=base, cap=cap, dialect=dialect, ws=ws, stream=stream)
        self.lay = lay
        self.call()

    def call(self):
        lay = self.lay
        cp.encode_framed_dense_batch(lay.d_in, lay.d_off, lay.d_len, self.d_out, self.off, self.len, self.st,
                                     **self.args)

    def fetch(self):
        torch.cuda.synchronize()
        self.h_off = self.off.cpu().numpy()
        self.h_len = self.len.cpu().numpy()
        self.h_st = self.st.cpu().numpy()
        assert not (self.h_st == cp.DEVICE_ERROR).any(), "a look-back gave up"
        self.h_out = None if self.d_out is None else self.d_out.cpu().numpy()
        return self

    def check(self, status, pieces):
        """The offsets are the running sum, every unit's bytes are its piece (none for a failed
        unit), everything outside [base, off[n]) is still the canary."""
        self.fetch()
        lens = np.array([len(p) for p in pieces], dtype=np.int64)
        exp_off = self.base + np.concatenate(([0], np.cumsum(lens)))
        assert np.array_equal(self.h_st, status), np.flatnonzero(self.h_st != status)[:8]
        assert np.array_equal(self.h_len, lens), np.flatnonzero(self.h_len != lens)[:8]
        assert np.array_equal(self.h_off, exp_off)
        end = int(exp_off[-1])
        stream = np.frombuffer(b"".join(pieces), dtype=np.uint8)
        got = self.h_out[self.base:end]
        if not np.array_equal(got, stream):
            bad = int(np.flatnonzero(got != stream)[0])
            unit = int(np.searchsorted(exp_off, self.base + bad, side="right")) - 1
            raise AssertionError(f"stream differs at byte {bad} (unit {unit}, {len(self.lay.units[unit])} B in)")
        assert (self.h_out[:self.base] == CANARY).all(), "bytes below out_base were written"
        assert (self.h_out[end:] == CANARY).all(), "bytes past the stream's end were written"


def check_both_calls(units, pad=None, dialects=DIALECTS):
    """The slot call and the dense call against the model, every unit."""
    lay = Layout(units, pad)
    for d in dialects:
        status, pieces = lay.model(d)
        Slots(lay, d).check(status, pieces)
        Dense(lay, d, sum(len(p) for p in pieces) + 64 + 3, base=3).check(status, pieces)
    return lay


# ---------------------------------------------------------------------------
# 1. the fixtures the C++ encoder and pycapnp wrote
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("raw,packed", PAIRS)
def test_host_call_reproduces_the_fixtures(raw, packed):
    assert cp.pack_message(fixture(raw), "cxx") == fixture(packed)
    st, p = oracle.pack(fixture(raw))
    assert cp.pack_message(fixture(raw), "zig") == p == cp.pack_packed(fixture(raw))


def test_batch_and_dense_calls_reproduce_the_fixtures():
    raws = [fixture(r) for r, _ in PAIRS]
    want = [fixture(p) for _, p in PAIRS]
    lay = Layout(raws, words8(raws))
    ok = np.zeros(len(raws), dtype=np.int32)
    assert lay.model("cxx")[1] == want, "the model itself reproduces the fixtures"
    Slots(lay, "cxx").check(ok, want)
    Dense(lay, "cxx", sum(len(p) for p in want) + 64).check(ok, want)


def test_write_packed_messages_is_capnp_convert():
    raws = [fixture(r) for r, _ in PAIRS]
    stream = cp.write_packed_messages(raws, "cxx")
    assert stream == b"".join(fixture(p) for _, p in PAIRS)
    frames, used, name = cp.read_packed_messages(stream)
    assert frames == raws and used == len(stream) and name.upper() == "OK"
    assert cp.write_packed_messages(raws) == b"".join(zig_pack(r) for r in raws)
    assert cp.write_packed_messages([]) == b""
    with pytest.raises(cp.TruncatedMessage, match="frame 2"):
        cp.write_packed_messages([raws[0], raws[2], raws[2][:-8], raws[3][:-4]], "cxx")
    with pytest.raises(cp.InvalidArgument, match="frame 0"):
        cp.write_packed_messages([raws[2] + bytes(8)], "zig")


# ---------------------------------------------------------------------------
# 2. piece boundaries
# ---------------------------------------------------------------------------
def test_piece_boundaries():
    b = fs.boundary_units()
    units = [fs.frame(v) for v in b.values()]
    lay = check_both_calls(units, words8(units))
    # said outright for the first: the zero run restarts at the boundary
    _, pieces = lay.model("cxx")
    assert pieces[0].endswith(bytes((0, 1, 0, 1)))
    assert cp.pack_message(units[0], "cxx").endswith(bytes((0, 1, 0, 1)))
    assert cp.pack_packed(units[0], "cxx").endswith(bytes((0, 3)))


# ---------------------------------------------------------------------------
# 3. segment counts
# ---------------------------------------------------------------------------
def test_segment_counts():
    rng = np.random.default_rng(0xF4A30003)
    units = list(fs.count_units(rng).values())
    err = fs.error_units()
    units += [err["count_513"][0], err["count_ffffffff"][0]]
    lay = check_both_calls(units)
    st, _ = lay.model("cxx")
    assert list(st[-2:]) == [cp.SEGMENT_COUNT_LIMIT_EXCEEDED, cp.INVALID_SEGMENT_COUNT] and (st[:-2] == 0).all()


# ---------------------------------------------------------------------------
# 4. unit errors between neighbours that stay exact
# ---------------------------------------------------------------------------
def error_batch():
    rng = np.random.default_rng(0xF4A30004)
    good = lambda: fs.random_frame(rng, max_segs=5, max_words=700)  # noqa: E731
    units, pad, names = [], [], []
    for name, (u, _) in fs.error_units().items():
        units += [good(), u]
        names += ["ok", name]
    units += [good(), fs.frame([fs.rand_words(rng, 20, 0.5), fs.rand_words(rng, 3, 0.5)]), good(), good()]
    names += ["ok", "at_4_mod_8", "ok", "ok"]
    pos = 0
    for name, u in zip(names, units):  # every unit on a word boundary, but one at 4 mod 8
        p = (-pos) % 8 + (4 if name == "at_4_mod_8" else 0)
        pad.append(p)
        pos += p + len(u)
    return units, pad, names


def test_unit_errors_with_exact_neighbours():
    units, pad, names = error_batch()
    lay = check_both_calls(units, pad)
    want = {k: v for k, (_, v) in fs.error_units().items()}
    want["at_4_mod_8"] = cp.INVALID_ARGUMENT
    want["ok"] = cp.OK
    for d in DIALECTS:
        st, pieces = lay.model(d)
        assert [int(s) for s in st] == [want[k] for k in names]
        assert all((len(p) == 0) == (s != 0) for s, p in zip(st, pieces))
    assert int(lay.in_off[names.index("at_4_mod_8")]) % 8 == 4


def test_host_call_errors():
    for name, (u, want) in fs.error_units().items():
        for d in DIALECTS:
            with pytest.raises(cp._ERRORS[want]):
                cp.pack_message(u, d)


# ---------------------------------------------------------------------------
# 5. tile edges
# ---------------------------------------------------------------------------
def test_tile_edges():
    rng = np.random.default_rng(0xF4A30005)
    e = fs.tile_edge_units(rng)
    units = list(e.values())
    # 16-aligned units (first segments at 8 mod 16 when the table has an odd number of words),
    # then the same units at 8 mod 16
    pad16 = []
    pos = 0
    for u in units:
        p = (-pos) % 16
        pad16.append(p)
        pos += p + len(u)
    lay = check_both_calls(units, pad16)
    assert (lay.in_off % 16 == 0).all()
    lay = check_both_calls(units, [p + 8 for p in pad16[:1]] + pad16[1:])
    assert (lay.in_off % 16 == 8).all()


# ---------------------------------------------------------------------------
# 6. space
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    """About 600 units: 1 to 40 segments, up to 3 tiles, some failed ones among them."""
    rng = np.random.default_rng(0xF4A30006)
    units = [fs.random_frame(rng) for _ in range(560)]
    units += [fs.frame([fs.rand_words(rng, int(rng.integers(0, 1500)), 0.5)]) for _ in range(30)]
    err = list(fs.error_units().values())
    units += [err[i % len(err)][0] for i in range(10)]
    order = rng.permutation(len(units))
    units = [units[i] for i in order]
    lay = Layout(units, words8(units))
    return lay, {d: lay.model(d) for d in DIALECTS}


@pytest.mark.parametrize("dialect", DIALECTS)
def test_mixed_batch_against_the_model(mixed, dialect):
    lay, model = mixed
    status, pieces = model[dialect]
    assert (status != 0).sum() == 10
    ws = cp.framed_workspace(lay.n)
    Slots(lay, dialect, ws=ws).check(status, pieces)
    Dense(lay, dialect, sum(len(p) for p in pieces) + 64 + 5, base=5).check(status, pieces)


@pytest.mark.parametrize("dialect", DIALECTS)
def test_slot_one_byte_short(mixed, dialect):
    lay, model = mixed
    status, pieces = model[dialect]
    need = np.array([len(p) for p in pieces], dtype=np.int64)
    short = (np.arange(lay.n) % 3 == 0) & (need > 0)
    s = Slots(lay, dialect, caps=np.where(short, need - 1, need))
    want = np.where(short, cp.OUT_OF_SPACE, status).astype(np.int32)
    assert np.array_equal(s.h_st, want)
    assert np.array_equal(s.h_len, need), "OUT_OF_SPACE reports the required size"
    for i in range(lay.n):
        o, c = int(s.off[i]), int(s.caps[i])
        assert (s.h_out[o + c:o + c + 32] == CANARY).all(), f"unit {i}: bytes at or past its capacity"
        if not short[i]:
            assert s.h_out[o:o + c].tobytes() == pieces[i], i


@pytest.mark.parametrize("dialect", DIALECTS)
def test_dense_space_cut(mixed, dialect):
    lay, model = mixed
    status, pieces = model[dialect]
    lens = np.array([len(p) for p in pieces], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lens)))
    total = int(off[-1])
    k = int(np.flatnonzero((lens > 1) & (np.arange(lay.n) > lay.n // 2))[0])
    assert (lens[k + 1:] == 0).any(), "a failed unit after the cut"
    cap = int(off[k]) + int(lens[k]) // 2  # the middle of unit k
    r = Dense(lay, dialect, total + 64, cap=cap).fetch()
    assert np.array_equal(r.h_len, lens), "every unit keeps its true size"
    assert np.array_equal(r.h_off, off) and int(r.h_off[-1]) == total
    want = np.where((np.arange(lay.n) >= k) & (lens > 0), cp.OUT_OF_SPACE, status)
    assert np.array_equal(r.h_st, want)  # a failed unit after k keeps its own status
    assert r.h_out[:int(off[k])].tobytes() == b"".join(pieces[:k])
    assert (r.h_out[int(off[k]):] == CANARY).all()
    # the retry with the end the first call reported
    Dense(lay, dialect, total + 64, cap=int(r.h_off[-1])).check(status, pieces)


@pytest.mark.parametrize("dialect", DIALECTS)
def test_sizes_only(mixed, dialect):
    lay, model = mixed
    status, pieces = model[dialect]
    lens = np.array([len(p) for p in pieces], dtype=np.int64)
    s = Slots(lay, dialect, sizes_only=True)
    assert np.array_equal(s.h_st, status) and np.array_equal(s.h_len, lens)
    assert (s.h_out == CANARY).all()
    r = Dense(lay, dialect, 0, base=7, sizes_only=True).fetch()
    assert np.array_equal(r.h_st, status) and np.array_equal(r.h_len, lens)
    assert np.array_equal(r.h_off, 7 + np.concatenate(([0], np.cumsum(lens))))


# ---------------------------------------------------------------------------
# 7. the Zig dialect is the unframed calls' bytes
# ---------------------------------------------------------------------------
def test_zig_dialect_equals_the_unframed_calls(mixed):
    lay, model = mixed
    status, pieces = model["zig"]
    ok = np.flatnonzero(status == 0)
    sub = Layout([lay.units[i] for i in ok], words8([lay.units[i] for i in ok]))
    n = sub.n
    s = Slots(sub, "zig")
    out = torch.full_like(s.d_out, CANARY)
    ln = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.encode_batch(sub.d_in, sub.d_off, sub.d_len, out, i64(s.off), i64(s.caps), ln, st)
    torch.cuda.synchronize()
    assert (st == 0).all().item() and (s.h_st == 0).all()
    assert torch.equal(ln, s.len) and torch.equal(out, s.d_out)
    total = int(ln.sum().item())
    r = Dense(sub, "zig", total + 64, base=1).fetch()
    out2 = torch.full_like(r.d_out, CANARY)
    off2 = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
    cp.encode_dense_batch(sub.d_in, sub.d_off, sub.d_len, out2, off2, ln, st, base=1)
    torch.cuda.synchronize()
    assert (st == 0).all().item() and (r.h_st == 0).all()
    assert torch.equal(off2, r.off) and torch.equal(ln, r.len) and torch.equal(out2, r.d_out)


# ---------------------------------------------------------------------------
# 8. every OK unit's output is exactly one packed message
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dialect", DIALECTS)
def test_round_trip(mixed, dialect):
    lay, model = mixed
    status, pieces = model[dialect]
    n = lay.n
    total = sum(len(p) for p in pieces)
    r = Dense(lay, dialect, total + 64, base=5)
    d_msg = torch.zeros_like(lay.d_in)
    mlen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    used = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    mst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.read_message_batch(r.d_out, r.off[:-1], r.len, d_msg, lay.d_off, lay.d_len, mlen, used, mst)
    r.check(status, pieces)
    ok = torch.from_numpy(status == 0).to(DEV)
    assert ok.sum().item() == n - 10
    assert (mst[ok] == 0).all().item()
    assert torch.equal(used[ok], r.len[ok]), "every message pops with consumed == out_len"
    assert torch.equal(mlen[ok], lay.d_len[ok])
    h_msg = d_msg.cpu().numpy()
    for i in np.flatnonzero(status == 0):
        o = int(lay.in_off[i])
        assert h_msg[o:o + len(lay.units[i])].tobytes() == lay.units[i], i
    # the stream without its offsets: the splitter finds the same rows
    rows = n + 8
    first = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    tab = torch.full((3, rows), -1, dtype=torch.int64, device=DEV)
    consumed = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    sst = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    cp.split_streams(r.d_out, i64([5]), i64([total]), first, tab[0], tab[1], tab[2], consumed, sst)
    torch.cuda.synchronize()
    assert sst.item() == 0 and consumed.item() == total and first[1].item() == n - 10
    k = n - 10
    assert torch.equal(tab[0][:k], r.off[:-1][ok])
    assert torch.equal(tab[1][:k], r.len[ok])
    assert torch.equal(tab[2][:k], lay.d_len[ok])


# ---------------------------------------------------------------------------
# 9. capture
# ---------------------------------------------------------------------------
def capture_batch(seed, n=600):
    rng = np.random.default_rng(seed)
    units = []
    for i in range(n):  # the same lengths and tables for every seed: only the data changes
        shape = np.random.default_rng(0xF4A30090 + i)
        count = int(shape.integers(1, 6))
        sizes = shape.integers(0, 120, count)
        if i % 37 == 0:
            sizes[0] = int(shape.integers(513, 1200))
        units.append(fs.frame([fs.rand_words(rng, int(s), 0.3 if seed & 1 else 0.7) for s in sizes]))
    return units


def test_graph_capture_replay():
    units = capture_batch(0xF4A30091)
    lay = Layout(units)
    status, pieces = lay.model("cxx")
    ws = cp.dense_workspace(lay.n)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        # warm-up outside the capture; room for any data of these lengths (10 bytes a word)
        r = Dense(lay, "cxx", int(lay.in_len.sum()) * 5 // 4 + 4096, base=3, ws=ws, stream=s)
    s.synchronize()
    r.check(status, pieces)
    r.args["stream"] = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.call()
    for seed in (0xF4A30092, 0xF4A30093):  # new data in the same input buffers, then replay
        new = Layout(capture_batch(seed))
        assert np.array_equal(new.in_off, lay.in_off) and np.array_equal(new.in_len, lay.in_len)
        torch.zeros(1 << 20, device=DEV).sum().item()  # other work between the replays
        lay.d_in.copy_(new.d_in)
        lay.units = new.units
        r.d_out.fill_(CANARY)
        r.st.fill_(-1)
        g.replay()
        r.check(*new.model("cxx"))
