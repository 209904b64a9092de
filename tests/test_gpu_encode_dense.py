"""capnp_packed_encode_dense_batch: the batch packed into ONE dense stream in unit order, in one
pass (MessageBuilder.writePackedTo unit after unit on one writer, message.zig:2209-2213;
DESIGN.md §2.10).

Every test fills d_out with a canary first and asserts that no unit came back DEVICE_ERROR (the
kernel's bounded look-back gave up). The expected stream is the concatenation of the oracle's
packPacked of every unit (oracle.pack / oracle.pack_batch; "cxx": pyref_cxx.pack_buffer).
"""
import numpy as np
import pytest

import capnp_packed as cp
import msggen
import oracle
import pyref_cxx

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = 0xA5


def rand_unit(rng, nbytes, p):
    """nbytes random bytes, each zero with probability p."""
    a = rng.integers(1, 256, nbytes, dtype=np.uint8)
    a[rng.random(nbytes) < p] = 0
    return a


class Layout:
    """Units laid out in one input buffer; pad[i] extra bytes go in front of unit i."""

    def __init__(self, units, pad=None):
        self.units = [np.ascontiguousarray(u, dtype=np.uint8) for u in units]
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
            self.h_in[self.in_off[i]:self.in_off[i] + len(u)] = u
        self.n = n
        self.d_in = torch.from_numpy(self.h_in).to(DEV)
        self.d_off = torch.from_numpy(self.in_off).to(DEV)
        self.d_len = torch.from_numpy(self.in_len).to(DEV)


def oracle_pieces(units, dialect="zig", skip=()):
    """Packed bytes per unit (b"" for the units in skip: the ones with an input error)."""
    n = len(units)
    if dialect == "cxx":
        return [b"" if i in skip else pyref_cxx.pack_buffer(units[i].tobytes()) for i in range(n)]
    lens = np.array([0 if i in skip else len(u) for i, u in enumerate(units)], dtype=np.uint64)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    in_off[1:] = np.cumsum(lens)
    inp = np.zeros(int(in_off[-1]) + 16, dtype=np.uint8)
    for i, u in enumerate(units):
        if i not in skip:
            inp[int(in_off[i]):int(in_off[i + 1])] = u
    slots = lens // 8 * 10 + 16
    out_off = np.zeros(n + 1, dtype=np.uint64)
    out_off[1:] = np.cumsum(slots)
    out, out_len, status = oracle.pack_batch(inp, in_off, out_off)
    assert (status == oracle.OK).all()
    return [out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]


class Run:
    """One encode_dense_batch call on a canary-filled output."""

    def __init__(self, lay, out_bytes, base=0, cap=None, dialect="zig", ws=None, stream=None, sizes_only=False):
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
        cp.encode_dense_batch(lay.d_in, lay.d_off, lay.d_len, self.d_out, self.off, self.len, self.st, **self.args)

    def fetch(self):
        torch.cuda.synchronize()
        self.h_off = self.off.cpu().numpy()
        self.h_len = self.len.cpu().numpy()
        self.h_st = self.st.cpu().numpy()
        assert not (self.h_st == cp.DEVICE_ERROR).any(), "a look-back gave up"
        self.h_out = None if self.d_out is None else self.d_out.cpu().numpy()
        return self

    def check_stream(self, pieces, status=None):
        """Offsets are the running sum, every unit's bytes are its piece, everything outside
        [base, off[n]) is still the canary."""
        self.fetch()
        lens = np.array([len(p) for p in pieces], dtype=np.int64)
        exp_off = self.base + np.concatenate(([0], np.cumsum(lens)))
        assert np.array_equal(self.h_len, lens)
        assert np.array_equal(self.h_off, exp_off)
        want = np.zeros(len(pieces), dtype=np.int32) if status is None else status
        assert np.array_equal(self.h_st, want)
        end = int(exp_off[-1])
        stream = np.frombuffer(b"".join(pieces), dtype=np.uint8)
        got = self.h_out[self.base:end]
        if not np.array_equal(got, stream):
            bad = int(np.flatnonzero(got != stream)[0])
            unit = int(np.searchsorted(exp_off, self.base + bad, side="right")) - 1
            raise AssertionError(f"stream differs at byte {bad} (unit {unit}, {len(self.lay.units[unit])} B in)")
        assert (self.h_out[:self.base] == CANARY).all(), "bytes below out_base were written"
        assert (self.h_out[end:] == CANARY).all(), "bytes past the stream's end were written"


# ---------------------------------------------------------------------------
# 1. mixed lengths against the oracle
# ---------------------------------------------------------------------------
MIX_LENGTHS = (0, 8, 64, 504, 4088, 4096, 4104, 8192, 12296, 69632)


def mixed_units(seed=0xD5E0001):
    rng = np.random.default_rng(seed)
    units = []
    for nbytes in MIX_LENGTHS:
        for p in (0.1, 0.5, 0.9):
            for _ in range(8):
                units.append(rand_unit(rng, nbytes, p))
        for _ in range(3):
            units.append(np.zeros(nbytes, dtype=np.uint8))
            units.append(rng.integers(1, 256, nbytes, dtype=np.uint8))
    order = rng.permutation(len(units))
    units = [units[i] for i in order]
    pad = [8 if rng.random() < 0.4 else 0 for _ in units]  # inputs at 8-but-not-16-aligned addresses
    return units, pad


@pytest.fixture(scope="module")
def mixed():
    units, pad = mixed_units()
    assert len(units) == 300
    lay = Layout(units, pad)
    assert (lay.in_off % 16 == 8).any() and (lay.in_off % 16 == 0).any()
    return lay, {"zig": oracle_pieces(units), "cxx": oracle_pieces(units, "cxx")}


@pytest.mark.parametrize("dialect", ["zig", "cxx"])
def test_mixed_lengths_against_the_oracle(mixed, dialect):
    lay, pieces = mixed
    total = sum(len(p) for p in pieces[dialect])
    Run(lay, 3 + total + 4096, base=3, dialect=dialect).check_stream(pieces[dialect])


# ---------------------------------------------------------------------------
# 2. more tiles than can be resident
# ---------------------------------------------------------------------------
def test_more_tiles_than_resident():
    n = 1 << 18
    rng = np.random.default_rng(0xD5E0002)
    lens = (rng.integers(1, 65, n) * 8).astype(np.uint64)  # 8 .. 512 B
    in_off = np.zeros(n + 1, dtype=np.uint64)
    in_off[1:] = np.cumsum(lens)
    U = int(in_off[-1])
    d_in = cp.generate(1, U, seed=0xD5E00022, zero_thresh=128, device=DEV)
    h_in = d_in.cpu().numpy()
    slots = lens // 8 * 10 + 16
    slot_off = np.zeros(n + 1, dtype=np.uint64)
    slot_off[1:] = np.cumsum(slots)
    o_out, o_len, o_st = oracle.pack_batch(h_in, in_off, slot_off)  # OpenMP
    assert (o_st == oracle.OK).all()
    exp_off = np.concatenate(([0], np.cumsum(o_len))).astype(np.int64)
    total = int(exp_off[-1])
    dense = np.empty(total, dtype=np.uint8)
    so, ln = slot_off.astype(np.int64), o_len.astype(np.int64)
    for i in range(n):  # the oracle's slots laid out densely
        dense[exp_off[i]:exp_off[i + 1]] = o_out[so[i]:so[i] + ln[i]]

    d_off = torch.from_numpy(in_off[:-1].astype(np.int64)).to(DEV)
    d_len = torch.from_numpy(lens.astype(np.int64)).to(DEV)
    d_out = torch.full((total + 256,), CANARY, dtype=torch.uint8, device=DEV)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
    plen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.encode_dense_batch(d_in, d_off, d_len, d_out, off, plen, st)
    # the three-call path on the device
    len3 = torch.zeros(n, dtype=torch.int64, device=DEV)
    st3 = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.encoded_size_batch(d_in, d_off, d_len, len3, st3)
    off3 = cp.lengths_to_offsets(len3)
    out3 = torch.full((total + 256,), CANARY, dtype=torch.uint8, device=DEV)
    cp.encode_batch(d_in, d_off, d_len, out3, off3[:-1].contiguous(), len3, len3.clone(), st3)
    torch.cuda.synchronize()
    assert not (st == cp.DEVICE_ERROR).any().item()
    assert (st == 0).all().item() and (st3 == 0).all().item()
    assert np.array_equal(off.cpu().numpy(), exp_off)
    assert np.array_equal(plen.cpu().numpy(), ln)
    assert torch.equal(off, off3)
    assert torch.equal(d_out, out3)
    h_out = d_out.cpu().numpy()
    assert np.array_equal(h_out[:total], dense)
    assert (h_out[total:] == CANARY).all()


# ---------------------------------------------------------------------------
# 3. uneven load
# ---------------------------------------------------------------------------
def test_uneven_load():
    rng = np.random.default_rng(0xD5E0003)
    big = 256 * 1024
    units = [rand_unit(rng, big, 0.5)]
    small = [rand_unit(rng, 64, 0.5) for _ in range(8192)]
    units += small[:4096] + [rand_unit(rng, big, 0.5)] + small[4096:]
    units += [rand_unit(rng, 4096, 0.5) for _ in range(4096)]
    lay = Layout(units)
    assert (lay.in_off[-4096:] % 16 == 0).all()
    pieces = oracle_pieces(units)
    ws = cp.dense_workspace(lay.n)
    r = Run(lay, sum(len(p) for p in pieces) + 512, ws=ws)
    r.check_stream(pieces)
    # workspace word 2: the longest look-back that had to wait, in ticks of the 100 MHz clock
    print(f"uneven load: longest look-back wait {int(ws[2].item()) / 100.0:.1f} us, give-up word {int(ws[1].item())}")
    assert int(ws[1].item()) == 0


# ---------------------------------------------------------------------------
# 4. errors inside the stream
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def thousand():
    rng = np.random.default_rng(0xD5E0004)
    lens = rng.integers(0, 76, 1000) * 8
    lens[::50] = 0  # empty units too
    units = [rand_unit(rng, int(x), 0.5) for x in lens]
    return units, oracle_pieces(units)


def test_errors_inside_the_stream():
    rng = np.random.default_rng(0xD5E0041)
    lens = rng.integers(1, 76, 1000) * 8
    units = [rand_unit(rng, int(x), 0.5) for x in lens]
    units[500] = rand_unit(rng, 44, 0.5)  # len % 8 == 4
    pad = [0] * 1000
    pad[400] = 4   # unit 400 starts at an address that is not 8-aligned ...
    pad[401] = 4   # ... and the ones after it are aligned again
    pad[501] = 4   # after the 44-byte unit
    lay = Layout(units, pad)
    assert lay.in_off[400] % 8 == 4 and lay.in_off[401] % 8 == 0 and lay.in_off[501] % 8 == 0
    pieces = oracle_pieces(units, skip=(400, 500))
    want = np.zeros(1000, dtype=np.int32)
    want[400] = cp.INVALID_ARGUMENT
    want[500] = cp.INVALID_MESSAGE_SIZE
    r = Run(lay, sum(len(p) for p in pieces) + 256, base=1)
    r.check_stream(pieces, status=want)
    assert r.h_len[400] == 0 and r.h_len[500] == 0


# ---------------------------------------------------------------------------
# 5. the space cut
# ---------------------------------------------------------------------------
def test_space_cut(thousand):
    units, pieces = thousand
    lay = Layout(units)
    lens = np.array([len(p) for p in pieces], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lens)))
    total = int(off[-1])
    k = 601
    assert lens[k] > 1 and (lens[k + 1:] == 0).any()
    cap = int(off[k]) + int(lens[k]) // 2  # the middle of unit k
    r = Run(lay, total + 64, cap=cap).fetch()
    assert np.array_equal(r.h_len, lens), "every unit keeps its true size"
    assert np.array_equal(r.h_off, off) and int(r.h_off[-1]) == total
    want = np.where((np.arange(1000) >= k) & (lens > 0), cp.OUT_OF_SPACE, cp.OK)
    assert np.array_equal(r.h_st, want)  # an empty unit after k is OK
    assert r.h_out[:int(off[k])].tobytes() == b"".join(pieces[:k])
    assert (r.h_out[int(off[k]):] == CANARY).all()
    # the retry with the end the first call reported
    Run(lay, total + 64, cap=int(r.h_off[-1])).check_stream(pieces)
    # one byte short of the last unit's end fails only that unit
    last = int(np.flatnonzero(lens > 0)[-1])
    r = Run(lay, total + 64, cap=total - 1).fetch()
    want = np.zeros(1000, dtype=np.int32)
    want[last] = cp.OUT_OF_SPACE
    assert np.array_equal(r.h_st, want) and np.array_equal(r.h_len, lens)
    assert r.h_out[:int(off[last])].tobytes() == b"".join(pieces[:last])
    assert (r.h_out[int(off[last]):] == CANARY).all()


# ---------------------------------------------------------------------------
# 6. sizes only
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dialect", ["zig", "cxx"])
def test_sizes_only(mixed, dialect):
    lay, _ = mixed
    r = Run(lay, 0, base=7, dialect=dialect, sizes_only=True).fetch()
    len3 = torch.zeros(lay.n, dtype=torch.int64, device=DEV)
    st3 = torch.full((lay.n,), -1, dtype=torch.int32, device=DEV)
    cp.encoded_size_batch(lay.d_in, lay.d_off, lay.d_len, len3, st3, dialect=dialect)
    off3 = cp.lengths_to_offsets(len3, base=7)
    torch.cuda.synchronize()
    assert (r.h_st == 0).all() and (st3 == 0).all().item()
    assert torch.equal(r.len, len3)
    assert torch.equal(r.off, off3)


# ---------------------------------------------------------------------------
# 7. round trip
# ---------------------------------------------------------------------------
def test_round_trip_decode(mixed):
    lay, pieces = mixed
    n = lay.n
    r = Run(lay, sum(len(p) for p in pieces["zig"]) + 64)
    d_dec = torch.zeros_like(lay.d_in)
    ulen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    ust = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.decode_batch(r.d_out, r.off[:-1], r.len, d_dec, lay.d_off, lay.d_len, ulen, ust)
    r.fetch()
    assert (ust == 0).all().item() and torch.equal(ulen, lay.d_len)
    assert torch.equal(d_dec, lay.d_in)


def test_round_trip_read_message():
    rng = np.random.default_rng(0xD5E0007)
    msgs = [np.frombuffer(msggen.random_message(rng), dtype=np.uint8) for _ in range(200)]
    lay = Layout(msgs)
    pieces = oracle_pieces(msgs)
    n = lay.n
    r = Run(lay, sum(len(p) for p in pieces) + 64, base=5)
    d_msg = torch.zeros_like(lay.d_in)
    mlen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    used = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    mst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.read_message_batch(r.d_out, r.off[:-1], r.len, d_msg, lay.d_off, lay.d_len, mlen, used, mst)
    r.check_stream(pieces)
    assert (mst == 0).all().item()
    assert torch.equal(used, r.len), "every message pops with consumed == out_len"
    assert torch.equal(mlen, lay.d_len)
    assert torch.equal(d_msg, lay.d_in)


# ---------------------------------------------------------------------------
# 8. state is per call
# ---------------------------------------------------------------------------
def small_batch(seed, n):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 200, n) * 8
    lens[::37] = rng.integers(513, 1500, len(lens[::37])) * 8  # some units of more than one tile
    units = [rand_unit(rng, int(x), 0.5) for x in lens]
    return Layout(units), oracle_pieces(units)


def test_back_to_back_on_one_workspace():
    a, pa = small_batch(0xD5E0081, 3000)
    b, pb = small_batch(0xD5E0082, 3000)
    ws = cp.dense_workspace(3000)
    ra = Run(a, sum(len(p) for p in pa) + 64, ws=ws)   # no synchronisation in between
    rb = Run(b, sum(len(p) for p in pb) + 64, base=2, ws=ws)
    ra.check_stream(pa)
    rb.check_stream(pb)
    c, pc = small_batch(0xD5E0083, 777)
    ws2 = cp.dense_workspace(777)
    rc = Run(c, sum(len(p) for p in pc) + 64, ws=ws2)
    rd = Run(a, sum(len(p) for p in pa) + 64, ws=ws)
    rc.check_stream(pc)
    rd.check_stream(pa)


def test_graph_capture_replay():
    lay, pieces = small_batch(0xD5E0084, 2000)
    ws = cp.dense_workspace(lay.n)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        # warm-up outside the capture; room for any data of these lengths (10 bytes a word)
        r = Run(lay, int(lay.in_len.sum()) * 5 // 4 + 4096, base=3, ws=ws, stream=s)
    s.synchronize()
    r.check_stream(pieces)
    r.args["stream"] = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.call()
    for seed in (0xD5E0085, 0xD5E0086):  # new data in the same input buffers, then replay
        rng = np.random.default_rng(seed)
        units = [rand_unit(rng, len(u), 0.3 if seed & 1 else 0.7) for u in lay.units]
        new = Layout(units)
        assert np.array_equal(new.in_off, lay.in_off)
        lay.d_in.copy_(new.d_in)
        lay.units = new.units
        r.d_out.fill_(CANARY)
        r.st.fill_(-1)
        g.replay()
        r.check_stream(oracle_pieces(units))


# ---------------------------------------------------------------------------
# 9. offsets past 2^31 and 2^32
# ---------------------------------------------------------------------------
def test_stream_longer_than_4_gib():
    # every unit reads the same 4 KiB of input, so the stream is one piece repeated: offsets
    # and written bytes are checked on the device across the 2^31 and 2^32 byte marks
    rng = np.random.default_rng(0xD5E0009)
    unit = rand_unit(rng, 4096, 0.3)
    piece = oracle_pieces([unit])[0]
    P = len(piece)
    n = (1 << 32) // P + 4099
    d_in = torch.from_numpy(unit).to(DEV)
    in_off = torch.zeros(n, dtype=torch.int64, device=DEV)
    in_len = torch.full((n,), 4096, dtype=torch.int64, device=DEV)
    base = 5
    total = n * P
    assert total > (1 << 32)
    d_out = torch.full((base + total + 64,), CANARY, dtype=torch.uint8, device=DEV)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
    plen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.encode_dense_batch(d_in, in_off, in_len, d_out, off, plen, st, base=base)
    torch.cuda.synchronize()
    assert not (st == cp.DEVICE_ERROR).any().item()
    assert (st == 0).all().item() and (plen == P).all().item()
    assert torch.equal(off, base + P * torch.arange(n + 1, dtype=torch.int64, device=DEV))
    ref = torch.from_numpy(np.frombuffer(piece, dtype=np.uint8).copy()).to(DEV)
    rows = d_out[base:base + total].view(n, P)
    step = 1 << 16  # compare in slabs: no 4 GiB temporary
    for i in range(0, n, step):
        assert (rows[i:i + step] == ref).all().item(), f"units {i}..{i + step}"
    assert (d_out[:base] == CANARY).all().item() and (d_out[base + total:] == CANARY).all().item()
