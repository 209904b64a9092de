"""The C++-dialect encoders on the device against tests/pyref_cxx.py and the
packed fixtures the C++ encoder and pycapnp wrote (tests/golden/fixtures)."""
import os

import numpy as np
import pytest
import torch

import capnp_packed as cp
import pyref_cxx as rx

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "fixtures")
PAIRS = [("binary", "packed"), ("segmented", "segmented-packed"),
         ("fixture_single.bin", "fixture_single_packed.bin"), ("fixture_far.bin", "fixture_far_packed.bin")]
DEV = "cuda"
CANARY = 0xA5


def fixture(name: str) -> bytes:
    with open(os.path.join(FIX, name), "rb") as f:
        return f.read()


def i64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)


def place(units, odd8=None):
    """The units end to end at 16-aligned offsets (odd8[i]: 8 past one, so 8- but not
    16-aligned) in one device buffer (torch allocations are 256-aligned)."""
    offs, pos = [], 0
    for i, u in enumerate(units):
        pos = (pos + 15) & ~15
        if odd8 is not None and odd8[i]:
            pos += 8
        offs.append(pos)
        pos += len(u)
    host = np.zeros(pos + 16, dtype=np.uint8)
    for o, u in zip(offs, units):
        host[o:o + len(u)] = np.frombuffer(u, dtype=np.uint8)
    return torch.from_numpy(host).to(DEV), np.array(offs, dtype=np.int64)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def direct_batch(d_in, off, ln, out, ooff, cap, olen, st, dialect):
    """capnp_packed_encode_batch_dialect itself (the Python wrappers route "zig" to the calls
    that existed before it)."""
    rc = cp.lib().capnp_packed_encode_batch_dialect(_p(d_in), _p(off), _p(ln), off.numel(), _p(out), _p(ooff),
                                                    _p(cap), _p(olen), _p(st), dialect, 0, 0, _stream())
    assert rc == cp.OK


def run_units(units, dialect="cxx", odd8=None, in_off=None, in_len=None, short=(), ws=None, default_call=False,
              direct=None):
    """Sizes-only call, lengths_to_offsets over (size + 1), then the write into exactly sized
    slots with one canary byte between them (unit i of `short`: a slot one byte short).
    Returns (sizes, size statuses, lengths, statuses, outputs, canaries intact)."""
    d_in, offs = place(units, odd8)
    n = len(units)
    off = i64(offs if in_off is None else in_off)
    ln = i64([len(u) for u in units] if in_len is None else in_len)
    kw = {} if default_call else {"dialect": dialect}
    sz = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    sst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    if direct is not None:
        direct_batch(d_in, off, ln, None, None, None, sz, sst, direct)
    else:
        cp.encoded_size_batch(d_in, off, ln, sz, sst, **kw)
    slots = cp.lengths_to_offsets(sz + 1)
    total = int(slots[-1].item())
    cap = sz.clone()
    for i in short:
        cap[i] -= 1
    out = torch.full((total + 16,), CANARY, dtype=torch.uint8, device=DEV)
    olen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    if direct is not None:
        direct_batch(d_in, off, ln, out, slots[:n].contiguous(), cap, olen, st, direct)
    else:
        cp.encode_batch(d_in, off, ln, out, slots[:n].contiguous(), cap, olen, st, ws=ws, **kw)
    torch.cuda.synchronize()
    h, so, hl, hc = out.cpu().numpy(), slots.cpu().numpy(), olen.cpu().numpy(), cap.cpu().numpy()
    outs = [h[so[i]:so[i] + hl[i]].tobytes() for i in range(n)]
    intact = all((h[so[i] + hc[i]:so[i + 1]] == CANARY).all() for i in range(n)) and (h[total:] == CANARY).all()
    return sz.cpu().numpy(), sst.cpu().numpy(), hl, st.cpu().numpy(), outs, intact, (out, slots, olen)


def check_units(units, **kw):
    sz, sst, ln, st, outs, intact, _ = run_units(units, **kw)
    exp = [rx.pack_buffer(u) for u in units]
    assert (sst == cp.OK).all() and (st == cp.OK).all()
    bad = [i for i in range(len(units)) if outs[i] != exp[i]]
    assert not bad, f"units {bad[:8]} differ from the reference rule"
    assert [int(x) for x in sz] == [len(e) for e in exp] and (sz == ln).all()
    assert intact


def run_messages(msgs, dialect="cxx", counts=None, direct=None):
    """Messages (lists of segments) through encode_message_batch: sizes only, then written."""
    segs = [s for m in msgs for s in m]
    d_seg, offs = place(segs if segs else [b""])
    seg_ptr = i64(offs[:len(segs)] + d_seg.data_ptr()) if segs else i64([0])
    seg_len = i64([len(s) for s in segs]) if segs else i64([0])
    cnt = [len(m) for m in msgs] if counts is None else counts
    first = torch.from_numpy(np.concatenate(([0], np.cumsum([len(m) for m in msgs])[:-1])).astype(np.int32)).to(DEV)
    count = torch.from_numpy(np.array(cnt, dtype=np.int32)).to(DEV)
    n = len(msgs)
    sz = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    sst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    def enc(d_out, ooff, cap, o_len, o_st):
        if direct is None:
            cp.encode_message_batch(seg_ptr, seg_len, first, count, d_out, ooff, cap, o_len, o_st, dialect=dialect)
        else:
            assert cp.lib().capnp_packed_encode_message_batch_dialect(
                _p(seg_ptr), _p(seg_len), _p(first), _p(count), n, _p(d_out), _p(ooff), _p(cap), _p(o_len),
                _p(o_st), direct, _stream()) == cp.OK

    enc(None, None, None, sz, sst)
    slots = cp.lengths_to_offsets(sz + 1)
    total = int(slots[-1].item())
    out = torch.full((total + 16,), CANARY, dtype=torch.uint8, device=DEV)
    olen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    enc(out, slots[:n].contiguous(), sz, olen, st)
    torch.cuda.synchronize()
    h, so, hl, hs = out.cpu().numpy(), slots.cpu().numpy(), olen.cpu().numpy(), sz.cpu().numpy()
    outs = [h[so[i]:so[i] + hl[i]].tobytes() for i in range(n)]
    intact = all((h[so[i] + hs[i]:so[i + 1]] == CANARY).all() for i in range(n)) and (h[total:] == CANARY).all()
    return hs, sst.cpu().numpy(), hl, st.cpu().numpy(), outs, intact, (out, slots, olen)


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------

def test_message_encoder_reproduces_the_fixtures():
    """Every unpacked fixture is parsed on the device (message_init_batch) and packed from its
    segments: the bytes are the committed C++ / pycapnp files."""
    raws = [fixture(r) for r, _ in PAIRS]
    d_in, offs = place(raws)
    n, ms = len(raws), 512
    off, ln = i64(offs), i64([len(r) for r in raws])
    cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
    so = torch.zeros(n * ms, dtype=torch.int64, device=DEV)
    sl = torch.zeros(n * ms, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.message_init_batch(d_in, off, ln, ms, cnt, so, sl, st)
    assert (st.cpu().numpy() == cp.OK).all()
    assert cnt.cpu().tolist() == [1, 125, 1, 4]
    seg_ptr = (so.view(n, ms) + off.view(n, 1) + d_in.data_ptr()).reshape(-1).contiguous()
    first = torch.arange(0, n * ms, ms, dtype=torch.int32, device=DEV)
    sz = torch.zeros(n, dtype=torch.int64, device=DEV)
    sst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.encode_message_batch(seg_ptr, sl, first, cnt, None, None, None, sz, sst, dialect="cxx")
    slots = cp.lengths_to_offsets(sz)
    out = torch.full((int(slots[-1].item()) + 16,), CANARY, dtype=torch.uint8, device=DEV)
    olen = torch.zeros(n, dtype=torch.int64, device=DEV)
    cp.encode_message_batch(seg_ptr, sl, first, cnt, out, slots[:n].contiguous(), sz, olen, st, dialect="cxx")
    torch.cuda.synchronize()
    assert (sst.cpu().numpy() == cp.OK).all() and (st.cpu().numpy() == cp.OK).all()
    h, s = out.cpu().numpy(), slots.cpu().numpy()
    for i, (_, packed) in enumerate(PAIRS):
        want = fixture(packed)
        assert int(sz[i]) == len(want) == int(olen[i])
        assert h[s[i]:s[i + 1]].tobytes() == want, PAIRS[i]
    assert (h[s[-1]:] == CANARY).all()


@pytest.mark.parametrize("raw,packed", PAIRS)
def test_raw_buffer_call_on_fixtures(raw, packed):
    data = fixture(raw)
    got = cp.pack_packed(data, dialect="cxx")
    if raw == "segmented":  # one piece: no restart at its segments
        assert got == rx.pack_buffer(data) and got != fixture(packed)
    else:
        assert got == fixture(packed)
    assert cp.unpack_packed(got) == data


def test_message_builder_reproduces_a_fixture():
    b = cp.MessageBuilder()
    for s in rx.split_framed(fixture("fixture_far.bin")):
        b.create_segment(s)
    assert b.to_packed_bytes(dialect="cxx") == fixture("fixture_far_packed.bin")
    assert cp.MessageBuilder().to_packed_bytes(dialect="cxx") == rx.pack_message([b""])


# ---------------------------------------------------------------------------
# known answers and run-state edges
# ---------------------------------------------------------------------------

KNOWN = [("B A B C", 33), ("A*257", 2060), ("A*256 B A", 2068), ("A*256 B B A B", 2084), ("A Z A", 22),
         ("Z*257", 4), ("", 0)]


def test_known_answers_single_buffer():
    for spec, size in KNOWN:
        data = rx.words(spec)
        got = cp.pack_packed(data, dialect="cxx")
        assert len(got) == size and got == rx.pack_buffer(data), spec
    assert cp.pack_packed(rx.words("B A B C")) != cp.pack_packed(rx.words("B A B C"), dialect="cxx")


def test_known_answers_batch():
    units = [rx.words(s) for s, _ in KNOWN]
    sz, _, ln, st, outs, intact, _ = run_units(units)
    assert [int(x) for x in ln] == [k for _, k in KNOWN] == [int(x) for x in sz]
    check_units(units)


def edge_specs():
    specs = ["A", "B", "C", "Z", "B A", "B B A B", "B*3 A B*3", "C B A", "Z B B A B Z B A"]
    for run in (255, 256, 257):
        for nxt in "ABCZ":
            specs.append(f"A*{run} {nxt}")
            specs.append(f"A B*{run - 1} {nxt}")
            specs.append(f"C A B A*{run - 3} {nxt} A B")
    specs += ["Z*256", "Z*257", "Z*256 A", "Z*257 B", "C Z*256 Z A"]
    for head in (7, 8, 63, 64, 255, 256, 257, 505, 511):
        for n in sorted({1, 2, 8, 9, 57, 256, 257, 300, 512 - head, 513 - head, 768 - head, 769 - head}):
            if n >= 1:
                specs.append(f"C*{head} A B*{n - 1} C A")
                specs.append(f"C*{head} A*{n} Z B")
                specs.append(f"B*{head} A*{n} B")
    return specs


def test_run_state_edges():
    check_units([rx.words(s) for s in edge_specs()])


def test_all_a_units_and_b_every_256th():
    units = []
    for n in (511, 512, 513, 1023, 1025, 4100):
        units.append(rx.words(f"A*{n}"))
        for phase in (0, 1, 255):
            units.append(rx.words(" ".join("B" if i % 256 == phase else "A" for i in range(n))))
    check_units(units)
    check_units(units, odd8=[True] * len(units))


def test_single_buffer_long_units():
    for spec in ("A*256 B A*300 B*300 A", "B*600 A B*700", "Z*700 A*513"):
        data = rx.words(spec)
        assert cp.pack_packed(data, dialect="cxx") == rx.pack_buffer(data), spec


# ---------------------------------------------------------------------------
# random mixed batch
# ---------------------------------------------------------------------------

SIZES = [0, 8, 64, 72, 512, 4096, 4104, 40960]
SIZE_P = np.array([1, 3, 3, 3, 4, 3, 2, 0.3])


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(20240611)
    units = []
    for i in range(2000):
        nb = int(rng.choice(SIZES, p=SIZE_P / SIZE_P.sum()))
        p = (0.02, 0.1, 0.5, 0.9, 0.0)[i % 5]
        a = rng.integers(1, 256, size=nb, dtype=np.uint8)
        a[rng.random(nb) < p] = 0
        units.append(a.tobytes())
    odd8 = [i % 2 == 1 for i in range(len(units))]
    return units, odd8, [rx.pack_buffer(u) for u in units]


def test_random_mixed_batch(mixed):
    units, odd8, exp = mixed
    assert {len(u) for u in units} == set(SIZES)
    sz, sst, ln, st, outs, intact, _ = run_units(units, odd8=odd8)
    assert (sst == cp.OK).all() and (st == cp.OK).all()
    bad = [i for i in range(len(units)) if outs[i] != exp[i]]
    assert not bad, f"units {bad[:8]} (bytes {[len(units[i]) for i in bad[:8]]}) differ from the reference rule"
    assert (sz == ln).all() and [int(x) for x in sz] == [len(e) for e in exp]
    assert intact


def test_workspace_call_matches(mixed):
    units, odd8, exp = mixed
    sub, sub8 = units[:300], odd8[:300]
    _, _, _, st, outs, intact, _ = run_units(sub, odd8=sub8, ws=cp.workspace(len(sub)))
    assert (st == cp.OK).all() and outs == exp[:300] and intact


def test_round_trip_through_the_default_decoder(mixed):
    units, odd8, exp = mixed
    _, _, _, _, _, _, (out, slots, olen) = run_units(units, odd8=odd8)
    n = len(units)
    ulen = [len(u) for u in units]
    uoff = np.concatenate(([0], np.cumsum(ulen)[:-1]))
    back = torch.full((sum(ulen) + 16,), CANARY, dtype=torch.uint8, device=DEV)
    blen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    bst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.decode_batch(out, slots[:n].contiguous(), olen, back, i64(uoff), i64(ulen), blen, bst)
    torch.cuda.synchronize()
    assert (bst.cpu().numpy() == cp.OK).all() and blen.cpu().tolist() == ulen
    assert back.cpu().numpy()[:sum(ulen)].tobytes() == b"".join(units)


def test_zig_dialect_is_the_existing_output(mixed):
    units, odd8, _ = mixed
    b = run_units(units, odd8=odd8, default_call=True)
    for a in (run_units(units, odd8=odd8, dialect="zig"), run_units(units, odd8=odd8, direct=cp.DIALECTS["zig"])):
        for x, y in zip(a[:4], b[:4]):
            assert (x == y).all()
        assert a[4] == b[4] and a[5] and b[5]
    data = b"".join(units[:40])
    want = cp.pack_packed(data)
    assert cp.pack_packed(data, dialect="zig") == want
    import ctypes
    out = ctypes.create_string_buffer(cp.encode_bound(len(data)))
    n = ctypes.c_size_t()
    assert cp.lib().capnp_packed_encode_dialect(data, len(data), out, len(out), ctypes.byref(n), 0) == cp.OK
    assert out.raw[:n.value] == want


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------

def test_errors_leave_their_neighbours_exact():
    good = [rx.words("B A B C"), rx.words("A*300 B A"), rx.words("Z*9 C A B")]
    units = [good[0], rx.words("A*40"), good[1], rx.words("A B C"), good[2], rx.words("A*16 B"), good[0]]
    d_in, offs = place(units)
    in_off, in_len = offs.copy(), np.array([len(u) for u in units], dtype=np.int64)
    in_len[3] -= 1   # len % 8 != 0
    in_off[5] += 4   # misaligned word side
    sz, sst, ln, st, outs, intact, _ = run_units(units, in_off=in_off, in_len=in_len, short=(1,))
    assert sst.tolist() == [cp.OK, cp.OK, cp.OK, cp.INVALID_MESSAGE_SIZE, cp.OK, cp.INVALID_ARGUMENT, cp.OK]
    assert st.tolist() == [cp.OK, cp.OUT_OF_SPACE, cp.OK, cp.INVALID_MESSAGE_SIZE, cp.OK, cp.INVALID_ARGUMENT, cp.OK]
    assert int(ln[1]) == len(rx.pack_buffer(units[1])) == int(sz[1])  # the required length
    assert int(ln[3]) == 0 and int(ln[5]) == 0
    for i in (0, 2, 4, 6):
        assert outs[i] == rx.pack_buffer(units[i])
    assert intact  # also the byte the short slot lacks


def test_out_of_space_on_a_long_unit():
    units = [rx.words("A*1030 B C"), rx.words("C*5")]
    sz, _, ln, st, outs, intact, _ = run_units(units, short=(0,))
    assert st.tolist() == [cp.OUT_OF_SPACE, cp.OK] and int(ln[0]) == len(rx.pack_buffer(units[0]))
    assert outs[1] == rx.pack_buffer(units[1]) and intact


# ---------------------------------------------------------------------------
# messages
# ---------------------------------------------------------------------------

def message_cases():
    a, b = rx.words, rx.words
    return [
        [b""],                                         # one empty segment
        [a("C A B C")],
        [a("C A"), a("A B")],                          # ends in A, starts with A: two records
        [a("C A"), b("B A")],                          # ends in A, starts with B
        [a("A*700 B"), b(""), a("B*3 A*300 Z*300")],   # multi-tile segments and an empty one
        [rx.word_a(k) if k % 3 else rx.word_b(k) for k in range(512)],
        [a("Z*3 A B")] * 64,
    ]


def test_messages():
    msgs = message_cases()
    sz, sst, ln, st, outs, intact, _ = run_messages(msgs)
    assert (sst == cp.OK).all() and (st == cp.OK).all() and (sz == ln).all() and intact
    for i, m in enumerate(msgs):
        assert outs[i] == rx.pack_message(m), f"message {i}"
    # the run does not cross the pieces
    assert outs[2] == rx.pack_piece(rx.segment_table(msgs[2])) + rx.pack_piece(msgs[2][0]) + rx.pack_piece(msgs[2][1])
    assert outs[2] != rx.pack_buffer(cp.frame_segments(msgs[2]))
    assert outs[3] != rx.pack_buffer(cp.frame_segments(msgs[3]))


def test_zero_segments_is_one_empty_segment():
    _, sst, _, st, outs, intact, _ = run_messages([[rx.words("A")], [rx.words("B")]], counts=[0, 1])
    assert st.tolist() == [cp.OK, cp.OK] and sst.tolist() == [cp.OK, cp.OK] and intact
    assert outs[0] == rx.pack_message([b""]) == cp.pack_packed(cp.frame_segments([b""]))
    assert outs[1] == rx.pack_message([rx.words("B")])


def test_too_many_segments_and_bad_segments():
    seg = rx.words("A")
    msgs = [[seg] * 513, [seg] * 512, [seg + b"\x01\x02\x03\x04"], [seg]]
    sz, sst, ln, st, outs, intact, _ = run_messages(msgs)
    assert st.tolist() == [cp.INVALID_ARGUMENT, cp.OK, cp.INVALID_ARGUMENT, cp.OK] == sst.tolist()
    assert int(ln[0]) == 0 and int(ln[2]) == 0 and intact
    assert outs[1] == rx.pack_message(msgs[1]) and outs[3] == rx.pack_message(msgs[3])


def test_message_out_of_space():
    msgs = [[rx.words("A*600")], [rx.words("C")]]
    segs = [s for m in msgs for s in m]
    d_seg, offs = place(segs)
    seg_ptr, seg_len = i64(offs + d_seg.data_ptr()), i64([len(s) for s in segs])
    first = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    count = torch.tensor([1, 1], dtype=torch.int32, device=DEV)
    want = [rx.pack_message(m) for m in msgs]
    cap = i64([len(want[0]) - 1, len(want[1])])
    off = i64([0, len(want[0])])
    out = torch.full((len(want[0]) + len(want[1]) + 16,), CANARY, dtype=torch.uint8, device=DEV)
    olen = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    st = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    cp.encode_message_batch(seg_ptr, seg_len, first, count, out, off, cap, olen, st, dialect="cxx")
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [cp.OUT_OF_SPACE, cp.OK] and olen.cpu().tolist() == [len(w) for w in want]
    h = out.cpu().numpy()
    assert h[len(want[0]) - 1] == CANARY and h[len(want[0]):len(want[0]) + len(want[1])].tobytes() == want[1]
    assert (h[len(want[0]) + len(want[1]):] == CANARY).all()


def test_read_message_batch_reads_the_message_outputs():
    msgs = message_cases()
    _, _, ln, _, outs, _, (out, slots, olen) = run_messages(msgs)
    n = len(msgs)
    framed = [cp.frame_segments(m) for m in msgs]
    flen = [len(f) for f in framed]
    foff = np.concatenate(([0], np.cumsum(flen)[:-1]))
    back = torch.full((sum(flen) + 16,), CANARY, dtype=torch.uint8, device=DEV)
    blen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    used = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    bst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.read_message_batch(out, slots[:n].contiguous(), olen, back, i64(foff), i64(flen), blen, used, bst)
    torch.cuda.synchronize()
    assert (bst.cpu().numpy() == cp.OK).all()
    assert blen.cpu().tolist() == flen and used.cpu().tolist() == [int(x) for x in ln]
    assert back.cpu().numpy()[:sum(flen)].tobytes() == b"".join(framed)


def test_zig_dialect_messages_are_the_existing_output():
    msgs = message_cases()
    for a in (run_messages(msgs, dialect="zig"), run_messages(msgs, direct=cp.DIALECTS["zig"])):
        assert (a[3] == cp.OK).all() and a[5]
        for i, m in enumerate(msgs):
            assert a[4][i] == cp.pack_packed(cp.frame_segments(m)), f"message {i}"
