"""The fused message encoders (capnp_packed_encode_message_batch / _dialect:
encode_message_kernel<WRITE, TILED> under the default dialect, encode_message_cxx_kernel under the
C++ one) and message_init_kernel on adversarial and segment-edge input, message by message and byte
for byte against the references: oracle.pack(pyref.frame(segs)) (message.zig:2123-2179) and
pyref_cxx.pack_message. The inputs are tests/message_streams.py's, judged on the CPU by
tests/test_message_streams.py:
- the count lattice: 0 .. 66, 127 .. 129, 255 .. 257, 511 and 512 segments of 0 .. 3 words, end to
  end at both base phases and gathered;
- empty segments first, last, in a row, all and all but one, in the gathered and the tiled route;
- hw + payload of 510 .. 514 words, a segment of 512 and of 513 words, segment edges around the
  tile ends of 1024- and 1536-word messages;
- Z and A runs of 255 .. 257 words across header -> segment 0, segment -> segment, a tile end with
  a segment edge or an empty segment in the look-ahead, and a message end inside it;
- one-word segments and alternating 1- and 2-word ones in every placement (shuffled, reversed,
  adjacent but listed in reverse, only the last link broken, the same bytes listed twice and
  shared by two messages);
- every ordered pair of routes for the two messages of a first-pass wave, at n of 1, 2, 3 and
  around 8 and 16;
- capacity walks around the need, the tile ends and the C++ dialect's piece ends;
- misaligned lengths and addresses on segment 0, 63, 64 and 299, and 513 segments, between valid
  neighbours;
- a random mix of the stress test's shapes.
Every slot lies between 64 sentinel bytes at a chosen `address & 15`; every empty segment's
address and every seg_first of a message without segments points at poison. Each test makes the
batch call and the sizes-only call and holds both to message_streams.check."""
import numpy as np
import pytest

import capnp_packed as cp
import message_streams as ms
import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
NEED_FULL = 0x7FFF0001  # what the first pass writes into `status` for the tiled pass


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def call(entry, *args):
    """The three entry points of the default dialect, and the C++ dialect's."""
    if entry == "default":
        cp.encode_message_batch(*args)
    elif entry in ("zig", "cxx"):
        cp.encode_message_batch(*args, dialect=entry)
    else:
        assert entry == "dialect_zig"
        seg_ptr, seg_len, first, count, d_out, out_off, out_cap, out_len, status = args
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        rc = cp.lib().capnp_packed_encode_message_batch_dialect(
            p(seg_ptr), p(seg_len), p(first), p(count), first.numel(), p(d_out), p(out_off), p(out_cap), p(out_len),
            p(status), 0, torch.cuda.current_stream().cuda_stream)
        assert rc == cp.OK


def run(b, dialect, prefill=-1, entry=None):
    """The batch call into a buffer of SENT and the sizes-only call, `status` and `out_len` of both
    holding `prefill` before. Returns the host results and the device tensors."""
    n = len(b.msgs)
    sl = b.slots[dialect]
    pool = torch.from_numpy(b.pool).to(DEV)
    base = pool.data_ptr()
    assert base % 256 == 0
    seg_ptr, seg_len = i64(b.seg_off + base), i64(b.seg_len)
    first, count = i32(b.first), i32(b.count)
    d_out = torch.full((ms.output_bytes(b, dialect),), ms.SENT, dtype=torch.uint8, device=DEV)
    out_len = torch.full((n,), prefill, dtype=torch.int64, device=DEV)
    status = torch.full((n,), prefill, dtype=torch.int32, device=DEV)
    sz_len, sz_st = out_len.clone(), status.clone()
    entry = entry or dialect
    call(entry, seg_ptr, seg_len, first, count, d_out, i64(sl.out_off), i64(sl.caps), out_len, status)
    call(entry, seg_ptr, seg_len, first, count, None, None, None, sz_len, sz_st)
    torch.cuda.synchronize()
    host = (d_out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy(), sz_len.cpu().numpy(),
            sz_st.cpu().numpy())
    return host, (d_out, out_len, pool)


def encode_and_check(b, dialect, prefill=-1, entry=None):
    host, dev = run(b, dialect, prefill, entry)
    out, ol, st, sz_len, sz_st = host
    seen = ms.check(b, out, ol, st, dialect)
    ms.check(b, None, sz_len, sz_st, dialect)
    return seen, host, dev


PREFILLS = [-1, 0, NEED_FULL]


@pytest.mark.parametrize("prefill", PREFILLS, ids=["-1", "0", "need_full"])
@pytest.mark.parametrize("dialect", ms.DIALECTS)
@pytest.mark.parametrize("name", list(ms.BUILDERS))
def test_builder(name, dialect, prefill):
    """One batch call and one sizes-only call per builder and dialect, `status` and `out_len` full
    of -1, of 0 and of the first pass's mark for the tiled pass before the call: no result depends
    on what the arrays held (the tiled pass takes exactly the messages this call's first pass
    marked)."""
    b = ms.BUILDERS[name]()
    seen, _, _ = encode_and_check(b, dialect, prefill)
    assert seen == ms.statuses(b, dialect) == ms.STATUSES[name]


@pytest.mark.parametrize("prefill", PREFILLS, ids=["-1", "0", "need_full"])
@pytest.mark.parametrize("dialect", ms.DIALECTS)
def test_wave_pairs(dialect, prefill):
    """m0 and m1 of a first-pass wave on every ordered pair of routes, and batches of odd and even
    n around a wave, a block and two blocks."""
    seen = set()
    for b in ms.wave_pairs():
        seen |= encode_and_check(b, dialect, prefill)[0]
    assert seen == ms.STATUSES["wave_pairs"]


def test_default_dialect_entry_points_agree():
    """capnp_packed_encode_message_batch, the wrapper's dialect="zig" and
    capnp_packed_encode_message_batch_dialect(..., ZIG): identical arrays and bytes on the random
    mix, each also held to the oracle."""
    b = ms.random_mixed()
    got = [encode_and_check(b, "zig", entry=e)[1] for e in ("default", "zig", "dialect_zig")]
    care = np.ones(got[0][0].size, dtype=bool)  # a slot that ended OUT_OF_SPACE is unspecified
    sl = b.slots["zig"]
    for i in np.flatnonzero(got[0][2] == cp.OUT_OF_SPACE):
        care[int(sl.out_off[i]):int(sl.out_off[i]) + sl.caps[i]] = False
    for other in got[1:]:
        assert np.array_equal(got[0][0][care], other[0][care])
        for a, c in zip(got[0][1:], other[1:]):
            assert np.array_equal(a, c)


@pytest.mark.parametrize("dialect", ms.DIALECTS)
@pytest.mark.parametrize("name", ["count_lattice", "tile_limit"])
def test_round_trip_from_the_slots(name, dialect):
    """The OK messages, still in their slots, read back by read_message_batch: the frames
    (pyref.frame of the segments) with consumed == out_len; message_init_batch over those frames
    returns the segment tables the messages were built from."""
    b = ms.BUILDERS[name]()
    seen, (_, ol, st, _, _), (d_out, _, _) = encode_and_check(b, dialect)
    assert seen == {cp.OK}
    n = len(b.msgs)
    frames = [ms.frame_of(m) for m in b.msgs]
    lens = np.array([len(f) for f in frames], dtype=np.int64)
    f_off = np.concatenate(([0], np.cumsum(lens + 64)[:-1])) + 64
    d_fr = torch.full((int(f_off[-1] + lens[-1]) + 64,), ms.SENT, dtype=torch.uint8, device=DEV)
    flen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    used = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    fst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    t_off = i64(f_off)
    cp.read_message_batch(d_out, i64(b.slots[dialect].out_off), i64(ol), d_fr, t_off, i64(lens), flen, used, fst)
    ms_ = ms.MAX_SEGS
    cnt = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    so = torch.full((n * ms_,), -1, dtype=torch.int64, device=DEV)
    sg = torch.full((n * ms_,), -1, dtype=torch.int64, device=DEV)
    ist = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.message_init_batch(d_fr, t_off, flen, ms_, cnt, so, sg, ist)
    torch.cuda.synchronize()
    assert (fst.cpu().numpy() == cp.OK).all() and (ist.cpu().numpy() == cp.OK).all()
    assert np.array_equal(flen.cpu().numpy(), lens) and np.array_equal(used.cpu().numpy(), ol)
    image = np.full(d_fr.numel(), ms.SENT, dtype=np.uint8)
    for o, f in zip(f_off, frames):
        image[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    assert np.array_equal(d_fr.cpu().numpy(), image)
    cnt, so, sg = cnt.cpu().numpy(), so.cpu().numpy().reshape(n, ms_), sg.cpu().numpy().reshape(n, ms_)
    for i in range(n):
        tab = ms.segment_table_of(b, i)
        assert cnt[i] == len(tab), i
        assert list(zip(so[i, :len(tab)].tolist(), sg[i, :len(tab)].tolist())) == tab, ms.describe(b, i, dialect)
        assert (so[i, len(tab):] == -1).all() and (sg[i, len(tab):] == -1).all(), i


INIT_SENT = 0x5A5A5A5A5A5A5A5A


@pytest.mark.parametrize("max_segs", [1, 2, 64, 512])
def test_message_init_batch(max_segs):
    """message_init_kernel against oracle.message_init (message.zig:341-394) on the lattice's
    frames, every truncation of a dozen of them and the header error vectors, frame i at
    `in_off & 7` = i % 8, the tables full of a sentinel before. Status and count are the
    oracle's (count 0 for a failed message); an OK message's listed entries are exact and entries
    j >= min(count, max_segs) of its row still hold the sentinel; an entry of a failed message's row
    holds the sentinel or what the table lists for that segment (include/capnp_packed.h: the
    segments before the one that runs past the data may be listed). So no message writes into
    another's row."""
    frames = ms.init_frames()
    n = len(frames)
    offs, pos = [], 64
    for i, f in enumerate(frames):
        pos += (i % 8 - pos) % 8
        offs.append(pos)
        pos += len(f) + 8
    host = np.full(pos + 64, 0x77, dtype=np.uint8)  # 0x77777777 segments: past any frame's end
    for o, f in zip(offs, frames):
        host[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    assert {o % 8 for o in offs} == set(range(8))
    cnt = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    so = torch.full((n * max_segs,), INIT_SENT, dtype=torch.int64, device=DEV)
    sg = torch.full((n * max_segs,), INIT_SENT, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.message_init_batch(torch.from_numpy(host).to(DEV), i64(offs), i64([len(f) for f in frames]), max_segs, cnt,
                          so, sg, st)
    torch.cuda.synchronize()
    cnt, st = cnt.cpu().numpy(), st.cpu().numpy()
    so, sg = so.cpu().numpy().reshape(n, max_segs), sg.cpu().numpy().reshape(n, max_segs)
    seen = set()
    for i, f in enumerate(frames):
        rc, table = oracle.message_init(f, max_segs=ms.MAX_SEGS)
        assert st[i] == ms.INIT_CODES[rc], (i, len(f))
        seen.add(int(st[i]))
        if rc != 0:
            assert cnt[i] == 0, i
            listed = ms.header_entries(f)
            for j in range(max_segs):
                for got, col in ((int(so[i, j]), 0), (int(sg[i, j]), 1)):
                    assert got == INIT_SENT or (j < len(listed) and got == listed[j][col]), (i, j, got)
            continue
        assert cnt[i] == len(table), i
        k = min(len(table), max_segs)
        assert list(zip(so[i, :k].tolist(), sg[i, :k].tolist())) == [(int(a), int(c)) for a, c in table[:k]], i
        assert (so[i, k:] == INIT_SENT).all() and (sg[i, k:] == INIT_SENT).all(), (i, len(table))
    assert seen == {cp.OK, cp.END_OF_STREAM, cp.INVALID_SEGMENT_COUNT, cp.SEGMENT_COUNT_LIMIT_EXCEEDED,
                    cp.TRUNCATED_MESSAGE}
