"""capnp_packed_build_fields_batch on the device against the model of
tests/build_streams.py. The output is pre-filled with a pattern and compared WHOLE with what the
model gives, so the bytes between and around the messages, the padding the call must write as
zeros and the untouched slots of failed messages are all covered."""
import random

import numpy as np
import pytest

import build_streams as bs
import capnp_packed as cp
from build_streams import Op

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
S = bs.STRUCT
LONG = (1 << 20) + 3
LENGTHS = list(range(0, 42)) + [255, 256, 257, 511, 512, 513, 4095, 4096, 4097]


def pattern(nbytes):
    return ((np.arange(nbytes, dtype=np.uint32) * 7 + 3) % 253).astype(np.uint8)


def c_ops(ops):
    return [cp.BuildOp(o.kind, o.offset, o.bit, o.target, o.dw, o.pw) for o in ops]


def upload_columns(cols, n_ops):
    """cols[i][k] -> op-major value / length / count tensors"""
    a = np.array(cols, dtype=np.uint64).reshape(len(cols), n_ops, 3)
    return [torch.from_numpy(np.ascontiguousarray(a[:, :, j].T).reshape(-1).view(np.int64)).to(DEV) for j in range(3)]


def upload_pool(pool, shift=0):
    d = torch.zeros(shift + len(pool) + 64, dtype=torch.uint8, device=DEV)
    if pool:
        d[shift:shift + len(pool)] = torch.from_numpy(np.frombuffer(pool, dtype=np.uint8).copy()).to(DEV)
    return d[shift:]


def sizes(ops, cols, pool):
    return [bs.build_message(ops, c, pool, sizes_only=True)[1] for c in cols]


def run_build(ops, cols, pool, offs, caps, out_bytes, pool_shift=0, d_pool=None, pool_len=None, stream=None):
    """One call with the output a pattern; returns nothing and asserts the whole output, the
    lengths and the statuses against the model."""
    n = len(cols)
    d_pool = upload_pool(pool, pool_shift) if d_pool is None else d_pool
    pool_len = len(pool) if pool_len is None else pool_len
    v, l, c = upload_columns(cols, len(ops))
    fill = pattern(out_bytes + 64)
    d_out = torch.from_numpy(fill.copy()).to(DEV)
    d_off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    d_cap = torch.tensor(caps, dtype=torch.int64, device=DEV)
    out_len = torch.full((n + 3,), -5, dtype=torch.int64, device=DEV)
    st = torch.full((n + 3,), -7, dtype=torch.int32, device=DEV)
    cp.build_fields_batch(d_pool, c_ops(ops), v, l, d_out, d_off, d_cap, out_len[:n], st[:n], count=c,
                          pool_len=pool_len, stream=stream)
    torch.cuda.synchronize()
    want, want_st, want_len = fill.copy(), np.full(n + 3, -7, dtype=np.int32), np.full(n + 3, -5, dtype=np.int64)
    base = d_out.data_ptr()
    for i in range(n):
        s, nbytes, framed = bs.build_message(ops, cols[i], pool, pool_len=pool_len, out_addr=base + offs[i],
                                             cap=caps[i])
        want_st[i], want_len[i] = s, nbytes
        if s == bs.OK:
            want[offs[i]:offs[i] + nbytes] = np.frombuffer(framed, dtype=np.uint8)
    assert np.array_equal(st.cpu().numpy(), want_st), (st.cpu().numpy()[:n], want_st[:n])
    assert np.array_equal(out_len.cpu().numpy(), want_len)
    got = d_out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[:3]}"
    return got, want_len[:n]


def dense_layout(lens, gaps=(0, 8), start=0):
    """messages back to back, with gaps that give both residues of the destination mod 16"""
    offs, at = [], start
    for i, ln in enumerate(lens):
        at += gaps[i % len(gaps)]
        offs.append(at)
        at += ln
    return offs, at


def check_program(ops, rows, **kw):
    pool, cols = bs.columns(ops, rows, pool_pad=kw.pop("pool_pad", 0))
    lens = sizes(ops, cols, pool)
    offs, total = dense_layout(lens, start=kw.pop("start", 0))
    return run_build(ops, cols, pool, offs, lens, total, **kw)


# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_with_absent_and_present_ops(n):
    rng = random.Random(n)
    ops = [Op(S, dw=2, pw=4), Op(bs.U64, 0), Op(bs.TEXT, 0), Op(S, 1, dw=1, pw=1), Op(bs.U16, 10), Op(bs.DATA, 0, target=3),
           Op(bs.BOOL, 3, bit=5, target=3), Op(bs.LIST_BIT, 2), Op(bs.LIST_32, 3), Op(bs.U32, 6)]
    rows = [bs.gen_row(rng, ops, bs.SHORT_LENGTHS + [600], absent=0.3) for _ in range(n)]
    check_program(ops, rows)


@pytest.mark.parametrize("pool_shift,start", [(0, 0), (5, 8)])
def test_every_length_and_source_alignment(pool_shift, start):
    """every length at every source alignment 0..15 as EVERY slice kind: a message carries the
    length as Text, Data, a bit list and a 16-bit list, all four at the row's alignment (the
    16-bit list rounds an odd length down, so 4095 and 4097 reach it as 4094 and 4096; the next
    test gives it odd-free edges of its own). The messages' sizes differ by words, so
    destinations fall on both residues mod 16."""
    ops = [Op(S, dw=1, pw=4), Op(bs.TEXT, 0), Op(bs.DATA, 1), Op(bs.LIST_BIT, 2), Op(bs.LIST_16, 3), Op(bs.U64, 0)]
    rng = random.Random(9)
    rows = []
    for ln in LENGTHS:
        for a in range(16):
            row = [None] + [bs.gen_slice(rng, ops[k].kind, ln) for k in range(1, 5)] + [rng.getrandbits(64)]
            rows.append((a, row))
    rng.shuffle(rows)  # a wave's rows are not neighbours in memory
    pool, cols = bs.columns(ops, [r for _, r in rows], align=[a for a, _ in rows for _ in range(4)])
    assert all(col[k][0] % 16 == a for (a, _), col in zip(rows, cols) for k in range(1, 5))
    lens = sizes(ops, cols, pool)
    offs, total = dense_layout(lens, start=start)
    assert {o % 16 for o in offs} == {0, 8}
    run_build(ops, cols, pool, offs, lens, total, pool_shift=pool_shift)


def test_wide_lists_at_their_own_edges():
    """16-, 32- and 64-bit lists at the element counts around the short-row threshold and 4 KiB,
    at every source alignment"""
    ops = [Op(S, dw=0, pw=3), Op(bs.LIST_16, 0), Op(bs.LIST_32, 1), Op(bs.LIST_64, 2)]
    rng = random.Random(10)
    rows = []
    for ln in (0, 8, 248, 256, 264, 504, 512, 520, 4088, 4096, 4104):
        for a in range(16):
            rows.append((a, [None] + [bs.gen_slice(rng, ops[k].kind, ln + 2 * (3 - k) * (k < 3)) for k in range(1, 4)]))
    pool, cols = bs.columns(ops, [r for _, r in rows], align=[a for a, _ in rows for _ in range(3)])
    lens = sizes(ops, cols, pool)
    offs, total = dense_layout(lens)
    run_build(ops, cols, pool, offs, lens, total)


@pytest.mark.parametrize("align", [0, 3, 8, 15])
def test_a_long_slice_among_short_ones(align):
    rng = random.Random(4 + align)
    ops = [Op(S, dw=1, pw=2), Op(bs.DATA, 0), Op(bs.TEXT, 1), Op(bs.U8, 3)]
    rows = [[None, b"abc", b"x", 1], [None, bs.gen_slice(rng, bs.DATA, LONG), bs.gen_slice(rng, bs.TEXT, 700), 2],
            [None, b"", b"", 3]]
    pool, cols = bs.columns(ops, rows, align=[(align + 5) % 16, 1, align, (align + 9) % 16, 0, 0])
    assert cols[1][1][0] % 16 == align and cols[1][1][1] == LONG
    lens = sizes(ops, cols, pool)
    offs, total = dense_layout(lens, start=8 * (align & 1))
    run_build(ops, cols, pool, offs, lens, total)


def test_programs_of_1_to_32_ops():
    seen = set()
    for ops, rows in bs.corpus(programs=32, rows=3):
        seen.add(len(ops))
        check_program(ops, rows)
    assert seen >= set(range(1, 33))


def test_63_struct_words_build_and_64_are_refused():
    rng = random.Random(6)
    ops = [Op(S, dw=30, pw=3), Op(S, 0, dw=28, pw=2), Op(bs.TEXT, 1, target=1), Op(bs.U64, 232), Op(bs.U32, 220, target=1),
           Op(bs.DATA, 2), Op(bs.U8, 239)]
    check_program(ops, [bs.gen_row(rng, ops, bs.SHORT_LENGTHS, absent=0.1) for _ in range(70)])
    z = torch.zeros(8, dtype=torch.int64, device=DEV)
    with pytest.raises(cp.InvalidArgument):
        cp.build_fields_batch(None, c_ops([Op(S, dw=30, pw=3), Op(S, 0, dw=29, pw=2)]), z, z, None, None, None, z[:1],
                              torch.zeros(1, dtype=torch.int32, device=DEV))


def test_good_and_failing_messages_in_one_wave():
    """one message per status among good ones; LIST_TOO_LARGE and OUT_OF_BOUNDS come from the
    column values alone, MESSAGE_TOO_LARGE from eight slices of 2^29 - 1 bytes of a real pool"""
    ops = ([Op(S, dw=1, pw=11)] + [Op(bs.DATA, p) for p in range(8)] +
           [Op(bs.LIST_16, 8), Op(bs.LIST_BIT, 9), Op(bs.TEXT, 10)])
    big = (1 << 29) - 1
    d_pool = torch.empty(1 << 29, dtype=torch.uint8, device=DEV)
    head = np.random.default_rng(1).integers(0, 256, size=4096, dtype=np.uint8)
    d_pool[:4096] = torch.from_numpy(head).to(DEV)
    pool_len = 1 << 29

    class Pool:  # the model reads only the head (failed messages read nothing)
        def __getitem__(self, s):
            assert s.stop <= 4096
            return head[s].tobytes()

        def __len__(self):
            return pool_len

    good = [(0, 0, 0)] + [(7 * p, 3 + p, 0) for p in range(8)] + [(100, 6, 0), (200, 2, 13), (300, 5, 0)]

    def with_(k, entry):
        return good[:k] + [entry] + good[k + 1:]

    cols = [good] * 20
    cols[2] = with_(9, (100, 7, 0))                      # LIST_16 of 7 bytes
    cols[5] = with_(10, (200, 3, 13))                    # 13 bits are 2 bytes
    cols[7] = with_(11, (0, big, 0))                     # TEXT: len + 1 = 2^29 elements
    cols[8] = with_(3, (pool_len - 4, 5, 0))             # runs past the pool
    cols[9] = with_(3, ((1 << 64) - 2, 4, 0))            # the sum would wrap
    cols[11] = [(0, 0, 0)] + [(0, big, 0)] * 8 + good[9:]  # 8 x 2^29 bytes padded: 4 GiB
    cols[15] = with_(1, (0, bs.ABSENT, 0))               # an absent op among them
    size = bs.build_message(ops, good, Pool(), sizes_only=True)[1]
    offs = [i * (size + 8) for i in range(20)]
    caps = [size] * 20
    offs[3] += 4                                         # a misaligned destination
    caps[13] = size - 8                                  # 8 short
    caps[11] = 0
    run_build(ops, cols, Pool(), offs, caps, 20 * (size + 8), d_pool=d_pool, pool_len=pool_len)
    want = {2: cp.INVALID_ARGUMENT, 3: cp.INVALID_ARGUMENT, 5: cp.INVALID_ARGUMENT, 7: cp.LIST_TOO_LARGE,
            8: cp.OUT_OF_BOUNDS, 9: cp.OUT_OF_BOUNDS, 11: cp.MESSAGE_TOO_LARGE, 13: cp.OUT_OF_SPACE}
    for i in range(20):
        st = bs.build_message(ops, cols[i], Pool(), out_addr=offs[i], cap=caps[i])[0]
        assert st == want.get(i, cp.OK), i


def test_sizes_then_offsets_then_dense_build():
    rng = random.Random(8)
    ops = [Op(S, dw=1, pw=2), Op(bs.U32, 4), Op(bs.TEXT, 0), Op(bs.LIST_64, 1)]
    n = 300
    rows = [bs.gen_row(rng, ops, bs.SHORT_LENGTHS + [257, 520]) for _ in range(n)]
    pool, cols = bs.columns(ops, rows)
    d_pool = upload_pool(pool)
    v, l, c = upload_columns(cols, len(ops))
    out_len = torch.zeros(n, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.build_fields_batch(d_pool, c_ops(ops), v, l, None, None, None, out_len, st, pool_len=len(pool))
    want = sizes(ops, cols, pool)
    assert out_len.cpu().tolist() == want and not st.cpu().numpy().any()
    off = cp.lengths_to_offsets(out_len)
    total = int(off[n].item())
    assert total == sum(want)
    d_out = torch.full((total + 16,), 0xCC, dtype=torch.uint8, device=DEV)
    cp.build_fields_batch(d_pool, c_ops(ops), v, l, d_out, off, out_len.clone(), out_len, st, pool_len=len(pool))
    torch.cuda.synchronize()
    frames = b"".join(bs.build_message(ops, col, pool, cap=1 << 40)[2] for col in cols)
    assert not st.cpu().numpy().any()
    assert d_out.cpu().numpy().tobytes() == frames + b"\xCC" * 16


def test_chain_build_validate_read_encode_split_read():
    """build -> validate_batch OK -> read_fields_batch returns the input columns -> the packed
    stream of encode_framed_dense_batch (both dialects) -> split_streams + read_message_batch give
    the built bytes back"""
    rng = random.Random(12)
    ops = [Op(S, dw=2, pw=3), Op(bs.U64, 0), Op(bs.U16, 8), Op(bs.BOOL, 10, bit=2), Op(bs.TEXT, 0), Op(bs.DATA, 1),
           Op(bs.LIST_BIT, 2)]
    n = 130
    rows = [bs.gen_row(rng, ops, bs.SHORT_LENGTHS + [300], absent=0.0) for _ in range(n)]
    pool, cols = bs.columns(ops, rows)
    lens = sizes(ops, cols, pool)
    offs, total = dense_layout(lens, gaps=(0,))
    got, _ = run_build(ops, cols, pool, offs, lens, total)
    d_msgs = torch.from_numpy(got[:total + 16].copy()).to(DEV)
    d_off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    d_len = torch.tensor(lens, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.validate_batch(d_msgs, d_off, d_len, st)
    assert not st.cpu().numpy().any()
    # the reads mirror the writes
    fields = [cp.Field(o.kind, o.offset, o.bit) for o in ops[1:]]
    nf = len(fields)
    out = torch.zeros(3, nf * n, dtype=torch.int64, device=DEV)
    fst = torch.full((nf * n,), -1, dtype=torch.int32, device=DEV)
    cp.read_fields_batch(d_msgs, d_off, d_len, fields, out[0], out[1], fst, out[2])
    assert not fst.cpu().numpy().any()
    r = out.cpu().numpy().reshape(3, nf, n)
    host = got.tobytes()
    for i, row in enumerate(rows):
        assert int(r[0, 0, i]) & bs.M64 == row[1] and r[0, 1, i] == row[2] & 0xFFFF and r[0, 2, i] == row[3] & 1
        for f, k in ((3, 4), (4, 5), (5, 6)):
            data, cnt = row[k] if k == 6 else (row[k], len(row[k]))
            content = bytearray(data)
            if k == 6 and cnt % 8:
                content[-1] &= (1 << (cnt % 8)) - 1
            assert (r[1, f, i], r[2, f, i]) == (len(data), cnt)
            assert host[r[0, f, i]:r[0, f, i] + len(data)] == bytes(content)
    # the read's columns, passed back unchanged, build the same bytes
    ops2 = [ops[0]] + ops[1:]
    cols_v = torch.cat([torch.zeros(n, dtype=torch.int64, device=DEV), out[0]])
    cols_l = torch.cat([torch.zeros(n, dtype=torch.int64, device=DEV), out[1]])
    cols_c = torch.cat([torch.zeros(n, dtype=torch.int64, device=DEV), out[2]])
    d_again = torch.full((total + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    len2 = torch.zeros(n, dtype=torch.int64, device=DEV)
    cp.build_fields_batch(d_msgs, c_ops(ops2), cols_v, cols_l, d_again, d_off, d_len, len2, st, count=cols_c,
                          pool_len=total)
    assert not st.cpu().numpy().any() and d_again[:total].cpu().numpy().tobytes() == host[:total]
    for dialect in ("zig", "cxx"):
        d_pk = torch.empty(cp.encode_bound(total) + 64, dtype=torch.uint8, device=DEV)
        pk_off = torch.empty(n + 1, dtype=torch.int64, device=DEV)
        pk_len = torch.empty(n, dtype=torch.int64, device=DEV)
        cp.encode_framed_dense_batch(d_msgs, d_off, d_len, d_pk, pk_off, pk_len, st, dialect=dialect)
        assert not st.cpu().numpy().any()
        end = int(pk_off[n].item())
        s_off = torch.zeros(1, dtype=torch.int64, device=DEV)
        s_len = torch.full((1,), end, dtype=torch.int64, device=DEV)
        first = torch.empty(2, dtype=torch.int64, device=DEV)
        tab = torch.empty((3, n), dtype=torch.int64, device=DEV)
        used = torch.empty(1, dtype=torch.int64, device=DEV)
        sst = torch.empty(1, dtype=torch.int32, device=DEV)
        cp.split_streams(d_pk, s_off, s_len, first, tab[0], tab[1], tab[2], used, sst)
        assert int(first[1].item()) == n and int(used.item()) == end and int(sst.item()) == cp.OK
        assert tab[2].cpu().tolist() == lens
        back = torch.full((total + 16,), 0xA5, dtype=torch.uint8, device=DEV)
        rl = torch.empty(n, dtype=torch.int64, device=DEV)
        rc = torch.empty(n, dtype=torch.int64, device=DEV)
        cp.read_message_batch(d_pk, tab[0], tab[1], back, d_off, d_len, rl, rc, st)
        assert not st.cpu().numpy().any() and rl.cpu().tolist() == lens
        assert back[:total].cpu().numpy().tobytes() == host[:total]


def test_graph_capture_of_sizes_offsets_build():
    rng = random.Random(13)
    ops = [Op(S, dw=1, pw=2), Op(bs.U64, 0), Op(bs.TEXT, 0), Op(bs.DATA, 1)]
    n = 100
    rows = [bs.gen_row(rng, ops, [0, 5, 16, 33, 600], absent=0.1) for _ in range(n)]
    pool, cols = bs.columns(ops, rows)
    d_pool = upload_pool(pool)
    v, l, c = upload_columns(cols, len(ops))
    want = sizes(ops, cols, pool)
    total = sum(want)
    out_len = torch.zeros(n, dtype=torch.int64, device=DEV)
    caps = torch.full((n,), 1 << 20, dtype=torch.int64, device=DEV)
    off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device=DEV)
    cops = c_ops(ops)

    def chain():
        cp.build_fields_batch(d_pool, cops, v, l, None, None, None, out_len, st, pool_len=len(pool))
        cp.lengths_to_offsets(out_len, out=off)
        cp.build_fields_batch(d_pool, cops, v, l, d_out, off, caps, out_len, st, pool_len=len(pool))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()  # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    v0 = v.clone()
    for salt in (1, 2):  # other values for each replay
        v2 = v0.clone()
        v2[n:2 * n] += salt
        v.copy_(v2)
        fill = pattern(total + 64)
        d_out.copy_(torch.from_numpy(fill).to(DEV))
        st.fill_(-1)
        out_len.zero_()
        g.replay()
        torch.cuda.synchronize()
        frames = b"".join(
            bs.build_message(ops, [col[0], ((col[1][0] + salt) & bs.M64,) + col[1][1:]] + col[2:], pool, cap=1 << 40)[2]
            for col in cols)
        assert not st.cpu().numpy().any() and out_len.cpu().tolist() == want
        assert d_out.cpu().numpy().tobytes() == frames + fill[total:].tobytes()


@pytest.mark.parametrize("seed", ["A", "B", "C", "D", "E"])
def test_message_builder_mirror(seed):
    from test_build_streams import VECTORS, words
    want = words(VECTORS[seed][1])
    b = cp.MessageBuilder()
    if seed == "A":
        root = b.allocate_struct(1, 1)
        root.write_u32(0, 0x11223344)
        root.write_text(0, "hi")
    elif seed == "B":
        root = b.allocate_struct(0, 2)
        child = root.init_struct(1, 1, 0)
        child.write_u8(7, 0xAB)
        root.write_data(0, bytes(range(1, 10)))
        child.write_bool(0, 3, True)
    elif seed == "C":
        b.allocate_struct(0, 1).write_text(0, b"")
    elif seed == "D":
        b.allocate_struct(0, 1).write_data(0, b"")
    else:
        root = b.allocate_struct(1, 2)
        root.init_struct(0, 0, 0)
        root.write_u16(6, 0xBEEF)
        root.write_bool_list(1, [True] * 11)
    assert b.to_bytes() == want
    assert bytes(b.segments[0]) == want[8:] and len(b.segments) == 1
    m = cp.Message.init(want)
    assert bytes(m.segments[0]) == want[8:]


def test_message_builder_with_segments_is_unchanged():
    b = cp.MessageBuilder()
    b.create_segment(bytes(16))
    b.create_segment(bytes(8))
    assert b.to_bytes() == cp.frame_segments([bytes(16), bytes(8)])
    with pytest.raises(cp.InvalidArgument):
        b.allocate_struct(1, 0)
    b = cp.MessageBuilder()
    b.allocate_struct(1, 0)
    with pytest.raises(cp.InvalidArgument):  # a built message has segment 0 only
        b.create_segment(bytes(8))
