"""capnp_packed_gather_batch on the device: a ragged byte copy, byte-exact at
every source and destination alignment. The destination is pre-filled with a pattern and
compared WHOLE against a numpy gather, so the gaps between rows, the bytes around the output
and neighbouring rows that share a 16-byte chunk are all covered."""
import numpy as np
import pytest

import capnp_packed as cp
import struct_streams as ss

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = list(range(0, 41)) + [255, 256, 257, 4095, 4096, 4097]
LONG = (1 << 20) + 3


def pattern(nbytes):
    return ((np.arange(nbytes, dtype=np.uint32) * 7 + 3) % 253).astype(np.uint8)


def gather(src, rows, out_bytes, cap=None, base_shift=(0, 0), stream=None, n_status_extra=5):
    """rows: (src_off, len, dst_off). Runs the call with the source at d_in + base_shift[0] and
    the output at d_out + base_shift[1] (the arrays' own base addresses misaligned); returns
    (output, statuses, expected output, expected statuses)."""
    si, so = base_shift
    n = len(rows)
    cap = out_bytes if cap is None else cap
    d_src = torch.zeros(si + len(src) + 64, dtype=torch.uint8, device=DEV)
    d_src[si:si + len(src)] = torch.from_numpy(src).to(DEV)
    fill = pattern(so + out_bytes + 64)
    d_out = torch.from_numpy(fill.copy()).to(DEV)
    a = np.asarray(rows, dtype=np.int64).reshape(n, 3)
    st = torch.full((n + n_status_extra,), -7, dtype=torch.int32, device=DEV)
    cp.gather_batch(d_src[si:], torch.from_numpy(a[:, 0].copy()).to(DEV), torch.from_numpy(a[:, 1].copy()).to(DEV),
                    d_out[so:], torch.from_numpy(a[:, 2].copy()).to(DEV), st[:n], cap=cap, stream=stream)
    torch.cuda.synchronize()
    want, want_st = fill.copy(), np.zeros(n + n_status_extra, dtype=np.int32)
    want_st[n:] = -7
    for k, (s, l, d) in enumerate(rows):
        if d + l > cap:
            want_st[k] = cp.OUT_OF_SPACE
        else:
            want[so + d:so + d + l] = src[s:s + l]
    return d_out.cpu().numpy(), st.cpu().numpy(), want, want_st


def check(got, st, want, want_st):
    assert np.array_equal(st, want_st)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[:3]}"


def alignment_rows(lengths, rng):
    """every (source alignment, destination alignment) pair for every length: the rows nearly
    back to back on the destination side (gaps of 0-15 bytes keep the pattern)"""
    rows, s, d = [], 0, 0
    for l in lengths:
        for sa in range(16):
            for da in range(16):
                s += (sa - s) % 16
                d += (da - d) % 16
                rows.append((s, l, d))
                s += l + int(rng.integers(0, 3))
                d += l
    return rows, s, d


@pytest.fixture(scope="module")
def source():
    return np.random.default_rng(77).integers(1, 256, size=5 << 20, dtype=np.uint8)


@pytest.mark.parametrize("base_shift", [(0, 0), (1, 0), (0, 9), (5, 13)])
def test_every_alignment_pair(source, base_shift):
    rng = np.random.default_rng(1)
    rows, s_end, d_end = alignment_rows(LENGTHS, rng)
    assert s_end + LONG + 16 < len(source)
    order = rng.permutation(len(rows)).tolist()  # a wave's rows are not neighbours in memory
    rows = [rows[i] for i in order] + [(s_end + 5, LONG, d_end + 11)]
    check(*gather(source, rows, d_end + 11 + LONG, base_shift=base_shift))


def test_rows_in_order_share_their_chunks(source):
    rows, s_end, d_end = alignment_rows(list(range(0, 41)), np.random.default_rng(2))
    check(*gather(source, rows, d_end))


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("length", [0, 1, 17, 513, 4097])
def test_batch_sizes(source, n, length):
    rows = [(3 + k * (length + 5), length, 1 + k * length) for k in range(n)]
    check(*gather(source, rows, 1 + n * length))


def test_rows_of_length_zero_touch_nothing(source):
    rows = [(k, 0, 3 * k) for k in range(200)] + [(0, 0, 600), (7, 9, 100), (0, 0, 109)]
    got, st, want, want_st = gather(source, rows, 600)
    check(got, st, want, want_st)
    assert (st[:203] == cp.OK).all()


def test_out_cap_cut(source):
    rng = np.random.default_rng(3)
    rows, d = [], 0
    for k in range(300):
        l = int(rng.integers(0, 700))
        rows.append((int(rng.integers(0, 1 << 20)), l, d))
        d += l
    rows.append((0, 4096, d))
    total = d + 4096
    for cap in (total, total - 1, d, d // 2, 17, 0):
        got, st, want, want_st = gather(source, rows, total, cap=cap)
        check(got, st, want, want_st)
        assert cap == total or (st == cp.OUT_OF_SPACE).any()
    # a length that wraps dst + len is cut too, and nothing is read for it
    got, st, want, want_st = gather(source, [(0, 8, 0), (0, (1 << 63) - 1, 1 << 62), (8, 8, 8)], 64, cap=64)
    assert st[:3].tolist() == [cp.OK, cp.OUT_OF_SPACE, cp.OK]
    assert np.array_equal(got[:16], source[:16]) and np.array_equal(got[16:], want[16:])


def test_padded_tensor(source):
    stride, n = 48, 100
    lens = [k % 49 for k in range(n)]
    rows = [(1000 + 53 * k, lens[k], k * stride) for k in range(n)]
    got, st, want, want_st = gather(source, rows, n * stride)
    check(got, st, want, want_st)


def widget_batch(copies):
    msgs = [ss.fixture("fixture_single.bin"), ss.fixture("fixture_far.bin")] * (copies // 2)
    buf, offs, lens = ss.layout(msgs, list(range(len(msgs))))
    return (torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).to(DEV),
            torch.as_tensor(np.asarray(offs, dtype=np.int64)).to(DEV), torch.as_tensor(np.asarray(lens, dtype=np.int64)).to(DEV))


def test_fields_then_offsets_then_gather():
    n = 130
    d_in, off, ln = widget_batch(n)
    fields = [cp.Field(cp.FIELD_DATA, 3), cp.Field(cp.FIELD_TEXT, 0), cp.Field(cp.FIELD_LIST_64, 9)]
    out = torch.zeros(3, 3 * n, dtype=torch.int64, device=DEV)
    st = torch.full((3 * n,), -1, dtype=torch.int32, device=DEV)
    cp.read_fields_batch(d_in, off, ln, fields, out[0], out[1], st, out[2])
    for f, want in enumerate((bytes([1, 2, 3, 4, 5]), b"widget", np.array([1.125, -2.25]).tobytes())):
        src_off, src_len = out[0][f * n:(f + 1) * n], out[1][f * n:(f + 1) * n]  # a column, unchanged
        dst_off = cp.lengths_to_offsets(src_len)
        total = len(want) * n
        dense = torch.full((total + 32,), 0xCC, dtype=torch.uint8, device=DEV)
        gst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        cp.gather_batch(d_in, src_off, src_len, dense, dst_off, gst, cap=total)
        torch.cuda.synchronize()
        assert int(dst_off[n].item()) == total
        assert (st.cpu().numpy() == 0).all() and (gst.cpu().numpy() == 0).all()
        got = dense.cpu().numpy().tobytes()
        assert got[:total] == want * n and got[total:] == b"\xCC" * 32


def test_graph_capture_and_two_replays(source):
    rows, s_end, d_end = alignment_rows([0, 5, 16, 33, 600], np.random.default_rng(4))
    n = len(rows)
    a = np.asarray(rows, dtype=np.int64)
    d_src = torch.from_numpy(source[:s_end + 64].copy()).to(DEV)
    cols = [torch.from_numpy(a[:, k].copy()).to(DEV) for k in range(3)]
    d_out = torch.zeros(d_end + 64, dtype=torch.uint8, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cp.gather_batch(d_src, cols[0], cols[1], d_out, cols[2], st, cap=d_end, stream=s)  # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cp.gather_batch(d_src, cols[0], cols[1], d_out, cols[2], st, cap=d_end)
    for shift in (1, 2):  # other source bytes for each replay
        src = np.roll(source[:s_end + 64], shift * 1001)
        d_src.copy_(torch.from_numpy(src.copy()).to(DEV))
        fill = pattern(d_end + 64)
        d_out.copy_(torch.from_numpy(fill).to(DEV))
        st.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = fill.copy()
        for so, l, do in rows:
            want[do:do + l] = src[so:so + l]
        assert np.array_equal(d_out.cpu().numpy(), want) and (st.cpu().numpy() == 0).all()
