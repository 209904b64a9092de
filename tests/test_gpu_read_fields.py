"""capnp_packed_read_fields_batch on the device against the plain-Python model
of the reference's read path (tests/struct_streams.py) and the four interop fixtures.

Messages lie back to back in shuffled order between fillers of nonzero bytes, so a read outside
a message changes a result; every output array has canaries on both sides."""
import numpy as np
import pytest

import capnp_packed as cp
import struct_streams as ss

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = -0x5A5A5A5A5A5A5A5B
CANARY32 = -0x5A5A5A5B
PAD = 19  # canary entries on each side of every output


def cfields(fields):
    return [cp.Field(f.kind, f.offset, f.bit, f.path) for f in fields]


def dev_bytes(raw):
    return torch.from_numpy(np.frombuffer(bytes(raw), dtype=np.uint8).copy()).to(DEV)


class Read:
    """One read_fields_batch call and its results on the host as [n_fields, n] arrays."""

    def __init__(self, d_in, offs, lens, fields, with_count=True, stream=None):
        self.n, self.nf = n, nf = len(offs), len(fields)
        self.d_in, self.fields, self.stream = d_in, cfields(fields), stream
        self.off = torch.as_tensor(np.asarray(offs, dtype=np.uint64).view(np.int64)).to(DEV)
        self.len = torch.as_tensor(np.asarray(lens, dtype=np.uint64).view(np.int64)).to(DEV)
        self.out = torch.full((3, 2 * PAD + nf * n), CANARY, dtype=torch.int64, device=DEV)
        self.st = torch.full((2 * PAD + nf * n,), CANARY32, dtype=torch.int32, device=DEV)
        self.with_count = with_count
        self.call()

    def call(self):
        k = slice(PAD, PAD + self.nf * self.n)
        cp.read_fields_batch(self.d_in, self.off, self.len, self.fields, self.out[0][k], self.out[1][k], self.st[k],
                             self.out[2][k] if self.with_count else None, stream=self.stream)

    def results(self):
        """(status, value, len, count), each [n_fields, n]; the canaries are checked on the way"""
        torch.cuda.synchronize()
        out, st = self.out.cpu().numpy(), self.st.cpu().numpy()
        k = PAD + self.nf * self.n
        assert (out[:, :PAD] == CANARY).all() and (out[:, k:] == CANARY).all(), "an output was written outside its range"
        assert (st[:PAD] == CANARY32).all() and (st[k:] == CANARY32).all()
        if not self.with_count:
            assert (out[2] == CANARY).all(), "d_count is NULL: nothing may be written for it"
        shape = (self.nf, self.n)
        return (st[PAD:k].reshape(shape), out[0][PAD:k].view(np.uint64).reshape(shape),
                out[1][PAD:k].view(np.uint64).reshape(shape), out[2][PAD:k].view(np.uint64).reshape(shape))

    def check(self, want):
        """want[i][f] = (status, value, len, count) of field f of message i"""
        st, v, l, c = self.results()
        for i in range(self.n):
            for f in range(self.nf):
                got = (int(st[f][i]), int(v[f][i]), int(l[f][i]), int(c[f][i]) if self.with_count else want[i][f][3])
                assert got == tuple(want[i][f]), f"message {i}, field {f} ({self.fields[f]}): {got} != {want[i][f]}"


@pytest.fixture(scope="module")
def corpus():
    """The corpus in one shuffled layout on the device, and the model's answers for all of
    struct_streams.FIELDS: (names, device buffer, offsets, lengths, want[i][f])."""
    named = ss.corpus()
    order = np.random.default_rng(20260).permutation(len(named)).tolist()
    msgs = [d for _, d in named]
    buf, offs, lens = ss.layout(msgs, order)
    want = [ss.read_fields(msgs[i], ss.FIELDS, base=offs[k]) for k, i in enumerate(order)]
    return [named[i][0] for i in order], dev_bytes(buf), offs, lens, want


def chunks(total, n):
    """index lists of n messages each that together cover range(total) (the last one wraps)"""
    return [[(a + j) % total for j in range(n)] for a in range(0, total, n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_corpus_against_the_model_32_fields(corpus, n):
    names, d_in, offs, lens, want = corpus
    for idx in chunks(len(names), n):
        Read(d_in, [offs[i] for i in idx], [lens[i] for i in idx], ss.FIELDS).check([want[i] for i in idx])


@pytest.mark.parametrize("n", [1, 65, 130])
def test_corpus_against_the_model_one_field_a_call(corpus, n):
    names, d_in, offs, lens, want = corpus
    for f, field in enumerate(ss.FIELDS):
        idx = chunks(len(names), n)[f % len(chunks(len(names), n))]
        Read(d_in, [offs[i] for i in idx], [lens[i] for i in idx], [field]).check([[want[i][f]] for i in idx])


def test_more_than_one_block(corpus):
    names, d_in, offs, lens, want = corpus
    idx = [i % len(names) for i in range(3 * 256 + 7)]
    for fields, cols in ((ss.FIELDS, range(32)), (ss.FIELDS[16:19], range(16, 19))):
        Read(d_in, [offs[i] for i in idx], [lens[i] for i in idx], fields).check(
            [[want[i][f] for f in cols] for i in idx])


@pytest.mark.parametrize("n", [1, 65])
def test_count_may_be_null(corpus, n):
    names, d_in, offs, lens, want = corpus
    idx = chunks(len(names), n)[1]
    Read(d_in, [offs[i] for i in idx], [lens[i] for i in idx], ss.FIELDS, with_count=False).check(
        [want[i] for i in idx])


def test_misaligned_offset_and_4gib_length_are_invalid_argument(corpus):
    names, d_in, offs, lens, want = corpus
    good = [i for i, nm in enumerate(names) if nm in ("one_segment", "5_segments_far_pointers", "data_long")]
    offs2 = [offs[good[0]], offs[good[1]] + 4, offs[good[1]], offs[good[2]], offs[good[2]] + 1, offs[good[0]]]
    lens2 = [lens[good[0]], lens[good[1]], lens[good[1]], 1 << 32, lens[good[2]], (1 << 63) + 8]
    bad = [(ss.INVALID_ARGUMENT, 0, 0, 0)] * 32
    Read(d_in, offs2, lens2, ss.FIELDS).check([want[good[0]], bad, want[good[1]], bad, bad, bad])


def test_same_message_many_times_and_paths_in_any_order(corpus):
    """the fields of one path need not be neighbours: the struct is resolved again"""
    names, d_in, offs, lens, want = corpus
    order = np.random.default_rng(5).permutation(32).tolist()
    i = names.index("512_segments_dfar_pointers")
    Read(d_in, [offs[i]] * 70, [lens[i]] * 70, [ss.FIELDS[f] for f in order]).check(
        [[want[i][f] for f in order]] * 70)


def test_graph_capture_and_two_replays(corpus):
    names, d_in0, offs, lens, want = corpus
    n = 65
    first, second = chunks(len(names), n)[:2]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r = Read(d_in0, [offs[i] for i in first], [lens[i] for i in first], ss.FIELDS, stream=s)  # warm-up
    s.synchronize()
    r.check([want[i] for i in first])
    r.stream = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.call()
    for idx in (second, first):  # the inputs change between the replays; the descriptors were captured
        r.off.copy_(torch.as_tensor(np.asarray([offs[i] for i in idx], dtype=np.int64)).to(DEV))
        r.len.copy_(torch.as_tensor(np.asarray([lens[i] for i in idx], dtype=np.int64)).to(DEV))
        r.out.fill_(CANARY)
        r.st.fill_(CANARY32)
        g.replay()
        r.check([want[i] for i in idx])


# ---- the interop fixtures, from their packed files -----------------------------------------------
PACKED = {"fixture_single.bin": "fixture_single_packed.bin", "fixture_far.bin": "fixture_far_packed.bin",
          "binary": "packed", "segmented": "segmented-packed"}


@pytest.fixture(scope="module")
def decoded():
    """The four packed fixtures through read_message_batch: (names, framed bytes on the device, offsets, lengths)"""
    names = sorted(PACKED)
    packed = [ss.fixture(PACKED[n]) for n in names]
    p_off = np.cumsum([0] + [len(p) for p in packed[:-1]])
    slot = max(len(ss.fixture(n)) for n in names) + 8
    d_pk = dev_bytes(b"".join(packed))
    d_out = torch.full((4 * slot + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    out_off = torch.arange(0, 4 * slot, slot, dtype=torch.int64, device=DEV)
    out_cap = torch.full((4,), slot, dtype=torch.int64, device=DEV)
    out_len = torch.zeros(4, dtype=torch.int64, device=DEV)
    used = torch.zeros(4, dtype=torch.int64, device=DEV)
    st = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    cp.read_message_batch(d_pk, torch.as_tensor(p_off).to(DEV), torch.as_tensor([len(p) for p in packed]).to(DEV),
                          d_out, out_off, out_cap, out_len, used, st)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * 4
    lens = out_len.cpu().tolist()
    assert lens == [len(ss.fixture(n)) for n in names]
    return names, d_out, out_off.cpu().tolist(), lens


def test_fixtures_from_their_packed_files(decoded):
    names, d_out, offs, lens = decoded
    host = d_out.cpu().numpy().tobytes()
    for k, name in enumerate(names):
        table = ss.TABLES[name]
        r = Read(d_out, [offs[k]], [lens[k]], [row[0] for row in table])
        st, v, l, c = r.results()
        got = [(int(st[f][0]), int(v[f][0]), int(l[f][0]), int(c[f][0])) for f in range(len(table))]
        ss.check_table(host, table, got)  # slice values are offsets from d_out: the bytes are read there
        assert got == ss.read_fields(ss.fixture(name), [row[0] for row in table], base=offs[k])


def test_fixtures_batched_together(decoded):
    names, d_out, offs, lens = decoded
    fields = [row[0] for row in ss.ALL_TYPES] + [row[0] for row in ss.WIDGET[:4]]
    Read(d_out, offs, lens, fields).check(
        [ss.read_fields(ss.fixture(n), fields, base=offs[k]) for k, n in enumerate(names)])


def test_struct_reader_mirror_on_the_fixtures():
    for name in ("fixture_single.bin", "fixture_far.bin"):
        root = cp.Message.init(ss.fixture(name)).get_root_struct()
        assert root.read_u32(0) == 123 and root.read_text(0) == b"widget"
        assert root.read_data(3) == bytes([1, 2, 3, 4, 5])
        assert root.read_u16_list(4) == [10, 20, 30] and root.read_u32_list(5) == [1000, 2000]
        assert root.read_u64_list(6) == [123456789, 987654321]
        assert root.read_bool_list(7) == [True, False, True, False, True]
        assert root.read_f32_list(8) == [1.25, 2.5, -3.75] and root.read_f64_list(9) == [1.125, -2.25]
        assert root.read_text(11) == b""
        with pytest.raises(cp.InvalidPointer):
            root.read_data(4)
        with pytest.raises(cp.OutOfBounds):
            root.read_data(11)
    for name, via in (("binary", cp.Message.init), ("segmented-packed", cp.Message.init_packed)):
        root = via(ss.fixture(name)).get_root_struct()
        assert root.read_bool(0, 0) is True and root.read_u8(1) == 133 and root.read_u16(2) == 53191
        assert root.read_union_discriminant(2) == 53191
        assert root.read_u32(4) == 4282621618 and root.read_u64(8) == 18446620616920539271
        assert root.read_u64(48) == 0 and root.read_u64(44) == 0 and root.read_u8(47) == 201
        assert root.read_text(0) == b"foo" and root.read_data(1) == b"bar"
        child = root.read_struct(2)
        assert child.read_u8(1) == 244 and child.read_text(0) == b"baz" and child.read_data(1) == b"qux"
        deep = child.read_struct(2).read_struct(2)
        assert deep.read_text(0) == b"really nested"
        with pytest.raises(cp.InvalidPointer):
            deep.read_struct(2)
        with pytest.raises(cp.InvalidPointer):
            root.read_u16_list(5)


def test_struct_reader_mirror_raises_the_root_errors():
    by_name = dict(ss.corpus())
    for name, err in (("root_null", cp.InvalidPointer), ("root_chain_8_hops", cp.NestingLimitExceeded),
                      ("dfar_first_word_is_struct", cp.InvalidFarPointer), ("far_root_segment_id", cp.InvalidSegmentId),
                      ("root_one_word_too_long", cp.TruncatedMessage), ("far_root_pad_past_segment", cp.OutOfBounds)):
        with pytest.raises(err):
            cp.Message.init(by_name[name]).get_root_struct()
