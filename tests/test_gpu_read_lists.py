"""capnp_packed_list_heads_batch -> capnp_packed_lengths_to_offsets ->
capnp_packed_read_elements_batch on the device against the plain-Python model
of the reference's list readers (tests/list_streams.py) and the four interop fixtures.

Messages lie back to back between fillers of nonzero bytes, so a read outside a message changes a
result; every output array has canaries on both sides, and the rows past the element total are
canaries too."""
import struct

import numpy as np
import pytest

import capnp_packed as cp
import list_streams as ls
import struct_streams as ss
from list_streams import LIST_POINTER, LIST_STRUCT
from struct_streams import F

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


def dev_i64(values):
    return torch.as_tensor(np.asarray(values, dtype=np.uint64).view(np.int64)).to(DEV)


class Chain:
    """heads -> lengths_to_offsets -> elements over one batch, every buffer allocated up front
    (so the three calls can be captured), and the results on the host."""

    def __init__(self, d_in, offs, lens, kind, pointer_index, fields, path=(), elem_cap=None, with_count=True,
                 numbering=True, stream=None, run=True):
        self.n, self.nf = n, nf = len(offs), len(fields)
        self.d_in, self.kind, self.pointer_index, self.path = d_in, kind, pointer_index, tuple(path)
        self.fields, self.stream, self.with_count, self.numbering = cfields(fields), stream, with_count, numbering
        self.off, self.len = dev_i64(offs), dev_i64(lens)
        self.head = torch.full((2 * PAD * 32 + 32 * n,), 0xA5, dtype=torch.uint8, device=DEV)
        self.count = torch.full((2 * PAD + n,), CANARY, dtype=torch.int64, device=DEV)
        self.hst = torch.full((2 * PAD + n,), CANARY32, dtype=torch.int32, device=DEV)
        self.start = torch.full((2 * PAD + n + 1,), CANARY, dtype=torch.int64, device=DEV)
        nbytes = cp.lib().capnp_packed_scan_scratch_bytes(n)
        self.scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=DEV)
        self.scratch_bytes = nbytes
        self.cap = elem_cap
        if run:
            self.heads()
            self.scan()
            if elem_cap is None:
                self.cap = self.total()
            self.alloc()
            self.elements()

    def alloc(self):
        size = 2 * PAD + self.nf * self.cap
        self.out = torch.full((3, size), CANARY, dtype=torch.int64, device=DEV)
        self.st = torch.full((size,), CANARY32, dtype=torch.int32, device=DEV)
        self.num = torch.full((2, 2 * PAD + self.cap), CANARY32, dtype=torch.int32, device=DEV)

    def heads(self):
        cp.list_heads_batch(self.d_in, self.off, self.len, self.kind, self.pointer_index,
                            self.head[32 * PAD:32 * (PAD + self.n)], self.count[PAD:PAD + self.n],
                            self.hst[PAD:PAD + self.n], self.path, stream=self.stream)

    def scan(self):
        cp._raise(cp.lib().capnp_packed_lengths_to_offsets(
            self.count[PAD:].data_ptr(), self.n, 0, self.start[PAD:].data_ptr(), self.scratch.data_ptr(),
            self.scratch_bytes, cp._stream(self.stream)), "lengths_to_offsets")

    def total(self):
        return int(self.start[PAD + self.n].item())

    def elements(self, start=None):
        k = slice(PAD, PAD + self.nf * self.cap)
        e = slice(PAD, PAD + self.cap)
        cp.read_elements_batch(self.d_in, self.off, self.len, self.head[32 * PAD:],
                               self.start[PAD:] if start is None else start, self.kind, self.cap, self.fields,
                               self.out[0][k], self.out[1][k], self.st[k], self.out[2][k] if self.with_count else None,
                               self.num[0][e] if self.numbering else None, self.num[1][e] if self.numbering else None,
                               stream=self.stream)

    def reset(self):
        for t, c in ((self.count, CANARY), (self.hst, CANARY32), (self.start, CANARY), (self.out, CANARY),
                     (self.st, CANARY32), (self.num, CANARY32)):
            t.fill_(c)
        self.head.fill_(0xA5)

    def results(self):
        """heads [n] (LIST_HEAD_DTYPE), counts, head statuses, start [n + 1], and per element:
        parent, index, and status / value / len / count as [n_fields, cap]; canaries checked"""
        torch.cuda.synchronize()
        n, nf, cap = self.n, self.nf, self.cap
        head = self.head.cpu().numpy()
        assert (head[:32 * PAD] == 0xA5).all() and (head[32 * (PAD + n):] == 0xA5).all()
        count, hst, start = self.count.cpu().numpy(), self.hst.cpu().numpy(), self.start.cpu().numpy()
        assert (count[:PAD] == CANARY).all() and (count[PAD + n:] == CANARY).all()
        assert (hst[:PAD] == CANARY32).all() and (hst[PAD + n:] == CANARY32).all()
        assert (start[:PAD] == CANARY).all() and (start[PAD + n + 1:] == CANARY).all()
        out, st, num = self.out.cpu().numpy(), self.st.cpu().numpy(), self.num.cpu().numpy()
        k = PAD + nf * cap
        assert (out[:, :PAD] == CANARY).all() and (out[:, k:] == CANARY).all(), "an output was written outside its range"
        assert (st[:PAD] == CANARY32).all() and (st[k:] == CANARY32).all()
        assert (num[:, :PAD] == CANARY32).all() and (num[:, PAD + cap:] == CANARY32).all()
        if not self.with_count:
            assert (out[2] == CANARY).all(), "d_count is NULL: nothing may be written for it"
        if not self.numbering:
            assert (num == CANARY32).all()
        shape = (nf, cap)
        return dict(head=head[32 * PAD:32 * (PAD + n)].view(cp.LIST_HEAD_DTYPE), counts=count[PAD:PAD + n],
                    head_status=hst[PAD:PAD + n], start=start[PAD:PAD + n + 1], parent=num[0][PAD:PAD + cap],
                    index=num[1][PAD:PAD + cap], status=st[PAD:k].reshape(shape), value=out[0][PAD:k].reshape(shape),
                    length=out[1][PAD:k].reshape(shape), count=out[2][PAD:k].reshape(shape))

    def check(self, want):
        """want[i] = (Head, rows) of message i (list_streams.read_list); rows may stop early when
        the capacity does (they are compared up to it)"""
        r = self.results()
        heads = [tuple(int(x) for x in (h["status"], h["elems_off"], h["count"], h["segment"], h["seg_begin"],
                                        h["seg_bytes"], h["data_words"], h["pointer_words"])) for h in r["head"]]
        assert heads == [w[0].tuple() for w in want]
        assert r["counts"].tolist() == [w[0].count for w in want]
        assert r["head_status"].tolist() == [w[0].status for w in want]
        assert r["start"].tolist() == np.concatenate([[0], np.cumsum([w[0].count for w in want])]).tolist()
        total = int(r["start"][-1])
        rows = min(total, self.cap)
        parent = np.repeat(np.arange(self.n), [w[0].count for w in want])[:rows]
        index = np.concatenate([np.arange(w[0].count) for w in want] + [np.zeros(0, dtype=np.int64)])[:rows]
        if self.numbering:
            assert r["parent"][:rows].tolist() == parent.tolist()
            assert r["index"][:rows].tolist() == index.tolist()
            assert (r["parent"][rows:] == CANARY32).all() and (r["index"][rows:] == CANARY32).all()
        exp = np.zeros((4, self.nf, rows), dtype=np.uint64)
        for e in range(rows):
            row = want[parent[e]][1][index[e]]
            for f in range(self.nf):
                exp[:, f, e] = row[f]
        for name, j in (("status", 0), ("value", 1), ("length", 2), ("count", 3)):
            if name == "count" and not self.with_count:
                continue
            got = r[name]
            if rows:
                g = got[:, :rows].astype(np.int64).view(np.uint64) if name != "status" else got[:, :rows].astype(np.uint64)
                bad = np.argwhere(g != exp[j])
                assert not len(bad), (f"{name}: field {bad[0][0]} ({self.fields[bad[0][0]]}) of element {bad[0][1]} "
                                      f"(message {parent[bad[0][1]]}, element {index[bad[0][1]]}): "
                                      f"{g[tuple(bad[0])]} != {exp[j][tuple(bad[0])]}")
            assert (got[:, rows:] == (CANARY32 if name == "status" else CANARY)).all(), f"{name} written past the total"
        return r


def model(msgs, offs, kind, pointer_index, fields, path=(), cap=None):
    """the model's answers for messages laid out at offs; at most cap elements in all are read"""
    want, left = [], cap
    for data, off in zip(msgs, offs):
        head, rows = ls.read_list(data, kind, pointer_index, fields, path, base=off, limit=left)
        if left is not None:
            left = max(0, left - head.count)
        want.append((head, rows))
    return want


# ---- the corpus ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """The corpus in one shuffled layout on the device: (names, messages in that order, buffer, offsets, lengths)"""
    named = ls.corpus()
    order = np.random.default_rng(20261).permutation(len(named)).tolist()
    msgs = [d for _, d in named]
    buf, offs, lens = ss.layout(msgs, order)
    return [named[i][0] for i in order], [msgs[i] for i in order], dev_bytes(buf), offs, lens


@pytest.mark.parametrize("run", ls.RUNS, ids=lambda r: f"{'struct' if r[0] == LIST_STRUCT else 'pointer'}-{r[1]}-{r[2]}")
def test_corpus_against_the_model(corpus, run):
    names, msgs, d_in, offs, lens = corpus
    kind, index, path = run
    fields = ls.fields_of(kind)
    r = Chain(d_in, offs, lens, kind, index, fields, path).check(model(msgs, offs, kind, index, fields, path))
    if run in ls.RUNS[:4]:  # the lists read as what they are: hundreds of elements, good fields and failing ones
        assert int(r["start"][-1]) > 150 and (r["status"] != 0).sum() > 100 and (r["status"] == 0).sum() > 100


def test_corpus_three_times_over_without_count_and_numbering(corpus):
    """more than one block of messages; d_count, d_parent and d_index NULL"""
    names, msgs, d_in, offs, lens = corpus
    reps = 3 * 256 // len(msgs) + 1
    for kind, index in ((LIST_STRUCT, 0), (LIST_POINTER, 1)):
        fields = ls.fields_of(kind)
        want = model(msgs, offs, kind, index, fields)
        Chain(d_in, offs * reps, lens * reps, kind, index, fields, with_count=False, numbering=False).check(want * reps)


def test_one_field_a_call_and_paths_in_any_order(corpus):
    names, msgs, d_in, offs, lens = corpus
    for kind, index in ((LIST_STRUCT, 0), (LIST_POINTER, 1)):
        fields = ls.fields_of(kind)
        order = np.random.default_rng(7).permutation(len(fields)).tolist()
        want = model(msgs, offs, kind, index, fields)
        pick = lambda cols: [(h, [[row[f] for f in cols] for row in rows]) for h, rows in want]
        Chain(d_in, offs, lens, kind, index, [fields[f] for f in order]).check(pick(order))
        for f in (0, len(fields) - 1):
            Chain(d_in, offs, lens, kind, index, [fields[f]]).check(pick([f]))


def test_misaligned_offset_and_4gib_length_are_invalid_argument(corpus):
    names, msgs, d_in, offs, lens = corpus
    g = names.index("near")
    offs2 = [offs[g], offs[g] + 4, offs[g], offs[g]]
    lens2 = [lens[g], lens[g], 1 << 32, lens[g]]
    good = ls.read_list(msgs[g], LIST_STRUCT, 0, ls.STRUCT_FIELDS, base=offs[g])
    bad = (ls.Head(ss.INVALID_ARGUMENT), [])
    Chain(d_in, offs2, lens2, LIST_STRUCT, 0, ls.STRUCT_FIELDS).check([good, bad, bad, good])


# ---- the interop fixtures, from their packed files ---------------------------------------------
PACKED = {"fixture_single.bin": "fixture_single_packed.bin", "fixture_far.bin": "fixture_far_packed.bin",
          "binary": "packed", "segmented": "segmented-packed"}


@pytest.fixture(scope="module")
def decoded():
    """The four packed fixtures through read_packed_messages, laid out on the device"""
    names = sorted(PACKED)
    frames = []
    for name in names:
        got, used, status = cp.read_packed_messages(ss.fixture(PACKED[name]))
        assert status == "Ok" and len(got) == 1 and bytes(got[0]) == ss.fixture(name)
        frames.append(bytes(got[0]))
    buf, offs, lens = ss.layout(frames, list(range(4)))
    return names, frames, dev_bytes(buf), offs, lens, buf


def test_fixtures_from_their_packed_files(decoded):
    names, frames, d_in, offs, lens, host = decoded
    w = [names.index("fixture_far.bin"), names.index("fixture_single.bin")]
    sub = lambda xs: [xs[i] for i in w]
    # the Widget lists, with the values the reference's interop test asserts
    r = Chain(d_in, sub(offs), sub(lens), LIST_STRUCT, 1, [F(ss.U32, 0), F(ss.U32, 4)]).check(
        model(sub(frames), sub(offs), LIST_STRUCT, 1, [F(ss.U32, 0), F(ss.U32, 4)]))
    assert r["counts"].tolist() == [3, 3] and r["value"].tolist() == [[1, 2, 3] * 2, [10, 20, 30] * 2]
    r = Chain(d_in, sub(offs), sub(lens), LIST_POINTER, 2, [F(ss.TEXT, 0)]).check(
        model(sub(frames), sub(offs), LIST_POINTER, 2, [F(ss.TEXT, 0)]))
    texts = [host[v:v + l] for v, l in zip(r["value"][0].tolist(), r["length"][0].tolist())]
    assert texts == [b"alpha", b"beta"] * 2
    r = Chain(d_in, sub(offs), sub(lens), LIST_POINTER, 10, [F(ss.LIST_16, 0)]).check(
        model(sub(frames), sub(offs), LIST_POINTER, 10, [F(ss.LIST_16, 0)]))
    lists = [host[v:v + l] for v, l in zip(r["value"][0].tolist(), r["length"][0].tolist())]
    assert lists == [struct.pack("<2H", 7, 8), struct.pack("<3H", 9, 10, 11)] * 2 and r["count"][0].tolist() == [2, 3] * 2
    # TestAllTypes' lists, one segment and 125 segments (double-far pads of layout B), batched with the Widgets
    sfields = [F(ss.U64, 0), F(ss.U64, 8), F(ss.U8, 47), F(ss.TEXT, 0), F(ss.DATA, 1), F(ss.TEXT, 0, path=(2,)),
               F(ss.LIST_16, 6)]
    r = Chain(d_in, offs, lens, LIST_STRUCT, 17, sfields).check(model(frames, offs, LIST_STRUCT, 17, sfields))
    assert [int(c) for c in r["counts"]] == [3 if n in ("binary", "segmented") else 0 for n in names]
    for index in (15, 16):
        Chain(d_in, offs, lens, LIST_POINTER, index, ls.POINTER_FIELDS).check(
            model(frames, offs, LIST_POINTER, index, ls.POINTER_FIELDS))


def test_struct_reader_mirrors_on_the_fixtures():
    for name in ("fixture_single.bin", "fixture_far.bin"):
        root = cp.Message.init(ss.fixture(name)).get_root_struct()
        lst = root.read_struct_list(1)
        assert lst.len() == 3
        assert [(lst.get(k).read_u32(0), lst.get(k).read_u32(4)) for k in range(3)] == [(1, 10), (2, 20), (3, 30)]
        assert lst.get(0).read_u64(8) == 0 and lst.get(2).read_text(0) == b""
        with pytest.raises(IndexError):
            lst.get(3)
        tags = root.read_text_list(2)
        assert tags.len() == 2 and [tags.get(0), tags.get(1)] == [b"alpha", b"beta"]
        with pytest.raises(IndexError):
            tags.get(2)
        pl = root.read_pointer_list(10)
        assert pl.len() == 2 and pl.get_u16_list(0) == [7, 8] and pl.get_u16_list(1) == [9, 10, 11]
        with pytest.raises(cp.InvalidPointer):
            pl.get_u32_list(0)
        with pytest.raises(cp.InvalidPointer):
            pl.get_text(0)  # a List(UInt16) is no text
        with pytest.raises(cp.InvalidPointer):
            pl.get_struct(1)
        with pytest.raises(cp.InvalidInlineCompositePointer):
            root.read_struct_list(2)
        with pytest.raises(cp.InvalidPointer):
            root.read_pointer_list(1)
        with pytest.raises(cp.OutOfBounds):
            root.read_text_list(11)
    a = cp.Message.init(ss.fixture("binary")).get_root_struct().read_struct_list(17)
    b = cp.Message.init_packed(ss.fixture("segmented-packed")).get_root_struct().read_struct_list(17)
    assert a.len() == b.len() == 3
    for k in range(3):
        assert a.get(k).read_text(0) == b.get(k).read_text(0) != b""
        assert a.get(k).read_u64(8) == b.get(k).read_u64(8)


def test_struct_reader_mirrors_on_the_corpus():
    by_name = dict(ls.corpus())
    root = cp.Message.init(by_name["dfar_a_list_elements_dfar"]).get_root_struct()
    lst = root.read_struct_list(0)
    e = lst.get(2)
    assert lst.len() == 3 and e.read_u32(0) == 3000 and e.read_u32(4) == 2 and e.read_bool(1, 3) is True
    assert e.read_text(0) == b"elem 2" and e.read_data(1) == bytes([2, 3, 4])
    assert e.read_struct(2).read_u32(0) == 79 and e.read_struct(2).read_text(0) == b"in 2"
    pl = root.read_pointer_list(1)
    assert pl.len() == 10 and pl.get_text(0) == b"alpha" and pl.get_text(1) == b"" and pl.get_text(8) == b"tail"
    assert pl.get_u16_list(2) == [7, 8] and pl.get_u64_list(5) == [1 << 40, 3] and pl.get_u32_list(6) == [1, 2, 3]
    assert pl.get_data(4) == bytes([9, 8, 7, 6, 5, 4, 3, 2, 1])
    s = pl.get_struct(3)
    assert s.read_u32(0) == 4242 and s.read_struct(0).read_data(0) == b"deep data"
    with pytest.raises(cp.InvalidPointer):
        pl.get_data(1)  # null
    with pytest.raises(cp.InvalidPointer):
        pl.get_struct(9)  # a capability
    child = root.read_struct(2)
    assert child.read_struct_list(0).len() == 2 and child.read_text_list(1).get(3) == b"no nul"
    for name, err in (("near_size_6", cp.InvalidInlineCompositePointer), ("far_lands_on_far", cp.InvalidPointer),
                      ("dfar_first_is_struct", cp.InvalidFarPointer), ("far_segment_id", cp.InvalidSegmentId),
                      ("near_words_past_segment", cp.OutOfBounds)):
        with pytest.raises(err):
            cp.Message.init(by_name[name]).get_root_struct().read_struct_list(0)
    with pytest.raises(cp.NestingLimitExceeded):
        cp.Message.init(by_name["plist_chain_8_hops"]).get_root_struct().read_pointer_list(1)


# ---- the parent lookup at its edges ---------------------------------------------------------------
def keyed(i, count, room=0, dw=1):
    """A one-segment message whose root (no data, one pointer) holds a struct list of `count`
    elements of dw data words, U32@0 = i and U32@4 = k; count None: a null list pointer (the head
    fails). `room` more elements' worth of words follow the list."""
    if count is None:
        words = [ss.struct_ptr(0, 0, 1), 0]
    else:
        words = [ss.struct_ptr(0, 0, 1), ss.list_ptr(0, 7, count * dw), ss.struct_ptr(count, dw, 0)]
        for k in range(count + room):
            words += [(i & 0xFFFFFFFF) | (k << 32)] + [0x3333333333333333] * (dw - 1)
    return ss.frame([struct.pack(f"<{len(words)}Q", *words)])


KEY_FIELDS = [F(ss.U64, 0), F(ss.U32, 4), F(ss.U32, 0)]


def keyed_chain(counts, elem_cap=None, fields=KEY_FIELDS, dw=1, **kw):
    msgs = [keyed(i, c, dw=dw) for i, c in enumerate(counts)]
    buf, offs, lens = ss.layout(msgs, list(range(len(msgs))))
    c = Chain(dev_bytes(buf), offs, lens, LIST_STRUCT, 0, fields, elem_cap=elem_cap, **kw)
    r = c.check(model(msgs, offs, LIST_STRUCT, 0, fields, cap=c.cap))
    rows = min(int(r["start"][-1]), c.cap)
    # the key says which message and which element a row was read from
    assert (r["value"][0][:rows] == (r["parent"][:rows].astype(np.int64) | (r["index"][:rows].astype(np.int64) << 32))).all()
    return r


@pytest.mark.parametrize("counts", [
    [1], [257], [600],                                   # one message: one element, two blocks, three blocks
    [0, 1] * 300, [1, 0] * 300,                          # alternating
    [5] + [0] * 300 + [7] + [3] * 100,                   # 300 empty lists inside one block's range: the fallback
    [0] * 300 + [2], [2] + [0] * 300, [1] * 255 + [0] * 257 + [1] * 300,
    [64] * 4, [256], [255, 1], [1] * 256,                # a total of exactly 256
    [128] * 4, [512], [1] * 512, [0, 511, 0, 1, 0],      # and of exactly 512
    [3, None, 4], [None, 2, None, None, 300, None],      # failed heads between good ones
], ids=lambda c: f"{len(c)}-messages-{sum(x or 0 for x in c)}-elements-{c[0]}")
def test_parent_lookup(counts):
    r = keyed_chain(counts)
    assert int(r["start"][-1]) == sum(x or 0 for x in counts)


def test_all_lists_empty_writes_nothing():
    r = keyed_chain([0] * 50, elem_cap=40)
    assert int(r["start"][-1]) == 0
    r = keyed_chain([None, 0, None], elem_cap=1)
    assert r["head_status"].tolist() == [ss.INVALID_POINTER, ss.OK, ss.INVALID_POINTER]


@pytest.mark.parametrize("cap", [1, 255, 256, 257, 599, 600, 601, 1000])
def test_elem_cap_smaller_and_larger_than_the_total(cap):
    r = keyed_chain([100, 0, 200, 300], elem_cap=cap)  # check() wants canaries in every row past min(total, cap)
    assert int(r["start"][-1]) == 600


def test_a_huge_list_of_zero_word_elements_is_bounded_by_elem_cap():
    words = [ss.struct_ptr(0, 0, 1), ss.list_ptr(0, 7, 0), ss.struct_ptr(100000, 0, 0)]
    msgs = [keyed(0, 3), ss.frame([struct.pack("<3Q", *words)]), keyed(2, 3)]
    buf, offs, lens = ss.layout(msgs, [0, 1, 2])
    fields = [F(ss.U32, 0), F(ss.U64, 8), F(ss.BOOL, 0, 1), F(ss.TEXT, 0)]
    c = Chain(dev_bytes(buf), offs, lens, LIST_STRUCT, 0, fields, elem_cap=1000)
    r = c.check(model(msgs, offs, LIST_STRUCT, 0, fields, cap=1000))
    assert r["counts"].tolist() == [3, 100000, 3] and int(r["start"][-1]) == 100006
    assert r["parent"].tolist() == [0] * 3 + [1] * 997 and r["index"][3:].tolist() == list(range(997))
    for name in ("status", "value", "length", "count"):  # each data field of a zero-word element is the default
        assert not r[name][:, 3:].any()


def test_a_start_array_that_is_not_the_heads_gives_invalid_argument():
    """counts 2, 5, 2, 5 ... read with the start array of 5, 2, 5, 2 ...: the messages with two
    elements are asked for five. Every message has room for five elements' words after its list
    pointer, so even without the check no read would leave its message."""
    counts = [2, 5] * 40
    msgs = [keyed(i, c, room=5 - c) for i, c in enumerate(counts)]
    buf, offs, lens = ss.layout(msgs, list(range(len(msgs))))
    c = Chain(dev_bytes(buf), offs, lens, LIST_STRUCT, 0, KEY_FIELDS)
    good = c.check(model(msgs, offs, LIST_STRUCT, 0, KEY_FIELDS))
    shifted = np.concatenate([[0], np.cumsum(counts[1:] + counts[:1])])
    assert shifted[-1] == c.cap
    c.out.fill_(CANARY)
    c.st.fill_(CANARY32)
    c.num.fill_(CANARY32)
    c.elements(start=dev_i64(shifted))
    r = c.results()
    for e in range(c.cap):
        i = int(np.searchsorted(shifted, e, side="right")) - 1
        k = e - int(shifted[i])
        assert (int(r["parent"][e]), int(r["index"][e])) == (i, k)
        if k < counts[i]:
            want = [(ss.OK, i | (k << 32), 8, 1), (ss.OK, k, 4, 1), (ss.OK, i, 4, 1)]
        else:
            want = [(ss.INVALID_ARGUMENT, 0, 0, 0)] * 3
        got = [(int(r["status"][f][e]), int(r["value"][f][e]), int(r["length"][f][e]), int(r["count"][f][e]))
               for f in range(3)]
        assert got == want, (e, i, k)
    assert good["counts"].tolist() == counts


# ---- elements -> gather ----------------------------------------------------------------------------
def test_text_list_strings_of_a_batch_as_dense_bytes():
    rng = np.random.default_rng(11)
    msgs, texts = [], []
    for i in range(300):
        b = ss.Builder(1)
        b.alloc(0, [ss.struct_ptr(0, 0, 1), 0])
        mine = [bytes(rng.integers(1, 255, size=int(rng.integers(0, 40)), dtype=np.uint8)) for _ in range(i % 7)]
        first = b.alloc(0, [0] * len(mine))
        b.seg[0][1] = ss.list_ptr(first - 2, 6, len(mine))
        for k, t in enumerate(mine):
            raw = t + b"\0"
            b.point((0, first + k), (0, b.alloc_bytes(0, raw)), lambda o, n=len(raw): ss.list_ptr(o, 2, n))
        msgs.append(b.bytes())
        texts += mine
    buf, offs, lens = ss.layout(msgs, list(range(len(msgs))))
    d_in = dev_bytes(buf)
    out = cp.read_list_batch(d_in, dev_i64(offs), dev_i64(lens), cp.LIST_POINTER, 0, [cp.Field(cp.FIELD_TEXT, 0)])
    head_status, counts, start, total, parent, index, value, length, count, status = out
    assert total == len(texts) and not head_status.cpu().numpy().any() and not status.cpu().numpy().any()
    assert counts.cpu().tolist() == [i % 7 for i in range(300)]
    dst_off = cp.lengths_to_offsets(length[0])
    nbytes = int(dst_off[-1].item())
    assert nbytes == sum(len(t) for t in texts)
    dense = torch.full((nbytes + 16,), 0xEE, dtype=torch.uint8, device=DEV)
    gst = torch.full((total,), -1, dtype=torch.int32, device=DEV)
    cp.gather_batch(d_in, value[0], length[0], dense, dst_off, gst, cap=nbytes)
    torch.cuda.synchronize()
    assert not gst.cpu().numpy().any()
    assert dense.cpu().numpy().tobytes() == b"".join(texts) + b"\xEE" * 16
    # with a capacity: nothing syncs, the total stays on the device, the rows past it are untouched
    out = cp.read_list_batch(d_in, dev_i64(offs), dev_i64(lens), cp.LIST_POINTER, 0, [cp.Field(cp.FIELD_TEXT, 0)],
                             max_elements=500)
    assert isinstance(out[3], torch.Tensor) and int(out[3].item()) == len(texts)
    assert out[6].shape == (1, 500) and out[7][0][:500].cpu().tolist() == [len(t) for t in texts[:500]]


# ---- graph capture -----------------------------------------------------------------------------------
def test_graph_capture_of_the_chain_and_replay_on_a_second_batch():
    def batch(seed):
        counts = np.random.default_rng(seed).integers(0, 9, size=700).tolist()
        msgs = [keyed(i + seed, c, dw=2) for i, c in enumerate(counts)]
        return msgs, ss.layout(msgs, list(range(len(msgs))))

    (m1, (buf1, offs1, lens1)), (m2, (buf2, offs2, lens2)) = batch(1), batch(2)
    size = max(len(buf1), len(buf2))
    d_in = torch.zeros(size, dtype=torch.uint8, device=DEV)
    d_in[:len(buf1)] = dev_bytes(buf1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    fields = [F(ss.U64, 0), F(ss.U64, 8), F(ss.U32, 4)]
    cap = 3000  # fixed: below the first batch's total or above it, the graph is the same
    c = Chain(d_in, offs1, lens1, LIST_STRUCT, 0, fields, elem_cap=cap, stream=s, run=False)
    c.alloc()
    with torch.cuda.stream(s):  # warm-up
        c.heads(), c.scan(), c.elements()
    s.synchronize()
    c.check(model(m1, offs1, LIST_STRUCT, 0, fields, cap=cap))
    g = torch.cuda.CUDAGraph()
    c.stream = None
    with torch.cuda.graph(g, stream=s):
        c.heads(), c.scan(), c.elements()
    for msgs, buf, offs, lens in ((m2, buf2, offs2, lens2), (m1, buf1, offs1, lens1)):
        d_in.zero_()
        d_in[:len(buf)] = dev_bytes(buf)
        c.off.copy_(dev_i64(offs))
        c.len.copy_(dev_i64(lens))
        c.reset()
        g.replay()
        c.check(model(msgs, offs, LIST_STRUCT, 0, fields, cap=cap))
