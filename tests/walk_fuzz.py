"""Generated messages, mutants and descriptor tables for the message walker
(capnp-zig_amd/csrc/kernels/message_walk.h): what test_walk_fuzz.py (the
host twin of the walker against the models, no GPU) and test_gpu_walk_fuzz.py (the three kernels
against the models) share. Everything here is deterministic from SEED.

Bases are the two corpus schemas (struct_streams.standard, list_streams.message) with every
layout choice drawn: the number of segments on both sides of kSrSegs = 4, which segment holds
what, near / far / double-far pointers, element shapes and counts, and far chains of 7 and 8
hops. A mutant is a base with one or two words damaged (at least half of them words the model's
walk of the base reads), a segment-table entry moved with the length kept, or a cut at any byte.
The corpora of struct_streams.py and list_streams.py stay as they are."""
import contextlib
import struct as _struct

import numpy as np

import list_streams as ls
import struct_streams as ss
from list_streams import LIST_POINTER, LIST_STRUCT
from struct_streams import F, far_ptr, list_ptr, struct_ptr

SEED = 20261021
NSEGS = (1, 2, 3, 4, 5, 6, 9)  # kSrSegs = 4: lookups below it and at or above it
ELEM_LIMIT = 64                # elements of one list the stand-alone program reads


# ---------------------------------------------------------------------------
# which words a walk reads
# ---------------------------------------------------------------------------
@contextlib.contextmanager
def recording():
    """the (segment, offset in the message) of every word the model reads, in order"""
    seen = []
    plain = ss.Msg.word

    def word(self, seg, pos):
        seen.append((seg, self.starts[seg] + pos))
        return plain(self, seg, pos)

    ss.Msg.word = word
    try:
        yield seen
    finally:
        ss.Msg.word = plain


# ---------------------------------------------------------------------------
# bases
# ---------------------------------------------------------------------------
def _pick(rng, items):
    return items[int(rng.integers(len(items)))]


def struct_base(rng):
    """struct_streams.standard with every choice drawn -> (bytes, a description)"""
    nseg = _pick(rng, NSEGS)
    home, pad_seg = int(rng.integers(nseg)), int(rng.integers(nseg))
    root = _pick(rng, ["far", "dfar"] + (["near", "near"] if home == 0 else []))
    ptrs = _pick(rng, ["near", "far", "dfar"])
    text = bytes(rng.integers(1, 255, size=int(rng.integers(0, 12)), dtype=np.uint8)) + (b"\0" if rng.random() < .6 else b"")
    data = bytes(rng.integers(0, 255, size=int(rng.integers(0, 20)), dtype=np.uint8))
    kw = dict(nseg=nseg, root=root, ptrs=ptrs, text=text, data=data, home=home, pad_seg=pad_seg)
    chain = None
    if rng.random() < .2:  # a far chain at the depth limit: 7 hops resolve, 8 do not
        chain, hops = _pick(rng, ["root", "child", "list"]), _pick(rng, [7, 8])
        if chain == "root":
            kw.update(root="far", root_hops=hops)
        elif chain == "child":
            kw["edit"] = lambda b, w: b.point((w["root_ptrs"][0], w["root_ptrs"][1] + 2), w["child"],
                                              lambda o: struct_ptr(o, 1, 2), via="far", hops=hops, pad_seg=pad_seg)
        else:
            kw["edit"] = lambda b, w: b.point((w["root_ptrs"][0], w["root_ptrs"][1] + 1), w["data"],
                                              lambda o: list_ptr(o, 2, len(data)), via="far", hops=hops, pad_seg=pad_seg)
        chain = (chain, hops)
    return ss.standard(**kw), dict(schema="struct", nseg=nseg, home=home, root=root, ptrs=ptrs, chain=chain)


def list_base(rng):
    """list_streams.message with every choice drawn -> (bytes, a description)"""
    nseg = _pick(rng, NSEGS)
    list_seg, eseg, pad_seg = (int(rng.integers(nseg)) for _ in range(3))
    via = _pick(rng, ["far", "dfar_a", "dfar_b"] + (["near", "near"] if list_seg == 0 else []))
    evia = _pick(rng, ["far", "dfar"] + (["near", "near"] if eseg == list_seg else []))
    count, pcount = int(rng.integers(0, 18)), int(rng.integers(0, 18))
    dw, pw = int(rng.integers(0, 5)), int(rng.integers(0, 5))
    chain, edit = None, None
    if rng.random() < .2:
        chain, hops = _pick(rng, ["plist", "slot", "elem"]), _pick(rng, [7, 8])
        if chain == "plist":
            edit = lambda b, w: b.point((0, w["root_ptrs"][1] + 1), w["plist_first"],
                                        lambda o: list_ptr(o, 6, w["plist_count"]), via="far", hops=hops, pad_seg=pad_seg)
        elif chain == "slot" and pcount:
            edit = lambda b, w: b.point(w["plist_first"], (0, w["root"][1]), lambda o: struct_ptr(o, 1, 4), via="far",
                                        hops=hops, pad_seg=pad_seg)
        elif chain == "elem" and count and pw:
            def edit(b, w):
                s, first = w["slist_first"]
                t = b.alloc_bytes(eseg, b"chained\0")
                b.point((s, first + dw), (eseg, t), lambda o: list_ptr(o, 2, 8), via="far", hops=hops, pad_seg=pad_seg)
        chain = (chain, hops) if edit else None
    data = ls.message(nseg=nseg, via=via, count=count, dw=dw, pw=pw, evia=evia, list_seg=list_seg, eseg=eseg,
                      pad_seg=pad_seg, pcount=pcount, edit=edit)
    return data, dict(schema="list", nseg=nseg, list_seg=list_seg, eseg=eseg, via=via, evia=evia, count=count,
                      dw=dw, pw=pw, chain=chain)


def read_words(data, schema):
    """offsets in `data` of the words the model's walk of this (undamaged) base reads: (the spine:
    the words on the way to a struct or to a list's head, every word read)"""
    out = []
    for spine in (True, False):
        with recording() as seen:
            if schema == "struct":
                ss.read_fields(data, [F(ss.U8, 0, path=(2, 1, 0)[:k]) for k in range(4)] if spine else ss.FIELDS)
            else:
                for kind, index, path in ls.RUNS:
                    ls.read_list(data, kind, index, [] if spine else ls.fields_of(kind), path)
        out.append(sorted({off for _, off in seen}))
    return tuple(out)


# ---------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------
KINDS = ("flip", "type", "far", "offset", "struct", "list", "null", "table", "cut")
_WEIGHTS = np.array([2, 2, 3, 3, 2, 3, .5, 1.5, 0], dtype=float)  # "cut" is drawn on its own (the `cut` share)
_SIZE_BYTES = {2: 1, 3: 2, 4: 4, 5: 8, 6: 8, 7: 8}


def _mutate_word(rng, kind, w, pw, seg_words, all_words):
    """word w at word index pw of a segment of seg_words words; all_words: every segment's words"""
    nseg = len(all_words)
    if kind == "flip":
        return w ^ (1 << int(rng.integers(64)))
    if kind == "type":
        return (w & ~3) | int(rng.integers(4))
    if kind == "null":
        return 0
    if kind == "far":
        which = int(rng.integers(4)) if w & 3 == 2 else 3
        double, pad, seg = (w >> 2) & 1, (w >> 3) & 0x1FFFFFFF, w >> 32
        if which in (1, 3):
            seg = _pick(rng, [nseg - 1, nseg, 0xFFFFFFFF, int(rng.integers(nseg)), int(rng.integers(nseg))])
        if which in (0, 3):
            double = int(rng.integers(2)) if which == 3 else double ^ 1
        if which in (2, 3):
            n = all_words[seg] if seg < nseg else seg_words
            pad = max(0, _pick(rng, [0, n - 2, n - 1, n, int(rng.integers(n + 1)), int(rng.integers(n + 1))]))
        return far_ptr(double, pad, seg)
    if kind == "offset":  # bits 2..31: a struct's or list's offset, a tag's count
        cur = ss.offset_words(w)
        to = _pick(rng, [0, seg_words - 1, seg_words, int(rng.integers(seg_words + 1))]) - pw - 1
        off = _pick(rng, [cur + 1, cur - 1, cur + 2, cur - 2, cur + int(rng.integers(-8, 9)), to, to, to])
        return (w & ~0xFFFFFFFC) | ((off & 0x3FFFFFFF) << 2)
    if kind == "struct":  # data words / pointers: a struct pointer's, a tag's
        dw, pc = (w >> 32) & 0xFFFF, w >> 48
        room = max(0, seg_words - (pw + 1 + ss.offset_words(w)))  # words to the segment's end, were it near
        if rng.random() < .5:
            dw = max(0, _pick(rng, [dw + 1, dw - 1, int(rng.integers(6)), room - pc, room - pc + 1]))
        else:
            pc = max(0, _pick(rng, [pc + 1, pc - 1, int(rng.integers(10)), room - dw, room - dw + 1]))
        return (w & 0xFFFFFFFF) | ((dw & 0xFFFF) << 32) | ((pc & 0xFFFF) << 48)
    if kind == "list":  # element size and count
        size, count = (w >> 32) & 7, w >> 35
        room = max(0, seg_words - (pw + 1 + ss.offset_words(w)))
        if rng.random() < .4:
            size = int(rng.integers(8))
        else:
            per = _SIZE_BYTES.get(size, 1)
            fill = 8 * room // per - (1 if size == 7 else 0)
            count = max(0, _pick(rng, [count + 1, count - 1, 0, int(rng.integers(20)), fill, fill + 1, 8 * room + 1]))
        return (w & 0xFFFFFFFF) | (size << 32) | ((count & 0x1FFFFFFF) << 35)
    raise ValueError(kind)


def mutate(rng, data, words, cut=.1):
    """one or two mutations of a base; `words`: read_words(base). A damaged word is one of the
    spine (a quarter), any word the walk reads (a third) or any word of the body."""
    buf = bytearray(data)
    nseg = _struct.unpack_from("<I", buf, 0)[0] + 1
    sizes = list(_struct.unpack_from(f"<{nseg}I", buf, 4))
    header = 4 * (1 + nseg + (1 - nseg % 2))
    starts = np.concatenate([[header], header + 8 * np.cumsum(sizes)])
    body = (len(buf) - header) // 8
    for _ in range(1 + int(rng.random() < .35)):
        if rng.random() < cut:
            return bytes(buf[:int(rng.integers(len(buf)))])
        kind = KINDS[int(rng.choice(len(KINDS), p=_WEIGHTS / _WEIGHTS.sum()))]
        if kind == "table":  # a segment boundary moves; the message keeps its length
            s, d = int(rng.integers(nseg)), _pick(rng, [1, -1, 2, -2])
            entry = lambda i: _struct.unpack_from("<I", buf, 4 + 4 * i)[0]
            _struct.pack_into("<I", buf, 4 + 4 * s, max(0, entry(s) + d))
            if nseg > 1 and rng.random() < .7:  # and the neighbour gives or takes the words
                t = s + 1 if s + 1 < nseg else s - 1
                _struct.pack_into("<I", buf, 4 + 4 * t, max(0, entry(t) - d))
            continue
        if body == 0:
            continue
        r = rng.random()
        pool = words[0] if r < .25 else words[1] if r < .6 else None
        at = _pick(rng, pool) if pool else header + 8 * int(rng.integers(body))
        if at + 8 > len(buf):  # (a message damaged before: the word is no longer there)
            continue
        seg = min(int(np.searchsorted(starts, at, side="right")) - 1, nseg - 1)
        w = _struct.unpack_from("<Q", buf, at)[0]
        w = _mutate_word(rng, kind, w, (at - int(starts[seg])) // 8, sizes[seg], sizes)
        _struct.pack_into("<Q", buf, at, w & 0xFFFFFFFFFFFFFFFF)
    return bytes(buf)


def mutants(n, schema, seed, per_base=6, cut=.1, plain=.04):
    """n mutants of `schema` ("struct", "list" or "both") bases; a `plain` share are bases as built"""
    rng = np.random.default_rng([SEED, seed])
    out = []
    while len(out) < n:
        which = schema if schema != "both" else _pick(rng, ["struct", "struct", "list"])
        data, about = (struct_base if which == "struct" else list_base)(rng)
        words = read_words(data, which)
        for _ in range(per_base):
            out.append(data if rng.random() < plain else mutate(rng, data, words, cut=cut))
    return out[:n]


# a handful of fixed cases for Message.init's first statuses (8, 9, 10) and an empty segment 0,
# which no mutation of a body word gives
HEADER_CASES = [b"", b"\0\0\0", _struct.pack("<I", 0xFFFFFFFF), _struct.pack("<I", 0xFFFFFFFF) + bytes(12),
                _struct.pack("<I", 512) + b"\0\0\0", _struct.pack("<I", 512) + bytes(4 * 513), _struct.pack("<I", 0),
                ss.frame([b""]), ss.frame([b"", bytes(16)]), _struct.pack("<I", 600) + bytes(20)]


def with_header_cases(msgs, seed, times=36):
    """msgs and `times` of each header case, shuffled: failing and good lanes share waves"""
    msgs = list(msgs) + HEADER_CASES * times
    order = np.random.default_rng([SEED, seed, 1]).permutation(len(msgs))
    return [msgs[i] for i in order]


# ---------------------------------------------------------------------------
# descriptor tables
# ---------------------------------------------------------------------------
_SCHEMAS = {  # (data words + 1, pointers + 1, the path that resolves) of the widest struct on the way
    "struct": (4, 9, (2, 1, 0)),  # struct_streams.standard's root: 3 data words, 8 pointers
    "elem": (5, 5, (2,)),         # list_streams' elements: up to 4 data words and 4 pointers
    "slot": (2, 2, (0, 0)),       # a pointer-list slot: no data, pointer 0 only
}
_SLICES = {  # the slices the schemas hold: path -> [(kind, pointer index)]
    "struct": {(): [(ss.TEXT, 0), (ss.DATA, 1), (ss.LIST_16, 3), (ss.LIST_32, 4), (ss.LIST_BIT, 5), (ss.LIST_64, 6),
                    (ss.TEXT, 7)], (2,): [(ss.TEXT, 0)], (2, 1, 0): [(ss.TEXT, 0)]},
    "elem": {(): [(ss.TEXT, 0), (ss.DATA, 1)], (2,): [(ss.TEXT, 0)]},
    "slot": {(): [(ss.TEXT, 0), (ss.DATA, 0), (ss.LIST_16, 0)], (0, 0): [(ss.DATA, 0)]},
}


def random_fields(rng, n, schema="struct"):
    """n descriptors of kinds 0..10: data offsets up to one word past the widest data section,
    pointer indices up to one past the widest pointer section, paths of 0..4 steps, a field
    repeating the path of the one before half of the time. So that a table also reads something,
    most paths are a prefix of one the schema has, and half of the slice reads on such a path
    name a slice the schema holds there. schema "slot": the three rules
    capnp_packed_read_elements_batch sets for a pointer list's descriptors."""
    data_words, pointers, good = _SCHEMAS[schema]
    out = []
    for f in range(n):
        if out and rng.random() < .5:
            path = out[-1].path
        elif rng.random() < .7:
            path = good[:int(rng.integers(len(good) + 1))]
        else:
            path = tuple(int(rng.integers(pointers + 1)) for _ in range(int(rng.integers(5))))
        kind = int(rng.integers(11))
        if schema == "slot":
            if path:
                path = (0,) + path[1:]  # a slot has pointer 0 only
            elif kind <= ss.BOOL:
                kind = int(rng.integers(ss.TEXT, 11))  # and no data section
        if kind <= ss.BOOL:
            offset = int(rng.integers(8 * data_words + 1))
        elif path in _SLICES[schema] and rng.random() < .5:
            kind, offset = _pick(rng, _SLICES[schema][path])
        else:
            offset = 0 if schema == "slot" and not path else int(rng.integers(pointers + 1))
        out.append(F(kind, offset, int(rng.integers(8)) if kind == ss.BOOL else 0, path))
    return out


def table_rng(*key):
    return np.random.default_rng([SEED, 77, *key])


def pack_fields(fields):
    """capnp_packed_field records (include/capnp_packed.h): 8 uint32 each"""
    return b"".join(_struct.pack("<8I", f.kind, f.offset, f.bit, len(f.path), *(tuple(f.path) + (0,) * 4)[:4])
                    for f in fields)


# ---------------------------------------------------------------------------
# the batches of test_walk_fuzz.py and test_gpu_walk_fuzz.py, and the models' answers for them
# ---------------------------------------------------------------------------
class Batch:
    """messages laid out back to back between distinct nonzero fillers (struct_streams.layout)"""

    def __init__(self, msgs):
        self.msgs = list(msgs)
        self.buf, self.offs, self.lens = ss.layout(self.msgs, list(range(len(self.msgs))))
        self.n = len(self.msgs)

    def head(self, n):
        return Batch(self.msgs[:n])


def fields_batch():
    """read_fields_batch with the fixed table: about 8,000 mutants of both schemas, shuffled, in
    32 blocks and a partial one"""
    b = Batch(with_header_cases(mutants(8000, "both", seed=1), seed=1))
    assert b.n % 256
    return b


def sweep_batch():
    """the swept tables' batch: 515 units, two blocks and a tail of three (the struct schema's,
    which the random tables are drawn for)"""
    b = Batch(with_header_cases(mutants(495, "struct", seed=3), seed=3, times=2))
    assert b.n == 515
    return b


def sweep_tables():
    """one random table for each n_fields in 1..32: every residue of kSrGroup, in any path order"""
    return [random_fields(table_rng(3, n), n) for n in range(1, 33)]


MAX_COUNT = 1000


def list_batch():
    """the list calls' batch: about 3,000 list-schema mutants (the runs that read no list as what
    it is take the first 1,000). A mutant that claims more than MAX_COUNT elements under any run
    is left out: elem_cap is what bounds such a claim (test_gpu_read_lists.py has that case), and
    here it would only set the size of every output."""
    keep = []
    for m in mutants(3300, "list", seed=2):
        if all(ls.read_list(m, kind, index, [], path, limit=0)[0].count <= MAX_COUNT for kind, index, path in ls.RUNS):
            keep.append(m)
    b = Batch(with_header_cases(keep[:3000], seed=2))
    assert len(keep) >= 3000 and b.n % 256 and 1000 % 256
    return b


def run_tables(run):
    """the tables of one list run: its schema's, and for a run that reads a list as what it is a
    random one as well"""
    kind = run[0]
    tables = [ls.fields_of(kind)]
    if run in ls.RUNS[:4]:
        tables.append(random_fields(table_rng(5, ls.RUNS.index(run)), 13, "elem" if kind == LIST_STRUCT else "slot"))
    return tables


def model_fields(batch, fields):
    """want[i][f] = (status, value, len, count), and per message whether the walk read a word of
    a segment at or past kSrSegs = 4"""
    want, high = [], []
    with recording() as seen:
        for m, off in zip(batch.msgs, batch.offs):
            k = len(seen)
            want.append(ss.read_fields(m, fields, base=off))
            high.append(any(seg >= 4 for seg, _ in seen[k:]))
    return want, high


def model_lists(batch, kind, pointer_index, fields, path=(), cap=None):
    """want[i] = (Head, rows) as test_gpu_read_lists.model gives them, and the same flag"""
    want, high, left = [], [], cap
    with recording() as seen:
        for m, off in zip(batch.msgs, batch.offs):
            k = len(seen)
            head, rows = ls.read_list(m, kind, pointer_index, fields, path, base=off, limit=left)
            if left is not None:
                left = max(0, left - head.count)
            want.append((head, rows))
            high.append(any(seg >= 4 for seg, _ in seen[k:]))
    return want, high


# ---------------------------------------------------------------------------
# the files of the stand-alone program (tests/host_walk/walk_host.cpp: main)
# ---------------------------------------------------------------------------
def write_units(path, msgs):
    with open(path, "wb") as f:
        f.write(_struct.pack("<I", len(msgs)))
        for m in msgs:
            f.write(_struct.pack("<I", len(m)) + m)


def write_tables(path, fields, runs):
    """the read_fields table, then (kind, pointer index, path, fields) per list run"""
    with open(path, "wb") as f:
        f.write(_struct.pack("<I", len(fields)) + pack_fields(fields))
        f.write(_struct.pack("<II", len(runs), ELEM_LIMIT))
        for kind, index, rpath, rfields in runs:
            f.write(_struct.pack("<7I", kind, index, len(rpath), *(tuple(rpath) + (0,) * 4)[:4]))
            f.write(_struct.pack("<I", len(rfields)) + pack_fields(rfields))


def program_runs():
    """the list runs of the stand-alone program: every run with its schema's fields, and the four
    that read a list as what it is with a random table too: 15 in all"""
    runs = [(k, i, p, ls.fields_of(k)) for k, i, p in ls.RUNS]
    for j, (k, i, p) in enumerate(ls.RUNS[:4]):
        runs.append((k, i, p, random_fields(table_rng(9, j), 13, "elem" if k == LIST_STRUCT else "slot")))
    return runs


def read_results(path, n, fields, runs):
    """what the program wrote -> (fields [n][f] of (status, value, len, count), per run a list of
    (head tuple, rows)); slice values are offsets in the message, as the models' with base 0"""
    raw = np.fromfile(path, dtype=np.uint64)
    at = 4 * n * len(fields)
    got_fields = raw[:at].reshape(n, len(fields), 4).tolist()
    got_runs = []
    for kind, index, rpath, rfields in runs:
        nf = len(rfields)
        heads = raw[at:at + 4 * n].copy().view(ls_head_dtype())
        at += 4 * n
        per = []
        for i in range(n):
            rows = int(raw[at])
            per.append((heads[i], raw[at + 1:at + 1 + rows * nf * 4].reshape(rows, nf, 4).tolist()))
            at += 1 + rows * nf * 4
        got_runs.append(per)
    assert at == len(raw)
    return got_fields, got_runs


def ls_head_dtype():
    """capnp_packed_list_head (include/capnp_packed.h), 32 bytes"""
    return np.dtype([("elems_off", "<u8"), ("count", "<u4"), ("segment", "<u4"), ("seg_begin", "<u4"),
                     ("seg_bytes", "<u4"), ("data_words", "<u2"), ("pointer_words", "<u2"), ("status", "<i4")])


def head_tuple(h):
    return tuple(int(h[k]) for k in ("status", "elems_off", "count", "segment", "seg_begin", "seg_bytes",
                                     "data_words", "pointer_words"))


if __name__ == "__main__":  # python walk_fuzz.py UNITS TABLES N: the sanitizer run's input
    import sys
    units, tables, n = sys.argv[1], sys.argv[2], int(sys.argv[3])
    msgs = with_header_cases(mutants(n, "both", seed=4, cut=1 / 7), seed=4, times=3)
    write_units(units, msgs)
    write_tables(tables, ss.FIELDS, program_runs())
    print(f"walk_fuzz: {len(msgs)} units ({sum(len(m) % 8 != 0 for m in msgs)} cut inside a word), "
          f"{len(program_runs())} list runs")
