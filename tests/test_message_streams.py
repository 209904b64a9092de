"""tests/message_streams.py judged without a device: the batches' layout (poison, placements,
slots), the routes each builder reaches (route_of restates encode_message_kernel's routing), the
two references against the oracle's decoder, the corpus' teeth (runs that cross a piece edge change
the bytes) and `check` itself against fabricated device results."""
import collections

import numpy as np
import pytest

import message_streams as ms
import oracle
import pyref_cxx

ALL_PAIRS = {(a, c) for a in ms.ROUTES for c in ms.ROUTES}


def all_batches():
    return [(name, f()) for name, f in ms.BUILDERS.items()] + [("wave_pairs", b) for b in ms.wave_pairs()]


def test_layout():
    for name, b in all_batches():
        n = len(b.msgs)
        assert b.pool.size % 8 == 0 and len(b.entries) == len(b.routes) == n
        words = b.pool.reshape(-1, 8)
        is_poison = (words == np.frombuffer(ms.POISON, dtype=np.uint8)).all(axis=1)
        seg_word = np.zeros(len(words), dtype=bool)
        for m, ent, f, c in zip(b.msgs, b.entries, b.first, b.count):
            assert c == len(m.segs)
            listed = list(zip(b.seg_off[f:f + c].tolist(), b.seg_len[f:f + c].tolist()))
            if c == 0:  # seg_first at a poison entry: a valid index whose use would show
                assert 0 <= f < len(b.seg_off) and b.seg_len[f] == 16 and is_poison[b.seg_off[f] // 8]
                continue
            assert listed == ent, (name, m.kind)
            for s, (ad, ln) in enumerate(ent):
                assert 8 <= ad and ad + ln + 8 <= b.pool.size, (name, m.kind)  # inside the pool, never null
                if m.bad and m.bad[:2] in (("len", s), ("ptr", s)):
                    assert (ad % 8, ln % 8) in ((0, 4), (4, 0))
                    ad, ln = ad - ad % 8, ln - ln % 8
                assert b.pool[ad:ad + ln].tobytes() == m.segs[s], (name, m.kind, s)
                seg_word[ad // 8:(ad + ln) // 8] = True
                if ln == 0 and not m.place[0:3] == "e2e" and not (m.place == "last_broken" and s < c - 1):
                    assert is_poison[ad // 8], (name, m.kind, s)  # an empty segment points at poison
        assert is_poison[~seg_word].all(), name  # whatever is no segment is poison
        assert not is_poison[seg_word].any(), name  # and no message holds a poison word
        assert is_poison[:ms.POOL_PAD // 8].all() and is_poison[-(ms.POOL_PAD // 8):].all()
        for d in ms.DIALECTS:
            sl = b.slots[d]
            ends = sl.out_off + np.array(sl.caps)
            assert sl.out_off[0] >= ms.FRONT and (sl.out_off[1:] - ends[:-1] >= ms.FRONT).all()
            assert sl.out_end == ends[-1] + ms.BACK


def test_empty_segments_break_links_outside_the_end_to_end_placements():
    """Two empty neighbours at one address would keep ptr + len == next ptr."""
    b = ms.empty_edges()
    for m, ent, r in zip(b.msgs, b.entries, b.routes):
        if m.place == "shuffle" and len(m.segs) <= ms.ONE_SEGS and ms.framed_words(m) <= ms.TILE:
            assert r == "gather", m.kind


@pytest.mark.parametrize("name", list(ms.BUILDERS))
def test_routes_reached(name):
    b = ms.BUILDERS[name]()
    got = collections.Counter(b.routes)
    assert set(got) >= ms.AIMED[name], (name, got)
    for d in ms.DIALECTS:
        assert ms.statuses(b, d) == ms.STATUSES[name], (name, d)
    assert max(ms.framed_words(m) for m in b.msgs) <= 4 * ms.TILE


def test_route_restates_the_kernel_rules():
    one = ms.letters("C")
    assert ms.route(ms.msg([], "")) == "e2e"
    assert ms.route(ms.msg([one] * 64, "", "e2e8")) == "e2e"
    assert ms.route(ms.msg([one] * 64, "", "shuffle")) == "gather"
    assert ms.route(ms.msg([one] * 64, "", "adj_rev")) == "gather"
    assert ms.route(ms.msg([one] * 64, "", "last_broken")) == "gather"
    assert ms.route(ms.msg([one] * 65, "", "e2e0")) == "tiled"
    assert ms.route(ms.msg([one] * 512, "", "e2e0")) == "tiled"
    assert ms.route(ms.msg([one] * 513, "", "e2e0", ("count",))) == "arg"
    assert ms.route(ms.msg([one * 511], "")) == "e2e" and ms.route(ms.msg([one * 512], "")) == "tiled"
    assert ms.route(ms.msg([one, one * 509], "")) == "e2e" and ms.route(ms.msg([one, one * 510], "")) == "tiled"
    assert ms.route(ms.msg([one * 513, b""], "", "shuffle")) == "tiled"
    assert ms.route(ms.msg([one, one], "", "e2e0", ("len", 1))) == "arg"
    assert ms.route(ms.msg([one, one], "", "shuffle", ("ptr", 0))) == "arg"
    assert [ms.header_words(c) for c in (1, 2, 3, 4, 63, 64, 512)] == [1, 2, 2, 3, 32, 33, 257]


def test_wave_pairs_cover_every_ordered_pair():
    bs = ms.wave_pairs()
    assert set(ms.wave_pair_routes(bs[0])) == ALL_PAIRS
    assert {len(b.msgs) for b in bs} >= {1, 2, 3, 7, 8, 9, 15, 16, 17}
    seen = set()
    for b in bs[1:]:
        seen |= set(ms.wave_pair_routes(b))
    assert len(seen) >= 12  # the small batches walk through the pairs too


def test_count_lattice_coverage():
    b = ms.count_lattice()
    by = collections.defaultdict(set)
    for m, r in zip(b.msgs, b.routes):
        by[len(m.segs)].add(r)
    assert set(by) == set(ms.COUNTS) and {0, 63, 64, 65, 66, 511, 512} <= set(by)
    for c, rs in by.items():
        assert rs == ({"tiled"} if c > 64 else {"e2e"} if c <= 1 else {"e2e", "gather"}), (c, rs)
    assert {ms.header_words(max(c, 1)) % 2 for c in by} == {0, 1}
    assert max(ms.header_words(c) for c in by) == 257
    # every segment size at every parity of the header entry that holds it
    assert {(len(s) // 8, k % 2) for m in b.msgs for k, s in enumerate(m.segs)} == {(w, p) for w in range(4) for p in (0, 1)}
    # both base phases of the end-to-end run and all four letters
    phases = {e[0][0] % 16 for m, e, r in zip(b.msgs, b.entries, b.routes) if r == "e2e" and m.segs}
    assert phases == {0, 8}
    assert {m.kind.split()[-1] for m in b.msgs} == set(ms.LATTICE_PATTERNS)


def test_empty_edges_coverage():
    b = ms.empty_edges()
    shapes = collections.Counter()
    for m, r in zip(b.msgs, b.routes):
        sizes = [len(s) // 8 for s in m.segs]
        runs = max(len(z) for z in "".join("e" if w == 0 else "x" for w in sizes).split("x"))
        for tag, hit in (("first", sizes[0] == 0), ("last", sizes[-1] == 0), ("two", runs == 2), ("more", runs >= 3),
                         ("all", sum(sizes) == 0), ("one", sum(1 for w in sizes if w) == 1)):
            shapes[(r, tag)] += hit
    for r in ("gather", "tiled"):
        for tag in ("first", "last", "two", "more", "one"):
            assert shapes[(r, tag)] > 0, (r, tag)
    assert shapes[("gather", "all")] > 0 and shapes[("tiled", "all")] > 0  # 65 empty segments are tiled
    assert {len(m.segs) for m, r in zip(b.msgs, b.routes) if r == "gather"} == set(range(2, 65))


def test_tile_limit_coverage():
    b = ms.tile_limit()
    got = {(len(m.segs), ms.framed_words(m), r) for m, r in zip(b.msgs, b.routes)}
    for c in ms.LIMIT_COUNTS:
        for w in ms.LIMIT_WORDS:
            want = {"tiled"} if w > ms.TILE else {"e2e"} if c == 1 else {"e2e", "gather"}
            assert {r for cc, ww, r in got if (cc, ww) == (c, w)} >= want, (c, w)
    sizes = {len(s) // 8 for m in b.msgs for s in m.segs}
    assert {512, 513} <= sizes
    edges = collections.Counter()
    for m in b.msgs:
        fw = ms.framed_words(m)
        if fw in (1024, 1536) and len(m.segs) == 3:
            edges[(fw, 2 + len(m.segs[0]) // 8)] += 1
    assert set(edges) == {(1024, 511), (1024, 512), (1024, 513), (1536, 511), (1536, 512), (1536, 513),
                          (1536, 1023), (1536, 1024), (1536, 1025)}


def test_references_decode_to_the_frame():
    """Both references are packed forms of the same framed bytes: the oracle's decoder
    (message.zig:88-145) gives pyref.frame(segs) back from each, and both fit encode_bound of the framed bytes (the C++
    bytes of a message can be the longer ones: a zero run cut at a piece edge takes two records)."""
    seen = set()
    for name, b in all_batches():
        for m, r in zip(b.msgs, b.routes):
            if r == "arg" or m.segs in seen:
                continue
            seen.add(m.segs)
            f = ms.frame_of(m)
            z, c = ms.reference(m.segs, "zig"), ms.reference(m.segs, "cxx")
            assert oracle.unpack(z) == (oracle.OK, f), (name, m.kind)
            assert oracle.unpack(c) == (oracle.OK, f), (name, m.kind)
            assert max(len(c), len(z)) <= ms.encode_bound(len(f))
    assert len(seen) > 3000


def test_run_edges_have_teeth():
    """Per edge kind: messages whose Zig bytes differ from the table and the segments packed on
    their own (an encoder that restarts a run at a piece edge fails on them), and whose C++ bytes
    differ from the frame packed as one piece (one that does not restart fails)."""
    zig, cxx, breakers = collections.Counter(), collections.Counter(), collections.defaultdict(set)
    for edge, m in ms.run_edge_messages():
        zig[edge] += ms.reference(m.segs, "zig") != ms.piecewise_zig(m.segs)
        cxx[edge] += ms.reference(m.segs, "cxx") != pyref_cxx.pack_buffer(ms.frame_of(m))
        breakers[edge] |= set("ABCZ") & set(m.kind.split())
    for edge in ("hdr", "seg", "tile"):
        assert zig[edge] >= 24 and cxx[edge] >= 24, (edge, zig, cxx)
        assert breakers[edge] == set("ABCZ")
    assert zig["tail"] > 0
    b = ms.run_edges()
    per = collections.Counter((e, r) for (e, _), r in zip(ms.run_edge_messages(), b.routes))
    assert per[("hdr", "e2e")] and per[("hdr", "gather")] and per[("seg", "e2e")] and per[("seg", "gather")]
    assert per[("tile", "tiled")] and per[("tail", "tiled")]
    # runs of exactly 255, 256 and 257 words in the Zig bytes
    import encode_streams as es
    runs = collections.Counter()
    for (e, m) in ms.run_edge_messages():
        zr, lr = es.runs(ms.reference(m.segs, "zig"))
        for r in zr + lr:
            runs[r] += 1
    assert runs[255] and runs[256] and runs[257]


def test_pairs_coverage():
    b = ms.pairs()
    assert {m.place for m in b.msgs if not isinstance(m.place, tuple)} == set(ms.PAIR_PLACES)
    shared = [m for m in b.msgs if isinstance(m.place, tuple)]
    assert len(shared) >= 20
    for m in shared:
        assert b.entries[m.place[1]] == b.entries[b.msgs.index(m)]
    twice = sum(len(set(e)) < len(e) for m, e in zip(b.msgs, b.entries) if m.place == "dedup")
    assert twice >= 10  # the same bytes listed twice in one message
    ones = [m for m in b.msgs if m.segs and all(len(s) == 8 for s in m.segs)]
    assert {len(m.segs) for m in ones} == set(ms.PAIR_COUNTS)
    alt = {(len(m.segs[0]) // 8, ms.header_words(len(m.segs)) % 2) for m in b.msgs
           if {len(s) for s in m.segs} == {8, 16}}
    assert alt == {(1, 0), (1, 1), (2, 0), (2, 1)}


def test_cap_walk_coverage():
    b = ms.cap_walk()
    for d in ms.DIALECTS:
        sl, ex = b.slots[d], b.exp[d]
        per = collections.defaultdict(set)
        for m, r, c, e in zip(b.msgs, b.routes, sl.caps, ex):
            per[(m.kind, r)].add(c - e.need)
        assert {r for _, r in per} == set(ms.ROUTES)
        for (kind, r), deltas in per.items():
            if r != "arg":
                assert {-1, 0, 1} <= deltas, (d, kind)
                need = next(e.need for m, e in zip(b.msgs, ex) if m.kind == kind)
                assert need > 64 or {-need + c for c in range(need + 2)} <= deltas, (d, kind)
    assert 18 <= len({m.kind for m in b.msgs}) <= 30


def test_errors_sit_between_valid_neighbours():
    b = ms.errors()
    n = len(b.msgs)
    spots = collections.Counter()
    for i, (m, r) in enumerate(zip(b.msgs, b.routes)):
        if r != "arg":
            continue
        assert 0 < i < n - 1 and b.routes[i - 1] != "arg" and b.routes[i + 1] != "arg"
        spots[(m.bad[0], len(m.segs), m.bad[1] if len(m.bad) > 1 else None, i % 2)] += 1
    for what in ("len", "ptr"):
        for c, s in ms.ERROR_SPOTS:
            assert spots[(what, c, s, 0)] and spots[(what, c, s, 1)], (what, c, s)
    assert spots[("count", 513, None, 0)] and spots[("count", 513, None, 1)]
    assert {(300, 299), (64, 63), (65, 64)} <= set(ms.ERROR_SPOTS)


def test_random_mixed_coverage():
    b = ms.random_mixed()
    assert 1500 <= len(b.msgs) <= 5000
    assert {m.place for m in b.msgs} == set(ms.PLACEMENTS)
    for d in ms.DIALECTS:
        sl, ex = b.slots[d], b.exp[d]
        assert {int(o) & 15 for o in sl.out_off} == set(range(16))
        delta = np.array(sl.caps) - np.array([e.need for e in ex])
        assert (delta == 0).sum() > 500 and 20 < (delta < 0).sum() < 200 and (delta > 0).sum() > 500


# ---- check against fabricated device results --------------------------------------------------------

def ideal(b, dialect):
    """What a correct device leaves: (out, out_len, status)."""
    sl, ex = b.slots[dialect], b.exp[dialect]
    out = np.full(ms.output_bytes(b, dialect), ms.SENT, dtype=np.uint8)
    out_len = np.zeros(len(b.msgs), dtype=np.int64)
    status = np.zeros(len(b.msgs), dtype=np.int32)
    for i, (e, c) in enumerate(zip(ex, sl.caps)):
        status[i], out_len[i] = ms.outcome(e, c)
        o = int(sl.out_off[i])
        if status[i] == oracle.OK:
            out[o:o + e.need] = np.frombuffer(e.ref, dtype=np.uint8)
        elif status[i] == oracle.OUT_OF_SPACE:
            out[o:o + c] = 0xC3  # unspecified: anything
    return out, out_len, status


@pytest.mark.parametrize("dialect", ms.DIALECTS)
def test_check_rejects_fabricated_faults(dialect):
    b = ms.cap_walk()
    sl, ex = b.slots[dialect], b.exp[dialect]
    out, out_len, status = ideal(b, dialect)
    assert ms.check(b, out, out_len, status, dialect) == ms.STATUSES["cap_walk"]
    sizes = np.array([e.need for e in ex]), np.array([e.st for e in ex], dtype=np.int32)
    ms.check(b, None, *sizes, dialect)
    ok = [i for i in range(len(b.msgs)) if status[i] == oracle.OK and 0 < ex[i].need < sl.caps[i]]
    err = [i for i in range(len(b.msgs)) if status[i] == oracle.INVALID_ARGUMENT and sl.caps[i] > 0]
    i, j = ok[len(ok) // 2], err[-1]
    o, oj = int(sl.out_off[i]), int(sl.out_off[j])

    def rejected(where, at=None, **kw):
        o2, l2, s2 = out.copy(), out_len.copy(), status.copy()
        if at is not None:
            o2[at] ^= 0x10
        for name, (k, v) in kw.items():
            {"length": l2, "stat": s2}[name][k] = v
        with pytest.raises(AssertionError) as info:
            ms.check(b, o2, l2, s2, dialect)
        assert where in str(info.value), (where, str(info.value))

    rejected("in the packed bytes", o + ex[i].need // 2)   # one byte flipped in the packed bytes
    rejected("in the packed bytes", o + ex[i].need - 1)
    rejected("in [out_len, cap)", o + ex[i].need)          # one byte written in [out_len, cap)
    rejected("in [out_len, cap)", o + sl.caps[i] - 1)
    rejected("before the slot", o - 1)                     # one byte before a slot
    rejected("before the slot", int(sl.out_off[0]) - ms.FRONT)
    rejected("past cap", o + sl.caps[i])                   # one byte past cap
    rejected("past cap", out.size - 1)
    rejected("", oj)                                       # an error slot touched
    rejected("", oj + sl.caps[j] - 1)
    rejected("status", stat=(i, -1))                       # an entry left at -1
    rejected("out_len", length=(i, -1))
    rejected("status", stat=(j, 0x7FFF0001))               # the first pass's mark left behind
    rejected("out_len", length=(i, ex[i].need + 1))
    tight = next(k for k in range(len(b.msgs)) if status[k] == oracle.OUT_OF_SPACE and sl.caps[k] > 0)
    rejected("past cap", int(sl.out_off[tight]) + sl.caps[tight])  # an OUT_OF_SPACE slot is free, its edge is not
    with pytest.raises(AssertionError):
        s2 = sizes[0].copy()
        s2[i] -= 1
        ms.check(b, None, s2, sizes[1], dialect)


def test_init_frames():
    frames = ms.init_frames()
    rcs = collections.Counter(oracle.message_init(f)[0] for f in frames)
    assert set(rcs) == {0, -1, -2, -3, -4} and rcs[-4] > 200
    counts = {len(oracle.message_init(f)[1]) for f in frames}
    assert {1, 2, 3, 63, 64, 65, 511, 512} <= counts
    cut_in_a_segment = 0
    for f in frames:
        rc, table = oracle.message_init(f)
        if rc == 0:
            assert ms.header_entries(f) == [(int(a), int(c)) for a, c in table]
        else:
            cut_in_a_segment += len(ms.header_entries(f)) > 1
    assert cut_in_a_segment > 100  # TRUNCATED_MESSAGE after entries that fit
