"""The inputs of tests/test_gpu_small_adversarial.py (tests/small_streams.py), judged by the
reference alone (oracle.unpack / oracle.decoded_size, message.zig:88-191), so that the device
tests cannot pass on a corpus that exercises nothing: the status mix, the expansion, the slot
capacities around the decoded size, where in a lane's 64-B ring every kind of byte falls, the
alignments and slot phases, the class bounds of every unit handed to the small decoders, the
lattice's exact packed lengths, and the group kernel's cut rule on the hand-built sequences."""
import collections

import numpy as np

import oracle
import small_streams as ss


def verdicts(b):
    return [ss.outcome(e, c, len(u), m) for u, e, c, m in zip(b.units, b.exp, b.caps, b.mis)]


def test_main_corpus_mix():
    b = ss.main_corpus()
    n = len(b.units)
    assert 3800 <= n <= 4400
    v = verdicts(b)
    cnt = collections.Counter(st for st, _ in v)
    print("main corpus:", n, "units;", dict(cnt), "kinds", dict(collections.Counter(b.kinds)))
    assert cnt[oracle.OK] >= 0.20 * n
    assert cnt[oracle.UNEXPECTED_EOF] >= 0.20 * n
    assert cnt[oracle.OUT_OF_SPACE] >= 0.05 * n
    assert set(cnt) == {oracle.OK, oracle.UNEXPECTED_EOF, oracle.OUT_OF_SPACE}
    big = sum(1 for st, ln in v if st == oracle.OK and ln >= 4096)
    print("OK units of 4 KiB and more:", big)
    assert big >= 100
    dec = [(len(e.ref), c) for e, c in zip(b.exp, b.caps) if e.st == oracle.OK]
    for d in (0, -1, 1):
        hits = sum(1 for size, c in dec if c == size + d)
        print(f"cap == size {d:+d}:", hits)
        assert hits >= 20, d
    assert sum(1 for c in b.caps if c % 8) >= 0.2 * n  # capacities are not multiples of 8 as a rule
    # every generator kind is there, and every unit of a kind that must fail does
    assert set(b.kinds) == {"random", "records", "cxx", "flip", "cut", "chain"}
    for k, e in zip(b.kinds, b.exp):
        if k in ("records", "cxx", "chain"):
            assert e.st == oracle.OK, k
    assert sum(1 for k, e in zip(b.kinds, b.exp) if k == "cut" and e.st == oracle.UNEXPECTED_EOF) >= 500


def test_main_corpus_coverage():
    b = ss.main_corpus()
    cov = ss.coverage(b.units, b.in_off)
    print("coverage pairs:", len(cov))
    for kind in ss.KINDS:
        assert {o for k, o in cov if k == kind} == set(range(64)), kind
    assert len(cov) == 6 * 64
    pairs = {(int(i) & 15, (int(o) >> 3) & 7) for i, o in zip(b.in_off, b.out_off)}
    assert pairs == {(s, p) for s in range(16) for p in range(8)}
    assert all(m == 0 for m in b.mis) and all(int(o) % 8 == 0 for o in b.out_off)


def test_zero_runs_complete_chunks_and_literals_hold_zero_bytes():
    """What the corpus is for: 00 counts over the whole byte in OK units (a zero run that spans
    and completes 64-B output chunks), and literal words that hold zero bytes."""
    b = ss.main_corpus()
    v = verdicts(b)
    counts, lit_zero = set(), 0
    for u, (st, _) in zip(b.units, v):
        if st != oracle.OK:
            continue
        for pos, t in ss.record_starts(u):
            if t == 0:
                counts.add(u[pos + 1])
            elif t == 0xFF and u[pos + 9]:
                lit_zero += 0 in u[pos + 10:pos + 10 + 8 * u[pos + 9]]
    assert counts == set(range(256))
    assert lit_zero >= 200


def test_small_test_units_are_small():
    """Every unit handed to a small-decoder test has at most 512 packed bytes and a slot of at
    most 8 KiB (the mixed corpus's others and the lattice are not bound: they are there for the
    other classes)."""
    batches = [ss.main_corpus(), *ss.single_units(), *ss.group_batches()[0], ss.refill().tile]
    batches += [ss.partial_wave(n) for n in (63, 64, 65, 257)]
    for b in batches:
        assert all(ss.is_small(b, i) for i in range(len(b.units)))
    m = ss.mixed_corpus()
    small = [i for i in range(len(m.units)) if ss.is_small(m, i)]
    assert [m.units[i] for i in small] == ss.main_corpus().units
    others = [i for i in range(len(m.units)) if not ss.is_small(m, i)]
    assert all(i % 3 == 2 for i in others) and len(others) == len(m.units) // 3
    assert all(len(m.units[i]) >= 600 for i in others)
    assert sum(1 for i in others if ss.pieces(m.units[i], int(m.in_off[i]) & 15) > ss.LONG_PIECES) == 6
    assert {st for st, _ in (v for i, v in enumerate(verdicts(m)) if i in set(others))} == {
        oracle.OK, oracle.UNEXPECTED_EOF, oracle.OUT_OF_SPACE}


def test_partial_waves_hold_the_misaligned_units():
    for n in (63, 64, 65, 257):
        b = ss.partial_wave(n)
        assert len(b.units) == n
        v = verdicts(b)
        assert b.units[1] == b"" and b.mis[1] and int(b.out_off[1]) % 8 and v[1] == (oracle.OK, 0)
        assert b.units[2] and b.mis[2] and int(b.out_off[2]) % 8 and v[2] == (oracle.INVALID_ARGUMENT, 0)
    one, empty_mis, full_mis = ss.single_units()
    assert verdicts(one)[0][0] == oracle.OK and verdicts(one)[0][1] > 0
    assert verdicts(empty_mis) == [(oracle.OK, 0)] and int(empty_mis.out_off[0]) % 8
    assert verdicts(full_mis) == [(oracle.INVALID_ARGUMENT, 0)] and int(full_mis.out_off[0]) % 8


def test_lattice_lengths_and_classes():
    b, claims = ss.lattice()
    want_p = {511, 512, 513} | {B + d for B in ss.MID_EDGES for d in (0, 1)}
    seen = collections.defaultdict(set)
    for i, (u, e, P) in enumerate(zip(b.units, b.exp, claims)):
        assert len(u) == P and e.st == oracle.OK and e.size_st == oracle.OK and e.size == len(e.ref), i
        s = int(b.in_off[i]) & 15
        seen[s].add(P)
        seen[s, "pieces"].add(ss.pieces(u, s))
    for s in range(16):
        assert want_p <= seen[s], s
        assert {ss.LONG_PIECES, ss.LONG_PIECES + 1} <= seen[s, "pieces"], s
        assert max(seen[s, "pieces"]) == ss.LONG_PIECES + 1
    # each stream sits in slots of its exact size, 8 short, 1 over and 1 short; the 8184 / 8192 /
    # 8200 slots hold units on both sides of the small class's packed-length bound
    by_unit = collections.defaultdict(set)
    for u, e, c in zip(b.units, b.exp, b.caps):
        by_unit[u].add(c - len(e.ref))
        by_unit[u, "abs"].add(c)
    for u in b.units:
        if len(u) > 10:
            assert {0, -8, 1, -1} <= by_unit[u]
    for P in (511, 512, 513):
        assert any(len(u) == P and {8184, 8192, 8200} <= by_unit[u, "abs"] for u in b.units), P
    tiny = [(u, c) for u, c in zip(b.units, b.caps) if len(u) <= 10]
    assert collections.Counter(tiny) == {(ss.chain(4), 8192): 16, (ss.chain(4) + b"\0\0", 8200): 16}
    assert all(st == oracle.OK for st, _ in (v for v, u in zip(verdicts(b), b.units) if len(u) <= 10))


def test_group_sequences_cut_where_they_claim():
    batches, where = ss.group_batches()
    assert all(len(b.units) == 4 * ss.GROUP_SEG for b in batches)  # one block, 4 wave ranges of GROUP_SEG

    def groups(name):
        bi, k, s_of = where[name]
        b = batches[bi]
        for i, s in enumerate(s_of):
            assert int(b.in_off[k + i]) & 15 == s
        np_ = [ss.pieces(b.units[k + i], s_of[i]) for i in range(ss.GROUP_SEG)]
        cw = [b.caps[k + i] >> 3 for i in range(ss.GROUP_SEG)]
        return b, k, np_, cw, ss.group_sizes(np_, cw)

    b, k, np_, cw, g = groups("pieces")
    assert np_[:8] == [33] * 8 and g == [7, 9]
    assert sum(np_[:7]) <= ss.GROUP_PIECES < sum(np_[:8]) and sum(cw[:8]) <= ss.GROUP_WORDS  # cut by the pieces
    assert all(st == oracle.OK for st, _ in verdicts(b)[k:k + 8])
    b, k, np_, cw, g = groups("words=1024")
    assert sum(cw[:5]) == ss.GROUP_WORDS and g == [5, 11] and sum(np_) <= ss.GROUP_PIECES
    b, k, np_, cw, g = groups("words>1024")
    assert cw[:2] == [512, 513] and g == [1, 15] and sum(np_) <= ss.GROUP_PIECES
    b, k, np_, cw, g = groups("lone")
    assert cw[1] == 1024 and g == [1, 1, 14]
    assert verdicts(b)[k + 1] == (oracle.OK, 8192)
    b, k, np_, cw, g = groups("odd")
    assert g == [16] and sum(1 for m in b.mis[k:k + 16] if m) == 2
    assert {st for st, _ in verdicts(b)[k:k + 16]} == {oracle.OK, oracle.OUT_OF_SPACE, oracle.INVALID_ARGUMENT}
    for name, at, st in (("first", 0, oracle.UNEXPECTED_EOF), ("middle", 7, oracle.OUT_OF_SPACE),
                         ("last", 15, oracle.UNEXPECTED_EOF)):
        b, k, np_, cw, g = groups(name)
        v = verdicts(b)[k:k + 16]
        assert g == [16] and v[at][0] == st, name
        assert all(x[0] == oracle.OK for i, x in enumerate(v) if i != at), name


def test_refill_batch():
    r = ss.refill()
    t = r.tile
    assert r.n == 1 << 20 and len(t.units) == ss.REFILL_TILE and len(set(zip(t.units, t.caps, t.mis))) > 600
    v = verdicts(t)
    heavy, light = range(ss.REFILL_HEAVY), range(ss.REFILL_HEAVY, ss.REFILL_TILE)
    assert all(t.caps[i] >= 4096 for i in heavy)
    assert sum(1 for i in heavy if v[i] == (oracle.OK, 8192)) >= 4
    assert sum(1 for i in heavy if v[i][0] == oracle.OUT_OF_SPACE) == 4
    assert np.mean([t.caps[i] for i in light]) <= 128
    assert sum(1 for i in light if len(t.units[i]) <= 2) >= 1500
    cnt = collections.Counter(v[i][0] for i in light)
    print("refill tile light units:", dict(cnt), "stride", r.stride)
    assert set(cnt) == {oracle.OK, oracle.UNEXPECTED_EOF, oracle.OUT_OF_SPACE, oracle.INVALID_ARGUMENT}
    assert min(cnt.values()) >= 40 and sum(1 for i in light if len(t.units[i]) == 0) >= 100
    # every unit once; every 64 consecutive batch positions: one expander among 63 light units of
    # the same tile, failing units of every status beside OK ones
    assert np.array_equal(np.sort(r.order), np.arange(r.n))
    j = (r.order % ss.REFILL_TILE).reshape(-1, 64)
    assert ((j < ss.REFILL_HEAVY).sum(axis=1) == 1).all()
    assert ((r.order // ss.REFILL_TILE).reshape(-1, 64) == (r.order // ss.REFILL_TILE).reshape(-1, 64)[:, :1]).all()
    st_of = np.array([s for s, _ in v])
    bad = st_of[j] != oracle.OK
    assert (bad.sum(axis=1) >= 4).all() and ((~bad).sum(axis=1) >= 16).all()
    # the slots of different units never overlap, canaries included, and device memory stays small
    assert r.stride >= t.out_end + ss.BACK and r.stride * (r.n // ss.REFILL_TILE) < (1 << 30) * 3 // 4
    assert (np.diff(np.sort(r.out_off)) >= ss.FRONT + ss.BACK).all()
    assert r.care_strict.all() and r.image[~r.care_prefix].tolist().count(ss.SENT) == int((~r.care_prefix).sum())
