"""The inputs of tests/test_gpu_encode_adversarial.py (tests/encode_streams.py), judged by the
reference alone (oracle.pack, message.zig:200-271), so that the device tests cannot pass on a
corpus that exercises nothing: the reference itself against two other implementations, where in
a 16-B output chunk every kind of byte falls, the run lengths on the 256-word cap, the classes
and bin edges, the tile-bound cases the long path's lookback and lookahead need, the capacity
walks, the order of the small list, the statuses, the layout and the sizes."""
import collections

import numpy as np
import pytest

import encode_streams as es
import oracle
import pyref
import pyref_cxx

ALL = list(es.BUILDERS) + [f"mixed-{k}" for k in es.MIXED]


def batch(name):
    if name.startswith("mixed-"):
        k = name[6:]
        return es.mixed_batch(int(k) if k.isdigit() else k)
    return es.BUILDERS[name]()


def total_coverage():
    cov = collections.Counter()
    for name in es.BUILDERS:
        cov.update(es.coverage(batch(name)))
    return cov


# ---- the reference ------------------------------------------------------------------------

def test_word_maker_is_pyref_cxx_words():
    for spec in ("A", "C*3 A Z*2 B*4 A*3", "Z*9 C B A*17 Z", "B*300"):
        assert es.words(spec) == pyref_cxx.words(spec)
    a = np.frombuffer(es.letters("ABCZ" * 64), dtype=np.uint8).reshape(-1, 8)
    assert ((a == 0).sum(axis=1).reshape(-1, 4) == [0, 1, 2, 8]).all()


@pytest.mark.parametrize("name", ALL)
def test_oracle_is_pyref_on_a_sample(name):
    """pyref.pack (plain Python) on a strided sample of the valid units, at most 400 KB a builder."""
    b = batch(name)
    valid = [i for i, e in enumerate(b.exp) if e.st == oracle.OK]
    budget, done = 400_000, 0
    for i in valid[::max(1, len(valid) // 97)]:
        if len(b.units[i]) > budget:
            continue
        budget -= len(b.units[i])
        assert pyref.pack(b.units[i]) == b.exp[i].ref, es.describe(b, i)
        done += 1
    assert done >= min(len(valid), 40)


@pytest.mark.parametrize("name", ALL)
def test_oracle_is_fast_pack_on_all(name):
    b = batch(name)
    valid = [i for i, e in enumerate(b.exp) if e.st == oracle.OK]
    lens = np.array([len(b.units[i]) for i in valid], dtype=np.uint64)
    in_off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    out_off = np.concatenate(([0], np.cumsum([es.encode_bound(int(n)) for n in lens]))).astype(np.uint64)
    inp = np.frombuffer(b"".join(b.units[i] for i in valid) + bytes(16), dtype=np.uint8)
    out, out_len, status = oracle.fast_pack_batch(inp, in_off, out_off)
    assert (status == oracle.OK).all()
    for j, i in enumerate(valid):
        o = int(out_off[j])
        e = b.exp[i]
        assert int(out_len[j]) == e.need and out[o:o + e.need].tobytes() == e.ref, es.describe(b, i)


def test_error_verdicts():
    assert oracle.pack(b"12345")[0] == oracle.INVALID_MESSAGE_SIZE
    assert es.verdict(bytes(8), 3) == es.Exp(oracle.INVALID_ARGUMENT, 0, b"")
    assert es.verdict(bytes(5), 3).st == oracle.INVALID_ARGUMENT  # both at once: the alignment first
    assert es.outcome(es.verdict(bytes(8)), 1) == (oracle.OUT_OF_SPACE, 2)
    assert es.outcome(es.verdict(bytes(8)), 2) == (oracle.OK, 2)
    assert es.outcome(es.verdict(b""), 0) == (oracle.OK, 0)


# ---- the coverage table ---------------------------------------------------------------------

def test_small_lattice_shape():
    shapes = es.lattice_shapes()
    assert len(shapes) == 804 == 67 * len(es.PATTERNS)
    assert {n for _, n, _ in shapes} == set(range(67))
    b = es.small_lattice()
    assert len(b.units) == 804 * 32 + 8 * es.EXTREMES
    seen = {(u, int(i) & 15, int(o) & 15) for u, i, o in zip(b.units, b.in_off, b.out_off)}
    for _, n, u in shapes:
        for inph in (0, 8):
            assert all((u, inph, slot) in seen for slot in range(16)), n
    # the patterns are what their names say
    zb = lambda u: (np.frombuffer(u, dtype=np.uint8).reshape(-1, 8) == 0).sum(axis=1).tolist()  # noqa: E731
    by = {(name, n): zb(u) for name, n, u in shapes if n == 10}
    assert by[("A", 10)] == [0] * 10 and by[("B", 10)] == [1] * 10 and by[("C", 10)] == [2] * 10
    assert by[("Z", 10)] == [8] * 10 and by[("ZA", 10)] == [8, 0] * 5 and by[("AC", 10)] == [0, 2] * 5
    assert by[("CA*", 10)] == [2] + [0] * 9 and by[("A*Z", 10)] == [0] * 9 + [8] and by[("Z*A", 10)] == [8] * 9 + [0]
    assert by[("AAZZ", 10)] == [0, 0, 8, 8, 0, 0, 8, 8, 0, 0] and by[("CAAAB", 10)] == [2, 0, 0, 0, 1] * 2
    assert by[("ZZZC", 10)] == [8, 8, 8, 2, 8, 8, 8, 2, 8, 8]


def test_chunk_positions_in_the_small_lattice():
    """encode_stream_kernel's output assembly: a tag, a literal word's first byte and a literal
    run's count byte at every position of a 16-B chunk, and count bytes patched in the chunk
    still in registers and in one already stored."""
    cov = es.coverage(es.small_lattice())
    for kind in ("tag", "lit", "count"):
        got = {k: cov[(kind, k)] for k in range(16)}
        print(kind, got)
        assert all(got.values()), kind
    print("count bytes: run ends in the same chunk", cov["same"], "in a later chunk", cov["later"])
    assert cov["same"] >= 10000 and cov["later"] >= 10000


def test_chunk_positions_in_every_builder():
    for name in es.BUILDERS:
        cov = es.coverage(batch(name))
        for kind in ("tag", "lit", "count"):
            assert all(cov[(kind, k)] for k in range(16)), (name, kind)
        assert cov["same"] and cov["later"], name


def test_run_lengths_on_the_cap():
    cov = total_coverage()
    for kind in ("zrun", "lrun"):
        for r in (1, 255, 256, 257):
            print(kind, r, cov[(kind, r)])
            assert cov[(kind, r)], (kind, r)
    # and on their own in the builders made for them
    for name in ("run_edges", "tile_edges"):
        cov = es.coverage(batch(name))
        assert all(cov[(kind, r)] for kind in ("zrun", "lrun") for r in (255, 256, 257)), name


def test_runs_walk():
    p = oracle.pack(es.words("Z*257 A*257 C Z A"))[1]
    assert es.runs(p) == ([257, 1], [257, 1])
    p = oracle.pack(es.words("Z*256 C A*256 B Z*512 A*511"))[1]
    assert es.runs(p) == ([256, 512], [256, 511])


def classes(b):
    return collections.Counter(es.unit_class(u, m) for u, m in zip(b.units, b.mis))


def test_classes_and_bin_edges():
    b = es.class_edges()
    cl = classes(b)
    print("class_edges:", dict(cl))
    assert all(cl[k] for k in (0, 1, 2, 3, "mid", "long", "huge"))
    assert es.unit_class(bytes(8 * 8192)) == "long" and es.unit_class(bytes(8 * 8193)) == "huge"
    valid = {(len(u) // 8, int(o) & 15) for u, m, o in zip(b.units, b.mis, b.in_off) if not m and len(u) % 8 == 0}
    for nw in es.CLASS_LENGTHS:
        for inph in (0, 8):
            assert (nw, inph) in valid, (nw, inph)
    for edge in (0, 7, 8, 9, 16, 17, 32, 33, 64, 65, 66, 512, 513, 8192, 8193):
        assert edge in es.CLASS_LENGTHS
    # every density at every length and phase
    assert sum(1 for u, m in zip(b.units, b.mis) if not m and len(u) % 8 == 0) == len(es.CLASS_LENGTHS) * 2 * 5
    # the error units: each kind in the small, the mid and the long range; the empty one
    errs = collections.Counter()
    for u, m in zip(b.units, b.mis):
        if m or len(u) % 8:
            rng_ = "small" if len(u) // 8 <= 64 else "mid" if len(u) // 8 <= 512 else "long"
            errs[(bool(m), bool(len(u) % 8), rng_ if u else "empty")] += 1
    assert errs == {(mm, sz, r): 1 for mm, sz in ((False, True), (True, False), (True, True))
                    for r in ("small", "mid", "long")} | {(True, False, "empty"): 1}
    # the small lattice reaches every bin edge too, and 64 words at 8 mod 16 (65 ring words)
    lat = es.small_lattice()
    got = {(len(u) // 8, int(o) & 15) for u, o in zip(lat.units, lat.in_off)}
    assert all((nw, inph) in got for nw in range(67) for inph in (0, 8))
    assert set(classes(lat)) == {0, 1, 2, 3, "mid"}


def test_extreme_waves_in_the_small_lattice():
    """Whole waves of the small list (64 entries from a multiple of 64) that alternate all-A and
    all-Z units of one bin."""
    b = es.small_lattice()
    order = es.small_list(b)
    kind = ["A" if "extreme" in b.kinds[i] and b.kinds[i][0] == "A" else
            "Z" if "extreme" in b.kinds[i] else "-" for i in order]
    tops = set()
    for w0 in range(0, len(order) - 63, 64):
        k = "".join(kind[w0:w0 + 64])
        if k in ("AZ" * 32, "ZA" * 32):
            lens = {len(b.units[i]) for i in order[w0:w0 + 64]}
            if len(lens) == 1:  # not a window across two bins' stretches
                tops.add(lens.pop() // 8)
    assert tops == set(es.BIN_TOPS)


def test_run_edges_placement():
    b = es.run_edges()
    starts, ends = collections.defaultdict(set), collections.defaultdict(set)
    followers = collections.defaultdict(set)
    for k in b.kinds:
        head, run, br, _ = k.split()
        h, (L, N) = int(head[2:]), (run[0], int(run[2:]))
        starts[(L, N)].add(h)
        ends[(L, N)].add(h + N)
        followers[(L, N, h)].add(br)
    assert set(starts) == {(L, N) for L in "ZA" for N in es.RUN_LENGTHS}
    for key in starts:
        assert set(range(0, 513, 8)) <= starts[key], key                   # every lane boundary of a tile
        assert {e % 512 for e in ends[key] if e % 8 == 0} == set(range(0, 512, 8)), key
        for x in es.RUN_SIDES:
            assert {x - 1, x, x + 1} <= starts[key], (key, x)
            if x + 1 >= key[1]:
                assert {e for e in (x - 1, x, x + 1) if e >= key[1]} <= ends[key], (key, x)
    assert all(f == set("ABCZ") for f in followers.values())
    cl = classes(b)
    assert cl["mid"] > 500 and cl["long"] > 500
    # the kinds describe the units
    for i in range(0, len(b.units), 501):
        assert b.units[i] == es.words(b.kinds[i])


def test_tile_edges_cases():
    b = es.tile_edges()
    assert len(b.units) == len(es.TILE_HEADS) * 2 * len(es.TILE_RUNS) * 4
    assert es.in_bytes(b) < 8 << 20
    tiles = collections.Counter()
    back, ahead, on_end = set(), set(), 0
    for i, k in enumerate(b.kinds):
        s = es.spell(k)
        assert b.units[i] == es.letters(s)
        nw = len(s)
        tiles[(nw + es.TILE - 1) // es.TILE] += 1
        on_end += nw % es.TILE == 0
        for L, a, e in es.run_spans(s):
            for t in range(es.TILE, nw, es.TILE):   # t: a tile start, and the end of the tile before
                if a < t < e:
                    back.add((L, "over 512" if t - a > 512 else "over 256" if t - a > 256 else "near"))
                if a < t <= e and e < nw:
                    ahead.add((L, e - t))
    print("tiles per unit:", dict(tiles), "units ending on a tile end:", on_end)
    assert set(tiles) == {2, 3, 4}
    assert on_end >= 50
    for L in "ZA":
        assert {(L, "near"), (L, "over 256"), (L, "over 512")} <= back   # second and third lookback pass
        assert {(L, 255), (L, 256), (L, 257)} <= ahead                    # the lookahead's la == 256 arm


def test_cap_cuts_walks():
    b = es.cap_cuts()
    caps_of = collections.defaultdict(set)
    for u, k, c, o in zip(b.units, b.kinds, b.caps, b.out_off):
        caps_of[(u, k, int(o) & 15)].add(c)
    cp0, cp1, cp2 = 0, 0, 0
    phases = collections.defaultdict(set)
    for (u, k, ph), caps in caps_of.items():
        need = es.verdict(u).need
        if k.startswith("small"):
            assert caps == set(range(need + 2)), k
            phases[u].add(ph)
            lc = [cp for cp, _ in es.literal_counts(es.verdict(u).ref)]
            cp0 += any(cp in caps for cp in lc)
            cp1 += any(cp + 1 in caps for cp in lc)
            cp2 += any(cp + 2 in caps for cp in lc)
        elif k.startswith("mid"):
            assert {0, 1, need - 1, need, need + 1} <= caps and len(caps) >= 5 + (need - 2) // 97 - 1, k
            assert 64 < len(u) // 8 <= 512
        elif k.startswith("long C x"):
            assert need == 7 * (len(u) // 8) and len(u) // 8 > 512
            assert {3583, 3584, 3585, 7167, 7168, 7169, need - 1, need} <= caps, k
        else:
            assert k.startswith("long ") and len(u) // 8 > 512 and {need - 1, need} <= caps and len(caps) > 20, k
            assert any(a < 512 < e or a < 1024 < e for _, a, e in es.run_spans(es.spell(k[5:])))
    print("small units walked:", len(phases), "with a literal run's cpos / +1 / +2 as a capacity:", cp0, cp1, cp2)
    assert len(es.CUT_SMALL) >= 40 and len(phases) >= 38 and all(p == set(es.CUT_PHASES) for p in phases.values())
    assert cp0 and cp1 and cp2
    assert sum(1 for k in caps_of if k[1].startswith("mid")) == 12
    assert es.statuses(b) == {oracle.OK, oracle.OUT_OF_SPACE}


def test_mixed_batches():
    for n in es.SMALL_ONLY:
        b = es.mixed_batch(n)
        assert len(b.units) == n and set(classes(b)) <= {0, 1, 2, 3}
    b = es.mixed_batch("minority")
    cl = classes(b)
    print("minority:", dict(cl))
    small = sum(cl[k] for k in range(4))
    assert 0 < small < cl["mid"] and cl["long"] >= 10 and cl["huge"] == 1
    order = es.small_list(b)
    assert order != list(range(len(order))) and all(cl[k] for k in range(4))
    b = es.mixed_batch("blocks3")
    assert len(b.units) == 3 * es.CLASS_BLOCK
    for blk, bins in enumerate(es.BLOCKS3_BINS):
        got = collections.Counter(es.unit_class(u, m) for u, m in
                                  zip(b.units[blk * 1024:(blk + 1) * 1024], b.mis[blk * 1024:(blk + 1) * 1024]))
        assert {k for k in got if isinstance(k, int)} == set(bins), (blk, got)
        assert got["mid"] >= 5
    empty = [set(range(4)) - set(bins) for bins in es.BLOCKS3_BINS]
    assert all(empty) and set().union(*empty) == set(range(4))
    # the list is not in batch order: a later block's bin 0 follows an earlier block's bin 3
    order = es.small_list(b)
    assert order != sorted(order) and sorted(order) == [i for i in range(3072) if es.unit_class(b.units[i]) != "mid"]


# ---- statuses, layout, sizes ----------------------------------------------------------------

def test_statuses():
    union = set()
    for name in es.BUILDERS:
        got = es.statuses(batch(name))
        assert got == es.STATUSES[name], name
        union |= got
    mixed = set()
    for k in es.MIXED:
        got = es.statuses(es.mixed_batch(k))
        assert oracle.OK in got and got <= es.STATUSES["mixed"], k
        mixed |= got
    assert mixed == es.STATUSES["mixed"]
    assert es.statuses(es.mixed_batch("minority")) == es.STATUSES["mixed"]
    assert es.statuses(es.mixed_batch("blocks3")) == {oracle.OK, oracle.OUT_OF_SPACE}
    assert union == {oracle.OK, oracle.OUT_OF_SPACE, oracle.INVALID_MESSAGE_SIZE, oracle.INVALID_ARGUMENT}


@pytest.mark.parametrize("name", ALL)
def test_layout_and_sizes(name):
    b = batch(name)
    n = len(b.units)
    assert n <= 130_000 and b.in_end + es.IN_PAD <= 64 << 20 and es.output_bytes(b) <= 96 << 20
    assert int(b.in_off[0]) >= es.IN_PAD
    lens = np.array([len(u) for u in b.units], dtype=np.int64)
    caps = np.array(b.caps, dtype=np.int64)
    mis = np.array(b.mis, dtype=np.int64)
    assert (b.in_off[1:] >= b.in_off[:-1] + lens[:-1]).all() and int(b.in_off[-1] + lens[-1]) == b.in_end
    assert (((b.in_off - mis) & 7) == 0).all() and ((mis >= 0) & (mis < 8)).all() and (caps >= 0).all()
    assert int(b.out_off[0]) >= es.FRONT
    assert (b.out_off[1:] >= b.out_off[:-1] + caps[:-1] + es.BACK + es.FRONT).all()
    assert es.output_bytes(b) >= int(b.out_off[-1] + caps[-1]) + es.BACK
    buf = es.input_buffer(b)
    assert buf.size == b.in_end + es.IN_PAD
    for i in range(0, n, max(1, n // 200)):
        o = int(b.in_off[i])
        assert buf[o:o + len(b.units[i])].tobytes() == b.units[i]


def test_slot_phases():
    for name in ("small_lattice", "run_edges", "tile_edges", "class_edges"):
        b = batch(name)
        assert {int(o) & 15 for o in b.out_off} == set(range(16)), name
        assert {int(o) & 15 for o, m in zip(b.in_off, b.mis) if not m} == {0, 8}, name
    assert {int(o) & 15 for o in es.cap_cuts().out_off} == set(es.CUT_PHASES)


def test_check_judges():
    """check() on the oracle's own output passes, and a byte in [out_len, cap), a byte past cap,
    a wrong length and an unwritten status each fail it."""
    b = es.mixed_batch(257)
    want = [es.outcome(e, c) for e, c in zip(b.exp, b.caps)]
    out = np.full(es.output_bytes(b), es.SENT, dtype=np.uint8)
    for i, (st, ln) in enumerate(want):
        o = int(b.out_off[i])
        if st == oracle.OK:
            out[o:o + ln] = np.frombuffer(b.exp[i].ref, dtype=np.uint8)
        elif st == oracle.OUT_OF_SPACE:
            out[o:o + b.caps[i]] = 0x11  # unspecified
    st = np.array([w[0] for w in want], dtype=np.int32)
    ln = np.array([w[1] for w in want], dtype=np.int64)
    assert es.check(b, out, ln, st) == es.statuses(b)
    sizes = np.array([e.need if e.st == oracle.OK else 0 for e in b.exp], dtype=np.int64)
    size_st = np.array([e.st for e in b.exp], dtype=np.int32)
    assert es.check(b, None, sizes, size_st) == {int(e.st) for e in b.exp}
    i = next(i for i, (s, n_) in enumerate(want) if s == oracle.OK and n_ < b.caps[i])
    j = next(i for i, (s, _) in enumerate(want) if s == oracle.OUT_OF_SPACE)
    for at in (int(b.out_off[i]) + want[i][1], int(b.out_off[i]) + b.caps[i], int(b.out_off[j]) - 1,
               int(b.out_off[j]) + b.caps[j], int(b.out_off[i])):
        bad = out.copy()
        bad[at] ^= 0xFF
        with pytest.raises(AssertionError):
            es.check(b, bad, ln, st)
    for k in (0, 1):
        bad = [ln.copy(), st.copy()]
        bad[k][i] = -1
        with pytest.raises(AssertionError):
            es.check(b, out, *bad)
